"""solver_plan (ldm/models/diffusion/dpm_solver/dpm_solver.py): the whole DPM-Solver -- orders 1-3, multistep / singlestep /
singlestep_fixed, the three grids, both solver types and both prediction forms -- as one record per model evaluation, each
followed by one launch of  x_out = A x_base + c0 m_cur + c1 h1 + c2 h2.

The records are run here in float64 numpy by a small interpreter (run_plan) on a problem with a closed form: data N(0, 0.8^2),
so eps(x, t) = sigma_t x / (alpha_t^2 0.64 + sigma_t^2) and the exact flow is x_t = x_T sqrt(alpha_t^2 0.64 + sigma_t^2) /
sqrt(alpha_T^2 0.64 + sigma_T^2).  The conditions on the error ratios are the orders of the methods (2, 4, 8 per halving of
the step for orders 1, 2, 3) with the slack the pre-asymptotic range of 20 .. 80 steps needs."""
import numpy as np
import pytest

from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import (NoiseScheduleVP, get_time_steps, multistep_2m_plan,
                                                                          singlestep_orders, solver_plan)

BETAS = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2
VAR = 0.64
X_T = 1.3


@pytest.fixture(scope="module")
def ns():
    return NoiseScheduleVP("discrete", betas=BETAS)


def eps_exact(ns, x, t):
    a, s = ns.marginal_alpha(t), ns.marginal_std(t)
    return s * x / (a * a * VAR + s * s)


def flow_exact(ns, t_from, t_to, x):
    scale = lambda t: np.sqrt(ns.marginal_alpha(t) ** 2 * VAR + ns.marginal_std(t) ** 2)
    return x * scale(t_to) / scale(t_from)


def run_plan(ns, plan, x, eps_fn=eps_exact):
    """The records as the sampler runs them: buffers by role, one model evaluation and one linear form per record."""
    buf = {"x": float(x), "y": None, "m0": None, "m1": None, "m2": None}
    for r in plan:
        xm = buf[r["model"]]
        e = eps_fn(ns, xm, r["t"])
        m = (xm - r["sigma_m"] * e) / r["alpha_m"] if r["value"] == "x0" else e
        out = r["c0"] * m
        if r["A"] != 0.:
            out += r["A"] * buf[r["base"]]
        for c, h in ((r["c1"], r["h1"]), (r["c2"], r["h2"])):
            assert (c != 0.) == (h is not None), r
            if h is not None:
                assert h != r["store"] and buf[h] is not None, r
                out += c * buf[h]
        buf[r["store"]] = m
        buf[r["out"]] = out
    return buf["x"]


def error(ns, steps, **kw):
    plan = solver_plan(ns, steps, skip_type="logSNR", **kw)
    return abs(run_plan(ns, plan, X_T) - flow_exact(ns, 1.0, 1e-3, X_T))


# ------------------------------------------------------------------------------------------------ the wired configuration
@pytest.mark.parametrize("steps", [2, 5, 14, 15, 20, 50])
@pytest.mark.parametrize("t_start", [None, 0.6])
def test_wired_configuration_is_the_2m_plan(ns, steps, t_start):
    old = multistep_2m_plan(ns, steps, order=2, lower_order_final=True, t_start=t_start)
    new = solver_plan(ns, steps, t_start=t_start)
    assert len(new) == len(old) == steps
    for o, n in zip(old, new):
        for key in ("A", "c0", "c1", "t_input"):
            assert n[key] == pytest.approx(o[key], rel=1e-13, abs=0.), (key, o, n)
        assert n["alpha_m"] == pytest.approx(o["alpha"], rel=1e-13) and n["sigma_m"] == pytest.approx(o["sigma"], rel=1e-13)
        assert n["order"] == o["order"] and n["c2"] == 0. and n["value"] == "x0"
        assert (n["base"], n["model"], n["out"]) == ("x", "x", "x")


def test_order_one_of_the_wired_plan(ns):
    old = multistep_2m_plan(ns, 1, order=1)
    new = solver_plan(ns, 1, order=1)
    assert len(new) == 1 and new[0]["A"] == pytest.approx(old[0]["A"], rel=1e-13)
    assert new[0]["c0"] == pytest.approx(old[0]["c0"], rel=1e-13) and new[0]["c1"] == 0.


# ------------------------------------------------------------------------------------------------ evaluation counts
@pytest.mark.parametrize("method,order,steps", [("multistep", 1, 7), ("multistep", 2, 7), ("multistep", 3, 7),
                                                ("multistep", 3, 20), ("singlestep", 1, 5), ("singlestep", 2, 6),
                                                ("singlestep", 2, 7), ("singlestep", 3, 6), ("singlestep", 3, 7),
                                                ("singlestep", 3, 8), ("singlestep", 3, 2), ("singlestep_fixed", 2, 8),
                                                ("singlestep_fixed", 3, 9), ("singlestep_fixed", 1, 4)])
@pytest.mark.parametrize("skip_type", ["logSNR", "time_uniform", "time_quadratic"])
@pytest.mark.parametrize("denoise", [False, True])
def test_one_record_per_evaluation(ns, method, order, steps, skip_type, denoise):
    plan = solver_plan(ns, steps, order=order, method=method, skip_type=skip_type, denoise_to_zero=denoise)
    assert len(plan) == steps + int(denoise)
    times = [r["t"] for r in plan]
    assert times[0] == 1.0 and all(a > b for a, b in zip(times, times[1:]))
    assert all(r["t_input"] == pytest.approx((r["t"] - 1e-3) * 1000., abs=1e-9) for r in plan)
    last = plan[-1]
    if denoise:
        assert (last["t"], last["A"], last["c0"], last["c1"], last["c2"], last["value"]) == (1e-3, 0., 1., 0., 0., "x0")
        last = plan[-2]
    assert last["t_next"] == 1e-3 and last["out"] == "x"
    assert np.isfinite(run_plan(ns, plan, X_T))


@pytest.mark.parametrize("steps,order,orders", [(6, 3, [3, 2, 1]), (7, 3, [3, 3, 1]), (8, 3, [3, 3, 2]), (7, 2, [2, 2, 2, 1]),
                                                (6, 2, [2, 2, 2]), (4, 1, [1, 1, 1, 1])])
def test_dpm_solver_fast_order_lists(ns, steps, order, orders):
    assert singlestep_orders(steps, order)[0] == orders
    plan = solver_plan(ns, steps, order=order, method="singlestep", skip_type="logSNR")
    assert [r["order"] for r in plan] == [o for o in orders for _ in range(o)]
    # the logSNR outer grid has K points after the start: the updates end on a uniform lambda grid of K intervals
    ends = [r["t_next"] for r in plan if r["out"] == "x"]
    lam = ns.marginal_lambda(np.array([1.0] + ends))
    assert np.allclose(np.diff(lam), (lam[-1] - lam[0]) / len(orders), rtol=1e-9)


def test_multistep_orders(ns):
    assert [r["order"] for r in solver_plan(ns, 6, order=3)] == [1, 2, 3, 3, 2, 1]
    assert [r["order"] for r in solver_plan(ns, 6, order=3, lower_order_final=False)] == [1, 2, 3, 3, 3, 3]
    assert [r["order"] for r in solver_plan(ns, 16, order=3)] == [1, 2] + [3] * 14
    third = solver_plan(ns, 16, order=3)[5]
    assert third["h1"] is not None and third["h2"] is not None and len({third["h1"], third["h2"], third["store"]}) == 3


# ------------------------------------------------------------------------------------------------ grids
@pytest.mark.parametrize("skip_type", ["logSNR", "time_uniform", "time_quadratic"])
@pytest.mark.parametrize("ends", [(1.0, 1e-3), (0.6, 1e-3), (1.0, 0.05)])
def test_grids(ns, skip_type, ends):
    ts = get_time_steps(ns, skip_type, ends[0], ends[1], 13)
    assert ts.dtype == np.float64 and ts.shape == (14,)
    assert ts[0] == ends[0] and ts[-1] == ends[1] and np.all(np.diff(ts) < 0)
    if skip_type == "logSNR":
        assert np.allclose(np.diff(ns.marginal_lambda(ts)), np.diff(ns.marginal_lambda(ts))[0], rtol=1e-6)
    if skip_type == "time_quadratic":
        assert np.allclose(np.diff(np.sqrt(ts)), np.diff(np.sqrt(ts))[0], rtol=1e-9)


def test_t_start_and_t_end_bound_the_plan(ns):
    plan = solver_plan(ns, 9, order=3, method="singlestep", skip_type="time_uniform", t_start=0.7, t_end=0.02)
    assert plan[0]["t"] == 0.7 and plan[-1]["t_next"] == 0.02


# ------------------------------------------------------------------------------------------------ convergence
def test_order_one_converges_at_first_order(ns):
    for method in ("multistep", "singlestep", "singlestep_fixed"):
        e = [error(ns, n, order=1, method=method) for n in (20, 40, 80)]
        for r in (e[0] / e[1], e[1] / e[2]):
            assert 1.8 <= r <= 2.2, (method, e)


@pytest.mark.parametrize("method", ["multistep", "singlestep_fixed"])
def test_order_two_converges_at_second_order(ns, method):
    # singlestep_fixed: 20 / 40 / 80 OUTER steps
    per = 2 if method == "singlestep_fixed" else 1
    e = [error(ns, n * per, order=2, method=method) for n in (20, 40, 80)]
    assert e[0] / e[1] >= 3.5 and e[1] / e[2] >= 3.5, e


def test_singlestep_fixed_order_three_converges_at_third_order(ns):
    e = [error(ns, 3 * n, order=3, method="singlestep_fixed") for n in (20, 40, 80)]
    assert e[0] / e[1] >= 6. and e[1] / e[2] >= 6., e


def test_multistep_order_three_beats_order_two(ns):
    """Its lower-order start holds the ratio near 4, so the condition is the error itself: below order 2's at 10 / 20 / 40 / 80
    steps, 1.4e-2 < 2.0e-2 ... 1.25e-4 < 3.8e-4.  Those figures are the runs WITHOUT lower_order_final, which only acts under
    15 steps: with it the 10-step run ends third order's advantage two updates early (order 3, 2, 1 at the end) and the
    reference's formulas give 2.7e-2 against order 2's 1.7e-2 -- so the flag is off here at every count, the flag's own
    effect is pinned by the last two assertions."""
    e3 = {n: error(ns, n, order=3, method="multistep", lower_order_final=False) for n in (10, 20, 40, 80)}
    e2 = {n: error(ns, n, order=2, method="multistep", lower_order_final=False) for n in (10, 20, 40, 80)}
    for n in (10, 20, 40, 80):
        assert e3[n] < e2[n], (n, e3, e2)
    assert e3[10] == pytest.approx(1.4e-2, rel=0.05) and e2[10] == pytest.approx(2.0e-2, rel=0.05)
    assert e3[80] == pytest.approx(1.25e-4, rel=0.05) and e2[80] == pytest.approx(3.8e-4, rel=0.05)
    for n in (20, 40, 80):      # from 15 steps on the flag changes nothing
        assert error(ns, n, order=3, method="multistep") == e3[n]
    assert error(ns, 10, order=3, method="multistep") == pytest.approx(2.7e-2, rel=0.05)


@pytest.mark.parametrize("kw", [dict(order=2, method="multistep", solver_type="taylor"),
                                dict(order=3, method="multistep", solver_type="taylor"),
                                dict(order=2, method="singlestep_fixed", solver_type="taylor"),
                                dict(order=3, method="singlestep_fixed", solver_type="taylor"),
                                dict(order=3, method="singlestep", solver_type="taylor"),
                                dict(order=1, method="multistep", predict_x0=False),
                                dict(order=2, method="multistep", predict_x0=False),
                                dict(order=3, method="multistep", predict_x0=False),
                                dict(order=2, method="singlestep_fixed", predict_x0=False),
                                dict(order=3, method="singlestep_fixed", predict_x0=False),
                                dict(order=3, method="singlestep", predict_x0=False),
                                dict(order=2, method="multistep", predict_x0=False, solver_type="taylor"),
                                dict(order=2, method="singlestep_fixed", predict_x0=False, solver_type="taylor"),
                                dict(order=3, method="singlestep_fixed", predict_x0=False, solver_type="taylor")],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_variants_reach_the_exact_value(ns, kw):
    steps = 80 if kw["method"] != "singlestep_fixed" else 80 * kw["order"]
    exact = flow_exact(ns, 1.0, 1e-3, X_T)
    got = run_plan(ns, solver_plan(ns, steps, skip_type="logSNR", **kw), X_T)
    assert abs(got - exact) <= 0.05 * abs(exact), (got, exact)
    if kw["order"] >= 2:        # and as a high-order method does, far inside the 5 %
        assert abs(got - exact) <= 1e-3 * abs(exact), (got, exact)
    assert all(r["value"] == ("eps" if kw.get("predict_x0") is False else "x0") for r in
               solver_plan(ns, steps, skip_type="logSNR", **kw))


def test_noise_form_carries_x_by_alpha(ns):
    for r in solver_plan(ns, 9, order=3, method="singlestep", predict_x0=False):
        if r["base"] == r["model"] == "x":
            a_s, a_t = ns.marginal_alpha(r["t"]), ns.marginal_alpha(r["t_next"])
            assert r["A"] == pytest.approx(float(a_t / a_s), rel=1e-12)


def test_denoise_to_zero_returns_the_data_prediction(ns):
    plan = solver_plan(ns, 10, denoise_to_zero=True, predict_x0=False)
    x = run_plan(ns, plan[:-1], X_T)
    r = plan[-1]
    x0 = (x - r["sigma_m"] * eps_exact(ns, x, r["t"])) / r["alpha_m"]
    assert run_plan(ns, plan, X_T) == x0 and r["value"] == "x0"


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ns):
    with pytest.raises(NotImplementedError, match="device-to-host error norm"):
        solver_plan(ns, 10, method="adaptive")
    with pytest.raises(ValueError, match="Got wrong method euler"):
        solver_plan(ns, 10, method="euler")
    for order in (0, 4, 2.5, True):
        with pytest.raises(ValueError, match="Solver order must be 1 or 2 or 3"):
            solver_plan(ns, 10, order=order)
    with pytest.raises(ValueError, match="'solver_type' must be either 'dpm_solver' or 'taylor', got midpoint"):
        solver_plan(ns, 10, solver_type="midpoint")
    with pytest.raises(ValueError, match="Unsupported skip_type cosine, need to be 'logSNR' or 'time_uniform' or "
                                         "'time_quadratic'"):
        solver_plan(ns, 10, skip_type="cosine")
    with pytest.raises(ValueError, match="Unsupported skip_type"):
        get_time_steps(ns, "cosine", 1.0, 1e-3, 4)
    with pytest.raises(ValueError, match="'order' must be '1' or '2' or '3'"):
        singlestep_orders(6, 4)
    for kw in (dict(steps=2, order=3), dict(steps=1, order=2, method="singlestep_fixed"), dict(steps=0, method="singlestep"),
               dict(steps=2.0), dict(steps=True, order=1)):
        with pytest.raises(ValueError, match="steps must be an int >="):
            solver_plan(ns, kw.pop("steps"), **kw)
    for kw in (dict(t_start=1e-3), dict(t_end=1.0), dict(t_start=1.5), dict(t_end=0.)):
        with pytest.raises(ValueError, match="need 0 < t_end < t_start"):
            solver_plan(ns, 5, **kw)
