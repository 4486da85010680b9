"""The host math of the two options the reference's DPM-Solver does not have (dpm_solver/dpm_solver.py): the Karras sigma grid
(skip_type="karras", rho) and the SDE form of the multistep update (solver_plan(..., sde_eta=, s_noise=): "DPM++ 2M SDE").

The yardstick is restated here.  Grid: sigma(t) = exp(-lambda(t)), the N + 1 points uniform in sigma^(1 / rho).  SDE update from
s to t, h = lambda_t - lambda_s, eta = sde_eta:
    A = (sigma_t / sigma_s) e^{-eta h},  phi = expm1(-(1 + eta) h),  cn = s_noise sigma_t sqrt(-expm1(-2 eta h))
    order 1: c0 = -alpha_t phi;   order 2: c0 = -alpha_t phi (1 + 1 / (2 r0)), c1 = alpha_t phi / (2 r0)
Two identities hold whatever eta is -- a constant data prediction is carried exactly (A alpha_s + c0 + c1 = alpha_t) and, with
s_noise = 1, the marginal variance is kept (A^2 sigma_s^2 + cn^2 = sigma_t^2) -- both checked to 1e-12."""
import numpy as np
import pytest

from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP, get_time_steps, solver_plan

BETAS = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2
GRIDS = ("logSNR", "time_uniform", "time_quadratic", "karras")
ETAS = (0.5, 1.0, 1.7)


@pytest.fixture(scope="module")
def ns():
    return NoiseScheduleVP("discrete", betas=BETAS)


# ------------------------------------------------------------------------------------------------ the Karras grid
@pytest.mark.parametrize("rho", [7.0, 3.0, 1.0])
@pytest.mark.parametrize("N,t_T,t_0", [(20, 1.0, 1e-3), (1, 1.0, 1e-3), (9, 0.6, 0.05)])
def test_karras_grid(ns, rho, N, t_T, t_0):
    ts = get_time_steps(ns, "karras", t_T, t_0, N, rho)
    assert ts.shape == (N + 1,) and ts[0] == t_T and ts[-1] == t_0            # the ends exactly
    assert np.all(np.diff(ts) < 0)
    s_T, s_0 = np.exp(-ns.marginal_lambda(t_T)), np.exp(-ns.marginal_lambda(t_0))
    sig = (s_T ** (1 / rho) + (np.arange(N + 1) / N) * (s_0 ** (1 / rho) - s_T ** (1 / rho))) ** rho
    closed = ns.inverse_lambda(-np.log(sig))
    assert np.max(np.abs(ts - closed)) <= 1e-12
    # the grid's own sigmas are the closed form's (the round trip through the interpolated schedule)
    assert np.allclose(np.exp(-ns.marginal_lambda(ts)), sig, rtol=1e-9, atol=0)


def test_karras_ends_on_the_sd_schedule(ns):
    """k-diffusion's well-known sigma_max / sigma_min of this schedule."""
    sig = np.exp(-ns.marginal_lambda(get_time_steps(ns, "karras", 1.0, 1e-3, 20)))
    assert abs(sig[0] - 14.6146) < 1e-4 and abs(sig[-1] - 0.029167) < 1e-6


def test_karras_reaches_every_method(ns):
    """singlestep's inner grids included: r1 of an order-2 step comes from a 2-interval Karras grid of the step's ends."""
    for method, order, steps in (("multistep", 3, 9), ("singlestep", 3, 9), ("singlestep", 2, 7), ("singlestep_fixed", 2, 8)):
        plan = solver_plan(ns, steps, order=order, skip_type="karras", method=method)
        other = solver_plan(ns, steps, order=order, skip_type="logSNR", method=method)
        assert len(plan) == len(other) and plan[0]["t"] == 1.0 and plan[-1]["t_next"] == 1e-3
        assert [r["t"] for r in plan] != [r["t"] for r in other]
        assert all(r["t"] > r["t_next"] for r in plan)
    steps7 = solver_plan(ns, 6, skip_type="karras", rho=7.)
    steps3 = solver_plan(ns, 6, skip_type="karras", rho=3.)
    assert [r["t"] for r in steps7] != [r["t"] for r in steps3]
    inner = get_time_steps(ns, "karras", 0.8, 0.4, 2)
    fixed = solver_plan(ns, 2, order=2, skip_type="karras", method="singlestep_fixed", t_start=0.8, t_end=0.4)
    assert abs(fixed[1]["t"] - inner[1]) < 1e-9


def test_rho_is_refused(ns):
    for bad in (0., -7., float("inf"), float("nan")):
        with pytest.raises(ValueError, match="rho"):
            get_time_steps(ns, "karras", 1.0, 1e-3, 5, bad)
        with pytest.raises(ValueError, match="rho"):
            solver_plan(ns, 5, skip_type="karras", rho=bad)
    # rho counts with the Karras grid only
    assert solver_plan(ns, 5, rho=-1.) == solver_plan(ns, 5)


# ------------------------------------------------------------------------------------------------ sde_eta == 0
def deterministic_plan(ns, steps, order, skip_type):
    """Today's records, restated from the deterministic midpoint formulas: (A, c0, c1) of every update."""
    ts = get_time_steps(ns, skip_type, 1.0, 1e-3, steps)
    lam, alpha, sigma = ns.marginal_lambda(ts), ns.marginal_alpha(ts), ns.marginal_std(ts)
    rows = []
    for k in range(steps):
        step = k + 1
        o = step if step < order else (min(order, steps + 1 - step) if steps < 15 else order)
        h = lam[k + 1] - lam[k]
        phi = np.expm1(-h)
        if o == 1:
            rows.append((sigma[k + 1] / sigma[k], -alpha[k + 1] * phi, 0.))
        else:
            r0 = (lam[k] - lam[k - 1]) / h
            rows.append((sigma[k + 1] / sigma[k], -alpha[k + 1] * phi * (1 + 0.5 / r0), 0.5 * alpha[k + 1] * phi / r0))
    return rows


@pytest.mark.parametrize("skip_type", GRIDS)
@pytest.mark.parametrize("S,order", [(S, order) for S in (1, 2, 9, 20) for order in (1, 2) if S >= order])   # (a run needs S >= order)
def test_eta_zero_is_the_deterministic_plan(ns, S, order, skip_type):
    plain = solver_plan(ns, S, order=order, skip_type=skip_type)
    assert solver_plan(ns, S, order=order, skip_type=skip_type, sde_eta=0., s_noise=1.) == plain      # record for record
    assert solver_plan(ns, S, order=order, skip_type=skip_type, sde_eta=0., s_noise=3.) == plain      # s_noise is not read
    assert all(r["cn"] == 0. for r in plain) and [r["draw"] for r in plain] == list(range(S))
    for r, (A, c0, c1) in zip(plain, deterministic_plan(ns, S, order, skip_type)):
        assert abs(r["A"] - A) <= 1e-15 and abs(r["c0"] - c0) <= 1e-15 and abs(r["c1"] - c1) <= 1e-15 and r["c2"] == 0.


# ------------------------------------------------------------------------------------------------ sde_eta > 0
@pytest.mark.parametrize("skip_type", GRIDS)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("eta", ETAS)
def test_sde_records(ns, eta, order, skip_type):
    S = 20
    plan = solver_plan(ns, S, order=order, skip_type=skip_type, sde_eta=eta)
    base = solver_plan(ns, S, order=order, skip_type=skip_type)
    assert len(plan) == S and [r["draw"] for r in plan] == list(range(S))
    assert [r["order"] for r in plan] == [r["order"] for r in base] and [r["t"] for r in plan] == [r["t"] for r in base]
    worst_mean = worst_var = 0.
    for r in plan:
        a_s, s_s = r["alpha_m"], r["sigma_m"]
        a_t, s_t = float(ns.marginal_alpha(r["t_next"])), float(ns.marginal_std(r["t_next"]))
        h = float(ns.marginal_lambda(r["t_next"]) - ns.marginal_lambda(r["t"]))
        assert r["cn"] > 0. and r["c2"] == 0. and (r["c1"] != 0.) == (r["order"] == 2)
        assert abs(r["A"] - s_t / s_s * np.exp(-eta * h)) <= 1e-15 * max(1., abs(r["A"]))
        assert abs(r["cn"] - s_t * np.sqrt(-np.expm1(-2 * eta * h))) <= 1e-15
        if r["order"] == 1:
            assert abs(r["c0"] + a_t * np.expm1(-(1 + eta) * h)) <= 1e-15
        worst_mean = max(worst_mean, abs(r["A"] * a_s + r["c0"] + r["c1"] - a_t))
        worst_var = max(worst_var, abs(r["A"] ** 2 * s_s ** 2 + r["cn"] ** 2 - s_t ** 2))
    print(f"eta {eta} order {order} {skip_type}: mean identity {worst_mean:.2e}, variance identity {worst_var:.2e}")
    assert worst_mean <= 1e-12 and worst_var <= 1e-12
    # cn is linear in s_noise, nothing else reads it
    for sn in (0., 0.5, 2.0):
        scaled = solver_plan(ns, S, order=order, skip_type=skip_type, sde_eta=eta, s_noise=sn)
        for r, q in zip(plan, scaled):
            assert abs(q["cn"] - sn * r["cn"]) <= 1e-15 and {k: v for k, v in q.items() if k != "cn"} == \
                {k: v for k, v in r.items() if k != "cn"}


def test_sde_order_rules_and_denoise_to_zero(ns):
    """lower_order_final and the first-step rule are the deterministic run's; denoise_to_zero's record draws nothing."""
    plan = solver_plan(ns, 9, sde_eta=1., skip_type="karras", denoise_to_zero=True)
    assert [r["order"] for r in plan] == [1, 2, 2, 2, 2, 2, 2, 2, 1, 1]
    assert plan[-1]["cn"] == 0. and plan[-1]["A"] == 0. and plan[-1]["c0"] == 1. and plan[-1]["draw"] == 9
    assert all(r["cn"] > 0. for r in plan[:-1])               # the last update to t_0 is stochastic too
    assert [r["order"] for r in solver_plan(ns, 9, sde_eta=1., lower_order_final=False)] == [1] + [2] * 8
    started = solver_plan(ns, 4, sde_eta=0.5, t_start=0.5)
    assert started[0]["t"] == 0.5 and all(r["cn"] > 0. for r in started)


def test_sde_refusals(ns):
    for kw in (dict(method="singlestep"), dict(method="singlestep_fixed"), dict(order=3), dict(predict_x0=False),
               dict(solver_type="taylor")):
        with pytest.raises(ValueError, match="sde_eta"):
            solver_plan(ns, 9, sde_eta=0.5, **kw)
        solver_plan(ns, 9, sde_eta=0., **kw)                    # the deterministic solver still takes them
    for name in ("sde_eta", "s_noise"):
        for bad in (-0.5, float("inf"), float("-inf"), float("nan")):
            with pytest.raises(ValueError, match=name):
                solver_plan(ns, 9, **{"sde_eta": 1., name: bad})
    with pytest.raises(ValueError, match="s_noise"):
        solver_plan(ns, 9, s_noise=-1.)


# ------------------------------------------------------------------------------------------------ the surfaces (no device)
class _Model:
    alphas_cumprod = np.cumprod(1.0 - BETAS)


def test_sampler_defaults_and_wired_flag():
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver.sampler import solver_options
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver.solver import SOLVER_DEFAULTS
    assert SOLVER_DEFAULTS["sde_eta"] == 0. and SOLVER_DEFAULTS["s_noise"] == 1. and SOLVER_DEFAULTS["rho"] == 7.
    assert DPMSolverSampler(_Model()).wired
    assert DPMSolverSampler(_Model(), rho=3., s_noise=2.).wired           # neither is read at the defaults of what reads it
    k = DPMSolverSampler(_Model(), skip_type="karras", sde_eta=1.0)
    assert not k.wired and k.solver["skip_type"] == "karras" and k.solver["sde_eta"] == 1.0
    assert not DPMSolverSampler(_Model(), skip_type="karras").wired and not DPMSolverSampler(_Model(), sde_eta=0.3).wired
    opts, wired = solver_options(k.solver, dict(rho=5., s_noise=0.5))
    assert not wired and opts["rho"] == 5. and opts["s_noise"] == 0.5 and opts["sde_eta"] == 1.0
    opts, wired = solver_options(SOLVER_DEFAULTS, dict(rho=5., s_noise=0.5))
    assert wired and opts["rho"] == 7. and opts["s_noise"] == 1.
    # a mistake shows where it is made
    with pytest.raises(ValueError, match="sde_eta"):
        DPMSolverSampler(_Model(), sde_eta=1.0, order=3)
    with pytest.raises(ValueError, match="sde_eta"):
        DPMSolverSampler(_Model(), sde_eta=-1.0)
    with pytest.raises(ValueError, match="rho"):
        DPMSolverSampler(_Model(), skip_type="karras", rho=0.)
    with pytest.raises(ValueError, match="s_noise"):
        DPMSolverSampler(_Model(), sde_eta=1.0, s_noise=float("nan"))


def test_pipeline_takes_the_options_and_sessions_refuse_them():
    from minddiffusion_amd.pipeline import DiffusionPipeline
    pipe = DiffusionPipeline(_Model(), sampler="dpm_solver", device="cpu", solver=dict(skip_type="karras", sde_eta=1.0, rho=5.))
    assert not pipe.sampler.wired and pipe._solver() == dict(skip_type="karras", sde_eta=1.0, rho=5.)
    with pytest.raises(ValueError, match="session.*multistep order-2.*rho, sde_eta, skip_type"):
        pipe.session(slots=2, H=64, W=64)
    with pytest.raises(ValueError, match="session.*sde_eta"):
        DiffusionPipeline(_Model(), sampler="dpm_solver", device="cpu", solver=dict(sde_eta=0.5)).session(slots=2, H=64, W=64)
    with pytest.raises(ValueError, match="unknown option.*eta"):
        DiffusionPipeline(_Model(), sampler="dpm_solver", device="cpu", solver=dict(eta=1.0))
    assert DiffusionPipeline(_Model(), sampler="dpm_solver", device="cpu", solver=dict(s_noise=2.))._solver() is None


def test_per_request_lists_are_refused_with_the_new_options():
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    for opts, names in ((dict(sde_eta=1.0), "sde_eta"), (dict(skip_type="karras"), "skip_type")):
        with pytest.raises(ValueError, match=f"per-request.*step table.*{names}"):
            DPMSolverSampler(_Model()).sample([4, 6], 2, (4, 8, 8), conditioning=object(), **opts)
