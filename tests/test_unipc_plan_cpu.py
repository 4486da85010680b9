"""uni_pc.unipc_plan (host, float64): its folded records against the paper's loop on arrays (tests/_unipc_util.py), against
solver_plan where UniPC without its corrector IS DPM-Solver++ 2M, and against the exact solution of the probability-flow ODE of
Gaussian data, where the order the corrector adds has to show.  Also the structure of the records and the host's refusals."""
import numpy as np
import pytest

import _unipc_util as U
from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import solver_plan
from minddiffusion_amd.ldm.models.diffusion.uni_pc import unipc_plan

T_0, T_T = 1e-3, 1.


@pytest.fixture(scope="module")
def ns():
    return U.sd_schedule()


@pytest.fixture(scope="module")
def gm(ns):
    return U.GaussianData(ns)


def plan_result(ns, gm, steps, **kw):
    return U.run_unipc_plan(unipc_plan(ns, steps, t_start=T_T, t_end=T_0, **kw), gm.value, gm.x_T)


@pytest.mark.parametrize("lower_order_final", [True, False])
@pytest.mark.parametrize("skip_type", ["time_uniform", "logSNR", "karras"])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("variant", ["bh1", "bh2"])
@pytest.mark.parametrize("predict_x0", [True, False])
def test_the_plan_is_the_papers_loop(ns, gm, predict_x0, variant, order, skip_type, lower_order_final):
    for steps in sorted({order, 5, 8}):
        kw = dict(order=order, variant=variant, predict_x0=predict_x0, lower_order_final=lower_order_final)
        got = plan_result(ns, gm, steps, skip_type=skip_type, **kw)
        ref = U.unipc_loop(ns, gm.value, gm.x_T, U.grid(ns, skip_type, steps, T_T, T_0), **kw)
        err = U.rel_l2(got, ref)
        assert err <= 1e-9, (steps, err)
        off = U.unipc_loop(ns, gm.value, gm.x_T, U.grid(ns, skip_type, steps, T_T, T_0), corrector=False, **kw)
        assert U.rel_l2(plan_result(ns, gm, steps, skip_type=skip_type, corrector=False, **kw), off) <= 1e-9
        if steps > 1:
            assert U.rel_l2(off, ref) > 1e-6        # the corrector is not a no-op in the restatement


@pytest.mark.parametrize("predict_x0", [True, False])
@pytest.mark.parametrize("order", [1, 2])
def test_without_the_corrector_bh2_is_dpm_solver_2m(ns, predict_x0, order):
    """UniP-1 is the first-order update and UniP-2 with B = expm1(hh) is the multistep second-order one."""
    kw = dict(order=order, predict_x0=predict_x0, t_start=T_T, t_end=T_0)
    uni = unipc_plan(ns, 7, variant="bh2", corrector=False, **kw)
    dpm = solver_plan(ns, 7, **kw)
    assert len(uni) == len(dpm) == 7
    worst = 0.
    for u, d in zip(uni, dpm):
        assert "Ac" not in u and u["order"] == d["order"] and u["t_input"] == d["t_input"] and u["value"] == d["value"]
        for a, b in zip(("Ap", "e0", "e1", "e2"), ("A", "c0", "c1", "c2")):
            worst = max(worst, abs(u[a] - d[b]))
            assert abs(u[a] - d[b]) <= 1e-12, (a, u[a], d[b])
    print(f"order {order} predict_x0 {predict_x0}: largest coefficient difference {worst:.3e}")


def test_order_3_is_ten_times_closer_to_the_exact_solution_than_2m(ns, gm):
    """A condition on the solver: the restatement alone gives 4.96e-5 / 7.3e-5 (16 / 20 evaluations) against 5.5e-3 / 3.7e-3
    of the DPM-Solver++ 2M plan."""
    exact = gm.exact(T_T, T_0)
    for steps in (16, 20):
        uni = U.rel_l2(plan_result(ns, gm, steps, order=3, variant="bh2", skip_type="logSNR"), exact)
        ref = U.rel_l2(U.unipc_loop(ns, gm.value, gm.x_T, U.grid(ns, "logSNR", steps, T_T, T_0), 3, "bh2", True), exact)
        dpm = U.rel_l2(U.run_solver_plan(solver_plan(ns, steps, skip_type="logSNR", t_start=T_T, t_end=T_0), gm.value, gm.x_T),
                       exact)
        print(f"{steps} evaluations: UniPC-3 bh2 plan {uni:.3e}, restatement {ref:.3e}, DPM-Solver++ 2M {dpm:.3e}")
        assert uni <= 0.1 * dpm and ref <= 0.1 * dpm


def test_the_corrector_pays_at_order_2(ns, gm):
    exact = gm.exact(T_T, T_0)
    on = U.rel_l2(plan_result(ns, gm, 20, order=2, variant="bh2", skip_type="logSNR"), exact)
    off = U.rel_l2(plan_result(ns, gm, 20, order=2, variant="bh2", skip_type="logSNR", corrector=False), exact)
    print(f"order 2 bh2, 20 evaluations: corrector on {on:.3e}, off {off:.3e}, ratio {on / off:.3f}")
    assert on <= 0.6 * off


def test_record_structure(ns):
    plan = unipc_plan(ns, 8, order=3)
    assert len(plan) == 8 and "Ac" not in plan[0] and all("Ac" in r for r in plan[1:])
    assert [r["corr_order"] for r in plan] == [0, 1, 2, 3, 3, 3, 3, 2]
    assert [r["order"] for r in plan] == [1, 2, 3, 3, 3, 3, 2, 1]
    assert [r["order"] for r in unipc_plan(ns, 8, order=3, lower_order_final=False)] == [1, 2, 3, 3, 3, 3, 3, 3]
    assert [r["order"] for r in unipc_plan(ns, 20, order=3)][-3:] == [3, 2, 1]      # for every N, not only under 15 steps
    for i, r in enumerate(plan):
        assert (r["base"], r["model"], r["corr_out"], r["out"]) == ("c", "x", "c", "x")
        assert r["value"] == "x0" and r["t_input"] == float(ns.model_input_time(r["t"]))
        # a history is named exactly where one of the two forms has a coefficient for it, and it is an earlier record's store
        d = [r.get(k, 0.) for k in ("d1", "d2", "d3")]
        e = [r["e1"], r["e2"], 0.]
        for j, k in enumerate(("h1", "h2", "h3")):
            assert (r[k] is not None) == (d[j] != 0. or e[j] != 0.)
            if r[k] is not None:
                assert r[k] == plan[i - 1 - j]["store"]
        assert r["store"] not in (r["h1"], r["h2"], r["h3"])
    assert plan[3]["d3"] != 0. and plan[3]["h3"] == plan[0]["store"]       # the corrector of order 3 reads three histories
    assert plan[-1]["e1"] == plan[-1]["e2"] == 0.                          # the last update: first order, predictor only
    assert plan[0]["t"] == 1. and abs(plan[-1]["t_next"] - 1e-3) < 1e-15
    # consistency: a constant model value c and x = alpha c + sigma e ... the data-prediction forms keep alpha_t: Ac alpha_s + sum(d) = alpha_t
    for r_prev, r in zip(plan, plan[1:]):
        a_s, a_t = r_prev["alpha_m"], r["alpha_m"]
        assert abs(r["Ac"] * a_s + r["d0"] + r["d1"] + r["d2"] + r["d3"] - a_t) < 1e-12
        assert abs(r_prev["Ap"] * a_s + r_prev["e0"] + r_prev["e1"] + r_prev["e2"] - a_t) < 1e-12
    off = unipc_plan(ns, 8, order=3, corrector=False)
    assert all("Ac" not in r for r in off)
    assert [(r["Ap"], r["e0"], r["e1"], r["e2"]) for r in off] == [(r["Ap"], r["e0"], r["e1"], r["e2"]) for r in plan]
    dz = unipc_plan(ns, 5, order=2, predict_x0=False, denoise_to_zero=True)
    assert len(dz) == 6 and all(r["value"] == "eps" for r in dz[:5])
    last = dz[-1]
    assert "Ac" not in last and (last["Ap"], last["e0"], last["e1"], last["e2"]) == (0., 1., 0., 0.) and last["value"] == "x0"
    assert last["t"] == 1e-3 and last["h1"] is None and last["store"] not in (dz[-2]["store"],)
    ts = unipc_plan(ns, 6, t_start=0.6)
    assert ts[0]["t"] == 0.6 and ts[0]["t_input"] == float(ns.model_input_time(0.6)) and len(ts) == 6
    assert unipc_plan(ns, 6, t_end=0.01)[-1]["t_next"] == 0.01
    karras = unipc_plan(ns, 6, skip_type="karras", rho=5.)
    assert [r["t"] for r in karras] != [r["t"] for r in unipc_plan(ns, 6, skip_type="karras", rho=7.)]


def test_plan_refusals(ns):
    for kw, match in ((dict(method="singlestep"), "only method 'multistep'"), (dict(method="adaptive"), "only method 'multistep'"),
                      (dict(order=0), "order must be 1, 2 or 3"), (dict(order=4), "order must be 1, 2 or 3"),
                      (dict(order=True), "order must be 1, 2 or 3"), (dict(variant="vary_coeff"), "variant must be 'bh1' or 'bh2'"),
                      (dict(variant="bh3"), "variant must be"), (dict(skip_type="cosine"), "Unsupported skip_type"),
                      (dict(skip_type="karras", rho=0.), "rho must be"), (dict(t_start=0.5, t_end=0.6), "t_end < t_start"),
                      (dict(t_start=1.5), "t_end < t_start")):
        with pytest.raises(ValueError, match=match):
            unipc_plan(ns, 8, **kw)
    for steps, order in ((2, 3), (1, 2), (0, 1), (2.0, 2), (True, 1)):
        with pytest.raises(ValueError, match="steps must be an int >= order"):
            unipc_plan(ns, steps, order=order)


class _HostModel:
    """What a sampler reads of a model before any device work."""
    alphas_cumprod = np.cumprod(1. - np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2)
    parameterization = "eps"


def test_sampler_refusals_precede_any_device_work():
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.uni_pc import UniPC, UniPCSampler
    sampler = UniPCSampler(_HostModel())
    assert (sampler.solver["order"], sampler.solver["variant"], sampler.solver["skip_type"]) == (3, "bh2", "time_uniform")
    c = object()
    call = lambda **kw: sampler.sample(**{**dict(S=8, batch_size=2, shape=(4, 8, 8), conditioning=c), **kw})
    for kw, match in ((dict(mask=c), "mask / x0 blending"), (dict(x0=c), "mask / x0 blending"),
                      (dict(image_guidance_scale=1.5), "three-branch guidance"), (dict(sde_eta=1.), "sde_eta: UniPC is an ODE solver"),
                      (dict(S=[8, 6]), "per-request"), (dict(unconditional_guidance_scale=[7.5, 3.]), "per-request"),
                      (dict(guidance_rescale=[0.5, 0.]), "per-request")):
        with pytest.raises(MdxError, match=match):
            call(**kw)
    for kw, match in ((dict(method="singlestep"), "only method 'multistep'"), (dict(order=4), "order must be"),
                      (dict(variant="vary_coeff"), "variant must be"), (dict(S=2), "steps must be an int >= order"),
                      (dict(guidance_rescale=1.5), "guidance_rescale"), (dict(t_start=2.), "t_start must be"),
                      (dict(thresholding=True, max_val=0.), "max_val")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    with pytest.raises(ValueError, match="variant must be"):
        UniPCSampler(_HostModel(), variant="vary_coeff")
    with pytest.raises(ValueError, match="unknown option"):
        UniPCSampler(_HostModel(), solver_type="taylor")
    solver = UniPC(lambda x, t: x, U.sd_schedule())
    with pytest.raises(MdxError, match="sde_eta"):
        solver.sample(None, sde_eta=0.5)
    with pytest.raises(MdxError, match="three-branch guidance"):
        solver.sample(None, image_guidance_scale=1.5)
    with pytest.raises(ValueError, match="only method 'multistep'"):
        solver.sample(None, method="singlestep")
    with pytest.raises(ValueError, match="steps must be an int >= order"):
        solver.sample(None, steps=2, order=3)
