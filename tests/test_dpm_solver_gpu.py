"""The whole DPM-Solver end to end: DPMSolverSampler's solver options on the tiny UNet of
test_unet_gpu.py::test_tiny_dpm_solver_trajectory (B 2, 8 x 8 latent, 6 context tokens) against tests/_dpm_full_util.py, a
torch-CPU restatement of the updates on the oracle UNet.

Bar: the project's own for this test family, check(..., rel_l2=1e-2, max_rel=1e-2), for every configuration.  (Should one miss it,
its bar becomes twice the oracle's own fp32 vs emulate_fp16() distance through the same restatement -- a CPU measurement on the
reference side only; never a figure taken from the kernel's output.)  None misses it: the device ends 1.4e-3 ... 2.1e-3 (rel-L2)
from the restatement, where the oracle's own fp32 and fp16-emulated runs of the same configurations end 1.4e-3 ... 2.4e-3 apart
(docs/PARITY.md has both per configuration).

Also here: one model evaluation and exactly one ops.sampler_step_lin launch per record and none of the 2M entries; the callbacks;
the pipeline's solver= defaults on txt2img, img2img and windowed(); the refusals of sessions and per-request lists."""
import numpy as np
import pytest
import torch

import _dpm_full_util as F
import _vpred_util as V
from _util import check
from oracle import ldm as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, T = 2, 8, 8, 6
SCALE = 3.0

# name -> (S, solver options)
CONFIGS = {
    "multistep3_logSNR_S12": (12, dict(order=3, skip_type="logSNR")),
    "multistep3_uniform_S16": (16, dict(order=3)),
    "singlestep3_logSNR_S8": (8, dict(order=3, skip_type="logSNR", method="singlestep")),
    "singlestep2_quadratic_S7": (7, dict(order=2, skip_type="time_quadratic", method="singlestep")),
    "singlestep_fixed3_S9": (9, dict(order=3, method="singlestep_fixed")),
    "multistep2_taylor_S10": (10, dict(solver_type="taylor")),
    "multistep2_noise_form_S10": (10, dict(predict_x0=False)),
    "multistep2_threshold_denoise_S10": (10, dict(thresholding=True, denoise_to_zero=True)),
}


@pytest.fixture(scope="module")
def tiny():
    model, cfg, params = V.tiny_eps_model()
    om = O.ModelOracle(O.UNetOracle(dict(cfg, num_heads=-1), params))
    D = cfg["context_dim"]
    x_T = np.random.RandomState(42).randn(B, 4, H, W).astype(np.float32)
    c = np.random.RandomState(1).randn(B, T, D).astype(np.float32)
    uc = np.repeat(np.random.RandomState(2).randn(1, T, D).astype(np.float32), B, 0)
    return model, om, x_T, c, uc


_REFS = {}


def reference(tiny, name):
    """(final latent, solver, options) of configuration `name` on the oracle side, computed once."""
    if name not in _REFS:
        _, om, x_T, c, uc = tiny
        S, opts = CONFIGS[name]
        opts = dict(opts)
        run = lambda **kw: F.sample(om, S, B, (4, H, W), c, x_T, unconditional_guidance_scale=SCALE,
                                    unconditional_conditioning=uc, **kw)
        if opts.get("thresholding"):
            # max_val from the oracle's run alone: the lower quartile of the thresholds of a run in which s always wins
            _, probe = run(**dict(opts, max_val=1e-6))
            opts["max_val"] = float(torch.quantile(torch.stack(probe.raw_s).min(dim=1).values, 0.25))
        ref, solver = run(**opts)
        _REFS[name] = (ref, solver, opts)
    return _REFS[name]


def sample(model, x_T, c, uc, S, opts, **kw):
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    d = lambda a: torch.tensor(a, device=DEV)
    return DPMSolverSampler(model).sample(S, B, (4, H, W), conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=SCALE,
                                          unconditional_conditioning=d(uc), verbose=False, **opts, **kw)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_configuration_against_the_restatement(tiny, monkeypatch, name):
    from minddiffusion_amd import ops
    model, _, x_T, c, uc = tiny
    S = CONFIGS[name][0]
    ref, solver, opts = reference(tiny, name)
    evals = S + int(bool(opts.get("denoise_to_zero")))
    assert solver.nfe == evals
    if opts.get("thresholding"):
        won = sum(bool((s > opts["max_val"]).all()) for s in solver.raw_s)
        print(f"{name}: max_val {opts['max_val']:.4f}, s > max_val in {won} of {len(solver.raw_s)} evaluations (oracle side)")
        assert len(solver.raw_s) == evals and 2 * won >= evals and won < evals
    count = {}
    for entry in ("sampler_step_lin", "sampler_step", "sampler_step_pred", "sampler_step_rescale", "sampler_step_table"):
        def counted(*a, _real=getattr(ops, entry), _entry=entry, **k):
            count[_entry] = count.get(_entry, 0) + 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, entry, counted)
    unet_calls = []
    real_nhwc = model.apply_model_nhwc
    monkeypatch.setattr(model, "apply_model_nhwc", lambda *a, **k: (unet_calls.append(1), real_nhwc(*a, **k))[1], raising=False)
    calls, values = [], []
    got, inter = sample(model, x_T, c, uc, S, opts, callback=lambda i: calls.append(i),
                        img_callback=lambda m, i: values.append((i, tuple(m.shape), float(m.abs().max()))))
    assert inter is None and calls == list(range(evals)) and [v[0] for v in values] == calls
    assert all(v[1] == (B, 4, H, W) and np.isfinite(v[2]) for v in values)
    if opts.get("thresholding"):
        assert all(v[2] <= 1.0 for v in values)                # a thresholded data prediction lies in [-1, 1]
    assert count == {"sampler_step_lin": evals} and len(unet_calls) == evals
    check(f"tiny_dpm_full_{name}", got, ref, rel_l2=1e-2, max_rel=1e-2)


def test_default_options_are_the_wired_run(tiny, monkeypatch):
    """Every option spelled out at its default: the launches and the bits of a call without them."""
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver.solver import SOLVER_DEFAULTS
    model, _, x_T, c, uc = tiny
    plain = sample(model, x_T, c, uc, 6, {})[0]
    count = {}
    for entry in ("sampler_step_lin", "sampler_step"):
        def counted(*a, _real=getattr(ops, entry), _entry=entry, **k):
            count[_entry] = count.get(_entry, 0) + 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, entry, counted)
    spelled = sample(model, x_T, c, uc, 6, dict(SOLVER_DEFAULTS, max_val=3.0))[0]      # (max_val is not read: no thresholding)
    assert count == {"sampler_step": 6} and torch.equal(plain, spelled)


def test_the_wired_configuration_through_the_new_entry(tiny):
    """DPM_Solver on model_wrapper's result runs the wired configuration through ops.sampler_step_lin: the same update as the
    wired launches, within the project's bar of the same oracle."""
    from oracle import dpm_solver as OD
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPM_Solver, NoiseScheduleVP, model_wrapper
    model, om, x_T, c, uc = tiny
    d = lambda a: torch.tensor(a, device=DEV)
    ns = NoiseScheduleVP("discrete", alphas_cumprod=np.asarray(model.alphas_cumprod, np.float64))
    fn = model_wrapper(model, ns, model_type="noise", guidance_type="classifier-free", condition=d(c),
                       unconditional_condition=d(uc), guidance_scale=SCALE)
    got = DPM_Solver(fn, ns, predict_x0=True).sample(d(x_T), steps=10, order=2, skip_type="time_uniform", method="multistep")
    ref, _ = OD.sample(om, 10, B, (4, H, W), c, x_T, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)
    check("tiny_dpm_full_DPM_Solver_wired", got, ref, rel_l2=1e-2, max_rel=1e-2)
    # the reference's own port target: singlestep order 3 on a logSNR grid, and a foreign (x, t_continuous) -> eps callable
    ref3, _ = F.sample(om, 12, B, (4, H, W), c, x_T, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc, order=3,
                       skip_type="logSNR", method="singlestep", predict_x0=False)
    got3 = DPM_Solver(fn, ns).sample(d(x_T), steps=12, order=3, skip_type="logSNR", method="singlestep")
    check("tiny_dpm_full_DPM_Solver_singlestep3", got3, ref3, rel_l2=1e-2, max_rel=1e-2)
    eps = fn(d(x_T), torch.tensor([0.5]))
    foreign = DPM_Solver(lambda x, t: fn(x, t), ns).sample(d(x_T), steps=12, order=3, skip_type="logSNR", method="singlestep")
    assert tuple(eps.shape) == (B, 4, H, W) and bool(torch.isfinite(eps).all())
    check("tiny_dpm_full_DPM_Solver_foreign_callable", foreign, ref3, rel_l2=1e-2, max_rel=1e-2)


def test_model_wrapper_and_solver_refusals(tiny):
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPM_Solver, NoiseScheduleVP, model_wrapper
    model = tiny[0]
    ns = NoiseScheduleVP("discrete", alphas_cumprod=np.asarray(model.alphas_cumprod, np.float64))
    for model_type in ("x_start", "score"):
        with pytest.raises(NotImplementedError, match=model_type):
            model_wrapper(model, ns, model_type=model_type)
    with pytest.raises(NotImplementedError, match="classifier's gradient"):
        model_wrapper(model, ns, guidance_type="classifier")
    with pytest.raises(ValueError, match="model_type"):
        model_wrapper(model, ns, model_type="flow")
    with pytest.raises(ValueError, match="guidance_type"):
        model_wrapper(model, ns, guidance_type="cfg")
    x = torch.zeros((B, 4, H, W), device=DEV)
    with pytest.raises(NotImplementedError, match="device-to-host error norm"):
        DPM_Solver(model_wrapper(model, ns), ns).sample(x, method="adaptive")
    with pytest.raises(ValueError, match="max_val"):
        DPM_Solver(model_wrapper(model, ns), ns, predict_x0=True, thresholding=True, max_val=0.)


# ------------------------------------------------------------------------------------------------ the pipeline
SOLVER = dict(order=3, skip_type="logSNR")


def test_pipeline_solver_defaults(tiny, monkeypatch):
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model, _, x_T, c, uc = tiny
    d = lambda a: torch.tensor(a, device=DEV)
    pipe = DiffusionPipeline(model, sampler="dpm_solver", solver=SOLVER)
    assert not pipe.sampler.wired and pipe.sampler.solver["order"] == 3 and pipe.sampler.solver["skip_type"] == "logSNR"
    c16, uc16 = d(c).half(), d(uc).half()
    S = 8
    # txt2img
    got = pipe(c=d(c), uc=d(uc), H=8 * H, W=8 * W, steps=S, scale=SCALE, seed=5)
    ref = DPMSolverSampler(model).sample(S, B, [4, H, W], conditioning=c16, x_T=pipe.start_noise(B, [4, H, W], 5).to(DEV),
                                         unconditional_guidance_scale=SCALE, unconditional_conditioning=uc16, verbose=False,
                                         **SOLVER)[0]
    assert torch.equal(got, ref)
    wired = DiffusionPipeline(model, sampler="dpm_solver")(c=d(c), uc=d(uc), H=8 * H, W=8 * W, steps=S, scale=SCALE, seed=5)
    assert not torch.equal(got, wired)
    # img2img: the last int(0.5 * S) steps from t_start, one launch each
    z0, noise = d(x_T) * 0.5, d(np.random.RandomState(9).randn(B, 4, H, W).astype(np.float32))
    count = []
    real = ops.sampler_step_lin
    monkeypatch.setattr(ops, "sampler_step_lin", lambda *a, **k: (count.append(1), real(*a, **k))[1])
    got = pipe.img2img(init_latent=z0, strength=0.5, c=d(c), uc=d(uc), steps=S, scale=SCALE, noise=noise)
    assert len(count) == S // 2
    sampler = DPMSolverSampler(model, **SOLVER)
    start, a, b = pipe._partial_start(S, S // 2, 0.)
    x_enc = sampler.stochastic_encode(z0, start, noise=noise)
    ref = sampler.sample(S // 2, B, [4, H, W], conditioning=c16, x_T=x_enc, t_start=start, unconditional_guidance_scale=SCALE,
                         unconditional_conditioning=uc16, verbose=False)[0]
    assert torch.equal(got, ref)
    # windowed() hands the options on, and its runs use them
    wp = pipe.windowed(window=8 * H)
    assert wp.sampler.solver == pipe.sampler.solver and not wp.sampler.wired
    del count[:]
    out = wp(c=d(c), uc=d(uc), H=8 * H, W=16 * W, steps=6, scale=SCALE, seed=5)
    assert len(count) == 6 and tuple(out.shape) == (B, 4, H, 2 * W) and bool(torch.isfinite(out).all())
    assert DiffusionPipeline(model, sampler="dpm_solver").windowed(window=8 * H).sampler.wired


def test_refusals_with_non_default_options(tiny):
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model, _, x_T, c, uc = tiny
    d = lambda a: torch.tensor(a, device=DEV)
    pipe = DiffusionPipeline(model, sampler="dpm_solver", solver=SOLVER)
    with pytest.raises(ValueError, match="session.*multistep order-2.*order, skip_type"):
        pipe.session(slots=2, H=8 * H, W=8 * W)
    with pytest.raises(ValueError, match="session.*multistep order-2"):
        pipe.serve([dict(c=d(c)[:1], uc=d(uc)[:1], steps=4)], slots=2, H=8 * H, W=8 * W, output="latent")
    for kw in (dict(S=[6, 8]), dict(unconditional_guidance_scale=[3.0, 5.0]), dict(guidance_rescale=[0.0, 0.7])):
        args = dict(S=6, batch_size=B, shape=(4, H, W), conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=SCALE,
                    unconditional_conditioning=d(uc), verbose=False, method="singlestep")
        args.update(kw)
        with pytest.raises(ValueError, match="per-request.*step table.*method"):
            DPMSolverSampler(model).sample(**args)
    with pytest.raises(ValueError, match="per-request.*order, skip_type"):
        pipe(c=d(c), uc=d(uc), H=8 * H, W=8 * W, steps=[6, 8], scale=SCALE)
    with pytest.raises(ValueError, match="solver= holds DPM-Solver options"):
        DiffusionPipeline(model, sampler="ddim", solver=SOLVER)
    with pytest.raises(ValueError, match="unknown option.*steps"):
        DiffusionPipeline(model, sampler="dpm_solver", solver=dict(steps=3))
    with pytest.raises(ValueError, match="Unsupported skip_type"):
        DPMSolverSampler(model, skip_type="cosine")
    with pytest.raises(NotImplementedError, match="adaptive"):
        DPMSolverSampler(model, method="adaptive")
    with pytest.raises(ValueError, match="max_val"):
        DPMSolverSampler(model, thresholding=True, max_val=-1.)


def test_v_prediction_with_guidance_rescale(monkeypatch):
    """What sits in front of the step -- a v model's conversion and the guidance rescale -- on the new path: multistep order 3
    on a logSNR grid against the restatement on the v oracle with the rescale in its apply_model (tests/_rescale_util.py)."""
    import _rescale_util as R
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    model, cfg, params = V.tiny_eps_model(parameterization="v")
    om = R.RescaleModelOracle(V.VModelOracle(O.UNetOracle(dict(cfg, num_heads=-1), params)), 0.7, SCALE, V.B)
    x_T, c, uc = V.tiny_inputs(cfg["context_dim"])
    opts = dict(order=3, skip_type="logSNR")
    ref, solver = F.sample(om, 10, V.B, (4, V.H, V.W), c, x_T, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc,
                           **opts)
    assert solver.nfe == 10 and len(om.factors) == 10
    d = lambda a: torch.tensor(a, device=DEV)
    got = DPMSolverSampler(model).sample(10, V.B, (4, V.H, V.W), conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=SCALE,
                                         unconditional_conditioning=d(uc), guidance_rescale=0.7, verbose=False, **opts)[0]
    check("tiny_dpm_full_v_rescale_multistep3_logSNR_S10", got, ref, rel_l2=1e-2, max_rel=1e-2)
