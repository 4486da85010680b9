"""The Karras grid and the SDE update of DPMSolverSampler end to end ("DPM++ 2M Karras", "DPM++ 2M SDE Karras") on the tiny UNet
of tests/test_dpm_solver_gpu.py (B 2, 8 x 8 latent, 6 context tokens) against tests/_dpm_sde_util.py, a torch-CPU restatement in
k-diffusion's un-folded form on the oracle UNet.  The same step noises are injected on both sides.

Bar: the family's own, check(..., rel_l2=1e-2, max_rel=1e-2), for every configuration.  (Should one miss it, its bar becomes
twice the oracle's own fp32 vs emulate_fp16() distance through the same restatement -- a CPU measurement on the reference side
only.  None needs it: those distances are 1.5e-3 ... 3.7e-3 rel-L2 for the configurations below, docs/PARITY.md has them.)
The noise matters: on the reference side alone the eta > 0 result lies at least 10 x the bar (rel-L2 >= 0.1) from the eta = 0
result of the same configuration (0.41 ... 1.15 measured), so a run that dropped or mis-scaled the noise cannot pass.

Also here: one model evaluation and exactly one ops.sampler_step_lin_noise launch per stochastic record and no other launch
for its noise; seeds= against injected ops.randn_seeded noises, bit for bit, in the sampler and in the pipeline; the options
through DPM_Solver, the pipeline's solver=, img2img, windowed() and hires()."""
import numpy as np
import pytest
import torch

import _dpm_sde_util as SD
import _vpred_util as V
from _util import check
from oracle import ldm as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, T = 2, 8, 8, 6
SCALE = 3.0

# name -> (S, solver options)
CONFIGS = {
    "2m_karras_S12": (12, dict(skip_type="karras")),
    "2m_sde_karras_S10": (10, dict(skip_type="karras", sde_eta=1.0)),
    "order1_sde_uniform_S8": (8, dict(order=1, sde_eta=0.5)),
    "2m_sde_karras_threshold_S10": (10, dict(skip_type="karras", sde_eta=1.0, thresholding=True)),
}
STEP_ENTRIES = ("sampler_step_lin", "sampler_step_lin_noise", "sampler_step", "sampler_step_pred", "sampler_step_rescale",
                "sampler_step_table", "randn_seeded")


def noises(n, seed=77):
    rng = np.random.RandomState(seed)
    return [rng.randn(B, 4, H, W).astype(np.float32) for _ in range(n)]


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
        run = lambda **kw: SD.sample(om, S, B, (4, H, W), c, x_T, unconditional_guidance_scale=SCALE,
                                     unconditional_conditioning=uc, step_noises=noises(S), **kw)
        if opts.get("thresholding"):
            # max_val from the oracle's run alone: the lower quartile of the thresholds of a run in which s always wins
            _, probe = run(**dict(opts, max_val=1e-6))
            opts["max_val"] = float(torch.quantile(torch.stack(probe.raw_s).min(dim=1).values, 0.25))
        ref, solver = run(**opts)
        if opts.get("sde_eta"):
            det, _ = run(**dict(opts, sde_eta=0.))
            moved = float((ref - det).norm() / det.norm())
            print(f"{name}: eta > 0 vs eta = 0 on the oracle side, rel-L2 {moved:.3f}")
            assert moved >= 0.1
        _REFS[name] = (ref, solver, opts)
    return _REFS[name]


def sample(model, x_T, c, uc, S, opts, sampler_kw=None, **kw):
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    d = lambda a: None if a is None else torch.tensor(a, device=DEV)
    return DPMSolverSampler(model, **(sampler_kw or {})).sample(S, B, (4, H, W), conditioning=d(c), x_T=d(x_T),
                                                                unconditional_guidance_scale=SCALE,
                                                                unconditional_conditioning=d(uc), verbose=False, **opts, **kw)


def count_entries(monkeypatch, ops, entries=STEP_ENTRIES):
    count = {}
    for entry in entries:
        def counted(*a, _real=getattr(ops, entry), _entry=entry, **k):
            count[_entry] = count.get(_entry, 0) + 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, entry, counted)
    return count


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_configuration_against_the_restatement(tiny, monkeypatch, name):
    from minddiffusion_amd import ops
    model, _, x_T, c, uc = tiny
    S = CONFIGS[name][0]
    ref, solver, opts = reference(tiny, name)
    assert solver.nfe == S and solver.updates == S
    noisy = S if opts.get("sde_eta") else 0
    if opts.get("thresholding"):
        won = sum(bool((s > opts["max_val"]).all()) for s in solver.raw_s)
        print(f"{name}: max_val {opts['max_val']:.4f}, s > max_val in {won} of {len(solver.raw_s)} evaluations (oracle side)")
        assert len(solver.raw_s) == S and 2 * won >= S and won < S
    count = count_entries(monkeypatch, ops)
    unet_calls = []
    real_nhwc = model.apply_model_nhwc
    monkeypatch.setattr(model, "apply_model_nhwc", lambda *a, **k: (unet_calls.append(1), real_nhwc(*a, **k))[1], raising=False)
    calls = []
    got, inter = sample(model, x_T, c, uc, S, opts, step_noises=noises(S) if noisy else None, callback=lambda i: calls.append(i),
                        eta=0.3)                # (`eta` is the reference's keyword: ignored, as the pipeline relies on)
    assert inter is None and calls == list(range(S)) and len(unet_calls) == S
    assert count == ({"sampler_step_lin_noise": S} if noisy else {"sampler_step_lin": S})
    check(f"tiny_dpm_sde_{name}", got, ref, rel_l2=1e-2, max_rel=1e-2)


def test_v_prediction_with_guidance_rescale():
    """What sits in front of the step -- a v model's conversion and the guidance rescale, the one-workgroup-per-sample launch
    form -- under the SDE update."""
    import _rescale_util as R
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    model, cfg, params = V.tiny_eps_model(parameterization="v")
    om = R.RescaleModelOracle(V.VModelOracle(O.UNetOracle(dict(cfg, num_heads=-1), params)), 0.7, SCALE, V.B)
    x_T, c, uc = V.tiny_inputs(cfg["context_dim"])
    opts = dict(skip_type="karras", sde_eta=1.0)
    run = lambda **kw: SD.sample(om, 10, V.B, (4, V.H, V.W), c, x_T, unconditional_guidance_scale=SCALE,
                                 unconditional_conditioning=uc, step_noises=noises(10), **kw)[0]
    ref, det = run(**opts), run(**dict(opts, sde_eta=0.))
    assert float((ref - det).norm() / det.norm()) >= 0.1
    d = lambda a: torch.tensor(a, device=DEV)
    got = DPMSolverSampler(model).sample(10, V.B, (4, V.H, V.W), conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=SCALE,
                                         unconditional_conditioning=d(uc), guidance_rescale=0.7, verbose=False,
                                         step_noises=noises(10), **opts)[0]
    check("tiny_dpm_sde_v_rescale_2m_sde_karras_S10", got, ref, rel_l2=1e-2, max_rel=1e-2)


# ------------------------------------------------------------------------------------------------ the noise sources
def test_seeds_draw_inside_the_step_launch(tiny, monkeypatch):
    """seeds=: sample b's x_T and step noises from seeds[b] alone -- the bits of a run fed ops.randn_seeded's tensors -- with
    one launch per record and no randn_seeded launch inside the loop."""
    from minddiffusion_amd import ops
    model, _, _, c, uc = tiny
    S, opts, seeds = 6, dict(skip_type="karras", sde_eta=1.0), [7, (1 << 64) - 3]
    st = ops.seeds_tensor(seeds, DEV)
    x_T = ops.randn_seeded(st, ops.RNG_X_T, 0, (4, H, W))
    injected = [ops.randn_seeded(st, ops.RNG_STEP, k, (4, H, W)) for k in range(S)]
    fed = sample(model, x_T.cpu().numpy(), c, uc, S, opts, step_noises=injected)[0]
    count = count_entries(monkeypatch, ops)
    seeded = sample(model, None, c, uc, S, opts, seeds=seeds)[0]
    assert count == {"sampler_step_lin_noise": S, "randn_seeded": 1}          # (the one draw: x_T, before the loop)
    assert torch.equal(seeded, fed)
    assert not torch.equal(sample(model, None, c, uc, S, opts, seeds=[7, 8])[0][1], seeded[1])
    with pytest.raises(ValueError, match="two sources"):
        sample(model, None, c, uc, S, opts, seeds=seeds, step_noises=injected)
    with pytest.raises(ValueError, match="two sources"):
        sample(model, None, c, uc, S, opts, seeds=seeds, sampler_kw=dict(generator=torch.Generator(device=DEV)))


def test_generator_draws_one_randn_per_record(tiny, monkeypatch):
    from minddiffusion_amd import ops
    model, _, x_T, c, uc = tiny
    S, opts = 5, dict(sde_eta=0.7)
    gen = lambda: torch.Generator(device=DEV).manual_seed(123)
    g = gen()
    injected = [torch.randn((B, 4, H, W), device=DEV, dtype=torch.float32, generator=g) for _ in range(S)]
    fed = sample(model, x_T, c, uc, S, opts, step_noises=injected)[0]
    count = count_entries(monkeypatch, ops)
    drawn = sample(model, x_T, c, uc, S, opts, sampler_kw=dict(generator=gen()))[0]
    assert count == {"sampler_step_lin_noise": S} and torch.equal(drawn, fed)
    other = sample(model, x_T, c, uc, S, opts, sampler_kw=dict(generator=torch.Generator(device=DEV).manual_seed(124)))[0]
    assert not torch.equal(other, drawn)
    # s_noise scales the noise only: 0 is the eta-damped deterministic run, whatever the noises are
    quiet = sample(model, x_T, c, uc, S, dict(opts, s_noise=0.), step_noises=injected)[0]
    quiet2 = sample(model, x_T, c, uc, S, dict(opts, s_noise=0.), step_noises=noises(S))[0]
    assert torch.equal(quiet, quiet2) and not torch.equal(quiet, fed)


# ------------------------------------------------------------------------------------------------ option plumbing
def test_default_options_are_the_wired_run(tiny, monkeypatch):
    """Every option spelled out at its default, the new ones included: the launches and the bits of a call without them; and a
    deterministic non-default run makes no noise launch."""
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver.solver import SOLVER_DEFAULTS
    model, _, x_T, c, uc = tiny
    plain = sample(model, x_T, c, uc, 6, {})[0]
    count = count_entries(monkeypatch, ops)
    spelled = sample(model, x_T, c, uc, 6, dict(SOLVER_DEFAULTS, rho=3., s_noise=2.))[0]    # (neither is read at the defaults)
    assert count == {"sampler_step": 6} and torch.equal(plain, spelled)
    count.clear()
    karras = sample(model, x_T, c, uc, 6, dict(skip_type="karras"))[0]
    assert count == {"sampler_step_lin": 6} and not torch.equal(karras, plain)
    assert not torch.equal(sample(model, x_T, c, uc, 6, dict(skip_type="karras", rho=3.))[0], karras)


def test_dpm_solver_surface(tiny):
    """DPM_Solver.sample(skip_type="karras", rho=, sde_eta=, s_noise=, seeds= | generator=) is the sampler's run."""
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPM_Solver, NoiseScheduleVP, model_wrapper
    model, _, x_T, c, uc = tiny
    d = lambda a: torch.tensor(a, device=DEV)
    ns = NoiseScheduleVP("discrete", alphas_cumprod=np.asarray(model.alphas_cumprod, np.float64))
    fn = model_wrapper(model, ns, model_type="noise", guidance_type="classifier-free", condition=d(c),
                       unconditional_condition=d(uc), guidance_scale=SCALE)
    S, seeds = 6, [3, 4]
    opts = dict(skip_type="karras", rho=5., sde_eta=1.0, s_noise=0.9)
    got = DPM_Solver(fn, ns, predict_x0=True).sample(d(x_T), steps=S, order=2, method="multistep", seeds=seeds, **opts)
    ref = sample(model, x_T, c, uc, S, opts, seeds=seeds)[0]
    assert torch.equal(got, ref)
    st = ops.seeds_tensor(seeds, DEV)
    fed = DPM_Solver(fn, ns, predict_x0=True).sample(d(x_T), steps=S, order=2, method="multistep", **opts,
                                                     step_noises=[ops.randn_seeded(st, ops.RNG_STEP, k, (4, H, W)) for k in range(S)])
    assert torch.equal(fed, got)
    with pytest.raises(ValueError, match="sde_eta"):
        DPM_Solver(fn, ns).sample(d(x_T), steps=S, order=2, method="multistep", sde_eta=1.0)      # predict_x0=False
    with pytest.raises(ValueError, match="sde_eta"):
        DPM_Solver(fn, ns, predict_x0=True).sample(d(x_T), steps=S, sde_eta=1.0)                # singlestep, order 3
    with pytest.raises(ValueError, match="two sources"):
        DPM_Solver(fn, ns, predict_x0=True).sample(d(x_T), steps=S, order=2, method="multistep", seeds=seeds,
                                                   generator=torch.Generator(device=DEV), **opts)


SOLVER = dict(skip_type="karras", sde_eta=1.0)


def test_pipeline_surfaces(tiny, monkeypatch):
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model, _, x_T, c, uc = tiny
    d = lambda a: torch.tensor(a, device=DEV)
    pipe = DiffusionPipeline(model, sampler="dpm_solver", solver=SOLVER)
    assert not pipe.sampler.wired and pipe.sampler.solver["sde_eta"] == 1.0 and pipe.sampler.solver["skip_type"] == "karras"
    c16, uc16 = d(c).half(), d(uc).half()
    S, seeds = 6, [21, 22]
    st = ops.seeds_tensor(seeds, DEV)
    step_z = lambda n: [ops.randn_seeded(st, ops.RNG_STEP, k, (4, H, W)) for k in range(n)]
    # txt2img with seeds: the sampler's run on injected randn_seeded noises, bit for bit; eta= is handed on and ignored
    got = pipe(c=d(c), uc=d(uc), H=8 * H, W=8 * W, steps=S, scale=SCALE, seeds=seeds, eta=0.4)
    ref = DPMSolverSampler(model).sample(S, B, [4, H, W], conditioning=c16, x_T=ops.randn_seeded(st, ops.RNG_X_T, 0, (4, H, W)),
                                         unconditional_guidance_scale=SCALE, unconditional_conditioning=uc16, verbose=False,
                                         step_noises=step_z(S), **SOLVER)[0]
    assert torch.equal(got, ref)
    assert not torch.equal(got, pipe(c=d(c), uc=d(uc), H=8 * H, W=8 * W, steps=S, scale=SCALE, seeds=[21, 23]))
    # img2img: the last S // 2 steps from t_start, one noise launch each, the draws counted from the partial run's start
    z0, noise = d(x_T) * 0.5, d(np.random.RandomState(9).randn(B, 4, H, W).astype(np.float32))
    count = count_entries(monkeypatch, ops, ("sampler_step_lin", "sampler_step_lin_noise", "sampler_step"))
    got = pipe.img2img(init_latent=z0, strength=0.5, c=d(c), uc=d(uc), steps=S, scale=SCALE, noise=noise, seeds=seeds)
    assert count == {"sampler_step_lin_noise": S // 2}
    sampler = DPMSolverSampler(model, **SOLVER)
    start, a, b = pipe._partial_start(S, S // 2, 0.)
    x_enc = sampler.stochastic_encode(z0, start, noise=noise)
    ref = sampler.sample(S // 2, B, [4, H, W], conditioning=c16, x_T=x_enc, t_start=start, unconditional_guidance_scale=SCALE,
                         unconditional_conditioning=uc16, verbose=False, step_noises=step_z(S // 2))[0]
    assert torch.equal(got, ref)
    # windowed() and hires() hand the options on, and their runs use them
    wp = pipe.windowed(window=8 * H)
    assert wp.sampler.solver == pipe.sampler.solver and not wp.sampler.wired
    count.clear()
    out = wp(c=d(c), uc=d(uc), H=8 * H, W=16 * W, steps=4, scale=SCALE, seeds=seeds)
    assert count == {"sampler_step_lin_noise": 4} and tuple(out.shape) == (B, 4, H, 2 * W) and bool(torch.isfinite(out).all())
    count.clear()
    big = pipe.hires(c=d(c), uc=d(uc), base=(8 * H, 8 * W), H=16 * H, W=16 * W, steps=4, strength=0.5, scale=SCALE, seeds=seeds)
    assert count == {"sampler_step_lin_noise": 4 + 2} and tuple(big.shape) == (B, 4, 2 * H, 2 * W)
    assert bool(torch.isfinite(big).all())
    # the refusals the other options get, through the same code
    with pytest.raises(ValueError, match="session.*multistep order-2.*sde_eta, skip_type"):
        pipe.session(slots=2, H=8 * H, W=8 * W)
    with pytest.raises(ValueError, match="per-request.*sde_eta, skip_type"):
        pipe(c=d(c), uc=d(uc), H=8 * H, W=8 * W, steps=[4, 6], scale=SCALE)
