"""UniPC end to end: UniPCSampler / UniPC on the tiny UNet of tests/test_dpm_solver_gpu.py (B 2, 8 x 8 latent, 6 context tokens)
against tests/_unipc_full_util.py, a torch-CPU restatement of the paper's update on the oracle UNet.

Bar: the project's own for this test family, check(..., rel_l2=1e-2, max_rel=1e-2), for every configuration.

Also here: one model evaluation and exactly one ops.sampler_step_pc launch per record and no other step launch; the callbacks;
per-sample seeds; the pipeline's sampler="uni_pc" on txt2img, img2img and windowed(); the refusals by message; and UniPC without
its corrector at order 2 / bh2 against DPMSolverSampler(order=2), the same mathematics through another launch."""
import numpy as np
import pytest
import torch

import _unipc_full_util as F
import _vpred_util as V
from _util import check
from oracle import ldm as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W, T = 2, 8, 8, 6
SCALE = 3.0
STEP_ENTRIES = ("sampler_step_pc", "sampler_step_lin", "sampler_step_lin_noise", "sampler_step", "sampler_step_pred",
                "sampler_step_rescale", "sampler_step_table")

# name -> (S, sampler options)
CONFIGS = {
    "order3_bh2_uniform_S8": (8, dict()),
    "order2_bh1_logSNR_S6": (6, dict(order=2, variant="bh1", skip_type="logSNR")),
    "order3_karras_threshold_S10": (10, dict(skip_type="karras", thresholding=True)),
    "order2_noise_form_S8": (8, dict(order=2, predict_x0=False)),
    "order3_no_corrector_S8": (8, dict(corrector=False)),
    "order3_t_start_S6": (6, dict(t_start=0.6)),
    "order2_denoise_to_zero_S6": (6, dict(order=2, denoise_to_zero=True)),
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
    from minddiffusion_amd.ldm.models.diffusion.uni_pc import UniPCSampler
    d = lambda a: torch.tensor(a, device=DEV)
    return UniPCSampler(model).sample(S, B, (4, H, W), conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=SCALE,
                                      unconditional_conditioning=d(uc), verbose=False, **opts, **kw)


def count_entries(monkeypatch, ops):
    count = {}
    for entry in STEP_ENTRIES:
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
    evals = S + int(bool(opts.get("denoise_to_zero")))
    assert solver.nfe == evals
    if opts.get("thresholding"):
        won = sum(bool((s > opts["max_val"]).all()) for s in solver.raw_s)
        print(f"{name}: max_val {opts['max_val']:.4f}, s > max_val in {won} of {len(solver.raw_s)} evaluations (oracle side)")
        assert len(solver.raw_s) == evals and 0 < won < evals
    count = count_entries(monkeypatch, ops)
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
    assert count == {"sampler_step_pc": evals} and len(unet_calls) == evals
    check(f"tiny_unipc_{name}", got, ref, rel_l2=1e-2, max_rel=1e-2)


def test_the_corrector_changes_the_result(tiny):
    on, off = reference(tiny, "order3_bh2_uniform_S8")[0], reference(tiny, "order3_no_corrector_S8")[0]
    assert float((on - off).norm() / on.norm()) > 1e-3


def test_v_prediction_with_guidance_rescale():
    import _rescale_util as R
    from minddiffusion_amd.ldm.models.diffusion.uni_pc import UniPCSampler
    model, cfg, params = V.tiny_eps_model(parameterization="v")
    om = R.RescaleModelOracle(V.VModelOracle(O.UNetOracle(dict(cfg, num_heads=-1), params)), 0.7, SCALE, V.B)
    x_T, c, uc = V.tiny_inputs(cfg["context_dim"])
    ref, solver = F.sample(om, 8, V.B, (4, V.H, V.W), c, x_T, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)
    assert solver.nfe == 8 and len(om.factors) == 8
    d = lambda a: torch.tensor(a, device=DEV)
    got = UniPCSampler(model).sample(8, V.B, (4, V.H, V.W), conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=SCALE,
                                     unconditional_conditioning=d(uc), guidance_rescale=0.7, verbose=False)[0]
    check("tiny_unipc_v_rescale_order3_S8", got, ref, rel_l2=1e-2, max_rel=1e-2)


def test_hybrid_conditioning():
    """Dict conditioning with a c_concat on both sides, as DPMSolverSampler takes it: it lives in GuidedModel."""
    import _inpaint_util as U
    from minddiffusion_amd.ldm.models.diffusion.uni_pc import UniPCSampler
    hybrid, om = U.tiny_model(DEV, 9), U.oracle_model()
    S, L = 8, U.LAT
    rng = np.random.RandomState(18)
    ctx = U.tiny_cfg()["context_dim"]
    x_T = rng.randn(U.B, 4, L, L).astype(np.float32)
    c = rng.randn(U.B, U.T, ctx).astype(np.float32)
    uc = np.repeat(rng.randn(1, U.T, ctx).astype(np.float32), U.B, 0)
    c_cat = np.concatenate([(rng.rand(U.B, 1, L, L) > 0.5).astype(np.float32), rng.randn(U.B, 4, L, L).astype(np.float32)], 1)
    dev = lambda a: torch.tensor(a, device=DEV)
    got = UniPCSampler(hybrid).sample(S, U.B, (4, L, L), conditioning={"c_concat": dev(c_cat), "c_crossattn": dev(c)}, x_T=dev(x_T),
                                      unconditional_guidance_scale=U.SCALE,
                                      unconditional_conditioning={"c_concat": dev(c_cat), "c_crossattn": dev(uc)}, verbose=False)[0]
    cat2 = torch.cat([torch.as_tensor(c_cat), torch.as_tensor(c_cat)])
    ref, _ = F.sample(om, S, U.B, (4, L, L), c, x_T, unconditional_guidance_scale=U.SCALE, unconditional_conditioning=uc,
                      apply=lambda x, tt, cc: om.apply_model(x, tt, {"c_concat": cat2, "c_crossattn": cc}))
    check("tiny_unipc_hybrid_order3_S8", got, ref, rel_l2=1e-2, max_rel=1e-2)


def test_a_seeded_row_is_the_batch_1_run(tiny, monkeypatch):
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.uni_pc import UniPCSampler
    model, _, _, c, uc = tiny
    d = lambda a: torch.tensor(a, device=DEV)
    seeds = [1234, 99]
    run = lambda rows, s: UniPCSampler(model).sample(6, len(s), (4, H, W), conditioning=d(c[rows]), seeds=s,
                                                     unconditional_guidance_scale=SCALE, unconditional_conditioning=d(uc[rows]),
                                                     verbose=False)[0]
    both = run(slice(0, 2), seeds)
    count = count_entries(monkeypatch, ops)
    for b in range(B):
        assert torch.equal(both[b:b + 1], run(slice(b, b + 1), seeds[b:b + 1])), b
    assert count == {"sampler_step_pc": 12}
    assert not torch.equal(both[0], both[1])
    with pytest.raises(ValueError):
        UniPCSampler(model, generator=torch.Generator(device=DEV)).sample(
            6, B, (4, H, W), conditioning=d(c), seeds=seeds, unconditional_conditioning=d(uc), verbose=False)


def test_the_solver_surface(tiny):
    """UniPC on model_wrapper's result and on a foreign (x, t_continuous) -> eps callable."""
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import NoiseScheduleVP
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver.solver import model_wrapper
    from minddiffusion_amd.ldm.models.diffusion.uni_pc import UniPC
    model, _, x_T, c, uc = tiny
    d = lambda a: torch.tensor(a, device=DEV)
    ns = NoiseScheduleVP("discrete", alphas_cumprod=np.asarray(model.alphas_cumprod, np.float64))
    fn = model_wrapper(model, ns, model_type="noise", guidance_type="classifier-free", condition=d(c),
                       unconditional_condition=d(uc), guidance_scale=SCALE)
    ref = reference(tiny, "order3_bh2_uniform_S8")[0]
    got = UniPC(fn, ns).sample(d(x_T), steps=8)
    check("tiny_unipc_UniPC_model_wrapper", got, ref, rel_l2=1e-2, max_rel=1e-2)
    foreign = UniPC(lambda x, t: fn(x, t), ns).sample(d(x_T), steps=8)
    check("tiny_unipc_UniPC_foreign_callable", foreign, ref, rel_l2=1e-2, max_rel=1e-2)
    ref2 = reference(tiny, "order2_bh1_logSNR_S6")[0]
    got2 = UniPC(fn, ns, variant="bh1").sample(d(x_T), steps=6, order=2, skip_type="logSNR")
    check("tiny_unipc_UniPC_bh1", got2, ref2, rel_l2=1e-2, max_rel=1e-2)


def test_without_the_corrector_order_2_is_dpm_solver_2m(tiny, monkeypatch):
    """UniP-2 / bh2 and DPM-Solver++ 2M are one update: the two samplers end within the bar of each other, each through its own
    launch (a t_end one part in 10^12 off its default keeps DPMSolverSampler off its wired launches and on solver_plan's)."""
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.uni_pc import UniPCSampler
    model, _, x_T, c, uc = tiny
    d = lambda a: torch.tensor(a, device=DEV)
    kw = dict(conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=SCALE, unconditional_conditioning=d(uc), verbose=False)
    count = count_entries(monkeypatch, ops)
    uni = UniPCSampler(model, order=2, variant="bh2", corrector=False).sample(8, B, (4, H, W), **kw)[0]
    assert count == {"sampler_step_pc": 8}
    count.clear()
    dpm = DPMSolverSampler(model, order=2).sample(8, B, (4, H, W), skip_type="time_uniform", t_end=1e-3 * (1 + 1e-12), **kw)[0]
    assert count == {"sampler_step_lin": 8}
    check("tiny_unipc_order2_no_corrector_vs_dpm_solver_2m", uni, dpm, rel_l2=1e-2, max_rel=1e-2)


# ------------------------------------------------------------------------------------------------ the pipeline
SOLVER = dict(order=2, variant="bh1", skip_type="logSNR")


def test_pipeline_uni_pc(tiny, monkeypatch):
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.uni_pc import UniPCSampler
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model, _, x_T, c, uc = tiny
    d = lambda a: torch.tensor(a, device=DEV)
    plain = DiffusionPipeline(model, sampler="uni_pc")
    assert isinstance(plain.sampler, UniPCSampler) and plain._solver() is None
    assert (plain.sampler.solver["order"], plain.sampler.solver["variant"], plain.sampler.solver["skip_type"]) == (3, "bh2", "time_uniform")
    pipe = DiffusionPipeline(model, sampler="uni_pc", solver=SOLVER)
    assert pipe._solver() == SOLVER
    c16, uc16 = d(c).half(), d(uc).half()
    S = 8
    # txt2img
    got = pipe(c=d(c), uc=d(uc), H=8 * H, W=8 * W, steps=S, scale=SCALE, seed=5)
    ref = UniPCSampler(model).sample(S, B, [4, H, W], conditioning=c16, x_T=pipe.start_noise(B, [4, H, W], 5).to(DEV),
                                     unconditional_guidance_scale=SCALE, unconditional_conditioning=uc16, verbose=False, **SOLVER)[0]
    assert torch.equal(got, ref)
    assert not torch.equal(got, plain(c=d(c), uc=d(uc), H=8 * H, W=8 * W, steps=S, scale=SCALE, seed=5))
    # img2img: the last int(0.5 * S) steps from t_start, one launch each
    z0, noise = d(x_T) * 0.5, d(np.random.RandomState(9).randn(B, 4, H, W).astype(np.float32))
    count = count_entries(monkeypatch, ops)
    got = pipe.img2img(init_latent=z0, strength=0.5, c=d(c), uc=d(uc), steps=S, scale=SCALE, noise=noise)
    assert count == {"sampler_step_pc": S // 2}
    sampler = UniPCSampler(model, **SOLVER)
    start, a, b = pipe._partial_start(S, S // 2, 0.)
    x_enc = sampler.stochastic_encode(z0, start, noise=noise)
    ref = sampler.sample(S // 2, B, [4, H, W], conditioning=c16, x_T=x_enc, t_start=start, unconditional_guidance_scale=SCALE,
                         unconditional_conditioning=uc16, verbose=False)[0]
    assert torch.equal(got, ref)
    # windowed() hands the sampler kind and its options on, and its runs use them
    wp = pipe.windowed(window=8 * H)
    assert isinstance(wp.sampler, UniPCSampler) and wp.sampler.solver == pipe.sampler.solver
    count.clear()
    out = wp(c=d(c), uc=d(uc), H=8 * H, W=16 * W, steps=6, scale=SCALE, seed=5)
    assert count == {"sampler_step_pc": 6} and tuple(out.shape) == (B, 4, H, 2 * W) and bool(torch.isfinite(out).all())
    assert isinstance(plain.windowed(window=8 * H).sampler, UniPCSampler)


def test_refusals_by_name(tiny):
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.uni_pc import UniPCSampler
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model, _, x_T, c, uc = tiny
    d = lambda a: torch.tensor(a, device=DEV)
    pipe = DiffusionPipeline(model, sampler="uni_pc")
    with pytest.raises(MdxError, match="session.*UniPC has no rows"):
        pipe.session(slots=2, H=8 * H, W=8 * W)
    with pytest.raises(MdxError, match="session.*UniPC has no rows"):
        pipe.serve([dict(c=d(c)[:1], uc=d(uc)[:1], steps=4)], slots=2, H=8 * H, W=8 * W, output="latent")
    with pytest.raises(MdxError, match="per-request.*UniPC takes scalars"):
        pipe(c=d(c), uc=d(uc), H=8 * H, W=8 * W, steps=[6, 8], scale=SCALE)
    with pytest.raises(MdxError, match="per-request.*UniPC takes scalars"):
        pipe(c=d(c), uc=d(uc), H=8 * H, W=8 * W, steps=6, scale=[3.0, 5.0])
    args = dict(S=6, batch_size=B, shape=(4, H, W), conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=SCALE,
                unconditional_conditioning=d(uc), verbose=False)
    mask = torch.ones((B, 1, H, W), device=DEV)
    for kw, err, match in ((dict(mask=mask, x0=d(x_T)), MdxError, "mask / x0 blending"),
                           (dict(image_guidance_scale=1.5), MdxError, "image_guidance_scale"),
                           (dict(sde_eta=1.0), MdxError, "sde_eta"),
                           (dict(method="singlestep"), ValueError, "only method 'multistep'"),
                           (dict(order=4), ValueError, "order must be 1, 2 or 3"),
                           (dict(variant="vary_coeff"), ValueError, "variant must be 'bh1' or 'bh2'"),
                           (dict(S=2), ValueError, "steps must be an int >= order")):
        with pytest.raises(err, match=match):
            UniPCSampler(model).sample(**{**args, **kw})
    with pytest.raises(NotImplementedError, match="mask blending"):
        pipe.img2img(init_latent=d(x_T), strength=0.5, c=d(c), uc=d(uc), steps=6, scale=SCALE, mask=mask)
    with pytest.raises(ValueError, match="unknown option.*steps"):
        DiffusionPipeline(model, sampler="uni_pc", solver=dict(steps=3))
    with pytest.raises(ValueError, match="solver= holds DPM-Solver options"):
        DiffusionPipeline(model, sampler="plms", solver=SOLVER)
