"""WindowedDiffusion end to end on the GPU, on the tiny UNet with 8 x 8 latent windows.  No tolerance anywhere: a windowed
evaluation must be torch.equal to the composition the test makes itself from the inner model (_window_util.HostComposition:
torch slicing, the inner model on the same window batches -- the same batch sizes, so the same launch plans -- and the numpy
restatement of the averaging arithmetic on the CPU), per call and over whole sampler runs; a single window the size of the canvas
must be the plain pipeline bit for bit; img2img with a mask blend, hybrid inpainting and a sampling session inherit both."""
import numpy as np
import pytest
import torch

import _inpaint_util as I
import _vpred_util as V
import _window_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIN, STRIDE = (8, 8), (4, 4)


@pytest.fixture(scope="module")
def tiny():
    eps_model, cfg, _ = V.tiny_eps_model()
    v_model, _, _ = V.tiny_eps_model(parameterization="v")
    rng = np.random.RandomState(523)
    d = lambda a: torch.tensor(a.astype(np.float32), device=DEV)
    return {"eps": eps_model, "v": v_model, "c": d(rng.randn(2, V.T, cfg["context_dim"])),
            "uc": d(rng.randn(2, V.T, cfg["context_dim"])), "ctx": cfg["context_dim"]}


def pipeline(model, kind):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    return DiffusionPipeline(model, kind, device=DEV)


def composed(model, kind, max_unet_batch=16):
    """The plain pipeline on the test's own host composition of the windowed model."""
    return pipeline(U.HostComposition(model, WIN, STRIDE, max_unet_batch), kind)


# ------------------------------------------------------------------------------------------------ one window: the identity
@pytest.mark.parametrize("kind,param,phi", [("ddim", "eps", 0.0), ("plms", "eps", 0.0), ("dpm_solver", "eps", 0.0),
                                            ("ddim", "v", 0.7)])
def test_a_single_window_is_the_plain_pipeline(tiny, kind, param, phi):
    pipe = pipeline(tiny[param], kind)
    kw = dict(c=tiny["c"], uc=tiny["uc"], H=64, W=64, steps=4, scale=3.0, seeds=[11, 12], guidance_rescale=phi)
    want = pipe(**kw).clone()
    wp = pipe.windowed(window=64)
    got = wp(**kw)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert wp.model.evals == 0 and wp.model.chunks == []          # forwarded: no window launch was made
    assert torch.equal(pipe.windowed(window=128)(**kw), want)       # a window larger than the canvas is the canvas


# ------------------------------------------------------------------------------------------------ one evaluation
@pytest.mark.parametrize("cap,chunks", [(16, [(0, 4)]), (8, [(0, 2), (2, 2)])])
@pytest.mark.parametrize("rows", ["one_temb_row", "temb_per_sample", "timesteps"])
def test_one_evaluation_is_its_composition(tiny, cap, chunks, rows):
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    model = tiny["eps"]
    wm = WindowedDiffusion(model, WIN, STRIDE, max_unet_batch=cap)
    gen = torch.Generator(DEV).manual_seed(29)
    x = torch.randn(2, 4, 8, 20, device=DEV, generator=gen)
    x_in = torch.cat([x, x]).contiguous()                           # canvas latent [2 * 2, 4, 8, 20]
    ctx = torch.cat([tiny["uc"], tiny["c"]]).to(torch.float16).contiguous()
    if rows == "temb_per_sample":
        t = torch.tensor([500., 300., 500., 300.], device=DEV)
        kw = {"temb": model.time_embedding_table(t)}
    else:
        t = torch.full((4,), 500., device=DEV)
        kw = {"temb": model.time_embedding_table(t[:1])[0]} if rows == "one_temb_row" else {}
    before = ops.get_option("unet_cfg_dup_check")
    ops.set_option("unet_cfg_dup_check", 1)
    try:
        got = wm.apply_model_nhwc(x_in, t, ctx, cfg_dup=True, **kw).clone()
        host = U.HostComposition(model, WIN, STRIDE, cap)
        want = host.apply_model_nhwc(x_in, t, ctx, cfg_dup=True, **kw)
    finally:
        ops.set_option("unet_cfg_dup_check", before)
    assert wm.chunks == chunks == host.chunks and wm.evals == 1 and wm.grid.ox == [0, 4, 8, 12]
    assert tuple(got.shape) == (4, 8 * 20, 8) and got.dtype == torch.float16
    print(f"cap {cap} {rows}: max|d| {float((got.float() - want.float()).abs().max()):.3e}")
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert not torch.equal(got[:2], got[2:]) and bool((got[..., 4:] == 0).all())
    # the NCHW form is the same pass behind ops.nhwc_to_nchw
    if rows == "timesteps":
        plain = wm.apply_model_nhwc(x_in, t, ctx).clone()             # (without the guidance-duplicate prefix)
        assert torch.equal(wm.apply_model(x_in, t, ctx), ops.nhwc_to_nchw(plain, 4, 8, 20))
        assert torch.equal(plain, host.apply_model_nhwc(x_in, t, ctx))


# ------------------------------------------------------------------------------------------------ whole runs
@pytest.mark.parametrize("kind,extra", [("ddim", {"eta": 1.0}), ("plms", {}), ("dpm_solver", {})])
def test_a_whole_run_is_its_composition(tiny, kind, extra):
    model = tiny["eps"]
    kw = dict(c=tiny["c"], uc=tiny["uc"], H=64, W=160, steps=4, scale=3.0, seeds=[21, 22], **extra)
    wp = pipeline(model, kind).windowed(window=64)
    got = wp(**kw).clone()
    ref = composed(model, kind)
    want = ref(**kw)
    assert tuple(got.shape) == (2, 4, 8, 20) and wp.model.chunks == [(0, 4)]
    assert wp.model.evals == ref.model.calls >= 4
    print(f"{kind}: max|d| {float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert wp.model.context_refreshes == 1                          # one prompt, one per-window repeat for the whole run


# ------------------------------------------------------------------------------------------------ the neighbours
def test_img2img_with_a_mask_blend_inherits_it(tiny):
    model = tiny["v"]
    gen = torch.Generator(DEV).manual_seed(31)
    z0 = torch.randn(2, 4, 8, 12, device=DEV, generator=gen)
    mask = (torch.rand(2, 1, 8, 12, device=DEV, generator=gen) > 0.5).float()
    kw = dict(init_latent=z0, strength=0.5, mask=mask, c=tiny["c"], uc=tiny["uc"], steps=4, scale=3.0, seeds=[31, 32],
              guidance_rescale=0.7)
    wp = pipeline(model, "ddim").windowed(window=64)
    got = wp.img2img(**kw).clone()
    assert wp.model.chunks == [(0, 2)] and wp.model.evals == 2     # t_enc = 2 of 4 steps on a 64 x 96 canvas
    assert torch.equal(got, composed(model, "ddim").img2img(**kw))


def test_a_session_inherits_it(tiny):
    """A 2-slot session on a 64 x 96 canvas, two requests of different steps: each equals its row of the per-request path on the
    windowed model (the same batch, so the same window batches and plans), as test_session_gpu.py compares."""
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    wp = pipeline(tiny["eps"], "ddim").windowed(window=64)
    steps, scales, seeds = [4, 2], [3.0, 5.0], [41, 42]
    sess = wp.session(slots=2, H=64, W=96, context_len=V.T, max_steps=4)
    handles = [sess.submit(c=tiny["c"][r], uc=tiny["uc"][r], steps=steps[r], scale=scales[r], eta=1.0, seed=seeds[r])
               for r in range(2)]
    sess.run_until_idle()
    assert [h.slot for h in handles] == [0, 1] and sess.unet_evals == 4 == wp.model.evals and wp.model.chunks == [(0, 2)]
    refreshes = wp.model.context_refreshes
    assert 1 <= refreshes <= 2                                       # the admissions' in-place context writes, nothing per tick
    for r, h in enumerate(handles):
        want = DDIMSampler(wp.model).sample([steps[r]] * 2, 2, (4, 8, 12), conditioning=tiny["c"],
                                            unconditional_conditioning=tiny["uc"], seeds=seeds,
                                            unconditional_guidance_scale=scales, eta=1.0, verbose=False)[0][r]
        assert tuple(h.latent.shape) == (4, 8, 12) and torch.equal(h.latent, want), r
    # and the per-request path itself is the composition
    ref = DDIMSampler(U.HostComposition(tiny["eps"], WIN, STRIDE)).sample(
        [4, 4], 2, (4, 8, 12), conditioning=tiny["c"], unconditional_conditioning=tiny["uc"], seeds=seeds,
        unconditional_guidance_scale=scales, eta=1.0, verbose=False)[0][0]
    assert torch.equal(handles[0].latent, ref)


def test_hybrid_inpainting_windows_c_concat_with_x():
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    model = I.tiny_model(DEV)                                       # 9 input channels
    rng = np.random.RandomState(43)
    image = torch.tensor(np.clip(0.5 * rng.randn(2, 3, 16, 24), -1, 1).astype(np.float32))
    mask = torch.zeros(2, 1, 16, 24)
    mask[0, 0, 4:12, 2:19] = 1.0
    mask[1, 0, 6:16, 10:24] = 1.0
    ctx = I.tiny_cfg()["context_dim"]
    c, uc = (torch.tensor(rng.randn(2, I.T, ctx).astype(np.float32), device=DEV) for _ in range(2))
    kw = dict(c=c, uc=uc, steps=4, scale=3.0, seeds=[51, 52], decode=False)
    # (the tiny VAE halves where the SD VAE divides by 8, so the window is given in latent pixels here)
    wp = pipeline(WindowedDiffusion(model, WIN, STRIDE), "plms")
    got = wp.inpaint(image, mask, **kw).clone()
    assert tuple(got.shape) == (2, 4, 8, 12) and wp.model.chunks == [(0, 2)] and wp.model.evals >= 4
    assert wp.model.grid.ox == [0, 4] and wp.model._in_bufs(torch.empty(4, 9, 8, 12, device=DEV), 2)["x"].shape[1] == 9
    assert torch.equal(got, composed(model, "plms").inpaint(image, mask, **kw))


# ------------------------------------------------------------------------------------------------ the context
def test_a_prompt_change_reprojects_the_context_once_per_change(tiny):
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    model = tiny["eps"]
    wm = WindowedDiffusion(model, WIN, STRIDE)
    gen = torch.Generator(DEV).manual_seed(61)
    x = torch.randn(2, 4, 8, 20, device=DEV, generator=gen)
    x_in = torch.cat([x, x]).contiguous()
    t = torch.full((4,), 400., device=DEV)
    ctx = torch.cat([tiny["uc"], tiny["c"]]).to(torch.float16).contiguous()
    host = U.HostComposition(model, WIN, STRIDE)
    first = wm.apply_model_nhwc(x_in, t, ctx, cfg_dup=True).clone()
    plan = model.unet._plans[(16, 8, 8)]
    runs = []
    plan.ctxops.append(lambda: runs.append(1))                      # counts the UNet's context projections from here on
    try:
        again = wm.apply_model_nhwc(x_in, t, ctx, cfg_dup=True).clone()
        assert torch.equal(again, first) and runs == [] and wm.context_refreshes == 1
        ctx[2:] = torch.randn(2, V.T, tiny["ctx"], device=DEV, generator=gen).to(torch.float16)      # in place: a new prompt
        changed = wm.apply_model_nhwc(x_in, t, ctx, cfg_dup=True).clone()
        assert runs == [1] and wm.context_refreshes == 2
        assert torch.equal(wm.apply_model_nhwc(x_in, t, ctx, cfg_dup=True), changed) and runs == [1]
        other = ctx.clone()                                         # another tensor object with the same values: once more
        assert torch.equal(wm.apply_model_nhwc(x_in, t, other, cfg_dup=True), changed)
        assert runs == [1, 1] and wm.context_refreshes == 3
    finally:
        plan.ctxops.pop()
    assert not torch.equal(changed, first)
    assert torch.equal(changed[:2], first[:2])                      # the unconditional half kept its prompt
    assert torch.equal(changed, host.apply_model_nhwc(x_in, t, ctx, cfg_dup=True))
