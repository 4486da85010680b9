"""WindowedDiffusion with wrap-around windows and with regions, end to end on the GPU, on the tiny UNet with 8 x 8 latent windows.
No tolerance anywhere.  A wrapped evaluation must be torch.equal to the composition the test makes itself from the inner model
(_window_regions_util.HostComposition: torch.roll plus slicing, the inner model on the same batch sizes, the numpy restatement
of the average on the CPU), per call and over whole sampler runs.  A region evaluation is held to the same composition with
the average done by ops.window_average_regions -- that isolates the wrapper's gather and context plumbing; the kernel's
arithmetic is tested in test_window_regions_kernels_gpu.py -- and a region's prompt must reach only its pixels."""
import numpy as np
import pytest
import torch

import _inpaint_util as I
import _vpred_util as V
import _window_regions_util as RU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIN, STRIDE = (8, 8), (4, 4)


@pytest.fixture(scope="module")
def tiny():
    eps_model, cfg, _ = V.tiny_eps_model()
    rng = np.random.RandomState(547)
    d = lambda a: torch.tensor(a.astype(np.float32), device=DEV)
    shape = (2, V.T, cfg["context_dim"])
    return {"eps": eps_model, "c": d(rng.randn(*shape)), "uc": d(rng.randn(*shape)), "cb": d(rng.randn(*shape)),
            "cc": d(rng.randn(*shape)), "ctx": cfg["context_dim"]}


def pipeline(model, kind):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    return DiffusionPipeline(model, kind, device=DEV)


def region_average(weights=None):
    """The average of a region HostComposition: ops.window_average_regions on a grid and a plan of the test's own."""
    from minddiffusion_amd import ops

    def average(win, host, canvas_hw, window_hw):
        g = ops.WindowGrid(canvas_hw, window_hw, STRIDE, wrap_x=host.wrap and canvas_hw[1] > window_hw[1])
        plan = ops.RegionPlan(g, host.masks)
        assert plan.pairs == host.pairs
        return ops.window_average_regions(win, g, int(host.inner.unet.final_channels), plan=plan, weights=weights)
    return average


def canvas_inputs(shape, seed):
    """(x_in [2b, C, Hc, Wc] with equal halves, t) of a guidance batch."""
    x = torch.randn((shape[0] // 2,) + tuple(shape[1:]), device=DEV, generator=torch.Generator(DEV).manual_seed(seed))
    return torch.cat([x, x]).contiguous(), torch.full((shape[0],), 500., device=DEV)


def left_right(Hc, Wc):
    m = np.zeros((2, Hc, Wc), np.float32)
    m[0, :, :Wc // 2] = 1.0
    m[1, :, Wc // 2:] = 1.0
    return m


def guided_ctx(tiny, name):
    return torch.cat([tiny["uc"], tiny[name]]).to(torch.float16).contiguous()


# ------------------------------------------------------------------------------------------------ one wrapped evaluation
@pytest.mark.parametrize("shape,cap,chunks", [((2, 4, 8, 32), 16, [(0, 8)]), ((2, 4, 8, 32), 8, [(0, 4), (4, 4)]),
                                              ((4, 4, 16, 24), 16, [(0, 4), (4, 4), (8, 4), (12, 4), (16, 2)])])
def test_one_wrapped_evaluation_is_its_composition(tiny, shape, cap, chunks):
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    model = tiny["eps"]
    wm = WindowedDiffusion(model, WIN, STRIDE, max_unet_batch=cap, wrap_x=True)
    x_in, t = canvas_inputs(shape, 29)
    half = shape[0] // 2
    ctx = torch.cat([tiny["uc"][:half], tiny["c"][:half]]).to(torch.float16).contiguous()
    temb = model.time_embedding_table(t[:1])[0]
    got = wm.apply_model_nhwc(x_in, t, ctx, temb=temb, cfg_dup=True).clone()
    host = RU.HostComposition(model, WIN, STRIDE, cap, wrap_x=True)
    want = host.apply_model_nhwc(x_in, t, ctx, temb=temb, cfg_dup=True)
    assert wm.chunks == chunks == host.chunks and wm.evals == 1 and wm.grid.wrap_x
    assert wm.grid.ox == list(range(0, shape[3], 4)) and wm.pairs == host.pairs == [(k, None) for k in range(wm.grid.N)]
    assert tuple(got.shape) == (shape[0], shape[2] * shape[3], 8) and got.dtype == torch.float16
    print(f"{shape} cap {cap}: max|d| {float((got.float() - want.float()).abs().max()):.3e}")
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert not torch.equal(got[:half], got[half:]) and bool((got[..., 4:] == 0).all())
    # the wrap is seen: the clamped grid gives another result at the seam
    plain = WindowedDiffusion(model, WIN, STRIDE, max_unet_batch=cap).apply_model_nhwc(x_in, t, ctx, temb=temb, cfg_dup=True)
    assert not torch.equal(plain, got)


# ------------------------------------------------------------------------------------------------ one region evaluation
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape,wrap,cap,npairs,nchunks", [((2, 4, 8, 32), True, 16, 8 + 8 + 5, 3),
                                                            ((2, 4, 8, 32), False, 64, 7 + 7 + 4, 1),
                                                            ((4, 4, 16, 24), True, 16, 18 + 18 + 12, 12)])
def test_one_region_evaluation_is_its_composition(tiny, shape, wrap, cap, npairs, nchunks, weighted):
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion, gaussian_weights
    model = tiny["eps"]
    wts = gaussian_weights(8, 8) if weighted else None
    wm = WindowedDiffusion(model, WIN, STRIDE, weights=wts, max_unet_batch=cap, wrap_x=wrap)
    x_in, t = canvas_inputs(shape, 31)
    half = shape[0] // 2
    ctxs = [torch.cat([tiny["uc"][:half], tiny[k][:half]]).to(torch.float16).contiguous() for k in ("c", "cb", "cc")]
    masks = RU.region_masks("ramp", shape[2], shape[3])
    masks[2, :, shape[3] // 2:] = 0.0                                 # the third region touches the left windows only
    with wm.regions(torch.from_numpy(masks), ctxs):
        got = wm.apply_model_nhwc(x_in, t, ctxs[0], cfg_dup=True).clone()
    host = RU.HostComposition(model, WIN, STRIDE, cap, wrap_x=wrap, masks=masks, contexts=ctxs,
                              region_average=region_average(None if wts is None else wts.to(DEV)))
    want = host.apply_model_nhwc(x_in, t, ctxs[0], cfg_dup=True)
    assert wm.pairs == host.pairs and wm.chunks == host.chunks and len(wm.chunks) == nchunks and wm.evals == 1
    assert len(wm.pairs) == npairs < 3 * wm.grid.N                    # pruned: not every window holds every region
    assert torch.equal(got, want) and bool(torch.isfinite(got).all()) and bool((got[..., 4:] == 0).all())


def test_a_regions_prompt_reaches_only_its_pixels(tiny):
    """Binary left / right masks: the left pixels are the windowed evaluation with context A alone, the right ones the one with
    B alone, bit for bit.  (One pair per UNet batch in all three runs, so the UNet's launch plans are the same.)"""
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    model = tiny["eps"]
    wm = WindowedDiffusion(model, WIN, STRIDE, max_unet_batch=2, wrap_x=True)
    x_in, t = canvas_inputs((2, 4, 8, 32), 37)
    a, b = guided_ctx(tiny, "c")[1::2].contiguous(), guided_ctx(tiny, "cb")[1::2].contiguous()     # rows [uc_1 ; c_1]
    only_a = wm.apply_model_nhwc(x_in, t, a).clone()
    only_b = wm.apply_model_nhwc(x_in, t, b).clone()
    with wm.regions(torch.from_numpy(left_right(8, 32)), [a, b]):
        both = wm.apply_model_nhwc(x_in, t, a).clone()
    # windows at 0 4 8 hold A only, 12 and (wrapped) 28 both, 16 20 24 B only
    assert wm.pairs == [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (4, 1), (5, 1), (6, 1), (7, 0), (7, 1)]
    assert len(wm.chunks) == 10
    left = torch.zeros(8, 32, dtype=torch.bool, device=DEV)
    left[:, :16] = True
    left = left.reshape(-1)
    assert torch.equal(both[:, left], only_a[:, left]) and torch.equal(both[:, ~left], only_b[:, ~left])
    assert not torch.equal(only_a[1], only_b[1]) and bool(torch.isfinite(both).all())


# ------------------------------------------------------------------------------------------------ whole runs
@pytest.mark.parametrize("kind,extra", [("ddim", {"eta": 1.0}), ("dpm_solver", {})])
def test_a_whole_wrapped_run_is_its_composition(tiny, kind, extra):
    model = tiny["eps"]
    kw = dict(c=tiny["c"], uc=tiny["uc"], H=64, W=256, steps=4, scale=3.0, seeds=[21, 22], **extra)
    wp = pipeline(model, kind).windowed(window=64, wrap_x=True)
    got = wp(**kw).clone()
    ref = pipeline(RU.HostComposition(model, WIN, STRIDE, wrap_x=True), kind)
    want = ref(**kw)
    assert tuple(got.shape) == (2, 4, 8, 32) and wp.model.chunks == [(0, 4), (4, 4)] and wp.model.grid.wrap_x
    assert wp.model.evals == ref.model.calls >= 4
    print(f"{kind}: max|d| {float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert wp.model.context_refreshes == 1                          # one prompt, one per-window repeat for the whole run


@pytest.mark.parametrize("kind,scale", [("plms", 3.0), ("ddim", 1.0)])
def test_a_whole_region_run_is_its_composition(tiny, kind, scale):
    """PLMS with two regions under guidance; DDIM with scale 1: no unconditional half, the contexts are the c_r alone."""
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model = tiny["eps"]
    m = torch.zeros(8, 24)
    m[:, 10:20] = 1.0
    m[2:6, 20:] = 0.5
    kw = dict(c=tiny["c"], uc=tiny["uc"], H=64, W=192, steps=4, scale=scale, seeds=[23, 24])
    wp = pipeline(model, kind).windowed(window=64, wrap_x=True)
    got = wp(regions=[{"c": tiny["cb"], "mask": m}], **kw).clone()
    assert wp.model._regions is None and wp.model.grid.wrap_x
    masks = DiffusionPipeline.background_mask(m[None]).numpy()
    ctxs = [guided_ctx(tiny, k) if scale != 1.0 else tiny[k].to(torch.float16).contiguous() for k in ("c", "cb")]
    ref = pipeline(RU.HostComposition(model, WIN, STRIDE, wrap_x=True, masks=masks, contexts=ctxs,
                                      region_average=region_average()), kind)
    want = ref(**kw)
    assert wp.model.pairs == ref.model.pairs and wp.model.chunks == ref.model.chunks
    assert 6 < len(wp.model.pairs) < 12 and wp.model.evals == ref.model.calls >= 4
    assert tuple(ctxs[0].shape)[0] == (4 if scale != 1.0 else 2)
    print(f"{kind} scale {scale}: max|d| {float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert not torch.equal(got, wp(**kw))                           # the region's prompt is seen


# ------------------------------------------------------------------------------------------------ the neighbours
def test_img2img_with_a_mask_blend_inherits_the_wrap(tiny):
    model = tiny["eps"]
    gen = torch.Generator(DEV).manual_seed(31)
    z0 = torch.randn(2, 4, 8, 24, device=DEV, generator=gen)
    mask = (torch.rand(2, 1, 8, 24, device=DEV, generator=gen) > 0.5).float()
    kw = dict(init_latent=z0, strength=0.5, mask=mask, c=tiny["c"], uc=tiny["uc"], steps=4, scale=3.0, seeds=[31, 32])
    wp = pipeline(model, "ddim").windowed(window=64, wrap_x=True)
    got = wp.img2img(**kw).clone()
    assert wp.model.chunks == [(0, 4), (4, 2)] and wp.model.evals == 2 and wp.model.grid.ox == [0, 4, 8, 12, 16, 20]
    assert torch.equal(got, pipeline(RU.HostComposition(model, WIN, STRIDE, wrap_x=True), "ddim").img2img(**kw))


def test_a_session_inherits_the_wrap(tiny):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    wp = pipeline(tiny["eps"], "ddim").windowed(window=64, wrap_x=True)
    steps, scales, seeds = [4, 2], [3.0, 5.0], [41, 42]
    sess = wp.session(slots=2, H=64, W=192, context_len=V.T, max_steps=4)
    handles = [sess.submit(c=tiny["c"][r], uc=tiny["uc"][r], steps=steps[r], scale=scales[r], eta=1.0, seed=seeds[r])
               for r in range(2)]
    sess.run_until_idle()
    assert sess.unet_evals == 4 == wp.model.evals and wp.model.chunks == [(0, 4), (4, 2)] and wp.model.grid.wrap_x
    for r, h in enumerate(handles):
        want = DDIMSampler(wp.model).sample([steps[r]] * 2, 2, (4, 8, 24), conditioning=tiny["c"],
                                            unconditional_conditioning=tiny["uc"], seeds=seeds,
                                            unconditional_guidance_scale=scales, eta=1.0, verbose=False)[0][r]
        assert tuple(h.latent.shape) == (4, 8, 24) and torch.equal(h.latent, want), r
    ref = DDIMSampler(RU.HostComposition(tiny["eps"], WIN, STRIDE, wrap_x=True)).sample(
        [4, 4], 2, (4, 8, 24), conditioning=tiny["c"], unconditional_conditioning=tiny["uc"], seeds=seeds,
        unconditional_guidance_scale=scales, eta=1.0, verbose=False)[0][0]
    assert torch.equal(handles[0].latent, ref)


def test_hybrid_inpainting_inherits_the_wrap_and_wrap_decode_is_pad_decode_crop():
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    model = I.tiny_model(DEV)                                       # 9 input channels, the tiny VAE attached
    rng = np.random.RandomState(43)
    image = torch.tensor(np.clip(0.5 * rng.randn(2, 3, 16, 48), -1, 1).astype(np.float32))
    mask = torch.zeros(2, 1, 16, 48)
    mask[0, 0, 4:12, 2:30] = 1.0
    mask[1, 0, 6:16, 20:48] = 1.0
    ctx = I.tiny_cfg()["context_dim"]
    c, uc = (torch.tensor(rng.randn(2, I.T, ctx).astype(np.float32), device=DEV) for _ in range(2))
    kw = dict(c=c, uc=uc, steps=4, scale=3.0, seeds=[51, 52], decode=False)
    # (the tiny VAE halves where the SD VAE divides by 8, so the window is given in latent pixels here)
    wp = pipeline(WindowedDiffusion(model, WIN, STRIDE, wrap_x=True), "plms")
    got = wp.inpaint(image, mask, **kw).clone()
    assert tuple(got.shape) == (2, 4, 8, 24) and wp.model.chunks == [(0, 4), (4, 2)] and wp.model.grid.wrap_x
    assert torch.equal(got, pipeline(RU.HostComposition(model, WIN, STRIDE, wrap_x=True), "plms").inpaint(image, mask, **kw))
    # the decoder at the seam: pad the latent circularly, decode, crop the padded image columns (the tiny VAE's factor is 2)
    plain = pipeline(model, "plms")
    wp = plain.windowed(window=64, wrap_x=True, seam_pad=16)
    assert wp.seam_cols == 2
    padded = torch.cat([got[..., -2:], got, got[..., :2]], -1).contiguous()
    want = torch.clamp((model.decode_first_stage(padded)[..., 4:-4] + 1.0) / 2.0, 0.0, 1.0)
    img = wp._decoded(got)
    assert tuple(img.shape) == (2, 3, 16, 48) and torch.equal(img, want)
    flat = plain._decoded(got)
    assert torch.equal(plain.windowed(window=64, wrap_x=True, seam_pad=0)._decoded(got), flat)
    assert torch.equal(plain.windowed(window=64, seam_pad=16)._decoded(got), flat)      # no wrap: no padding
    assert not torch.equal(img, flat) and bool(torch.isfinite(img).all())
    # inpaint(decode=True) goes through the same decode
    out = wp.inpaint(image, mask, composite=False, **dict(kw, decode=True))
    assert tuple(out.shape) == (2, 3, 16, 48) and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------ the contexts
def test_a_regions_prompt_change_reprojects_once_and_an_unchanged_one_does_not(tiny):
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    model = tiny["eps"]
    wm = WindowedDiffusion(model, WIN, STRIDE, max_unet_batch=32, wrap_x=True)
    x_in, t = canvas_inputs((4, 4, 8, 20), 61)
    a, b = guided_ctx(tiny, "c"), guided_ctx(tiny, "cb")
    masks = torch.from_numpy(left_right(8, 20))
    gen = torch.Generator(DEV).manual_seed(62)
    with wm.regions(masks, [a, b]):
        first = wm.apply_model_nhwc(x_in, t, a, cfg_dup=True).clone()
        assert len(wm.chunks) == 1 and wm.context_refreshes == 1 and len(wm.pairs) == 8
        plan = model.unet._plans[(4 * 8, 8, 8)]
        runs = []
        plan.ctxops.append(lambda: runs.append(1))                  # counts the UNet's context projections from here on
        try:
            again = wm.apply_model_nhwc(x_in, t, a, cfg_dup=True).clone()
            assert torch.equal(again, first) and runs == [] and wm.context_refreshes == 1
            b[2:] = torch.randn(2, V.T, tiny["ctx"], device=DEV, generator=gen).to(torch.float16)    # in place: a new prompt
            changed = wm.apply_model_nhwc(x_in, t, a, cfg_dup=True).clone()
            assert runs == [1] and wm.context_refreshes == 2
            assert torch.equal(wm.apply_model_nhwc(x_in, t, a, cfg_dup=True), changed) and runs == [1]
        finally:
            plan.ctxops.pop()
        assert not torch.equal(changed, first) and torch.equal(changed[:2], first[:2])     # the unconditional half kept its prompt
        left = torch.zeros(8, 20, dtype=torch.bool, device=DEV)
        left[:, :10] = True
        assert torch.equal(changed[:, left.reshape(-1)], first[:, left.reshape(-1)])       # and so did region A's pixels
        # a call that does not fit the regions
        for bad in (a[:2].contiguous(), a.float(), a[:, :3].contiguous(), None):
            with pytest.raises(MdxError, match="the call's cond"):
                wm.apply_model_nhwc(x_in, t, bad)
        with pytest.raises(MdxError, match="the masks are for a 8x20 canvas"):
            wm.apply_model_nhwc(torch.zeros(4, 4, 8, 24, device=DEV), t, a)
        with pytest.raises(MdxError, match="already inside"):
            with wm.regions(masks, [a, b]):
                pass
    assert wm._regions is None


def test_outside_the_block_the_wrapper_is_the_one_without_the_new_arguments(tiny):
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    model = tiny["eps"]
    x_in, t = canvas_inputs((4, 4, 8, 20), 71)
    ctx = guided_ctx(tiny, "c")
    want = WindowedDiffusion(model, WIN, STRIDE).apply_model_nhwc(x_in, t, ctx, cfg_dup=True).clone()
    wm = WindowedDiffusion(model, WIN, STRIDE, wrap_x=False)
    with wm.regions(torch.from_numpy(left_right(8, 20)), [ctx, guided_ctx(tiny, "cb")]):
        inside = wm.apply_model_nhwc(x_in, t, ctx, cfg_dup=True).clone()
    got = wm.apply_model_nhwc(x_in, t, ctx, cfg_dup=True)
    assert torch.equal(got, want) and not torch.equal(inside, want) and wm.chunks == [(0, 4)] and wm.evals == 2
    # N == 1 still forwards, bit for bit, with wrap_x too
    x1, t1 = canvas_inputs((4, 4, 8, 8), 72)
    w1 = WindowedDiffusion(model, WIN, STRIDE, wrap_x=True)
    assert torch.equal(w1.apply_model_nhwc(x1, t1, ctx, cfg_dup=True), model.apply_model_nhwc(x1, t1, ctx, cfg_dup=True))
    assert w1.evals == 0
