"""Resampling and hires fix -- the parts that need no GPU: the tap tables of minddiffusion_amd/resample.py against F.interpolate
in float64, their structural properties, the host-side refusals of mdx_resample_f32 / mdx_resample_noised_f32, and the argument
refusals and step accounting of DiffusionPipeline.hires on a stub model (as tests/test_img2img_cpu.py does it)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _resample_util import apply_tables
from minddiffusion_amd import resample as R

# (H_in, W_in) -> (H_out, W_out): non-integer up, x2, x1/2, odd down, same size, mixed
SIZES = [((6, 10), (9, 25)), ((8, 8), (16, 16)), ((16, 12), (8, 6)), ((7, 9), (5, 4)), ((5, 5), (5, 5)), ((12, 20), (7, 33))]
AXES = sorted({(a[k], b[k]) for a, b in SIZES for k in (0, 1)})


def resample64(x, size, mode, antialias):
    H, W = x.shape[-2:]
    return apply_tables(x, *R.tap_table(H, size[0], mode, antialias, dtype=np.float64),
                        *R.tap_table(W, size[1], mode, antialias, dtype=np.float64))


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_tap_tables_are_f_interpolate_in_float64(sizes, mode, antialias):
    a, b = sizes
    x = np.clip(1.5 * np.random.RandomState(5).randn(2, 3, *a), -5.0, 5.0)
    ref = F.interpolate(torch.from_numpy(x), size=b, mode=mode, align_corners=False, antialias=antialias).numpy()
    err = float(np.abs(resample64(x, b, mode, antialias) - ref).max())
    print("TAP_TABLE_VS_TORCH", a, b, mode, antialias, err)
    assert err <= 1e-12


@pytest.mark.parametrize("a,b", [((4, 6), (8, 12)), ((12, 9), (4, 3)), ((5, 5), (15, 5)), ((8, 8), (8, 8))])
def test_nearest_is_torch_nearest_at_integer_ratios(a, b):
    x = np.random.RandomState(6).randn(1, 2, *a)
    ref = F.interpolate(torch.from_numpy(x), size=b, mode="nearest").numpy()
    assert np.array_equal(resample64(x, b, "nearest", False), ref)
    start, w = R.tap_table(7, 5, "nearest")                  # elsewhere: the integer rule, (i * n_in) // n_out
    assert start.tolist() == [0, 1, 2, 4, 5] and w.shape == (5, 1) and bool((w == 1.0).all())


@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("mode", R.MODES)
def test_table_structure(mode, antialias, wrap):
    """fp32 rows sum to 1, at most 32 taps, int32 / float32 arrays, zero padding behind a row's own taps, and the LDS strip
    the kernel sizes from the geometry holds what every 16-row tile reaches."""
    for n_in, n_out in AXES + [(64, 128), (128, 64), (64, 8), (40, 8)]:
        if (mode == "lanczos3" and n_in > 5 * n_out) or (mode == "bicubic" and antialias and n_in >= 8 * n_out):
            continue                                         # more than 32 taps: the refusal has its own test
        start, w = R.tap_table(n_in, n_out, mode, antialias, wrap)
        assert start.dtype == np.int32 and w.dtype == np.float32 and start.shape == (n_out,) and w.shape[0] == n_out
        assert 1 <= w.shape[1] <= R.MAX_TAPS
        assert float(np.abs(w.astype(np.float64).sum(1) - 1.0).max()) <= 1e-6
        assert R.tile_span(start, w.shape[1], n_in) <= R.strip_rows(n_in, n_out, w.shape[1])
        if not wrap:
            assert int(start.max()) <= n_in - 1 and int(start.min()) >= -2
        if n_in == n_out:                                    # the identity: one tap of weight exactly 1
            assert start.tolist() == list(range(n_in)) and w.shape == (n_out, 1) and bool((w == 1.0).all())


def test_lanczos3_weights_are_symmetric_for_symmetric_geometry():
    for n_in, n_out in ((8, 16), (16, 8), (9, 6), (6, 10)):
        for wrap in (False, True):
            start, w = R.tap_table(n_in, n_out, "lanczos3", wrap=wrap, dtype=np.float64)
            T = w.shape[1]
            for i in range(n_out):
                # output i and its mirror image n_out - 1 - i: the mirrored taps carry the same weights
                dense = lambda j: {int(start[j]) + k: w[j, k] for k in range(T) if w[j, k] != 0.0}
                a, b = dense(i), dense(n_out - 1 - i)
                assert sorted(a) == sorted(n_in - 1 - k for k in b)
                assert max(abs(a[k] - b[n_in - 1 - k]) for k in a) <= 1e-14
    # fp32 tables of the x2 case: the two phases are mirror images, bit for bit, away from the edges
    start, w = R.tap_table(8, 16, "lanczos3")
    assert np.array_equal(w[6], w[7][::-1])


def test_wrap_keeps_the_full_support():
    """No tap is truncated or clamped: every row has the interior's weights, and the indices run past both ends."""
    for mode, aa in (("bilinear", False), ("bicubic", False), ("bicubic", True), ("lanczos3", True)):
        start, w = R.tap_table(8, 16, mode, aa, wrap=True, dtype=np.float64)
        assert int(start.min()) < 0 and int((start + w.shape[1] - 1).max()) > 7
        assert np.allclose(w[0], w[2], rtol=0, atol=1e-15) and np.allclose(w[1], w[15], rtol=0, atol=1e-15)
        # integer scale: rolling the input by k rolls the output by 2 k, in float64 to rounding
        x = np.random.RandomState(7).randn(1, 1, 4, 8)
        ys, yw = R.tap_table(4, 4, mode, aa, dtype=np.float64)
        out = apply_tables(x, ys, yw, start, w, wrap_x=True)
        rolled = apply_tables(np.roll(x, 3, -1), ys, yw, start, w, wrap_x=True)
        assert float(np.abs(rolled - np.roll(out, 6, -1)).max()) <= 1e-14


def test_too_many_taps_and_bad_arguments_are_refused():
    with pytest.raises(ValueError, match="taps"):
        R.tap_table(128, 8, "bicubic", antialias=True)       # x1/16: 4 * 16 + 1 taps
    with pytest.raises(ValueError, match="taps"):
        R.tap_table(96, 16, "lanczos3")                       # x1/6: 37 taps
    R.tap_table(128, 17, "bicubic", antialias=True)           # just above x1/8 fits
    R.tap_table(80, 16, "lanczos3")                           # x1/5 fits
    with pytest.raises(ValueError, match="mode"):
        R.tap_table(8, 16, "area")
    with pytest.raises(ValueError, match="positive"):
        R.tap_table(0, 16, "bicubic")


# ------------------------------------------------------------------------------------------------ the C entries' host-side refusals
def test_resample_argument_validation_without_gpu():
    """Every refusal of mdx_resample_f32 / mdx_resample_noised_f32 happens on the host, before any launch (code + message)."""
    from minddiffusion_amd import _lib
    lib = _lib.load()
    P = 1 << 20                              # disjoint non-null addresses: nothing is dereferenced
    IN, OUT, YS, YW, XS, XW, NZ, SD, Z0, XT = (P * (k + 1) for k in range(10))

    def plain(inp=IN, out=OUT, B=2, C=4, Hi=8, Wi=8, Ho=16, Wo=16, ys=YS, yw=YW, Ty=4, xs=XS, xw=XW, Tx=4, wrap=0):
        return lib.mdx_resample_f32(inp, out, B, C, Hi, Wi, Ho, Wo, ys, yw, Ty, xs, xw, Tx, wrap, None)

    def noised(inp=IN, B=2, C=4, Hi=8, Wi=8, Ho=16, Wo=16, Ty=4, Tx=4, noise=NZ, seeds=None, z0=Z0, xt=XT):
        return lib.mdx_resample_noised_f32(inp, B, C, Hi, Wi, Ho, Wo, YS, YW, Ty, XS, XW, Tx, 0, 0.5, 0.8, 0.6, noise, seeds, 3, 0,
                                           z0, xt, None)

    def refused(call, name, msg, **kw):
        assert call(**kw) == -1
        err = lib.mdx_last_error()
        assert name in err and msg in err, err

    for kw in (dict(inp=None), dict(out=None), dict(ys=None), dict(yw=None), dict(xs=None), dict(xw=None)):
        refused(plain, b"mdx_resample_f32", b"null pointer", **kw)
    for kw in (dict(B=0), dict(C=-1), dict(Hi=0), dict(Wi=0), dict(Ho=0), dict(Wo=-4), dict(B=20000, C=4)):
        refused(plain, b"mdx_resample_f32", b"bad extents", **kw)
    for kw in (dict(Tx=0), dict(Tx=33), dict(Ty=0), dict(Ty=33)):
        refused(plain, b"mdx_resample_f32", b"must be in [1, 32]", **kw)
    refused(plain, b"mdx_resample_f32", b"out overlaps in", out=IN + 64)
    refused(plain, b"mdx_resample_f32", b"out overlaps in", inp=OUT + 2 * 4 * 16 * 16 * 4 - 4)
    refused(plain, b"mdx_resample_f32", b"very large downscale", Hi=2100, Ho=100, Ty=1)
    refused(noised, b"mdx_resample_noised_f32", b"null pointer", inp=None)
    refused(noised, b"mdx_resample_noised_f32", b"bad extents", Ho=0)
    refused(noised, b"mdx_resample_noised_f32", b"must be in [1, 32]", Tx=40)
    refused(noised, b"mdx_resample_noised_f32", b"no output", z0=None, xt=None)
    refused(noised, b"mdx_resample_noised_f32", b"needs a noise source", noise=None)
    refused(noised, b"mdx_resample_noised_f32", b"overlaps in", z0=IN)
    refused(noised, b"mdx_resample_noised_f32", b"overlaps in", xt=IN + 16)
    refused(noised, b"mdx_resample_noised_f32", b"different tensors", z0=XT + 32)
    refused(noised, b"mdx_resample_noised_f32", b"overlaps noise", xt=NZ)
    refused(noised, b"mdx_resample_noised_f32", b"very large downscale", Hi=2100, Ho=100, Ty=1)


# ------------------------------------------------------------------------------------------------ DiffusionPipeline.hires on a stub
def _ldm(**kw):
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    return LatentDiffusion(object(), linear_start=0.00085, linear_end=0.0120, timesteps=1000, **kw)


def _pipe(sampler="ddim"):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    return DiffusionPipeline(_ldm(), sampler, device="cpu")


def test_hires_refusals(monkeypatch):
    from minddiffusion_amd import distributed
    from minddiffusion_amd._lib import MdxError
    c = torch.zeros(1, 7, 64)
    for sampler in ("ddim", "plms", "dpm_solver"):
        p = _pipe(sampler)
        for bad in (0.0, -0.1, 1.01, float("nan")):
            with pytest.raises(ValueError, match="strength"):
                p.hires(c=c, strength=bad)
        with pytest.raises(ValueError, match="strength"):
            p.hires(c=c, strength=0.01, steps=50)                         # t_enc = int(0.5) = 0
        with pytest.raises(ValueError, match="strength"):
            p.hires(c=c, strength=0.3, steps=50, hires_steps=3)           # t_enc = int(0.9) = 0: hires_steps counts
        with pytest.raises(ValueError, match="hires_steps"):
            p.hires(c=c, hires_steps=0)
        for kw in (dict(H=1020), dict(W=4), dict(base=(500, 512)), dict(base=(512, 0))):
            with pytest.raises(MdxError, match="multiples of 8"):
                p.hires(c=c, **kw)
        with pytest.raises(MdxError, match="pair"):
            p.hires(c=c, base=512)
        with pytest.raises(ValueError, match="upscaler"):
            p.hires(c=c, upscaler="esrgan")
        with pytest.raises(ValueError, match="guidance_rescale"):
            p.hires(c=c, guidance_rescale=1.5)
        with pytest.raises(ValueError, match="one int"):
            p.hires(c=c, steps=[10])
        with pytest.raises(MdxError, match="prompts"):
            p.hires()
        with pytest.raises(MdxError, match="regions= needs a windowed pipeline"):
            p.hires(c=c, H=512, W=512, regions=[{"c": c, "mask": torch.ones(64, 64)}])
        with pytest.raises(MdxError, match="multiples of 8"):
            p.upscale_latent(torch.zeros(1, 4, 8, 8), 100, 128)
    hybrid = _pipe()
    hybrid.model.model.conditioning_key = "hybrid"
    with pytest.raises(MdxError, match="hybrid"):
        hybrid.hires(c=c)
    monkeypatch.setattr(distributed, "world", lambda: (0, 2))
    with pytest.raises(MdxError, match="single rank"):
        _pipe().hires(c=c)


def _count_runs(monkeypatch, pipe_cls):
    """Stand-ins for the three device stages: every sampler run is logged as (the model it ran on, evaluations, latent shape)."""
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import _SamplerBase
    log = []

    def sample(self, S, batch_size, shape, x_T=None, t_start=None, **kw):
        log.append((self.model, "partial" if t_start is not None else "full", int(S), (batch_size,) + tuple(shape)))
        return torch.zeros(batch_size, *shape), {}

    def decode(self, x_latent, cond, t_start, **kw):
        log.append((self.model, "partial", int(t_start), tuple(x_latent.shape)))
        return torch.zeros_like(x_latent), {}
    monkeypatch.setattr(_SamplerBase, "sample", sample)
    monkeypatch.setattr(DPMSolverSampler, "sample", sample)
    monkeypatch.setattr(_SamplerBase, "decode", decode)
    monkeypatch.setattr(_SamplerBase, "stochastic_encode", lambda self, x0, t, noise=None, **kw: x0)
    monkeypatch.setattr(DPMSolverSampler, "stochastic_encode", lambda self, x0, t, noise=None, **kw: x0)
    monkeypatch.setattr(ops, "resample", lambda x, size, mode="bicubic", antialias=None, wrap_x=False, out=None:
                        (log.append(("resample", tuple(x.shape), tuple(size), mode, wrap_x)),
                         torch.zeros(x.shape[0], x.shape[1], *size))[1])
    return log


@pytest.mark.parametrize("sampler", ["ddim", "plms", "dpm_solver"])
@pytest.mark.parametrize("strength,steps,hires_steps,t_enc", [(0.6, 50, None, 30), (0.5, 4, None, 2), (0.75, 20, 10, 7),
                                                               (1.0, 5, 8, 8)])
def test_hires_step_accounting_and_the_default_second_pipeline(monkeypatch, sampler, strength, steps, hires_steps, t_enc):
    """`steps` evaluations at the base size, the latent resampled once, then t_enc = int(strength * (hires_steps or steps)) at
    the target size, on self.windowed(window=base) -- built once and kept -- when the target is larger than the base."""
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    from minddiffusion_amd.pipeline import DiffusionPipeline
    log = _count_runs(monkeypatch, DiffusionPipeline)
    p = _pipe(sampler)
    c = torch.zeros(2, 7, 64)
    out, zb = p.hires(c=c, H=128, W=192, base=(64, 96), upscaler="latent-bilinear", strength=strength, steps=steps,
                      hires_steps=hires_steps, return_base=True)
    assert tuple(zb.shape) == (2, 4, 8, 12) and tuple(out.shape) == (2, 4, 16, 24)
    first, up, second = log
    assert first == (p.model, "full", steps, (2, 4, 8, 12))
    assert up == ("resample", (2, 4, 8, 12), (16, 24), "bilinear", False)
    assert isinstance(second[0], WindowedDiffusion) and second[0].inner is p.model and second[0].window == (8, 12)
    assert second[1:] == ("partial", t_enc, (2, 4, 16, 24))
    kept = second[0]
    del log[:]
    p.hires(c=c, H=128, W=192, base=(64, 96), strength=strength, steps=steps, hires_steps=hires_steps)
    assert log[2][0] is kept                                             # the windowed pipeline of a base is built once


def test_hires_second_pipeline_choices(monkeypatch):
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    from minddiffusion_amd.pipeline import DiffusionPipeline
    log = _count_runs(monkeypatch, DiffusionPipeline)
    c = torch.zeros(1, 7, 64)
    p = _pipe()
    # the target is the base size: the pipeline itself runs both passes
    p.hires(c=c, H=64, W=64, base=(64, 64), steps=4, strength=0.5)
    assert [r[0] for r in log] == [p.model, "resample", p.model] and log[1][1:3] == ((1, 4, 8, 8), (8, 8))
    # a windowed pipeline: the first pass on its inner model, the second on itself; its wrap_x reaches the upscale
    del log[:]
    w = p.windowed(window=64, wrap_x=True)
    w.hires(c=c, H=64, W=256, base=(64, 128), steps=4, strength=0.5, upscaler="latent-nearest")
    assert log[0] == (p.model, "full", 4, (1, 4, 8, 16))
    assert log[1] == ("resample", (1, 4, 8, 16), (8, 32), "nearest", True)
    assert log[2] == (w.model, "partial", 2, (1, 4, 8, 32)) and isinstance(w.model, WindowedDiffusion)
    # an explicit second pipeline wins
    del log[:]
    other = _pipe()
    p.hires(c=c, H=128, W=128, base=(64, 64), steps=4, strength=0.5, second=other)
    assert log[2][0] is other.model
    # upscale_latent: one resample to the latent grid of the image size, wrap_x from the pipeline
    del log[:]
    assert tuple(w.upscale_latent(torch.zeros(1, 4, 8, 16), 64, 256, mode="bilinear").shape) == (1, 4, 8, 32)
    assert log == [("resample", (1, 4, 8, 16), (8, 32), "bilinear", True)]
