"""Windowed UNet evaluation -- the parts that need no GPU: the window grid and its coverage, the chunk lists, every refusal of
the two entries of csrc/window.hip (on the host, before any launch), of WindowedDiffusion and of DiffusionPipeline.windowed,
the C declarations against include/mdx.h, and the numpy restatement the GPU tests compare against (tests/_window_util.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _window_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20         # disjoint non-null addresses P, 2P, ...: nothing is dereferenced by a refused call


# ------------------------------------------------------------------------------------------------ the grid
def test_window_offsets():
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion import windowed
    assert windowed.window_offsets is ops.window_offsets
    assert ops.window_offsets(20, 8, 4) == [0, 4, 8, 12]
    assert ops.window_offsets(18, 8, 4) == [0, 4, 8, 10]            # the last window is clamped, not padded
    assert ops.window_offsets(8, 8, 4) == [0]
    assert ops.window_offsets(256, 64, 32) == [0, 32, 64, 96, 128, 160, 192]      # the panorama of the design note: 7 windows
    assert ops.window_offsets(9, 8, 8) == [0, 1]
    for bad in ((7, 8, 4), (8, 0, 1), (20, 8, 9), (20, 8, 0)):
        with pytest.raises(MdxError, match="window_offsets"):
            ops.window_offsets(*bad)


def test_every_pixel_is_covered_and_the_counts_are_the_hand_computed_ones():
    from minddiffusion_amd import ops
    g = ops.WindowGrid((8, 20), (8, 8), (4, 4))
    assert (g.ny, g.nx, g.N) == (1, 4, 4) and g.host.dtype == np.int32 and g.host.tolist() == [0, 0, 4, 8, 12]
    assert g.coverage()[0].tolist() == [1] * 4 + [2] * 12 + [1] * 4 and np.array_equal(g.coverage(), np.tile(g.coverage()[0], (8, 1)))
    g = ops.WindowGrid((8, 18), (8, 8), (4, 4))                     # offsets 0 4 8 10: columns 10, 11 lie under three windows
    assert g.coverage()[0].tolist() == [1] * 4 + [2] * 6 + [3] * 2 + [2] * 4 + [1] * 2
    g = ops.WindowGrid((12, 20), (8, 8), (4, 4))
    assert (g.ny, g.nx) == (2, 4) and [g.origin(k) for k in (0, 3, 4, 7)] == [(0, 0), (0, 12), (4, 0), (4, 12)]
    rows, cols = np.array([1] * 4 + [2] * 4 + [1] * 4), np.array([1] * 4 + [2] * 12 + [1] * 4)
    assert np.array_equal(g.coverage(), rows[:, None] * cols[None, :])
    for canvas, win, stride in (((8, 20), (8, 8), (4, 4)), ((13, 29), (8, 8), (3, 5)), ((64, 256), (64, 64), (32, 32))):
        g = ops.WindowGrid(canvas, win, stride)
        cov = np.zeros(canvas, np.int64)
        for k in range(g.N):
            oy, ox = g.origin(k)
            assert 0 <= oy <= canvas[0] - win[0] and 0 <= ox <= canvas[1] - win[1]
            cov[oy:oy + win[0], ox:ox + win[1]] += 1
        assert cov.min() >= 1 and np.array_equal(cov, g.coverage())


@pytest.mark.parametrize("NB", [2, 4, 6])
def test_chunks_partition_the_windows_in_order_under_the_cap(NB):
    from minddiffusion_amd.ldm.models.diffusion.windowed import chunk_list
    for N in (1, 2, 7, 8, 21):
        chunks = chunk_list(N, NB, 16)
        assert [k for k0, n in chunks for k in range(k0, k0 + n)] == list(range(N))
        assert all(1 <= n and NB * n <= 16 for _, n in chunks)
        assert all(n == 16 // NB for _, n in chunks[:-1])            # only the last chunk may be short
    assert chunk_list(7, 2, 16) == [(0, 7)] and chunk_list(7, 4, 16) == [(0, 4), (4, 3)]
    assert chunk_list(7, 6, 16) == [(0, 2), (2, 2), (4, 2), (6, 1)]


def test_a_canvas_batch_above_the_cap_is_refused():
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.windowed import chunk_list
    with pytest.raises(MdxError, match="max_unet_batch"):
        chunk_list(7, 18, 16)


# ------------------------------------------------------------------------------------------------ the C entries
def _refuser(entry, call):
    from minddiffusion_amd import _lib
    lib = _lib.load()

    def refused(msg, **kw):
        assert call(lib, **kw) == -1
        err = lib.mdx_last_error()
        assert entry in err and msg in err, err
    return refused


def _table(values):
    return (ctypes.c_int * len(values))(*values)


def test_gather_argument_validation_without_gpu():
    def call(lib, canvas=P, out=2 * P, off=3 * P, host=(0, 0, 4, 8, 12), ny=1, nx=4, k0=0, n=4, NB=2, C=4, Hc=8, Wc=20, h=8,
             w=8):
        t = None if host is None else _table(host)
        return lib.mdx_window_gather_f32(canvas, out, off, t, ny, nx, k0, n, NB, C, Hc, Wc, h, w, None)
    refused = _refuser(b"mdx_window_gather_f32", call)
    for name in ("canvas", "out", "off", "host"):
        refused(b"null pointer", **{name: None})
    for kw in ({"NB": 0}, {"C": 0}, {"h": 0}, {"w": -1}, {"ny": 0}, {"nx": 0}, {"Hc": 0}):
        refused(b"bad extents", **kw)
    refused(b"larger than the canvas", h=9)
    refused(b"larger than the canvas", w=21)
    refused(b"an offset leaves the canvas", host=(0, 0, 4, 8, 13))
    refused(b"an offset leaves the canvas", host=(0, -1, 4, 8, 12))
    refused(b"an offset leaves the canvas", host=(1, 0, 4, 8, 12))
    refused(b"start at 0 and end at L - w", host=(0, 0, 4, 8, 11))
    refused(b"must ascend", host=(0, 0, 8, 4, 12))
    refused(b"uncovered", host=(0, 0, 12), nx=2, n=2)
    for k0, n in ((-1, 2), (0, 0), (0, 5), (3, 2)):
        refused(b"not inside the grid", k0=k0, n=n)
    refused(b"out overlaps canvas", out=P + 64)


def test_average_argument_validation_without_gpu():
    def call(lib, win=P, out=2 * P, wts=None, nw=0, off=3 * P, host=(0, 0, 4, 8, 12), ny=1, nx=4, NB=2, C=4, ld=8, Hc=8, Wc=20,
             h=8, w=8):
        t = None if host is None else _table(host)
        return lib.mdx_window_average_f16(win, out, wts, nw, off, t, ny, nx, NB, C, ld, Hc, Wc, h, w, None)
    refused = _refuser(b"mdx_window_average_f16", call)
    for name in ("win", "out", "off", "host"):
        refused(b"null pointer", **{name: None})
    for kw in ({"NB": 0}, {"C": 0}, {"h": 0}, {"w": -1}, {"ny": 0}, {"nx": 0}, {"Wc": 0}):
        refused(b"bad extents", **kw)
    refused(b"larger than the canvas", h=9)
    refused(b"larger than the canvas", w=21)
    refused(b"an offset leaves the canvas", host=(0, 0, 4, 8, 13))
    refused(b"an offset leaves the canvas", host=(0, 0, 4, 8, -2))
    refused(b"uncovered", host=(0, 0, 12), nx=2)
    refused(b"ld must be", ld=0)                                    # ld < C
    refused(b"ld must be", C=9)
    refused(b"ld must be", ld=12)
    refused(b"16-byte aligned", win=P + 8)
    refused(b"out overlaps windows", out=P + 64)
    for nw in (0, -64):
        refused(b"non-positive weight count", wts=4 * P, nw=nw)
    refused(b"63 weights for a window of 8 x 8", wts=4 * P, nw=63)


def test_the_window_entries_are_declared_as_the_header_declares_them():
    from minddiffusion_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.S)
    kinds = {"int": _lib.c_int, "float": _lib.c_float, "mdx_stream_t": _lib.c_void_p}
    for name in ("mdx_window_gather_f32", "mdx_window_average_f16"):
        args = [a.strip() for a in re.search(rf"\bint {name}\s*\(([^)]*)\)", header).group(1).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is _lib.c_int and len(argtypes) == len(args), name
        for a, ty in zip(args, argtypes):
            want = _lib.c_void_p if "*" in a else kinds[a.rsplit(" ", 1)[0].replace("const ", "")]
            assert ty is want, (name, a)
        assert args[-1].startswith("mdx_stream_t")
    assert hasattr(_lib.load(), "mdx_window_gather_f32") and hasattr(_lib.load(), "mdx_window_average_f16")


# ------------------------------------------------------------------------------------------------ Python refusals
class _Net:
    channel_mult = (1, 2)
    num_classes = None
    final_channels = 4
    device = torch.device("cpu")


def _ldm(net=None, **kw):
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    return LatentDiffusion(net or _Net(), linear_start=0.00085, linear_end=0.0120, timesteps=1000, **kw)


def test_windowed_diffusion_refusals(monkeypatch):
    from minddiffusion_amd import distributed
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion, gaussian_weights
    wm = WindowedDiffusion(_ldm(), window=(8, 8))
    assert wm.stride == (4, 4) and wm.window == (8, 8) and wm.max_unet_batch == 16 and wm.chunks == []
    with pytest.raises(MdxError, match="class-conditional"):
        WindowedDiffusion(_ldm(conditioning_key="adm"), window=(8, 8))
    labelled = _Net()
    labelled.num_classes = 10
    with pytest.raises(MdxError, match="class-conditional"):
        WindowedDiffusion(_ldm(labelled), window=(8, 8))
    with pytest.raises(MdxError, match="not divisible by 2"):
        WindowedDiffusion(_ldm(), window=(8, 9))
    with pytest.raises(MdxError, match="already windowed"):
        WindowedDiffusion(wm)
    for bad in (15, 0, 1, -2, 3.5, True):
        with pytest.raises(MdxError, match="max_unet_batch"):
            WindowedDiffusion(_ldm(), window=(8, 8), max_unet_batch=bad)
    for bad in ((0, 4), (4, 9), (9, 4)):
        with pytest.raises(MdxError, match="stride"):
            WindowedDiffusion(_ldm(), window=(8, 8), stride=bad)
    for bad in ("64", (8, 8, 8), (8.5, 8), None):
        with pytest.raises(MdxError, match="window must be an int"):
            WindowedDiffusion(_ldm(), window=bad)
    with pytest.raises(MdxError, match="weights have shape"):
        WindowedDiffusion(_ldm(), window=(8, 8), weights=torch.ones(8, 4))
    with pytest.raises(MdxError, match="weights have shape"):
        WindowedDiffusion(_ldm(), window=(8, 8), weights=torch.ones(64))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        w = torch.ones(8, 8)
        w[3, 5] = bad
        with pytest.raises(MdxError, match="positive"):
            WindowedDiffusion(_ldm(), window=(8, 8), weights=w)
    assert WindowedDiffusion(_ldm(), window=(8, 8), weights=gaussian_weights(8, 8)).weights.shape == (8, 8)
    with pytest.raises(MdxError, match="CUDA"):
        wm.apply_model_nhwc(torch.zeros(2, 4, 8, 20), torch.zeros(2), None)
    monkeypatch.setattr(distributed, "world", lambda: (0, 2))
    with pytest.raises(MdxError, match="single rank"):
        WindowedDiffusion(_ldm(), window=(8, 8))


def test_everything_not_overridden_is_the_inner_models():
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    inner = _ldm(parameterization="v", scale_factor=0.5)
    wm = WindowedDiffusion(inner, window=(8, 8))
    assert wm.inner is inner and wm.unet is inner.unet and wm.model is inner.model
    assert wm.model.conditioning_key == "crossattn" and wm.parameterization == "v" and wm.scale_factor == 0.5
    assert wm.alphas_cumprod is inner.alphas_cumprod and wm.num_timesteps == 1000
    assert wm.first_stage_model is None and wm.cond_stage_model is None
    assert wm.load_lora.__self__ is inner and wm.set_lora_scale.__self__ is inner and wm.unload_lora.__self__ is inner
    assert wm.time_embedding_table.__self__ is inner
    with pytest.raises(AttributeError):
        wm.no_such_attribute
    g = wm.grid_for(8, 20)
    assert (g.h, g.w, g.oy, g.ox) == (8, 8, [0], [0, 4, 8, 12]) and wm.grid_for(8, 20) is g
    g = wm.grid_for(4, 20)                                          # a window larger than the canvas: the canvas extent
    assert (g.h, g.w, g.oy) == (4, 8, [0])
    assert wm.grid_for(8, 8).N == 1


def test_gaussian_weights():
    from minddiffusion_amd.ldm.models.diffusion.windowed import gaussian_weights
    w = gaussian_weights(8, 12)
    assert w.dtype == torch.float32 and tuple(w.shape) == (8, 12) and bool((w > 0).all())
    assert torch.equal(w, w.flip(0)) and torch.equal(w, w.flip(1))   # symmetric about the centre
    assert float(w.max()) == float(w[3, 5]) and float(w[0, 0]) == float(w.min())
    d = (np.arange(8) - 3.5) / (0.5 * 8)
    assert np.allclose(gaussian_weights(8, 1)[:, 0].numpy(), np.exp(-0.5 * d ** 2), rtol=1e-6)
    assert float(gaussian_weights(8, 8, sigma_frac=0.25)[0, 0]) < float(w[0, 0])
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma_frac"):
            gaussian_weights(8, 8, bad)


def test_pipeline_windowed_refusals_and_units():
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    from minddiffusion_amd.pipeline import DiffusionPipeline
    import minddiffusion_amd
    assert minddiffusion_amd.WindowedDiffusion is WindowedDiffusion
    for kind in ("ddim", "plms", "dpm_solver"):
        pipe = DiffusionPipeline(_ldm(), kind, device="cpu")
        wp = pipe.windowed(window=64)
        assert isinstance(wp, DiffusionPipeline) and wp is not pipe and type(wp.sampler) is type(pipe.sampler)
        assert isinstance(wp.model, WindowedDiffusion) and wp.model.inner is pipe.model and wp.device == pipe.device
        assert wp.model.window == (8, 8) and wp.model.stride == (4, 4) and wp.sampler.model is wp.model
        assert pipe.windowed(window=(64, 128), stride=(16, 64), max_unet_batch=8).model.stride == (2, 8)
        for bad in (60, (64, 4), 0, -64):
            with pytest.raises(MdxError, match="multiples of 8"):
                pipe.windowed(window=bad)
        with pytest.raises(MdxError, match="multiples of 8"):
            pipe.windowed(window=64, stride=12)
        with pytest.raises(MdxError, match="max_unet_batch"):
            pipe.windowed(window=64, max_unet_batch=7)
    with pytest.raises(MdxError, match="DiffusionPipeline.windowed"):
        DiffusionPipeline(_ldm(), object(), device="cpu").windowed(window=64)


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_numpy_average_is_the_stated_arithmetic():
    """A check of the YARDSTICK, not of the product (it passes without the feature): tests/_window_util.py, which the GPU tests
    compare against, is held to sums written out by hand in np.float32, and its own grid rule and chunk list to the hand values
    the product's are held to above."""
    assert U.offsets(20, 8, 4) == [0, 4, 8, 12] and U.offsets(18, 8, 4) == [0, 4, 8, 10] and U.offsets(8, 8, 4) == [0]
    assert U.offsets(256, 64, 32) == [0, 32, 64, 96, 128, 160, 192] and U.offsets(9, 8, 8) == [0, 1]
    assert U.chunks(7, 2, 16) == [(0, 7)] and U.chunks(7, 4, 16) == [(0, 4), (4, 3)] and U.chunks(4, 4, 8) == [(0, 2), (2, 2)]
    rng = np.random.RandomState(0)
    oy, ox = [0], [0, 4, 8, 10]
    win = rng.randn(2 * 4, 64, 8).astype(np.float16)
    out, cnt = U.average_ref(win, oy, ox, 8, 8, 8, 18, 4)
    assert out.dtype == np.float16 and out.shape == (2, 8 * 18, 8) and cnt[0].tolist() == [1] * 4 + [2] * 6 + [3] * 2 + [2] * 4 + [1] * 2
    e = win.reshape(2, 4, 8, 8, 8)
    o = out.reshape(2, 8, 18, 8)
    assert np.array_equal(o[:, :, :4, :4], e[:, 0, :, :4, :4]) and np.array_equal(o[:, :, 16:, :4], e[:, 3, :, 6:, :4])
    # column 10 lies under windows 1, 2, 3 at their columns 6, 2, 0
    acc = e[:, 1, :, 6, :4].astype(np.float32)
    acc = (acc + e[:, 2, :, 2, :4].astype(np.float32)).astype(np.float32)
    acc = (acc + e[:, 3, :, 0, :4].astype(np.float32)).astype(np.float32)
    assert np.array_equal(o[:, :, 10, :4], (acc / np.float32(3)).astype(np.float16))
    assert not o[..., 4:].any()
    ref64, _ = U.weighted_ref64(win, np.ones((8, 8), np.float32), oy, ox, 8, 8, 8, 18, 4)
    ulp = np.spacing(np.abs(ref64).astype(np.float16)).astype(np.float64)
    assert np.all(np.abs(out.astype(np.float64) - ref64.astype(np.float64)) <= ulp)
    x = torch.arange(2 * 3 * 8 * 18, dtype=torch.float32).reshape(2, 3, 8, 18)
    got = U.gather_ref(x, oy, ox, 8, 8, 1, 2)
    assert tuple(got.shape) == (4, 3, 8, 8) and torch.equal(got[1], x[0, :, :, 8:16]) and torch.equal(got[2], x[1, :, :, 4:12])
