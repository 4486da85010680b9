"""Regions and wrap-around windows of the windowed evaluation -- the parts that need no GPU: the wrapped grid and its coverage,
RegionPlan's pair lists, the chunk lists over pairs, every host refusal of mdx_window_gather_rows_f32 and
mdx_window_average_regions_f16 (before any launch) and of the Python layers, the pipeline's background mask, the C declarations
against include/mdx.h, and the CPU confirmation that a float32 emulation of the region arithmetic stays inside the bound the GPU
test holds the kernel to (tests/_window_regions_util.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _window_regions_util as RU
import _window_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20         # disjoint non-null addresses P, 2P, ...: nothing is dereferenced by a refused call


# ------------------------------------------------------------------------------------------------ the wrapped grid
def test_wrapped_offsets_and_coverage_by_hand():
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    g = ops.WindowGrid((8, 20), (8, 8), (4, 4), wrap_x=True)
    assert g.wrap_x and g.ox == [0, 4, 8, 12, 16] and (g.ny, g.nx, g.N) == (1, 5, 5)
    assert g.host.dtype == np.int32 and g.host.tolist() == [0, 0, 4, 8, 12, 16]
    assert g.columns(4).tolist() == [16, 17, 18, 19, 0, 1, 2, 3]             # the window at 16 straddles the seam
    assert np.array_equal(g.coverage(), np.full((8, 20), 2))                  # Wc % s == 0: w / s everywhere
    g = ops.WindowGrid((8, 18), (8, 8), (4, 3), wrap_x=True)
    assert g.ox == [0, 3, 6, 9, 12, 15] and g.nx == 6                         # nx = ceil(18 / 3)
    # column x is covered by the offsets o with (x - o) mod 18 < 8: 0..7 back from x, those that are multiples of 3
    assert g.coverage()[0].tolist() == [sum((x - o) % 18 < 8 for o in g.ox) for x in range(18)]
    assert g.coverage()[0].tolist() == [3, 3, 2] * 6
    g = ops.WindowGrid((8, 20), (8, 8), (4, 6), wrap_x=True)                  # Wc % s != 0: the last gap is short
    assert g.ox == [0, 6, 12, 18] and g.coverage()[0].tolist() == [sum((x - o) % 20 < 8 for o in g.ox) for x in range(20)]
    assert g.coverage().min() >= 1
    g = ops.WindowGrid((12, 20), (8, 8), (4, 4), wrap_x=True)                 # rows never wrap; k = iy * nx + ix
    assert g.oy == [0, 4] and [g.origin(k) for k in (0, 4, 5, 9)] == [(0, 0), (0, 16), (4, 0), (4, 16)]
    assert np.array_equal(g.coverage(), np.array([1] * 4 + [2] * 4 + [1] * 4)[:, None] * np.full(20, 2)[None, :])
    plain = ops.WindowGrid((8, 20), (8, 8), (4, 4))
    assert not plain.wrap_x and plain.ox == [0, 4, 8, 12]                     # the default is the clamped grid
    for bad in ((8, 20), (8, 21)), ((8, 20), (8, 8), (4, 9)):
        with pytest.raises(MdxError, match="window_offsets"):
            ops.WindowGrid(bad[0], bad[1], bad[2] if len(bad) > 2 else (4, 4), wrap_x=True)
    # the restatement the GPU tests use gives the same
    assert RU.wrap_offsets(18, 3) == [0, 3, 6, 9, 12, 15] and RU.x_offsets(20, 8, 4, True) == [0, 4, 8, 12, 16]
    assert RU.x_offsets(20, 8, 4, False) == [0, 4, 8, 12] and RU.x_offsets(8, 8, 4, True) == [0]
    assert np.array_equal(RU.coverage([0, 4], [0, 4, 8, 12, 16], 8, 8, 12, 20), g.coverage())


def test_a_wrapped_grid_is_refused_by_the_clamped_entries():
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    g = ops.WindowGrid((8, 20), (8, 8), (4, 4), wrap_x=True)
    for call in (lambda: ops.window_gather(torch.zeros(1), g), lambda: ops.window_average(torch.zeros(1), g, 4)):
        with pytest.raises(MdxError):
            call()


# ------------------------------------------------------------------------------------------------ the pairs
def test_region_plan_pair_lists_by_hand():
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    g = ops.WindowGrid((8, 20), (8, 8), (4, 4), wrap_x=True)                  # windows at 0 4 8 12 16
    m = np.zeros((3, 8, 20), np.float32)
    m[0] = 1.0                                                                # the background: everywhere
    m[1, :, 9:11] = 0.5                                                       # columns 9, 10: windows at 4 and 8
    m[2, 2, 1] = 1.0                                                          # one pixel at column 1: the windows at 0 and at 16
    plan = ops.RegionPlan(g, m)
    assert plan.R == 3 and plan.pairs == [(0, 0), (0, 2), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (4, 0), (4, 2)]
    assert plan.P == 9 and plan.pair_window.host.tolist() == [0, 0, 1, 1, 2, 2, 3, 4, 4]
    assert plan.pair_region.host.tolist() == [0, 2, 0, 1, 0, 1, 0, 0, 2] and plan.pair_first.host.tolist() == [0, 2, 4, 6, 7, 9]
    assert all(t.host.dtype == np.int32 for t in (plan.pair_window, plan.pair_region, plan.pair_first))
    assert plan.pairs == RU.pair_list(m, g.oy, g.ox, 8, 8)
    # a region touching only the seam-straddling window: columns 18, 19 lie in the windows at 12 and 16, column 19 alone ...
    m = np.zeros((2, 8, 20), np.float32)
    m[0] = 1.0
    m[1, :, 2:4] = 1.0                                                        # columns 2, 3: the window at 0 and, wrapped, at 16
    plan = ops.RegionPlan(g, m)
    assert [k for k, r in plan.pairs if r == 1] == [0, 4]
    clamped = ops.RegionPlan(ops.WindowGrid((8, 20), (8, 8), (4, 4)), m)      # without wrap only the window at 0 holds them
    assert [k for k, r in clamped.pairs if r == 1] == [0] and clamped.P == 5
    # a pixel with M_r > 0 has every covering window active for r
    rng = np.random.RandomState(5)
    g2 = ops.WindowGrid((12, 18), (8, 8), (4, 3), wrap_x=True)
    m = (rng.rand(3, 12, 18) > 0.9).astype(np.float32)
    m[0] = 1.0
    plan = ops.RegionPlan(g2, m)
    assert plan.pairs == RU.pair_list(m, g2.oy, g2.ox, 8, 8) == sorted(plan.pairs)
    for r, y, x in zip(*np.nonzero(m)):
        for k in range(g2.N):
            if 0 <= y - g2.origin(k)[0] < 8 and (x - g2.origin(k)[1]) % 18 < 8:
                assert (k, r) in plan.pairs
    for bad, msg in ((np.ones((3, 8, 18)), "shape"), (np.ones((8, 20)), "shape"), (-np.ones((1, 8, 20)), ">= 0"),
                     (np.full((1, 8, 20), np.nan), "finite"), (np.full((1, 8, 20), np.inf), "finite")):
        with pytest.raises(MdxError, match=msg):
            ops.RegionPlan(g, bad.astype(np.float32))
    hole = np.ones((2, 8, 20), np.float32)
    hole[:, 3, 7] = 0.0
    with pytest.raises(MdxError, match="sum to > 0"):
        ops.RegionPlan(g, hole)


def test_chunks_over_pairs():
    from minddiffusion_amd.ldm.models.diffusion.windowed import chunk_list
    assert chunk_list(9, 4, 16) == [(0, 4), (4, 4), (8, 1)] == U.chunks(9, 4, 16)
    assert chunk_list(9, 2, 16) == [(0, 8), (8, 1)] and chunk_list(5, 4, 32) == [(0, 5)]


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
    return None if values is None else (ctypes.c_int * len(values))(*values)


def test_gather_rows_argument_validation_without_gpu():
    def call(lib, canvas=P, out=2 * P, off=3 * P, host=(0, 0, 4, 8, 12, 16), ny=1, nx=5, rows=4 * P, rows_host=(4, 0, 4), n=3,
             wrap=1, NB=2, C=4, Hc=8, Wc=20, h=8, w=8):
        return lib.mdx_window_gather_rows_f32(canvas, out, off, _table(host), ny, nx, rows, _table(rows_host), n, wrap, NB, C, Hc,
                                              Wc, h, w, None)
    refused = _refuser(b"mdx_window_gather_rows_f32", call)
    for name in ("canvas", "out", "off", "host", "rows", "rows_host"):
        refused(b"null pointer", **{name: None})
    for kw in ({"NB": 0}, {"C": 0}, {"h": 0}, {"w": -1}, {"ny": 0}, {"nx": 0}, {"Hc": 0}):
        refused(b"bad extents", **kw)
    refused(b"wrap_x must be 0 or 1", wrap=2)
    refused(b"larger than the canvas", h=9)
    refused(b"larger than the canvas", w=21)
    # the wrapped axis: start at 0, ascend, every gap <= w, the last < Wc, Wc - last <= w
    refused(b"an offset leaves the canvas", host=(0, 0, 4, 8, 12, 20))
    refused(b"an offset leaves the canvas", host=(0, -4, 4, 8, 12, 16))
    refused(b"must start at 0", host=(0, 4, 8, 12, 16, 19))
    refused(b"must ascend", host=(0, 0, 8, 4, 12, 16))
    refused(b"uncovered", host=(0, 0, 4, 13, 16), nx=4)                       # a gap of 9
    refused(b"uncovered", host=(0, 0, 4, 8, 11), nx=4)                        # 20 - 11 > 8: columns 19 .. are not reached
    # the same table without wrap is the clamped rule's to judge: the window at 16 leaves the canvas
    refused(b"an offset leaves the canvas", wrap=0)
    refused(b"start at 0 and end at L - w", wrap=0, host=(0, 0, 4, 8, 11), nx=4, rows_host=(0, 1, 2))
    refused(b"non-positive row count", n=0)
    for rows_host in ((0, 5, 1), (-1, 0, 0)):
        refused(b"not inside the grid", rows_host=rows_host)
    refused(b"out overlaps canvas", out=P + 64)


def test_average_regions_argument_validation_without_gpu():
    pairs_w, pairs_r, first = (0, 0, 1, 2, 3, 4, 4), (0, 1, 0, 0, 0, 0, 1), (0, 2, 3, 4, 5, 7)

    def call(lib, win=P, out=2 * P, wts=None, nw=0, off=3 * P, host=(0, 0, 4, 8, 12, 16), ny=1, nx=5, wrap=1, pw=pairs_w,
             pr=4 * P, pr_host=pairs_r, pf=5 * P, pf_host=first, Pn=7, masks=6 * P, R=2, NB=2, C=4, ld=8, Hc=8, Wc=20, h=8, w=8):
        return lib.mdx_window_average_regions_f16(win, out, wts, nw, off, _table(host), ny, nx, wrap, _table(pw), pr,
                                                  _table(pr_host), pf, _table(pf_host), Pn, masks, R, NB, C, ld, Hc, Wc, h, w,
                                                  None)
    refused = _refuser(b"mdx_window_average_regions_f16", call)
    for name in ("win", "out", "off", "host", "pw", "pr", "pr_host", "pf", "pf_host", "masks"):
        refused(b"null pointer", **{name: None})
    for kw in ({"NB": 0}, {"C": 0}, {"h": 0}, {"w": -1}, {"ny": 0}, {"nx": 0}, {"Wc": 0}):
        refused(b"bad extents", **kw)
    refused(b"wrap_x must be 0 or 1", wrap=-1)
    refused(b"larger than the canvas", h=9)
    refused(b"an offset leaves the canvas", host=(0, 0, 4, 8, 12, 20))
    refused(b"must start at 0", host=(0, 2, 4, 8, 12, 16))
    refused(b"must ascend", host=(0, 0, 4, 4, 12, 16))
    refused(b"uncovered", host=(0, 0, 4, 8, 11), nx=4)
    refused(b"an offset leaves the canvas", wrap=0)
    refused(b"ld must be", ld=0)
    refused(b"ld must be", C=9)
    refused(b"ld must be", ld=12)
    refused(b"bad pair or region count", Pn=0)
    refused(b"bad pair or region count", R=-1)
    # no regions: no masks, and the pairs are the windows
    refused(b"masks without regions", R=0, Pn=5)
    refused(b"the pairs are the windows", R=0, masks=None, Pn=7)
    # the pair tables
    refused(b"from 0 to P", pf_host=(1, 2, 3, 4, 5, 7))
    refused(b"from 0 to P", pf_host=(0, 2, 3, 4, 5, 6))
    refused(b"must not descend", pf_host=(0, 2, 1, 4, 5, 7))
    refused(b"must not descend", pf_host=(0, 2, 3, 4, 9, 7))
    refused(b"sorted by window", pw=(0, 1, 1, 2, 3, 4, 4))
    refused(b"is region 2 of 2", pr_host=(0, 2, 0, 0, 0, 0, 1))
    refused(b"is region -1 of 2", pr_host=(-1, 1, 0, 0, 0, 0, 1))
    refused(b"must ascend", pr_host=(1, 0, 0, 0, 0, 0, 1))
    refused(b"must ascend", pr_host=(0, 0, 0, 0, 0, 0, 1))
    refused(b"16-byte aligned", win=P + 8)
    refused(b"16-byte aligned", out=2 * P + 2)
    refused(b"out overlaps windows", out=P + 64)
    for nw in (0, -64):
        refused(b"non-positive weight count", wts=7 * P, nw=nw)
    refused(b"63 weights for a window of 8 x 8", wts=7 * P, nw=63)


def test_the_two_entries_are_declared_as_the_header_declares_them():
    from minddiffusion_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.S)
    kinds = {"int": _lib.c_int, "float": _lib.c_float, "mdx_stream_t": _lib.c_void_p}
    for name, nargs in (("mdx_window_gather_rows_f32", 17), ("mdx_window_average_regions_f16", 25)):
        args = [a.strip() for a in re.search(rf"\bint {name}\s*\(([^)]*)\)", header).group(1).split(",")]
        res, argtypes = _lib.SIGNATURES[name]
        assert res is _lib.c_int and len(argtypes) == len(args) == nargs, name
        for a, ty in zip(args, argtypes):
            want = _lib.c_void_p if "*" in a else kinds[a.rsplit(" ", 1)[0].replace("const ", "")]
            assert ty is want, (name, a)
        assert args[-1].startswith("mdx_stream_t") and "int wrap_x" in args
        assert hasattr(_lib.load(), name)


# ------------------------------------------------------------------------------------------------ Python refusals
class _Net:
    channel_mult = (1, 2)
    num_classes = None
    final_channels = 4
    device = torch.device("cpu")


def _ldm(**kw):
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    return LatentDiffusion(_Net(), linear_start=0.00085, linear_end=0.0120, timesteps=1000, **kw)


def test_ops_refusals_without_gpu():
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    g = ops.WindowGrid((8, 20), (8, 8), (4, 4), wrap_x=True)
    with pytest.raises(MdxError, match="GPU"):
        ops.window_gather_rows(torch.zeros(2, 4, 8, 20), g, [0, 1])
    with pytest.raises(MdxError, match="GPU"):
        ops.window_average_regions(torch.zeros(10, 64, 8, dtype=torch.float16), g, 4)


def test_windowed_diffusion_wrap_and_region_refusals():
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    wm = WindowedDiffusion(_ldm(), window=(8, 8), wrap_x=True)
    assert wm.wrap_x and wm.pairs == [] and wm.chunks == [] and not WindowedDiffusion(_ldm(), window=(8, 8)).wrap_x
    assert wm.grid_for(8, 20).wrap_x and wm.grid_for(8, 20).ox == [0, 4, 8, 12, 16]
    assert not wm.grid_for(8, 8).wrap_x and wm.grid_for(8, 8).N == 1          # a canvas of one window has nothing to wrap
    assert not wm.grid_for(8, 6).wrap_x and wm.grid_for(8, 6).N == 1
    ones = torch.ones(2, 8, 20)
    cpu = [torch.zeros(2, 7, 64), torch.zeros(2, 7, 64)]
    for masks, ctxs, msg in ((torch.ones(8, 20), cpu, r"expected \[R, Hc, Wc\]"), (ones, cpu[:1], "1 contexts for 2 masks"),
                             (ones, cpu, "CUDA")):
        with pytest.raises(MdxError, match=msg):
            with wm.regions(masks, ctxs):
                pass
    assert wm._regions is None


def test_pipeline_region_refusals_and_the_background_mask(monkeypatch):
    from minddiffusion_amd import distributed
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.pipeline import DiffusionPipeline
    pipe = DiffusionPipeline(_ldm(), "ddim", device="cpu")
    wp = pipe.windowed(window=64, wrap_x=True)
    assert wp.model.wrap_x and wp.seam_cols == 8 and pipe.seam_cols == 0
    assert pipe.windowed(window=64, wrap_x=True, seam_pad=0).seam_cols == 0 and pipe.windowed(window=64, seam_pad=16).seam_cols == 0
    assert pipe.windowed(window=64, wrap_x=True, seam_pad=16).seam_cols == 2 and not pipe.windowed(window=64).model.wrap_x
    for bad in (-8, 12, 8.0, True):
        with pytest.raises(MdxError, match="seam_pad"):
            pipe.windowed(window=64, wrap_x=True, seam_pad=bad)
    c = torch.zeros(2, 7, 64)
    m = torch.zeros(8, 20)
    m[:, 10:] = 1.0
    kw = dict(c=c, uc=c, H=64, W=160, steps=2)
    with pytest.raises(MdxError, match="needs a windowed pipeline"):
        pipe(regions=[{"c": c, "mask": m}], **kw)
    with pytest.raises(MdxError, match="needs a windowed pipeline"):
        pipe.img2img(init_latent=torch.zeros(2, 4, 8, 20), c=c, uc=c, steps=2, regions=[{"c": c, "mask": m}])
    for bad, msg in ((torch.zeros(8, 18), "the mask is"), (torch.zeros(1, 8, 20), "the mask is"), (m * 1.5, r"\[0, 1\]"),
                     (m - 0.5, r"\[0, 1\]"), (m * float("nan"), "finite"), (m + float("inf"), "finite")):
        with pytest.raises(MdxError, match=msg):
            wp(regions=[{"c": c, "mask": bad}], **kw)
    for bad in ([], [{"mask": m}], [{"c": c, "prompt": "x", "mask": m}], [{"c": c}], ["x"]):
        with pytest.raises(MdxError, match="region"):
            wp(regions=bad, **kw)
    with pytest.raises(MdxError, match=r"c must be a tensor \[2 \| 1, T, D\]"):
        wp(regions=[{"c": torch.zeros(3, 7, 64), "mask": m}], **kw)
    monkeypatch.setattr(distributed, "world", lambda: (0, 2))
    with pytest.raises(MdxError, match="single rank"):
        wp(regions=[{"c": c, "mask": m}], batch_size=2, **kw)
    # region 0 is the call's own prompt on 1 - max_r m_r: the masks sum to >= 1 everywhere
    a, b = torch.zeros(8, 20), torch.zeros(8, 20)
    a[:, :8], b[:, 4:12] = 0.5, 0.75
    full = DiffusionPipeline.background_mask(torch.stack([a, b]))
    assert tuple(full.shape) == (3, 8, 20) and torch.equal(full[1], a) and torch.equal(full[2], b)
    assert full[0, 0].tolist() == [0.5] * 4 + [0.25] * 8 + [1.0] * 8 and float(full.sum(0).min()) >= 1.0


def test_use_cfg_is_the_guided_models_rule():
    from minddiffusion_amd.ldm.models.diffusion import guided
    uc = torch.zeros(1)
    assert guided.use_cfg(uc, None, 3.0) and guided.use_cfg(None, uc, 3.0) and guided.use_cfg(uc, None, [1.0, 2.0])
    assert not guided.use_cfg(None, None, 3.0) and not guided.use_cfg(uc, None, 1.0) and not guided.use_cfg(uc, None, [1.0, 1.0])


# ------------------------------------------------------------------------------------------------ the yardstick
def test_the_numpy_wrapped_average_is_the_stated_arithmetic():
    """A check of the yardstick: sums written out by hand in np.float32 at the seam."""
    rng = np.random.RandomState(1)
    oy, ox = [0], [0, 4, 8, 12, 16]
    win = rng.randn(2 * 5, 64, 8).astype(np.float16)
    out, cnt = RU.average_wrap_ref(win, oy, ox, 8, 8, 8, 20, 4)
    assert out.dtype == np.float16 and out.shape == (2, 160, 8) and np.array_equal(cnt, np.full((8, 20), 2))
    e, o = win.reshape(2, 5, 8, 8, 8), out.reshape(2, 8, 20, 8)
    # column 1 lies under the window at 0 (its column 1) and, wrapped, under the window at 16 (its column 5): ascending k
    acc = (e[:, 0, :, 1, :4].astype(np.float32) + e[:, 4, :, 5, :4].astype(np.float32)).astype(np.float32)
    assert np.array_equal(o[:, :, 1, :4], (acc / np.float32(2)).astype(np.float16))
    acc = (e[:, 3, :, 6, :4].astype(np.float32) + e[:, 4, :, 2, :4].astype(np.float32)).astype(np.float32)
    assert np.array_equal(o[:, :, 18, :4], (acc / np.float32(2)).astype(np.float16)) and not o[..., 4:].any()
    # without wrap it is the existing restatement
    w4 = win[:8]
    assert np.array_equal(RU.average_wrap_ref(w4, oy, ox[:4], 8, 8, 8, 20, 4)[0], U.average_ref(w4, oy, ox[:4], 8, 8, 8, 20, 4)[0])
    x = torch.arange(2 * 3 * 8 * 20, dtype=torch.float32).reshape(2, 3, 8, 20)
    got = RU.gather_rows_ref(x, oy, ox, 8, 8, [4, 1, 4])
    assert tuple(got.shape) == (6, 3, 8, 8) and torch.equal(got[0], torch.cat([x[0, :, :, 16:], x[0, :, :, :4]], 2))
    assert torch.equal(got[1], x[0, :, :, 4:12]) and torch.equal(got[2], got[0]) and torch.equal(got[4], x[1, :, :, 4:12])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["stripes", "ramp"])
@pytest.mark.parametrize("name", sorted(RU.CANVASES))
def test_a_float32_emulation_of_the_region_arithmetic_stays_inside_the_bound(name, kind, weighted):
    """The bound the GPU test holds the kernel to, confirmed on the CPU on the same inputs: the float32 emulation of the stated
    arithmetic (first term q * e, then fma, qsum by adds, one divide, one rounding to fp16) is within
    ulp16 / 2 + (2 T + 3) 2^-24 sum |q e| / sum q of the float64 mean, at every element."""
    from minddiffusion_amd.ldm.models.diffusion.windowed import gaussian_weights
    shape, oy, ox, _ = RU.canvas_grid(name)
    win, pairs, masks = RU.pair_outputs(name, kind)
    wts = gaussian_weights(8, 8).numpy() if weighted else None
    ref, T, mag = RU.region_ref64(win, pairs, masks, wts, oy, ox, 8, 8, 4)
    got = RU.region_emul32(win, pairs, masks, wts, oy, ox, 8, 8, 4).reshape(ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    bound = RU.region_bound(got, ref, T, mag)
    print(f"{name} {kind} weighted={weighted}: P={len(pairs)}, T up to {T.max()}, worst err / bound {float((err / bound).max()):.3f}")
    assert err.shape == bound.shape and np.all(err <= bound)
    assert T.min() >= 1 and (name != "clamped" or kind != "stripes" or (T == 1).any())
