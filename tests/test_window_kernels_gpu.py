"""The two launches of csrc/window.hip on the GPU.  mdx_window_gather_f32 is a copy: torch.equal to torch slicing, in its float4
and its scalar form, on a sub-range of the windows, with a NaN sentinel around what it may write.  mdx_window_average_f16 with
uniform weights is held, bit for bit, to the arithmetic include/mdx.h states, restated in numpy on the CPU (_window_util.py);
with weights to one fp16 ulp of the float64 weighted mean: fp32 accumulation error (about 1e-6 relative) is far below half an
fp16 ulp (4.9e-4 relative), so only values within 1e-6 of a rounding tie can land on the neighbouring fp16 number."""
import numpy as np
import pytest
import torch

import _window_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (canvas [NB, C, Hc, Wc], window, stride): one row of four windows in the float4 form; the clamped last offset 10, which is no
# multiple of 4, so the scalar form; a 2-D grid of 2 x 4 windows with 9 channels (the hybrid inpainting UNet's input)
CASES = {"vector": ((4, 4, 8, 20), (8, 8), (4, 4)), "clamped": ((4, 4, 8, 18), (8, 8), (4, 4)), "grid2d": ((2, 9, 12, 20), (8, 8), (4, 4))}


def grid_of(case):
    from minddiffusion_amd import ops
    shape, win, stride = CASES[case]
    return ops.WindowGrid(shape[2:], win, stride), shape


_INPUTS = {}


def window_outputs(case, ld=8):
    """Random fp16 window outputs [NB * N, h * w, ld] (every channel filled: [C, ld) of the result must still be 0) and their
    uniform reference, made once."""
    if case not in _INPUTS:
        g, shape = grid_of(case)
        win = np.random.RandomState(len(case)).randn(shape[0] * g.N, g.h * g.w, ld).astype(np.float16)
        _INPUTS[case] = (win, U.average_ref(win, g.oy, g.ox, g.h, g.w, g.Hc, g.Wc, 4))
    return _INPUTS[case]


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("case", sorted(CASES))
def test_gather_is_torch_slicing(case):
    from minddiffusion_amd import ops
    g, shape = grid_of(case)
    assert {"vector": [0, 4, 8, 12], "clamped": [0, 4, 8, 10], "grid2d": [0, 4, 8, 12]}[case] == g.ox
    assert g.ny == (2 if case == "grid2d" else 1)
    x = torch.randn(shape, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    got = ops.window_gather(x, g)
    assert tuple(got.shape) == (shape[0] * g.N, shape[1], 8, 8)
    assert torch.equal(got, U.gather_ref(x, g.oy, g.ox, 8, 8, 0, g.N))
    # the row order keeps a [uncond ; cond] canvas batch a [uncond ; cond] window batch
    half = shape[0] // 2
    x[half:] = x[:half]
    got = ops.window_gather(x, g)
    assert torch.equal(got[:half * g.N], got[half * g.N:])


@pytest.mark.parametrize("case", sorted(CASES))
def test_gather_of_a_sub_range_writes_its_rows_only(case):
    from minddiffusion_amd import ops
    g, shape = grid_of(case)
    x = torch.randn(shape, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    for k0, n in ((1, 2), (g.N - 1, 1), (0, 3)):        # ("clamped": (1, 2) is the float4 form, the ranges with window 3 are not)
        rows = shape[0] * n
        buf = torch.full((rows + 2, shape[1], 8, 8), float("nan"), device=DEV)
        ops.window_gather(x, g, k0, n, out=buf[1:1 + rows])
        assert torch.equal(buf[1:1 + rows], U.gather_ref(x, g.oy, g.ox, 8, 8, k0, n))
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())


def test_the_two_gather_forms_move_the_same_bits():
    from minddiffusion_amd import ops
    g, shape = grid_of("vector")
    store = torch.randn(shape[0] * shape[1] * 8 * 20 + 1, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    y = store[1:].view(shape)                           # 4 bytes off a 16-byte boundary: the scalar form
    x = y.clone()                                       # the same values in an allocation of their own: the float4 form
    assert y.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    want = ops.window_gather(x, g)
    assert torch.equal(ops.window_gather(y, g), want) and torch.equal(want, U.gather_ref(y, g.oy, g.ox, 8, 8, 0, 4))


# ------------------------------------------------------------------------------------------------ average
@pytest.mark.parametrize("case", sorted(CASES))
def test_uniform_average_is_the_stated_arithmetic_bit_for_bit(case):
    from minddiffusion_amd import ops
    g, shape = grid_of(case)
    win, (want, cnt) = window_outputs(case)
    got = ops.window_average(torch.from_numpy(win).to(DEV), g, 4)
    assert got.dtype == torch.float16 and tuple(got.shape) == (shape[0], g.Hc * g.Wc, 8)
    got = got.cpu().numpy()
    diff = np.abs(got.astype(np.float32) - want.astype(np.float32)).max()
    print(f"{case}: counts {sorted(set(cnt.ravel().tolist()))}, max|d| {diff:.3e}")
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert np.array_equal(cnt, g.coverage()) and cnt.max() >= (3 if case == "clamped" else 2)
    # a pixel under one window is that window's value; channels [4, 8) are 0
    o = got.reshape(shape[0], g.Hc, g.Wc, 8)
    e = win.reshape(shape[0], g.N, 8, 8, 8)
    ys, xs = np.nonzero(cnt == 1)
    assert len(ys) > 0
    for y, x in zip(ys, xs):
        (k,) = [k for k in range(g.N) if 0 <= y - g.origin(k)[0] < 8 and 0 <= x - g.origin(k)[1] < 8]
        oy, ox = g.origin(k)
        assert np.array_equal(o[:, y, x, :4].view(np.uint16), e[:, k, y - oy, x - ox, :4].view(np.uint16))
    assert not o[..., 4:].any()


@pytest.mark.parametrize("case", sorted(CASES))
def test_average_footprint(case):
    """A NaN in one window's output reaches exactly the pixels that window covers; the staging buffer and what lies around the
    canvas buffer keep their bits."""
    from minddiffusion_amd import ops
    g, shape = grid_of(case)
    NB = shape[0]
    win = torch.from_numpy(window_outputs(case)[0]).to(DEV)
    k = g.N - 2
    win.view(NB, g.N, 64, 8)[1, k] = float("nan")
    before = win.clone()
    pix = g.Hc * g.Wc
    buf = torch.full((NB + 2, pix, 8), 7.0, dtype=torch.float16, device=DEV)
    ops.window_average(win, g, 4, out=buf[1:1 + NB])
    assert torch.equal(win.view(torch.int16), before.view(torch.int16))
    assert bool((buf[0] == 7.0).all()) and bool((buf[-1] == 7.0).all())
    nan = torch.isnan(buf[1:1 + NB, :, :4]).all(-1).view(NB, g.Hc, g.Wc).cpu()
    want = torch.zeros(NB, g.Hc, g.Wc, dtype=torch.bool)
    oy, ox = g.origin(k)
    want[1, oy:oy + 8, ox:ox + 8] = True
    assert torch.equal(nan, want)
    assert not bool(torch.isnan(buf[1:1 + NB, :, 4:]).any()) and bool((buf[1:1 + NB, :, 4:] == 0).all())


@pytest.mark.parametrize("case", sorted(CASES))
def test_weighted_average_is_within_one_fp16_ulp_of_the_float64_mean(case):
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.windowed import gaussian_weights
    g, shape = grid_of(case)
    win = window_outputs(case)[0]
    wts = gaussian_weights(8, 8)
    got = ops.window_average(torch.from_numpy(win).to(DEV), g, 4, weights=wts.to(DEV)).cpu().numpy()
    want, cnt = U.weighted_ref64(win, wts.numpy(), g.oy, g.ox, 8, 8, g.Hc, g.Wc, 4)
    ulp = np.spacing(np.abs(want)).astype(np.float64)              # fp16 spacing at the reference value
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{case}: weighted, elements off by one ulp: {int((err > 0).sum())} of {err.size}")
    assert np.all(err <= ulp)
    o, e = got.reshape(shape[0], g.Hc, g.Wc, 8), win.reshape(shape[0], g.N, 8, 8, 8)
    for y, x in zip(*np.nonzero(cnt == 1)):                         # exact under one window
        (k,) = [k for k in range(g.N) if 0 <= y - g.origin(k)[0] < 8 and 0 <= x - g.origin(k)[1] < 8]
        assert np.array_equal(o[:, y, x, :4].view(np.uint16), e[:, k, y - g.origin(k)[0], x - g.origin(k)[1], :4].view(np.uint16))
    assert not o[..., 4:].any()
    # equal weights are the plain mean up to the same bound (w * e and the fma are exact for w = 1: the same bits)
    ones = ops.window_average(torch.from_numpy(win).to(DEV), g, 4, weights=torch.ones(8, 8, device=DEV)).cpu().numpy()
    assert np.array_equal(ones.view(np.uint16), window_outputs(case)[1][0].view(np.uint16))


def test_wider_rows_are_averaged_chunk_by_chunk():
    from minddiffusion_amd import ops
    g, shape = grid_of("clamped")
    win = np.random.RandomState(9).randn(2 * g.N, 64, 16).astype(np.float16)
    got = ops.window_average(torch.from_numpy(win).to(DEV), g, 11).cpu().numpy()
    assert np.array_equal(got.view(np.uint16), U.average_ref(win, g.oy, g.ox, 8, 8, 8, 18, 11)[0].view(np.uint16))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    g, shape = grid_of("vector")
    x = torch.zeros(shape, device=DEV)
    win = torch.zeros(shape[0] * g.N, 64, 8, dtype=torch.float16, device=DEV)
    with pytest.raises(MdxError, match="GPU"):
        ops.window_gather(x.cpu(), g)
    with pytest.raises(MdxError, match="expected torch.float32"):
        ops.window_gather(x.half(), g)
    with pytest.raises(MdxError, match="canvas: shape"):
        ops.window_gather(x[:, :, :, :18].contiguous(), g)
    with pytest.raises(MdxError, match="out: shape"):
        ops.window_gather(x, g, 0, 2, out=torch.zeros(4, 4, 8, 8, device=DEV))
    for k0, n in ((0, 5), (-1, 2), (4, 1), (2, 0)):
        with pytest.raises(MdxError, match="not inside the grid"):
            ops.window_gather(x, g, k0, n)
    with pytest.raises(MdxError, match="windows: shape"):
        ops.window_average(win[:-1], g, 4)
    with pytest.raises(MdxError, match="windows: shape"):
        ops.window_average(win[:, :60].contiguous(), g, 4)
    with pytest.raises(MdxError, match="expected torch.float16"):
        ops.window_average(win.float(), g, 4)
    with pytest.raises(MdxError, match="ld must be"):
        ops.window_average(win, g, 9)
    with pytest.raises(MdxError, match="weights: shape"):
        ops.window_average(win, g, 4, weights=torch.ones(64, device=DEV))
    with pytest.raises(MdxError, match="out: shape"):
        ops.window_average(win, g, 4, out=torch.zeros(shape[0], 8 * 20, 16, dtype=torch.float16, device=DEV))
    bad = ops.WindowGrid((8, 20), (8, 8), (4, 4))
    bad.host[4] = 13                                    # the host table is what is checked: refused before any launch
    with pytest.raises(MdxError, match="an offset leaves the canvas"):
        ops.window_gather(x, bad)
    with pytest.raises(MdxError, match="an offset leaves the canvas"):
        ops.window_average(win, bad, 4)
