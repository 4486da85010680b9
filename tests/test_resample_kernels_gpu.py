"""mdx_resample_f32 / mdx_resample_noised_f32 on the GPU: parity against a float64 restatement that applies the SAME fp32 tables
(tests/_resample_util.py), the bit-exact structure the header promises, the fused form's two ties, the footprint, the refusals.

Shapes: the smallest that reach every path -- 1x4x6x10 -> 9x25 (scalar stores, non-integer ratios), 2x4x8x8 -> 16x16 (vector
stores), 2x3x16x12 -> 8x6 (antialiased, 8 taps), 1x4x7x9 -> 5x4 -- and two that cross the 16 x 32 output tile in both directions
with partial tiles at the edges, 1x2x20x24 -> 40x72 (vector stores) and -> 37x45 (scalar).
The parity bound is derived (parity_bound), not measured; the measured distance is logged through _util.check.
"""
import ctypes

import numpy as np
import pytest
import torch

import _guard as G
from _resample_util import apply_tables, parity_bound
from _util import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [((1, 4, 6, 10), (9, 25)), ((2, 4, 8, 8), (16, 16)), ((2, 3, 16, 12), (8, 6)), ((1, 4, 7, 9), (5, 4)),
         ((1, 2, 20, 24), (40, 72)), ((1, 2, 20, 24), (37, 45))]
MODES = ("nearest", "bilinear", "bicubic", "lanczos3")
A, Bc = np.float32(0.8366), np.float32(0.5478)


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def _input(shape, seed=3):
    return np.clip(1.5 * np.random.RandomState(seed).randn(*shape), -5.0, 5.0).astype(np.float32)


def _tables(shape, size, mode, antialias=None, wrap_x=False):
    """The fp32 tables ops.resample builds for this call (antialias None: on for an axis that shrinks)."""
    from minddiffusion_amd import resample as R
    H, W = shape[-2:]
    ys, yw = R.tap_table(H, size[0], mode, size[0] < H if antialias is None else antialias)
    xs, xw = R.tap_table(W, size[1], mode, size[1] < W if antialias is None else antialias, wrap_x)
    return ys, yw, xs, xw


def misaligned_out(shape):
    """A contiguous fp32 view that starts one float past a 16-byte boundary."""
    n = int(np.prod(shape))
    flat = torch.full((n + 1,), -7.0, dtype=torch.float32, device=DEV)
    view = flat[1:].view(shape)
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("wrap_x", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{'x'.join(map(str, c[0]))}to{c[1][0]}x{c[1][1]}")
def test_resample_vs_float64_on_the_same_tables(ops, case, mode, wrap_x):
    shape, size = case
    x = _input(shape)
    ys, yw, xs, xw = _tables(shape, size, mode, wrap_x=wrap_x)
    ref = apply_tables(x.astype(np.float64), ys, yw.astype(np.float64), xs, xw.astype(np.float64), wrap_x=wrap_x)
    got = ops.resample(torch.tensor(x, device=DEV), size, mode, wrap_x=wrap_x)
    torch.cuda.synchronize()
    assert tuple(got.shape) == shape[:2] + size
    bound = parity_bound(yw, xw, np.abs(x).max())
    check(f"resample_{mode}_{'x'.join(map(str, shape))}_to_{size[0]}x{size[1]}_wrap{int(wrap_x)}", got, ref, max_abs=bound,
          taps=[int(xw.shape[1]), int(yw.shape[1])])


def test_antialias_can_be_forced_either_way(ops):
    """antialias=True on an upscale and False on a downscale are their own tables (torch's two definitions), not the default."""
    for shape, size, aa in (((1, 2, 8, 8), (16, 16), True), ((2, 3, 16, 12), (8, 6), False)):
        x = _input(shape, 4)
        ys, yw, xs, xw = _tables(shape, size, "bicubic", antialias=aa)
        ref = apply_tables(x.astype(np.float64), ys, yw.astype(np.float64), xs, xw.astype(np.float64))
        got = ops.resample(torch.tensor(x, device=DEV), size, "bicubic", antialias=aa)
        check(f"resample_bicubic_aa{int(aa)}_{size[0]}x{size[1]}", got, ref, max_abs=parity_bound(yw, xw, np.abs(x).max()))
        assert not torch.equal(got, ops.resample(torch.tensor(x, device=DEV), size, "bicubic"))


# ------------------------------------------------------------------------------------------------ bit-exact structure
@pytest.mark.parametrize("mode", MODES)
def test_same_size_returns_the_input(ops, mode):
    for shape in ((1, 4, 6, 10), (2, 4, 8, 16), (1, 2, 20, 72)):
        x = torch.tensor(_input(shape, 5), device=DEV)
        for wrap_x in (False, True):
            assert torch.equal(ops.resample(x, shape[2:], mode, wrap_x=wrap_x), x)


def test_nearest_x2_is_repeat_interleave(ops):
    for shape in ((2, 4, 8, 8), (1, 3, 5, 7), (1, 2, 20, 24)):
        x = torch.tensor(_input(shape, 6), device=DEV)
        got = ops.resample(x, (2 * shape[2], 2 * shape[3]), "nearest")
        assert torch.equal(got, x.repeat_interleave(2, 2).repeat_interleave(2, 3))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,s", [((2, 4, 8, 8), 2), ((1, 2, 6, 20), 2), ((1, 3, 8, 7), 3)])
def test_wrap_x_roll_identity(ops, mode, shape, s):
    """With wrap_x, at an integer scale, no column tap is clamped: rolling the input by k columns rolls the output by s * k, bit
    for bit (output j + s k reads the rolled input through the same weights in the same order).  Rows are resampled too; their
    clamps see the same values either way."""
    x = torch.tensor(_input(shape, 7), device=DEV)
    size = (2 * shape[2], s * shape[3])
    out = ops.resample(x, size, mode, wrap_x=True)
    for k in (1, 3, shape[3] - 1):
        assert torch.equal(ops.resample(torch.roll(x, k, -1).contiguous(), size, mode, wrap_x=True), torch.roll(out, s * k, -1))
    # and without wrap_x the edge replicates instead: the outermost columns differ from the wrapped ones
    if mode != "nearest":
        assert not torch.equal(ops.resample(x, size, mode)[..., 0], out[..., 0])


@pytest.mark.parametrize("mode", ["nearest", "bilinear", "bicubic"])
def test_replicate_edge_keeps_a_constant_row(ops, mode):
    """Without wrap_x, rows that are constant along x stay that constant in the first and last output columns (and everywhere),
    with torch.equal: at x2 and x4 the bilinear and bicubic (A = -0.75) weights are dyadic rationals that sum to exactly 1, and
    the row constants are multiples of 1/8, so every product and every partial sum of the fma chain is exact -- only a wrong edge
    rule (zero padding, wrapping) changes the bits.  Same-size rows, so the vertical pass is the identity.  Both store widths."""
    rows = torch.arange(-16, 16, dtype=torch.float32, device=DEV).view(2, 2, 8, 1) / 8.0
    x = rows.expand(2, 2, 8, 12).contiguous()
    for Wo in (24, 48):
        want = rows.expand(2, 2, 8, Wo)
        for out in (None, misaligned_out((2, 2, 8, Wo))):
            got = ops.resample(x, (8, Wo), mode, out=out)
            assert torch.equal(got[..., 0], want[..., 0]) and torch.equal(got[..., -1], want[..., -1]) and torch.equal(got, want)
    # the other modes' weights are not dyadic: the same property inside the derived parity bound
    for m, aa in (("lanczos3", None), ("bicubic", True)):
        ys, yw, xs, xw = _tables(x.shape, (8, 24), m, antialias=aa)
        got = ops.resample(x, (8, 24), m, antialias=aa)
        off_one = float(np.abs(xw.astype(np.float64).sum(1) - 1.0).max())        # the fp32 weights sum to 1 only to rounding
        assert float((got - rows).abs().max()) <= parity_bound(yw, xw, 2.0) + 2.0 * off_one


@pytest.mark.parametrize("case", CASES[:4], ids=lambda c: f"{'x'.join(map(str, c[0]))}to{c[1][0]}x{c[1][1]}")
def test_a_batch_is_its_samples_run_alone(ops, case):
    (_, C, H, W), size = case
    x = torch.tensor(_input((3, C, H, W), 8), device=DEV)
    for mode in ("bicubic", "lanczos3"):
        whole = ops.resample(x, size, mode)
        for b in range(3):
            assert torch.equal(whole[b:b + 1], ops.resample(x[b:b + 1].contiguous(), size, mode))


@pytest.mark.parametrize("mode", MODES)
def test_vector_and_scalar_stores_give_the_same_bits(ops, mode):
    """W_out = 16 into an aligned out (16-byte stores) and into a view of the same shape 4 bytes past alignment (scalar stores)."""
    for shape, size in (((2, 4, 8, 8), (16, 16)), ((1, 2, 20, 24), (40, 72))):
        x = torch.tensor(_input(shape, 9), device=DEV)
        vec = ops.resample(x, size, mode)
        assert vec.data_ptr() % 16 == 0
        out = misaligned_out(shape[:2] + size)
        assert ops.resample(x, size, mode, out=out) is out
        assert torch.equal(out, vec)


# ------------------------------------------------------------------------------------------------ the fused form
def _noised_outs(shape, misaligned):
    mk = misaligned_out if misaligned else (lambda s: torch.full(s, -7.0, dtype=torch.float32, device=DEV))
    return mk(shape), mk(shape)


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("case", [CASES[1], CASES[0], CASES[2], CASES[4]], ids=["vec16", "scalar25", "down", "tiles"])
def test_resample_noised_ties(ops, case, misaligned):
    """z0 at scale 1 is mdx_resample_f32's output; xt is randn_seeded + q_sample on z0 -- with a passed noise and with seeds, in
    both store widths; either output may be left out; scale 0.18215 is one fp32 multiply."""
    shape, size = case
    oshape = shape[:2] + size
    x = torch.tensor(_input(shape, 10), device=DEV)
    r = ops.resample(x, size, "bicubic")
    seeds = ops.seeds_tensor([11, 2 ** 63 + 5][:shape[0]], DEV)
    drawn = ops.randn_seeded(seeds, ops.RNG_ENCODE, 0, oshape[1:])
    given = torch.tensor(np.random.RandomState(12).randn(*oshape).astype(np.float32), device=DEV)
    for scale in (1.0, 0.18215):
        z_want = r if scale == 1.0 else r * torch.tensor(scale, dtype=torch.float32, device=DEV)
        for src, nz in (("noise", given), ("seeds", drawn)):
            kw = {"noise": given} if src == "noise" else {"seeds": seeds}
            z0, xt = _noised_outs(oshape, misaligned)
            got = ops.resample_noised(x, size, A, Bc, scale=scale, z0_out=z0, xt_out=xt, **kw)
            assert got[0] is z0 and got[1] is xt
            assert torch.equal(z0, z_want), (scale, src)
            assert torch.equal(xt, ops.q_sample(z0.clone(), nz, A, Bc)), (scale, src)
            # either output alone: the same bits
            only_z, none = ops.resample_noised(x, size, A, Bc, scale=scale, xt_out=False)
            assert none is None and torch.equal(only_z, z0)
            none, only_t = ops.resample_noised(x, size, A, Bc, scale=scale, z0_out=False,
                                               xt_out=_noised_outs(oshape, misaligned)[1], **kw)
            assert none is None and torch.equal(only_t, xt)
    # another stream / draw is another noise: the arguments reach the generator
    other = ops.resample_noised(x, size, A, Bc, seeds=seeds, stream=ops.RNG_X_T, draw=2)[1]
    assert torch.equal(other, ops.q_sample(r, ops.randn_seeded(seeds, ops.RNG_X_T, 2, oshape[1:]), A, Bc))


def test_resample_noised_wrapper_refusals(ops):
    from minddiffusion_amd._lib import MdxError
    x = torch.zeros(2, 4, 8, 8, device=DEV)
    seeds = ops.seeds_tensor([1, 2], DEV)
    with pytest.raises(MdxError, match="exactly one"):
        ops.resample_noised(x, (16, 16), 1.0, 0.0)
    with pytest.raises(MdxError, match="exactly one"):
        ops.resample_noised(x, (16, 16), 1.0, 0.0, noise=torch.zeros(2, 4, 16, 16, device=DEV), seeds=seeds)
    with pytest.raises(MdxError, match="no output"):
        ops.resample_noised(x, (16, 16), 1.0, 0.0, seeds=seeds, z0_out=False, xt_out=False)
    with pytest.raises(MdxError, match="seeds"):
        ops.resample_noised(x, (16, 16), 1.0, 0.0, seeds=ops.seeds_tensor([1, 2, 3], DEV))
    with pytest.raises(MdxError, match="noise"):
        ops.resample_noised(x, (16, 16), 1.0, 0.0, noise=torch.zeros(2, 4, 16, 15, device=DEV))
    with pytest.raises(MdxError, match="mode"):
        ops.resample(x, (16, 16), "area")
    with pytest.raises(MdxError, match="taps"):
        ops.resample(torch.zeros(1, 1, 128, 8, device=DEV), (8, 8), "bicubic")
    with pytest.raises(MdxError, match="GPU"):
        ops.resample(torch.zeros(1, 1, 8, 8), (16, 16))


# ------------------------------------------------------------------------------------------------ footprint
@pytest.mark.parametrize("case", [CASES[1], CASES[0], CASES[4], CASES[5]], ids=["vec16", "scalar25", "tiles_vec", "tiles_scalar"])
def test_footprint(ops, case):
    """Guard bands around out, z0_out and xt_out keep their bits, every payload element is written, and the input and the
    tables are what they were."""
    shape, size = case
    oshape = shape[:2] + size
    x = torch.tensor(_input(shape, 13), device=DEV)
    keep = x.clone()
    ops.resample(x, size, "bicubic")                                 # (uploads the tables)
    tables = [t for key, pair in ops._TAP_TABLES.items() for t in pair]
    before = [t.clone() for t in tables]
    buf, view = G.guarded(oshape, dtype=torch.float32)
    ops.resample(x, size, "bicubic", out=view)
    G.assert_footprint(buf, view, "resample", written=True)
    seeds = ops.seeds_tensor(list(range(shape[0])), DEV)
    bz, vz = G.guarded(oshape, dtype=torch.float32)
    bt, vt = G.guarded(oshape, dtype=torch.float32)
    ops.resample_noised(x, size, A, Bc, scale=0.5, seeds=seeds, z0_out=vz, xt_out=vt)
    G.assert_footprint(bz, vz, "resample_noised z0", written=True)
    G.assert_footprint(bt, vt, "resample_noised xt", written=True)
    assert torch.equal(x, keep) and all(torch.equal(a, b) for a, b in zip(tables, before))


# ------------------------------------------------------------------------------------------------ refusals launch nothing
def test_refusals_return_invalid_and_launch_nothing(ops):
    from minddiffusion_amd import _lib
    from minddiffusion_amd._lib import MdxError
    lib = _lib.load()
    x = torch.tensor(_input((2, 4, 8, 8), 14), device=DEV)
    ys, yw, xs, xw = (torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in _tables(x.shape, (16, 16), "bicubic"))
    out = torch.full((2, 4, 16, 16), G.SENT, dtype=torch.float32, device=DEV)
    z0, xt = out.clone(), out.clone()
    noise = torch.zeros_like(out)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def plain(inp=x, o=out, B=2, C=4, Hi=8, Wi=8, Ho=16, Wo=16, y_s=ys, y_w=yw, Ty=4, x_s=xs, x_w=xw, Tx=4):
        return lib.mdx_resample_f32(p(inp), p(o), B, C, Hi, Wi, Ho, Wo, p(y_s), p(y_w), Ty, p(x_s), p(x_w), Tx, 0, stream)

    def noised(inp=x, Ho=16, Tx=4, nz=noise, sd=None, z=z0, t=xt):
        return lib.mdx_resample_noised_f32(p(inp), 2, 4, 8, 8, Ho, 16, p(ys), p(yw), 4, p(xs), p(xw), Tx, 0, 1.0, 0.8, 0.6, p(nz),
                                           p(sd), 3, 0, p(z), p(t), stream)
    bad_plain = [dict(inp=None), dict(o=None), dict(y_s=None), dict(y_w=None), dict(x_s=None), dict(x_w=None), dict(B=0),
                 dict(C=0), dict(Hi=0), dict(Wi=-1), dict(Ho=0), dict(Wo=0), dict(Tx=0), dict(Tx=33), dict(Ty=0), dict(Ty=33),
                 dict(inp=out), dict(Hi=2100, Ho=100, Ty=1)]
    for kw in bad_plain:
        assert plain(**kw) == -1, kw
    bad_noised = [dict(inp=None), dict(Ho=0), dict(Tx=33), dict(z=None, t=None), dict(nz=None), dict(inp=z0), dict(inp=xt),
                  dict(z=xt), dict(nz=xt), dict(nz=z0)]
    for kw in bad_noised:
        assert noised(**kw) == -1, kw
    torch.cuda.synchronize()
    sent = torch.full_like(out, G.SENT)
    assert torch.equal(out, sent) and torch.equal(z0, sent) and torch.equal(xt, sent)
    # the very large downscale, through the wrapper: the message says what it is
    with pytest.raises(MdxError, match="very large downscale"):
        ops.resample(torch.zeros(1, 1, 2100, 4, device=DEV), (100, 4), "nearest")
    # and the same arguments, unbroken, do launch
    assert plain() == 0 and noised() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ops.resample(x, (16, 16), "bicubic")) and torch.equal(z0, out)
