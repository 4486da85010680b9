"""mdx_tile_blend_f32 on the GPU, bit for bit against the numpy float32 restatement of its arithmetic (tests/_tile_util.py):
the vector and the scalar form, 2-, 3- and 4-fold cover, ramps 1 / 4 / 8, both modes, misaligned bases, a wrapped grid, more than
one pass of the grid-stride loop, and the footprint (only `out` is written)."""
import numpy as np
import pytest
import torch

import _tile_util as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NB, C, TH, TW = 2, 3, 8, 8

# (canvas, stride): the x offsets are (0, 4, 8, 12) -- 16-byte lanes -- or (0, 3, 6, 9, 12) -- single floats
GRIDS = {"vec_2fold": ((8, 20), (4, 4)), "vec_4fold": ((12, 20), (4, 4)), "scalar_3fold": ((8, 20), (4, 3))}


def _grid(name, wrap=False):
    from minddiffusion_amd import ops
    canvas, stride = GRIDS[name]
    g = ops.WindowGrid(canvas, (TH, TW), stride, wrap_x=wrap)
    assert g.oy == T.offsets(canvas[0], TH, stride[0]) and g.ox == T.offsets(canvas[1], TW, stride[1], wrap)
    return g


def _tiles(n, seed, shape=(C, TH, TW)):
    """Values around [-1.5, 1.5]: MDX_TILE_UNIT clamps on both sides."""
    return (np.random.RandomState(seed).standard_normal((n,) + shape) * 0.8).astype(np.float32)


def _offset_view(t, by):
    """The same values at a base `by` floats past a fresh allocation's."""
    flat = torch.empty(t.numel() + by, dtype=t.dtype, device=t.device)
    view = flat[by:].view(t.shape)
    view.copy_(t)
    return view


def test_the_grids_are_the_ones_the_cases_name():
    assert _grid("vec_2fold").ox == [0, 4, 8, 12] and _grid("vec_2fold").oy == [0]
    assert _grid("vec_4fold").oy == [0, 4] and int(_grid("vec_4fold").coverage().max()) == 4
    assert _grid("scalar_3fold").ox == [0, 3, 6, 9, 12] and int(_grid("scalar_3fold").coverage().max()) == 3
    assert int(_grid("vec_2fold").coverage().max()) == 2 and int(_grid("vec_2fold").coverage().min()) == 1


@pytest.mark.parametrize("mode", ["raw", "unit"])
@pytest.mark.parametrize("ramp", [1, 4, 8])
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_bits(name, ramp, mode):
    from minddiffusion_amd import ops
    g = _grid(name)
    tiles = _tiles(NB * g.N, 7 + ramp)
    ref, cnt = T.blend_ref(tiles, g.oy, g.ox, g.Hc, g.Wc, ramp, ramp, mode)
    assert np.array_equal(cnt, g.coverage())
    td = torch.tensor(tiles, device=DEV)
    got = ops.tile_blend(td, g, ramp, mode=mode)
    assert got.dtype == torch.float32 and tuple(got.shape) == (NB, C, g.Hc, g.Wc)
    assert torch.equal(got.cpu(), torch.from_numpy(ref))
    raw = ops.tile_blend(td, g, ramp)
    if mode == "unit":
        assert torch.equal(got, torch.clamp((raw + 1.0) / 2.0, 0.0, 1.0))
        assert float(got.min()) == 0.0 and float(got.max()) == 1.0           # both clamps are exercised
    # single-cover pixels are the tile's own bits (tile 0 owns the canvas' top-left pixel in every grid here)
    single = torch.from_numpy(cnt == 1)
    assert bool(single[0, 0]) and torch.equal(raw[:, :, 0, 0].cpu(), torch.from_numpy(tiles.reshape(NB, g.N, C, TH, TW)[:, 0, :, 0, 0]))
    gathered = T.gather_ref(raw.cpu(), g.oy, g.ox, TH, TW).reshape(NB, g.N, C, TH, TW)
    for k, (a, b) in enumerate((a, b) for a in g.oy for b in g.ox):
        own = single[a:a + TH, b:b + TW]
        assert torch.equal(gathered[:, k][..., own], torch.from_numpy(tiles.reshape(NB, g.N, C, TH, TW)[:, k])[..., own])


def test_different_ramps_per_axis_and_an_out_argument():
    from minddiffusion_amd import ops
    g = _grid("vec_4fold")
    tiles = _tiles(NB * g.N, 3)
    ref, _ = T.blend_ref(tiles, g.oy, g.ox, g.Hc, g.Wc, 2, 3)
    out = torch.full((NB, C, g.Hc, g.Wc), float("nan"), device=DEV)
    assert ops.tile_blend(torch.tensor(tiles, device=DEV), g, (2, 3), out=out) is out
    assert torch.equal(out.cpu(), torch.from_numpy(ref))


@pytest.mark.parametrize("which", ["tiles", "out", "both"])
@pytest.mark.parametrize("mode", ["raw", "unit"])
def test_a_misaligned_base_takes_the_scalar_form(which, mode):
    """A base one float past a 16-byte boundary cannot take 16-byte accesses: the same bits from the scalar form."""
    from minddiffusion_amd import ops
    g = _grid("vec_4fold")
    tiles = _tiles(NB * g.N, 11)
    ref, _ = T.blend_ref(tiles, g.oy, g.ox, g.Hc, g.Wc, 4, 4, mode)
    td = torch.tensor(tiles, device=DEV)
    out = torch.empty((NB, C, g.Hc, g.Wc), dtype=torch.float32, device=DEV)
    if which in ("tiles", "both"):
        td = _offset_view(td, 1)
        assert td.data_ptr() % 16 == 4 and td.is_contiguous()
    if which in ("out", "both"):
        out = _offset_view(out, 1)
        assert out.data_ptr() % 16 == 4
    ops.tile_blend(td, g, 4, out=out, mode=mode)
    assert torch.equal(out.cpu(), torch.from_numpy(ref))


@pytest.mark.parametrize("stride,form", [(4, "vector"), (3, "scalar")])
@pytest.mark.parametrize("mode", ["raw", "unit"])
def test_a_wrapped_grid(stride, form, mode):
    from minddiffusion_amd import ops
    g = ops.WindowGrid((12, 16), (TH, TW), (4, stride), wrap_x=True)
    assert g.ox == list(range(0, 16, stride)) == T.offsets(16, TW, stride, wrap=True) and g.oy == [0, 4]
    tiles = _tiles(NB * g.N, 5)
    ref, cnt = T.blend_ref(tiles, g.oy, g.ox, g.Hc, g.Wc, 4, 4, mode)
    assert np.array_equal(cnt, g.coverage()) and cnt.min() >= 2          # every column lies under two tiles or more
    got = ops.tile_blend(torch.tensor(tiles, device=DEV), g, 4, mode=mode)
    assert torch.equal(got.cpu(), torch.from_numpy(ref))


def test_wrap_equivariance():
    """One tile row, Wc = 16, TW = 8, offsets (0, 4, 8, 12): every pixel has two terms, and two fp32 terms commute -- rolling
    the tile set by one tile rolls the output by 4 columns, bit for bit."""
    from minddiffusion_amd import ops
    g = ops.WindowGrid((8, 16), (TH, TW), (8, 4), wrap_x=True)
    assert g.ox == [0, 4, 8, 12] and g.ny == 1 and int(g.coverage().min()) == int(g.coverage().max()) == 2
    tiles = torch.tensor(_tiles(NB * g.N, 9), device=DEV)
    rolled = tiles.reshape(NB, g.N, C, TH, TW).roll(1, dims=1).reshape(NB * g.N, C, TH, TW).contiguous()
    for mode in ("raw", "unit"):
        for ramp in (1, 4):
            a = ops.tile_blend(tiles, g, ramp, mode=mode)
            b = ops.tile_blend(rolled, g, ramp, mode=mode)
            assert torch.equal(b, a.roll(4, dims=-1))
    assert not torch.equal(a, b)


def test_more_than_one_pass_of_the_grid_stride_loop():
    """2 x 3 x 384 x 512 outputs are 294 912 four-column items, above the 4096 x 64 lanes of the capped grid."""
    from minddiffusion_amd import ops
    g = ops.WindowGrid((384, 512), (256, 256), (128, 128))
    assert NB * C * g.Hc * g.Wc // 4 > 4096 * 64 and g.N == 6
    tiles = _tiles(NB * g.N, 13, (C, 256, 256))
    ref, _ = T.blend_ref(tiles, g.oy, g.ox, g.Hc, g.Wc, 128, 128, "unit")
    got = ops.tile_blend(torch.tensor(tiles, device=DEV), g, 128, mode="unit")
    assert torch.equal(got.cpu(), torch.from_numpy(ref))


@pytest.mark.parametrize("name,shift", [("vec_4fold", 0), ("scalar_3fold", 0), ("vec_4fold", 1)])
def test_footprint(name, shift):
    """`out` sits between NaN guard bands: the bands stay NaN, every element of out is written, `tiles` keeps its bits."""
    from minddiffusion_amd import ops
    g = _grid(name)
    tiles = torch.tensor(_tiles(NB * g.N, 17), device=DEV)
    before = tiles.clone()
    n, band = NB * C * g.Hc * g.Wc, 1024 + shift
    buf = torch.full((band + n + 1024,), float("nan"), device=DEV)
    out = buf[band:band + n].view(NB, C, g.Hc, g.Wc)
    assert out.data_ptr() % 16 == 4 * shift
    ops.tile_blend(tiles, g, 4, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:band]).all()) and bool(torch.isnan(buf[band + n:]).all())
    assert not bool(torch.isnan(out).any())
    assert torch.equal(tiles, before)
    ref, _ = T.blend_ref(before.cpu().numpy(), g.oy, g.ox, g.Hc, g.Wc, 4, 4)
    assert torch.equal(out.cpu(), torch.from_numpy(ref))


def test_refusals_launch_nothing():
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    g = _grid("vec_2fold")
    tiles = torch.tensor(_tiles(NB * g.N, 1), device=DEV)
    out = torch.full((NB, C, g.Hc, g.Wc), float("nan"), device=DEV)
    for kw in ({"ramp": 0}, {"ramp": (4, 4097)}, {"ramp": 4, "mode": "uint8"}):
        with pytest.raises(MdxError):
            ops.tile_blend(tiles, g, out=out, **kw)
    with pytest.raises(MdxError, match="tiles"):
        ops.tile_blend(tiles[:-1], g, 4, out=out)
    with pytest.raises(MdxError, match="out"):
        ops.tile_blend(tiles, g, 4, out=out[:, :, :, :-4].contiguous())
    with pytest.raises(MdxError):
        ops.tile_blend(tiles.half(), g, 4)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
