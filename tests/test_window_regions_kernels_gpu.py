"""mdx_window_gather_rows_f32 and mdx_window_average_regions_f16 (csrc/window.hip; they share their kernels with the two plain
entries, which are held equal to them here) on the GPU.  The gather is a copy: torch.equal
to torch.roll plus slicing, with a window that straddles the seam, in its float4 and its scalar form, for a row table with
repeats and for a sub-range, with a NaN sentinel around what it may write.  The average without regions is held bit for bit to
the numpy restatement of the stated arithmetic (wrapped) and to the existing entry (not wrapped; and with one all-ones region);
with regions every element is held to ulp16 / 2 + (2 T + 3) 2^-24 sum |q e| / sum q around the float64 mean -- half an fp16
ulp for the one rounding to fp16, plus the fp32 accumulation bound: one rounding per multiply, fma, add and divide, which
matters only where terms cancel.  (tests/test_windowed_regions_cpu.py confirms that bound for a float32 emulation of the
arithmetic on these inputs.)"""
import numpy as np
import pytest
import torch

import _window_regions_util as RU
import _window_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WRAPPED = ["grid2d", "odd3", "seam4"]


def grid_of(name):
    from minddiffusion_amd import ops
    shape, s, wrap = RU.CANVASES[name]
    return ops.WindowGrid(shape[2:], (8, 8), (4, s), wrap_x=wrap), shape


def plan_of(name, kind):
    from minddiffusion_amd import ops
    g, shape = grid_of(name)
    win, pairs, masks = RU.pair_outputs(name, kind)
    plan = ops.RegionPlan(g, masks)
    assert plan.pairs == pairs
    return g, shape, plan, win, masks


# ------------------------------------------------------------------------------------------------ gather by rows
@pytest.mark.parametrize("name", WRAPPED)
def test_gather_rows_is_roll_plus_slice(name):
    from minddiffusion_amd import ops
    g, shape = grid_of(name)
    assert g.ox == {"seam4": [0, 4, 8, 12, 16], "odd3": [0, 3, 6, 9, 12, 15], "grid2d": [0, 4, 8, 12, 16]}[name]
    assert g.ny == (2 if name == "grid2d" else 1) and g.ox[-1] + 8 > shape[3]           # the last window straddles the seam
    x = torch.randn(shape, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    got = ops.window_gather_rows(x, g, range(g.N))
    assert tuple(got.shape) == (shape[0] * g.N, shape[1], 8, 8)
    assert torch.equal(got, RU.gather_rows_ref(x, g.oy, g.ox, 8, 8, range(g.N)))
    half = shape[0] // 2                                  # a [uncond ; cond] canvas batch stays a [uncond ; cond] window batch
    x[half:] = x[:half]
    got = ops.window_gather_rows(x, g, range(g.N))
    assert torch.equal(got[:half * g.N], got[half * g.N:])


@pytest.mark.parametrize("name", WRAPPED)
def test_gather_rows_with_repeats_and_a_sub_range_writes_its_rows_only(name):
    from minddiffusion_amd import ops
    g, shape = grid_of(name)
    x = torch.randn(shape, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    last = g.N - 1
    for rows in ([last, 0, last, last, 1], [g.nx - 1], list(range(1, 4)), ops.WindowRows([2, 2])):
        ids = rows.host.tolist() if isinstance(rows, ops.WindowRows) else rows
        n = shape[0] * len(ids)
        buf = torch.full((n + 2, shape[1], 8, 8), float("nan"), device=DEV)
        ops.window_gather_rows(x, g, rows, out=buf[1:1 + n])
        assert torch.equal(buf[1:1 + n], RU.gather_rows_ref(x, g.oy, g.ox, 8, 8, ids)), ids
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())


def test_the_two_gather_rows_forms_move_the_same_bits():
    from minddiffusion_amd import ops
    g, shape = grid_of("seam4")
    store = torch.randn(shape[0] * shape[1] * 8 * 20 + 1, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    y = store[1:].view(shape)                           # 4 bytes off a 16-byte boundary: the scalar form
    x = y.clone()                                       # the same values in an allocation of their own: the float4 form
    assert y.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    want = ops.window_gather_rows(x, g, range(g.N))
    assert torch.equal(ops.window_gather_rows(y, g, range(g.N)), want)
    assert torch.equal(want, RU.gather_rows_ref(y, g.oy, g.ox, 8, 8, range(g.N)))


def test_gather_rows_on_a_clamped_grid_is_the_existing_gather():
    from minddiffusion_amd import ops
    g, shape = grid_of("clamped")
    x = torch.randn(shape, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    assert torch.equal(ops.window_gather_rows(x, g, range(1, 4)), ops.window_gather(x, g, 1, 3))


@pytest.mark.parametrize("Wc,misalign", [(20, False), (18, False), (20, True)])
def test_a_range_and_its_row_table_gather_the_same_bits(Wc, misalign):
    """The two gather entries share one kernel: a proper sub-range, and the row table that names it, on a grid the float4 form
    takes (x offsets 0 4 8 12), on one it cannot take (0 4 8 10), and on the first with the canvas 4 bytes off a 16-byte
    boundary (the scalar form again); a NaN row before and after what may be written stays NaN."""
    from minddiffusion_amd import ops
    shape = (2, 4, 8, Wc)
    g = ops.WindowGrid(shape[2:], (8, 8), (4, 4))
    assert g.ox == ([0, 4, 8, 12] if Wc == 20 else [0, 4, 8, 10]) and g.N == 4
    store = torch.randn(2 * 4 * 8 * Wc + 1, device=DEV, generator=torch.Generator(DEV).manual_seed(7))
    x = store[1:].view(shape) if misalign else store[1:].view(shape).clone()
    assert x.data_ptr() % 16 == (4 if misalign else 0)
    k0, n = 1, 2
    bufs = torch.full((2, 2 * n + 2, 4, 8, 8), float("nan"), device=DEV)
    ops.window_gather(x, g, k0, n, out=bufs[0, 1:1 + 2 * n])
    ops.window_gather_rows(x, g, range(k0, k0 + n), out=bufs[1, 1:1 + 2 * n])
    assert torch.equal(bufs[0, 1:-1], bufs[1, 1:-1]) and torch.equal(bufs[0, 1:-1], U.gather_ref(x, g.oy, g.ox, 8, 8, k0, n))
    assert bool(torch.isnan(bufs[:, 0]).all()) and bool(torch.isnan(bufs[:, -1]).all())


# ------------------------------------------------------------------------------------------------ the uniform wrapped average
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", WRAPPED)
def test_wrapped_average_without_regions(name, weighted):
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.windowed import gaussian_weights
    g, shape = grid_of(name)
    win = np.random.RandomState(len(name)).randn(shape[0] * g.N, 64, 8).astype(np.float16)
    cnt = RU.coverage(g.oy, g.ox, 8, 8, g.Hc, g.Wc)
    assert np.array_equal(cnt, g.coverage())
    if name != "odd3":                                  # Wc % s == 0: every pixel of a row band has the count w / s
        assert all(len(set(row.tolist())) == 1 for row in cnt) and cnt[0, 0] == 2
    if not weighted:
        got = ops.window_average_regions(torch.from_numpy(win).to(DEV), g, 4).cpu().numpy()
        want, cnt_ref = RU.average_wrap_ref(win, g.oy, g.ox, 8, 8, g.Hc, g.Wc, 4)
        print(f"{name}: counts {sorted(set(cnt.ravel().tolist()))}, differing elements {int((got != want).sum())}")
        assert np.array_equal(cnt, cnt_ref) and np.array_equal(got.view(np.uint16), want.view(np.uint16))
        return
    wts = gaussian_weights(8, 8)
    got = ops.window_average_regions(torch.from_numpy(win).to(DEV), g, 4, weights=wts.to(DEV)).cpu().numpy()
    pairs, ones = [(k, 0) for k in range(g.N)], np.ones((1, g.Hc, g.Wc), np.float32)
    ref, T, mag = RU.region_ref64(win, pairs, ones, wts.numpy(), g.oy, g.ox, 8, 8, 4)
    got = got.reshape(ref.shape)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= RU.region_bound(got, ref, T, mag)) and np.array_equal(T, cnt)


# ------------------------------------------------------------------------------------------------ the existing entry
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape,stride", [((4, 4, 8, 20), (4, 4)), ((4, 4, 8, 18), (4, 4)), ((2, 9, 12, 20), (4, 4))])
def test_no_regions_and_one_all_ones_region_are_the_existing_entry_bit_for_bit(shape, stride, weighted):
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.windowed import gaussian_weights
    g = ops.WindowGrid(shape[2:], (8, 8), stride)
    win = torch.from_numpy(np.random.RandomState(shape[3]).randn(shape[0] * g.N, 64, 8).astype(np.float16)).to(DEV)
    wts = gaussian_weights(8, 8).to(DEV) if weighted else None
    want = ops.window_average(win, g, 4, weights=wts)
    assert torch.equal(ops.window_average_regions(win, g, 4, weights=wts), want)             # R == 0
    plan = ops.RegionPlan(g, torch.ones(1, *shape[2:]))
    assert plan.pairs == [(k, 0) for k in range(g.N)]
    assert torch.equal(ops.window_average_regions(win, g, 4, plan=plan, weights=wts), want)  # R == 1, M == 1
    assert bool(torch.isfinite(want).all())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ld,C", [(8, 4), (16, 4), (16, 11)])
def test_the_two_average_entries_agree_on_wider_rows_of_a_two_row_grid(ld, C, weighted):
    """The two average entries share one kernel: ld == 16 is two 16-byte chunks per pixel, C == 11 ends inside the second."""
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.windowed import gaussian_weights
    g = ops.WindowGrid((12, 20), (8, 8), (4, 4))
    assert (g.ny, g.nx) == (2, 4)
    win = torch.from_numpy(np.random.RandomState(ld + C).randn(2 * g.N, 64, ld).astype(np.float16)).to(DEV)
    wts = gaussian_weights(8, 8).to(DEV) if weighted else None
    want = ops.window_average(win, g, C, weights=wts)
    assert torch.equal(ops.window_average_regions(win, g, C, weights=wts), want)
    assert bool(torch.isfinite(want).all()) and want[..., :C].any() and not want[..., C:].any()


# ------------------------------------------------------------------------------------------------ the wrapper's shared buffers
def test_plain_and_region_calls_on_one_wrapper_do_not_leak_into_each_other():
    """A plain clamped call in several chunks, a region call and a plain call again on ONE WindowedDiffusion -- they share the
    chunk loop, the staging buffer and the input buffers -- are each what a fresh wrapper gives, bit for bit."""
    import _vpred_util as V
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    model, cfg, _ = V.tiny_eps_model()
    gen = torch.Generator(DEV).manual_seed(11)
    x = torch.randn((1, 4, 8, 32), device=DEV, generator=gen)
    x_in, t = torch.cat([x, x]).contiguous(), torch.full((2,), 500., device=DEV)
    ctxs = [torch.randn((2, V.T, cfg["context_dim"]), device=DEV, generator=gen).half() for _ in range(3)]
    masks = RU.region_masks("ramp", 8, 32)
    masks[2, :, 16:] = 0.0                                            # the third region touches the left windows only
    new = lambda: WindowedDiffusion(model, (8, 8), (4, 4), max_unet_batch=8)

    def plain(wm):
        out = wm.apply_model_nhwc(x_in, t, ctxs[0], cfg_dup=True).clone()
        assert wm.chunks == [(0, 4), (4, 3)] and wm.pairs == [(k, None) for k in range(7)] and not wm.grid.wrap_x
        return out

    def regions(wm):
        with wm.regions(torch.from_numpy(masks), ctxs):
            out = wm.apply_model_nhwc(x_in, t, ctxs[0], cfg_dup=True).clone()
        assert wm.pairs == RU.pair_list(masks, wm.grid.oy, wm.grid.ox, 8, 8) and 7 < len(wm.pairs) < 21 and len(wm.chunks) > 1
        return out

    wm = new()
    first, both, again = plain(wm), regions(wm), plain(wm)
    assert wm.evals == 3 and torch.equal(first, plain(new())) and torch.equal(both, regions(new())) and torch.equal(again, first)
    assert not torch.equal(both, first) and bool(torch.isfinite(both).all())


# ------------------------------------------------------------------------------------------------ regions
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["stripes", "ramp"])
@pytest.mark.parametrize("name", sorted(RU.CANVASES))
def test_region_average_is_within_the_bound_of_the_float64_mean(name, kind, weighted):
    """Every element: |got - ref64| <= ulp16 / 2 + (2 T + 3) 2^-24 sum |q e| / sum q; ulp16 the fp16 spacing at
    max(|got|, |ref64|), T the pixel's term count."""
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.windowed import gaussian_weights
    g, shape, plan, win, masks = plan_of(name, kind)
    wts = gaussian_weights(8, 8) if weighted else None
    got = ops.window_average_regions(torch.from_numpy(win).to(DEV), g, 4, plan=plan,
                                     weights=None if wts is None else wts.to(DEV)).cpu().numpy()
    ref, T, mag = RU.region_ref64(win, plan.pairs, masks, None if wts is None else wts.numpy(), g.oy, g.ox, 8, 8, 4)
    assert got.dtype == np.float16 and got.shape == (shape[0], g.Hc * g.Wc, 8)
    got4 = got.reshape(ref.shape)
    err = np.abs(got4.astype(np.float64) - ref)
    bound = RU.region_bound(got4, ref, T, mag)
    with np.errstate(over="ignore"):
        off = int((got4 != ref.astype(np.float16)).sum())
    print(f"{name} {kind} weighted={weighted}: P={plan.P}, T up to {T.max()}, {off} of {err.size} elements differ from the "
          f"rounded float64 mean, worst err / bound {float((err / bound).max()):.3f}")
    assert err.shape == bound.shape == got4.shape and np.all(err <= bound)      # no element is left out
    assert not got4[..., 4:].any()                                              # pad channels are 0
    # a pixel with one non-zero term is that window row's halves bit for bit
    e = win.reshape(shape[0], plan.P, 8, 8, 8)
    ys, xs = np.nonzero(T == 1)
    assert len(ys) > 0 or not (name == "clamped" and kind == "stripes")
    terms = RU.region_terms(plan.pairs, masks, None if wts is None else wts.numpy(), g.oy, g.ox, 8, 8)
    for y, x in zip(ys, xs):
        hit = [(p, int(np.nonzero(rows == y)[0][0]), int(np.nonzero(cols == x)[0][0])) for p, (rows, cols, q) in enumerate(terms)
               if y in rows and x in cols and q[np.nonzero(rows == y)[0][0], np.nonzero(cols == x)[0][0]] > 0]
        (p, yy, xx), = hit
        assert np.array_equal(got4[:, y, x, :4].view(np.uint16), e[:, p, yy, xx, :4].view(np.uint16))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", sorted(RU.CANVASES))
def test_the_nan_footprint_of_a_pair_is_where_its_q_is_positive(name, weighted):
    """A pair row filled with NaN reaches exactly the pixels where its q > 0: a pixel where its mask is zero stays finite (the
    term is skipped before the row is read); the inputs and what lies around the output keep their bits."""
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.windowed import gaussian_weights
    g, shape, plan, win, masks = plan_of(name, "stripes")
    NB = shape[0]
    wts = gaussian_weights(8, 8).to(DEV) if weighted else None
    terms = RU.region_terms(plan.pairs, masks, None, g.oy, g.ox, 8, 8)
    cut = 0                                                             # pairs whose stripe cuts through their window
    for p in (0, plan.P // 2, plan.P - 1):
        w = torch.from_numpy(win).to(DEV)
        w.view(NB, plan.P, 64, 8)[1, p] = float("nan")
        before = w.clone()
        buf = torch.full((NB + 2, g.Hc * g.Wc, 8), 7.0, dtype=torch.float16, device=DEV)
        ops.window_average_regions(w, g, 4, plan=plan, out=buf[1:1 + NB], weights=wts)
        assert torch.equal(w.view(torch.int16), before.view(torch.int16))
        assert bool((buf[0] == 7.0).all()) and bool((buf[-1] == 7.0).all())
        nan = torch.isnan(buf[1:1 + NB, :, :4]).all(-1).view(NB, g.Hc, g.Wc).cpu().numpy()
        anynan = torch.isnan(buf[1:1 + NB]).any(-1).view(NB, g.Hc, g.Wc).cpu().numpy()
        rows, cols, q = terms[p]
        want = np.zeros((NB, g.Hc, g.Wc), bool)
        want[1][np.ix_(rows, cols)] = q > 0
        assert (q > 0).any()
        cut += bool((q == 0).any())
        assert np.array_equal(nan, want) and np.array_equal(anynan, want)
        assert bool((buf[1:1 + NB, :, 4:] == 0).all())
    assert cut >= 2


def test_wider_rows_are_averaged_chunk_by_chunk():
    from minddiffusion_amd import ops
    g, shape, plan, _, masks = plan_of("odd3", "ramp")
    win = np.random.RandomState(9).randn(2 * plan.P, 64, 16).astype(np.float16)
    got = ops.window_average_regions(torch.from_numpy(win).to(DEV), g, 11, plan=plan).cpu().numpy()
    ref, T, mag = RU.region_ref64(win, plan.pairs, masks, None, g.oy, g.ox, 8, 8, 11)
    got = got.reshape(ref.shape)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= RU.region_bound(got, ref, T, mag)) and not got[..., 11:].any()
    assert got[..., 8:11].any()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    g, shape, plan, win, masks = plan_of("seam4", "stripes")
    x = torch.zeros(shape, device=DEV)
    w = torch.from_numpy(win).to(DEV)
    with pytest.raises(MdxError, match="expected torch.float32"):
        ops.window_gather_rows(x.half(), g, [0])
    with pytest.raises(MdxError, match="canvas: shape"):
        ops.window_gather_rows(x[:, :, :, :16].contiguous(), g, [0])
    with pytest.raises(MdxError, match="out: shape"):
        ops.window_gather_rows(x, g, [0, 1], out=torch.zeros(4, 4, 8, 8, device=DEV))
    for rows in ([], [5], [-1, 0]):
        with pytest.raises(MdxError, match="not inside the grid"):
            ops.window_gather_rows(x, g, rows)
    with pytest.raises(MdxError, match="wrapped grid"):
        ops.window_gather(x, g)
    with pytest.raises(MdxError, match="wrapped grid"):
        ops.window_average(w, g, 4)
    with pytest.raises(MdxError, match="windows: shape"):
        ops.window_average_regions(w[:-1], g, 4, plan=plan)
    with pytest.raises(MdxError, match="windows: shape"):
        ops.window_average_regions(w, g, 4)                           # P rows, not N, without the plan
    with pytest.raises(MdxError, match="expected torch.float16"):
        ops.window_average_regions(w.float(), g, 4, plan=plan)
    with pytest.raises(MdxError, match="ld must be"):
        ops.window_average_regions(w, g, 9, plan=plan)
    with pytest.raises(MdxError, match="weights: shape"):
        ops.window_average_regions(w, g, 4, plan=plan, weights=torch.ones(64, device=DEV))
    with pytest.raises(MdxError, match="out: shape"):
        ops.window_average_regions(w, g, 4, plan=plan, out=torch.zeros(shape[0], 160, 16, dtype=torch.float16, device=DEV))
    with pytest.raises(MdxError, match="another grid"):
        ops.window_average_regions(w, grid_of("seam4")[0], 4, plan=plan)
    bad, _ = grid_of("seam4")
    bad.host[5] = 20                                    # the host table is what is checked: refused before any launch
    with pytest.raises(MdxError, match="an offset leaves the canvas"):
        ops.window_gather_rows(x, bad, [0])
    bad_plan = ops.RegionPlan(g, masks)
    bad_plan.pair_region.host[1] = 7
    with pytest.raises(MdxError, match="is region 7 of 3"):
        ops.window_average_regions(w, g, 4, plan=bad_plan)
