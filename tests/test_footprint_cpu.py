"""Host-side half of the footprint tests: the guard helper (tests/_guard.py) on CPU tensors, and the coverage of the GEMM / conv case
table of tests/test_footprint_gpu.py -- every row resolved on the host (mdx_gemm_check / mdx_gemm_query launch nothing and never
dereference a pointer), no row refused, every row resolving to the launch form it names, and every supported cell of the matrix
{launch form} x {M tail, N tail, strided out_ld, unsplit, ticket reduce, reduce kernel} filled.  The cells a form does not support
are listed with what the library answers when asked for them (two refusals, seven silent redirections to another form), and that
answer is checked too."""
import re

import numpy as np
import pytest
import torch

import _guard as G
from _footprint_cases import case, expected_query, make_desc, out_hw, out_ld, width


# --------------------------------------------------------------------------- the helper
def test_guard_reports_writes_into_either_pad():
    for dtype in (torch.float16, torch.float32):
        buf, view = G.guarded((5, 24), dtype, device="cpu")
        assert view.shape == (5, 24) and bool((view == G.SENT).all()) and buf.numel() >= 5 * 24 + 2 * 4096
        view.fill_(1.0)
        G.assert_footprint(buf, view, "clean", written=True)
        first = view.storage_offset()
        buf[first - 1] = 0.5
        with pytest.raises(AssertionError, match="in front of its output"):
            G.assert_footprint(buf, view, "front")
        buf[first - 1] = G.SENT
        buf[first + view.numel()] = 0.5
        with pytest.raises(AssertionError, match="behind its output"):
            G.assert_footprint(buf, view, "behind")
        buf[first + view.numel()] = G.SENT
        buf[0] = float("nan")                     # a NaN is not the sentinel either
        with pytest.raises(AssertionError, match="in front"):
            G.assert_footprint(buf, view, "nan")


def test_guard_reports_a_write_into_a_stride_gap_and_an_unwritten_element():
    buf, view = G.guarded((2, 3, 8), torch.float16, strides=(3 * 16 + 32, 16, 1), device="cpu")
    view.fill_(2.0)
    G.assert_footprint(buf, view, "clean", written=True)
    off = view.storage_offset()
    buf[off + 8] = 2.0                            # column 8 of row 0: between N = 8 and out_ld = 16
    with pytest.raises(AssertionError, match="stride gap"):
        G.assert_footprint(buf, view, "column gap")
    buf[off + 8] = G.SENT
    buf[off + 3 * 16 + 5] = 2.0                   # between the samples
    with pytest.raises(AssertionError, match="stride gap"):
        G.assert_footprint(buf, view, "sample gap")
    buf[off + 3 * 16 + 5] = G.SENT
    view[1, 2, 7] = G.SENT
    G.assert_footprint(buf, view, "footprint alone does not ask for coverage")
    with pytest.raises(AssertionError, match="1 elements of the output were not written"):
        G.assert_footprint(buf, view, "unwritten", written=True)
    # a sub-range of a wider output: the rows in front of it must survive
    buf, full = G.guarded((2, 10, 8), torch.float16, device="cpu")
    sub = full[:, 4:]
    sub.fill_(1.0)
    G.assert_footprint(buf, sub, "sub-range", written=True)
    full[1, 3, 0] = 1.0
    with pytest.raises(AssertionError, match="stride gap"):
        G.assert_footprint(buf, sub, "text rows")
    # a buffer nothing may touch (an all-False mask)
    buf, view = G.guarded((4, 4), torch.float32, device="cpu")
    G.assert_footprint(buf, torch.zeros_like(buf, dtype=torch.bool), "untouched")
    view[0, 0] = 0.0
    with pytest.raises(AssertionError, match="must not touch"):
        G.assert_footprint(buf, torch.zeros_like(buf, dtype=torch.bool), "touched")


def test_guard_pad_is_derived_from_the_largest_tile():
    """2 x 256 rows of the output's row stride, never less than 4096 elements (tests/_guard.py docstring)."""
    for shape, strides, row in (((7, 8), None, 8), ((7, 8), (200, 1), 200), ((2, 5, 72), (5 * 80, 80, 1), 80), ((2, 4, 4, 64), (16 * 72, 4 * 72, 72, 1), 72),
                                ((33,), None, 1)):
        buf, view = G.guarded(shape, torch.float16, strides=strides, device="cpu")
        want = max(4096, 2 * 256 * row)
        span = 1 + sum((s - 1) * st for s, st in zip(view.shape, view.stride()))
        assert view.storage_offset() >= want and buf.numel() - view.storage_offset() - span >= want, (shape, strides)
        assert view.storage_offset() % 64 == 0


def test_poisoned_keeps_the_values_bit_exact_and_everything_else_nan():
    rng = np.random.RandomState(0)
    a = rng.standard_normal((3, 5, 8)).astype(np.float16)
    buf, view = G.poisoned(a, (3, 5, 8), (5 * 24 + 16, 24, 1), device="cpu")
    assert view.dtype == torch.float16 and np.array_equal(view.numpy().view(np.int16), a.view(np.int16))
    mask = G.payload_mask(buf, view)
    assert int(mask.sum()) == a.size and bool(torch.isnan(buf[~mask]).all()) and not bool(torch.isnan(buf[mask]).any())
    # memory a header requires to be finite: zero, NaN only beyond it
    v = rng.standard_normal((2, 4, 77)).astype(np.float32)
    buf, view = G.poisoned(v, (2, 4, 77), (4 * 88 + 64, 88, 1), dtype=torch.float16, zero_shape=(2, 4, 88), device="cpu")
    assert np.array_equal(view.numpy(), v.astype(np.float16))
    rows = buf.as_strided((2, 4, 88), (4 * 88 + 64, 88, 1), view.storage_offset())
    assert bool((rows[:, :, 77:] == 0).all())
    outer = G.payload_mask(buf, rows)
    assert bool(torch.isnan(buf[~outer]).all()) and int((~outer).sum()) >= 2 * 4096 + 64


# --------------------------------------------------------------------------- coverage of the GPU file's case table
class _NoTensors(dict):
    """make_desc asks for tensors by name; on the host one dummy serves for all (pointers are never dereferenced)."""
    _t = torch.zeros((1,), dtype=torch.float16)

    def __missing__(self, k):
        return self._t


PROPS = ("M tail", "N tail", "strided out_ld", "unsplit", "ticket reduce", "reduce kernel")


def resolve(ops, c):
    """(accepted, query or error text, workspace bytes) of case c under the library option the case sets."""
    from minddiffusion_amd import _lib
    keep = ops.get_option("gemm_lean_dense")
    try:
        if c["lean"] is not None:
            ops.set_option("gemm_lean_dense", c["lean"])
        d = make_desc(ops, c, _NoTensors())
        need = ops.gemm_workspace_bytes(d)
        if need:
            d.workspace, d.workspace_bytes = 4096, need          # exactly what the library asks for
        if c["colstats"]:
            d.colstats_out, d.colstats_cap = 4096, 1 << 20
        if not ops.gemm_check(d):
            return False, _lib.load().mdx_last_error().decode(), need
        return True, ops.gemm_query(d), need
    finally:
        ops.set_option("gemm_lean_dense", keep)


def observed_form(c, q):
    """The launch form from what mdx_gemm_query reports (not from the label the case carries), as far as the query can tell:
      * generic / lean / 128 x 160 / the 256-row conv core: out7[3], out7[1], out7[0];
      * HALO 8 x 16 patches against HALO8 (two 8 x 8 samples per tile): out7[5], the rows per colstats_out row block -- a HALO8 tile
        straddles two samples and reports 0, an 8 x 16 patch reports 128.  A split that goes through the reduce kernel reports 64 for
        both: there the library's own rule (8 x 8 images, option gemm_halo8) is all there is, and for the other rows it is asserted
        to agree with the query;
      * the query has NO field for the weight-streaming form or for the sub-pixel form: they follow from the descriptor (w_frag /
        w_sub) -- plan_gemm refuses w_frag on any launch that is not the HALO conv ("fragment-major weights (w_frag) are read by the
        HALO 3x3 conv only"), and a descriptor with w_sub that resolves to 256-row tiles runs the sub-pixel core (conv8p_wanted)."""
    if q[3] == 2:
        return "t160" if q[1] == 160 else "lean"
    if q[3] == 0:
        return "generic"
    if q[0] == 256:
        return "subpix" if c["w_sub"] else "conv8p"
    if c["w_frag"]:
        return "wfrag"
    by_rule = (c["H"], c["W"]) == (8, 8)
    if not (q[2] > 1 and q[6] == 0):
        assert (q[5] == 0) == by_rule, (c["id"], q)
    return "halo8" if by_rule else "halo"


def properties(c, q, need, form):
    Ho, Wo = out_hw(c)
    M = c["B"] * Ho * Wo
    props = set()
    if form in ("halo8", "wfrag"):
        if (c["H"], c["W"]) == (8, 8) and c["B"] % 2:
            props.add("M tail")                                   # two samples per 128-row tile: the last tile is half empty
    elif form in ("generic", "lean", "t160") and M % q[0]:
        props.add("M tail")
    if c["N"] % q[1]:
        props.add("N tail")
    if out_ld(c) > width(c):
        props.add("strided out_ld")
    tail_split = form in ("conv8p", "subpix") and need > 0        # conv8p reports one split: its tail tiles split on tickets
    if q[2] == 1 and not tail_split:
        props.add("unsplit")
    if (q[2] > 1 and q[6] == 1) or tail_split:
        props.add("ticket reduce")
    if q[2] > 1 and q[6] == 0:
        props.add("reduce kernel")
    return props


# Cells a form does not support: what is asked for, and what the library answers.  Only the two cells of the 128 x 160 tile are
# REFUSED (the message of mdx_gemm_check is given); the other seven are accepted and silently run another form ("elsewhere": the
# condition on mdx_gemm_query is given) -- there is no refusal message to list for them.
C8 = dict(ks=3, tile_m=256, stages=8)
UNSUPPORTED = {
    # a HALO patch grid tiles the image exactly (H % 8 == 0, W % 16 == 0): any other image runs on the generic kernel
    ("halo", "M tail"): (case("halo_12x16", "halo", 1, 12, 16, 64, 72, ks=3), "elsewhere", lambda q: q[3] == 0),
    # conv8p / its sub-pixel form tile the image into whole 16 x 16 patches; where they do not apply the forced tile_m = 256 (and a
    # forced split with it) is dropped and the launch runs on 128-row tiles: the 8 x 16-patch HALO kernel (24 x 16 is a whole number of
    # its patches) or, for an upsampling conv, the generic kernel
    ("conv8p", "M tail"): (case("conv8p_24x16", "conv8p", 1, 24, 16, 64, 72, **C8), "elsewhere", lambda q: q[0] == 128 and q[3] == 1),
    ("subpix", "M tail"): (case("subpix_24x16", "subpix", 1, 24, 16, 64, 64, **C8, up=1, w_sub=True), "elsewhere", lambda q: q[0] == 128 and q[3] == 0),
    # an explicit split takes the launch away from conv8p: the 16 x 16-patch HALO kernel runs it (and reports the split count)
    ("conv8p", "reduce kernel"): (case("conv8p_s5", "conv8p", 1, 16, 16, 320, 72, **C8, splitk=5), "elsewhere", lambda q: q[2] == 5 and q[6] == 0),
    ("subpix", "reduce kernel"): (case("subpix_s5", "subpix", 1, 16, 16, 320, 64, **C8, up=1, w_sub=True, splitk=5), "elsewhere", lambda q: q[0] == 128 and q[3] == 0),
    # a sub-pixel N tile stays inside one parity's weight rows: the tile the library picks always divides N (192 -> 192 / 96 / 64)
    ("subpix", "N tail"): (case("subpix_N192", "subpix", 1, 16, 16, 64, 192, **C8, up=1, w_sub=True), "elsewhere", lambda q: q[0] == 256 and 192 % q[1] == 0),
    # the 128 x 160 tile runs unsplit
    ("t160", "ticket reduce"): (case("t160_s2", "t160", 1, 129, 1, 320, 200, lean=1, tile_m=128, tile_n=160, splitk=2), "refused", "tile_n = 160 runs with tile_m = 128, unsplit"),
    ("t160", "reduce kernel"): (case("t160_s5", "t160", 1, 129, 1, 320, 200, lean=1, tile_m=128, tile_n=160, splitk=5), "refused", "tile_n = 160 runs with tile_m = 128, unsplit"),
    # the lean kernel reduces on tickets only: a deeper split runs on the generic kernel + reduce kernel
    ("lean", "reduce kernel"): (case("lean_s5", "lean", 1, 129, 1, 320, 72, lean=1, splitk=5), "elsewhere", lambda q: q[3] == 0 and q[6] == 0),
}


def test_case_table_covers_every_supported_cell():
    from minddiffusion_amd import ops
    from test_footprint_gpu import CASES          # the GPU file's table (importing it touches no device)
    from _footprint_cases import FORMS
    matrix = {(f, p): [] for f in FORMS for p in PROPS}
    refused = []
    for c in CASES:
        ok, q, need = resolve(ops, c)
        if not ok:
            refused.append((c["id"], q))
            continue
        exp = expected_query(c)
        assert all(q[k] == v for k, v in exp.items()), f"{c['id']}: resolves to {q}, the case expects {exp}"
        form = observed_form(c, q)
        assert form == c["form"], f"{c['id']}: runs the {form} form, the case names {c['form']}"
        if c["splitk"] > 1 or c["id"].startswith("conv8p_tail_split"):
            assert need > 0, c["id"]
        for p in properties(c, q, need, form):
            matrix[(form, p)].append(c["id"])
    assert not refused, f"rows the library refuses: {refused}"
    empty = [cell for cell, ids in matrix.items() if not ids and cell not in UNSUPPORTED]
    assert not empty, f"supported cells without a case: {empty}"
    filled_but_listed = [cell for cell in UNSUPPORTED if matrix[cell]]
    assert not filled_but_listed, f"cells listed as unsupported that the table fills: {filled_but_listed}"


@pytest.mark.parametrize("cell", sorted(UNSUPPORTED), ids=lambda c: f"{c[0]}-{c[1].replace(' ', '_')}")
def test_unsupported_cells_answer_as_listed(cell):
    from minddiffusion_amd import ops
    c, kind, what = UNSUPPORTED[cell]
    ok, q, _ = resolve(ops, c)
    if kind == "refused":
        assert not ok and re.search(re.escape(what), q), (ok, q)
    else:
        assert ok and what(q), (ok, q)


@pytest.mark.parametrize("H,W", [(24, 16), (16, 24), (8, 16), (20, 16), (16, 40), (12, 12), (40, 24)])
@pytest.mark.parametrize("up", [0, 1])
def test_forced_conv8p_on_an_image_that_is_not_whole_patches_runs_128_row_tiles(H, W, up):
    """The "M tail" cells of conv8p and its sub-pixel form for more than one geometry: whenever H or W is not a multiple of 16 the forced
    tile_m = 256 / stages = 8 is accepted and dropped, never run on a partial patch."""
    from minddiffusion_amd import ops
    ok, q, _ = resolve(ops, case(f"c8_{H}x{W}_{up}", "conv8p", 2, H, W, 64, 64, **C8, up=up, w_sub=bool(up)))
    assert ok and q[0] == 128 and q[2] == 1, (ok, q)
