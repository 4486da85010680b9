"""mdx_sampler_step_table_f32 on the GPU: the fused sampler step with every per-sample scalar read from a device table.

The contract is bit-identity: an active row b computes exactly (torch.equal) what the scalar entry ops.sampler_update would
pick for that row's scalars computes on sample b alone -- so this file carries no tolerance; the scalar entries are held to
numpy by test_kernels_gpu.py / test_vpred_gpu.py / test_guidance_rescale_gpu.py.  Also here: a zero coefficient skips a live
pointer, inactive rows are carried over and nothing else of them is written, the launch writes only its outputs, the
aliasing the scalar entries allow, and the refusals.
"""
import ctypes

import numpy as np
import pytest
import torch

import _step_table_util as U
from _guard import SENT, assert_footprint, guarded

pytestmark = pytest.mark.gpu
DEV = U.DEV
SHAPES = {
    "3x4x5x7": (3, 4, 5, 7),        # 140 elements per sample: fewer than a workgroup, not a multiple of a wave
    "2x4x33x37": (2, 4, 33, 37),    # 4 884 per sample: several ragged trips, more than 4 x 1024
    "5x4x8x8": (5, 4, 8, 8),        # mixtures of active and inactive rows
}
PHIS = {0: (0.0,), 1: (0.3, 0.0, 1.0)}      # any_rescale -> the rows' guidance rescales (mixed: rows with 0 among them)


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def is_sentinel(t):
    return bool((t == SENT).all())


@pytest.mark.parametrize("any_rescale", [0, 1])
@pytest.mark.parametrize("separate_xm", [False, True])
@pytest.mark.parametrize("sigma", [0.0, 0.3])
@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("pred", [0, 1])
@pytest.mark.parametrize("shape", ["3x4x5x7", "2x4x33x37"])
def test_row_equals_the_scalar_entry_bit_for_bit(ops, shape, pred, order, sigma, separate_xm, any_rescale):
    a = U.case(SHAPES[shape], pred, order, sigma, separate_xm, seed=order + 4 * pred + 8 * int(separate_xm))
    rows = U.rows_for(a, PHIS[any_rescale])
    got = U.run_table(ops, a, rows, any_rescale)
    entries = set()
    for b in range(len(rows)):
        entries.add(U.scalar_entry(pred, float(rows[b]["phi"]), True))
        U.assert_row_equals_scalar(got, U.run_scalar(ops, a, rows, b), b, (shape, pred, order, sigma, separate_xm, any_rescale))
    if any_rescale:
        assert "rescale" in entries and len(entries) == 2          # the mixture is one: rescaled rows and plain ones
        f = got[3].cpu().numpy()
        assert np.all(f[[float(r["phi"]) == 0 for r in rows]] == 1.0) and np.all(f[[float(r["phi"]) != 0 for r in rows]] != 1.0)
    else:
        assert torch.equal(got[3], torch.ones_like(got[3]))


@pytest.mark.parametrize("pred", [0, 1])
def test_without_an_unconditional_output_rows_equal_the_unguided_scalar_entry(ops, pred):
    """out_u NULL: no combine, no rescale whatever the rows' phi says (ops.sampler_update's rule)."""
    a = U.case(SHAPES["3x4x5x7"], pred, 1, 0.3, True, seed=31)
    rows = U.rows_for(a, (0.3, 0.0, 1.0))
    got = U.run_table(ops, a, rows, 0, no_u=True)
    for b in range(len(rows)):
        U.assert_row_equals_scalar(got, U.run_scalar(ops, a, rows, b, no_u=True), b, ("no_u", pred))


@pytest.mark.parametrize("any_rescale", [0, 1])
@pytest.mark.parametrize("pred", [0, 1])
def test_a_zero_coefficient_skips_a_live_pointer(ops, pred, any_rescale):
    """Row 1 has c1 == 0 and row 2 sigma == 0 while the other rows use old1 and the noise; what the pointers hold in those
    rows is NaN.  The rows come out finite and equal the scalar entry called with that pointer NULL."""
    a = U.case(SHAPES["5x4x8x8"], pred, 1, 0.3, True, seed=32)
    rows = U.rows_for(a, PHIS[any_rescale])
    rows[1]["coef"] = (rows[1]["coef"][0], np.float32(0), np.float32(0), np.float32(0))
    s_at, s_1mat, s_ap, _, _ = rows[2]["update"]
    rows[2]["update"] = (s_at, s_1mat, s_ap, np.sqrt(1 - s_ap ** 2), np.float32(0))
    old1, noise = U.dev32(a["olds"][0]), U.dev32(a["noise"])
    old1[1], noise[2] = float("nan"), float("nan")
    got = U.run_table(ops, a, rows, any_rescale, olds=[old1], noise=noise)
    for b in range(len(rows)):
        drop = {1: ("old1",), 2: ("noise",)}.get(b, ())
        U.assert_row_equals_scalar(got, U.run_scalar(ops, a, rows, b, drop=drop), b, ("zero_coef", pred, any_rescale))


@pytest.mark.parametrize("alias_x", [False, True])
@pytest.mark.parametrize("any_rescale", [0, 1])
@pytest.mark.parametrize("pred", [0, 1])
def test_inactive_rows_are_carried_over_and_nothing_else_of_them_is_written(ops, pred, any_rescale, alias_x):
    a = U.case(SHAPES["5x4x8x8"], pred, 3, 0.3, True, seed=33)
    active = (1, 0, 1, 1, 0)
    rows = U.rows_for(a, PHIS[any_rescale], active=active)
    for b, on in enumerate(active):      # an inactive row's scalars are never read: poison them
        if not on:
            rows[b]["scale"] = rows[b]["phi"] = np.float32("nan")
            rows[b]["update"] = (np.float32(0),) * 5
    x_t = U.dev32(a["x"])
    got = U.run_table(ops, a, rows, any_rescale, x_t=x_t, x_prev=x_t if alias_x else None)
    x_in = U.dev32(a["x"])
    for b, on in enumerate(active):
        if on:
            U.assert_row_equals_scalar(got, U.run_scalar(ops, a, rows, b), b, ("inactive", pred, any_rescale, alias_x))
        else:
            assert torch.equal(got[0][b], x_in[b])
            assert is_sentinel(got[1][b]) and is_sentinel(got[2][b]) and is_sentinel(got[3][b])


@pytest.mark.parametrize("any_rescale", [0, 1])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_launch_writes_only_its_outputs(ops, shape, any_rescale):
    a = U.case(SHAPES[shape], 1, 3, 0.3, True, seed=34)
    rows = U.rows_for(a, PHIS[any_rescale], active=(1, 1, 0))
    B = len(rows)
    bufs, views = zip(*[guarded(SHAPES[shape], torch.float32, device=DEV) for _ in range(3)] +
                      [guarded((B,), torch.float32, device=DEV)])
    U.run_table(ops, a, rows, any_rescale, outs=views)
    for buf, view, name in zip(bufs, views, ("x_prev", "pred_x0", "e_t_out", "factor_out")):
        assert_footprint(buf, view, f"step_table_{shape}_{name}")
    on = torch.tensor([r["active"] != 0 for r in rows], device=DEV)
    assert not (views[0] == SENT).any()                               # x_prev: every row, the carried-over ones too
    for v in views[1:]:
        assert not (v[on] == SENT).any() and is_sentinel(v[~on])


def test_sampler_step_table_aliasing(ops):
    """x_prev == x_model (the second call of the PLMS first step) and x_prev == x give exactly the non-aliased results."""
    eq = lambda got, ref: all(torch.equal(g, r) for g, r in zip(got, ref))
    for shape in ("3x4x5x7", "2x4x33x37"):
        for any_rescale in (0, 1):
            a = U.case(SHAPES[shape], 1, 1, 0.3, True, seed=25)
            rows = U.rows_for(a, PHIS[any_rescale])
            ref = U.run_table(ops, a, rows, any_rescale)
            xm_t = U.dev32(a["xm"])
            got = U.run_table(ops, a, rows, any_rescale, xm_t=xm_t, x_prev=xm_t)
            assert got[0] is xm_t and eq(got, ref)
            x_t = U.dev32(a["x"])
            got = U.run_table(ops, a, rows, any_rescale, x_t=x_t, x_prev=x_t)
            assert got[0] is x_t and eq(got, ref)
            # x_model == NULL with x_prev == x: both aliases at once
            b = U.case(SHAPES[shape], 1, 1, 0.3, False, seed=25)
            ref = U.run_table(ops, b, rows, any_rescale)
            x_t = U.dev32(b["x"])
            assert eq(U.run_table(ops, b, rows, any_rescale, x_t=x_t, x_prev=x_t), ref)


def test_refusals_leave_the_outputs_untouched(ops):
    """Everything mdx_sampler_step_pred_f32 refuses, a NULL table, any_rescale without out_u or with C * H * W < 2: -1, a
    message that names the entry, and no launch."""
    from minddiffusion_amd import _lib
    lib = _lib.load()
    shape = SHAPES["3x4x5x7"]
    a = U.case(shape, 1, 1, 0.3, True, seed=35)
    table = U.table_of(ops, U.rows_for(a, (0.3,)))
    x, ou, oc = U.dev32(a["x"]), U.out_buf(a["vu"]), U.out_buf(a["vc"])
    outs = [torch.full(shape, SENT, device=DEV) for _ in range(3)] + [torch.full((shape[0],), SENT, device=DEV)]
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(x=x, out_u=ou, out_c=oc, out_ld=8, pred=1, x_prev=outs[0], table=table, any_rescale=1, B=3, C=4, H=5, W=7):
        return lib.mdx_sampler_step_table_f32(p(x), None, p(out_u), p(out_c), out_ld, pred, None, None, None, None, p(outs[2]),
                                              p(x_prev), p(outs[1]), p(table), any_rescale, p(outs[3]), B, C, H, W, None)

    def refused(msg, **kw):
        assert call(**kw) == -1
        err = lib.mdx_last_error()
        assert b"mdx_sampler_step_table_f32" in err and msg in err, err

    refused(b"null table", table=None)
    refused(b"null table", table=None, any_rescale=0)
    refused(b"needs the unconditional output", out_u=None)
    refused(b"C * H * W >= 2", C=1, H=1, W=1)
    refused(b"pred_type", pred=2)
    refused(b"null pointer", x=None)
    refused(b"null pointer", out_c=None)
    refused(b"null pointer", x_prev=None)
    refused(b"bad extents", out_ld=3)
    refused(b"bad extents", B=0)
    refused(b"bad extents", any_rescale=0, B=65536)
    with pytest.raises(_lib.MdxError, match="table"):
        ops.sampler_step_table(x, None, ou, oc, 1, [], None, outs[2], outs[0], outs[1], table[:2], 1)
    torch.cuda.synchronize()
    assert all(is_sentinel(t) for t in outs)
    assert call(any_rescale=0, out_u=None) == 0 and call() == 0        # and the same arguments, not refused, do launch
    torch.cuda.synchronize()
    assert not any(is_sentinel(t) for t in outs)
