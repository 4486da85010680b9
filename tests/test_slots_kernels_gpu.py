"""The three launches of a sampling session on the GPU: mdx_sampler_step_slots_f32, mdx_randn_slots_f32, mdx_slot_gather_f32.

Every equality is torch.equal.  The step is held to mdx_sampler_step_table_f32 called on the rows sched[b][pos_b] gathered on the
host (the table entry is held to the scalar entries by test_step_table_gpu.py); the draws to ops.randn_seeded with the slot's own
draw counter; the gather to a torch indexing expression.  A slot that is not active keeps the sentinel every output starts with.
"""
import ctypes

import numpy as np
import pytest
import torch

import _step_table_util as U
from _guard import SENT

pytestmark = pytest.mark.gpu
DEV = U.DEV
# six slots at tick 5, cap 4:       pos 0   pos 2   pos -1   pos 4 = len   ACTIVE == 0   pos 3, zero coefficients
TICK, CAP = 5, 4
STARTS, LENS = [5, 3, 6, 1, 4, 2], [4, 4, 4, 4, 3, 4]
POS = [TICK - s for s in STARTS]
IN_RANGE = [0 <= p < n for p, n in zip(POS, LENS)]
ROW_ACTIVE = (1, 1, 1, 1, 0, 1)
ACTIVE = [r and bool(a) for r, a in zip(IN_RANGE, ROW_ACTIVE)]
PHIS = {0: (0.0,), 1: (0.3, 0.0, 1.0)}          # with any_rescale slot 1 is a phi == 0 row inside the rescale launch
SHAPES = {"6x4x8x8": (6, 4, 8, 8),              # 256 elements per sample: fewer than one 1024-thread workgroup
          "6x4x24x24": (6, 4, 24, 24)}          # 2304: several trips per thread


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def is_sentinel(t):
    return bool((t == SENT).all())


def test_the_case_covers_what_it_says():
    assert POS == [0, 2, -1, 4, 1, 3] and IN_RANGE == [True, True, False, False, True, True]
    assert ACTIVE == [True, True, False, False, False, True]


@pytest.mark.parametrize("alias_x", [False, True])
@pytest.mark.parametrize("any_rescale", [0, 1])
@pytest.mark.parametrize("pred", [0, 1])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_step_slots_equals_the_table_entry_on_the_gathered_rows(ops, shape, pred, any_rescale, alias_x):
    a = U.case(SHAPES[shape], pred, 3, 0.3, True, seed=41 + pred)
    B = SHAPES[shape][0]
    rows = U.rows_for(a, PHIS[any_rescale], active=ROW_ACTIVE)
    # slot 5: every history coefficient and sigma exactly 0 while old1..3 and the noise are live for the others -- and NaN there
    rows[5]["coef"] = (rows[5]["coef"][0], np.float32(0), np.float32(0), np.float32(0))
    s_at, s_1mat, s_ap, _, _ = rows[5]["update"]
    rows[5]["update"] = (s_at, s_1mat, s_ap, np.sqrt(1 - s_ap ** 2), np.float32(0))
    olds, noise = [U.dev32(o) for o in a["olds"]], U.dev32(a["noise"])
    for t in olds + [noise]:
        t[5] = float("nan")
    own = U.table_of(ops, rows)                                   # row b: what slot b's request holds at ITS position
    # every other position of a slot holds another request's (active) row: a wrong index or a row read for a slot that is out
    # of range changes an output
    decoy = U.table_of(ops, U.rows_for(a, (0.5,)))
    sched = torch.stack([decoy.roll(k + 1, 0) for k in range(CAP)], 1).contiguous()          # [B, CAP, ROW]
    for b in range(B):
        if IN_RANGE[b]:
            sched[b, POS[b]] = own[b]
    # the host-side reference: the table entry on the gathered rows, a slot out of range as an inactive row
    ref_rows = [dict(r, active=r["active"] if IN_RANGE[b] else 0.0) for b, r in enumerate(rows)]
    x_ref = U.dev32(a["x"])
    want = U.run_table(ops, a, ref_rows, any_rescale, x_t=x_ref, x_prev=x_ref if alias_x else None, olds=olds, noise=noise)

    xd = U.dev32(a["x"])
    got = (xd if alias_x else U.sentinel_like(xd), U.sentinel_like(xd), U.sentinel_like(xd), torch.full((B,), SENT, device=DEV))
    ops.sampler_step_slots(xd, U.dev32(a["xm"]), U.out_buf(a["vu"]), U.out_buf(a["vc"]), pred, olds, noise, got[2], got[0],
                           got[1], sched, i32(STARTS), i32(LENS), TICK, any_rescale, got[3])
    torch.cuda.synchronize()
    x_in = U.dev32(a["x"])
    for b in range(B):
        for g, w, name in zip(got, want, ("x_prev", "pred_x0", "e_t_out", "factor_out")):
            assert torch.equal(g[b], w[b]), (shape, pred, any_rescale, alias_x, b, name)
        if ACTIVE[b]:
            assert all(bool(torch.isfinite(g[b]).all()) for g in got), b
            assert not any(is_sentinel(g[b]) for g in got), b
        else:
            assert torch.equal(got[0][b], x_in[b]), b                                      # x_prev[b] == x[b]
            assert is_sentinel(got[1][b]) and is_sentinel(got[2][b]) and is_sentinel(got[3][b]), b
    if any_rescale:
        f = got[3].cpu().numpy()
        assert f[1] == 1.0 and f[0] != 1.0 and f[5] != 1.0        # the phi == 0 row, and rows that do rescale


@pytest.mark.parametrize("dropout", [0.0, 0.25])
@pytest.mark.parametrize("path", ["vector", "element"])
def test_randn_slots_draws_with_the_slots_own_counter(ops, path, dropout):
    starts, lens = i32([5, 3, 6, 1]), i32([2, 4, 4, 4])           # pos 0, 2, -1 (not started), 4 == len (ended)
    pos = [0, 2, None, None]
    seeds = ops.seeds_tensor([11, -3, 1 << 40, 7], DEV)
    sample = (4, 8, 8) if path == "vector" else (3, 5, 7)         # n = 256, or n = 105 into an output offset by one float
    n = int(np.prod(sample))
    base = torch.full((4 * n + 4,), SENT, device=DEV)
    off = 0 if path == "vector" else 1
    out = base[off:off + 4 * n].view(4, *sample)
    assert out.is_contiguous() and (out.data_ptr() % 16 == 0) == (path == "vector")
    stream, draw0, scale = ops.RNG_STEP, 3, 0.75
    assert ops.randn_slots(seeds, stream, draw0, starts, lens, TICK, out, scale=scale, dropout=dropout) is out
    torch.cuda.synchronize()
    for b, p in enumerate(pos):
        if p is None:
            assert is_sentinel(out[b]), b
            continue
        want = ops.randn_seeded(seeds[b:b + 1], stream, draw0 + p, sample, scale=scale, dropout=dropout)
        assert torch.equal(out[b:b + 1], want), (path, dropout, b)
        assert not torch.equal(out[b:b + 1], ops.randn_seeded(seeds[b:b + 1], stream, draw0 + p + 1, sample, scale=scale,
                                                             dropout=dropout))
        if dropout:
            assert 0 < int((out[b] == 0).sum()) < n
    assert is_sentinel(base[:off]) and is_sentinel(base[off + 4 * n:])


@pytest.mark.parametrize("n", [12, 7, 1028, 1027])
def test_slot_gather_is_the_indexing_expression(ops, n):
    """n with and without n % 4 == 0; 1028 / 1027 floats take more than one workgroup per slot."""
    B, reps = 6, 2
    rng = np.random.RandomState(n)
    src = torch.tensor(rng.randn(B, CAP, n).astype(np.float32), device=DEV)
    out = torch.full((reps * B, n), SENT, device=DEV)
    ops.slot_gather(src, i32(STARTS), i32(LENS), TICK, out, reps=reps)
    torch.cuda.synchronize()
    want = torch.full_like(out, SENT)
    on = [b for b in range(B) if IN_RANGE[b]]
    for r in range(reps):
        want[[r * B + b for b in on]] = src[on, [POS[b] for b in on]]
    assert torch.equal(out, want)
    assert is_sentinel(out[2]) and is_sentinel(out[B + 3]) and not is_sentinel(out[B + 4])
    # a slot_len beyond cap never reaches past the slot's own rows
    ops.slot_gather(src, i32([TICK - CAP] * B), i32([CAP + 3] * B), TICK, out, reps=reps)
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_refusals_return_invalid_and_leave_the_outputs_untouched(ops):
    from minddiffusion_amd import _lib
    lib = _lib.load()
    shape = (3, 4, 5, 7)
    a = U.case(shape, 1, 1, 0.3, True, seed=35)
    sched = U.table_of(ops, U.rows_for(a, (0.3,)))[:, None].repeat(1, CAP, 1).contiguous()
    x, ou, oc = U.dev32(a["x"]), U.out_buf(a["vu"]), U.out_buf(a["vc"])
    st, ln = i32([0, 0, 0]), i32([CAP] * 3)
    outs = [torch.full(shape, SENT, device=DEV) for _ in range(3)] + [torch.full((3,), SENT, device=DEV)]
    seeds = ops.seeds_tensor([1, 2, 3], DEV)
    rnd = torch.full(shape, SENT, device=DEV)
    src = torch.zeros((3, CAP, 8), device=DEV)
    dst = torch.full((6, 8), SENT, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def step(x=x, out_u=ou, out_c=oc, pred=1, sched=sched, start=st, length=ln, cap=CAP, tick=1, any_rescale=1, B=3):
        return lib.mdx_sampler_step_slots_f32(p(x), None, p(out_u), p(out_c), 8, pred, None, None, None, None, p(outs[2]),
                                              p(outs[0]), p(outs[1]), p(sched), p(start), p(length), cap, tick, any_rescale,
                                              p(outs[3]), B, 4, 5, 7, None)

    def randn(seeds=seeds, out=rnd, start=st, length=ln, tick=1, dropout=0.0, n=140):
        return lib.mdx_randn_slots_f32(p(seeds), 1, 0, 1.0, dropout, p(out), p(start), p(length), tick, 3, n, None)

    def gather(src=src, start=st, length=ln, cap=CAP, tick=1, dst=dst, n=8, reps=2):
        return lib.mdx_slot_gather_f32(p(src), p(start), p(length), cap, tick, p(dst), 3, n, reps, None)

    def refused(call, name, msg, **kw):
        assert call(**kw) == -1, (name, kw)                           # MDX_E_INVALID
        err = lib.mdx_last_error()
        assert name in err and msg in err, err

    for kw, msg in ((dict(sched=None), b"null slot pointer"), (dict(start=None), b"null slot pointer"),
                    (dict(length=None), b"null slot pointer"), (dict(cap=0), b"cap"), (dict(cap=-2), b"cap"),
                    (dict(tick=-1), b"tick"), (dict(out_u=None), b"needs the unconditional output"),
                    (dict(pred=2), b"pred_type"), (dict(x=None), b"null pointer"), (dict(out_c=None), b"null pointer"),
                    (dict(B=0), b"bad extents"), (dict(B=65536, any_rescale=0), b"bad extents")):
        refused(step, b"mdx_sampler_step_slots_f32", msg, **kw)
    for kw, msg in ((dict(seeds=None), b"null"), (dict(out=None), b"null"), (dict(start=None), b"null"),
                    (dict(length=None), b"null"), (dict(tick=-1), b"tick"), (dict(dropout=1.0), b"dropout_p"),
                    (dict(n=0), b"bad extents")):
        refused(randn, b"mdx_randn_slots_f32", msg, **kw)
    for kw, msg in ((dict(src=None), b"null"), (dict(dst=None), b"null"), (dict(start=None), b"null"),
                    (dict(length=None), b"null"), (dict(cap=0), b"cap"), (dict(tick=-1), b"tick"), (dict(reps=0), b"bad extents"),
                    (dict(n=0), b"bad extents")):
        refused(gather, b"mdx_slot_gather_f32", msg, **kw)
    with pytest.raises(_lib.MdxError, match="sched"):
        ops.sampler_step_slots(x, None, ou, oc, 1, [], None, outs[2], outs[0], outs[1], sched[:2], st, ln, 1, 1)
    with pytest.raises(_lib.MdxError, match="slot_len"):
        ops.sampler_step_slots(x, None, ou, oc, 1, [], None, outs[2], outs[0], outs[1], sched, st, ln.long(), 1, 1)
    with pytest.raises(_lib.MdxError, match="slot_gather: out has shape"):
        ops.slot_gather(src, st, ln, 1, dst[:3])
    torch.cuda.synchronize()
    assert all(is_sentinel(t) for t in outs + [rnd, dst])
    assert step() == 0 and randn() == 0 and gather() == 0            # and the same arguments, not refused, do launch
    torch.cuda.synchronize()
    assert not any(is_sentinel(t) for t in outs + [rnd, dst])
