"""mdx_slot_blend_f32 on the GPU: the per-slot mask blend of a sampling session against the two launches it replaces
(ops.randn_seeded(RNG_BLEND) then ops.q_sample(mask=)), bit for bit; against a float64 numpy restatement built from
tests/_seeded_util.py at mdx_q_sample_f32's tolerance (rel-L2 1e-5: fp32 elementwise arithmetic on given inputs); its footprint
(tests/_guard.py) and the isolation of a slot from its neighbours (tests/_isolation.py).

Three slots, cap 4: slot 0 blends from tick 0 (its slot_len of 6 is cut to cap: active on ticks 0 .. 3), slot 1 is active on ticks
0 .. 2 with blend off, slot 2 blends on ticks 2 and 3 only (slot_start 2).  Ticks 0 .. 5 see every slot before, inside and past
its window.  Three launch forms: HW = 64 (one float4 per lane), HW = 35 (one float), HW = 64 on buffers that start one float past
a 16-byte boundary (one float, by alignment).
"""
import numpy as np
import pytest
import torch

import _guard as G
import _isolation as I
import _seeded_util as SU
from _util import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, C, CAP = 3, 4, 4
START, LEN, ON = [0, 0, 2], [6, 3, 2], [1, 0, 1]
SEEDS = [-7, 11, (1 << 63) + 5]                      # a negative seed and one >= 2^63 on the two slots that blend
TICKS = range(6)
DRAW0S = [0, (1 << 32) - 2]                          # the second wraps: draw0 + 2 = 0 (mod 2^32)
FORMS = {"vec4": ((8, 8), False), "scalar_hw35": ((5, 7), False), "scalar_misaligned": ((8, 8), True)}


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def pos_of(b, tick):
    p = tick - START[b]
    return p if 0 <= p < min(LEN[b], CAP) else None


def blends(b, tick):
    return ON[b] != 0 and pos_of(b, tick) is not None


def host_case(hw, seed=0):
    """x0, keep, img [B, C, h, w] and blend_ab [B, CAP, 2], every slot its own values; keep holds exact 0, exact 1 and fractions."""
    rng = np.random.RandomState(100 + seed)
    shape = (B, C) + hw
    x0, img = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    keep = rng.rand(*shape).astype(np.float32)
    pick = rng.randint(0, 3, size=shape)
    keep[pick == 0], keep[pick == 1] = 0.0, 1.0
    assert (keep == 0).any() and (keep == 1).any() and ((keep > 0) & (keep < 1)).any()
    th = rng.uniform(0.1, 1.4, size=(B, CAP))
    ab = np.stack([np.cos(th), np.sin(th)], axis=2).astype(np.float32)
    return x0, keep, img, ab


def placed(a, misaligned, fill=None):
    """(buf, view): a contiguous device view holding `a` inside a sentinel-filled allocation (tests/_guard.py); misaligned: the
    view starts one float past a 16-byte boundary.  fill: a value for the whole view instead of `a`."""
    n = int(np.prod(a.shape))
    buf, v = G.guarded((n + 1,), torch.float32, device=DEV)
    off = v.storage_offset() + (1 if misaligned else 0)
    view = buf.as_strided(tuple(a.shape), G._contiguous(a.shape), off)
    assert view.data_ptr() % 16 == (4 if misaligned else 0) and view.is_contiguous()
    if fill is None:
        view.copy_(torch.from_numpy(a))
    else:
        view.fill_(fill)
    return buf, view


def tables(ops, ab, on=ON, start=START, length=LEN, seeds=SEEDS):
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    return dict(seeds=ops.seeds_tensor(seeds, DEV), blend_ab=torch.tensor(ab, device=DEV), blend_on=i32(on),
                slot_start=i32(start), slot_len=i32(length))


def launch(ops, x0, keep, img, t, draw0, tick):
    ops.slot_blend(x0, keep, img, t["seeds"], ops.RNG_BLEND, draw0, t["blend_ab"], t["blend_on"], t["slot_start"], t["slot_len"],
                   tick)
    torch.cuda.synchronize()
    return img


_REF = {}


def two_launches(ops, hw, draw0, tick):
    """{b: (blended row, q row)} of the slots that blend at `tick`, from the launches the entry replaces, on aligned tensors of
    ONE sample: randn_seeded at draw0 + pos_b (mod 2^32), then q_sample with the mask, in place on the row (and without it: q).
    Computed once per (shape, draw0, tick)."""
    key = (hw, draw0, tick)
    if key not in _REF:
        x0, keep, img, ab = host_case(hw)
        d = lambda a: torch.tensor(a, device=DEV)
        out = {}
        for b in range(B):
            if not blends(b, tick):
                continue
            p = pos_of(b, tick)
            noise = ops.randn_seeded(ops.seeds_tensor(SEEDS[b:b + 1], DEV), ops.RNG_BLEND, (draw0 + p) % (1 << 32), (C,) + hw)
            row = d(img[b:b + 1])
            ops.q_sample(d(x0[b:b + 1]), noise, ab[b, p, 0], ab[b, p, 1], out=row, mask=d(keep[b:b + 1]), img=row)
            out[b] = (row[0], ops.q_sample(d(x0[b:b + 1]), noise, ab[b, p, 0], ab[b, p, 1])[0])
        torch.cuda.synchronize()
        _REF[key] = out
    return _REF[key]


@pytest.mark.parametrize("draw0", DRAW0S)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_slot_blend_is_the_two_launches_it_replaces(ops, form, draw0):
    """The main check: every row that blends is torch.equal to randn_seeded + q_sample(mask=) on that row -- so the float4 and the
    scalar forms agree element for element --, keep == 0 leaves the old bits, keep == 1 gives q; every other row keeps its bits."""
    hw, mis = FORMS[form]
    x0, keep, img, ab = host_case(hw)
    t = tables(ops, ab)
    x0_d, keep_d = placed(x0, mis)[1], placed(keep, mis)[1]
    old = torch.tensor(img, device=DEV)
    keep_a = torch.tensor(keep, device=DEV)
    assert any(blends(0, k) for k in TICKS) and not any(blends(1, k) for k in TICKS)
    assert [k for k in TICKS if blends(2, k)] == [2, 3] and [k for k in TICKS if blends(0, k)] == [0, 1, 2, 3]
    for tick in TICKS:
        got = launch(ops, x0_d, keep_d, placed(img, mis)[1], t, draw0, tick)
        want = two_launches(ops, hw, draw0, tick)
        for b in range(B):
            if b not in want:
                assert torch.equal(got[b].view(torch.int32), old[b].view(torch.int32)), (form, tick, b)
                continue
            row, q = want[b]
            print(f"{form} draw0 {draw0} tick {tick} slot {b}: max|d| {float((got[b] - row).abs().max()):.3e}")
            assert torch.equal(got[b], row), (form, tick, b)
            assert not torch.equal(got[b], old[b])
            zero, one = keep_a[b] == 0, keep_a[b] == 1
            assert torch.equal(got[b][zero].view(torch.int32), old[b][zero].view(torch.int32))
            assert torch.equal(got[b][one].view(torch.int32), q[one].view(torch.int32))
    # the same draw on two ticks apart is another draw: slot 0 at ticks 0 and 1 differ
    assert not torch.equal(two_launches(ops, hw, draw0, 0)[0][0], two_launches(ops, hw, draw0, 1)[0][0])


@pytest.mark.parametrize("form", sorted(FORMS))
def test_slot_blend_vs_float64(ops, form):
    hw, mis = FORMS[form]
    x0, keep, img, ab = host_case(hw)
    t = tables(ops, ab)
    f, n = np.float64, C * hw[0] * hw[1]
    for draw0 in DRAW0S:
        for tick in (1, 2):
            got = launch(ops, placed(x0, mis)[1], placed(keep, mis)[1], placed(img, mis)[1], t, draw0, tick)
            rows = [b for b in range(B) if blends(b, tick)]
            ref = []
            for b in rows:
                p = pos_of(b, tick)
                nz = SU.normals64(SEEDS[b], SU.RNG_BLEND, (draw0 + p) % (1 << 32), n).reshape((C,) + hw)
                q = f(ab[b, p, 0]) * x0[b].astype(f) + f(ab[b, p, 1]) * nz
                ref.append(keep[b].astype(f) * q + (1.0 - keep[b].astype(f)) * img[b].astype(f))
            assert rows == ([0] if tick == 1 else [0, 2])
            check(f"slot_blend_{form}_draw{draw0}_tick{tick}", got[rows], np.stack(ref), rel_l2=1e-5)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_slot_blend_writes_only_the_rows_that_blend(ops, form):
    """img starts as the sentinel everywhere: after the launch only the spans of the active slots that blend may differ from it --
    the spans of the slot with blend off and of the slots outside their window, and both pads, still hold it.  The inputs, in
    guarded allocations of their own, keep every bit."""
    hw, mis = FORMS[form]
    x0, keep, img, ab = host_case(hw)
    t = tables(ops, ab)
    for tick in TICKS:
        xb, xv = placed(x0, mis)
        kb, kv = placed(keep, mis)
        ib, iv = placed(img, mis, fill=G.SENT)
        before = {k: v.clone() for k, v in dict(t, x0=xb, keep=kb).items()}
        launch(ops, xv, kv, iv, t, 0, tick)
        rows = [b for b in range(B) if blends(b, tick)]
        if rows:
            G.assert_footprint(ib, [iv[b] for b in rows], f"slot_blend {form} tick {tick}")
            assert all(bool((iv[b] != G.SENT).any()) for b in rows)
        else:
            G.assert_footprint(ib, torch.zeros(ib.numel(), dtype=torch.bool, device=DEV), f"slot_blend {form} tick {tick}")
        for k, v in dict(t, x0=xb, keep=kb).items():
            same = v.view(torch.int32) if v.dtype == torch.float32 else v
            assert torch.equal(same, before[k].view(same.dtype)), (form, tick, k)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_slot_blend_isolates_a_slot_from_its_neighbours(ops, form):
    """Slot 0's bits at tick 2 do not change when the neighbours' x0, keep, img, seeds, blend_ab rows, blend_on, slot_start and
    slot_len change (re-drawn, NaN, Inf; the integer tables take other values)."""
    hw, mis = FORMS[form]
    x0, keep, img, ab = host_case(hw)
    t = tables(ops, ab)
    d = lambda a: torch.tensor(a, device=DEV)
    inputs = dict(t, x0=d(x0), keep=d(keep), img=d(img))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    per_sample = {"x0": {"axis": 0}, "keep": {"axis": 0}, "img": {"axis": 0}, "blend_ab": {"axis": 0},
                  "seeds": {"axis": 0, "other": torch.tensor([SEEDS[0], 99, -3], dtype=torch.int64)},
                  "blend_on": {"axis": 0, "other": i32([1, 1, 0])}, "slot_start": {"axis": 0, "other": i32([0, 2, 1])},
                  "slot_len": {"axis": 0, "other": i32([6, 1, 4])}}

    def run(inp):
        dev = {k: placed(inp[k].cpu().numpy(), mis)[1] for k in ("x0", "keep", "img")}
        return launch(ops, dev["x0"], dev["keep"], dev["img"], inp, 0, 2)

    I.assert_isolated(f"slot_blend_{form}", run, inputs, per_sample, 0, lambda out, b: [out[b]], seed=5)


def test_slot_blend_wrapper_refuses_bad_tensors(ops):
    from minddiffusion_amd._lib import MdxError
    x0, keep, img, ab = host_case((8, 8))
    t = tables(ops, ab)
    d = lambda a: torch.tensor(a, device=DEV)
    args = lambda **kw: [dict(dict(t, x0=d(x0), keep=d(keep), img=d(img), stream=ops.RNG_BLEND, draw0=0, tick=0), **kw)[k]
                         for k in ("x0", "keep", "img", "seeds", "stream", "draw0", "blend_ab", "blend_on", "slot_start",
                                   "slot_len", "tick")]
    for kw, word in ((dict(x0=d(x0)[:2]), "x0"), (dict(keep=d(keep)[:, :1]), "keep"), (dict(blend_ab=d(ab)[:, :, 0]), "blend_ab"),
                     (dict(blend_on=t["blend_on"][:2]), "blend_on"), (dict(slot_len=t["slot_len"].to(torch.int64)), "slot_len"),
                     (dict(img=d(img).cpu()), "GPU"), (dict(draw0=1 << 32), "draw0"), (dict(stream=1 << 31), "stream")):
        with pytest.raises(MdxError, match=word):
            ops.slot_blend(*args(**kw))
    with pytest.raises(MdxError, match="tick"):
        ops.slot_blend(*args(tick=-1))
