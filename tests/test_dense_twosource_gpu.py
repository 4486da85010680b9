"""The K-segmented A operand of the lean dense kernel (csrc/dense.hip, template flag SEG): a 1x1 launch whose K runs over two row-major
sources, [a | a2] with row strides c1 and c2 (c1 % 64 == 0, c2 % 64 == 0: a K tile never straddles them).

Contract: bit-identical to the generic kernel on the same descriptor (option gemm_lean_dense 1 vs 0) -- same K order per output, same
MFMA operand order, same epilogue.  Shapes are the smallest at which the source switch can go wrong:
  * M 64 and 192 (192 is ragged against the 128-row tile: rows past M of BOTH sources must read as zero), N = 128;
  * (c1, c2) = (64, 64): the switch falls inside the tiles staged before the K loop; (256, 64): the second source starts at K tile 4,
    which every ring but the six-deep one issues from the steady loop;
    (128, 192): five K tiles, a 2-way in-kernel split takes 3 + 2 and its first half straddles the boundary at tile 2;
  * unsplit and the 2-way in-kernel (ticket) split; the 64 x 64, 64 x 128, 128 x 64, 128 x 128 tiles at the default ring depth, depth 2
    and the deepest depth each tile is built with;
  * bias + residual + row statistics, and bias + residual + column statistics (the library produces one kind of statistics per
    launch; column statistics exist where tokens per sample are whole M tiles -- ops.gemm_query says so -- so the 128-row tiles
    produce them at M = 128 instead of 64 | 192).
One case per tile is also checked against an fp32 torch matmul at the tolerance of the dense cases of tests/test_kernels_gpu.py
(rel-L2 1e-3: fp16 output rounding + accumulation order), and one case per tile and launch form runs inside sentinel guard bands
(tests/_guard.py): nothing outside out / the statistics buffers is written, and a, a2 and w keep their bits.
"""
import math

import numpy as np
import pytest
import torch

import _guard as G
from _util import check, h16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 128
TILES = [(64, 64), (64, 128), (128, 64), (128, 128)]
DEEPEST = {(64, 64): 6, (64, 128): 6, (128, 64): 4, (128, 128): 3}
SOURCES = [(64, 64), (256, 64), (128, 192)]


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def operands(ops):
    """One set of operands per (M, c1, c2), made once and left unchanged: poisoned a / a2 (NaN around them), packed w, bias, residual
    and the fp32 reference."""
    made = {}

    def get(M, c1, c2):
        key = (M, c1, c2)
        if key not in made:
            r = np.random.RandomState(1000 * M + 10 * c1 + c2)
            K = c1 + c2
            a = h16(r.standard_normal((M, c1)))
            a2 = h16(r.standard_normal((M, c2)))
            w = h16(r.standard_normal((N, K)) / math.sqrt(K))
            bias = r.standard_normal(N).astype(np.float32)
            res = h16(r.standard_normal((M, N)))
            t = dict(abuf_a=G.poisoned(a, dtype=torch.float16, device=DEV), abuf_a2=G.poisoned(a2, dtype=torch.float16, device=DEV),
                     w=ops.pack_gemm_weight(torch.from_numpy(w).to(DEV, torch.float16)),
                     bias=torch.from_numpy(bias).to(DEV), res=torch.from_numpy(res).to(DEV, torch.float16))
            t["a"], t["a2"] = t["abuf_a"][1], t["abuf_a2"][1]
            t["keep"] = {k: t[k].clone() for k in ("a", "a2", "w")}
            x = torch.from_numpy(np.concatenate([a, a2], 1))
            t["ref"] = x @ torch.from_numpy(w).T + torch.from_numpy(bias) + torch.from_numpy(res)
            made[key] = t
        return made[key]
    return get


def launch(ops, t, M, c1, c2, bm, bn, splitk, stages, stat, lean, guard=False):
    """One launch; returns (query, out, statistics or None, guards)."""
    ops.set_option("gemm_lean_dense", lean)
    guards = []
    if guard:
        obuf, out = G.guarded((M, N), device=DEV)
        guards.append((obuf, out, "out"))
    else:
        out = torch.zeros((M, N), dtype=torch.float16, device=DEV)
    kw = dict(a2=t["a2"], c2=c2, bias=t["bias"], residual=t["res"], residual_ld=N, tile_m=bm, tile_n=bn, splitk=splitk, stages=stages)
    d = ops.make_gemm_desc(t["a"], t["w"], N, 1, M, 1, c1, out, N, **kw)
    need = ops.gemm_workspace_bytes(d)
    ws = ops.new_gemm_workspace(max(need, 16), DEV)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    st = None
    if stat == "row":
        if guard:
            sbuf, st = G.guarded((M, N // 64, 2), torch.float32, device=DEV)
            guards.append((sbuf, st, "stats_out"))
        else:
            st = torch.zeros((M, N // 64, 2), dtype=torch.float32, device=DEV)
        d.stats_out = st.data_ptr()
    elif stat == "col":
        rows = ops.gemm_query(d)[5]
        if rows == 0:
            return None, None, None, []
        assert M % rows == 0
        if guard:
            sbuf, st = G.guarded((M // rows, N, 2), torch.float32, device=DEV)
            guards.append((sbuf, st, "colstats_out"))
        else:
            st = torch.zeros((M // rows, N, 2), dtype=torch.float32, device=DEV)
        d.colstats_out, d.colstats_cap = st.data_ptr(), M // rows
    q = ops.gemm_query(d)
    ops.gemm_run(d)
    torch.cuda.synchronize()
    d._keep = (ws, out, st)
    return q, out, st, guards


@pytest.mark.parametrize("c1,c2", SOURCES)
@pytest.mark.parametrize("bm,bn", TILES)
def test_two_source_lean_dense_is_bit_identical_to_the_generic_kernel(ops, operands, bm, bn, c1, c2):
    keep = ops.get_option("gemm_lean_dense")
    ran = 0
    try:
        for M in (64, 192) + ((128,) if bm == 128 else ()):
            t = operands(M, c1, c2)
            for splitk in (1, 2):
                for stages in (0, 2, DEEPEST[(bm, bn)]):
                    for stat in ("row", "col") if M != 128 else ("col",):
                        name = f"M{M}_c{c1}+{c2}_{bm}x{bn}_s{splitk}_st{stages}_{stat}"
                        q1, o1, s1, _ = launch(ops, t, M, c1, c2, bm, bn, splitk, stages, stat, 1)
                        if q1 is None:      # no column statistics from this tile at this M (see the module docstring)
                            assert stat == "col" and M % bm != 0, name
                            continue
                        q0, o0, s0, _ = launch(ops, t, M, c1, c2, bm, bn, splitk, stages, stat, 0)
                        assert q1[3] == 2 and q0[3] == 0, f"{name}: launch forms {q1} / {q0} (2 = lean dense kernel, 0 = generic)"
                        assert tuple(q1[:3]) == (bm, bn, splitk) and tuple(q0[:3]) == (bm, bn, splitk), f"{name}: resolved to {q1} / {q0}"
                        assert splitk == 1 or (q1[6] == 1 and q0[6] == 1), f"{name}: the split is not the in-kernel reduce"
                        assert torch.equal(o1, o0), f"{name}: out differs, max |d| = {float((o1.float() - o0.float()).abs().max())}"
                        assert torch.equal(s1, s0), f"{name}: statistics differ"
                        ran += 1
    finally:
        ops.set_option("gemm_lean_dense", keep)
    assert ran == (24 if bm == 64 else 18), ran      # every case but column statistics at M = 64 | 192 on the 128-row tiles


@pytest.mark.parametrize("bm,bn", TILES)
def test_two_source_lean_dense_against_fp32_matmul(ops, operands, bm, bn):
    keep = ops.get_option("gemm_lean_dense")
    try:
        M, c1, c2 = 192, 128, 192
        t = operands(M, c1, c2)
        q, out, st, _ = launch(ops, t, M, c1, c2, bm, bn, 2, 0, "row", 1)
        assert q[3] == 2, q
        check(f"dense_twosource_{bm}x{bn}_M{M}_c{c1}+{c2}", out, t["ref"], rel_l2=1e-3)
        o = out.double().reshape(M, N // 64, 64)
        check(f"dense_twosource_{bm}x{bn}_stats", st, torch.stack([o.sum(-1), (o * o).sum(-1)], -1), rel_l2=1e-5)
    finally:
        ops.set_option("gemm_lean_dense", keep)


@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("bm,bn", TILES)
def test_two_source_lean_dense_footprint(ops, operands, bm, bn, splitk):
    """Guard bands around out and the statistics buffers stay untouched, every output element is written, the inputs keep their bits."""
    keep = ops.get_option("gemm_lean_dense")
    try:
        c1, c2 = 256, 64
        for M, stat in ((192, "row"), (128 if bm == 128 else 192, "col")):
            t = operands(M, c1, c2)
            name = f"footprint_twosource_{bm}x{bn}_M{M}_s{splitk}_{stat}"
            q, out, st, guards = launch(ops, t, M, c1, c2, bm, bn, splitk, 0, stat, 1, guard=True)
            assert q is not None and q[3] == 2, (name, q)
            for gbuf, gview, label in guards:
                G.assert_footprint(gbuf, gview, f"{name}:{label}", written=True)
            for k in ("a", "a2", "w"):
                assert torch.equal(t[k], t["keep"][k]), f"{name}: input {k} was modified"
            check(name, out, t["ref"], rel_l2=1e-3)
    finally:
        ops.set_option("gemm_lean_dense", keep)


def test_two_source_lean_dense_keeps_fp16_subnormal_weights(ops):
    """The composite weight of ops.compose_ff_proj can lie mostly in the fp16 subnormal range (tests/test_ff_proj_compose_cpu.py
    emulates the launch with subnormals kept).  Here the matrix pipe gets such a weight: entries ~ N(0, 2e-5) -- about 99 % below
    2^-14 -- and no bias or residual that could hide a flush to zero: a kernel that flushed them would return (almost) zeros, rel-L2
    ~ 1.  Bound: rel-L2 1e-3 against the fp32 matmul of the same fp16 values, as the other dense cases (outputs ~ 4e-4 are fp16
    normals: their rounding is 2^-11 relative; the few below 6e-5 add at most 3e-8 absolute each)."""
    M, c1, c2 = 128, 256, 64
    r = np.random.RandomState(7)
    a = h16(r.standard_normal((M, c1)))
    a2 = h16(r.standard_normal((M, c2)))
    w = h16(2e-5 * r.standard_normal((N, c1 + c2)))
    assert float(((np.abs(w) < 2.0 ** -14) & (w != 0)).mean()) > 0.9
    ref = torch.from_numpy(np.concatenate([a, a2], 1)) @ torch.from_numpy(w).T
    wp = ops.pack_gemm_weight(torch.from_numpy(w).to(DEV, torch.float16))
    keep = ops.get_option("gemm_lean_dense")
    try:
        ops.set_option("gemm_lean_dense", 1)
        out = torch.zeros((M, N), dtype=torch.float16, device=DEV)
        d = ops.make_gemm_desc(torch.from_numpy(a).to(DEV, torch.float16), wp, N, 1, M, 1, c1, out, N,
                               a2=torch.from_numpy(a2).to(DEV, torch.float16), c2=c2, tile_m=64, tile_n=64, splitk=1)
        assert ops.gemm_query(d)[3] == 2
        ops.gemm_run(d)
        torch.cuda.synchronize()
        check("dense_twosource_subnormal_weights", out, ref, rel_l2=1e-3)
    finally:
        ops.set_option("gemm_lean_dense", keep)
