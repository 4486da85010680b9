"""The 128 x 160 tile of the lean dense kernel (csrc/dense.hip: four waves 4 x 1, epilogue_w41; GEGLU packed 80 'a' | 80 gate).

Reference and tolerance are those of test_kernels_gpu.py::test_gemm_geglu: fp16-rounded operands, fp32 torch matmul, the oracle's
gelu_tanh, rel-L2 <= 2e-3.  The tile keeps the K order, the MFMA operand order and the epilogue arithmetic of the other tiles, so
on top of the parity check a launch on it must give the BITS of the same launch on the 64 x 128 tile.
"""
import math

import numpy as np
import pytest
import torch

from _util import check, h16
from oracle import ldm as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.float16)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.float32)


def _problem(ops, M, N, K, geglu, bias, res, ln, seed):
    """Operands of out = [GEGLU](LN?(a) W^T + b) (+ res) and the fp32 reference.  Returns (a, unit -> kwargs with packed weights, ref)."""
    r = np.random.RandomState(seed)
    a = h16(r.standard_normal((M, K)) + (0.5 if ln else 0.0))
    w = h16(r.standard_normal((N, K)) / math.sqrt(K))
    bv = r.standard_normal(N).astype(np.float32) if bias else None
    No = N // 2 if geglu else N
    rs = h16(r.standard_normal((M, No))) if res else None
    af = torch.tensor(a).float()
    wt, bt, st_ = dev16(w), (dev32(bv) if bias else None), None
    common = {}
    if ln:
        g = (1 + 0.3 * r.standard_normal(K)).astype(np.float32)
        be = (0.3 * r.standard_normal(K)).astype(np.float32)
        xs = a.astype(np.float32).reshape(M, K // 64, 64)
        stats = np.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).astype(np.float32)
        wt, st_, bt = ops.fold_layernorm(dev16(w), dev32(g), dev32(be), dev32(bv) if bias else None)
        common.update(ln_stats=dev32(stats))
        mu, var = af.mean(1, keepdim=True), af.var(1, keepdim=True, unbiased=False)
        af = (af - mu) / torch.sqrt(var + 1e-5) * torch.tensor(g) + torch.tensor(be)
    y = af @ torch.tensor(w).float().T
    if bias:
        y = y + torch.tensor(bv)
    if geglu:
        xa, gate = y.chunk(2, dim=-1)
        y = xa * O.gelu_tanh(gate)
    if res:
        y = y + torch.tensor(rs).float()
        common.update(residual=dev16(rs), residual_ld=No)

    def packed(unit):
        kw = dict(common)
        if geglu:
            il = lambda t: ops.geglu_interleave(t[:N // 2], t[N // 2:], unit)
            kw.update(w=ops.pack_gemm_weight(il(wt)), epilogue=ops.EPI_GEGLU, geglu_unit=0 if unit == 64 else unit)
            if bt is not None:
                kw["bias"] = il(bt)
            if st_ is not None:
                kw["ln_s"] = il(st_)
        else:
            kw.update(w=ops.pack_gemm_weight(wt))
            if bt is not None:
                kw["bias"] = bt
            if st_ is not None:
                kw["ln_s"] = st_
        return kw
    return dev16(a), packed, y, No


def _run(ops, da, kw, M, N, K, No, fill=0.0, **tile):
    kw = dict(kw)
    w = kw.pop("w")
    out = torch.full((M, No), fill, dtype=torch.float16, device=DEV)
    d = ops.make_gemm_desc(da, w, N, 1, M, 1, K, out, No, splitk=1, **tile, **kw)
    q = ops.gemm_query(d)
    ops.gemm_run(d)
    torch.cuda.synchronize()
    return out, q


_CASES = [
    # name, M, N, K, geglu, bias, residual, LayerNorm fold
    ("geglu16_target", 512, 10240, 1280, True, True, False, True),       # the two target launches of the batch-2 plan (norm3 folded)
    ("geglu32_target", 2048, 5120, 640, True, True, False, True),
    ("geglu16_nofold", 512, 10240, 1280, True, True, False, False),
    ("geglu32_nobias", 2048, 5120, 640, True, False, False, False),
    ("geglu_res", 256, 1280, 320, True, True, True, False),
    ("geglu_m_edge", 200, 2560, 320, True, True, False, True),           # M % 128 != 0: rows past M in the last tile
    ("plain_target_like", 2048, 1920, 640, False, True, True, False),    # 16 x 12 blocks
    ("plain_n_edge", 512, 1200, 640, False, True, True, False),          # N % 160 != 0 (and % 64 != 0): an 80-column edge tile
    ("plain_n_edge_ln", 256, 448, 320, False, True, False, True),        # 2.8 tiles: the last one reads past the packed weight
    ("plain_m_edge", 300, 640, 1280, False, True, True, True),
    ("plain_bare", 384, 960, 640, False, False, False, False),
]


@pytest.mark.parametrize("case", _CASES, ids=lambda c: c[0])
def test_tile160_matches_the_reference(ops, case):
    name, M, N, K, geglu, bias, res, ln = case
    da, packed, ref, No = _problem(ops, M, N, K, geglu, bias, res, ln, sum(map(ord, name)))
    out, q = _run(ops, da, packed(80), M, N, K, No, tile_m=128, tile_n=160)
    assert q[0] == 128 and q[1] == 160 and q[2] == 1 and q[3] == 2, f"{name}: resolved to {q} (want the lean kernel on 128 x 160)"
    assert out.shape == (M, No)
    check(f"tile160_{name}", out, ref, rel_l2=2e-3)


@pytest.mark.parametrize("stages", [2, 3])
@pytest.mark.parametrize("case", [c for c in _CASES if c[0] in ("geglu16_target", "geglu32_target", "plain_target_like",
                                                                 "plain_m_edge", "geglu_res")], ids=lambda c: c[0])
def test_tile160_is_bit_identical_to_the_64x128_tile(ops, case, stages):
    name, M, N, K, geglu, bias, res, ln = case
    da, packed, ref, No = _problem(ops, M, N, K, geglu, bias, res, ln, sum(map(ord, name)))
    new, q1 = _run(ops, da, packed(80), M, N, K, No, tile_m=128, tile_n=160, stages=stages)
    old, q0 = _run(ops, da, packed(64), M, N, K, No, tile_m=64, tile_n=128)
    assert (q1[0], q1[1], q1[3]) == (128, 160, 2) and (q0[0], q0[1]) == (64, 128), (q1, q0)
    assert torch.equal(new, old), f"{name}: max |d| = {float((new.float() - old.float()).abs().max())}"


@pytest.mark.parametrize("unit,tile", [(64, dict(tile_m=128, tile_n=160)), (80, dict(tile_m=64, tile_n=128)), (80, dict(tile_m=128, tile_n=128)),
                                       (80, dict())])
def test_geglu_packing_unit_must_match_the_tile(ops, unit, tile):
    """Weights packed for one tile on the other would pair wrong columns without an error: refused, and nothing is written.  (80, {}):
    a unit-80 descriptor of a shape the tile table has no 160-column row for resolves to a 128-column tile -- refused as well."""
    from minddiffusion_amd._lib import MdxError
    M, N, K = 256, 1280, 320
    da, packed, ref, No = _problem(ops, M, N, K, True, True, False, False, 7)
    kw = packed(unit)
    w = kw.pop("w")
    out = torch.full((M, No), 7.0, dtype=torch.float16, device=DEV)
    d = ops.make_gemm_desc(da, w, N, 1, M, 1, K, out, No, splitk=1, **tile, **kw)
    assert not ops.gemm_check(d)
    with pytest.raises(MdxError):
        ops.gemm_query(d)
    with pytest.raises(MdxError):
        ops.gemm_run(d)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused launch wrote to its output"


def test_tile160_declines_what_its_epilogue_does_not_carry(ops):
    from minddiffusion_amd._lib import MdxError
    M, N, K = 256, 640, 320
    da, packed, ref, No = _problem(ops, M, N, K, False, True, False, False, 9)
    kw = packed(80)
    w = kw.pop("w")
    out = torch.zeros((M, N), dtype=torch.float16, device=DEV)
    stats = torch.zeros((M, N // 64, 2), dtype=torch.float32, device=DEV)
    for extra in (dict(stats_out=stats), dict(tile_m=64), dict(splitk=2)):
        a = dict(tile_m=128, tile_n=160, splitk=1)
        a.update(extra)
        d = ops.make_gemm_desc(da, w, N, 1, M, 1, K, out, N, **a, **kw)
        ws = ops.new_gemm_workspace(1 << 22, DEV)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        assert not ops.gemm_check(d), extra
        with pytest.raises(MdxError):
            ops.gemm_run(d)
