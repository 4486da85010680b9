"""GEGLU packing units (ops.geglu_interleave / geglu_repack; include/mdx.h mdx_gemm_desc.geglu_unit): pure data movement, no GPU."""
import ctypes

import pytest
import torch

from minddiffusion_amd import ops
from minddiffusion_amd._lib import GemmDesc


@pytest.mark.parametrize("unit", [64, 80])
@pytest.mark.parametrize("half,K", [(320, 64), (1280, 320), (5120, 128)])
def test_geglu_pack_roundtrip(unit, half, K):
    g = torch.Generator().manual_seed(half + K + unit)
    w = torch.randn((2 * half, K), generator=g).to(torch.float16)
    b = torch.randn(2 * half, generator=g)
    wi = ops.geglu_interleave(w[:half], w[half:], unit)
    bi = ops.geglu_interleave(b[:half], b[half:], unit)
    # every 2 * unit-wide tile: `unit` 'a' rows, then the gate rows of the SAME output columns
    for t in (0, half // unit - 1):
        assert torch.equal(wi[2 * unit * t:2 * unit * t + unit], w[unit * t:unit * t + unit])
        assert torch.equal(wi[2 * unit * t + unit:2 * unit * (t + 1)], w[half + unit * t:half + unit * (t + 1)])
        assert torch.equal(bi[2 * unit * t + unit:2 * unit * (t + 1)], b[half + unit * t:half + unit * (t + 1)])
    a2, g2 = ops.geglu_deinterleave(wi, unit)
    assert torch.equal(a2, w[:half]) and torch.equal(g2, w[half:])
    # through the kernel's packed storage and back (what the planner does when a plan wants the other unit)
    packed = ops.pack_gemm_weight(wi)
    assert torch.equal(ops.unpack_gemm_weight(packed, 2 * half, K), wi)
    other = 80 if unit == 64 else 64
    re = ops.pack_gemm_weight(ops.geglu_repack(ops.unpack_gemm_weight(packed, 2 * half, K), unit, other))
    assert torch.equal(re, ops.pack_gemm_weight(ops.geglu_interleave(w[:half], w[half:], other)))
    assert torch.equal(ops.geglu_repack(ops.geglu_repack(bi, unit, other), other, unit), bi)


def test_geglu_unit_64_is_the_packing_the_loader_always_made():
    half, K = 640, 64
    w = torch.arange(2 * half * K, dtype=torch.float32).reshape(2 * half, K)
    nt = half // 64
    old = torch.stack([w[:half].reshape(nt, 64, K), w[half:].reshape(nt, 64, K)], 1).reshape(2 * half, K)
    assert torch.equal(ops.geglu_interleave(w[:half], w[half:], 64), old)
    assert torch.equal(ops.geglu_interleave(w[:half], w[half:]), old)


def test_geglu_unit_is_the_last_field_of_the_descriptor():
    """Same field order on both sides of the C ABI (include/mdx.h): geglu_unit follows act_slope_n at the end of mdx_gemm_desc."""
    names = [f[0] for f in GemmDesc._fields_]
    assert names[-2:] == ["act_slope_n", "geglu_unit"]
    assert GemmDesc.geglu_unit.offset == GemmDesc.act_slope_n.offset + ctypes.sizeof(ctypes.c_int)
    src = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "mdx.h")).read()
    body = src[src.index("typedef struct mdx_gemm_desc"):src.index("} mdx_gemm_desc;")] if "typedef struct mdx_gemm_desc" in src else src[:src.index("} mdx_gemm_desc;")]
    assert body.rstrip().endswith("int geglu_unit;")



def test_tile160_table_is_well_formed():
    """csrc/gemm_tuned160.inc: the rows of the 128 x 160 tile, consulted in front of gemm_tuned.inc -- tile 128 x 160, unsplit, ring 2 | 3,
    dense (ksize 1), a launch variant the tile carries (no statistics / split store / row bias bits), one row per shape and variant."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minddiffusion_amd", "csrc", "gemm_tuned160.inc")
    seen = set()
    for ln in open(path):
        if ln.lstrip().startswith("//") or not ln.strip():
            continue
        m = re.match(r"\s*\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\},", ln)
        assert m, ln
        M, N, K, ks, bm, bn, ns, var1, st = map(int, m.groups())
        assert M > 0 and N % 8 == 0 and K % 64 == 0 and ks == 1 and (bm, bn, ns) == (128, 160, 1) and st in (2, 3)
        var = var1 - 1
        assert var >= 0 and not var & (1 | 8 | 32 | 64 | 128 | 512 | 1024 | 2048), ln
        assert ((var >> 1) & 3) in (0, 1) and (((var >> 1) & 3) == 0 or N % 160 == 0), ln
        assert (M, N, K, var1) not in seen, f"duplicate shape {ln}"
        seen.add((M, N, K, var1))
