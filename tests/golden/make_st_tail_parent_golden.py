"""Writes tests/golden/st_tail_parent.npz: the stage-0 output of mdx_st_tail_f16 at B = 1, tokens = 64, C = 320, a 77-token context
in a capacity-80 buffer, heads 5 and 8 at tile_rows 64 and 32 -- what
tests/test_long_context_gpu.py::test_st_tail_one_chunk_keeps_the_parent_bits compares against, bit for bit.

The committed file was recorded on an MI355X with the libmdx.so of commit 193299c (the one before the fused tail took
contexts of more than 96 keys).  To record it again after an INTENDED numeric change of the one-chunk path: build the commit
whose outputs are to be pinned (MDX_LIBRARY may name its libmdx.so), keep tests/test_stchain_gpu.py from this tree, and on a
machine with the GPU run

    python tests/golden/make_st_tail_parent_golden.py

Each case is run twice and must reproduce itself before it is written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import test_stchain_gpu as S  # noqa: E402

B, TOKENS, C, CTX_LEN, CAP = 1, 64, 320, 77, 80
CASES = [(heads, rows) for heads in (5, 8) for rows in (64, 32)]


def case_inputs(heads):
    return S.make_case(300 + heads, B, TOKENS, C, heads, CTX_LEN, 1024 if heads == 5 else 768, ctx_cap=CAP)


def main():
    from minddiffusion_amd import ops
    out = {}
    for heads, rows in CASES:
        w, x = case_inputs(heads)
        a, _ = S.run_fused(ops, w, x, B, TOKENS, C, heads, CTX_LEN, rows, 0, ctx_cap=CAP)
        b, _ = S.run_fused(ops, w, x, B, TOKENS, C, heads, CTX_LEN, rows, 0, ctx_cap=CAP)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (heads, rows)
        out[f"h{heads}_r{rows}"] = a.cpu().numpy()
    np.savez(os.path.join(HERE, "st_tail_parent.npz"), **out)
    print("wrote st_tail_parent.npz:", ", ".join(out))


if __name__ == "__main__":
    main()
