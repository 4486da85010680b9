"""Writes tests/golden/request_paths_parent.npz: the final latents of the runs of tests/_request_paths.py, which
tests/test_request_paths_gpu.py::test_paths_are_bit_identical_to_the_parent_commit compares against, bit for bit.

The committed file was recorded on an MI355X with the library, samplers, session and pipeline of commit 010c9c4 (the one
before the samplers built their launches from one step plan).  To record it again after an INTENDED numeric change: build the
commit whose outputs are to be pinned, keep tests/_request_paths.py from this tree, and on a machine with the GPU run

    python tests/golden/make_request_paths_parent_golden.py [output directory]

Each case is run twice and must reproduce itself before it is written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import _request_paths as P  # noqa: E402


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else HERE
    models = P.build_models("cuda:0")
    a = P.request_paths(models, "cuda:0")
    b = P.request_paths(models, "cuda:0")
    out = {}
    for name in a:
        assert torch.equal(a[name], b[name]), name
        assert torch.isfinite(a[name]).all(), name
        out[name] = a[name].cpu().numpy()
    os.makedirs(dst, exist_ok=True)
    np.savez(os.path.join(dst, "request_paths_parent.npz"), **out)
    print(f"wrote request_paths_parent.npz ({len(out)} cases):", ", ".join(out))


if __name__ == "__main__":
    main()
