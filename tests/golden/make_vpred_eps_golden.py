"""Writes tests/golden/vpred_eps_parent.npz: the final latents of the short "eps" tiny-UNet sampler runs that
tests/test_vpred_gpu.py::test_eps_sampler_runs_are_bit_identical_to_the_parent_commit compares against, bit for bit.

The committed file was recorded on an MI355X with libmdx.so, _lib.py and ops.py of commit 45a5ce3 (the one before
mdx_sampler_step_pred_f32 existed).  To record it again after an INTENDED numeric change of the eps path: build the
commit whose outputs are to be pinned, keep tests/_vpred_util.py from this tree, and on a machine with the GPU run

    python tests/golden/make_vpred_eps_golden.py

Each case is run twice and must reproduce itself before it is written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import _vpred_util as V  # noqa: E402


def main():
    model, cfg, _ = V.tiny_eps_model()
    out = {}
    for name in V.EPS_IDENTITY_CASES:
        a = V.product_trajectory(name, model, cfg["context_dim"], "cuda:0")
        b = V.product_trajectory(name, model, cfg["context_dim"], "cuda:0")
        assert torch.equal(a, b), name
        out[name] = a.cpu().numpy()
    np.savez(os.path.join(HERE, "vpred_eps_parent.npz"), **out)
    print("wrote vpred_eps_parent.npz:", ", ".join(out))


if __name__ == "__main__":
    main()
