"""Writes tests/golden/seeded_parent.npz: the final latents of the `seeds=None` sampler runs that
tests/test_seeded_noise_gpu.py::test_default_runs_are_bit_identical_to_the_parent_commit compares against, bit for bit.

The committed file was recorded on an MI355X with the library and samplers of commit a9a6743 (the one before the samplers
took `seeds=`).  To record it again after an INTENDED numeric change of the default path: build the commit whose outputs
are to be pinned, keep tests/_seeded_default_runs.py from this tree, and on a machine with the GPU run

    python tests/golden/make_seeded_parent_golden.py [output directory]

Each case is run twice and must reproduce itself before it is written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import _seeded_default_runs as R  # noqa: E402
import _vpred_util as V  # noqa: E402


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else HERE
    model, cfg, _ = V.tiny_eps_model()
    a = R.default_runs(model, cfg["context_dim"], "cuda:0")
    b = R.default_runs(model, cfg["context_dim"], "cuda:0")
    out = {}
    for name in a:
        assert torch.equal(a[name], b[name]), name
        out[name] = a[name].cpu().numpy()
    os.makedirs(dst, exist_ok=True)
    np.savez(os.path.join(dst, "seeded_parent.npz"), **out)
    print("wrote seeded_parent.npz:", ", ".join(out))


if __name__ == "__main__":
    main()
