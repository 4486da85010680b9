"""Writes tests/golden/step_family_parent.json: one SHA-256 digest per case and output tensor of the launches of
tests/_step_family_cases.py, which tests/test_step_family_bits_gpu.py compares against, bit for bit.

The committed file was recorded on an MI355X with the library of commit 8dbf1f2 (the one before the step family moved to
csrc/sampler_step.hip and its arithmetic was written once per family).  To record it again after an INTENDED numeric change:
build the library whose outputs are to be pinned, select it with MDX_LIBRARY (or build it in place), keep
tests/_step_family_cases.py from this tree, and on a machine with the GPU run

    python tests/golden/make_step_family_parent_golden.py [output directory]

Each case is run twice and must reproduce itself before it is written.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import _step_family_cases as S  # noqa: E402


def main():
    from minddiffusion_amd import ops
    dst = sys.argv[1] if len(sys.argv) > 1 else HERE
    a = S.digests(ops, "cuda:0")
    b = S.digests(ops, "cuda:0")
    for name in a:
        assert a[name] == b[name], name
    os.makedirs(dst, exist_ok=True)
    with open(os.path.join(dst, "step_family_parent.json"), "w") as f:
        json.dump(a, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote step_family_parent.json ({len(a)} cases, {sum(len(v) for v in a.values())} digests)")


if __name__ == "__main__":
    main()
