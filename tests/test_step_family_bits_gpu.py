"""Every launch form of the fused sampler step family gives the bits it gave at the parent commit.

tests/golden/sampler_paths_parent.npz and request_paths_parent.npz pin whole sampler runs on a 2 x 4 x 8 x 8 latent: 256
elements per sample, one trip of every loop and no partial quad.  tests/golden/step_family_parent.json pins the kernels
themselves: a SHA-256 digest of every output tensor of the single launches of tests/_step_family_cases.py -- every kernel
instantiation of csrc/sampler_step.hip on shapes with a partial last quad, quads that straddle channels and a second trip of
the one-workgroup-per-sample loops -- recorded on an MI355X against the library of the commit before the family's arithmetic
was written once per family (tests/golden/make_step_family_parent_golden.py).  The tolerance is zero: the kernels are
deterministic and the arithmetic is meant to be the same."""
import json
import os

import pytest

import _step_family_cases as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
with open(os.path.join(ROOT, "tests", "golden", "step_family_parent.json")) as _f:
    GOLD = json.load(_f)


@pytest.fixture(scope="module")
def got():
    from minddiffusion_amd import ops
    return S.digests(ops, DEV)


def test_the_golden_file_and_the_case_table_name_the_same_cases(got):
    assert sorted(GOLD) == sorted(S.cases())
    assert sorted(GOLD) == sorted(got)


@pytest.mark.parametrize("name", sorted(GOLD))
def test_launch_is_bit_identical_to_the_parent_commit(got, name):
    assert got[name] == GOLD[name], name
