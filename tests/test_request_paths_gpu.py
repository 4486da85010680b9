"""The per-request and session paths compute what they computed at the parent commit.

tests/golden/sampler_paths_parent.npz pins scalar runs only.  tests/golden/request_paths_parent.npz holds the final latents of
the runs of tests/_request_paths.py -- sample() with per-sample lists (the StepTable path) for the three samplers on the eps
and the v model, and DiffusionPipeline.serve through two slots (the rows of a session) -- recorded on an MI355X before the
samplers built their launches from one step plan (tests/golden/make_request_paths_parent_golden.py).  The tolerance is zero:
the host code only decides which launches are made with which rows."""
import os

import numpy as np
import pytest

import _request_paths as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "request_paths_parent.npz"))


@pytest.fixture(scope="module")
def paths():
    return {name: t.cpu().numpy() for name, t in P.request_paths(P.build_models(DEV), DEV).items()}


def test_the_golden_file_and_the_runs_name_the_same_cases(paths):
    assert sorted(GOLD.files) == sorted(paths)


@pytest.mark.parametrize("name", sorted(GOLD.files))
def test_paths_are_bit_identical_to_the_parent_commit(paths, name):
    assert np.array_equal(paths[name], GOLD[name]), name
