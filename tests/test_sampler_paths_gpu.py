"""The LDM sampling path computes what it computed at the parent commit, through the library entries it went through there.

tests/golden/sampler_paths_parent.npz holds the final latent of every run of tests/_sampler_paths.py, recorded on an MI355X
before the samplers shared one guided-model call and one step dispatch (tests/golden/make_sampler_paths_parent_golden.py).
The tolerance is zero: the host code only decides which launches are made with which arguments, and include/mdx.h documents
the three step entries as bit-identical where they overlap -- which is also why the second test counts the entries: a switched
entry would not show in the latents."""
import os

import numpy as np
import pytest
import torch

import _sampler_paths as P
import _vpred_util as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.fixture(scope="module")
def models():
    return P.build_models(DEV)


@pytest.fixture(scope="module")
def paths(models):
    return {name: t.cpu().numpy() for name, t in P.sampler_paths(models, DEV).items()}


GOLD = np.load(os.path.join(ROOT, "tests", "golden", "sampler_paths_parent.npz"))


def test_the_golden_file_and_the_runs_name_the_same_cases(paths):
    assert sorted(GOLD.files) == sorted(paths)


@pytest.mark.parametrize("name", sorted(GOLD.files))
def test_paths_are_bit_identical_to_the_parent_commit(paths, name):
    assert np.array_equal(paths[name], GOLD[name]), name


# ------------------------------------------------------------------------------------------------ which entry is launched
S = 4
# case -> (model, sample() keywords, guidance scale, {entry: launches per model evaluation})
ENTRY_CASES = {
    "eps": ("eps", {}, 3.0, {"sampler_step": 1}),
    "v": ("v", {}, 3.0, {"sampler_step_pred": 1}),
    "rescale_cfg": ("eps", dict(guidance_rescale=0.7), 3.0, {"sampler_step_rescale": 1}),
    "v_rescale_cfg": ("v", dict(guidance_rescale=0.7), 3.0, {"sampler_step_rescale": 1}),
    "rescale_scale1": ("eps", dict(guidance_rescale=0.7), 1.0, {"sampler_step": 1}),
    # a corrector: pass 1 (the CFG combine, where the rescale belongs), then pass 2 on the corrected eps, one half, no rescale
    "corrector": ("eps", dict(score_corrector=True), 3.0, {"sampler_step": 2}),
    "corrector_rescale": ("eps", dict(score_corrector=True, guidance_rescale=0.7), 3.0,
                          {"sampler_step_rescale": 1, "sampler_step": 1}),
}


# (DPMSolverSampler takes no score corrector)
ENTRY_RUNS = [(case, kind) for case in sorted(ENTRY_CASES) for kind in ("plms", "ddim", "dpm")
              if not (kind == "dpm" and "score_corrector" in ENTRY_CASES[case][1])]


@pytest.mark.parametrize("case,kind", ENTRY_RUNS)
def test_the_step_entry_launched_is_the_one_the_parent_launched(models, monkeypatch, case, kind):
    """Evaluations: S for DDIM / DPM-Solver, S + 1 for PLMS; every evaluation launches exactly the entries of its case."""
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    model, kw, scale, per_eval = ENTRY_CASES[case]
    kw = dict(kw)
    if kw.pop("score_corrector", False):
        kw["score_corrector"] = P._Corrector()
    count = {}
    for entry in ("sampler_step", "sampler_step_pred", "sampler_step_rescale"):
        def counted(*a, _real=getattr(ops, entry), _entry=entry, **k):
            count[_entry] = count.get(_entry, 0) + 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, entry, counted)
    d = lambda a: torch.tensor(a, device=DEV)
    x_T, c, uc = (d(a) for a in V.tiny_inputs(models["ctx_dim"]))
    cls = {"plms": PLMSSampler, "ddim": DDIMSampler, "dpm": DPMSolverSampler}[kind]
    cls(models[model]).sample(S, V.B, (4, V.H, V.W), conditioning=c, x_T=x_T, unconditional_guidance_scale=scale,
                              unconditional_conditioning=uc, verbose=False, **kw)
    evals = S + (kind == "plms")
    assert count == {entry: n * evals for entry, n in per_eval.items()}
