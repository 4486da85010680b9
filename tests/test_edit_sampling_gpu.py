"""InstructPix2Pix editing on the GPU: the three samplers under three-branch guidance against the unchanged oracle samplers on
the proxy model of tests/_edit_util.py, pipe.edit against its hand composition, and the launches an edit run makes.

Bound: the project's for short tiny-UNet trajectories, rel-L2 <= 1e-2 (and max|d| <= 1e-2 max|ref| where
test_inpaint_gpu.test_dpm_solver_hybrid_vs_oracle uses it: DPM-Solver)."""
import numpy as np
import pytest
import torch

import _dpm_full_util as DF
import _edit_util as E
from _util import check
from oracle import dpm_solver as OD
from oracle import ldm as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model():
    return E.edit_model(DEV)


@pytest.fixture(scope="module")
def inp():
    return E.edit_inputs()


def _sampler(model, kind, **kw):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    return {"plms": PLMSSampler, "ddim": DDIMSampler, "dpm_solver": DPMSolverSampler}[kind](model, **kw)


def _run(model, kind, inp, S=E.S, s_t=E.S_T, s_i=E.S_I, **kw):
    cond, uc = E.dicts(inp, DEV)
    return _sampler(model, kind).sample(S, E.B, E.SHAPE, conditioning=cond, x_T=torch.tensor(inp["x_T"], device=DEV),
                                        unconditional_guidance_scale=s_t, unconditional_conditioning=uc, verbose=False,
                                        image_guidance_scale=s_i, **kw)[0]


def _pipe(model, kind, **kw):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    return DiffusionPipeline(model, kind, device=DEV, **kw)


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("kind", ["plms", "ddim", "dpm_solver"])
def test_three_branch_sampling_vs_proxy_oracle(model, inp, kind):
    proxy = E.EditProxy(inp["c_cat"], inp["c"], inp["uc"])
    got = _run(model, kind, inp)
    if kind == "dpm_solver":
        ref = OD.sample(proxy, E.S, E.B, E.SHAPE, inp["c"], inp["x_T"])[0]
        check("tiny_edit_dpm_solver", got, ref, rel_l2=1e-2, max_rel=1e-2)
    else:
        ref = O.sample(proxy, E.S, E.B, E.SHAPE, inp["c"], inp["x_T"], kind)[0]
        check(f"tiny_edit_{kind}", got, ref, rel_l2=1e-2)
    assert proxy.calls == (E.S + 1 if kind == "plms" else E.S)             # one three-branch evaluation each


def test_three_branch_ddim_with_guidance_rescale_vs_proxy_oracle(model, inp):
    proxy = E.EditProxy(inp["c_cat"], inp["c"], inp["uc"], phi=0.7)
    got = _run(model, "ddim", inp, guidance_rescale=0.7)
    check("tiny_edit_ddim_rescale0.7", got, O.sample(proxy, E.S, E.B, E.SHAPE, inp["c"], inp["x_T"], "ddim")[0], rel_l2=1e-2)
    assert float((got - _run(model, "ddim", inp)).norm() / got.norm()) > 1e-3, "the rescale changed nothing"


# ------------------------------------------------------------------------------------------------ the pipeline
@pytest.mark.parametrize("kind", ["plms", "ddim", "dpm_solver"])
def test_edit_is_the_hand_composition(model, inp, kind):
    pipe = _pipe(model, kind)
    image = torch.tensor(inp["image"])
    c, uc = torch.tensor(inp["c"]), torch.tensor(inp["uc"])
    kw = dict(c=c, uc=uc, steps=E.S, scale=E.S_T, image_scale=E.S_I, seed=11, decode=False)
    got = pipe.edit(image, **kw)
    assert tuple(got.shape) == (E.B,) + E.SHAPE
    # c_concat: the posterior mode, not scaled
    c_cat = model.first_stage_model.encode(image.to(DEV), sample=False)
    assert torch.equal(model.encode_edit_image(image.to(DEV)), c_cat)
    cond, ucd = E.dicts(inp, DEV, c_cat=c_cat)
    x_T = pipe.start_noise(E.B, E.SHAPE, 11).to(DEV)
    want = _sampler(model, kind).sample(E.S, E.B, E.SHAPE, conditioning=cond, x_T=x_T, unconditional_guidance_scale=E.S_T,
                                        unconditional_conditioning=ucd, verbose=False, eta=0.0, image_guidance_scale=E.S_I)[0]
    assert torch.equal(got, want)
    # a batch-1 image is the expanded one
    assert torch.equal(pipe.edit(image[:1], **kw), pipe.edit(image[:1].expand(2, -1, -1, -1), **kw))


def test_edit_edits_and_rows_do_not_depend_on_their_neighbours(model, inp):
    pipe = _pipe(model, "ddim")
    image = torch.tensor(inp["image"])
    c, uc = torch.tensor(inp["c"]), torch.tensor(inp["uc"])
    kw = dict(steps=E.S, scale=E.S_T, decode=False)
    base = pipe.edit(image, c=c, uc=uc, seeds=[5, 6], **kw)
    assert not torch.equal(base, pipe.edit(image, c=c, uc=uc, seeds=[5, 6], image_scale=0.5, **kw))
    assert not torch.equal(base, pipe.edit(image.flip(0), c=c, uc=uc, seeds=[5, 6], **kw))
    assert torch.equal(base, pipe.edit(image, c=c, uc=uc, seeds=[5, 6], **kw))
    alone = pipe.edit(image[1:], c=c[1:], uc=uc[1:], seeds=[6], eta=0.5, **kw)
    both = pipe.edit(image, c=c, uc=uc, seeds=[5, 6], eta=0.5, **kw)
    assert torch.equal(alone[0], both[1])
    # decoded outputs
    x = pipe.edit(image, c=c, uc=uc, seeds=[5, 6], steps=2)
    u8 = pipe.edit(image, c=c, uc=uc, seeds=[5, 6], steps=2, output="uint8")
    assert tuple(x.shape) == (E.B, 3, E.IMG, E.IMG) and float(x.min()) >= 0. and float(x.max()) <= 1.
    assert u8.dtype == torch.uint8 and torch.equal(u8, (x * 255).to(torch.uint8).permute(0, 2, 3, 1))


STEP_OPS = ("sampler_step", "sampler_step_pred", "sampler_step_rescale", "sampler_step_dual", "sampler_step_table",
            "sampler_step_lin", "sampler_step_lin_noise", "sampler_step_lin_dual", "randn_seeded", "q_sample", "nchw_to_nhwc")


@pytest.mark.parametrize("kind,solver", [("plms", None), ("ddim", None), ("dpm_solver", None), ("dpm_solver", dict(order=3))])
def test_edit_launch_count(model, inp, monkeypatch, kind, solver):
    """One step launch per model evaluation, and no per-step launch the two-branch hybrid run does not make."""
    from minddiffusion_amd import ops
    count = {}
    for name in STEP_OPS:
        real = getattr(ops, name)

        def counted(*a, _real=real, _name=name, **k):
            count[_name] = count.get(_name, 0) + 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    evals = []
    real_eval = model.apply_model_nhwc
    monkeypatch.setattr(model, "apply_model_nhwc", lambda x, *a, **k: evals.append(int(x.shape[0])) or real_eval(x, *a, **k))
    cond, uc = E.dicts(inp, DEV)
    x_T = torch.tensor(inp["x_T"], device=DEV)
    kw = dict(conditioning=cond, x_T=x_T, unconditional_guidance_scale=E.S_T, unconditional_conditioning=uc, verbose=False)
    s = _sampler(model, kind, **(solver or {}))
    s.sample(E.S, E.B, E.SHAPE, image_guidance_scale=E.S_I, **kw)
    dual, n_dual = dict(count), list(evals)
    count.clear()
    del evals[:]
    s.sample(E.S, E.B, E.SHAPE, **kw)
    pair, n_pair = dict(count), list(evals)
    assert n_dual == [3 * E.B] * len(n_pair) and n_pair == [2 * E.B] * len(n_pair)
    entry = "sampler_step_lin_dual" if solver else "sampler_step_dual"
    assert dual.pop(entry) == len(n_dual)                                   # exactly one step launch per model evaluation
    pair_steps = sum(pair.pop(k, 0) for k in ("sampler_step", "sampler_step_pred", "sampler_step_rescale", "sampler_step_lin"))
    assert pair_steps == len(n_pair)
    # nothing else that the pair run does not make as well (a run's first call at a new UNet batch may add set-up launches)
    assert all(n <= pair.get(k, 0) for k, n in dual.items()), (dual, pair)


# ------------------------------------------------------------------------------------------------ DPM-Solver options
def test_dpm_solver_options_with_image_guidance(model, inp):
    run = lambda **kw: _run(model, "dpm_solver", inp, S=6, **kw)
    a = run(order=3, skip_type="logSNR", method="singlestep")
    assert torch.equal(a, run(order=3, skip_type="logSNR", method="singlestep")) and bool(torch.isfinite(a).all())
    proxy = E.EditProxy(inp["c_cat"], inp["c"], inp["uc"])
    ref = DF.sample(proxy, 6, E.B, E.SHAPE, inp["c"], inp["x_T"], order=3, skip_type="logSNR", method="singlestep")[0]
    check("tiny_edit_dpm_order3_logSNR_singlestep", a, ref, rel_l2=1e-2, max_rel=1e-2)
    b = run(skip_type="karras", sde_eta=1.0, seeds=[7, 8])
    assert torch.equal(b, run(skip_type="karras", sde_eta=1.0, seeds=[7, 8])) and bool(torch.isfinite(b).all())
    assert not torch.equal(b, run(skip_type="karras", sde_eta=1.0, seeds=[7, 9]))
    t = run(thresholding=True, max_val=1.0, guidance_rescale=0.5)
    assert torch.equal(t, run(thresholding=True, max_val=1.0, guidance_rescale=0.5)) and bool(torch.isfinite(t).all())
