"""Per-request steps / guidance scale / guidance rescale in one sampling batch, on the GPU: PLMS, DDIM (eta 0, and eta 1 with
seeds) and DPM-Solver on the tiny UNet read as an eps and as a v model, and DiffusionPipeline on top.

The chain to the oracle-tested scalar path is two equalities (torch.equal): lists that repeat one value equal the scalar call,
and row b of a mixed batch equals row b of the batch of the same size run with sample b's parameters -- same batch size, so
same launch plans; a sample's rows depend on that sample's inputs alone.  Only the comparison with a request served at another
batch size has a bound: BATCH_REL_L2 of test_seeded_noise_gpu.py, the project's bound for launch-plan differences.
"""
import numpy as np
import pytest
import torch

import _img2img_util as I2I
import _inpaint_util as INP
import _vpred_util as V
from test_seeded_noise_gpu import BATCH_REL_L2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LATENT = (4, 8, 8)
# steps [1, 4, 3] on DPM-Solver; PLMS / DDIM take [1, 4, 2]: make_ddim_timesteps has no 3-step grid on 1000 training steps
# (its uniform grid 1000 // 3 ends on timestep 1000 and is refused; S has to divide 1000)
DPM_STEPS, DDIM_STEPS = [1, 4, 3], [1, 4, 2]
SCALES, PHIS = [1.5, 3.0, 7.5], [0.0, 0.7, 0.3]
SEEDS = [5, 7, 9]
KINDS = ["plms", "ddim", "ddim_eta1", "dpm"]


def steps_of(kind):
    return DPM_STEPS if kind == "dpm" else DDIM_STEPS


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def tiny():
    v_model, cfg, _ = V.tiny_eps_model(parameterization="v")
    eps_model, _, _ = V.tiny_eps_model()
    rng = np.random.RandomState(301)
    d = lambda a: torch.tensor(a.astype(np.float32), device=DEV)
    return {"v": v_model, "eps": eps_model, "x_T": d(rng.randn(3, *LATENT)), "c": d(rng.randn(3, V.T, cfg["context_dim"])),
            "uc": d(np.repeat(rng.randn(1, V.T, cfg["context_dim"]), 3, 0))}


def sampler_of(kind, model):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    return {"plms": PLMSSampler, "ddim": DDIMSampler, "ddim_eta1": DDIMSampler, "dpm": DPMSolverSampler}[kind](model)


def run(tiny, param, kind, S, scale, phi, rows=slice(None), x_T=True, seeds=None, **kw):
    """One sample() on rows `rows` of the fixture's batch; ddim_eta1 draws its step noise from the rows' seeds."""
    b = len(range(3)[rows])
    if kind == "ddim_eta1":
        kw.update(eta=1.0)
        seeds = SEEDS[rows] if seeds is None else seeds
    if seeds is not None:
        kw.update(seeds=seeds)
    if x_T:
        kw.update(x_T=tiny["x_T"][rows])
    return sampler_of(kind, tiny[param]).sample(S, b, LATENT, conditioning=tiny["c"][rows],
                                                unconditional_conditioning=tiny["uc"][rows], unconditional_guidance_scale=scale,
                                                guidance_rescale=phi, verbose=False, **kw)[0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("param", ["eps", "v"])
def test_uniform_lists_equal_the_scalar_call(tiny, param, kind):
    want = run(tiny, param, kind, 4, 3.0, 0.5)
    got = run(tiny, param, kind, [4, 4, 4], [3.0, 3.0, 3.0], [0.5, 0.5, 0.5])
    assert bool(torch.isfinite(got).all())
    print(f"uniform {param} {kind}: max|d| {float((got - want).abs().max()):.3e}")
    assert torch.equal(got, want)
    # one list is enough to take the table path, and a tensor is a list
    assert torch.equal(run(tiny, param, kind, 4, torch.tensor([3.0, 3.0, 3.0]), 0.5), want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("param", ["eps", "v"])
def test_a_mixed_row_equals_the_row_of_a_uniform_batch(tiny, param, kind):
    """Row b of the mixed batch against row b of the batch-3 scalar run with sample b's steps, scale and rescale."""
    STEPS = steps_of(kind)
    mixed = run(tiny, param, kind, STEPS, SCALES, PHIS)
    assert bool(torch.isfinite(mixed).all())
    for b in range(3):
        uniform = run(tiny, param, kind, STEPS[b], SCALES[b], PHIS[b])
        print(f"mixed {param} {kind} row {b}: rel-L2 {rel_l2(mixed[b], uniform[b]):.3e}")
        assert torch.equal(mixed[b], uniform[b]), b
    assert not torch.equal(mixed[1], run(tiny, param, kind, STEPS[0], SCALES[0], PHIS[0])[1])      # the parameters do matter


@pytest.mark.parametrize("kind", KINDS)
def test_a_request_does_not_depend_on_the_batch_it_is_served_in(tiny, ops, kind, monkeypatch):
    """Sample 1 of the mixed batch against the same request -- 4 steps, scale 3, rescale 0.7, seed 7 -- served alone: every
    ops.randn_seeded draw is bit-identical, the latents differ by the launch plans of the two UNet batches."""
    STEPS = steps_of(kind)
    drawn = []
    real = ops.randn_seeded

    def spy(*a, **k):
        out = real(*a, **k)
        drawn.append(out.clone())
        return out
    monkeypatch.setattr(ops, "randn_seeded", spy)
    three = run(tiny, "v", kind, STEPS, SCALES, PHIS, x_T=False, seeds=SEEDS)
    d3, drawn[:] = list(drawn), []
    one = run(tiny, "v", kind, STEPS[1], SCALES[1], PHIS[1], rows=slice(1, 2), x_T=False, seeds=SEEDS[1:2])
    d1 = list(drawn)
    assert len(d3) == len(d1) == (1 + STEPS[1] if kind == "ddim_eta1" else 1)
    for a, b in zip(d3, d1):
        assert torch.equal(a[1], b[0])
    err = rel_l2(three[1], one[0])
    print(f"{kind}: request of seed 7 in the mixed batch vs alone, rel-L2 {err:.3e}")
    assert err <= BATCH_REL_L2


@pytest.mark.parametrize("param", ["eps", "v"])
def test_scalar_arguments_never_reach_the_table_entry(tiny, ops, monkeypatch, param):
    from minddiffusion_amd.pipeline import DiffusionPipeline

    def refuse(*a, **k):
        raise AssertionError("scalar arguments: must not go through ops.sampler_step_table")
    monkeypatch.setattr(ops, "sampler_step_table", refuse)
    for kind in KINDS:
        for scale, phi in ((3.0, 0.0), (3.0, 0.5), (1.0, 0.5)):
            assert bool(torch.isfinite(run(tiny, param, kind, 4, scale, phi)).all())
    pipe = DiffusionPipeline(tiny[param], "ddim", device=DEV)
    pipe(c=tiny["c"].cpu(), uc=tiny["uc"].cpu(), H=64, W=64, steps=4, scale=3.0, guidance_rescale=0.5)
    with pytest.raises(AssertionError, match="sampler_step_table"):
        run(tiny, param, "ddim", 4, [3.0] * 3, 0.0)


@pytest.mark.parametrize("kind", KINDS)
def test_the_table_goes_up_once_per_run(tiny, kind, monkeypatch):
    """One StepTable per sample(), uploaded once before the loop; inside the loop the launches read slices of that tensor."""
    from minddiffusion_amd.ldm.models.diffusion import schedule as G
    tables, seen = [], []
    real = G.StepTable.upload

    def upload(self, device):
        tables.append(self)
        return real(self, device)
    monkeypatch.setattr(G.StepTable, "upload", upload)

    def callback(i):
        seen.append((tables[0].uploads, tables[0].device_table.data_ptr(), len(tables)))
    STEPS = steps_of(kind)
    run(tiny, "v", kind, STEPS, SCALES, PHIS, callback=callback)
    assert len(tables) == 1 and tables[0].uploads == 1
    n_calls = max(STEPS) + int(kind == "plms")
    assert tuple(tables[0].device_table.shape) == (n_calls, 3, 16) and tables[0].device_table.is_cuda
    assert len(seen) == max(STEPS) and set(seen) == {(1, tables[0].device_table.data_ptr(), 1)}


@pytest.mark.parametrize("kind", KINDS)
def test_a_list_run_launches_the_table_entry_once_per_evaluation_and_no_scalar_entry(tiny, ops, kind, monkeypatch):
    """S = [2, 4]: max(S) launches of ops.sampler_step_table (one more for PLMS' double first step), none of the three scalar
    entries, one upload."""
    from minddiffusion_amd.ldm.models.diffusion import schedule as SCH
    S = [2, 4]
    count = {}
    for entry in ("sampler_step", "sampler_step_pred", "sampler_step_rescale", "sampler_step_table"):
        def counted(*a, _real=getattr(ops, entry), _entry=entry, **k):
            count[_entry] = count.get(_entry, 0) + 1
            return _real(*a, **k)
        monkeypatch.setattr(ops, entry, counted)
    uploads = []
    real = SCH.StepTable.upload
    monkeypatch.setattr(SCH.StepTable, "upload", lambda self, device: (uploads.append(self), real(self, device))[1])
    got = run(tiny, "v", kind, S, SCALES[:2], PHIS[:2], rows=slice(0, 2))
    assert bool(torch.isfinite(got).all())
    assert count == {"sampler_step_table": max(S) + int(kind == "plms")}
    assert len(uploads) == 1 and uploads[0].uploads == 1


@pytest.mark.parametrize("kind", KINDS)
def test_callbacks_fire_once_per_iteration_and_a_finished_row_keeps_its_prediction(tiny, kind):
    """img_callback's pred_x0 on every iteration: a row that has finished is bit-equal to its last prediction, and finite
    (DPM-Solver ping-pongs two buffers: steps [1, 4, 3] has a row that is never written in one of them by a launch)."""
    STEPS = steps_of(kind)
    preds, calls = [], []
    run(tiny, "eps", kind, STEPS, SCALES, PHIS, img_callback=lambda p, i: preds.append((i, p.clone())), callback=calls.append)
    assert [i for i, _ in preds] == calls == list(range(max(STEPS)))
    for b, s in enumerate(STEPS):
        last = preds[s - 1][1][b]
        assert bool(torch.isfinite(last).all())
        for i in range(s, max(STEPS)):
            assert torch.equal(preds[i][1][b], last), (b, i)
        if s > 1:
            assert not torch.equal(preds[s - 2][1][b], last), b       # while it runs, the prediction does move


# ------------------------------------------------------------------------------------------------ pipeline
def test_pipeline_forwards_the_lists(tiny):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.pipeline import DiffusionPipeline
    c, uc = tiny["c"][:2], tiny["uc"][:2]
    kw = dict(steps=[2, 4], scale=[2.0, 5.0], guidance_rescale=[0.0, 0.5], seeds=[3, 4])
    got = DiffusionPipeline(tiny["v"], "ddim", device=DEV)(c=c.cpu(), uc=uc.cpu(), H=64, W=64, **kw)
    direct = DDIMSampler(tiny["v"]).sample([2, 4], 2, LATENT, conditioning=c.half(), unconditional_conditioning=uc.half(),
                                           unconditional_guidance_scale=[2.0, 5.0], guidance_rescale=[0.0, 0.5], seeds=[3, 4],
                                           verbose=False)[0]
    assert bool(torch.isfinite(got).all()) and torch.equal(got, direct)


@pytest.mark.parametrize("kind", ["plms", "ddim", "dpm_solver"])
def test_img2img_takes_scale_and_rescale_lists(tiny, kind):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    pipe = DiffusionPipeline(tiny["v"], kind, device=DEV)
    z0 = torch.tensor(I2I.start_inputs()[0], device=DEV)
    kw = dict(init_latent=z0, strength=0.6, c=tiny["c"][:2].cpu(), uc=tiny["uc"][:2].cpu(), steps=5, seeds=[3, 4])
    got = pipe.img2img(scale=[2.0, 5.0], guidance_rescale=[0.0, 0.5], **kw)
    for b, (scale, phi) in enumerate(((2.0, 0.0), (5.0, 0.5))):
        uniform = pipe.img2img(scale=scale, guidance_rescale=phi, **kw)
        print(f"img2img {kind} row {b}: rel-L2 {rel_l2(got[b], uniform[b]):.3e}")
        assert torch.equal(got[b], uniform[b]), b
    with pytest.raises(ValueError, match="img2img: `strength` fixes one grid"):
        pipe.img2img(scale=2.0, **dict(kw, steps=[5, 4]))


def test_inpaint_takes_scale_and_rescale_lists():
    from minddiffusion_amd.pipeline import DiffusionPipeline
    inp = INP.pipe_inputs()
    pipe = DiffusionPipeline(INP.tiny_model(DEV), "plms", device=DEV)
    kw = dict(c=inp["c"], uc=inp["uc"], steps=INP.S, seed=11, post_noise=inp["post"], decode=False)
    got = pipe.inpaint(inp["image"], inp["mask"], scale=[2.0, 7.5], guidance_rescale=[0.0, 0.5], **kw)
    for b, (scale, phi) in enumerate(((2.0, 0.0), (7.5, 0.5))):
        uniform = pipe.inpaint(inp["image"], inp["mask"], scale=scale, guidance_rescale=phi, **kw)
        print(f"inpaint row {b}: rel-L2 {rel_l2(got[b], uniform[b]):.3e}")
        assert torch.equal(got[b], uniform[b]), b
    # strength < 1 goes through decode(): lists are allowed there too
    part = pipe.inpaint(inp["image"], inp["mask"], scale=[2.0, 7.5], strength=0.6, noise=inp["noise"], **kw)
    assert torch.equal(part[1], pipe.inpaint(inp["image"], inp["mask"], scale=7.5, strength=0.6, noise=inp["noise"], **kw)[1])
    with pytest.raises(ValueError, match="inpaint: `strength` fixes one grid"):
        pipe.inpaint(inp["image"], inp["mask"], scale=2.0, **dict(kw, steps=[5, 4]))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(tiny):
    from minddiffusion_amd._lib import MdxError
    with pytest.raises(MdxError, match="steps: 2 values for a batch of 3"):
        run(tiny, "eps", "plms", [1, 2], 3.0, 0.0)
    with pytest.raises(MdxError, match="scale: 4 values for a batch of 3"):
        run(tiny, "eps", "dpm", 3, [3.0] * 4, 0.0)
    with pytest.raises(ValueError, match="int >= 1"):
        run(tiny, "eps", "ddim", [1, 0, 2], 3.0, 0.0)
    with pytest.raises(IndexError, match="choose S dividing"):          # a sample's own grid is the existing function's
        run(tiny, "eps", "ddim", [1, 4, 3], 3.0, 0.0)
    for kind in ("plms", "dpm"):
        with pytest.raises(ValueError, match="guidance_rescale"):
            run(tiny, "eps", kind, 4, 3.0, [0.0, 1.5, 0.0])

    class Identity:
        def modify_score(self, model, e_t, x, t, c, **kw):
            return e_t
    for kind in ("ddim", "dpm"):
        with pytest.raises(ValueError, match="score_corrector"):
            run(tiny, "eps", kind, 4, [3.0] * 3, 0.0, score_corrector=Identity())
    mask, x0 = torch.ones(3, 1, 8, 8, device=DEV), tiny["x_T"]
    with pytest.raises(ValueError, match="per-sample S"):
        run(tiny, "eps", "ddim", [2, 4, 4], 3.0, 0.0, mask=mask, x0=x0)
    with pytest.raises(ValueError, match="per-sample S"):
        run(tiny, "eps", "dpm", [2, 3, 3], 3.0, 0.0, t_start=0.5)
    # scale and rescale lists are allowed with a mask (the blend draws come from the seeds: the two runs see the same ones)
    mask[:, :, 4:] = 0.0
    got = run(tiny, "eps", "ddim", 4, SCALES, PHIS, mask=mask, x0=x0, seeds=SEEDS)
    assert torch.equal(got[1], run(tiny, "eps", "ddim", 4, SCALES[1], PHIS[1], mask=mask, x0=x0, seeds=SEEDS)[1])
