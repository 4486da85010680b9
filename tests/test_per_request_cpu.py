"""Per-request steps / guidance scale / guidance rescale -- the parts that need no GPU: the StepTable every sampler builds
before its loop holds, per sample, the very float32 scalars the scalar path computes for that sample's step count alone
(through the shared functions of schedule.py), rows beyond a sample's last step are inactive, the model-input timesteps follow
each sample's own grid; and the validation of the builder and of the pipeline's list checks."""
import numpy as np
import pytest

from minddiffusion_amd import ops
from minddiffusion_amd._lib import MdxError
from minddiffusion_amd.ldm.models.diffusion import schedule as G
from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP, multistep_2m_plan
from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler

STEPS = [2, 5, 5, 1]
SCALES = [1.5, 3.0, 7.5, 1.0]
PHIS = [0.0, 0.7, 0.3, 1.0]


class StubModel:
    """What a sampler reads of a LatentDiffusion before it touches the device: the SD linear schedule."""
    num_timesteps = 1000
    parameterization = "eps"

    def __init__(self):
        self.betas = np.linspace(0.00085 ** 0.5, 0.0120 ** 0.5, 1000, dtype=np.float64) ** 2
        self.alphas_cumprod = np.cumprod(1.0 - self.betas)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])


def bits(values):
    return np.asarray([np.float32(float(v)) for v in values], np.float32).view(np.uint32)


def assert_row(row, scale, phi, model_point, coef, update, tag):
    assert row[ops.STEP_ACTIVE] == 1.0, tag
    got = row.view(np.uint32)
    assert got[ops.STEP_CFG_SCALE] == bits([scale])[0] and got[ops.STEP_RESCALE] == bits([phi])[0], tag
    assert np.array_equal(got[ops.STEP_SQRT_AT_MODEL:ops.STEP_SQRT_ONE_MINUS_AT_MODEL + 1], bits(model_point)), tag
    assert np.array_equal(got[ops.STEP_C0:ops.STEP_C0 + 4], bits(coef)), tag
    assert np.array_equal(got[ops.STEP_SQRT_AT:ops.STEP_SIGMA + 1], bits(update)), tag
    assert not row[14:].any(), tag


def assert_inactive(row, tag):
    assert not row.any(), tag


def test_row_layout_matches_the_header():
    """ops.STEP_* are the MDX_STEP_* of include/mdx.h."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "mdx.h")).read()
    macros = {k: int(v) for k, v in re.findall(r"#define MDX_STEP_(\w+) (\d+)", hdr)}
    assert macros == {"ROW": ops.STEP_ROW, "ACTIVE": ops.STEP_ACTIVE, "CFG_SCALE": ops.STEP_CFG_SCALE,
                      "RESCALE": ops.STEP_RESCALE, "SQRT_AT_MODEL": ops.STEP_SQRT_AT_MODEL,
                      "SQRT_ONE_MINUS_AT_MODEL": ops.STEP_SQRT_ONE_MINUS_AT_MODEL, "C0": ops.STEP_C0,
                      "SQRT_AT": ops.STEP_SQRT_AT, "SQRT_ONE_MINUS_AT": ops.STEP_SQRT_ONE_MINUS_AT,
                      "SQRT_A_PREV": ops.STEP_SQRT_A_PREV, "DIR_COEF": ops.STEP_DIR_COEF, "SIGMA": ops.STEP_SIGMA}
    assert ops.STEP_ROW == 16 and ops.STEP_SIGMA == 13


@pytest.mark.parametrize("cls,eta", [(PLMSSampler, 0.0), (DDIMSampler, 0.0), (DDIMSampler, 0.5)])
def test_plms_ddim_table_rows_are_each_samples_own_scalars(cls, eta):
    model = StubModel()
    sampler = cls(model)
    grids = {}
    for s in sorted(set(STEPS)):
        sampler.make_schedule(s, ddim_eta=eta, verbose=False)
        grids[s] = sampler.time_grid(False, None, None)
    multistep = cls is PLMSSampler
    table, t_rows, total = G.step_table([G.ddim_steps(sampler, grids[s], multistep) for s in STEPS], SCALES, PHIS, True,
                                        second_call_row=multistep)
    host = table.host()
    assert total == max(STEPS) and host.shape == (total + int(multistep), len(STEPS), ops.STEP_ROW)
    assert t_rows.shape == (total + int(multistep), len(STEPS))
    for b, s in enumerate(STEPS):
        # what the scalar path does for S = s alone (plms_sampling's loop): its own sampler, schedule and grid
        alone = cls(model)
        alone.make_schedule(s, ddim_eta=eta, verbose=False)
        time_range, alphas, alphas_prev, sqrt_1m, sigmas = alone.time_grid(False, None, None)
        assert time_range.shape[0] == s
        point = lambda t: (alone.sqrt_alphas_cumprod[int(t)], alone.sqrt_one_minus_alphas_cumprod[int(t)])
        k = 0
        for i in range(total):
            if i >= s:
                for kk in range(k, k + (2 if multistep and i == 0 else 1)):
                    assert_inactive(host[kk, b], (b, i))
                assert t_rows[i, b] == time_range[-1]              # an ended sample keeps its last timestep
                k += 1
                continue
            update = G.ddim_step_scalars(alphas, alphas_prev, sqrt_1m, sigmas, s - i - 1)
            assert (float(update[4]) != 0) == (eta != 0)
            assert t_rows[i, b] == time_range[i]
            if multistep and i == 0:
                i_next = min(1, s - 1)
                assert_row(host[0, b], SCALES[b], PHIS[b], point(time_range[0]), G.PLMS_FIRST, update, (b, "first"))
                assert_row(host[1, b], SCALES[b], PHIS[b], point(time_range[i_next]), G.PLMS_SECOND, update, (b, "second"))
                assert t_rows[total, b] == time_range[i_next]
                k = 2
                continue
            coef = G.PLMS_AB[min(i, 3)] if multistep else (1., 0., 0., 0.)
            assert_row(host[k, b], SCALES[b], PHIS[b], point(time_range[i]), coef, update, (b, i))
            k += 1
    assert G.PLMS_AB[1:] == ((3. / 2, -1. / 2, 0., 0.), (23. / 12, -16. / 12, 5. / 12, 0.),
                             (55. / 24, -59. / 24, 37. / 24, -9. / 24))


def test_dpm_table_rows_are_each_samples_own_plan():
    model = StubModel()
    ns = NoiseScheduleVP("discrete", alphas_cumprod=DPMSolverSampler(model).alphas_cumprod)
    table, t_rows, total = G.step_table([G.dpm_steps(ns, s) for s in STEPS], SCALES, PHIS, True)
    host = table.host()
    assert total == max(STEPS) and host.shape == (total, len(STEPS), ops.STEP_ROW) and t_rows.shape == (total, len(STEPS))
    f = np.float32
    for b, s in enumerate(STEPS):
        plan = multistep_2m_plan(ns, s, order=2 if s >= 2 else 1, lower_order_final=True)      # sampler.py's call for S = s
        assert len(plan) == s
        for k in range(total):
            if k >= s:
                assert_inactive(host[k, b], (b, k))
                assert t_rows[k, b] == f(plan[-1]["t_input"])
                continue
            p = plan[k]
            update = (f(p["alpha"]), f(p["sigma"]), f(p["A"] * p["alpha"] + p["c0"]), f(p["A"] * p["sigma"]), f(p["c1"]))
            assert update == G.dpm_step_scalars(p)
            assert_row(host[k, b], SCALES[b], PHIS[b], (f(p["alpha"]), f(p["sigma"])), (1., 0., 0., 0.), update, (b, k))
            assert t_rows[k, b] == f(p["t_input"])
        # order and lower_order_final are the sample's own: its first and (for 2 <= S < 15) its last step are first order
        c1 = host[:s, b, ops.STEP_SIGMA]
        assert c1[0] == 0 and (s < 2 or c1[s - 1] == 0) and all(c1[1:s - 1] != 0)
    up = table.uploads
    assert up == 0 and table.device_table is None                    # nothing has gone to a device


def test_unguided_table_never_rescales():
    t = G.StepTable([1.0, 1.0], [0.7, 0.3], guided=False)
    t.append([((1, 0), (1, 0, 0, 0), (.5, .5, .7, .1, 0)), None])
    assert not t.host()[..., ops.STEP_RESCALE].any()


def test_builder_validation():
    row = ((0.8, 0.6), (1., 0., 0., 0.), (0.5, 0.5, 0.7, 0.1, 0.0))
    with pytest.raises(MdxError, match="batch of 2"):
        G.StepTable([1.0, 2.0], [0.0])
    with pytest.raises(MdxError, match="batch of 2"):
        G.StepTable([1.0, 2.0], [0.0, 0.0]).append([row])
    for bad, what in (((0.8, float("nan")), "finite"), ((0.8, float("inf")), "finite")):
        t = G.StepTable([1.0, 2.0], [0.0, 0.0])
        t.append([row, (bad, row[1], row[2])])
        with pytest.raises(ValueError, match=what):
            t.host()
    t = G.StepTable([1.0, float("inf")], [0.0, 0.0])
    t.append([row, row])
    with pytest.raises(ValueError, match="finite"):
        t.host()
    t = G.StepTable([1.0, 2.0], [0.0, 1.5])
    t.append([row, row])
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        t.host()
    t = G.StepTable([1.0, 2.0], [0.0, 0.5])
    t.append([row, (row[0], row[1], (0.0, 0.5, 0.7, 0.1, 0.0))])
    with pytest.raises(ValueError, match="sqrt_at == 0"):
        t.host()
    t = G.StepTable([1.0, 2.0], [0.0, 0.5])                          # ... on an inactive row nothing is read: fine
    t.append([row, None])
    assert t.host().shape == (1, 2, ops.STEP_ROW)


def test_per_request_validation():
    assert G.per_request(4, 3.0, 0.5, 3) is None                     # all scalars: the scalar path
    assert G.per_request([1, 4, 3], 3.0, 0.5, 3) == ([1, 4, 3], [3.0] * 3, [0.5] * 3)
    assert G.per_request(4, np.array([1.5, 3.0]), 0.0, 2) == ([4, 4], [1.5, 3.0], [0.0, 0.0])
    import torch
    assert G.per_request(torch.tensor([2, 3]), 3.0, torch.tensor(0.5), 2) == ([2, 3], [3.0, 3.0], [0.5, 0.5])
    assert G.per_request(None, [1.0, 2.0], 0.0, 2)[0] is None
    with pytest.raises(MdxError, match="steps: 2 values for a batch of 3"):
        G.per_request([1, 2], 3.0, 0.0, 3)
    with pytest.raises(MdxError, match="scale: 4 values for a batch of 3"):
        G.per_request(4, [1.0] * 4, 0.0, 3)
    with pytest.raises(MdxError, match="guidance_rescale: 1 values for a batch of 3"):
        G.per_request(4, 3.0, [0.5], 3)
    for bad in ([1, 0, 3], [1, -2, 3], [1, 2.5, 3], [1, True, 3], [1, 4.0, 3], [1, float("nan"), 3], [1, float("inf"), 3],
                np.array([1.0, 4.0, 3.0]), [1, "4", 3]):
        with pytest.raises(ValueError, match="int >= 1"):
            G.per_request(bad, 3.0, 0.0, 3)
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            G.per_request(4, 3.0, [0.0, bad, 0.0], 3)
    with pytest.raises(ValueError, match="finite"):
        G.per_request(4, [1.0, float("nan"), 2.0], 0.0, 3)
    assert G.per_request(np.array([2, 5, 1]), 3.0, 0.0, 3)[0] == [2, 5, 1]      # integer arrays are ints


def test_pipeline_list_checks_need_no_gpu():
    from minddiffusion_amd.pipeline import DiffusionPipeline as P
    assert P.check_request_lists("x", None, 30, 7.5, 0.7) == 0.7
    assert P.check_request_lists("x", 2, [30, 50], [7.5, 5.0], [0.0, 0.7]) == [0.0, 0.7]
    with pytest.raises(ValueError, match="guidance_rescale"):
        P.check_request_lists("x", None, 30, 7.5, 1.5)
    with pytest.raises(MdxError, match="scale: 2 values for a batch of 3"):
        P.check_request_lists("x", 3, 30, [7.5, 5.0], 0.0)
    with pytest.raises(ValueError, match="int >= 1"):
        P.check_request_lists("x", None, [30, 0], 7.5, 0.0)
    with pytest.raises(ValueError, match="guidance_rescale"):
        P.check_request_lists("x", None, 30, 7.5, [0.0, 1.5])
    for what in ("img2img", "inpaint"):
        with pytest.raises(ValueError, match=f"{what}: `strength` fixes one grid"):
            P.check_request_lists(what, None, [30, 50], 7.5, 0.0, steps_list=False)
        assert P.check_request_lists(what, 2, 30, [7.5, 5.0], [0.0, 0.7], steps_list=False) == [0.0, 0.7]


def test_lists_need_a_single_rank(monkeypatch):
    from minddiffusion_amd import distributed as D
    from minddiffusion_amd.pipeline import DiffusionPipeline as P
    monkeypatch.setattr(D, "world", lambda: (0, 2))
    with pytest.raises(MdxError, match=r"runs on a single rank \(the sharded form is not built\)"):
        P.check_request_lists("DiffusionPipeline", None, 30, [7.5, 5.0], 0.0)
    assert P.check_request_lists("DiffusionPipeline", None, 30, 7.5, 0.5) == 0.5      # scalars still shard
