"""One description of a run (ldm/models/diffusion/schedule.py), no GPU and no library needed.

1. The tables schedule.ddim_steps / dpm_steps / step_table build are, bit for bit, the ones the samplers' own table builders
   made at the parent commit (tests/golden/step_plans_parent.npz, written by tests/golden/make_step_plans_parent_golden.py from
   the cases of tests/_step_plans.py): the float32 rows, the model-input timesteps and the loop length, compared as uint32
   with tolerance zero.
2. A scalar run hands ops.sampler_update the very bits of its row: ScalarSteps.launch(k, ...) against row k of the step_table
   built from the same plan."""
import os

import numpy as np
import pytest

import _step_plans as P
from minddiffusion_amd import ops
from minddiffusion_amd.ldm.models.diffusion import schedule as SCH
from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP
from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
from test_per_request_cpu import StubModel

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_plans_parent.npz"))
CASES = P.cases()
SAMPLERS = {"plms": PLMSSampler, "ddim": DDIMSampler}


def plans_of(model, case):
    """The per-sample plans of a case, through the public functions only."""
    sampler, eta = P.KINDS[case["kind"]]
    if sampler == "dpm":
        ac = DPMSolverSampler(model).alphas_cumprod
        ns = NoiseScheduleVP("discrete", alphas_cumprod=ac)
        t_start = case.get("t_start")
        if case.get("t_enc") is not None:
            t_start = SCH.dpm_partial_start(ac.shape[0], case["of"], case["t_enc"])
        return [SCH.dpm_steps(ns, s, t_start) for s in case["steps"]]
    s = SAMPLERS[sampler](model)
    by_steps = {}
    for n in sorted(set(case["steps"])):
        s.make_schedule(n, ddim_eta=eta, verbose=False)
        grid = s.time_grid(case.get("original_steps", False), case.get("timesteps"), case.get("t_enc"))
        by_steps[n] = SCH.ddim_steps(s, grid, sampler == "plms")
    return [by_steps[n] for n in case["steps"]]


def table_of(model, case):
    return SCH.step_table(plans_of(model, case), case["scales"], case["rescales"], case["guided"],
                          second_call_row=P.KINDS[case["kind"]][0] == "plms")


def test_the_golden_file_and_the_case_list_name_the_same_cases():
    assert sorted(GOLD.files) == sorted(f"{name}__{part}" for name in CASES for part in ("table", "t_rows", "total"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_are_bit_identical_to_the_parent_commit(name):
    table, t_rows, total = table_of(StubModel(), CASES[name])
    host = table.host()
    want, want_t = GOLD[name + "__table"], GOLD[name + "__t_rows"]
    assert host.dtype == want.dtype == np.float32 and t_rows.dtype == want_t.dtype == np.float32
    assert host.shape == want.shape and t_rows.shape == want_t.shape
    assert np.array_equal(host.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(t_rows.view(np.uint32), want_t.view(np.uint32))
    assert total == int(GOLD[name + "__total"])
    if not CASES[name]["guided"]:
        assert not host[..., ops.STEP_RESCALE].any()                   # no unconditional half: no row rescales


@pytest.mark.parametrize("cls", [PLMSSampler, DDIMSampler])
def test_a_step_count_without_a_ddim_grid_is_still_refused(cls):
    """Why the equal-steps list of PLMS / DDIM is [4, 4] and not [3, 3]."""
    with pytest.raises(IndexError, match="choose S dividing"):
        cls(StubModel()).make_schedule(P.NO_DDIM_GRID, verbose=False)


# ------------------------------------------------------------------------------------------ scalar launches hand over the row
def one_sample_plan(kind, steps):
    case = dict(kind=kind, steps=[steps])
    return plans_of(StubModel(), case)[0]


SCALAR_CASES = {"plms_S1": ("plms", 1), "plms_S5": ("plms", 5), "ddim_eta0.5_S5": ("ddim_eta0.5", 5), "dpm_S1": ("dpm", 1),
                "dpm_S5": ("dpm", 5)}


@pytest.mark.parametrize("name", sorted(SCALAR_CASES))
def test_a_scalar_launch_hands_over_the_bits_of_its_row(monkeypatch, name):
    kind, n = SCALAR_CASES[name]
    scale, phi = 3.0, 0.7
    plan = one_sample_plan(kind, n)
    table, _, _ = SCH.step_table([plan], [scale], [phi], True, second_call_row=kind == "plms")
    host = table.host()
    active = host[..., ops.STEP_ACTIVE] != 0
    table_sigma = [bool(v) for v in (active & (host[..., ops.STEP_SIGMA] != 0)).any(1)]     # StepTable.upload()'s rule
    seen = []
    monkeypatch.setattr(ops, "sampler_update", lambda *a: seen.append(a))
    monkeypatch.setattr(ops, "sampler_step_table", lambda *a, **k: pytest.fail("a scalar run reached the table entry"))
    steps = SCH.ScalarSteps(plan, scale, phi)
    assert len(plan) == host.shape[0] == n + (kind == "plms") and steps.any_sigma == table_sigma
    bits = lambda values: np.asarray([float(v) for v in values], np.float32).view(np.uint32)
    tags = ["x", "out_u", "out_c", "olds", "noise", "e_t_out", "x_prev", "pred_x0", "x_model"]
    for k in range(len(plan)):
        steps.launch(k, "x", "out_u", "out_c", ops.PRED_V, "olds", "noise", "e_t_out", "x_prev", "pred_x0", "x_model")
        x, out_u, out_c, got_scale, pred, olds, coef, update, got_phi, x_model, am, bm = seen[k]
        assert [x, out_u, out_c, olds, *update[5:], x_model] == tags and pred == ops.PRED_V and len(update) == 9
        row = host[k, 0].view(np.uint32)
        assert host[k, 0, ops.STEP_ACTIVE] == 1.0
        assert bits([got_scale])[0] == row[ops.STEP_CFG_SCALE] and bits([got_phi])[0] == row[ops.STEP_RESCALE]
        assert np.array_equal(bits([am, bm]), row[ops.STEP_SQRT_AT_MODEL:ops.STEP_SQRT_ONE_MINUS_AT_MODEL + 1])
        assert np.array_equal(bits(coef), row[ops.STEP_C0:ops.STEP_C0 + 4])
        assert np.array_equal(bits(update[:5]), row[ops.STEP_SQRT_AT:ops.STEP_SIGMA + 1])
    assert len(seen) == len(plan)
