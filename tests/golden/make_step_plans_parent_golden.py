"""Writes tests/golden/step_plans_parent.npz: for every case of tests/_step_plans.py the StepTable.host() array, the
model-input timesteps t_rows and the loop length total, which tests/test_step_plans_cpu.py compares against bit for bit.

The committed file was recorded on the CPU (no library needed) at commit 010c9c4, the one before the samplers built their
launches from one step plan.  This script calls the PRIVATE methods that commit had -- _SamplerBase._step_table / _time_grid,
DPMSolverSampler._step_table, session._dpm_start -- which later trees no longer have: it only runs on a checkout of that commit,
with tests/_step_plans.py and this file from the current tree:

    python tests/golden/make_step_plans_parent_golden.py [output directory]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import _step_plans as P  # noqa: E402
from test_per_request_cpu import StubModel  # noqa: E402


def parent_table(model, case):
    from minddiffusion_amd.ldm.models.diffusion import session
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    sampler, eta = P.KINDS[case["kind"]]
    lists = (case["scales"], case["rescales"], case["guided"])
    if sampler == "dpm":
        d = DPMSolverSampler(model)
        ns = NoiseScheduleVP("discrete", alphas_cumprod=d.alphas_cumprod)
        t_start = case.get("t_start")
        if case.get("t_enc") is not None:
            t_start = session._dpm_start(d, case["of"], case["t_enc"])
        return DPMSolverSampler._step_table(ns, case["steps"], *lists, t_start=t_start)
    s = {"plms": PLMSSampler, "ddim": DDIMSampler}[sampler](model)
    grids = {}
    for n in sorted(set(case["steps"])):
        s.make_schedule(n, ddim_eta=eta, verbose=False)
        grids[n] = s._time_grid(case.get("original_steps", False), case.get("timesteps"), case.get("t_enc"))
    return s._step_table([grids[n] for n in case["steps"]], *lists)


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else HERE
    model = StubModel()
    out = {}
    for name, case in P.cases().items():
        table, t_rows, total = parent_table(model, case)
        out[name + "__table"] = table.host()
        out[name + "__t_rows"] = t_rows
        out[name + "__total"] = np.int64(total)
    os.makedirs(dst, exist_ok=True)
    np.savez_compressed(os.path.join(dst, "step_plans_parent.npz"), **out)
    print(f"wrote step_plans_parent.npz ({len(out) // 3} cases)")


if __name__ == "__main__":
    main()
