"""The step tables that tests/golden/step_plans_parent.npz pins (tests/test_step_plans_cpu.py and
tests/golden/make_step_plans_parent_golden.py share this list): per case, which sampler builds the table, for which per-sample
step counts, scales and rescales, on which grid.  Numpy only; the schedule is the StubModel's of test_per_request_cpu.py."""
# kind -> (sampler, eta)
KINDS = {"plms": ("plms", 0.0), "ddim": ("ddim", 0.0), "ddim_eta0.5": ("ddim", 0.5), "dpm": ("dpm", 0.0)}
SCALES = [1.5, 3.0, 7.5, 1.0]
PHIS = [0.0, 0.7, 0.3, 1.0]
# make_ddim_timesteps has no 3-step grid on 1000 training steps (its uniform grid ends on timestep 1000 and is refused): the
# equal-steps list is [3, 3] for DPM-Solver and [4, 4] for PLMS / DDIM
NO_DDIM_GRID = 3


def step_lists(kind):
    return [[2, 5, 5, 1], [1], [3, 3] if kind == "dpm" else [4, 4]]


def cases():
    """name -> dict(kind, steps, scales, rescales, guided, and the grid options: t_enc (DDIM / PLMS: decode()'s t_start on the
    steps-step grid; DPM-Solver: the continuous start of the last t_enc of `of` steps), original_steps / timesteps
    (plms_sampling's grid options), t_start (DPM-Solver's continuous start time))."""
    out = {}

    def add(name, kind, steps, guided=True, **grid):
        n = len(steps)
        out[name] = dict(kind=kind, steps=steps, scales=SCALES[:n], rescales=PHIS[:n], guided=guided, **grid)

    for kind in KINDS:
        for steps in step_lists(kind):
            add(f"{kind}_S" + "_".join(str(s) for s in steps), kind, steps)
        add(f"{kind}_unguided", kind, [2, 5, 5, 1], guided=False)
        for t_enc in range(1, 5):
            if kind == "dpm":
                if t_enc < 4:
                    add(f"dpm_t_enc{t_enc}_of_4", kind, [t_enc, t_enc], t_enc=t_enc, of=4)
            else:
                add(f"{kind}_t_enc{t_enc}_of_4", kind, [4, 4], t_enc=t_enc)
        if kind == "dpm":
            add("dpm_t_start0.6", kind, [3, 3], t_start=0.6)
        else:
            add(f"{kind}_original_steps6", kind, [5, 5], original_steps=True, timesteps=6)
            add(f"{kind}_timesteps4_prefix", kind, [5, 5], timesteps=4)
    return out
