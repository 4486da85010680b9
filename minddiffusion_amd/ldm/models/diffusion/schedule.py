"""Which fused step launches a run makes, with which scalars -- host only, numpy until StepTable.upload().
One sample's run is a list of Step in launch order: ddim_steps() (PLMS / DDIM; the PLMS order is written there and nowhere else)
or dpm_steps().  A sampler's loop launches from one of two objects with one surface (any_sigma[k], launch(k, ...)): ScalarSteps
hands a plan's scalars to ops.sampler_update as kernel arguments; a StepTable -- step_table() merges the plans of a batch into
one -- to ops.sampler_step_table as rows.  Both hold the float32 of the same Step, so a row is the scalar call's arguments to the
bit.  Also here: per-request parameters (as_sequence, per_request), partial runs (check_strength, dpm_partial_start), pred_type().
"""
import collections

import numpy as np
import torch

from .... import ops
from ...._lib import MdxError


def pred_type(model):
    """ops.PRED_V for a `parameterization: "v"` model, else ops.PRED_EPS."""
    return ops.PRED_V if getattr(model, "parameterization", "eps") == "v" else ops.PRED_EPS


# ---- the scalars of one fused step launch
PLMS_FIRST, PLMS_SECOND = (1., 0., 0., 0.), (.5, .5, 0., 0.)        # pseudo improved Euler (plms.py:231-235)
PLMS_AB = ((1., 0., 0., 0.),                                         # no history: DDIM
           (3. / 2, -1. / 2, 0., 0.),                                # Adams-Bashforth 2, plms.py:236-238
           (23. / 12, -16. / 12, 5. / 12, 0.),                       # AB-3, plms.py:239-241
           (55. / 24, -59. / 24, 37. / 24, -9. / 24))                # AB-4, plms.py:242-244


def ddim_step_scalars(alphas, alphas_prev, sqrt_one_minus_alphas, sigmas, index):
    """(sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma) of get_x_prev_and_pred_x0 (plms.py:210-228) at grid
    `index`, float32."""
    a_t, a_prev = np.float32(alphas[index]), np.float32(alphas_prev[index])
    sigma_t = np.float32(sigmas[index])
    return (np.sqrt(a_t), np.float32(sqrt_one_minus_alphas[index]), np.sqrt(a_prev),
            np.sqrt(np.float32(1.) - a_prev - sigma_t ** 2), sigma_t)


def dpm_step_scalars(p):
    """The same five for update p of multistep_2m_plan, x_next = A x + c0 x0 + c1 x0_prev written as the step kernel's
    sqrt_a_prev * pred_x0 + dir_coef * e' + sigma * noise (noise = x0_prev), float32."""
    f = np.float32
    return f(p["alpha"]), f(p["sigma"]), f(p["A"] * p["alpha"] + p["c0"]), f(p["A"] * p["sigma"]), f(p["c1"])


def dpm_model_point(p):
    """(alpha, sigma) where update p evaluates the model: the v -> eps conversion's coefficients, float32."""
    return np.float32(p["alpha"]), np.float32(p["sigma"])


# ---- one sample's run.  t_input: the model-input timestep of the evaluation the launch consumes; model_point: (sqrt_at,
# sqrt_one_minus_at) there (a v output is converted to eps with them); coef: the four multistep coefficients; update: the five above
Step = collections.namedtuple("Step", "t_input model_point coef update")


def ddim_steps(sampler, grid, multistep):
    """The launches of one sample on grid = sampler.time_grid(...), of n steps, in order.  DDIM: n, each on its own model
    output alone.  PLMS: n + 1 -- the two of the pseudo improved Euler step (both take the first step's update scalars; the
    second evaluates the model at the sample's own min(1, n - 1)), then Adams-Bashforth 2, 3, 4, 4, ..."""
    time_range, alphas, alphas_prev, sqrt_one_minus_alphas, sigmas = grid
    n = int(time_range.shape[0])

    def step(i, coef, i_model=None):
        t = time_range[i if i_model is None else i_model]
        return Step(t, (sampler.sqrt_alphas_cumprod[int(t)], sampler.sqrt_one_minus_alphas_cumprod[int(t)]), coef,
                    ddim_step_scalars(alphas, alphas_prev, sqrt_one_minus_alphas, sigmas, n - i - 1))
    if not multistep:
        return [step(i, PLMS_AB[0]) for i in range(n)]
    return ([step(0, PLMS_FIRST), step(0, PLMS_SECOND, min(1, n - 1))]
            + [step(i, PLMS_AB[min(i, 3)]) for i in range(1, n)])


def dpm_steps(ns, steps, t_start=None):
    """The `steps` launches of one sample's DPM-Solver++(2M) run as the reference wires it (sampler.py:80-92): second order
    from two steps on, first-order first and (below 15 steps) last update.  t_start: a continuous start time below T."""
    from .dpm_solver.dpm_solver import multistep_2m_plan    # (the package's __init__ imports the sampler, which imports this file)
    plan = multistep_2m_plan(ns, steps, order=2 if steps >= 2 else 1, lower_order_final=True, t_start=t_start)
    return [Step(p["t_input"], dpm_model_point(p), PLMS_AB[0], dpm_step_scalars(p)) for p in plan]


class ScalarSteps:
    """A run of one plan for the whole batch, its scalars plain kernel arguments: the surface of an uploaded StepTable
    (any_sigma, launch) over ops.sampler_update, which picks the entry.  No device work of its own.  image_scale: the middle
    scale of three-branch guidance; launch() then takes the middle output out_m."""

    def __init__(self, plan, scale, guidance_rescale, image_scale=None):
        self.plan, self.scale, self.guidance_rescale, self.image_scale = plan, scale, guidance_rescale, image_scale
        self.any_sigma = [float(s.update[4]) != 0.0 for s in plan]      # the float32, as a table row decides it

    def launch(self, k, x, out_u, out_c, pred_type, olds, noise, e_t_out, x_prev, pred_x0, x_model=None, out_m=None):
        """Call k of the run: one ops.sampler_update launch with plan[k]'s scalars."""
        s = self.plan[k]
        if out_m is not None and self.image_scale is None:
            raise MdxError("ScalarSteps: a middle output out_m without an image_scale")
        mid = {} if out_m is None else {"out_m": out_m, "mid_scale": self.image_scale}      # (None: today's call, as it was)
        ops.sampler_update(x, out_u, out_c, self.scale, pred_type, olds, s.coef, s.update + (noise, e_t_out, x_prev, pred_x0),
                           self.guidance_rescale, x_model, *s.model_point, **mid)


# ---- per-request parameters: `scale`, `guidance_rescale` and `steps` as one value per sample of the batch
def as_sequence(value):
    """None for a scalar, else the list of a sequence / 1-d array / 1-d tensor."""
    if isinstance(value, torch.Tensor):
        return None if value.dim() == 0 else value.detach().cpu().tolist() if value.dim() == 1 else value
    if isinstance(value, np.ndarray):
        return None if value.ndim == 0 else value.tolist() if value.ndim == 1 else value
    return list(value) if isinstance(value, (list, tuple)) else None


def per_request(steps, scale, guidance_rescale, batch):
    """None when all three are scalars (the scalar path); else (steps, scales, rescales) as lists of `batch` values -- a
    scalar among them repeated -- checked: lengths equal the batch, every steps[b] an int >= 1, every rescale in [0, 1],
    every scale finite.  `steps` None: the step count is not per request here (a run on a schedule already made)."""
    seqs = {"steps": as_sequence(steps), "scale": as_sequence(scale), "guidance_rescale": as_sequence(guidance_rescale)}
    if all(v is None for v in seqs.values()):
        return None
    for name, v in seqs.items():
        if v is not None and (not isinstance(v, list) or len(v) != batch):
            n = len(v) if isinstance(v, list) else tuple(v.shape)
            raise MdxError(f"{name}: {n} values for a batch of {batch}")
    out_steps = None
    if steps is not None:
        out_steps = seqs["steps"] if seqs["steps"] is not None else [steps] * batch
        for s in out_steps:      # an int: no bool, no float (4.0, NaN and inf included)
            if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or int(s) < 1:
                raise ValueError(f"steps: every entry must be an int >= 1, got {s!r}")
        out_steps = [int(s) for s in out_steps]
    scales = [float(s) for s in (seqs["scale"] if seqs["scale"] is not None else [scale] * batch)]
    if not all(np.isfinite(scales)):
        raise ValueError(f"scale: every entry must be finite, got {scales!r}")
    phis = seqs["guidance_rescale"] if seqs["guidance_rescale"] is not None else [guidance_rescale] * batch
    for phi in phis:
        if not 0. <= float(phi) <= 1.:
            raise ValueError(f"guidance_rescale must be in [0, 1], got {phi!r}")
    return out_steps, scales, [float(phi) for phi in phis]


class StepTable:
    """Every per-sample scalar of every fused step launch of one run, as ops.sampler_step_table reads it: a sampler appends, per
    model evaluation and in loop order, the rows it would otherwise have passed as scalars; upload() then makes ONE
    [n_calls, B, ops.STEP_ROW] device tensor, and launch k reads slice k of it.  Pure numpy until upload().

    scales / rescales: the guidance scale and guidance rescale of every sample.  guided: whether the run has an unconditional
    half to combine (without one no row rescales, as in ops.sampler_update)."""

    def __init__(self, scales, rescales, guided=True):
        self.scales = np.asarray(scales, np.float32)
        self.rescales = np.asarray(rescales, np.float32) if guided else np.zeros(len(scales), np.float32)
        self.batch = int(self.scales.shape[0])
        if self.rescales.shape != (self.batch,):
            raise MdxError(f"StepTable: {self.rescales.shape[0]} guidance rescales for a batch of {self.batch}")
        self.calls = []
        self.uploads = 0
        self.device_table = None

    def append(self, rows):
        """rows: one entry per sample -- None for a sample whose schedule has ended (an inactive row), else
        (model_point, coef4, update5): (sqrt_at_model, sqrt_one_minus_at_model), the multistep coefficients, and
        (sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma).  Returns the call's index."""
        if self.device_table is not None:
            raise MdxError("StepTable: append() after upload()")
        if len(rows) != self.batch:
            raise MdxError(f"StepTable: {len(rows)} rows for a batch of {self.batch}")
        t = np.zeros((self.batch, ops.STEP_ROW), np.float32)
        for b, row in enumerate(rows):
            if row is None:
                continue
            model_point, coef, update = row
            t[b, ops.STEP_ACTIVE] = 1.
            t[b, ops.STEP_CFG_SCALE] = self.scales[b]
            t[b, ops.STEP_RESCALE] = self.rescales[b]
            t[b, ops.STEP_SQRT_AT_MODEL:ops.STEP_SQRT_ONE_MINUS_AT_MODEL + 1] = [float(v) for v in model_point]
            t[b, ops.STEP_C0:ops.STEP_C0 + 4] = [float(v) for v in coef]
            t[b, ops.STEP_SQRT_AT:ops.STEP_SIGMA + 1] = [float(v) for v in update]
        self.calls.append(t)
        return len(self.calls) - 1

    def host(self):
        """The validated [n_calls, B, STEP_ROW] float32 array."""
        t = np.stack(self.calls) if self.calls else np.zeros((0, self.batch, ops.STEP_ROW), np.float32)
        if not np.isfinite(t).all():
            k, b, j = (int(v[0]) for v in np.nonzero(~np.isfinite(t)))
            raise ValueError(f"StepTable: call {k}, sample {b}: entry {j} is not finite")
        on = t[..., ops.STEP_ACTIVE] != 0
        phi = t[..., ops.STEP_RESCALE]
        if ((phi < 0) | (phi > 1))[on].any():
            raise ValueError("StepTable: guidance_rescale must be in [0, 1]")
        if (t[..., ops.STEP_SQRT_AT][on] == 0).any():
            raise ValueError("StepTable: sqrt_at == 0 on an active row (pred_x0 divides by it)")
        return t

    def upload(self, device):
        """The one host-to-device copy of the run; afterwards self.device_table[k] is the table of call k."""
        t = self.host()
        self.active = t[..., ops.STEP_ACTIVE] != 0
        self.any_rescale = [bool(v) for v in (self.active & (t[..., ops.STEP_RESCALE] != 0)).any(1)]
        self.any_sigma = [bool(v) for v in (self.active & (t[..., ops.STEP_SIGMA] != 0)).any(1)]
        self.device_table = torch.as_tensor(t).to(device)
        self.uploads += 1
        return self.device_table

    def launch(self, k, x, out_u, out_c, pred_type, olds, noise, e_t_out, x_prev, pred_x0, x_model=None):
        """Call k of the run: one ops.sampler_step_table launch on slice k."""
        ops.sampler_step_table(x, x_model, out_u, out_c, pred_type, olds, noise, e_t_out, x_prev, pred_x0,
                               self.device_table[k], self.any_rescale[k] and out_u is not None)


def step_table(plans, scales, rescales, guided, second_call_row=False):
    """(StepTable, model-input timesteps t_rows, loop iterations) of a batch whose sample b runs plans[b] (lengths may differ):
    call k holds plans[b][k] as sample b's row.  A sample whose plan has ended has an inactive row and keeps its last timestep.
    t_rows [iterations, B] is indexed by LOOP ITERATION, one model evaluation each.  second_call_row (PLMS): iteration 0
    consumes calls 0 and 1, iteration i >= 1 call i + 1, and the timesteps of call 1's evaluation are appended as the LAST row."""
    n_calls = max(len(p) for p in plans)
    table = StepTable(scales, rescales, guided)
    for k in range(n_calls):
        table.append([(p[k].model_point, p[k].coef, p[k].update) if k < len(p) else None for p in plans])
    total = n_calls - int(second_call_row)
    calls = [i + int(second_call_row and i > 0) for i in range(total)] + [1] * int(second_call_row)
    t_rows = [[p[min(k, len(p) - 1)].t_input for p in plans] for k in calls]
    return table, np.array(t_rows, dtype=np.float32), total


# ---- partial runs (img2img): the last t_enc of `steps` steps
def check_strength(what, strength, steps):
    """t_enc = int(strength * steps), the steps of the `steps`-step schedule that remain to run."""
    if not 0.0 < float(strength) <= 1.0:
        raise ValueError(f"{what}: strength must be in (0, 1], got {strength!r}")
    t_enc = int(float(strength) * steps)
    if t_enc == 0:
        raise ValueError(f"{what}: strength {strength!r} leaves no step of {steps} to run")
    return t_enc


def dpm_partial_start(n_ddpm, steps, t_enc):
    """The continuous time the last t_enc of `steps` DPM-Solver steps begin at, on a schedule of n_ddpm training steps: the
    point t_enc / steps of the way from the grid's end 1 / n_ddpm to T = 1."""
    t_0 = 1.0 / n_ddpm
    return t_0 + (1.0 - t_0) * t_enc / steps
