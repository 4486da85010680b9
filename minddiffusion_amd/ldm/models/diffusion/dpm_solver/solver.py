"""The reference's solver surface (ldm/models/diffusion/dpm_solver/dpm_solver.py): ``model_wrapper`` (:170-329) and
``DPM_Solver(model_fn, noise_schedule, predict_x0, thresholding, max_val).sample(...)`` (:332-1123) on the fused path.

The arithmetic is dpm_solver.solver_plan's (host, float64): one record per model evaluation.  run_solver_plan is the one loop
that drives a plan -- DPMSolverSampler's non-default configurations and DPM_Solver.sample both end in it: per record one
GuidedModel call (the UNet on the guidance batch) and ONE ops.sampler_step_lin launch, which turns the UNet output into the
model value (CFG combine, guidance rescale, v -> eps, data prediction, dynamic thresholding) and forms the update; a record
of a stochastic plan (sde_eta > 0: cn != 0) goes through ops.sampler_step_lin_noise instead, which adds cn * N(0, 1) in the
same launch -- drawn inside it from per-sample seeds, or read from a tensor.  The
latents ("x", "y") and the model-value slots ("m0" .. "m2") are allocated once; the plan's roles rotate them by reference.
"""
import numpy as np
import torch

from ..... import ops
from ....._lib import MdxError
from ..guided import GuidedModel, check_guidance_rescale, check_seed_sources, check_seeds
from .dpm_solver import VALUE_X0, solver_plan

SOLVER_DEFAULTS = dict(order=2, skip_type="time_uniform", method="multistep", solver_type="dpm_solver", predict_x0=True,
                       thresholding=False, max_val=1., denoise_to_zero=False, lower_order_final=True, t_end=None, sde_eta=0.,
                       s_noise=1., rho=7.)
PLAN_OPTIONS = ("order", "skip_type", "method", "solver_type", "predict_x0", "lower_order_final", "denoise_to_zero", "t_end", "rho",
                "sde_eta", "s_noise")      # SOLVER_DEFAULTS' keys that are solver_plan's arguments


def check_max_val(thresholding, max_val):
    """`max_val` of dynamic thresholding as a finite float > 0 (1.0 when thresholding is off: it is not read)."""
    if not thresholding:
        return 1.
    v = float(max_val)
    if not (np.isfinite(v) and v > 0.):
        raise ValueError(f"max_val must be a finite number > 0, got {max_val!r}")
    return v


def run_solver_plan(plan, guided, x, scale, pred, guidance_rescale=0., thresholding=False, max_val=1., callback=None,
                    img_callback=None, seeds=None, generator=None, step_noises=None, image_scale=None):
    """Run `plan` (solver_plan's records) from the latent x ([B, C, H, W] fp32, overwritten: the run's "x" buffer) with
    guided = GuidedModel(..., t_steps=[r["t_input"] for r in plan]); returns the result, which is x.  No device work in the
    loop besides the model call and the step launch; callback(i) and img_callback(model value, i) fire once per evaluation.
    The noise of a record with cn != 0 (a stochastic plan): with `seeds` (the [B] device tensor of check_seeds) drawn inside the
    step launch, stream ops.RNG_STEP, draw = the record's index -- no launch and no tensor of its own; else step_noises[index]
    (test injection); else one torch.randn from `generator`.  A record with cn == 0 makes the launch it has always made.
    image_scale (with a three-branch `guided`): every record's launch is ops.sampler_step_lin_dual on guided.out_m.
    A record of uni_pc.unipc_plan (it has "Ap") runs in the same loop: ONE ops.sampler_step_pc launch, which writes the
    corrected latent to the record's "corr_out" buffer and the predicted one, the next model input, to "out"."""
    roles = {name for r in plan for name in (r["model"], r["base"], r["out"], r["store"], r.get("corr_out", "x"))}
    bufs = {name: torch.empty_like(x) for name in sorted(roles - {"x"})}
    bufs["x"] = x
    for i, r in enumerate(plan):
        out_u, out_c = guided(bufs[r["model"]], i)
        x0 = r["value"] == VALUE_X0
        hist = [None if r.get(k) is None else bufs[r[k]] for k in ("h1", "h2", "h3")]
        kw = dict(thresholding=thresholding and x0, max_val=max_val)
        args = (bufs[r["base"]], bufs[r["model"]], out_u, out_c, scale, pred, guidance_rescale,
                ops.VALUE_X0 if x0 else ops.VALUE_EPS, r["alpha_m"], r["sigma_m"])
        if "Ap" in r:       # a record of uni_pc.unipc_plan: the corrector and the next predictor, ONE ops.sampler_step_pc launch
            if image_scale is not None:
                raise MdxError("run_solver_plan: a UniPC record does not take three-branch guidance (image_scale)")
            corr = tuple(r[k] for k in ("Ac", "d0", "d1", "d2", "d3")) if "Ac" in r else None
            ops.sampler_step_pc(*args, *hist, corr, (r["Ap"], r["e0"], r["e1"], r["e2"]), bufs[r["store"]], bufs[r["corr_out"]],
                                bufs[r["out"]], **kw)
        else:
            args += (hist[0], hist[1], r["A"], r["c0"], r["c1"], r["c2"], bufs[r["store"]], bufs[r["out"]])
            if image_scale is not None:
                args = args[:3] + (guided.out_m, out_c, scale, image_scale) + args[5:]
            if r["cn"] == 0.:
                if image_scale is not None:
                    ops.sampler_step_lin_dual(*args, **kw)
                else:
                    ops.sampler_step_lin(*args, **kw)
            else:
                noise = None
                if seeds is None and step_noises is not None:
                    noise = torch.as_tensor(step_noises[r["draw"]]).to(device=x.device, dtype=torch.float32).contiguous()
                elif seeds is None:
                    noise = torch.randn(x.shape, device=x.device, dtype=torch.float32, generator=generator)
                step = ops.sampler_step_lin_noise if image_scale is None else ops.sampler_step_lin_dual
                step(*args, r["cn"], noise=noise, seeds=seeds, stream=ops.RNG_STEP, draw=r["draw"], **kw)
        if callback:
            callback(i)
        if img_callback:
            img_callback(bufs[r["store"]], i)
    return bufs["x"]


class _ModelFn:
    """apply_model(x, t_input, cond) of a callable model(x, t_input[, cond]) (what the reference hands model_wrapper)."""

    def __init__(self, fn):
        self.fn = fn

    def apply_model(self, x, t, cond=None):
        return self.fn(x, t) if cond is None else self.fn(x, t, cond)


class _ContinuousFn:
    """apply_model of a foreign noise-prediction function (x, t_continuous) -> eps: the model-input time GuidedModel passes is
    mapped back to the continuous time (get_model_input_time :256-265 inverted)."""

    def __init__(self, fn, total_N):
        self.fn, self.total_N = fn, total_N

    def apply_model(self, x, t, cond=None):
        return self.fn(x, t / 1000. + 1. / self.total_N)


class WrappedModel:
    """What model_wrapper returns: the model, its conditioning and its guidance scale, kept apart so that DPM_Solver runs them
    on the fused path; called as the reference's model_fn(x, t_continuous) it returns the guided noise prediction, NCHW fp32."""

    def __init__(self, model, noise_schedule, model_type, condition, unconditional_condition, guidance_scale):
        self.model = model if hasattr(model, "apply_model") or hasattr(model, "apply_model_nhwc") else _ModelFn(model)
        self.noise_schedule, self.model_type = noise_schedule, model_type
        self.condition, self.unconditional_condition = condition, unconditional_condition
        self.guidance_scale = float(guidance_scale)
        self.pred = ops.PRED_V if model_type == "v" else ops.PRED_EPS

    def guided(self, x, t_inputs):
        return GuidedModel(self.model, int(x.shape[0]), tuple(x.shape[1:]), self.condition, self.unconditional_condition, None,
                           None, self.guidance_scale, x.device, t_inputs)

    def __call__(self, x, t_continuous):
        ns = self.noise_schedule
        t = float(torch.as_tensor(t_continuous).reshape(-1)[0])
        x = x.to(torch.float32).contiguous()
        out_u, out_c = self.guided(x, [float(ns.model_input_time(t))])(x, 0)
        eps, unused = torch.empty_like(x), torch.empty_like(x)
        ops.sampler_step_lin(x, x, out_u, out_c, self.guidance_scale, self.pred, 0., ops.VALUE_EPS, float(ns.marginal_alpha(t)),
                             float(ns.marginal_std(t)), None, None, 0., 1., 0., 0., eps, unused)
        return eps


def model_wrapper(model, noise_schedule, model_type="noise", model_kwargs=None, guidance_type="uncond", condition=None,
                  unconditional_condition=None, guidance_scale=1., classifier_fn=None, classifier_kwargs=None,
                  image_guidance_scale=None):
    """dpm_solver.py:170-329 for what the fused path carries: model_type "noise" | "v", guidance_type "uncond" |
    "classifier-free".  model: a LatentDiffusion of this package (its NHWC fast path is used), any object with the reference's
    apply_model(x, t_input, cond) -> eps | v NCHW, or a callable model(x, t_input, cond).  image_guidance_scale (three-branch
    guidance) is DPMSolverSampler.sample's: refused here."""
    if image_guidance_scale is not None:
        raise MdxError("model_wrapper: image_guidance_scale is not carried by model_wrapper / DPM_Solver (the ported reference "
                       "surface has no c_concat): use DPMSolverSampler.sample(image_guidance_scale=)")
    if model_type in ("x_start", "score"):
        raise NotImplementedError(f"model_type {model_type!r}: the step launch converts a noise or a v output "
                                  f"(MDX_PRED_EPS | MDX_PRED_V) to the model value, no other")
    if model_type not in ("noise", "v"):
        raise ValueError(f"model_type must be 'noise', 'x_start', 'v' or 'score', got {model_type!r}")
    if guidance_type == "classifier":
        raise NotImplementedError("guidance_type 'classifier' needs the classifier's gradient with respect to x at every "
                                  "evaluation: there is no backward pass on the fused path")
    if guidance_type not in ("uncond", "classifier-free"):
        raise ValueError(f"guidance_type must be 'uncond', 'classifier' or 'classifier-free', got {guidance_type!r}")
    if model_kwargs:
        raise NotImplementedError("model_kwargs: the fused path calls apply_model(x, t, cond) only")
    if guidance_type == "uncond":
        unconditional_condition, guidance_scale = None, 1.
    return WrappedModel(model, noise_schedule, model_type, condition, unconditional_condition, guidance_scale)


class DPM_Solver:
    """dpm_solver.py:332-1123.  model_fn: model_wrapper's result (the fused path end to end) or any callable
    (x, t_continuous) -> noise prediction NCHW, whose output is re-laid for the step launch as GuidedModel does for a foreign
    apply_model.  method 'adaptive' is refused (solver_plan says why)."""

    def __init__(self, model_fn, noise_schedule, predict_x0=False, thresholding=False, max_val=1.):
        self.model = model_fn
        self.noise_schedule = noise_schedule
        self.predict_x0 = bool(predict_x0)
        self.thresholding = bool(thresholding)
        self.max_val = check_max_val(self.thresholding, max_val)

    def sample(self, x, steps=20, t_start=None, t_end=None, order=3, skip_type="time_uniform", method="singlestep",
               lower_order_final=True, denoise_to_zero=False, solver_type="dpm_solver", atol=0.0078, rtol=0.05, callback=None,
               img_callback=None, rho=7., sde_eta=0., s_noise=1., seeds=None, generator=None, step_noises=None,
               image_guidance_scale=None):
        """rho (with skip_type="karras"), sde_eta, s_noise: solver_plan's options, not in the reference.  The noise of a
        stochastic run (sde_eta > 0): per sample from `seeds` (one int per sample), drawn inside the step launches; else from
        `generator` (None: torch's default); step_noises injects it for tests."""
        if image_guidance_scale is not None:
            raise MdxError("DPM_Solver.sample: image_guidance_scale is not carried by model_wrapper / DPM_Solver (the ported "
                           "reference surface has no c_concat): use DPMSolverSampler.sample(image_guidance_scale=)")
        ns = self.noise_schedule
        plan = solver_plan(ns, steps, order=order, skip_type=skip_type, method=method, solver_type=solver_type,
                           predict_x0=self.predict_x0, lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero,
                           t_start=t_start, t_end=t_end, rho=rho, sde_eta=sde_eta, s_noise=s_noise)
        check_seed_sources(seeds, generator, step_noises=step_noises)
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4):
            raise MdxError("DPM_Solver.sample: x must be a CUDA(HIP) tensor [B, C, H, W]")
        seeds = check_seeds(seeds, int(x.shape[0]), x.device)
        x = x.to(torch.float32).contiguous().clone()
        t_inputs = [r["t_input"] for r in plan]
        if isinstance(self.model, WrappedModel):
            guided, scale, pred = self.model.guided(x, t_inputs), self.model.guidance_scale, self.model.pred
        else:
            guided = GuidedModel(_ContinuousFn(self.model, ns.total_N), int(x.shape[0]), tuple(x.shape[1:]), None, None, None,
                                 None, 1., x.device, t_inputs)
            scale, pred = 1., ops.PRED_EPS
        return run_solver_plan(plan, guided, x, scale, pred, check_guidance_rescale(0.), self.thresholding, self.max_val,
                               callback, img_callback, seeds, generator, step_noises)
