"""UniPC on the fused path: ``UniPC(model_fn, noise_schedule, ...).sample(...)`` -- the solver surface of the UniPC paper's
code, on a dpm_solver.model_wrapper(...) result or a foreign callable, as DPM_Solver takes them -- and ``UniPCSampler(model)``
with PLMSSampler's / DPMSolverSampler's ``sample(...)`` keywords.

Execution: uni_pc.unipc_plan's records (host, float64) run by dpm_solver/solver.run_solver_plan -- per model evaluation one
UNet forward (GuidedModel: the guidance batch, hybrid conditioning, the time-embedding table built once) and ONE
``mdx_sampler_step_pc_f32`` launch, which turns the UNet output into the model value (CFG combine, guidance rescale, v -> eps,
data prediction, dynamic thresholding), corrects the latent at the evaluation's time with it and predicts the latent at the
next time from the corrected one.  The model is never evaluated on a corrected latent, so a run of S steps costs S evaluations
(S + 1 with denoise_to_zero).  Not carried, and refused by name: sessions, per-request lists, mask / x0 blending, three-branch
guidance, SDE noise, any method but 'multistep', the 'vary_coeff' variant.
"""
import numpy as np
import torch

from ..... import ops
from ....._lib import MdxError
from ..dpm_solver.dpm_solver import NoiseScheduleVP, check_rho
from ..dpm_solver.solver import WrappedModel, _ContinuousFn, check_max_val, run_solver_plan
from ..guided import (GuidedModel, check_guidance_rescale, check_seed_sources, check_seeds, noised_latent, split_conditioning,
                      start_latent)
from ..schedule import per_request, pred_type
from .uni_pc import unipc_plan

UNIPC_DEFAULTS = dict(order=3, variant="bh2", skip_type="time_uniform", method="multistep", predict_x0=True, thresholding=False,
                      max_val=1., lower_order_final=True, corrector=True, t_end=None, denoise_to_zero=False, rho=7.)
PLAN_OPTIONS = ("order", "variant", "skip_type", "method", "predict_x0", "lower_order_final", "corrector", "t_end",
                "denoise_to_zero", "rho")      # UNIPC_DEFAULTS' keys that are unipc_plan's arguments


def refuse_unsupported(what, **given):
    """The options of the other samplers that UniPC does not carry, by name."""
    why = dict(mask="mask / x0 blending is PLMSSampler's / DDIMSampler's", x0="mask / x0 blending is PLMSSampler's / DDIMSampler's",
               image_guidance_scale="three-branch guidance (image_guidance_scale, edit) is not carried by the UniPC step launch",
               sde_eta="sde_eta: UniPC is an ODE solver (the SDE update is DPMSolverSampler's)",
               s_noise="s_noise goes with sde_eta (DPMSolverSampler's)", solver_type="solver_type is DPM-Solver's option")
    for name, value in given.items():
        if value is not None and not (name in ("sde_eta",) and float(value) == 0.):
            raise MdxError(f"{what}: {why[name]}")


class UniPC:
    """model_fn: model_wrapper's result (model types "noise" and "v", classifier-free guidance; the fused path end to end) or
    any callable (x, t_continuous) -> noise prediction NCHW."""

    def __init__(self, model_fn, noise_schedule, predict_x0=True, thresholding=False, max_val=1., variant="bh2"):
        self.model = model_fn
        self.noise_schedule = noise_schedule
        self.predict_x0 = bool(predict_x0)
        self.thresholding = bool(thresholding)
        self.max_val = check_max_val(self.thresholding, max_val)
        self.variant = variant

    def sample(self, x, steps=20, t_start=None, t_end=None, order=3, skip_type="time_uniform", method="multistep",
               lower_order_final=True, denoise_to_zero=False, corrector=True, rho=7., callback=None, img_callback=None,
               sde_eta=None, image_guidance_scale=None):
        refuse_unsupported("UniPC.sample", sde_eta=sde_eta, image_guidance_scale=image_guidance_scale)
        ns = self.noise_schedule
        plan = unipc_plan(ns, steps, order=order, variant=self.variant, predict_x0=self.predict_x0,
                          lower_order_final=lower_order_final, corrector=corrector, skip_type=skip_type, rho=rho,
                          t_start=t_start, t_end=t_end, denoise_to_zero=denoise_to_zero, method=method)
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4):
            raise MdxError("UniPC.sample: x must be a CUDA(HIP) tensor [B, C, H, W]")
        x = x.to(torch.float32).contiguous().clone()
        t_inputs = [r["t_input"] for r in plan]
        if isinstance(self.model, WrappedModel):
            guided, scale, pred = self.model.guided(x, t_inputs), self.model.guidance_scale, self.model.pred
        else:
            guided = GuidedModel(_ContinuousFn(self.model, ns.total_N), int(x.shape[0]), tuple(x.shape[1:]), None, None, None,
                                 None, 1., x.device, t_inputs)
            scale, pred = 1., ops.PRED_EPS
        return run_solver_plan(plan, guided, x, scale, pred, 0., self.thresholding, self.max_val, callback, img_callback)


class UniPCSampler:
    def __init__(self, model, **kwargs):
        """kwargs: generator, and the defaults of sample()'s solver options (UNIPC_DEFAULTS' keys)."""
        self.model = model
        self.alphas_cumprod = np.asarray(model.alphas_cumprod, dtype=np.float64)
        self.generator = kwargs.get("generator", None)
        unknown = sorted(set(kwargs) - set(UNIPC_DEFAULTS) - {"generator"})
        if unknown:
            raise ValueError(f"UniPCSampler: unknown option(s) {', '.join(unknown)}; known: {', '.join(sorted(UNIPC_DEFAULTS))}")
        self.solver = dict(UNIPC_DEFAULTS, **{k: v for k, v in kwargs.items() if k in UNIPC_DEFAULTS and v is not None})
        opts = self._options({})        # a mistake shows where it is made: the plan of a short run, built and dropped
        unipc_plan(self._schedule(), 3 * opts["order"], **{k: opts[k] for k in PLAN_OPTIONS if k != "denoise_to_zero"})

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    def _schedule(self):
        return NoiseScheduleVP("discrete", alphas_cumprod=self.alphas_cumprod)

    def _options(self, given):
        opts = {k: self.solver[k] if given.get(k) is None else given[k] for k in UNIPC_DEFAULTS}
        opts["max_val"] = check_max_val(opts["thresholding"], opts["max_val"])
        opts["rho"] = check_rho(opts["rho"]) if opts["skip_type"] == "karras" else UNIPC_DEFAULTS["rho"]
        return opts

    # ---- img2img: a run that starts at a continuous time t_start below T, as DPMSolverSampler has it
    def _check_t_start(self, t_start):
        t, n = float(t_start), self.alphas_cumprod.shape[0]
        if not 1.0 / n < t <= 1.0:
            raise ValueError(f"t_start must be a continuous time in (1/{n}, 1], got {t_start!r}")
        return t

    def q_coefficients(self, t_start):
        """(marginal_alpha, marginal_std) at the continuous time t_start."""
        ns, t = self._schedule(), self._check_t_start(t_start)
        return float(ns.marginal_alpha(t)), float(ns.marginal_std(t))

    def stochastic_encode(self, x0, t_start, noise=None, seeds=None):
        """x0 noised to the continuous time t_start, one ops.q_sample launch into a fresh tensor (DPMSolverSampler's)."""
        a, b = self.q_coefficients(t_start)
        return noised_latent(x0, a, b, noise, self.generator, seeds)

    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, guidance_rescale=0., t_start=None, seeds=None, order=None, variant=None,
               skip_type=None, rho=None, method=None, predict_x0=None, thresholding=None, max_val=None, lower_order_final=None,
               corrector=None, t_end=None, denoise_to_zero=None, image_guidance_scale=None, sde_eta=None, s_noise=None,
               solver_type=None, **kwargs):
        """S model evaluations (S + 1 with denoise_to_zero), each followed by ONE ops.sampler_step_pc launch; callback(i) and
        img_callback(model value, i) fire once per evaluation.  order (1-3), variant ("bh1" | "bh2"), skip_type (dpm_solver's
        four grids, rho with "karras"), predict_x0, thresholding / max_val, lower_order_final, corrector, t_end,
        denoise_to_zero: unipc_plan's options; None: the sampler's default (UNIPC_DEFAULTS unless the constructor was given
        another).  seeds, x_T, t_start (from stochastic_encode(., t_start)), hybrid conditioning, v-prediction and
        guidance_rescale work as in DPMSolverSampler; `eta` is ignored as there.  Refused: per-request S / scale / rescale
        lists, mask / x0, image_guidance_scale, sde_eta, any method but 'multistep'."""
        what = "UniPCSampler.sample"
        refuse_unsupported(what, mask=mask, x0=x0, image_guidance_scale=image_guidance_scale, sde_eta=sde_eta, s_noise=s_noise,
                           solver_type=solver_type)
        if per_request(S, unconditional_guidance_scale, guidance_rescale, batch_size) is not None:
            raise MdxError(f"{what}: per-request S / guidance scale / guidance_rescale lists run on the step table, whose rows "
                           f"hold the DPM-Solver++ 2M update only: UniPC takes scalars")
        opts = self._options(dict(order=order, variant=variant, skip_type=skip_type, rho=rho, method=method,
                                  predict_x0=predict_x0, thresholding=thresholding, max_val=max_val,
                                  lower_order_final=lower_order_final, corrector=corrector, t_end=t_end,
                                  denoise_to_zero=denoise_to_zero))
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        check_seed_sources(seeds, self.generator)
        if t_start is not None:
            t_start = self._check_t_start(t_start)
        plan = unipc_plan(self._schedule(), S, t_start=t_start, **{k: opts[k] for k in PLAN_OPTIONS})
        if conditioning is None:
            raise MdxError("UniPCSampler: conditioning is required (classifier-free guidance on a text-conditional UNet)")
        cond, uc, c_cat, uc_cat, dev = split_conditioning(self.model, conditioning, unconditional_conditioning, x_T)
        size = (batch_size,) + tuple(shape)
        seeds = check_seeds(seeds, batch_size, dev)
        img = start_latent(x_T, seeds, size, dev, self.generator)
        scale = float(unconditional_guidance_scale)
        guided = GuidedModel(self.model, batch_size, tuple(shape), cond, uc, c_cat, uc_cat, scale, dev,
                             [r["t_input"] for r in plan])
        return run_solver_plan(plan, guided, img, scale, pred_type(self.model), guidance_rescale, opts["thresholding"],
                               opts["max_val"], callback, img_callback), None
