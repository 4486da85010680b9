"""DPMSolverSampler -- MI355X-native mirror of the reference's ldm/models/diffusion/dpm_solver/sampler.py:20-92
(SURVEY 8(f) item 3).  Same constructor and ``sample(...)`` keywords; as wired by the reference:
``NoiseScheduleVP('discrete', alphas_cumprod)``, classifier-free guidance on a noise-prediction model,
``DPM_Solver(predict_x0=True, thresholding=False).sample(steps=S, skip_type='time_uniform', method='multistep',
order=2, lower_order_final=True)``: S UNet evaluations at FRACTIONAL timesteps (t - 1/1000) * 1000.

Execution: per step one UNet forward (replayed hipGraph, CFG batch [uncond; cond] built once) and ONE launch of the
fused ``mdx_sampler_step_f32`` kernel.  With e = CFG-combined eps, x0 = (x - sigma_s e) / alpha_s the 2M update
    x_next = A x + c0 x0 + c1 x0_prev,   x = alpha_s x0 + sigma_s e
is exactly that kernel's  sqrt_a_prev * pred_x0 + dir_coef * e' + sigma * noise  with
    sqrt_at = alpha_s, sqrt_one_minus_at = sigma_s, sqrt_a_prev = A alpha_s + c0, dir_coef = A sigma_s,
    sigma = c1, noise = x0_prev  -- so no extra elementwise passes and no extra kernel.
A `parameterization: "v"` model goes through ``mdx_sampler_step_pred_f32``, which first converts the CFG-combined v to
e = alpha_s v + sigma_s x (the reference's model_wrapper for model_type "v", dpm_solver.py:281-284) in the same launch.
`guidance_rescale` != 0 with guidance on goes through ``mdx_sampler_step_rescale_f32``: the CFG-combined output (eps or v)
is rescaled per sample to the conditional output's std in the same launch (not in the reference).
Hybrid (inpainting) conditioning -- {"c_concat": ..., "c_crossattn": ...}, the dict forms PLMSSampler takes, an unconditional
c_concat of its own included -- is not in the reference's DPM-Solver wiring: the c_concat channels are written into the UNet's
input batch once, only the latent channels are refreshed per step.  `mask` / `x0` blending stays with PLMS / DDIM.
Differences from the reference, both on the fp32 side of its fp16 arithmetic: the time grid and the schedule scalars
are float64 on the host (the reference casts the grid to fp16, dpm_solver.py:415), and x stays fp32 (sampler.py:88
casts the start noise to fp16).
The rest of the reference's solver -- orders 1-3, singlestep / singlestep_fixed, the logSNR and time_quadratic grids, the
'taylor' solver type, the noise-prediction form, dynamic thresholding, denoise_to_zero, t_end -- is reached through sample()'s
solver options (or the constructor's defaults for them): any option off its default runs dpm_solver.solver_plan's records through
solver.run_solver_plan, one ``mdx_sampler_step_lin_f32`` launch per model evaluation.  The wired configuration below stays on
the launches it has always made.
Not in the reference: skip_type="karras" (the Karras sigma grid, exponent `rho`: "DPM++ 2M Karras") and sde_eta > 0 (the SDE
form of the multistep update with fresh noise each step, scaled by `s_noise`: "DPM++ 2M SDE", diffusers' "sde-dpmsolver++") --
solver options like the others; a stochastic record's launch is ``mdx_sampler_step_lin_noise_f32``, which draws its noise
itself from the per-sample seeds.  `eta`, which the pipeline hands every sampler, stays ignored here as in the reference.
One loop: schedule.dpm_steps gives every sample's launches, and the loop launches from a schedule.ScalarSteps (scalar S, scale and
rescale: kernel arguments) or from a StepTable merged from the samples' plans and uploaded once (any of them per sample).
"""
import numpy as np
import torch

from ....._lib import MdxError
from ..guided import (GuidedModel, check_guidance_rescale, check_image_guidance, check_seed_sources, check_seeds, noised_latent,
                      split_conditioning, start_latent)
from ..schedule import ScalarSteps, dpm_steps, per_request, pred_type, step_table
from .dpm_solver import NoiseScheduleVP, check_rho, check_sde, solver_plan
from .solver import PLAN_OPTIONS, SOLVER_DEFAULTS, check_max_val, run_solver_plan


def solver_options(defaults, given):
    """The solver options of a run: `given` (None: not given) over `defaults`, and whether they are the wired configuration
    (max_val counts only with thresholding on, rho only with the "karras" grid, s_noise only with sde_eta > 0)."""
    opts = {k: defaults[k] if given.get(k) is None else given[k] for k in SOLVER_DEFAULTS}
    opts["max_val"] = check_max_val(opts["thresholding"], opts["max_val"])
    opts["rho"] = check_rho(opts["rho"]) if opts["skip_type"] == "karras" else SOLVER_DEFAULTS["rho"]
    opts["sde_eta"], opts["s_noise"] = check_sde(opts["sde_eta"], opts["s_noise"])      # (solver_plan checks what eta goes with)
    return opts, all(opts[k] == v for k, v in SOLVER_DEFAULTS.items())


class DPMSolverSampler:
    def __init__(self, model, **kwargs):
        """kwargs: generator, and the defaults of sample()'s solver options (SOLVER_DEFAULTS' keys: order, skip_type, method,
        solver_type, predict_x0, thresholding, max_val, denoise_to_zero, lower_order_final, t_end, sde_eta, s_noise, rho)."""
        self.model = model
        self.alphas_cumprod = np.asarray(model.alphas_cumprod, dtype=np.float64)
        self.generator = kwargs.get("generator", None)
        self.solver = dict(SOLVER_DEFAULTS, **{k: v for k, v in kwargs.items() if k in SOLVER_DEFAULTS and v is not None})
        opts, self.wired = solver_options(self.solver, {})
        if not self.wired:      # a mistake shows where it is made: the plan of a short run, built and dropped
            solver_plan(NoiseScheduleVP("discrete", alphas_cumprod=self.alphas_cumprod), 3 * opts["order"],
                        **{k: opts[k] for k in PLAN_OPTIONS if k != "denoise_to_zero"})

    def register_buffer(self, name, attr):
        setattr(self, name, attr)

    # ---- img2img: a run that starts at a continuous time t_start below T (dpm_solver.py:958-1075, `t_start`)
    def _check_t_start(self, t_start):
        t, n = float(t_start), self.alphas_cumprod.shape[0]
        if not 1.0 / n < t <= 1.0:
            raise ValueError(f"t_start must be a continuous time in (1/{n}, 1], got {t_start!r}")
        return t

    def q_coefficients(self, t_start):
        """(marginal_alpha, marginal_std) at the continuous time t_start."""
        ns = NoiseScheduleVP("discrete", alphas_cumprod=self.alphas_cumprod)
        t = self._check_t_start(t_start)
        return float(ns.marginal_alpha(t)), float(ns.marginal_std(t))

    def stochastic_encode(self, x0, t_start, noise=None, seeds=None):
        """x0 noised to the continuous time t_start: marginal_alpha(t_start) x0 + marginal_std(t_start) noise.  One ops.q_sample
        launch; a fresh tensor.  `noise` None: drawn per sample from `seeds` (ops.RNG_ENCODE), or without seeds from the sampler's
        generator."""
        a, b = self.q_coefficients(t_start)
        return noised_latent(x0, a, b, noise, self.generator, seeds)

    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, guidance_rescale=0., t_start=None, seeds=None, order=None, skip_type=None,
               method=None, solver_type=None, predict_x0=None, thresholding=None, max_val=None, denoise_to_zero=None,
               lower_order_final=None, t_end=None, sde_eta=None, s_noise=None, rho=None, step_noises=None,
               image_guidance_scale=None, **kwargs):
        """image_guidance_scale: None, or the image scale s_I of three-branch guidance (InstructPix2Pix), as PLMSSampler.sample
        takes it: dict conditioning on both sides with a c_concat each, the batch [uu ; ui ; ci] per evaluation, the combine
        inside the one step launch (ops.sampler_step_dual, with solver options ops.sampler_step_lin_dual).  Every solver option
        works with it but method="adaptive"; per-request lists do not.
        order, skip_type, method, solver_type, predict_x0, thresholding, max_val, denoise_to_zero, lower_order_final, t_end:
        the options of the reference's DPM_Solver(...).sample(...) (dpm_solver.solver_plan); sde_eta, s_noise, rho: the SDE
        update and the Karras grid (solver_plan; not in the reference); None: the sampler's default
        (SOLVER_DEFAULTS unless the constructor was given another).  With every option at SOLVER_DEFAULTS -- multistep, order 2,
        time_uniform, data prediction, no thresholding -- the run is the wired one described above, launch for launch.
        Otherwise the plan's records are run by solver.run_solver_plan: S model evaluations (S + 1 with denoise_to_zero), each
        followed by ONE ops.sampler_step_lin launch; callback(i) and img_callback(model value, i) fire once per evaluation,
        where the model value is the data prediction, or with predict_x0=False the noise prediction.  seeds, x_T, t_start,
        hybrid conditioning, v-prediction and guidance_rescale work as in the wired run.  Refused with non-default options:
        per-request lists (below) -- the step table's rows hold the 2M update only.
        t_start: a continuous time in (1 / N, T] -- the S evaluations then cover [t_start, 1 / N] instead of [T, 1 / N], from
        x_T = stochastic_encode(., t_start) (the reference's DPM_Solver.sample(t_start=), dpm_solver.py:958-1075).  S == 1 is a
        single first-order update.
        seeds: `batch_size` ints, one per sample -- x_T of sample b then depends on seeds[b] alone (ops.randn_seeded), and so
        does its step noise with sde_eta > 0: stream ops.RNG_STEP, draw = the record's index, drawn INSIDE the step launch (no
        launch and no tensor of its own); None: the sampler's generator, one torch.randn per stochastic record.  step_noises
        (tests): step_noises[k] is record k's noise.  `eta` (the reference's keyword) is ignored as in the reference.
        Per request: S, unconditional_guidance_scale and guidance_rescale each take a scalar or `batch_size` values; with any
        sequence every step is one ops.sampler_step_table launch on the rows of a StepTable built and uploaded before the
        loop.  Sample b runs its own multistep_2m_plan of S[b] steps -- its order and its lower-order final step included -- on
        loop iterations 0 .. S[b] - 1 and is carried along unchanged afterwards; the loop runs max(S) iterations, callbacks
        fire once per iteration, and in the data prediction handed to img_callback a finished sample holds its last value.  The
        guidance batch is used if any scale differs from 1; a sample whose scale is exactly 1.0 then goes through the
        combine eu + 1 * (ec - eu) and is not promised bit-equal to an unguided run.  Refused: an S list whose values DIFFER with
        t_start (a list that repeats one value is one grid and passes); any sequence with score_corrector or quantize_x0."""
        opts, wired = solver_options(self.solver, dict(
            order=order, skip_type=skip_type, method=method, solver_type=solver_type, predict_x0=predict_x0,
            thresholding=thresholding, max_val=max_val, denoise_to_zero=denoise_to_zero, lower_order_final=lower_order_final,
            t_end=t_end, sde_eta=sde_eta, s_noise=s_noise, rho=rho))
        per = per_request(S, unconditional_guidance_scale, guidance_rescale, batch_size)
        if per is not None and not wired:
            changed = sorted(k for k, v in SOLVER_DEFAULTS.items() if opts[k] != v)
            raise ValueError(f"per-request S / guidance scale / guidance_rescale lists run on the step table, whose rows hold "
                             f"the multistep order-2 update only: not with the solver options {', '.join(changed)}")
        if per is None:
            guidance_rescale = check_guidance_rescale(guidance_rescale)
        else:
            if score_corrector is not None or quantize_x0:
                raise ValueError("per-sample guidance scale / rescale / steps run inside the fused step launch: not with "
                                 "score_corrector or quantize_x0")
            if len(set(per[0])) > 1 and t_start is not None:
                raise ValueError("per-sample S with different values runs every sample's own full schedule: not with t_start")
        if image_guidance_scale is not None and opts["method"] == "adaptive":
            raise MdxError("DPMSolverSampler.sample: image_guidance_scale does not run with method='adaptive'")
        image_scale = check_image_guidance("DPMSolverSampler.sample", self.model, image_guidance_scale, conditioning,
                                           unconditional_conditioning, per, mask, x0)
        ig = {} if image_scale is None else {"image_scale": image_scale}      # (None: every call below as it was)
        check_seed_sources(seeds, self.generator, step_noises=step_noises)
        if t_start is not None:
            t_start = self._check_t_start(t_start)
        if conditioning is None:
            raise MdxError("DPMSolverSampler: conditioning is required (classifier-free guidance on a text-conditional UNet)")
        if mask is not None or x0 is not None:
            raise NotImplementedError("mask/x0 blending is implemented by PLMSSampler / DDIMSampler (WK inpaint.py uses PLMS); "
                                      "the reference never passes it to DPMSolverSampler")
        # bare or hybrid (inpainting) conditioning, the forms PLMSSampler takes
        cond, uc, c_cat, uc_cat, dev = split_conditioning(self.model, conditioning, unconditional_conditioning, x_T)
        if cond is not None and cond.shape[0] != batch_size:
            print(f"Warning: Got {cond.shape[0]} conditionings but batch-size is {batch_size}")
        size = (batch_size,) + tuple(shape)
        seeds = check_seeds(seeds, batch_size, dev)
        img = start_latent(x_T, seeds, size, dev, self.generator)
        ns = NoiseScheduleVP("discrete", alphas_cumprod=self.alphas_cumprod)
        if not wired:
            # the whole solver: one loop over solver_plan's records, t_rows = every evaluation's t_input (one time-embedding
            # table per run, as below)
            plan = solver_plan(ns, S, t_start=t_start, **{k: opts[k] for k in PLAN_OPTIONS})
            scale = float(unconditional_guidance_scale)
            guided = GuidedModel(self.model, batch_size, tuple(shape), cond, uc, c_cat, uc_cat, scale, dev,
                                 [r["t_input"] for r in plan], **ig)
            return run_solver_plan(plan, guided, img, scale, pred_type(self.model), guidance_rescale, opts["thresholding"],
                                   opts["max_val"], callback, img_callback, seeds, self.generator, step_noises, **ig), None
        # the launches of the run (schedule.dpm_steps) behind one surface: kernel arguments, or per request the rows of a table.
        # Either way a sample's previous data prediction is read only while its own float32 c1 is non-zero.
        counts = [S] * batch_size if per is None else per[0]
        by_steps = {s: dpm_steps(ns, s, t_start) for s in sorted(set(counts))}
        if per is None:
            scale, total = float(unconditional_guidance_scale), S
            steps, t_rows = ScalarSteps(by_steps[S], scale, guidance_rescale, **ig), [s.t_input for s in by_steps[S]]
        else:
            scale = per[1]
            steps, t_rows, total = step_table([by_steps[s] for s in counts], scale, per[2], not (uc is None and uc_cat is None))
            steps.upload(dev)
        # (model_wrapper :316-322 builds the [uncond; cond] batch)
        guided = GuidedModel(self.model, batch_size, tuple(shape), cond, uc, c_cat, uc_cat, scale, dev, t_rows, **ig)
        # The data predictions ping-pong between two buffers and a table launch writes only active rows, so on the iteration a
        # sample ends its last prediction is copied into the other buffer too: whichever one img_callback is handed shows the
        # finished sample's last value.  (Samples that end with the run -- all of them, with one S -- need no copy.)
        ending = {k: [b for b, s in enumerate(counts) if s - 1 == k] for k in range(total - 1)}
        x0_bufs = [torch.empty_like(img), torch.empty_like(img)]
        x_next = torch.empty_like(img)
        # model_wrapper, model_type "v" (dpm_solver.py:281-284): eps = alpha_t v + sigma_t x, in the step launch
        pred = pred_type(self.model)
        for k in range(total):
            eps_u, eps_c = guided(img, k)
            cur, prev = x0_bufs[k & 1], x0_bufs[(k & 1) ^ 1]
            mid = {} if image_scale is None else {"out_m": guided.out_m}
            steps.launch(k, img, eps_u, eps_c, pred, [], prev if steps.any_sigma[k] else None, None, x_next, cur, **mid)
            for b in ending.get(k, ()):
                prev[b].copy_(cur[b])
            img, x_next = x_next, img
            if callback:
                callback(k)
            if img_callback:
                img_callback(cur, k)
        return img, None
