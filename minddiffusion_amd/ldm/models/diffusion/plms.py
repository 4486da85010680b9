"""PLMSSampler -- MI355X-native mirror of the reference's ldm/models/diffusion/plms.py
(make_schedule :34-67, sample :69-122, plms_sampling :124-179, p_sample_plms :182-247; Wukong copy
WK/ldm/models/diffusion/plms.py:185-215 for the dict-conditioning form).

Same class name, constructor and ``sample(...)`` keyword surface.  What changes is the execution:
  * the host loop only enqueues work: one UNet forward (a replayed hipGraph) and ONE fused
    elementwise kernel per step (mdx_sampler_step_f32: CFG combine + Adams-Bashforth mix + x0/dir/x_prev;
    mdx_sampler_step_pred_f32 for a `parameterization: "v"` model, which adds the v -> eps conversion to the same launch;
    mdx_sampler_step_rescale_f32 when `guidance_rescale` != 0, which adds the per-sample std rescale of the CFG-combined
    output to the same launch),
    instead of ~15 separately dispatched MindSpore ops (plms.py:192-197, 218-226, 235-244);
  * the constant [2B,77,D] CFG context concat (plms.py:194) is built once, not every step, and its
    cross-attention K/V projections are cached inside the UNet;
  * per-step scalars are host floats (no `ms.numpy.full` tensors, plms.py:212-215).
Results are identical in structure to the reference (S+1 UNet calls for PLMS, intermediates dict,
callbacks once per step).
img2img (not in the reference): ``stochastic_encode(x0, t_enc)`` + ``decode(x_t, cond, t_start)`` run the last t_start steps
of the schedule through the same loop; the per-step mask blend of that path is one mdx_q_sample_f32 launch.
Per-sample seeds (not in the reference): with ``seeds=`` every draw -- x_T, the eta > 0 step noise, the mask blend, the
stochastic_encode noise -- is one mdx_randn_f32 launch keyed by the sample's own seed (ops.randn_seeded), so a sample does not
depend on the batch it is served in; without it the sampler's generator draws for the whole batch, as before.
Per-request parameters (not in the reference): S, unconditional_guidance_scale and guidance_rescale given as one value per
sample -- every step is then ONE mdx_sampler_step_table_f32 launch that reads each sample's scalars from its row of a table
built and uploaded once before the loop (schedule.StepTable); scalars keep the three entries above.
Either way the loop launches from ONE steps object made before it: schedule.ddim_steps says which launches a sample's run makes
with which scalars, and a schedule.ScalarSteps or an uploaded StepTable hands launch k its scalars (arguments / a table slice).
"""
import itertools

import numpy as np
import torch

from .... import ops
from ...._lib import MdxError
from ...modules.diffusionmodules.util import make_ddim_sampling_parameters, make_ddim_timesteps
from .guided import (GuidedModel, _Draws, _first_tensor, check_guidance_rescale, check_image_guidance, check_seed_sources,
                     check_seeds, noised_latent, split_conditioning, start_latent)
from .schedule import ScalarSteps, ddim_steps, per_request, pred_type, step_table


class _SamplerBase:
    """Shared loop for PLMSSampler (multistep) and DDIMSampler (single step)."""

    multistep = True

    def __init__(self, model, schedule="linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        self.verbose_print = kwargs.get("verbose_print", False)
        self.generator = kwargs.get("generator", None)

    # ---- plms.py:34-67
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if self.multistep and ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize,
                                                  num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps,
                                                  verbose=verbose and self.verbose_print)
        alphas_cumprod = np.asarray(self.model.alphas_cumprod, dtype=np.float32)
        assert alphas_cumprod.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        self.betas = self.model.betas
        self.alphas_cumprod = alphas_cumprod
        self.alphas_cumprod_prev = np.asarray(self.model.alphas_cumprod_prev, dtype=np.float32)
        self.sqrt_alphas_cumprod = np.sqrt(alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1. - alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1. - alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1. / alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1. / alphas_cumprod - 1)
        ddim_sigmas, ddim_alphas, ddim_alphas_prev = make_ddim_sampling_parameters(
            alphacums=alphas_cumprod, ddim_timesteps=self.ddim_timesteps, eta=ddim_eta,
            verbose=verbose and self.verbose_print)
        self.ddim_sigmas = ddim_sigmas
        self.ddim_alphas = ddim_alphas
        self.ddim_alphas_prev = ddim_alphas_prev
        self.ddim_sqrt_one_minus_alphas = np.sqrt(1. - ddim_alphas).astype(np.float32)
        self.ddim_sigmas_for_original_num_steps = np.float32(ddim_eta) * np.sqrt(
            (1 - self.alphas_cumprod_prev) / (1 - self.alphas_cumprod) *
            (1 - self.alphas_cumprod / self.alphas_cumprod_prev))

    # ---- plms.py:69-122
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0.,
               score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, guidance_rescale=0., seeds=None,
               image_guidance_scale=None, **kwargs):
        """image_guidance_scale: None, or the image scale s_I of three-branch guidance (InstructPix2Pix) -- conditioning and
        unconditional_conditioning are then dicts with a c_concat each (the image latent and its zero), every model evaluation
        runs the batch [uu ; ui ; ci] and the step launch combines e_uu + s_I (e_ui - e_uu) + s_T (e_ci - e_ui), s_T =
        unconditional_guidance_scale, in the one launch (ops.sampler_step_dual).  Not with per-request lists, mask / x0, windowed
        or controlled models, several ranks.
        seeds: `batch_size` ints, one per sample -- every draw of sample b (x_T, the eta > 0 step noise, the mask blend)
        then depends on seeds[b] alone and not on the batch around it (ops.randn_seeded); None: the sampler's generator.
        Per request: S, unconditional_guidance_scale and guidance_rescale each take a scalar or `batch_size` values (list,
        tuple, 1-d array or tensor).  With any sequence the run reads its step scalars from a StepTable (one
        ops.sampler_step_table launch per model evaluation).  Sample b runs its own complete S[b]-step schedule on loop
        iterations 0 .. S[b] - 1 and is carried along unchanged afterwards; the loop runs max(S) iterations, callbacks and
        intermediates fire once per iteration, and a finished sample's pred_x0 holds its last value.  The guidance batch is
        used if any scale differs from 1; a sample whose scale is exactly 1.0 then goes through the combine
        eu + 1 * (ec - eu) and is not promised bit-equal to an unguided run.  eta, temperature and noise_dropout stay
        scalars.  Refused: an S list whose values DIFFER with mask / x0, timesteps= or ddim_use_original_steps (a list that
        repeats one value is one grid and passes); any sequence with score_corrector or quantize_x0 (they leave the fused
        launch)."""
        per = per_request(S, unconditional_guidance_scale, guidance_rescale, batch_size)
        if per is None:
            guidance_rescale = check_guidance_rescale(guidance_rescale)
        check_image_guidance(f"{type(self).__name__}.sample", self.model, image_guidance_scale, conditioning,
                             unconditional_conditioning, per, mask, x0)       # (an S list is seen here only)
        if conditioning is not None:
            cbs = _first_tensor(conditioning).shape[0]
            if cbs != batch_size:
                print(f"Warning: Got {cbs} conditionings but batch-size is {batch_size}")
        grids = None
        if per is not None and len(set(per[0])) > 1:
            if mask is not None or x0 is not None or kwargs.get("timesteps") is not None or kwargs.get("ddim_use_original_steps"):
                raise ValueError("per-sample S with different values runs every sample's own full schedule: not with "
                                 "mask / x0, timesteps= or ddim_use_original_steps")
            by_steps = {}
            for s_b in sorted(set(per[0])):                          # ends on max(S): the schedule the sampler keeps
                self.make_schedule(ddim_num_steps=s_b, ddim_eta=eta, verbose=verbose)
                by_steps[s_b] = self.time_grid(False, None, None)
            grids = [by_steps[s_b] for s_b in per[0]]
        else:
            self.make_schedule(ddim_num_steps=S if per is None else per[0][0], ddim_eta=eta, verbose=verbose)
        if per is not None:
            unconditional_guidance_scale, guidance_rescale = per[1], per[2]
        C, H, W = shape
        size = (batch_size, C, H, W)
        if verbose:
            print(f'Data shape for {type(self).__name__} sampling is {size}')
        # the reference's sample() always runs the S-step DDIM grid (plms.py:107-121); `timesteps` /
        # `ddim_use_original_steps` are plms_sampling() options (plms.py:134-142) and are forwarded when given
        return self.plms_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                  quantize_denoised=quantize_x0, mask=mask, x0=x0,
                                  ddim_use_original_steps=bool(kwargs.get("ddim_use_original_steps", False)),
                                  timesteps=kwargs.get("timesteps"), dropout_masks=kwargs.get("dropout_masks"),
                                  step_noises=kwargs.get("step_noises"),
                                  noise_dropout=noise_dropout, temperature=temperature,
                                  score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, x_T=x_T,
                                  log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, verbose=verbose,
                                  blend_noises=kwargs.get("blend_noises"), guidance_rescale=guidance_rescale, seeds=seeds,
                                  grids=grids, image_guidance_scale=image_guidance_scale)

    # ---- img2img: upstream LDM's DDIMSampler.stochastic_encode / decode (neither reference tree has them).
    # t_enc / t_start count the model evaluations that REMAIN (1 .. S; PLMS spends one more on its first step): the partial run
    # walks grid indices t_enc - 1 ... 0, and stochastic_encode noises to the level of the first step that will run,
    # ddim_alphas[t_enc - 1] = alphas_cumprod[ddim_timesteps[t_enc - 1]].  Upstream noises to index t_enc and then starts
    # denoising at t_enc - 1 -- one grid point of noise more than the run removes, and no way to say strength = 1 (index S does
    # not exist); here t_enc == S is the full run from x_T's own level.
    def _need_schedule(self, what):
        if not hasattr(self, "ddim_timesteps"):
            raise MdxError(f"{type(self).__name__}.{what}: call make_schedule(ddim_num_steps, ddim_eta) first")

    @staticmethod
    def _check_t_start(t_start, n):
        if isinstance(t_start, bool) or int(t_start) != t_start or not 1 <= int(t_start) <= n:
            raise ValueError(f"t_start / t_enc must be an integer in [1, {n}] (the model evaluations that remain), got {t_start!r}")
        return int(t_start)

    def q_coefficients(self, t_enc, use_original_steps=False):
        """(sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod)) at the first step a decode(t_start=t_enc) runs."""
        self._need_schedule("stochastic_encode")
        if use_original_steps:
            t = self._check_t_start(t_enc, self.ddpm_num_timesteps) - 1
        else:
            t = int(self.ddim_timesteps[self._check_t_start(t_enc, self.ddim_timesteps.shape[0]) - 1])
        return self.sqrt_alphas_cumprod[t], self.sqrt_one_minus_alphas_cumprod[t]

    def stochastic_encode(self, x0, t_enc, use_original_steps=False, noise=None, seeds=None):
        """x0 noised to where decode(t_start=t_enc) starts: sqrt(a) x0 + sqrt(1 - a) noise, a = ddim_alphas[t_enc - 1] (see the
        note above for the difference from upstream LDM, which uses index t_enc).  One ops.q_sample launch; a fresh tensor.
        `noise` None: drawn per sample from `seeds` (ops.RNG_ENCODE), or without seeds from the sampler's generator."""
        a, b = self.q_coefficients(t_enc, use_original_steps)
        return noised_latent(x0, a, b, noise, self.generator, seeds)

    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1., unconditional_conditioning=None,
               use_original_steps=False, callback=None, img_callback=None, mask=None, x0=None, guidance_rescale=0.,
               log_every_t=100, seeds=None, image_guidance_scale=None, **test_injection_kwargs):
        """The last t_start steps of the schedule make_schedule() set up (its eta included), from x_latent =
        stochastic_encode(., t_start): plms_sampling's loop on ts[:t_start].  t_start == S is sample(S, x_T=x_latent).
        mask / x0: 1 = keep x0 (the init latent), blended every step by one in-place ops.q_sample launch.
        seeds: per-sample seeds of the step and blend draws, as sample() takes them.
        image_guidance_scale: three-branch guidance, as sample() takes it.
        test_injection_kwargs: step_noises / blend_noises / dropout_masks, as sample() takes them.
        Returns (samples, intermediates)."""
        self._need_schedule("decode")
        unknown = set(test_injection_kwargs) - {"step_noises", "blend_noises", "dropout_masks"}
        if unknown:
            raise TypeError(f"decode() got unexpected keyword arguments {sorted(unknown)}")
        x_latent = torch.as_tensor(x_latent)
        grid = self.ddpm_num_timesteps if use_original_steps else self.ddim_timesteps.shape[0]
        return self.plms_sampling(cond, tuple(x_latent.shape), x_T=x_latent, ddim_use_original_steps=use_original_steps,
                                  callback=callback, img_callback=img_callback, mask=mask, x0=x0, log_every_t=log_every_t,
                                  unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, verbose=False,
                                  guidance_rescale=guidance_rescale, t_start=self._check_t_start(t_start, grid), seeds=seeds,
                                  image_guidance_scale=image_guidance_scale, **test_injection_kwargs)

    # ---- which timesteps, and which tables `index` selects from (plms.py:134-142, 205-208)
    def time_grid(self, ddim_use_original_steps, timesteps, t_start):
        """(time_range, alphas, alphas_prev, sqrt_one_minus_alphas, sigmas): the timesteps in loop order (descending) and the
        tables the grid index selects from.  t_start keeps the last t_start steps."""
        if ddim_use_original_steps:
            # every DDPM step (or the first `timesteps` of them): tables are the model's alphas_cumprod themselves.  The
            # reference reads `self.model.ddim_sigmas_for_original_num_steps` (plms.py:208), an attribute make_schedule
            # creates on the SAMPLER (plms.py:64-67): we use the sampler's.
            n_orig = int(self.ddpm_num_timesteps if timesteps is None else timesteps)
            if not 0 < n_orig <= self.ddpm_num_timesteps:
                raise ValueError(f"timesteps must be in (0, {self.ddpm_num_timesteps}] with ddim_use_original_steps")
            if t_start is not None:
                n_orig = self._check_t_start(t_start, n_orig)
            return (np.arange(n_orig - 1, -1, -1, dtype=np.int64), self.alphas_cumprod, self.alphas_cumprod_prev,
                    self.sqrt_one_minus_alphas_cumprod, np.asarray(self.ddim_sigmas_for_original_num_steps, dtype=np.float32))
        ts = self.ddim_timesteps
        if timesteps is not None:                                    # plms.py:137-139: a prefix of the DDIM grid
            n_ddim = ts.shape[0]
            subset_end = int(min(timesteps / n_ddim, 1) * n_ddim) - 1
            ts = ts[:subset_end]
            if ts.shape[0] == 0:
                raise ValueError(f"timesteps={timesteps} selects an empty subset of the {n_ddim}-step DDIM grid")
        if t_start is not None:
            ts = ts[:self._check_t_start(t_start, ts.shape[0])]
        return np.flip(ts), self.ddim_alphas, self.ddim_alphas_prev, self.ddim_sqrt_one_minus_alphas, self.ddim_sigmas

    def _check_options(self, mask, x0, score_corrector, quantize_denoised, noise_dropout):
        if mask is not None and x0 is None:
            raise ValueError("mask blending needs x0 (plms.py:154)")
        # quantize_x0 / score_corrector (plms.py:199-201, 218-219) call into caller-supplied objects (a first stage with
        # .quantize, a corrector with .modify_score) between the pieces of the fused step; see step() in plms_sampling
        if score_corrector is not None and self.model.parameterization != "eps":
            raise AssertionError('score_corrector needs parameterization == "eps" (plms.py:200)')
        if quantize_denoised and not hasattr(getattr(self.model, "first_stage_model", None), "quantize"):
            raise MdxError("quantize_x0 needs model.first_stage_model.quantize (plms.py:219)")
        if not 0. <= float(noise_dropout) < 1.:
            raise ValueError("noise_dropout must be in [0, 1)")

    # ---- plms.py:124-179 + 182-247
    def plms_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, verbose=True, blend_noises=None,
                      dropout_masks=None, step_noises=None, guidance_rescale=0., t_start=None, seeds=None, grids=None,
                      image_guidance_scale=None):
        """t_start (decode() passes it, nothing else does): run only the LAST t_start steps of the grid -- grid indices
        t_start - 1 ... 0, ts[:t_start] -- from x_T, a latent at the noise level of index t_start - 1.  In that mode the
        mask / x0 blend of every step is one ops.q_sample launch, in place.
        unconditional_guidance_scale / guidance_rescale: a scalar, or one value per sample -- then every step is one
        ops.sampler_step_table launch on the rows of a StepTable built and uploaded before the loop (sample()).
        grids (sample() passes it, nothing else does): one time_grid() per sample, each sample its own step count.
        In order: validate, normalise the conditioning and draw the start latent, select the time grid, build the guided model
        call, loop."""
        per = per_request(None, unconditional_guidance_scale, guidance_rescale, shape[0])
        if per is None:
            guidance_rescale = check_guidance_rescale(guidance_rescale)
        elif score_corrector is not None or quantize_denoised:
            raise ValueError("per-sample guidance scale / rescale / steps run inside the fused step launch: not with "
                             "score_corrector or quantize_x0")
        image_scale = check_image_guidance(f"{type(self).__name__}.sample", self.model, image_guidance_scale, cond,
                                           unconditional_conditioning, per, mask, x0)
        ig = {} if image_scale is None else {"image_scale": image_scale}      # (None: every call below as it was)
        check_seed_sources(seeds, self.generator, step_noises=step_noises, blend_noises=blend_noises, dropout_masks=dropout_masks)
        self._check_options(mask, x0, score_corrector, quantize_denoised, noise_dropout)
        corrector_kwargs = corrector_kwargs or {}
        cond, uc, c_cat, uc_cat, dev = split_conditioning(self.model, cond, unconditional_conditioning, x_T)
        b = shape[0]
        # per-sample seeds: every draw below becomes one ops.randn_seeded launch, (stream, draw) = what it is for and which one
        seeds = check_seeds(seeds, b, dev)
        img = start_latent(x_T, seeds, shape, dev, self.generator)
        grid = self.time_grid(ddim_use_original_steps, timesteps, t_start)
        time_range = grid[0]
        total_steps = int(time_range.shape[0])
        if verbose:
            print(f"Running {type(self).__name__} Sampling with {total_steps} timesteps")
        scale = float(unconditional_guidance_scale) if per is None else per[1]
        if mask is not None:
            mask = torch.as_tensor(mask).to(device=dev, dtype=torch.float32)
            x0 = torch.as_tensor(x0).to(device=dev, dtype=torch.float32)
            if t_start is not None:     # the blend kernel's operands: contiguous, the mask [B, 1 | C, H, W]
                x0 = x0.expand(shape).contiguous()
                if mask.dim() != 4 or mask.shape[1] not in (1, shape[1]):
                    raise MdxError(f"mask must be [B, 1, H, W] or [B, C, H, W], got {tuple(mask.shape)}")
                mask = mask.expand((b, mask.shape[1]) + tuple(shape[2:])).contiguous()
        # every scalar of every launch (schedule.ddim_steps) behind one surface: kernel arguments, or per request the rows of a
        # table.  second_row: the row of the guided model's timesteps that PLMS' second evaluation reads
        if per is None:
            steps, t_rows = ScalarSteps(ddim_steps(self, grid, self.multistep), scale, guidance_rescale, **ig), time_range
            second_row = min(1, total_steps - 1)
        else:
            plans = [ddim_steps(self, g, self.multistep) for g in grids or [grid] * b]
            steps, t_rows, total_steps = step_table(plans, per[1], per[2], not (uc is None and uc_cat is None),
                                                    second_call_row=self.multistep)
            steps.upload(dev)
            second_row = total_steps                                  # the one step_table appended after the loop's
        guided = GuidedModel(self.model, b, tuple(shape[1:]), cond, uc, c_cat, uc_cat, scale, dev, t_rows, **ig)
        draws = _Draws(seeds, self.generator, dev, shape, step_noises, dropout_masks, blend_noises, temperature, noise_dropout)

        intermediates = {'x_inter': [img.clone()], 'pred_x0': [img.clone()]}
        pool = [torch.empty_like(img) for _ in range(4)]  # eps history buffers (3 live + 1 being written)
        hist = []                                         # newest first; at most 3 (plms.py:169-171)
        pred_x0 = torch.empty_like(img)
        x_next = torch.empty_like(img)
        hook_e = torch.empty_like(img) if score_corrector is not None else None
        hook_x = torch.empty_like(img) if score_corrector is not None else None
        hook_p = torch.empty_like(img) if quantize_denoised else None
        # a v-prediction model (SD 2.x 768-v): the step kernel converts the UNet's output to eps at the point (xm, tm) the model
        # was evaluated at; everything after that -- history, pred_x0, x_prev -- is the eps path.  Guidance rescale: the
        # CFG-combined output of every model evaluation is pulled back to the conditional output's per-sample std inside the
        # step launch.  ops.sampler_update picks the entry.
        pred = pred_type(self.model)
        calls = itertools.count()

        def step(x, eps_u, eps_c, olds, e_out, x_out, p_out, xm=None):
            """The next launch of the run: one get_x_prev_and_pred_x0 (plms.py:210-228) on e' = coef[0] * e_t + sum coef[k] *
            olds[k-1], e_t = the CFG-combined model output (optionally written to e_out), with the scalars `steps` holds for it.
            xm: the image the model output was evaluated at when not x (what a score corrector is handed, plms.py:201, and where
            a v output is converted to eps).  The two hooks are scalar-only: they read steps.plan."""
            k = next(calls)
            mid = {} if image_scale is None else {"out_m": guided.out_m}      # the middle output of the evaluation just made
            if score_corrector is not None:
                # e_t leaves the fused kernel (pass 1: CFG combine only -- the rescale belongs to the combine that produces
                # e_t, so to this pass), goes through the caller's modify_score, and re-enters as a single NHWC fp16 model
                # output (pass 2: multistep mix + update)
                # (a corrector implies an eps model -- _check_options -- so hook_e holds eps and PRED_EPS is the whole story)
                ops.sampler_update(x, eps_u, eps_c, scale, ops.PRED_EPS, [], (1., 0., 0., 0.),
                                   (1., 0., 1., 0., 0., None, hook_e, hook_x, None), guidance_rescale,
                                   **({} if not mid else dict(mid, mid_scale=image_scale)))
                mid = {}
                tvec = torch.full((b,), int(steps.plan[k].t_input), device=dev, dtype=torch.long)
                e_mod = score_corrector.modify_score(self.model, hook_e, x if xm is None else xm, tvec, cond,
                                                     **corrector_kwargs)
                e_mod = torch.as_tensor(e_mod).to(device=dev, dtype=torch.float32).contiguous()
                if tuple(e_mod.shape) != tuple(x.shape):
                    raise MdxError(f"score_corrector returned shape {tuple(e_mod.shape)}, expected {tuple(x.shape)}")
                eps_c = ops.nchw_to_nhwc(e_mod, (x.shape[1] + 7) // 8 * 8)
                eps_u = None
            noise = draws.step() if steps.any_sigma[k] else None
            if quantize_denoised and p_out is None:
                p_out = hook_p
            steps.launch(k, x, eps_u, eps_c, pred, olds, noise, e_out, x_out, p_out, xm, **mid)
            if quantize_denoised:
                # pred_x0, _, *_ = first_stage_model.quantize(pred_x0) (plms.py:218-219); x_prev is linear in pred_x0
                q = self.model.first_stage_model.quantize(p_out)[0]
                q = torch.as_tensor(q).to(device=dev, dtype=torch.float32)
                x_out.add_((q - p_out) * float(steps.plan[k].update[2]))        # sqrt_a_prev
                p_out.copy_(q)

        # (per request with step counts that differ, time_range is the longest grid -- sample() made that schedule last -- and
        # index / step_t of a sample are its own: the table's, and t_rows')
        for i, step_t in enumerate(time_range):
            index = total_steps - i - 1
            if mask is not None:
                noise = draws.blend(i, x0)
                if t_start is not None:                               # q_sample + blend, one launch, in place
                    ops.q_sample(x0, noise.contiguous(), self.sqrt_alphas_cumprod[int(step_t)],
                                 self.sqrt_one_minus_alphas_cumprod[int(step_t)], out=img, mask=mask, img=img)
                else:
                    ts = torch.full((b,), int(step_t), device=dev, dtype=torch.long)
                    img_orig = self.model.q_sample(x0, ts, noise)
                    img = img_orig * mask + (1. - mask) * img
            eps_u, eps_c = guided(img, i)
            if not self.multistep:
                step(img, eps_u, eps_c, [], None, x_next, pred_x0)
            else:
                e_buf = pool.pop()
                if not hist:
                    # Pseudo Improved Euler (2nd order), plms.py:231-235: S+1 UNet calls in total
                    step(img, eps_u, eps_c, [], e_buf, x_next, None)
                    eps_u2, eps_c2 = guided(x_next, second_row)
                    step(img, eps_u2, eps_c2, [e_buf], None, x_next, pred_x0, xm=x_next)
                else:             # Adams-Bashforth 2 / 3 / 4, plms.py:236-244
                    step(img, eps_u, eps_c, hist, e_buf, x_next, pred_x0)
                hist.insert(0, e_buf)
                if len(hist) > 3:
                    pool.append(hist.pop())
            img, x_next = x_next, img
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if index % log_every_t == 0 or index == total_steps - 1:
                intermediates['x_inter'].append(img.clone())
                intermediates['pred_x0'].append(pred_x0.clone())
        return img, intermediates


class PLMSSampler(_SamplerBase):
    """Reference: ldm/models/diffusion/plms.py:27 ``class PLMSSampler``."""
    multistep = True
