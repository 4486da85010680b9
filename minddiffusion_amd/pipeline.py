"""DiffusionPipeline -- what the reference's txt2img.py main loop does around the sampler
(vision/stablediffusionv2/txt2img.py:242-268; Wukong: wukong-huahua/txt2img.py:255-281):

    uc = model.get_learned_conditioning(B * [""]); c = model.get_learned_conditioning(prompts)
    shape = [4, H // 8, W // 8]
    samples, _ = sampler.sample(S=steps, conditioning=c, batch_size=B, shape=shape, verbose=False,
                                unconditional_guidance_scale=scale, unconditional_conditioning=uc, eta=eta, x_T=x_T)
    x = model.decode_first_stage(samples)

Text encoding and VAE decode are outside the hot path: pass precomputed
conditioning tensors (c, uc), or attach ``model.cond_stage_model`` / ``model.first_stage_model``.
With torch.distributed initialised the global batch is sharded across ranks (distributed.py).
"""
import contextlib

import numpy as np
import torch

from . import distributed as D
from . import ops
from ._lib import MdxError
from .ldm.models.diffusion.ddim import DDIMSampler
from .ldm.models.diffusion.guided import check_guidance_rescale, use_cfg
from .ldm.models.diffusion.plms import PLMSSampler
from .ldm.models.diffusion.schedule import as_sequence, check_strength, dpm_partial_start, per_request
from .ldm.modules.encoders import WINDOW, pad_conditioning


class DiffusionPipeline:
    def __init__(self, model, sampler="ddim", device=None, solver=None):
        """solver: with sampler='dpm_solver', the defaults of DPMSolverSampler's solver options -- dict(order=3,
        skip_type="logSNR", method="singlestep", ...), see DPMSolverSampler.sample; every run of this pipeline, and of the
        pipelines windowed() and hires() derive from it, then uses them.  With sampler='uni_pc' (UniPCSampler: the multistep
        predictor-corrector, order 3, bh2) solver holds that sampler's options -- dict(order=2, variant="bh1",
        skip_type="karras", corrector=False, ...), see UniPCSampler.sample."""
        self.model = model
        self.device = torch.device(device) if device is not None else model.unet.device
        if solver is not None and sampler not in ("dpm_solver", "uni_pc"):
            raise ValueError("solver= holds DPM-Solver options: pass sampler='dpm_solver' (or a DPMSolverSampler built with them)")
        if isinstance(sampler, str):
            if sampler not in ("ddim", "plms", "dpm_solver", "uni_pc"):
                raise ValueError("sampler must be 'ddim', 'plms', 'dpm_solver' or 'uni_pc'")
            if sampler == "uni_pc":
                from .ldm.models.diffusion.uni_pc import UniPCSampler
                sampler = UniPCSampler(model, **(solver or {}))
            elif sampler == "dpm_solver":
                from .ldm.models.diffusion.dpm_solver import DPMSolverSampler
                from .ldm.models.diffusion.dpm_solver.solver import SOLVER_DEFAULTS
                unknown = sorted(set(solver or {}) - set(SOLVER_DEFAULTS))
                if unknown:
                    raise ValueError(f"solver: unknown option(s) {', '.join(unknown)}; known: {', '.join(sorted(SOLVER_DEFAULTS))}")
                sampler = DPMSolverSampler(model, **(solver or {}))    # txt2img.py --dpm_solver
            else:
                sampler = (DDIMSampler if sampler == "ddim" else PLMSSampler)(model)
        self.sampler = sampler
        self.seam_cols = 0            # latent columns of circular padding per side around the decoder (windowed(wrap_x=True))
        self._hires_kept = {}         # hires(): the inner pipeline of a windowed one, and one windowed pipeline per base size

    def start_noise(self, batch, shape, seed):
        """numpy RandomState(seed).randn -- the reference's own practice for reproducible x_T
        (wukong-huahua/inpaint.py:68-70); MindSpore's StandardNormal stream is not reproducible."""
        return torch.from_numpy(np.random.RandomState(seed).randn(batch, *shape).astype(np.float32))

    @staticmethod
    def check_seeds(seeds, batch):
        """`seeds=`: one int per sample of the GLOBAL batch (a sequence or a 1-d tensor); returned as a list, None stays None."""
        if seeds is None:
            return None
        seeds = seeds.tolist() if isinstance(seeds, torch.Tensor) else list(seeds)
        if len(seeds) != batch:
            raise MdxError(f"DiffusionPipeline: {len(seeds)} seeds for a global batch of {batch}")
        return seeds

    def seeded_noise(self, seeds, stream, shape):
        """N(0, 1) [len(seeds), *shape] on the pipeline's device, sample b from seeds[b] alone (ops.randn_seeded, draw 0)."""
        return ops.randn_seeded(ops.seeds_tensor(seeds, self.device), stream, 0, tuple(shape))

    def match_conditioning(self, c, uc, from_prompts=False):
        """Long prompts ([B, n * 77, D], encoders.chunk_token_ids): the samplers run c and uc as ONE [2B, T, D] context, so both
        need the same number of windows.  The shorter one is extended with the encoding of the empty window: with prompts= that
        is uc's own row; with tensors the attached text encoder supplies it, and without one the caller has to
        (encoders.pad_conditioning)."""
        if c is None or uc is None or c.shape[1] == uc.shape[1]:
            return c, uc
        if from_prompts:
            empty = uc[:1, :WINDOW]
        elif getattr(self.model, "cond_stage_model", None) is not None:
            empty = self.model.get_learned_conditioning([""])[:, :WINDOW]
        else:
            raise MdxError(f"DiffusionPipeline: c has {c.shape[1]} context tokens and uc {uc.shape[1]}, and no text encoder is "
                           f"attached to encode the empty window: bring them to one length with "
                           f"minddiffusion_amd.ldm.modules.encoders.pad_conditioning(c, uc, empty)")
        return pad_conditioning(c, uc, empty)

    def fit_context(self, c):
        """Single rank: a context longer than the UNet's capacity raises the capacity to the next multiple of 80 (lengths in
        between share plans; UNetModel.set_max_context_len drops the plans when the value changes)."""
        unet = getattr(self.model, "unet", None)
        T = int(c.shape[1])
        if hasattr(unet, "set_max_context_len") and T > int(unet.max_context_len):
            unet.set_max_context_len(80 * -(-T // 80))

    # ---- what every entry point does around its sampler call
    @property
    def _dpm(self):
        """DPM-Solver starts a partial run at a continuous time and has no decode(); PLMS / DDIM count grid steps."""
        from .ldm.models.diffusion.dpm_solver import DPMSolverSampler
        return isinstance(self.sampler, DPMSolverSampler) or self._unipc

    @property
    def _unipc(self):
        from .ldm.models.diffusion.uni_pc import UniPCSampler
        return isinstance(self.sampler, UniPCSampler)

    def _solver(self):
        """The solver options this pipeline's DPMSolverSampler or UniPCSampler holds off their defaults (None: none, or another
        sampler): what a derived pipeline's sampler is built with."""
        if self._unipc:
            from .ldm.models.diffusion.uni_pc.sampler import UNIPC_DEFAULTS
            return {k: v for k, v in self.sampler.solver.items() if v != UNIPC_DEFAULTS[k]} or None
        if not self._dpm or self.sampler.wired:
            return None
        from .ldm.models.diffusion.dpm_solver.solver import SOLVER_DEFAULTS
        return {k: v for k, v in self.sampler.solver.items() if v != SOLVER_DEFAULTS[k]}

    def _encoded(self, prompts, c, uc, required=True):
        """(c, uc) with one number of context windows: the prompts encoded (txt2img.py:246-251), or the tensors given."""
        if prompts is not None:
            uc = self.model.get_learned_conditioning(len(prompts) * [""])   # txt2img.py:246-248
            c = self.model.get_learned_conditioning(list(prompts))            # txt2img.py:251
        if c is None and required:
            raise MdxError("DiffusionPipeline: pass prompts (with a text encoder attached) or (c, uc) tensors")
        return self.match_conditioning(c, uc, from_prompts=prompts is not None)

    def _on_device(self, c, uc, B):
        """Single rank: c and uc fp16 on the device, a batch-1 uc repeated, the UNet's context capacity fitted to them."""
        c = c.to(self.device, torch.float16)
        uc = None if uc is None else uc.to(self.device, torch.float16)
        if uc is not None and uc.shape[0] == 1 and B > 1:
            uc = uc.expand(B, -1, -1).contiguous()
        self.fit_context(c)
        return c, uc

    def _draw(self, given, seeds, stream, shape, sd):
        """N(0, 1) [B, ...]: the tensor a caller passed, else sample b from seeds[b] alone, else RandomState(sd) as start_noise."""
        if given is not None:
            return given
        if seeds is not None:
            return self.seeded_noise(seeds, stream, shape[1:])
        return self.start_noise(shape[0], shape[1:], sd)

    @staticmethod
    def _sampler_kw(guidance_rescale, seeds):
        """The keywords only a run that uses them hands its sampler (a caller's own sampler object may not take them)."""
        kw = {"guidance_rescale": guidance_rescale} if guidance_rescale != 0. else {}
        if seeds is not None:
            kw["seeds"] = seeds
        return kw

    @staticmethod
    def check_request_lists(what, batch, steps, scale, guidance_rescale, steps_list=True):
        """`steps`, `scale` and `guidance_rescale` of a call, each one value or one per sample of the batch (the samplers'
        per-request form, schedule.per_request): the checked guidance_rescale.  batch None: the lengths are the sampler's to
        check.  steps_list False: a partial run -- `strength` fixes one grid for the whole batch -- takes one step count.
        Any list needs a single rank."""
        seq = {k: as_sequence(v) is not None for k, v in (("steps", steps), ("scale", scale),
                                                            ("guidance_rescale", guidance_rescale))}
        if not any(seq.values()):
            return check_guidance_rescale(guidance_rescale)
        if seq["steps"] and not steps_list:
            raise ValueError(f"{what}: `strength` fixes one grid for the whole batch: steps must be one int, not one per sample")
        if D.world()[1] > 1:
            raise MdxError(f"{what}: per-sample steps / scale / guidance_rescale runs on a single rank (the sharded form is "
                           f"not built)")
        if batch is None:
            batch = max(len(as_sequence(v)) for k, v in (("steps", steps), ("scale", scale),
                                                          ("guidance_rescale", guidance_rescale)) if seq[k])
        per_request(steps, scale, guidance_rescale, batch)
        return guidance_rescale

    def _partial_start(self, steps, t_enc, eta):
        """(start, a, b): where the last t_enc of `steps` steps begin -- a grid index for PLMS / DDIM, for DPM-Solver the
        continuous time t_0 + (T - t_0) * t_enc / steps of the full run's own intervals -- and the forward-process coefficients
        a * x0 + b * noise of that level."""
        if self._dpm:
            start = dpm_partial_start(self.sampler.alphas_cumprod.shape[0], steps, t_enc)
        else:
            self.sampler.make_schedule(ddim_num_steps=steps, ddim_eta=eta, verbose=False)
            start = t_enc
        return (start,) + tuple(self.sampler.q_coefficients(start))

    def _run_partial(self, x_enc, cond, uc, start, t_enc, scale, callback, img_callback, kw, mask=None, x0=None):
        """The last t_enc steps from x_enc, a latent noised to `start` (_partial_start): the final latent."""
        common = dict(unconditional_guidance_scale=scale, unconditional_conditioning=uc, callback=callback,
                      img_callback=img_callback, **kw)
        if self._dpm:
            return self.sampler.sample(S=t_enc, conditioning=cond, batch_size=int(x_enc.shape[0]), shape=list(x_enc.shape[1:]),
                                       verbose=False, x_T=x_enc, t_start=start, **common)[0]
        blend_kw = {} if mask is None else {"mask": mask, "x0": x0}
        return self.sampler.decode(x_enc, cond, t_enc, **blend_kw, **common)[0]

    def _decode_latent(self, samples):
        """model.decode_first_stage; on a wrap_x pipeline with seam_pad > 0 the latent is padded circularly by seam_cols columns
        per side first and the padded image columns are cropped, so the decoder's 3 x 3 convs see the other edge of the panorama
        where they would see zeros.  (GroupNorm and the mid attention are global: this is not exact periodicity.)  With VAE
        tiling on (enable_vae_tiling) the VAE takes the pipeline's wrap_x instead and nothing is padded: the seam is a tile
        boundary like any other."""
        vae = self._tiled_vae()
        if vae is not None:
            return vae.decode(1. / self.model.scale_factor * samples, wrap_x=bool(getattr(self.model, "wrap_x", False)))
        pad = min(int(self.seam_cols), int(samples.shape[-1]))
        if pad <= 0:
            return self.model.decode_first_stage(samples)             # txt2img.py:265-266
        padded = torch.cat([samples[..., -pad:], samples, samples[..., :pad]], -1).contiguous()
        x = self.model.decode_first_stage(padded)
        cut = pad * (int(x.shape[-1]) // int(padded.shape[-1]))        # (the VAE's own factor: 8 for SD)
        return x[..., cut:int(x.shape[-1]) - cut].contiguous()

    def _decoded(self, samples):
        vae = self._tiled_vae()
        if vae is not None:                                           # (the [0, 1] conversion inside the blend launch)
            return vae.decode_unit(1. / self.model.scale_factor * samples, wrap_x=bool(getattr(self.model, "wrap_x", False)))
        x = self._decode_latent(samples)
        return torch.clamp((x + 1.0) / 2.0, 0.0, 1.0)

    # ---- tiled VAE (AutoencoderKL.enable_tiling): the setting lives on the VAE, which windowed() and hires() pipelines share
    def _tiled_vae(self):
        vae = getattr(self.model, "first_stage_model", None)
        return vae if getattr(vae, "tiling", None) is not None else None

    def _vae(self, what):
        vae = getattr(self.model, "first_stage_model", None)
        if not hasattr(vae, "enable_tiling"):
            raise MdxError(f"DiffusionPipeline.{what}: no VAE with tiling attached (model.first_stage_model)")
        return vae

    def enable_vae_tiling(self, tile=64, overlap=16, max_tile_batch=8):
        """Decode and encode canvases larger than `tile` latent pixels tile by tile (AutoencoderKL.enable_tiling); on a wrap_x
        pipeline the decode wraps its tiles around the seam and seam_pad is not used."""
        self._vae("enable_vae_tiling").enable_tiling(tile=tile, overlap=overlap, max_tile_batch=max_tile_batch)
        return self

    def disable_vae_tiling(self):
        self._vae("disable_vae_tiling").disable_tiling()
        return self

    # ---- regional prompts (ldm/models/diffusion/windowed.py): a mask over the canvas and a prompt each
    @staticmethod
    def background_mask(masks):
        """[R, h, w] region masks in [0, 1] -> [1 + R, h, w] with the call's own prompt as region 0 on 1 - max_r m_r: the
        masks then sum to >= 1 at every pixel."""
        return torch.cat([(1.0 - masks.max(0).values)[None], masks], 0)

    def _check_regions_allowed(self, what, regions):
        """regions= is refused, before any work, on a pipeline that is not windowed and on several ranks."""
        from .ldm.models.diffusion.windowed import WindowedDiffusion
        if regions is None:
            return
        if not isinstance(self.model, WindowedDiffusion):
            raise MdxError(f"{what}: regions= needs a windowed pipeline (DiffusionPipeline.windowed)")
        if D.world()[1] > 1:
            raise MdxError(f"{what}: regions= runs on a single rank (the sharded form is not built)")

    def _region_scope(self, what, regions, c, uc, scale, latent_hw, image_hw):
        """The `with` block of a call's `regions=[{"prompt": ... | "c": ..., "mask": m}, ...]` (None: no block).  c / uc: the
        call's conditioning as the sampler gets it, on the device.  m: [h, w] at the latent grid, or [H, W] at the image's,
        reduced with ops.inpaint_resize_mask; values in [0, 1]; shared by the batch.  The contexts are laid out as GuidedModel
        will lay out its own, by guided.use_cfg: cat([uc, c_r]) under guidance, c_r without."""
        if regions is None:
            return contextlib.nullcontext()
        self._check_regions_allowed(what, regions)
        regions = list(regions)
        if not regions:
            raise MdxError(f"{what}: regions= is empty")
        B, (h, w) = int(c.shape[0]), (int(v) for v in latent_hw)
        masks, ctxs = [], [c]
        for i, reg in enumerate(regions):
            if not isinstance(reg, dict) or "mask" not in reg or ("prompt" in reg) == ("c" in reg):
                raise MdxError(f"{what}: region {i} must be a dict with 'mask' and exactly one of 'prompt' and 'c'")
            m = torch.as_tensor(reg["mask"]).to(torch.float32)
            if m.dim() != 2 or tuple(m.shape) not in ((h, w), tuple(int(v) for v in image_hw)):
                raise MdxError(f"{what}: region {i}: the mask is {tuple(m.shape)}, expected {(h, w)} (the latent grid) or "
                               f"{tuple(int(v) for v in image_hw)} (the image)")
            if not bool(torch.isfinite(m).all()) or float(m.min()) < 0.0 or float(m.max()) > 1.0:
                raise MdxError(f"{what}: region {i}: mask values must be finite and in [0, 1]")
            m = m.to(self.device)
            if tuple(m.shape) != (h, w):
                m = ops.inpaint_resize_mask(m[None, None].contiguous(), (h, w))[0, 0]
            masks.append(m)
            if "prompt" in reg:
                cr = self.model.get_learned_conditioning(B * [reg["prompt"]])
            else:
                cr = reg["c"]
                if not (isinstance(cr, torch.Tensor) and cr.dim() == 3 and int(cr.shape[0]) in (1, B)):
                    raise MdxError(f"{what}: region {i}: c must be a tensor [{B} | 1, T, D]")
            cr = cr.to(self.device, c.dtype)
            ctxs.append(cr.expand(B, -1, -1) if cr.shape[0] != B else cr)
        T = max(int(x.shape[1]) for x in ctxs + ([uc] if uc is not None else []))
        if any(int(x.shape[1]) != T for x in ctxs) or (uc is not None and int(uc.shape[1]) != T):
            if getattr(self.model, "cond_stage_model", None) is None:
                raise MdxError(f"{what}: the region contexts and the call's c / uc differ in length and no text encoder is "
                               f"attached to encode the empty window: bring them to one length with encoders.pad_conditioning")
            if uc is not None and int(uc.shape[1]) != T:
                raise MdxError(f"{what}: a region's context is longer than the call's own c / uc ({T} tokens): give the call "
                               f"a prompt of as many windows, or pad c and uc with encoders.pad_conditioning")
            empty = self.model.get_learned_conditioning([""])[:, :WINDOW]
            longest = next(x for x in ctxs if int(x.shape[1]) == T)
            ctxs = [pad_conditioning(x, longest, empty)[0] for x in ctxs]
        self.fit_context(ctxs[0])
        guided = use_cfg(uc, None, scale)
        ctxs = [(torch.cat([uc.to(x.dtype), x], 0) if guided else x).contiguous() for x in ctxs]
        return self.model.regions(self.background_mask(torch.stack(masks)), ctxs)

    # ---- ControlNet (ldm/models/diffusion/controlled.py): a hint image steers the UNet through its skip connections
    @property
    def _controlled(self):
        return bool(getattr(self.model, "is_controlled", False))

    def _refuse_controlled(self, what):
        if self._controlled:
            raise MdxError(f"DiffusionPipeline.{what}: not on a controlled pipeline (ControlNet runs in __call__ and img2img)")

    def controlled(self, controlnet):
        """A new DiffusionPipeline on ControlledDiffusion(self.model, controlnet): the same sampler kind, solver defaults and
        device, all weights shared.  Its __call__ and img2img take control_image= (the hint, [B | 1, hint_channels, H, W] in
        [0, 1] at the image's size), control_scale= (a float, one per sample, or one per residual) and control_uncond= (False:
        the unconditional half of the guidance batch runs without control, and the ControlNet at half the batch); without
        control_image they do what they do here.  Single rank; not windowed, not hires, no sessions."""
        from .ldm.models.diffusion.controlled import ControlledDiffusion
        try:
            kind = self._session_sampler()
        except MdxError:
            raise MdxError(f"DiffusionPipeline.controlled: the new pipeline gets a sampler of this one's kind, 'ddim', 'plms' or "
                           f"'dpm_solver' / 'uni_pc'; this one's is a {type(self.sampler).__name__}") from None
        return DiffusionPipeline(ControlledDiffusion(self.model, controlnet), kind, self.device, solver=self._solver())

    def _check_control_allowed(self, what, image):
        """control_image= is refused, before any work, on a pipeline that is not controlled and on several ranks."""
        if image is None:
            return
        if not self._controlled:
            raise MdxError(f"{what}: control_image= needs a controlled pipeline (DiffusionPipeline.controlled)")
        if D.world()[1] > 1:
            raise MdxError(f"{what}: control_image= runs on a single rank (the sharded form is not built)")

    def _control_scope(self, what, image, scale, uncond, B, latent_hw):
        """The `with` block of a call's control_image= (None: no block): the hint on the device, one row per sample."""
        if image is None:
            return contextlib.nullcontext()
        self._check_control_allowed(what, image)
        hint = torch.as_tensor(image)
        want = tuple(8 * int(v) for v in latent_hw)
        if hint.dim() != 4 or int(hint.shape[0]) not in (1, B) or tuple(int(v) for v in hint.shape[2:]) != want:
            raise MdxError(f"{what}: control_image is {tuple(hint.shape)}, expected [{B} | 1, hint_channels, {want[0]}, {want[1]}] "
                           f"(8 x the latent)")
        hint = hint.to(self.device, torch.float32)
        if hint.shape[0] != B:
            hint = hint.expand(B, -1, -1, -1)
        return self.model.control(hint.contiguous(), scale=scale, uncond=uncond)

    def __call__(self, prompts=None, c=None, uc=None, H=512, W=512, steps=50, scale=9.0, eta=0.0, x_T=None, seed=42,
                 decode=False, gather=False, callback=None, img_callback=None, batch_size=None, per_sample_uc=False,
                 guidance_rescale=0.0, seeds=None, regions=None, control_image=None, control_scale=1.0, control_uncond=True):
        """Multi-rank runs: every rank calls with the same `prompts` list (or the same `batch_size` when rank 0 passes
        precomputed (c, uc) tensors); only rank 0's c / uc / x_T are used, the other ranks may pass None.
        seeds: one int per sample of the global batch, every rank the same list: sample b's x_T and step noise then depend on
        seeds[b] alone -- not on the batch it is served in, its row or its rank (ops.randn_seeded).  None: `seed`, one
        RandomState draw for the whole batch.
        guidance_rescale in [0, 1]: the samplers' keyword (CFG rescale for v-prediction checkpoints), every rank the same.
        steps, scale and guidance_rescale each take one value or one per sample (a list): independent requests -- "30 steps,
        scale 7.5" and "50 steps, scale 5, rescale 0.7" -- then share one UNet batch, every sample on its own schedule
        (the samplers' per-request form).  Single rank only.
        regions (a windowed pipeline, single rank): [{"prompt": ... | "c": [B | 1, T, D], "mask": m}, ...] -- regional prompts;
        m [H/8, W/8] or [H, W] in [0, 1], shared by the batch.  The call's own prompt is region 0, on 1 - max_r m_r.
        control_image / control_scale / control_uncond (a controlled pipeline, single rank): see controlled()."""
        guidance_rescale = self.check_request_lists("DiffusionPipeline", None, steps, scale, guidance_rescale)
        rank, n = D.world()
        self._check_control_allowed("DiffusionPipeline", control_image)
        self._check_regions_allowed("DiffusionPipeline", regions)
        shape = [4, H // 8, W // 8]                                   # txt2img.py:253
        if rank == 0:
            c, uc = self._encoded(prompts, c, uc, required=n == 1)
        if n > 1:
            # (the broadcast payload is sized by the UNet's capacity: for long prompts every rank calls
            # unet.set_max_context_len beforehand; broadcast_conditioning's length check is the guard)
            B = len(prompts) if prompts is not None else (int(c.shape[0]) if c is not None else batch_size)
            if B is None:
                raise MdxError("DiffusionPipeline: ranks without the conditioning tensor need prompts= or batch_size= "
                               "(the global batch) to size the broadcast")
            unet = self.model.unet
            seeds = self.check_seeds(seeds, B)
            if rank == 0:                     # the global x_T rides the one broadcast, seeded or not
                x_T = self._draw(x_T, seeds, ops.RNG_X_T, [B] + shape, seed)
            if seeds is not None:
                lo, hi = D.shard_bounds(B, rank, n)
                seeds = seeds[lo:hi]
            to_dev = lambda t: None if t is None else t.to(self.device)
            # exactly ONE collective: T, the uc form and the noise flag ride in the payload header (distributed.py)
            c, uc, x_T = D.broadcast_conditioning(
                to_dev(c) if rank == 0 else None, to_dev(uc) if rank == 0 else None, to_dev(x_T) if rank == 0 else None,
                B, (int(getattr(unet, "max_context_len", 80)), int(unet.context_dim)), shape, self.device,
                per_sample_uc=per_sample_uc)
        else:
            B = int(c.shape[0])
            self.check_request_lists("DiffusionPipeline", B, steps, scale, guidance_rescale)
            seeds = self.check_seeds(seeds, B)
            x_T = self._draw(x_T, seeds, ops.RNG_X_T, [B] + shape, seed)
            c, uc = self._on_device(c, uc, B)
            x_T = x_T.to(self.device)
        # guidance_rescale needs nothing from the batch sharding: its statistic is per sample, over that sample's C * H * W;
        # the seeds are this rank's samples': the eta > 0 step draws
        with self._region_scope("DiffusionPipeline", regions, c, uc, scale, shape[1:], (H, W)), \
                self._control_scope("DiffusionPipeline", control_image, control_scale, control_uncond, int(c.shape[0]), shape[1:]):
            samples, inter = self.sampler.sample(S=steps, conditioning=c, batch_size=int(c.shape[0]), shape=shape, verbose=False,
                                                 unconditional_guidance_scale=scale, unconditional_conditioning=uc,
                                                 eta=eta, x_T=x_T, callback=callback, img_callback=img_callback,
                                                 **self._sampler_kw(guidance_rescale, seeds))
        if decode:
            samples = self._decoded(samples)
        if gather and n > 1:
            samples = D.gather_latents(samples)
        return samples

    # ---- InstructPix2Pix editing (Brooks et al. 2023; not in the reference): "change this picture as the sentence says"
    def edit(self, image, prompts=None, c=None, uc=None, steps=50, scale=7.5, image_scale=1.5, eta=0.0, seed=42, seeds=None,
             x_T=None, guidance_rescale=0.0, output="float", decode=True, callback=None, img_callback=None):
        """Edit `image` as the instruction (prompts, or c / uc) says, on an 8-channel hybrid model (LatentEditDiffusion).

        image [B | 1, 3, H, W] in [-1, 1], H and W multiples of 8; a batch-1 image is repeated to the prompt batch.  Every model
        evaluation runs three branches -- (empty text, zero image latent), (empty text, image latent), (instruction, image
        latent) -- and the step launch combines them, e_uu + image_scale (e_ui - e_uu) + scale (e_ci - e_ui): `scale` pulls
        towards the instruction, `image_scale` towards the input picture.  c_concat = model.encode_edit_image(image), the
        posterior mode, unscaled; its unconditional counterpart is zeros.  x_T, seed / seeds, eta and guidance_rescale as in
        __call__ (scale, image_scale, steps and guidance_rescale are scalars here).  Single rank; not on a windowed, controlled
        or hires-derived pipeline.  decode False: the final latent.  Otherwise the VAE decoder (tile by tile with VAE tiling
        on, as the encode): output "float" [B, 3, H, W] in [0, 1], "uint8" [B, H, W, 3]."""
        what = "DiffusionPipeline.edit"
        if self._windowed:
            raise MdxError(f"{what}: not on a windowed pipeline (windowed edits are not built)")
        self._refuse_controlled("edit")
        if getattr(self, "_hires_derived", False):
            raise MdxError(f"{what}: not on a hires-derived pipeline (hires edits are not built)")
        if D.world()[1] > 1:
            raise MdxError(f"{what}: runs on a single rank (the sharded form is not built)")
        if output not in ("float", "uint8"):
            raise ValueError(f"{what}: output must be 'float' or 'uint8', got {output!r}")
        key = getattr(getattr(self.model, "model", None), "conditioning_key", "crossattn")
        cin = getattr(getattr(self.model, "unet", None), "in_channels", None)
        if key != "hybrid" or cin != 8 or not hasattr(self.model, "encode_edit_image"):
            raise MdxError(f"{what}: needs an InstructPix2Pix model -- 8 input channels under conditioning_key 'hybrid' "
                           f"(LatentEditDiffusion, configs.WUKONG_EDIT_UNET); this one has {cin} input channels under {key!r}")
        for name, v in (("steps", steps), ("scale", scale), ("image_scale", image_scale), ("guidance_rescale", guidance_rescale)):
            if as_sequence(v) is not None:
                raise MdxError(f"{what}: {name} is one value for the batch (per-request lists do not run with image guidance)")
        guidance_rescale = check_guidance_rescale(guidance_rescale)
        if not (isinstance(image, torch.Tensor) and image.dim() == 4 and image.shape[1] == 3):
            raise MdxError(f"{what}: image must be a tensor [B | 1, 3, H, W] in [-1, 1]")
        H, W = int(image.shape[2]), int(image.shape[3])
        if H % 8 or W % 8 or H < 8 or W < 8:
            raise MdxError(f"{what}: the image's H and W must be positive multiples of 8, got {H} x {W}")
        c, uc = self._encoded(prompts, c, uc)
        if uc is None:
            raise MdxError(f"{what}: needs the unconditional context uc (the empty prompt's encoding) with c")
        B = int(c.shape[0])
        if int(image.shape[0]) not in (1, B):
            raise MdxError(f"{what}: {int(image.shape[0])} images for a batch of {B} (1 or the batch)")
        seeds = self.check_seeds(seeds, B)
        c, uc = self._on_device(c, uc, B)
        image = image.to(device=self.device, dtype=torch.float32)
        c_cat = self.model.encode_edit_image(image.contiguous())      # (a batch-1 image is encoded once)
        if c_cat.shape[0] != B:
            c_cat = c_cat.expand(B, -1, -1, -1).contiguous()
        lat = tuple(c_cat.shape)
        x_T = self._draw(x_T, seeds, ops.RNG_X_T, list(lat), seed)
        cond = {"c_concat": c_cat, "c_crossattn": c}
        uc_full = {"c_concat": torch.zeros_like(c_cat), "c_crossattn": uc}
        samples = self.sampler.sample(S=steps, conditioning=cond, batch_size=B, shape=list(lat[1:]), verbose=False, eta=eta,
                                      x_T=x_T.to(self.device), unconditional_guidance_scale=scale,
                                      unconditional_conditioning=uc_full, callback=callback, img_callback=img_callback,
                                      image_guidance_scale=image_scale, **self._sampler_kw(guidance_rescale, seeds))[0]
        if not decode:
            return samples
        if output == "float":
            return self._decoded(samples)
        return ops.inpaint_composite(self._decode_latent(samples).to(torch.float32).contiguous(), None, None, output="uint8")

    # ---- large canvases (ldm/models/diffusion/windowed.py): the UNet evaluated in overlapping windows of the trained size
    def windowed(self, window=512, stride=None, weights=None, max_unet_batch=16, wrap_x=False, seam_pad=64):
        """A new DiffusionPipeline on WindowedDiffusion(self.model, ...): the same sampler kind and device, all weights
        shared.  On it __call__(..., H=512, W=2048), img2img, inpaint, session(H=, W=) and serve run as they do here, the UNet
        evaluated per step on overlapping windows of the canvas and averaged where they overlap.  window / stride: IMAGE
        pixels, ints or (H, W) pairs, multiples of 8 (stride None: half the window); weights: None or [window / 8] positive
        latent-pixel weights (windowed.gaussian_weights); max_unet_batch: the largest UNet batch one chunk of windows makes.
        wrap_x: the windows wrap around the right edge of the canvas into the left one (a 360-degree panorama); decoding then
        pads the latent circularly by seam_pad IMAGE pixels (a multiple of 8; 0: the plain decode) per side and crops them.
        The new pipeline's __call__, img2img and inpaint take regions= (regional prompts)."""
        from .ldm.models.diffusion.windowed import WindowedDiffusion, _pair
        self._refuse_controlled("windowed")

        def latent(v, name):
            if v is None:
                return None
            a, b = _pair(v, name)
            if a < 8 or b < 8 or a % 8 or b % 8:
                raise MdxError(f"DiffusionPipeline.windowed: {name} is in image pixels, positive multiples of 8, got {v!r}")
            return a // 8, b // 8
        try:
            kind = self._session_sampler()
        except MdxError:
            raise MdxError(f"DiffusionPipeline.windowed: the new pipeline gets a sampler of this one's kind, 'ddim', 'plms' or "
                           f"'dpm_solver' / 'uni_pc'; this one's is a {type(self.sampler).__name__}") from None
        if isinstance(seam_pad, bool) or not isinstance(seam_pad, (int, np.integer)) or seam_pad < 0 or seam_pad % 8:
            raise MdxError(f"DiffusionPipeline.windowed: seam_pad is in image pixels, a multiple of 8 >= 0, got {seam_pad!r}")
        model = WindowedDiffusion(self.model, latent(window, "window"), latent(stride, "stride"), weights, max_unet_batch,
                                  wrap_x=wrap_x)
        pipe = DiffusionPipeline(model, kind, self.device, solver=self._solver())
        pipe.seam_cols = int(seam_pad) // 8 if wrap_x else 0
        return pipe

    # ---- continuous batching (ldm/models/diffusion/session.py): requests join and leave a running UNet batch
    def _session_sampler(self):
        from .ldm.models.diffusion.dpm_solver import DPMSolverSampler
        from .ldm.models.diffusion.uni_pc import UniPCSampler
        for cls, name in ((DPMSolverSampler, "dpm_solver"), (UniPCSampler, "uni_pc"), (PLMSSampler, "plms"), (DDIMSampler, "ddim")):
            if isinstance(self.sampler, cls):
                return name
        raise MdxError(f"DiffusionPipeline.session: pass sampler='ddim' or 'dpm_solver' (the pipeline's sampler is a "
                       f"{type(self.sampler).__name__})")

    def session(self, slots=4, H=512, W=512, sampler=None, context_len=WINDOW, max_steps=50, temperature=1.0,
                noise_dropout=0.0, empty=None, sample_posterior=True):
        """A SamplingSession on this pipeline's model: `slots` samples of one latent shape whose requests come and go
        (submit / step / run_until_idle).  sampler: 'ddim' or 'dpm_solver' (default: the pipeline's; PLMS is refused).
        sample_posterior: whether submit(init_image=) requests sample the VAE posterior or take its mode."""
        from .ldm.models.diffusion.session import SamplingSession
        self._refuse_controlled("session")
        if (sampler or self._session_sampler()) == "uni_pc":
            raise MdxError("DiffusionPipeline.session: a session's slots step through the slot kernels, whose rows hold the DDIM "
                           "and the DPM-Solver++ 2M update: UniPC has no rows there (pass sampler='ddim' or 'dpm_solver')")
        if (sampler or self._session_sampler()) == "dpm_solver" and not self._unipc and self._solver():
            raise ValueError(f"DiffusionPipeline.session: a session's slots step through the slot kernels, whose rows hold the "
                             f"multistep order-2 DPM-Solver update only: not with the solver options "
                             f"{', '.join(sorted(self._solver()))} (pass sampler='ddim', or use a pipeline without solver=)")
        return SamplingSession(self.model, slots, H=H, W=W, sampler=sampler or self._session_sampler(),
                               context_len=context_len, max_steps=max_steps, temperature=temperature,
                               noise_dropout=noise_dropout, device=self.device, empty=empty, sample_posterior=sample_posterior)

    def serve(self, requests, slots=4, H=512, W=512, output="float", sampler=None, temperature=1.0, noise_dropout=0.0,
              empty=None):
        """Drain a list of requests -- dicts of SamplingSession.submit's keywords, the img2img ones (init_latent / init_image,
        strength, keep_mask) included -- through one session of `slots` slots;
        the results come back in REQUEST order, whatever order they finished in.  output: 'latent' [N, 4, H/8, W/8]; 'float'
        [N, 3, H, W] in [0, 1], what __call__(decode=True) returns; 'uint8' [N, H, W, 3], truncated as inpaint.py:112-115."""
        self._refuse_controlled("serve")
        if output not in ("latent", "float", "uint8"):
            raise ValueError("output must be 'latent', 'float' or 'uint8'")
        requests = list(requests)
        if not requests:
            raise MdxError("DiffusionPipeline.serve: no requests")
        lens = [int(r[k].shape[-2]) for r in requests for k in ("c", "uc") if isinstance(r.get(k), torch.Tensor)]
        if not lens or any(r.get("prompt") is not None for r in requests):
            lens.append(WINDOW)
        max_steps = max([int(r["steps"]) for r in requests if isinstance(r.get("steps"), (int, np.integer))] + [30])
        sess = self.session(slots, H, W, sampler, max(lens), max_steps, temperature, noise_dropout, empty)
        handles = [sess.submit(**r) for r in requests]
        sess.run_until_idle()
        self.last_session = sess
        latents = torch.stack([h.latent for h in handles])
        if output == "latent":
            return latents
        images = torch.cat([self._decoded(latents[i:i + slots]) for i in range(0, len(handles), slots)])
        if output == "float":
            return images
        return (images * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def img2img(self, init_image=None, init_latent=None, strength=0.75, prompts=None, c=None, uc=None, steps=50, scale=9.0,
                eta=0.0, seed=42, noise=None, post_noise=None, sample_posterior=True, mask=None, decode=False, callback=None,
                img_callback=None, guidance_rescale=0.0, seeds=None, regions=None, control_image=None, control_scale=1.0,
                control_uncond=True):
        """Start from an image instead of pure noise: encode it, noise the latent to the level `strength` selects, and run only
        the remaining t_enc = int(strength * steps) of the `steps`-step schedule (strength 1: all of them).

        init_image [B, 3, H, W] in [-1, 1] (needs model.first_stage_model with an encoder) or init_latent [B, C, h, w]
        (already scaled by model.scale_factor): exactly one of them.  noise / post_noise: the N(0, 1) draws of the forward
        process and of the VAE posterior at the latent's shape; None = numpy RandomState(seed) / RandomState(seed + 1), as
        start_noise().  sample_posterior False: the posterior's mode.  mask [B, 1, h, w] at latent resolution, 1 = keep the
        init image there (PLMS / DDIM only).  Conditioning, decode and guidance_rescale as in __call__.  Single rank only.
        seeds: one int per sample; the forward noise (ops.RNG_ENCODE), the posterior noise (ops.RNG_POSTERIOR) and the step and
        blend draws of sample b then depend on seeds[b] alone.  A passed noise / post_noise still wins.
        scale and guidance_rescale each take one value or one per sample; steps is one int (`strength` fixes one grid).
        regions: regional prompts on a windowed pipeline, as in __call__ (masks at the latent's or the init image's size).
        control_image / control_scale / control_uncond: ControlNet on a controlled pipeline, as in __call__ (the hint at 8 x the
        latent's size)."""
        guidance_rescale = self.check_request_lists("img2img", None, steps, scale, guidance_rescale, steps_list=False)
        self._check_regions_allowed("img2img", regions)
        self._check_control_allowed("img2img", control_image)
        if (init_image is None) == (init_latent is None):
            raise ValueError("img2img: pass exactly one of init_image and init_latent")
        t_enc = check_strength("img2img", strength, steps)
        if D.world()[1] > 1:
            raise MdxError("img2img runs on a single rank (the sharded form is not built)")
        if mask is not None and self._dpm:
            raise NotImplementedError("img2img: mask blending is implemented by PLMSSampler / DDIMSampler")
        c, uc = self._encoded(prompts, c, uc)
        B = int(c.shape[0])
        self.check_request_lists("img2img", B, steps, scale, guidance_rescale, steps_list=False)
        seeds = self.check_seeds(seeds, B)
        c, uc = self._on_device(c, uc, B)
        start, a, b = self._partial_start(steps, t_enc, eta)
        if init_image is not None:
            vae = self.model.first_stage_model
            if vae is None or not hasattr(vae, "encode_noised"):
                raise MdxError("img2img(init_image=) needs a VAE with an encoder attached (model.first_stage_model)")
            x = init_image.to(device=self.device, dtype=torch.float32)
            shape = vae.latent_shape(x.shape)                         # the encoder's output size, not H // 8
            if seeds is not None and x.shape[0] != B:
                raise MdxError(f"img2img: {x.shape[0]} init images but {B} conditionings")
            z0, x_enc = vae.encode_noised(x, self.model.scale_factor, a, b, self._draw(noise, seeds, ops.RNG_ENCODE, shape, seed),
                                          post_noise=(self._draw(post_noise, seeds, ops.RNG_POSTERIOR, shape, seed + 1)
                                                      if sample_posterior else None),
                                          sample=sample_posterior)
        else:
            z0 = init_latent.to(device=self.device, dtype=torch.float32).contiguous()
            if seeds is not None and z0.shape[0] != B:
                raise MdxError(f"img2img: {z0.shape[0]} init images but {B} conditionings")
            x_enc = self.sampler.stochastic_encode(z0, start, noise=self._draw(noise, seeds, ops.RNG_ENCODE, z0.shape, seed))
        if z0.shape[0] != B:
            raise MdxError(f"img2img: {z0.shape[0]} init images but {B} conditionings")
        image_hw = tuple(init_image.shape[2:]) if init_image is not None else tuple(8 * int(v) for v in z0.shape[2:])
        with self._region_scope("img2img", regions, c, uc, scale, z0.shape[2:], image_hw), \
                self._control_scope("img2img", control_image, control_scale, control_uncond, B, z0.shape[2:]):
            samples = self._run_partial(x_enc, c, uc, start, t_enc, scale, callback, img_callback,
                                        self._sampler_kw(guidance_rescale, seeds), mask=mask, x0=z0)
        return self._decoded(samples) if decode else samples

    # ---- hires fix: sample at the trained size, enlarge, re-sample the end of the schedule at the target size
    HIRES_UPSCALERS = {"latent-nearest": "nearest", "latent-bilinear": "bilinear", "latent-bicubic": "bicubic",
                       "image-bicubic": "bicubic", "image-lanczos3": "lanczos3"}

    @property
    def _windowed(self):
        from .ldm.models.diffusion.windowed import WindowedDiffusion
        return isinstance(self.model, WindowedDiffusion)

    def upscale_latent(self, z, H, W, mode="bicubic"):
        """z [B, C, h, w] resampled to the latent grid of an H x W image, [B, C, H / 8, W / 8]: one ops.resample launch.  On a
        wrap_x pipeline the columns wrap around, so a panorama still closes."""
        if H % 8 or W % 8 or H < 8 or W < 8:
            raise MdxError(f"upscale_latent: H and W are in image pixels, positive multiples of 8, got {H!r} x {W!r}")
        z = z.to(device=self.device, dtype=torch.float32).contiguous()
        return ops.resample(z, (H // 8, W // 8), mode, wrap_x=bool(getattr(self.model, "wrap_x", False)))

    def _hires_pipelines(self, H, W, base, second):
        """(first, second): the pipeline of the first pass -- this one, or on a windowed pipeline one on its inner, un-windowed
        model -- and of the second: `second` when given, this one when the target is the base size or this one is windowed,
        else self.windowed(window=base), built once per base and kept so that its plans survive."""
        kept = self._hires_kept
        first = self
        if self._windowed:
            if "inner" not in kept:
                kept["inner"] = DiffusionPipeline(self.model.inner, self._session_sampler(), self.device, solver=self._solver())
                kept["inner"]._hires_derived = True
            first = kept["inner"]
        if second is None:
            if (H, W) == base or self._windowed:
                second = self
            else:
                if base not in kept:
                    kept[base] = self.windowed(window=base)
                    kept[base]._hires_derived = True
                second = kept[base]
        return first, second

    def hires(self, prompts=None, c=None, uc=None, H=1024, W=1024, base=(512, 512), upscaler="latent-bicubic", strength=0.6,
              steps=50, hires_steps=None, scale=9.0, eta=0.0, seed=42, seeds=None, guidance_rescale=0.0, second=None,
              decode=False, return_base=False, regions=None):
        """Hires fix: a full `steps`-step run at base = (H0, W0), where the checkpoint composes well; the result enlarged to
        H x W; and the last t_enc = int(strength * (hires_steps or steps)) steps of the schedule run again at the target size.

        First pass: exactly self(..., H=base[0], W=base[1], steps=steps, ...); on a windowed pipeline it runs on the inner,
        un-windowed model.  upscaler: "latent-nearest" / "latent-bilinear" / "latent-bicubic" resample the latent
        (ops.resample; with seeds one fused ops.resample_noised launch that also noises it, stream ops.RNG_ENCODE, draw 0 at the
        new shape -- what img2img(init_latent=, seeds=) draws); "image-bicubic" / "image-lanczos3" decode, clamp to [-1, 1],
        resample the image and encode it as img2img(init_image=) does; a callable img [B, 3, h, w] in [-1, 1] ->
        [B, 3, H', W'] (an SRGAN.sr_handle, anything else) takes the resample's place.  Second pass: on `second` -- default: this
        pipeline when (H, W) == base or it is windowed, else self.windowed(window=base), built once and kept -- through the same
        partial-run path as img2img, so samplers, v-prediction, guidance rescale, scale / guidance_rescale lists and seeds all
        carry over; on a wrap_x second pipeline the upscale wraps around too.  regions: regional prompts of the second pass.
        return_base: (result, first-pass latent).  Single rank; the hybrid (9-channel) model is refused."""
        self._refuse_controlled("hires")
        guidance_rescale = self.check_request_lists("hires", None, steps, scale, guidance_rescale, steps_list=False)
        if hires_steps is not None and (isinstance(hires_steps, bool) or not isinstance(hires_steps, (int, np.integer))
                                        or hires_steps < 1):
            raise ValueError(f"hires: hires_steps must be a positive int or None, got {hires_steps!r}")
        hsteps = int(steps if hires_steps is None else hires_steps)
        check_strength("hires", strength, hsteps)
        if D.world()[1] > 1:
            raise MdxError("hires runs on a single rank (the sharded form is not built)")
        try:
            base = (int(base[0]), int(base[1]))
        except (TypeError, IndexError, ValueError):
            raise MdxError(f"hires: base is an (H, W) pair in image pixels, got {base!r}") from None
        if any(v < 8 or v % 8 for v in (H, W) + base):
            raise MdxError(f"hires: H, W and base are in image pixels, positive multiples of 8, got {H!r} x {W!r}, base {base!r}")
        if getattr(getattr(self.model, "model", None), "conditioning_key", "crossattn") == "hybrid":
            raise MdxError("hires: the hybrid (9-channel) inpainting model is not supported (inpaint() is its entry point)")
        if not callable(upscaler) and upscaler not in self.HIRES_UPSCALERS:
            raise ValueError(f"hires: upscaler must be one of {sorted(self.HIRES_UPSCALERS)} or a callable, got {upscaler!r}")
        first, second = self._hires_pipelines(H, W, base, second)
        second._check_regions_allowed("hires", regions)
        c, uc = self._encoded(prompts, c, uc)
        z_base = first(c=c, uc=uc, H=base[0], W=base[1], steps=steps, scale=scale, eta=eta, seed=seed, seeds=seeds,
                       guidance_rescale=guidance_rescale)
        wrap = bool(getattr(second.model, "wrap_x", False))
        kw = dict(strength=strength, c=c, uc=uc, steps=hsteps, scale=scale, eta=eta, seed=seed, seeds=seeds,
                  guidance_rescale=guidance_rescale, regions=regions, decode=decode)
        if callable(upscaler) or upscaler.startswith("image-"):
            img = torch.clamp(self.model.decode_first_stage(z_base).to(torch.float32), -1.0, 1.0).contiguous()
            f = int(img.shape[-1]) // int(z_base.shape[-1])           # (the VAE's own factor: 8 for SD)
            size = (H // 8 * f, W // 8 * f)
            if callable(upscaler):
                big = upscaler(img)
                if not (isinstance(big, torch.Tensor) and tuple(big.shape) == tuple(img.shape[:2]) + size):
                    raise MdxError(f"hires: the upscaler returned {tuple(getattr(big, 'shape', ()))}, expected "
                                   f"{tuple(img.shape[:2]) + size}")
            else:
                big = ops.resample(img, size, self.HIRES_UPSCALERS[upscaler], wrap_x=wrap)
            out = second.img2img(init_image=big, **kw)
        elif seeds is None:
            z_up = ops.resample(z_base, (H // 8, W // 8), self.HIRES_UPSCALERS[upscaler], wrap_x=wrap)
            out = second.img2img(init_latent=z_up, **kw)
        else:
            out = second._hires_seeded(z_base, (H, W), self.HIRES_UPSCALERS[upscaler], wrap, strength, c, uc, hsteps, scale, eta,
                                       seeds, guidance_rescale, regions, decode)
        return (out, z_base) if return_base else out

    def _hires_seeded(self, z_base, hw, mode, wrap, strength, c, uc, steps, scale, eta, seeds, guidance_rescale, regions, decode):
        """img2img(init_latent=resample(z_base), seeds=) with the resample, the seeded draw and the q-sample as ONE launch
        (ops.resample_noised): the same bits, two launches fewer, and neither the enlarged latent nor the noise is stored (no
        mask blends here, so the start latent is all the run needs)."""
        t_enc = check_strength("hires", strength, steps)
        B = int(c.shape[0])
        self.check_request_lists("hires", B, steps, scale, guidance_rescale, steps_list=False)
        seeds = self.check_seeds(seeds, B)
        if z_base.shape[0] != B:
            raise MdxError(f"hires: {z_base.shape[0]} first-pass latents but {B} conditionings")
        c, uc = self._on_device(c, uc, B)
        start, a, b = self._partial_start(steps, t_enc, eta)
        latent_hw = (hw[0] // 8, hw[1] // 8)
        _, x_enc = ops.resample_noised(z_base, latent_hw, a, b, seeds=ops.seeds_tensor(seeds, self.device), stream=ops.RNG_ENCODE,
                                       draw=0, mode=mode, wrap_x=wrap, z0_out=False)
        with self._region_scope("hires", regions, c, uc, scale, latent_hw, hw):
            samples = self._run_partial(x_enc, c, uc, start, t_enc, scale, None, None, self._sampler_kw(guidance_rescale, seeds))
        return self._decoded(samples) if decode else samples

    # ---- inpainting: wukong-huahua/inpaint.py, image and mask in, composited image out
    @staticmethod
    def _check_inpaint_inputs(image, mask, batch=None):
        """image [B | 1, 3, H, W], mask [B | 1, 1, H, W] of one size; returns the batch they imply (`batch` when given)."""
        if not (isinstance(image, torch.Tensor) and image.dim() == 4):
            raise MdxError("inpaint: image must be a tensor [B, 3, H, W] in [-1, 1]")
        if not (isinstance(mask, torch.Tensor) and mask.dim() == 4 and mask.shape[1] == 1):
            raise MdxError("inpaint: mask must be a tensor [B, 1, H, W] (>= 0.5 = repaint)")
        if tuple(mask.shape[2:]) != tuple(image.shape[2:]):
            raise MdxError(f"inpaint: mask is {tuple(mask.shape[2:])}, image {tuple(image.shape[2:])}")
        bi, bm = int(image.shape[0]), int(mask.shape[0])
        B = max(bi, bm) if batch is None else int(batch)
        if bi not in (1, B) or bm not in (1, B):
            raise MdxError(f"inpaint: {bi} images and {bm} masks for a batch of {B} (each must be 1 or the batch)")
        return B

    def _inpaint_to_device(self, image, mask, B):
        """fp32 on the device; a batch-1 image is repeated (make_batch_sd, inpaint.py:57-62), a batch-1 mask stays one plane
        (the kernels share it).  The mask is binarised where it arrives, as make_batch_sd does on the host (inpaint.py:51-52)."""
        image = image.to(device=self.device, dtype=torch.float32)
        if image.shape[0] != B:
            image = image.expand(B, -1, -1, -1)
        mask = (mask >= 0.5).to(torch.float32).to(self.device)
        return image.contiguous(), mask.contiguous()

    def _inpaint_vae(self):
        vae = getattr(self.model, "first_stage_model", None)
        if vae is None or not hasattr(vae, "encode_concat"):
            raise MdxError("inpaint needs a VAE with an encoder attached (model.first_stage_model)")
        return vae

    def inpaint_conditioning(self, image, mask, post_noise=None, sample_posterior=True, seed=42, seeds=None, batch_size=None):
        """c_concat [B, 5, h, w] of the hybrid (9-channel) UNet as inpaint.py:76-85 builds it: cat(mask at the latent grid,
        scale_factor * encode(image * (mask < 0.5))).  Three steps on the device: the masked-image launch, the VAE encoder, the
        concat launch.  image [B | 1, 3, H, W] in [-1, 1]; mask [B | 1, 1, H, W], >= 0.5 = repaint.  The posterior draw:
        post_noise [B, 4, h, w], else per sample from `seeds` (ops.RNG_POSTERIOR), else RandomState(seed + 1) as img2img;
        sample_posterior False: the mode.  batch_size: the batch to repeat batch-1 inputs to (default: what the inputs imply)."""
        vae = self._inpaint_vae()
        if batch_size is None and seeds is not None:
            batch_size = len(seeds)
        B = self._check_inpaint_inputs(image, mask, batch_size)
        seeds = self.check_seeds(seeds, B)
        image, mask = self._inpaint_to_device(image, mask, B)
        return self._inpaint_c_concat(vae, image, mask, post_noise, sample_posterior, seeds, seed)[0]

    def _inpaint_c_concat(self, vae, image, mask, post_noise, sample_posterior, seeds, seed):
        """image / mask as _inpaint_to_device leaves them: the posterior draw (None for the mode), one masked-image launch, the
        encoder, one concat launch.  Returns (c_concat, the posterior draw)."""
        post = None
        if sample_posterior:                                          # (the encoder's output size, not H // 8)
            post = self._draw(post_noise, seeds, ops.RNG_POSTERIOR, vae.latent_shape(image.shape), seed + 1)
        masked = ops.inpaint_mask_image(image, mask)
        return vae.encode_concat(masked, mask, self.model.scale_factor, post_noise=post, sample=sample_posterior), post

    def inpaint(self, image, mask, prompts=None, c=None, uc=None, steps=30, scale=7.5, eta=0.0, strength=1.0, seed=42,
                seeds=None, x_T=None, noise=None, post_noise=None, sample_posterior=True, mask_blur=0.0, composite=True,
                decode=True, output="float", guidance_rescale=0.0, callback=None, img_callback=None, regions=None):
        """Repaint the masked region of an image (wukong-huahua/inpaint.py:65-117; its CLI defaults: PLMS, 30 steps, scale 7.5).

        image [B | 1, 3, H, W] in [-1, 1]; mask [B | 1, 1, H, W], >= 0.5 = repaint; batch-1 inputs are repeated to the
        conditioning's batch.  Conditioning (prompts, or c / uc), guidance_rescale and seeds as in img2img.  Single rank only.
        A hybrid model (LatentInpaintDiffusion, 9 input channels) follows the reference: c_concat = inpaint_conditioning(),
        the same c_concat in the conditional and the unconditional dict, x_T = start_noise(B, shape, seed) (ops.RNG_X_T with
        seeds), a full `steps`-step run.  strength < 1 starts instead from the encoded unmasked image noised to the level
        int(strength * steps) selects, as img2img (noise: the forward draw).  A plain 4-channel model takes the blend path:
        img2img(init_image=image, mask=1 - mask at the latent grid) (PLMS / DDIM only).
        decode False: the final latent.  Otherwise the VAE decoder and ONE output launch: with composite, the original image
        is kept outside the mask, alpha * decoded + (1 - alpha) * image with alpha = the binarised mask, or with mask_blur
        (a Gaussian sigma in pixels, > 0) alpha = max(m, G * m) -- the mask widened outward, exactly 1 on the hole; composite
        False returns the decoder's picture as the reference does.  output "float": [B, 3, H, W] in [0, 1]; "uint8":
        [B, H, W, 3], (uint8)(255 v) as inpaint.py:112-115.
        scale and guidance_rescale each take one value or one per sample; steps is one int, as in img2img.
        regions: regional prompts on a windowed pipeline, as in __call__ (masks at the latent's or the image's size)."""
        guidance_rescale = self.check_request_lists("inpaint", None, steps, scale, guidance_rescale, steps_list=False)
        self._check_regions_allowed("inpaint", regions)
        if output not in ("float", "uint8"):
            raise ValueError(f"inpaint: output must be 'float' or 'uint8', got {output!r}")
        t_enc = check_strength("inpaint", strength, steps)
        mask_blur = float(mask_blur)
        if not mask_blur >= 0.0:
            raise ValueError(f"inpaint: mask_blur must be >= 0, got {mask_blur!r}")
        if mask_blur > 0.0:
            ops.feather_weights(mask_blur)                            # (the radius cap, before any work)
        if D.world()[1] > 1:
            raise MdxError("inpaint runs on a single rank (the sharded form is not built)")
        c, uc = self._encoded(prompts, c, uc)
        B = int(c.shape[0])
        self.check_request_lists("inpaint", B, steps, scale, guidance_rescale, steps_list=False)
        seeds = self.check_seeds(seeds, B)
        try:
            self._check_inpaint_inputs(image, mask, B)
        except MdxError as e:
            raise MdxError(f"{e} -- the batch is the conditioning's, {B}") from None
        hybrid = getattr(getattr(self.model, "model", None), "conditioning_key", "crossattn") == "hybrid"
        if not hybrid and self._dpm:
            raise NotImplementedError("inpaint with a 4-channel model blends under the mask every step: implemented by "
                                      "PLMSSampler / DDIMSampler")
        vae = self._inpaint_vae()
        image, mask = self._inpaint_to_device(image, mask, B)
        if not hybrid:
            # the blend path: img2img's mask means KEEP
            keep = 1.0 - ops.inpaint_resize_mask(mask, vae.latent_shape(image.shape)[2:])
            samples = self.img2img(init_image=image, strength=strength, c=c, uc=uc, steps=steps, scale=scale, eta=eta, seed=seed,
                                   noise=noise, post_noise=post_noise, sample_posterior=sample_posterior, mask=keep,
                                   callback=callback, img_callback=img_callback, guidance_rescale=guidance_rescale, seeds=seeds,
                                   regions=regions)
        else:
            c, uc = self._on_device(c, uc, B)
            lat = vae.latent_shape(image.shape)
            c_cat, post = self._inpaint_c_concat(vae, image, mask, post_noise, sample_posterior, seeds, seed)
            cond = {"c_concat": c_cat, "c_crossattn": c}                  # inpaint.py:88
            uc_full = None if uc is None else {"c_concat": c_cat, "c_crossattn": uc}      # inpaint.py:91-92
            kw = self._sampler_kw(guidance_rescale, seeds)
            scope = self._region_scope("inpaint", regions, c, uc, scale, lat[2:], image.shape[2:])
            if t_enc == steps:
                # the reference's run (strength 1): pure noise, every step; neither mask nor x0 goes to the sampler (inpaint.py's
                # x0= without a mask is inert)
                x_T = self._draw(x_T, seeds, ops.RNG_X_T, lat, seed)
                with scope:
                    samples = self.sampler.sample(S=steps, conditioning=cond, batch_size=B, shape=list(lat[1:]), verbose=False,
                                                  eta=eta, x_T=x_T.to(self.device), unconditional_guidance_scale=scale,
                                                  unconditional_conditioning=uc_full, callback=callback,
                                                  img_callback=img_callback, **kw)[0]
            else:
                # strength < 1: start from the (unmasked) image's own latent, noised to where the last t_enc steps begin -- img2img
                start, a, b = self._partial_start(steps, t_enc, eta)
                _, x_enc = vae.encode_noised(image, self.model.scale_factor, a, b,
                                             self._draw(noise, seeds, ops.RNG_ENCODE, lat, seed), post_noise=post,
                                             sample=sample_posterior)
                with scope:
                    samples = self._run_partial(x_enc, cond, uc_full, start, t_enc, scale, callback, img_callback, kw)
        if not decode:
            return samples
        x = self._decode_latent(samples).to(torch.float32).contiguous()
        alpha = None
        if composite:
            alpha = ops.mask_feather(mask, mask_blur) if mask_blur > 0.0 else mask
        return ops.inpaint_composite(x, image if composite else None, alpha, output=output)
