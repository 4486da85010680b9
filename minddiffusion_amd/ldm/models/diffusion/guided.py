"""What PLMSSampler, DDIMSampler and DPMSolverSampler do before and inside their loops in the same way: the conditioning a
caller may hand over (split_conditioning), the start latent and the other draws of a run with the checks of their sources
(start_latent, check_seed_sources / check_seeds, noised_latent, _Draws; check_guidance_rescale), and the model call of one step
on the classifier-free-guidance batch (use_cfg, GuidedModel).  Which launches a run makes with which scalars is schedule.py's."""
import os

import numpy as np
import torch

from .... import ops
from ...._lib import MdxError


def _first_tensor(c):
    while isinstance(c, (dict, list, tuple)):
        c = c[list(c.keys())[0]] if isinstance(c, dict) else c[0]
    return c


def split_conditioning(model, cond, uc, x_T=None):
    """(cond, uc, c_cat, uc_cat, device) from what sample() was given, bare or as a dict, by the DiffusionWrapper key of the
    model (WK ddpm.py:361-374), handed over the way plms.py:188-195 does it: a bare conditioning goes to the keyword the key
    reads -- 'crossattn': the text context; 'concat': extra input channels (cond and uncond halves may differ); 'adm': class
    labels [B] (concatenated [uncond; cond] like a text context); None: no conditioning at all.
    Hybrid (inpainting) conditioning is {"c_concat": mask + masked-image latent, "c_crossattn": text} (inpaint.py:84-88, WK
    plms.py:188-205).  WK plms.py:191-201 concatenates [uncond[k]; cond[k]] for EVERY dict key: an unconditional c_concat that
    differs from the conditional one goes into the unconditional half (inpaint.py passes the same tensor in both)."""
    key = getattr(getattr(model, "model", None), "conditioning_key", "crossattn")
    c_cat = uc_cat = None
    if key == "concat":
        c_cat = _first_tensor(cond["c_concat"] if isinstance(cond, dict) else cond)
        if uc is not None:
            uc_cat = _first_tensor(uc["c_concat"] if isinstance(uc, dict) else uc)
        cond = uc = None
    elif isinstance(cond, dict) and "c_concat" in cond:
        c_cat = _first_tensor(cond["c_concat"])
        cond = cond["c_crossattn"]
        if isinstance(uc, dict):
            if uc.get("c_concat") is not None:
                uc_cat = _first_tensor(uc["c_concat"])
            uc = uc["c_crossattn"]
    if key is None:
        cond = uc = None
    cond = _first_tensor(cond) if cond is not None else None
    uc = _first_tensor(uc) if uc is not None else None
    if key in ("crossattn", "hybrid") and not (isinstance(cond, torch.Tensor) and cond.is_cuda):
        raise MdxError("conditioning must be a CUDA(HIP) tensor [B, T, context_dim]")
    if key == "adm" and cond is None:
        raise MdxError("'adm' conditioning needs the class labels [B] as `conditioning`")
    if key == "concat" and c_cat is None:
        raise MdxError("'concat' conditioning needs the extra input channels [B, C', H, W] as `conditioning`")
    if isinstance(cond, torch.Tensor) and cond.is_cuda:
        dev = cond.device
    elif isinstance(c_cat, torch.Tensor) and c_cat.is_cuda:
        dev = c_cat.device
    elif isinstance(x_T, torch.Tensor) and x_T.is_cuda:
        dev = x_T.device
    else:
        dev = model.unet.device
    if cond is not None:
        cond = torch.as_tensor(cond).to(dev)
        uc = None if uc is None else torch.as_tensor(uc).to(dev)
    return cond, uc, c_cat, uc_cat, dev


def start_latent(x_T, seeds, size, dev, generator):
    """The latent a run starts from, [B, C, H, W] fp32: a copy of x_T, else one ops.randn_seeded launch from the per-sample
    `seeds` (stream ops.RNG_X_T, draw 0), else the sampler's generator."""
    if x_T is None and seeds is not None:
        return ops.randn_seeded(seeds, ops.RNG_X_T, 0, tuple(size[1:]))
    if x_T is None:
        return torch.randn(size, device=dev, dtype=torch.float32, generator=generator)
    return torch.as_tensor(x_T).to(device=dev, dtype=torch.float32).contiguous().clone()


def check_guidance_rescale(value):
    """`guidance_rescale` (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", 3.4) as a float in
    [0, 1]; anything else, NaN included, is a ValueError."""
    phi = float(value)
    if not 0. <= phi <= 1.:
        raise ValueError(f"guidance_rescale must be in [0, 1], got {value!r}")
    return phi


def check_image_guidance(what, model, image_scale, cond, uc, per, mask=None, x0=None):
    """`image_guidance_scale` of the samplers (three-branch guidance, InstructPix2Pix): None stays None; otherwise the float,
    after every refusal the three samplers share -- what the run needs (dict conditioning on both sides with a c_concat each,
    a scalar guidance scale) and what it does not combine with.  per: schedule.per_request's result."""
    if image_scale is None:
        return None
    from .... import distributed as D
    from .windowed import WindowedDiffusion
    if isinstance(image_scale, bool) or np.ndim(image_scale) != 0:
        raise MdxError(f"{what}: image_guidance_scale is one float for the batch (per-request image scales are not built), "
                       f"got {image_scale!r}")
    s = float(image_scale)
    if not np.isfinite(s):
        raise ValueError(f"{what}: image_guidance_scale must be finite, got {image_scale!r}")
    if per is not None:
        raise MdxError(f"{what}: image_guidance_scale does not run with per-request lists of S, "
                       "unconditional_guidance_scale or guidance_rescale (the step table has no middle branch)")
    if mask is not None or x0 is not None:
        raise MdxError(f"{what}: image_guidance_scale does not run with mask= / x0=")
    if isinstance(model, WindowedDiffusion):
        raise MdxError(f"{what}: image_guidance_scale does not run on a WindowedDiffusion model")
    if getattr(model, "is_controlled", False):
        raise MdxError(f"{what}: image_guidance_scale does not run on a ControlledDiffusion model")
    if D.world()[1] > 1:
        raise MdxError(f"{what}: image_guidance_scale runs on a single rank (several ranks are not built)")
    for name, c in (("conditioning", cond), ("unconditional_conditioning", uc)):
        if not isinstance(c, dict):
            raise MdxError(f"{what}: image_guidance_scale needs {name} as a dict with 'c_concat' and 'c_crossattn'")
        for k in ("c_concat", "c_crossattn"):
            if c.get(k) is None:
                raise MdxError(f"{what}: image_guidance_scale needs {name}['{k}']")
    return s


def check_seed_sources(seeds, generator=None, **injected):
    """A second source for the draws that `seeds=` covers -- the sampler's generator, or one of the test-injection keywords -- is a
    caller's mistake: ValueError."""
    if seeds is None:
        return
    if generator is not None:
        raise ValueError("seeds= and a sampler generator are two sources for the same draws: pass one of them")
    given = sorted(k for k, v in injected.items() if v is not None)
    if given:
        raise ValueError(f"seeds= and {', '.join(given)}= are two sources for the same draws: pass one of them")


def check_seeds(seeds, batch, device):
    """`seeds=` of the samplers: None stays None; otherwise the int64 device tensor of `batch` per-sample seeds
    (ops.seeds_tensor)."""
    if seeds is None:
        return None
    seeds = ops.seeds_tensor(seeds, device)
    if seeds.shape[0] != batch:
        raise MdxError(f"seeds: {seeds.shape[0]} seeds for a batch of {batch}")
    return seeds


def noised_latent(x0, a, b, noise, generator, seeds=None):
    """stochastic_encode of every sampler: a * x0 + b * noise as one ops.q_sample launch into a fresh tensor; `noise` None is
    drawn per sample from `seeds` (stream ops.RNG_ENCODE, draw 0), or without seeds from `generator`."""
    if not (isinstance(x0, torch.Tensor) and x0.is_cuda):
        raise MdxError("stochastic_encode: x0 must be a CUDA(HIP) tensor [B, C, H, W]")
    x0 = x0.to(torch.float32).contiguous()
    check_seed_sources(seeds, generator)
    seeds = check_seeds(seeds, x0.shape[0], x0.device)
    if noise is None and seeds is not None:
        noise = ops.randn_seeded(seeds, ops.RNG_ENCODE, 0, tuple(x0.shape[1:]))
    elif noise is None:
        noise = torch.randn(x0.shape, device=x0.device, dtype=torch.float32, generator=generator)
    noise = torch.as_tensor(noise).to(device=x0.device, dtype=torch.float32).contiguous()
    return ops.q_sample(x0, noise, a, b)


class _Draws:
    """The N(0, 1) draws inside the loop: per sample from `seeds` (one ops.randn_seeded launch each), else the injected
    tensors (tests feed the oracle the same ones), else the sampler's generator."""

    def __init__(self, seeds, generator, dev, shape, step_noises, dropout_masks, blend_noises, temperature, noise_dropout):
        self.seeds, self.generator, self.dev, self.shape = seeds, generator, dev, tuple(shape)
        self.step_noises, self.dropout_masks, self.blend_noises = step_noises, dropout_masks, blend_noises
        self.temperature, self.noise_dropout = temperature, noise_dropout
        self.steps_drawn = 0

    def step(self):
        """temperature * N(0, 1) of the next eta > 0 step, after plms.py:224-225 `ops.dropout(noise, p=noise_dropout)`: zero
        with probability p, the rest scaled by 1 / (1 - p) -- with seeds inside the one launch; dropout_masks[k] (1 = keep)
        injects the mask of the k-th draw."""
        k, p = self.steps_drawn, self.noise_dropout
        self.steps_drawn += 1
        if self.seeds is not None:
            return ops.randn_seeded(self.seeds, ops.RNG_STEP, k, self.shape[1:], scale=self.temperature, dropout=p)
        if self.step_noises is not None:
            noise = torch.as_tensor(self.step_noises[k]).to(device=self.dev, dtype=torch.float32) * self.temperature
        else:
            noise = torch.randn(self.shape, device=self.dev, dtype=torch.float32, generator=self.generator) * self.temperature
        if p > 0.:
            if self.dropout_masks is not None:
                keep = torch.as_tensor(self.dropout_masks[k]).to(device=self.dev, dtype=torch.float32)
            else:
                keep = (torch.rand(self.shape, device=self.dev, generator=self.generator) >= p).to(torch.float32)
            noise = noise * keep / (1. - float(p))
        return noise

    def blend(self, i, x0):
        """The q_sample noise of the mask blend at loop index i (plms.py:153-157; WK: q_sample gets explicit noise)."""
        if self.seeds is not None:
            return ops.randn_seeded(self.seeds, ops.RNG_BLEND, i, self.shape[1:])
        if self.blend_noises is not None:
            return torch.as_tensor(self.blend_noises[i]).to(device=self.dev, dtype=torch.float32)
        return torch.randn(x0.shape, device=self.dev, dtype=torch.float32, generator=self.generator)


def use_cfg(uc, uc_cat, scale):
    """Whether a run evaluates the guidance batch [uncond ; cond]: not without an unconditional context and an unconditional
    c_concat, and not when the scale -- every scale of a per-request list -- is exactly 1.  GuidedModel's rule; whoever lays
    out a context the way GuidedModel will (the pipeline's region contexts) asks this function."""
    return not ((uc is None and uc_cat is None) or bool(np.all(np.asarray(scale) == 1.)))


class GuidedModel:
    """The model call of step i on the guidance batch [uncond; cond] (plms.py:192-195): ``guided(x, i) -> (out_u, out_c)``,
    NHWC fp16 halves of one UNet output (out_u None without guidance).  Everything that does not change over the run is made
    here, once: the [2B, T, D] context (plms.py:194 rebuilds the concat every step), the UNet's input batch with the c_concat
    channels of a hybrid model written into it (step i copies only the latent channels), the timestep rows, and the
    timestep-only part of the UNet for all steps.

    scale: the guidance scale; 1, or neither an unconditional context nor an unconditional c_concat, means no guidance batch.
    Per request: one scale per sample; the guidance batch is used if any of them differs from 1 (a sample whose scale is
    exactly 1 then goes through the combine eu + 1 * (ec - eu), which is not promised bit-equal to an unguided run).
    t_steps: the model-input timestep of every step, in loop order (the UNet's sinusoid takes float timesteps,
    util.py:111-131); per request [n_calls, B], every sample its own (a sample whose schedule has ended keeps its last one):
    the timestep-only part is then computed once over the DISTINCT timesteps and step i gathers its [nb, emb_total] rows.

    image_scale: not None = three-branch guidance (InstructPix2Pix): the batch is [uu ; ui ; ci] = (uc, uc_cat), (uc, c_cat),
    (cond, c_cat), always all three whatever the scales are, and ``guided.out_m`` is the middle third of the output of the last
    call (None in every other run) -- the step launch combines out_u + image_scale (out_m - out_u) + scale (out_c - out_m)."""

    def __init__(self, model, b, shape, cond, uc, c_cat, uc_cat, scale, dev, t_steps, image_scale=None):
        self.model, self.b, self.cx = model, b, shape[0]
        self.out_m = None
        self.dual = image_scale is not None
        if self.dual:
            self._init_dual(b, shape, cond, uc, c_cat, uc_cat, dev, t_steps)
            return
        self.use_cfg = use_cfg(uc, uc_cat, scale)
        nb = self.nb = 2 * b if self.use_cfg else b
        if cond is None:
            self.c_in = None
        else:
            self.c_in = torch.cat([uc.to(cond.dtype), cond], 0).contiguous() if self.use_cfg else cond.contiguous()
        self.x_in = None
        if self.use_cfg or c_cat is not None:
            ccat = 0 if c_cat is None else int(c_cat.shape[1])
            self.x_in = torch.empty((nb, self.cx + ccat) + tuple(shape[1:]), device=dev, dtype=torch.float32)
            if c_cat is not None:                                    # DiffusionWrapper 'hybrid': cat(x, c_concat), written once
                cc = c_cat.to(device=dev, dtype=torch.float32)
                self.x_in[nb - b:, self.cx:] = cc                    # batch = [uncond ; cond]
                if self.use_cfg:
                    self.x_in[:b, self.cx:] = cc if uc_cat is None else uc_cat.to(device=dev, dtype=torch.float32)
        # the two halves of a guidance batch are the same UNet input unless the unconditional branch has its own c_concat
        self.same_halves = self.use_cfg and self.c_in is not None and (c_cat is None or uc_cat is None)
        self._init_times(t_steps, dev)

    def _init_dual(self, b, shape, cond, uc, c_cat, uc_cat, dev, t_steps):
        """The three-branch batch, made once: x_in [3B, cx + ccat, h, w] with the c_concat channels [uc_cat ; c_cat ; c_cat],
        the context [uc ; uc ; cond], the timestep rows three times."""
        missing = [name for name, v in (("a conditioning c_crossattn", cond), ("an unconditional c_crossattn", uc),
                                        ("a c_concat", c_cat), ("an unconditional c_concat", uc_cat)) if v is None]
        if missing:
            raise MdxError(f"image guidance (image_scale) needs {' and '.join(missing)}")
        if np.ndim(t_steps) == 2:
            raise MdxError("image guidance (image_scale) does not take per-request timesteps [n_calls, B]")
        self.use_cfg = True
        nb = self.nb = 3 * b
        self.c_in = torch.cat([uc.to(cond.dtype), uc.to(cond.dtype), cond], 0).contiguous()
        cc = c_cat.to(device=dev, dtype=torch.float32)
        ucc = uc_cat.to(device=dev, dtype=torch.float32)
        if tuple(ucc.shape) != tuple(cc.shape):
            raise MdxError(f"image guidance: the unconditional c_concat {tuple(ucc.shape)} is not the c_concat's {tuple(cc.shape)}")
        self.x_in = torch.empty((nb, self.cx + int(cc.shape[1])) + tuple(shape[1:]), device=dev, dtype=torch.float32)
        self.x_in[:b, self.cx:] = ucc                                # batch = [uu ; ui ; ci]
        self.x_in[b:2 * b, self.cx:] = cc
        self.x_in[2 * b:, self.cx:] = cc
        self.same_halves = False                                     # the branches differ in x
        self._init_times(t_steps, dev)

    def _init_times(self, t_steps, dev):
        model, nb = self.model, self.nb
        # (a fresh array: the flipped view of a ONE-step grid still counts as contiguous and keeps its negative stride)
        t_host = np.array(t_steps, dtype=np.float32)
        self.temb_rows = None
        if t_host.ndim == 2:                                         # per request: [n_calls, B]
            self._per_request_times(t_host, dev)
            return
        t_all = torch.as_tensor(t_host, device=dev)
        # the timestep-only part of the UNet (time_embed MLP + the ResBlock emb_layers, openaimodel.py:550-551,188) for
        # ALL steps in one batched pass; step i then hands row i to the UNet instead of recomputing it.
        # Not for a class-conditional UNet: label_emb(y) joins emb per call.
        self.temb_all = None
        if (hasattr(model, "time_embedding_table") and os.environ.get("MDX_SAMPLER_TEMB_TABLE", "1") != "0"
                and getattr(getattr(model, "unet", None), "num_classes", None) is None):
            self.temb_all = model.time_embedding_table(t_all)
        self.t_all = t_all[:, None].expand(t_all.shape[0], nb).contiguous()

    def _per_request_times(self, t_host, dev):
        """t_all [n_calls, nb] -- for the guidance batch [uncond; cond] duplicates, so both halves still carry the same
        timesteps -- and, where the model has a timestep-only table, that table over the distinct timesteps plus the
        [n_calls, nb] row numbers step i gathers.  Two copies to the device, before the loop."""
        if t_host.shape[1] != self.b:
            raise MdxError(f"GuidedModel: timesteps for {t_host.shape[1]} samples, batch of {self.b}")
        reps = self.nb // self.b
        self.t_all = torch.as_tensor(np.tile(t_host, (1, reps)), device=dev)
        self.temb_all = None
        if (hasattr(self.model, "time_embedding_table") and os.environ.get("MDX_SAMPLER_TEMB_TABLE", "1") != "0"
                and getattr(getattr(self.model, "unet", None), "num_classes", None) is None):
            distinct, rows = np.unique(t_host, return_inverse=True)
            self.temb_all = self.model.time_embedding_table(torch.as_tensor(distinct, device=dev))
            self.temb_rows = torch.as_tensor(np.tile(rows.reshape(t_host.shape), (1, reps)).astype(np.int64), device=dev)

    def _temb(self, i):
        if self.temb_rows is None:
            return self.temb_all[i]
        return self.temb_all.index_select(0, self.temb_rows[i])

    def _eps_nhwc(self, x, i, cfg_dup=False):
        """Prefer the NHWC fast path of our LatentDiffusion; any object with the reference's apply_model(x, t, cond) -> NCHW
        eps still works (its output is re-laid-out by a HIP kernel)."""
        if hasattr(self.model, "apply_model_nhwc"):
            kw = {} if self.temb_all is None else {"temb": self._temb(i)}
            if cfg_dup:     # both halves of the batch are the same x and t: only the contexts differ
                kw["cfg_dup"] = True
            return self.model.apply_model_nhwc(x, self.t_all[i], self.c_in, **kw)
        e = self.model.apply_model(x, self.t_all[i], self.c_in).to(torch.float32).contiguous()
        return ops.nchw_to_nhwc(e, (e.shape[1] + 7) // 8 * 8)

    def __call__(self, x, i):
        b, cx, x_in = self.b, self.cx, self.x_in
        if self.dual:
            x_in[:b, :cx].copy_(x)
            x_in[b:2 * b, :cx].copy_(x)
            x_in[2 * b:, :cx].copy_(x)
            out = self._eps_nhwc(x_in, i)
            self.out_m = out[b:2 * b]
            return out[:b], out[2 * b:]
        if self.use_cfg:
            x_in[:b, :cx].copy_(x)
            x_in[b:, :cx].copy_(x)
            out = self._eps_nhwc(x_in, i, cfg_dup=self.same_halves)
            return out[:b], out[b:]
        if x_in is not None:
            x_in[:, :cx].copy_(x)
            return None, self._eps_nhwc(x_in, i)
        return None, self._eps_nhwc(x, i)
