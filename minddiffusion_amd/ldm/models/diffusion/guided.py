"""What PLMSSampler, DDIMSampler and DPMSolverSampler do before and inside their loops in the same way: the conditioning a
caller may hand over (split_conditioning), the start latent (start_latent), and the model call of one step on the
classifier-free-guidance batch (GuidedModel)."""
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


# ---- the scalars of one fused step launch.  The scalar path hands them to ops.sampler_update, the per-request path writes
# them into a StepTable row: both call these functions, so a row holds the very float32 the scalar call would have passed.
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
    the timestep-only part is then computed once over the DISTINCT timesteps and step i gathers its [nb, emb_total] rows."""

    def __init__(self, model, b, shape, cond, uc, c_cat, uc_cat, scale, dev, t_steps):
        self.model, self.b, self.cx = model, b, shape[0]
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
        if self.use_cfg:
            x_in[:b, :cx].copy_(x)
            x_in[b:, :cx].copy_(x)
            out = self._eps_nhwc(x_in, i, cfg_dup=self.same_halves)
            return out[:b], out[b:]
        if x_in is not None:
            x_in[:, :cx].copy_(x)
            return None, self._eps_nhwc(x_in, i)
        return None, self._eps_nhwc(x, i)
