"""ControlledDiffusion -- a LatentDiffusion steered by a ControlNet (Zhang et al. 2023; not in the reference): a second network
reads a hint image (edges, depth, pose, scribble) and its residuals are added to the UNet's skip connections and middle
output (cldm.py of the paper's repository: ControlLDM.apply_model).

The class is a model wrapper in the style of WindowedDiffusion: samplers and the pipeline reach the network through
``apply_model_nhwc`` and ``time_embedding_table`` alone, so PLMS / DDIM / DPM-Solver, v-prediction, guidance rescale, per-request
lists, seeds and img2img run unchanged.  ``with cm.control(hint, scale, uncond):`` is the scope in which control applies;
outside it every call forwards to the inner model, bit for bit.  Per model call inside the scope: one ControlNet evaluation
(ControlNet.forward_residuals, its own plan and hipGraph) and one UNet evaluation on the control plan
(UNetModel.forward_nhwc(control=)), whose single extra launch adds the 13 residuals (ops.ControlAdd).

time_embedding_table(t) inside the scope is the UNet's table and the ControlNet's side by side along the last axis;
apply_model_nhwc splits the row it is handed, so GuidedModel's per-run table and per-request gathers work as they do.
"""
import contextlib
import weakref

import numpy as np
import torch

from .... import distributed as D
from ...._lib import MdxError
from ...modules.diffusionmodules.controlnet import HINT_SCALE, ControlNet
from ...modules.diffusionmodules.openaimodel import Control

# what a ControlNet must share with the UNet it steers: everything that shapes input_blocks / middle_block and their inputs
_SHARED_CONFIG = ("in_channels", "model_channels", "num_res_blocks", "attention_resolutions", "channel_mult", "conv_resample",
                  "num_heads", "num_head_channels", "use_scale_shift_norm", "resblock_updown", "transformer_depth",
                  "context_dim", "legacy", "use_linear")


class ControlledDiffusion:
    """model: a LatentDiffusion with conditioning_key 'crossattn'; controlnet: a ControlNet built from the UNet's config
    (plus hint_channels).  Everything else -- the schedule arrays, parameterization, unet, the first and cond stage models, the
    LoRA calls -- is the inner model's."""

    is_controlled = True

    def __init__(self, model, controlnet):
        from .windowed import WindowedDiffusion
        if isinstance(model, WindowedDiffusion) or getattr(model, "is_controlled", False):
            raise MdxError("ControlledDiffusion: the inner model is a wrapper already (windowed canvases are not controlled: the "
                           "hint has no per-window form)")
        key = getattr(getattr(model, "model", None), "conditioning_key", "crossattn")
        unet = getattr(model, "unet", None)
        if key != "crossattn" or getattr(unet, "num_classes", None) is not None:
            raise MdxError(f"ControlledDiffusion: needs a text-conditional model (conditioning_key 'crossattn', no class "
                           f"labels); got conditioning_key={key!r}: 'hybrid', 'concat' and 'adm' models are not controlled")
        if D.world()[1] > 1:
            raise MdxError("ControlledDiffusion: runs on a single rank (the sharded form is not built)")
        if not isinstance(controlnet, ControlNet):
            raise MdxError(f"ControlledDiffusion: controlnet must be a ControlNet, got {type(controlnet).__name__}")
        diff = [k for k in _SHARED_CONFIG if getattr(controlnet, k) != getattr(unet, k)]
        if diff:
            raise MdxError(f"ControlledDiffusion: the ControlNet's config differs from the UNet's in {', '.join(diff)} "
                           f"(a ControlNet is built from the UNet's config plus hint_channels)")
        if controlnet.device != unet.device:
            raise MdxError(f"ControlledDiffusion: the ControlNet is on {controlnet.device}, the UNet on {unet.device}")
        self.inner, self.controlnet = model, controlnet
        self.n_res = len(controlnet.input_blocks) + 1       # residuals per evaluation: one per input block + the middle block's
        self.evals = 0              # controlled model calls
        self.last_control_batch = None      # rows the ControlNet ran on in the last controlled call
        self._scope = None

    def __getattr__(self, name):    # (only reached for what the wrapper does not define)
        if name in ("inner", "controlnet"):
            raise AttributeError(name)
        return getattr(self.inner, name)

    # ---- the scope
    @contextlib.contextmanager
    def control(self, hint, scale=1.0, uncond=True):
        """Inside the block every model call is controlled.  hint: [B | 1, hint_channels, 8 h, 8 w] in [0, 1] for an h x w
        latent; one row is shared by every sample.  scale: one float, one per sample ([B]), one per residual ([n_res] = 13 on
        the SD UNets, input blocks first, the middle block last) or an [n_res, B] table.  On the guidance batch [uncond ; cond]
        (2 B rows) uncond=True gives both halves the hint; uncond=False leaves the unconditional rows without control -- their
        src_row is -1 -- and runs the ControlNet on the conditional half alone ("guess mode": half its cost).  A batch of B
        rows (no guidance) is controlled in every row either way; with a one-row hint and uncond=False an even batch is read as
        the guidance batch."""
        if self._scope is not None:
            raise MdxError("ControlledDiffusion.control: already inside a control block")
        cn = self.controlnet
        if not (isinstance(hint, torch.Tensor) and hint.dim() == 4 and int(hint.shape[1]) == cn.hint_channels):
            raise MdxError(f"ControlledDiffusion.control: hint must be a tensor [B | 1, {cn.hint_channels}, 8 h, 8 w]")
        if int(hint.shape[2]) % HINT_SCALE or int(hint.shape[3]) % HINT_SCALE:
            raise MdxError(f"ControlledDiffusion.control: the hint's size {tuple(hint.shape[2:])} is not {HINT_SCALE} x a latent "
                           f"grid")
        s = np.asarray(scale.detach().cpu() if isinstance(scale, torch.Tensor) else scale, dtype=np.float64)
        if s.ndim > 2 or not np.all(np.isfinite(s)):
            raise MdxError("ControlledDiffusion.control: scale must be finite: a float, [B], [n_res] or [n_res, B]")
        self._scope = {"hint": hint.to(cn.device), "scale": s, "uncond": bool(uncond), "prep": {}}
        try:
            yield self
        finally:
            self._scope = None

    def _scale_table(self, s, b, nb):
        """fp32 [n_res, nb] from the scope's scale: per-sample values repeat over the halves of a guidance batch."""
        n = self.n_res
        if s.ndim == 0:
            tab = np.full((n, b), float(s))
        elif s.ndim == 2:
            if s.shape != (n, b):
                raise MdxError(f"ControlledDiffusion: a scale table must be [{n}, {b}] (residuals x samples), got {s.shape}")
            tab = s
        elif len(s) == n and len(s) == b:
            raise MdxError(f"ControlledDiffusion: a scale list of {n} entries is ambiguous at a batch of {b}: pass [{n}, {b}]")
        elif len(s) == n:
            tab = np.repeat(s[:, None], b, 1)
        elif len(s) == b:
            tab = np.repeat(s[None, :], n, 0)
        else:
            raise MdxError(f"ControlledDiffusion: scale has {len(s)} entries; expected 1, {b} (per sample) or {n} (per residual)")
        return np.ascontiguousarray(np.tile(tab, (1, nb // b)), dtype=np.float32)

    def _prepare(self, NB, H, W, device):
        """What one (batch, latent size) needs inside the scope, made once: the hint batch the ControlNet runs on (one tensor
        object, so the hint block runs once), the row map and the scale table."""
        sc = self._scope
        key = (NB, H, W)
        hint = sc["hint"]
        ent = sc["prep"].get(key)
        if ent is not None:
            if ent["hint_version"] != hint._version:        # the caller edited the hint in place: refresh ours in place
                if ent["hint"] is not hint:
                    ent["hint"].copy_(hint.expand_as(ent["hint"]) if hint.shape[0] == 1 else hint)
                ent["hint_version"] = hint._version
            return ent
        hb = int(hint.shape[0])
        if (int(hint.shape[2]), int(hint.shape[3])) != (HINT_SCALE * H, HINT_SCALE * W):
            raise MdxError(f"ControlledDiffusion: the hint is {tuple(hint.shape[2:])}, a {H} x {W} latent needs "
                           f"{(HINT_SCALE * H, HINT_SCALE * W)} (the hint is at image resolution, {HINT_SCALE} x the latent)")
        if hb == NB:
            b, guided = NB, False
        elif NB == 2 * hb:
            b, guided = hb, True
        elif hb == 1:
            guided = (not sc["uncond"]) and NB % 2 == 0
            b = NB // 2 if guided else NB
        else:
            raise MdxError(f"ControlledDiffusion: a hint of {hb} rows does not fit a model batch of {NB} (expected {hb}, "
                           f"{2 * hb} for the guidance batch, or a one-row hint)")
        half = guided and not sc["uncond"]          # the ControlNet runs on the conditional half only
        nb_cn = b if (half or not guided) else NB
        rows = ([-1] * b + list(range(b))) if half else list(range(NB))
        h32 = hint.to(torch.float32)
        if hb == nb_cn:
            hint_cn = h32.contiguous()
        elif hb == 1:
            hint_cn = h32.expand(nb_cn, -1, -1, -1).contiguous()
        else:                                       # [uncond ; cond]: the hint repeated to both halves
            hint_cn = torch.cat([h32, h32], 0)
        scale = torch.from_numpy(self._scale_table(sc["scale"], b, NB)).to(device)
        ent = sc["prep"][key] = {"b": b, "half": half, "nb_cn": nb_cn, "rows": rows, "hint": hint_cn, "scale": scale,
                                 "hint_version": hint._version, "cond": None}
        return ent

    @staticmethod
    def _cond_half(ent, cond, b):
        """cond[b:] as ONE view object per conditioning tensor: the ControlNet's context cache is keyed by the tensor object
        (and the version counter a view shares with its base), so a fresh slice per call would re-project the context every step."""
        kept = ent["cond"]
        if kept is None or kept[0]() is not cond:
            kept = ent["cond"] = (weakref.ref(cond), cond[b:])
        return kept[1]

    # ---- the model call
    def time_embedding_table(self, t):
        """Outside the scope the UNet's table; inside, [S, emb_total(UNet) + emb_total(ControlNet)]: both networks' timestep-only
        parts side by side, split again by apply_model_nhwc."""
        tab = self.inner.time_embedding_table(t)
        if self._scope is None:
            return tab
        return torch.cat([tab, self.controlnet.time_embedding_table(t)], -1).contiguous()

    def apply_model_nhwc(self, x, t, cond, temb=None, cfg_dup=False):
        """LatentDiffusion.apply_model_nhwc with the ControlNet's residuals added inside the UNet (the scope); outside the scope
        the inner model's call, unchanged.  Control plans make no use of cfg_dup."""
        if self._scope is None:
            return self.inner.apply_model_nhwc(x, t, cond, temb=temb, cfg_dup=cfg_dup)
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4):
            raise MdxError("ControlledDiffusion: x must be a CUDA(HIP) tensor [NB, C, H, W] (no CPU fallback)")
        if not (isinstance(cond, torch.Tensor) and cond.is_cuda):
            raise MdxError("ControlledDiffusion: a text context is required")
        cn, unet = self.controlnet, self.inner.unet
        NB, _, H, W = (int(v) for v in x.shape)
        ent = self._prepare(NB, H, W, x.device)
        b, half = ent["b"], ent["half"]
        if cn.max_context_len != unet.max_context_len:      # (the pipeline fits the UNet's capacity to long prompts)
            cn.set_max_context_len(unet.max_context_len)
        eu = unet._emb_total
        temb_u = temb_c = None
        if temb is not None:
            if temb.shape[-1] != eu + cn._emb_total:
                raise MdxError(f"ControlledDiffusion: temb rows must come from this wrapper's time_embedding_table() inside the "
                               f"control block ({eu + cn._emb_total} values, got {temb.shape[-1]})")
            temb_u, temb_c = temb[..., :eu], temb[..., eu:]
        x_c, t_c, cond_c = x, t, cond
        if half:
            x_c, cond_c = x[b:], self._cond_half(ent, cond, b)
            if isinstance(t, torch.Tensor) and t.dim() == 1 and t.shape[0] == NB:
                t_c = t[b:]
            if temb_c is not None and temb_c.dim() == 2:
                temb_c = temb_c[b:]
        res = cn.forward_residuals(x_c, t_c, cond_c, ent["hint"], temb=temb_c)
        self.evals += 1
        self.last_control_batch = ent["nb_cn"]
        return self.inner.apply_model_nhwc(x, t, cond, temb=temb_u, control=Control(res, ent["rows"], ent["scale"]))

    def apply_model(self, x_noisy, t, cond=None, return_ids=False, c_concat=None, c_crossattn=None):
        """The NCHW form (LatentDiffusion.apply_model): inside the scope the same pass, then ops.nhwc_to_nchw."""
        if self._scope is None:
            return self.inner.apply_model(x_noisy, t, cond, return_ids=return_ids, c_concat=c_concat, c_crossattn=c_crossattn)
        from .... import ops
        _, c_crossattn = self.inner._split_cond(cond, c_concat, c_crossattn)
        x = x_noisy.to(torch.float32).contiguous()
        out = self.apply_model_nhwc(x, t, c_crossattn)
        return ops.nhwc_to_nchw(out, int(self.inner.unet.final_channels), int(x.shape[2]), int(x.shape[3]))
