"""Shared helpers of the guidance-rescale tests (test_guidance_rescale_cpu.py / test_guidance_rescale_gpu.py).

Guidance rescale (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4), per sample b on
the model outputs as the UNet wrote them (v for a v model, eps for an eps model), N = C * H * W:
    m    = out_u + scale * (out_c - out_u)
    f[b] = phi * std(out_c[b]) / std(m[b]) + (1 - phi)        unbiased std; f[b] = 1 when std(m[b]) is 0 or not finite
    m'   = f[b] * m
RescaleModelOracle puts exactly that into `apply_model` WITHOUT touching oracle/: called with the doubled [uncond; cond] batch
it returns cat([m', m']) (for a v model: the eps converted from m'), so the oracle samplers' own combine
e_u + scale * (e_c - e_u) gives m' back and their unchanged trajectories ARE the rescaled ones -- one rescale per model
evaluation, the second evaluation of the PLMS first step included.
"""
import numpy as np
import torch

import _vpred_util as V
from oracle import ldm as O

PHIS = (0.7, 1.0)
# the guided cases of _vpred_util.TRAJECTORIES (without guidance there is nothing to rescale)
CASES = ("ddim_S5_scale3.0", "plms_S5_scale3.0", "plms_S10_scale7.5", "dpm_S10_scale7.5", "ddim_S5_eta0.6")


def rescale_factor(out_c, m, phi):
    """f[b] in float64 from [B, C, H, W] arrays / tensors."""
    c = np.asarray(out_c, np.float64).reshape(len(out_c), -1)
    m = np.asarray(m, np.float64).reshape(len(m), -1)
    s_c, s_m = c.std(axis=1, ddof=1), m.std(axis=1, ddof=1)
    ok = np.isfinite(s_m) & (s_m > 0)
    return np.where(ok, phi * s_c / np.where(ok, s_m, 1.0) + (1.0 - phi), 1.0)


class _Rescale:
    """apply_model of the doubled batch -> the rescaled combine in both halves; any other batch passes through."""

    def _raw(self, x, t, cond):
        raise NotImplementedError

    def _finish(self, m2, x, t):
        return m2

    def apply_model(self, x, t, cond=None):
        x = torch.as_tensor(x, dtype=torch.float32)
        if x.shape[0] != 2 * self.rescale_b:
            return super().apply_model(x, t, cond)
        u, c = self._raw(x, t, cond).chunk(2, dim=0)
        m = O.r16(u + O.r16(self.rescale_scale * O.r16(c - u)))          # the oracle's own rounding of the combine
        f = rescale_factor(c.numpy(), m.numpy(), self.rescale_phi)
        self.factors.append(f)
        m = O.r16(m * torch.tensor(f, dtype=torch.float32).reshape(-1, 1, 1, 1))
        return self._finish(torch.cat([m, m], 0), x, t)


class _RescaleEps(_Rescale, O.ModelOracle):
    def _raw(self, x, t, cond):
        return O.ModelOracle.apply_model(self, x, t, cond)


class _RescaleV(_Rescale, V.VModelOracle):
    def _raw(self, x, t, cond):
        return self.raw_v(x, t, cond)

    def _finish(self, m2, x, t):          # the conversion stays in apply_model, as in VModelOracle
        a, b = self.ab(t)
        return O.r16(a * m2 + b * x)


def RescaleModelOracle(base, phi, scale, b):
    """The oracle `base` (a VModelOracle, or a plain O.ModelOracle) with guidance rescale `phi` at guidance scale `scale`
    for batches of `b` samples."""
    om = (_RescaleV if isinstance(base, V.VModelOracle) else _RescaleEps)(base.unet)
    om.conditioning_key = base.conditioning_key
    om.rescale_phi, om.rescale_scale, om.rescale_b, om.factors = float(phi), float(scale), int(b), []
    return om


def oracle_trajectory(name, base, ctx_dim, phi):
    scale = V.TRAJECTORIES[name][2]
    return V.oracle_trajectory(name, RescaleModelOracle(base, phi, scale, V.B), ctx_dim)


def product_trajectory(name, model, ctx_dim, dev, **sample_kw):
    """_vpred_util.product_trajectory with extra sample() keywords (guidance_rescale=phi, score_corrector=...)."""
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    sampler, S, scale, extra = V.TRAJECTORIES[name]
    x_T, c, uc = V.tiny_inputs(ctx_dim)
    d = lambda a: torch.tensor(a, device=dev)
    kw = dict(sample_kw)
    if extra == "eta":
        kw.update(eta=0.6, step_noises=V.step_noises(S))
    elif extra == "blend":
        m, x0 = V.blend_inputs()
        kw.update(mask=d(m), x0=d(x0), blend_noises=V.step_noises(S, seed=79))
    cls = {"plms": PLMSSampler, "ddim": DDIMSampler, "dpm": DPMSolverSampler}[sampler]
    return cls(model).sample(S, V.B, (4, V.H, V.W), conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=scale,
                             unconditional_conditioning=d(uc), verbose=False, **kw)[0]
