"""Shared helpers of the v-prediction tests (test_vpred_cpu.py / test_vpred_gpu.py).

VModelOracle reads the oracle UNet's output as v WITHOUT touching oracle/: its apply_model returns
    a * unet(x, t, c) + b * x        (eps = a v + b x, upstream LDM predict_eps_from_z_and_v)
with (a, b) = (sqrt(alphas_cumprod[t]), sqrt(1 - alphas_cumprod[t])) of the call's own t.  The oracle's unchanged eps
samplers on top of it therefore ARE the v-prediction trajectory: the conversion happens per model call at the call's own
(x, t), which is exactly what the product's fused step has to reproduce (including the second evaluation of the PLMS first
step at (x_next, t_next)).
"""
import numpy as np
import torch

from oracle import dpm_solver as OD
from oracle import ldm as O


class VModelOracle(O.ModelOracle):
    """ModelOracle whose network output is v.  `raw_v(x, t, c)` is the v output itself (what a v checkpoint's UNet returns);
    `apply_model` is what the oracle's eps samplers call and returns the converted eps = a v + b x."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.parameterization = "v"
        self._ns = OD.NoiseScheduleVP("discrete", alphas_cumprod=self.alphas_cumprod)

    def ab(self, t):
        """(a, b) of the model call: the oracle's tables at an integer t (O.sample), NoiseScheduleVP at
        t_continuous = t_input / 1000 + 1 / 1000 for the fractional model-input times of OD.sample."""
        t = torch.as_tensor(t)
        if t.is_floating_point():
            tc = t.to(torch.float64) / 1000.0 + 1.0 / 1000.0
            a, b = self._ns.marginal_alpha(tc), self._ns.marginal_std(tc)
        else:
            a = torch.as_tensor(self.sqrt_alphas_cumprod)[t]
            b = torch.as_tensor(self.sqrt_one_minus_alphas_cumprod)[t]
        return (O.r16(a.to(torch.float32)).reshape(-1, 1, 1, 1), O.r16(b.to(torch.float32)).reshape(-1, 1, 1, 1))

    def raw_v(self, x, t, cond=None):
        return super().apply_model(x, t, cond)

    def apply_model(self, x, t, cond=None):
        a, b = self.ab(t)
        x = torch.as_tensor(x, dtype=torch.float32)
        return O.r16(a * self.raw_v(x, t, cond) + b * x)     # emulate_fp16: the sampler's x is fp32, eps an fp16 tensor


# ------------------------------------------------------------------------------------------------ tiny-UNet trajectory cases
TINY_SEED = 3
B, H, W, T = 2, 8, 8, 6


def tiny_inputs(ctx_dim, seed=119):
    """Start noise and the two contexts of the tiny trajectory cases (the uncond context is one row, repeated).
    On seed 119 the oracle's own fp32 and emulate_fp16() runs of every v case stay inside the trajectory bound
    (test_vpred_cpu.py asserts it; the guided 10-step PLMS case is the tightest, 8.9e-3 / 9.1e-3)."""
    x_T = np.random.RandomState(seed).randn(B, 4, H, W).astype(np.float32)
    c = np.random.RandomState(seed + 1).randn(B, T, ctx_dim).astype(np.float32)
    uc = np.repeat(np.random.RandomState(seed + 2).randn(1, T, ctx_dim).astype(np.float32), B, 0)
    return x_T, c, uc


def step_noises(n, seed=77):
    rng = np.random.RandomState(seed)
    return [rng.randn(B, 4, H, W).astype(np.float32) for _ in range(n)]


def blend_inputs(seed=78):
    rng = np.random.RandomState(seed)
    return (rng.rand(B, 1, H, W) > 0.5).astype(np.float32), rng.randn(B, 4, H, W).astype(np.float32)


# name -> (sampler, S, scale, extras); the oracle side of every case is oracle_trajectory(), shared by the CPU seed check
# (fp32 vs emulate_fp16 inside the bound) and the GPU parity test
TRAJECTORIES = {
    "plms_S5_scale3.0": ("plms", 5, 3.0, None),
    "plms_S10_scale7.5": ("plms", 10, 7.5, None),
    "ddim_S5_scale3.0": ("ddim", 5, 3.0, None),
    "ddim_S4_scale1.0": ("ddim", 4, 1.0, None),
    "ddim_S5_eta0.6": ("ddim", 5, 3.0, "eta"),
    # mask / x0 blending runs without guidance: at scale 3.0 the oracle's own fp32 and fp16-emulated runs of this case are
    # 1.2e-2 ... 1.5e-2 apart, outside the bound the device is held to (guided PLMS is covered by the two cases above)
    "plms_S5_blend": ("plms", 5, 1.0, "blend"),
    "dpm_S10_scale7.5": ("dpm", 10, 7.5, None),
    "dpm_S15_scale1.0": ("dpm", 15, 1.0, None),
}


def oracle_trajectory(name, omodel, ctx_dim):
    """Final latent of case `name` from the oracle's own samplers on `omodel` (a VModelOracle, or a plain one)."""
    sampler, S, scale, extra = TRAJECTORIES[name]
    x_T, c, uc = tiny_inputs(ctx_dim)
    if sampler == "dpm":
        return OD.sample(omodel, S, B, (4, H, W), c, x_T, unconditional_guidance_scale=scale,
                         unconditional_conditioning=uc)[0]
    kw = {}
    if extra == "eta":
        it = iter(step_noises(S))
        kw.update(eta=0.6, noise_fn=lambda shp: next(it))
    elif extra == "blend":
        m, x0 = blend_inputs()
        kw.update(mask=m, x0=x0, blend_noises=step_noises(S, seed=79))
    return O.sample(omodel, S, B, (4, H, W), c, x_T, sampler, unconditional_guidance_scale=scale,
                    unconditional_conditioning=uc, **kw)[0]


def product_trajectory(name, model, ctx_dim, dev):
    """The same case through the product's samplers on `model` (anything with the LatentDiffusion sampler surface)."""
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    sampler, S, scale, extra = TRAJECTORIES[name]
    x_T, c, uc = tiny_inputs(ctx_dim)
    d = lambda a: torch.tensor(a, device=dev)
    kw = {}
    if extra == "eta":
        kw.update(eta=0.6, step_noises=step_noises(S))
    elif extra == "blend":
        m, x0 = blend_inputs()
        kw.update(mask=d(m), x0=d(x0), blend_noises=step_noises(S, seed=79))
    cls = {"plms": PLMSSampler, "ddim": DDIMSampler, "dpm": DPMSolverSampler}[sampler]
    return cls(model).sample(S, B, (4, H, W), conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=scale,
                             unconditional_conditioning=d(uc), verbose=False, **kw)[0]


# short "eps" runs of all three samplers (they must keep going through mdx_sampler_step_f32)
EPS_IDENTITY_CASES = ("ddim_S4_scale1.0", "ddim_S5_scale3.0", "plms_S5_scale3.0", "dpm_S10_scale7.5")


def tiny_eps_model(graph=True, **ldm_kw):
    """LatentDiffusion ("eps" unless ldm_kw says otherwise) around the seeded tiny UNet, and its oracle parameters."""
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    cfg = dict(TINY_UNET)
    params = O.init_params(dict(cfg, num_heads=-1), seed=TINY_SEED)
    net = UNetModel(**cfg)
    net.use_graph = graph
    net.load_state_dict(params)
    return LatentDiffusion(net, linear_start=0.00085, linear_end=0.0120, timesteps=1000, **ldm_kw), cfg, params
