"""Shared helpers of the InstructPix2Pix tests (test_dual_guidance_cpu.py / test_edit_sampling_gpu.py).

Three-branch guidance is linear in the model output, so the oracle side needs nothing changed under oracle/: EditProxy is a model
whose apply_model(x, t, cond) runs ModelOracle.apply_model on the batch [uu ; ui ; ci] and returns
    e_uu + s_i (e_ui - e_uu) + s_t (e_ci - e_ui)
in fp32 (optionally rescaled to std(e_ci), tests/_rescale_util.py's formula), and the unchanged oracle samplers run it at
guidance scale 1 -- one combine per model evaluation, the second evaluation of the PLMS first step included.
"""
import numpy as np
import torch

import _inpaint_util as U
import _rescale_util as R
from oracle import ldm as O

B, S, T, LAT, IMG = U.B, U.S, U.T, U.LAT, U.IMG
S_T, S_I = 7.5, 1.5
SHAPE = (4, LAT, LAT)


def edit_model(dev):
    """LatentEditDiffusion around the seeded tiny 8-channel UNet (tests/_inpaint_util.py's weights), the tiny VAE attached."""
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentEditDiffusion
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    net = UNetModel(**dict(U.tiny_cfg(8), device=dev))
    net.load_state_dict(U.tiny_params(8))
    model = LatentEditDiffusion(unet_config=net, linear_start=0.00085, linear_end=0.0120, timesteps=1000,
                                scale_factor=U.SCALE_FACTOR)
    vae = AutoencoderKL(ddconfig=dict(TINY_VAE_DDCONFIG), embed_dim=4, device=dev)
    vae.load_state_dict(U.vae_params())
    model.first_stage_model = vae
    return model


def edit_inputs(seed=43):
    """Two different images, the start latent, an image latent of its own (for the sampler-level tests) and the two contexts."""
    rng = np.random.RandomState(seed)
    image = np.clip(0.5 * rng.randn(B, 3, IMG, IMG), -1, 1).astype(np.float32)
    x_T = rng.randn(B, *SHAPE).astype(np.float32)
    c_cat = rng.randn(B, *SHAPE).astype(np.float32)
    ctx = U.tiny_cfg(8)["context_dim"]
    c = rng.randn(B, T, ctx).astype(np.float32)
    uc = np.repeat(rng.randn(1, T, ctx).astype(np.float32), B, 0)
    return dict(image=image, x_T=x_T, c_cat=c_cat, c=c, uc=uc)


class EditProxy(O.ModelOracle):
    """The three-branch combination as ONE model output (see the module docstring).  phi: guidance rescale, in torch."""

    def __init__(self, c_cat, c, uc, s_t=S_T, s_i=S_I, phi=0.0):
        super().__init__(O.UNetOracle(dict(U.tiny_cfg(8), num_heads=-1), U.tiny_params(8)), conditioning_key="hybrid")
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
        cc = t(c_cat)
        self.cat3 = torch.cat([torch.zeros_like(cc), cc, cc], 0)            # [uu ; ui ; ci]
        self.ctx3 = torch.cat([t(uc), t(uc), t(c)], 0)
        self.s_t, self.s_i, self.phi = float(s_t), float(s_i), float(phi)

    def apply_model(self, x, t, cond=None):
        x = torch.as_tensor(x, dtype=torch.float32)
        t = torch.as_tensor(t).reshape(-1)
        if t.shape[0] == 1:
            t = t.expand(x.shape[0])
        out = O.ModelOracle.apply_model(self, torch.cat([x, x, x], 0), torch.cat([t, t, t], 0),
                                        {"c_concat": self.cat3, "c_crossattn": self.ctx3}).to(torch.float32)
        e_uu, e_ui, e_ci = out.chunk(3, dim=0)
        e = e_uu + self.s_i * (e_ui - e_uu) + self.s_t * (e_ci - e_ui)
        if self.phi:
            f = R.rescale_factor(e_ci.numpy(), e.numpy(), self.phi)
            e = e * torch.tensor(f, dtype=torch.float32).reshape(-1, 1, 1, 1)
        return e


def dicts(inp, dev, c_cat=None):
    """(conditioning, unconditional_conditioning) as pipe.edit builds them: the image latent and its zero."""
    d = lambda a: torch.as_tensor(a).to(dev)
    cc = d(inp["c_cat"]) if c_cat is None else c_cat
    return ({"c_concat": cc, "c_crossattn": d(inp["c"]).half()},
            {"c_concat": torch.zeros_like(cc), "c_crossattn": d(inp["uc"]).half()})
