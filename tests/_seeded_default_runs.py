"""The `seeds=None` sampler runs that tests/golden/seeded_parent.npz pins (tests/test_seeded_noise_gpu.py and
tests/golden/make_seeded_parent_golden.py share them): every draw comes from a seeded torch generator, as it did before
per-sample seeds existed.  Tiny UNet of _vpred_util, 2 x 4 x 8 x 8 latent, 4 steps."""
import torch

import _vpred_util as V

S = 4
GEN_SEED = 1234


def default_runs(model, ctx_dim, dev):
    """name -> final latent (device tensor).  x_T, the eta > 0 step noise and the dropout mask are all torch draws."""
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    _, c, uc = V.tiny_inputs(ctx_dim)
    d = lambda a: torch.tensor(a, device=dev)
    cases = {"plms": (PLMSSampler, {}),
             "ddim_eta1": (DDIMSampler, dict(eta=1.0)),
             "ddim_eta1_temp_drop": (DDIMSampler, dict(eta=1.0, temperature=0.8, noise_dropout=0.25))}
    out = {}
    for name, (cls, kw) in cases.items():
        g = torch.Generator(device=dev).manual_seed(GEN_SEED)
        out[name] = cls(model, generator=g).sample(S, V.B, (4, V.H, V.W), conditioning=d(c), unconditional_guidance_scale=3.0,
                                                   unconditional_conditioning=d(uc), verbose=False, **kw)[0]
    return out
