"""The per-request and session runs that tests/golden/request_paths_parent.npz pins (tests/test_request_paths_gpu.py and
tests/golden/make_request_paths_parent_golden.py share them): what tests/_sampler_paths.py leaves out, because its runs all
take scalars -- the runs whose step scalars come from a StepTable (sample() with per-sample lists) and from the rows of a
session's slots (DiffusionPipeline.serve).  Built from the public surface only (sampler classes, sample, DiffusionPipeline),
so the file runs unchanged on the tree that recorded the golden file and on every later one.  Tiny models of _vpred_util,
2 x 4 x 8 x 8 latent, at most 5 steps."""
import numpy as np
import torch

import _vpred_util as V

STEPS, SCALES, PHIS = [2, 5], [1.5, 3.0], [0.0, 0.7]
SEEDS = [11, (1 << 40) + 3]
SHAPE = (4, V.H, V.W)
SLOTS = 2
# the four requests of a session case: (steps, scale, guidance_rescale, seed)
REQUESTS = [(4, 1.5, 0.0, 5), (2, 3.0, 0.7, 7), (5, 7.5, 0.3, 9), (4, 3.0, 0.0, 11)]


def build_models(dev):
    """eps and v readings of the tiny UNet."""
    eps, cfg, _ = V.tiny_eps_model()
    v, _, _ = V.tiny_eps_model(parameterization="v")
    return {"eps": eps, "v": v, "ctx_dim": cfg["context_dim"]}


def request_paths(models, dev):
    """name -> final latents (device tensor)."""
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    from minddiffusion_amd.pipeline import DiffusionPipeline
    cls = {"plms": PLMSSampler, "ddim": DDIMSampler, "dpm": DPMSolverSampler}
    d = lambda a: torch.tensor(a, device=dev)
    x_T, c, uc = (d(a) for a in V.tiny_inputs(models["ctx_dim"]))
    out = {}

    def run(name, model, kind, steps=STEPS, x_start=x_T, **kw):
        start = {} if x_start is None else {"x_T": x_start}
        out[name] = cls[kind](models[model]).sample(steps, V.B, SHAPE, conditioning=c, unconditional_conditioning=uc,
                                                    unconditional_guidance_scale=SCALES, guidance_rescale=PHIS, verbose=False,
                                                    **start, **kw)[0]

    # ---- sample() on a StepTable: every sample its own step count, scale and rescale
    for model in ("eps", "v"):
        for kind in cls:
            run(f"{model}_{kind}_lists", model, kind)
        run(f"{model}_ddim_lists_eta0.5_seeds", model, "ddim", x_start=None, eta=0.5, seeds=SEEDS)
        run(f"{model}_dpm_uniform_t_start", model, "dpm", steps=[3, 3], t_start=0.6)
    # ---- sessions: four requests through two slots
    rng = np.random.RandomState(211)
    n = len(REQUESTS)
    cs = d(rng.randn(n, V.T, models["ctx_dim"]).astype(np.float32))
    ucs = d(np.repeat(rng.randn(1, V.T, models["ctx_dim"]).astype(np.float32), n, 0))
    z0 = d(rng.randn(*SHAPE).astype(np.float32))
    keep = d((rng.rand(1, V.H, V.W) > 0.5).astype(np.float32))
    for model, kind in (("eps", "ddim"), ("v", "ddim"), ("eps", "dpm_solver"), ("v", "dpm_solver")):
        reqs = [dict(c=cs[r], uc=ucs[r], steps=s, scale=scale, guidance_rescale=phi, seed=seed,
                     eta=0.5 if (kind == "ddim" and r == 2) else 0.0)
                for r, (s, scale, phi, seed) in enumerate(REQUESTS)]
        if kind == "ddim":                                               # the last 3 of 4 steps, blended with z0 every tick
            reqs[3].update(init_latent=z0, strength=0.75, keep_mask=keep)
        else:                                                            # the last 2 of 4 steps from a continuous start time
            reqs[3].update(init_latent=z0, strength=0.5)
        out[f"{model}_serve_{kind}"] = DiffusionPipeline(models[model], kind, device=dev).serve(
            reqs, slots=SLOTS, H=8 * V.H, W=8 * V.W, output="latent")
    return out
