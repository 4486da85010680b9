"""The sampler and pipeline runs that tests/golden/sampler_paths_parent.npz pins (tests/test_sampler_paths_gpu.py and
tests/golden/make_sampler_paths_parent_golden.py share them): one run per branch of the LDM sampling path -- the three
samplers, eps and v models, guidance on and off, guidance rescale, a score corrector, the two mask blends, the plms_sampling
grid options, hybrid conditioning, and the pipeline's entry points with the latent as output.  Built from the public surface
only (sampler classes, sample / decode / make_schedule, DiffusionPipeline), so the file runs unchanged on the tree that
recorded the golden file and on every later one.  Tiny models of _vpred_util / _inpaint_util, 2 x 4 x 8 x 8 latent, 4-5 steps."""
import numpy as np
import torch

import _inpaint_util as U
import _vpred_util as V
from test_unet_gpu import _Corrector

S = 5
SCALE = 3.0
GEN_SEED = 4321
SEEDS = [11, (1 << 40) + 3]
SHAPE = (4, V.H, V.W)


def build_models(dev):
    """eps and v readings of the tiny UNet, the 9-channel hybrid model and the 4-channel model with the tiny VAE."""
    eps, cfg, _ = V.tiny_eps_model()
    v, _, _ = V.tiny_eps_model(parameterization="v")
    return {"eps": eps, "v": v, "ctx_dim": cfg["context_dim"], "hybrid": U.tiny_model(dev, 9), "plain": U.tiny_model(dev, 4)}


def sampler_paths(models, dev):
    """name -> final latent (device tensor)."""
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    from minddiffusion_amd.pipeline import DiffusionPipeline
    cls = {"plms": PLMSSampler, "ddim": DDIMSampler, "dpm": DPMSolverSampler}
    d = lambda a: torch.tensor(a, device=dev)
    x_T, c, uc = (d(a) for a in V.tiny_inputs(models["ctx_dim"]))
    mask, x0 = (d(a) for a in V.blend_inputs())
    gen = lambda: torch.Generator(device=dev).manual_seed(GEN_SEED)
    out = {}

    def run(name, model, kind, steps=S, scale=SCALE, guided=True, x_start=x_T, generator=None, **kw):
        guide = dict(unconditional_guidance_scale=scale, unconditional_conditioning=uc) if guided else {}
        start = {} if x_start is None else {"x_T": x_start}
        out[name] = cls[kind](models[model], generator=generator).sample(steps, V.B, SHAPE, conditioning=c, verbose=False,
                                                                         **start, **guide, **kw)[0]

    # ---- eps model: the three samplers, noise sources, blends, grid options
    run("eps_plms_cfg", "eps", "plms")
    run("eps_plms_unguided", "eps", "plms", guided=False)
    run("eps_ddim_eta0", "eps", "ddim")
    run("eps_ddim_eta1_temp_drop_generator", "eps", "ddim", x_start=None, generator=gen(), eta=1.0, temperature=0.8,
        noise_dropout=0.25)
    run("eps_ddim_eta1_seeds", "eps", "ddim", x_start=None, eta=1.0, seeds=SEEDS)
    run("eps_plms_blend_generator", "eps", "plms", x_start=None, generator=gen(), mask=mask, x0=x0)
    ddim = DDIMSampler(models["eps"])
    ddim.make_schedule(S, ddim_eta=0.0, verbose=False)
    out["eps_ddim_decode_blend_seeds"] = ddim.decode(ddim.stochastic_encode(x0, 3, noise=x_T), c, 3, mask=mask, x0=x0, seeds=SEEDS,
                                                     unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)[0]
    run("eps_plms_original_steps6", "eps", "plms", ddim_use_original_steps=True, timesteps=6)
    run("eps_plms_timesteps_prefix", "eps", "plms", timesteps=4)      # the first 3 of the 5 grid points
    run("eps_dpm_S5_cfg", "eps", "dpm")
    run("eps_dpm_S1", "eps", "dpm", steps=1)
    run("eps_dpm_t_start", "eps", "dpm", steps=3, t_start=0.6)
    # ---- guidance rescale and the score corrector
    for kind in cls:
        run(f"eps_{kind}_rescale", "eps", kind, guidance_rescale=0.7)
    run("eps_ddim_rescale_scale1", "eps", "ddim", scale=1.0, guidance_rescale=0.7)
    for kind in ("plms", "ddim"):
        run(f"eps_{kind}_corrector", "eps", kind, score_corrector=_Corrector(), corrector_kwargs=dict(gain=0.9))
        run(f"eps_{kind}_corrector_rescale", "eps", kind, score_corrector=_Corrector(), corrector_kwargs=dict(gain=0.9),
            guidance_rescale=0.7)
    # ---- v model (PLMS: the second evaluation of its first step is at xm != x)
    for kind in cls:
        run(f"v_{kind}", "v", kind)
        run(f"v_{kind}_rescale", "v", kind, guidance_rescale=0.7)
    # ---- hybrid model, direct sampler calls
    inp = {k: t.to(dev) for k, t in U.pipe_inputs().items()}
    rng = np.random.RandomState(97)
    c_cat, uc_cat = (d(rng.randn(U.B, 5, U.LAT, U.LAT).astype(np.float32)) for _ in range(2))
    hx_T = d(rng.randn(U.B, 4, U.LAT, U.LAT).astype(np.float32))
    hc = {"c_concat": c_cat, "c_crossattn": inp["c"]}

    def hybrid(name, kind, uc_dict):
        guide = {} if uc_dict is None else dict(unconditional_guidance_scale=U.SCALE, unconditional_conditioning=uc_dict)
        out[name] = cls[kind](models["hybrid"]).sample(U.S, U.B, (4, U.LAT, U.LAT), conditioning=hc, x_T=hx_T, verbose=False,
                                                       **guide)[0]
    hybrid("hybrid_plms_same_c_concat", "plms", {"c_concat": c_cat, "c_crossattn": inp["uc"]})
    hybrid("hybrid_plms_own_uc_concat", "plms", {"c_concat": uc_cat, "c_crossattn": inp["uc"]})
    hybrid("hybrid_plms_unguided", "plms", None)
    hybrid("hybrid_dpm", "dpm", {"c_concat": c_cat, "c_crossattn": inp["uc"]})
    # ---- pipeline, latent out
    pipe = lambda model, kind: DiffusionPipeline(models[model], kind, device=dev)
    ckw = dict(c=c, uc=uc, H=8 * V.H, W=8 * V.W, steps=S, scale=SCALE)
    out["pipe_call_seed"] = pipe("eps", "plms")(seed=7, **ckw)
    out["pipe_call_seeds"] = pipe("eps", "ddim")(seeds=SEEDS, eta=0.5, **ckw)
    ikw = dict(init_latent=x0, strength=0.6, c=c, uc=uc, steps=S, scale=SCALE, seed=7)
    out["pipe_img2img_ddim"] = pipe("eps", "ddim").img2img(**ikw)
    out["pipe_img2img_dpm"] = pipe("eps", "dpm_solver").img2img(**ikw)
    # (the blend draws of a masked run come from `seeds`: without them they are torch's global generator's)
    out["pipe_img2img_ddim_mask"] = pipe("eps", "ddim").img2img(mask=mask, seeds=SEEDS, **ikw)
    pkw = dict(c=inp["c"], uc=inp["uc"], steps=U.S, scale=U.SCALE, seed=7, decode=False)
    for kind in ("plms", "dpm_solver"):
        out[f"pipe_inpaint_hybrid_{kind}"] = pipe("hybrid", kind).inpaint(inp["image"], inp["mask"], **pkw)
        out[f"pipe_inpaint_hybrid_{kind}_strength0.5"] = pipe("hybrid", kind).inpaint(inp["image"], inp["mask"], strength=0.5,
                                                                                     **pkw)
    out["pipe_inpaint_blend_plms"] = pipe("plain", "plms").inpaint(inp["image"], inp["mask"], seeds=SEEDS, **pkw)
    return out
