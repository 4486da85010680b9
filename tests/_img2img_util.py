"""Shared helpers of the img2img tests (test_img2img_cpu.py / test_img2img_gpu.py).

A partial run -- the last t_enc model evaluations of an S-step schedule, from x0 noised to the level of the first step that
runs -- is expressed on the oracle WITHOUT touching oracle/:
  * PLMS / DDIM: O.sample(..., x_T=x_enc, timesteps=t_enc + 1).  The reference's prefix rule (plms.py:137-139) keeps
    int(min(timesteps / S, 1) * S) - 1 grid points, which for the pairs used here is exactly t_enc (oracle_partial asserts
    it, and the number of model calls); timesteps=None when t_enc == S.
  * DPM-Solver++: PartialDPMSolver.sample(t_start=), the oracle solver's loop on linspace(t_start, t_0, steps + 1)
    (the reference's DPM_Solver.sample(t_start=), dpm_solver.py:958-1075).
"""
import numpy as np
import torch

import _vpred_util as V
from oracle import dpm_solver as OD
from oracle import ldm as O

B, H, W = V.B, V.H, V.W
SHAPE = (4, H, W)

# name -> (parameterization, sampler, S, t_enc, scale, extra)
CASES = {
    "eps_ddim_S10_t7_scale7.5": ("eps", "ddim", 10, 7, 7.5, None),
    "eps_plms_S10_t5_scale7.5": ("eps", "plms", 10, 5, 7.5, None),
    "eps_ddim_S5_t3_eta0.6": ("eps", "ddim", 5, 3, 3.0, "eta"),
    "eps_plms_S8_t4_mask": ("eps", "plms", 8, 4, 1.0, "mask"),
    "eps_ddim_S8_t4_mask": ("eps", "ddim", 8, 4, 3.0, "mask"),
    "eps_plms_S6_t1_scale3.0": ("eps", "plms", 6, 1, 3.0, None),
    "v_ddim_S10_t7_scale7.5": ("v", "ddim", 10, 7, 7.5, None),
    "v_plms_S5_t3_scale3.0": ("v", "plms", 5, 3, 3.0, None),
    # DPM-Solver++: one guided run and one with a single (first-order) evaluation
    "eps_dpm_S10_t6_scale7.5": ("eps", "dpm", 10, 6, 7.5, None),
    "eps_dpm_S8_t1_scale3.0": ("eps", "dpm", 8, 1, 3.0, None),
}


def start_inputs(seed=211):
    """The init latent and the forward-process noise of every case."""
    rng = np.random.RandomState(seed)
    return rng.randn(B, *SHAPE).astype(np.float32), rng.randn(B, *SHAPE).astype(np.float32)


def dpm_t_start(S, t_enc, n=1000):
    """The continuous time the last t_enc of the S-step grid's intervals start at."""
    t_0 = 1.0 / n
    return t_0 + (1.0 - t_0) * t_enc / S


def oracle_model(param, cfg, params):
    unet = O.UNetOracle(dict(cfg, num_heads=-1), params)
    return V.VModelOracle(unet) if param == "v" else O.ModelOracle(unet)


class PartialDPMSolver(OD.DPM_Solver):
    """oracle DPM_Solver whose sample() takes the reference's `t_start` (dpm_solver.py:958, :1040-1041)."""

    def sample(self, x, steps, t_start=None, order=2, lower_order_final=True):
        ns = self.noise_schedule
        t_0, t_T = 1.0 / ns.total_N, (ns.T if t_start is None else t_start)
        order = min(order, steps)                       # a one-evaluation run is one first-order update
        timesteps = torch.linspace(t_T, t_0, steps + 1, dtype=torch.float64)
        vec_t = timesteps[0].expand((x.shape[0],))
        model_prev_list = [self.model_fn(x, vec_t)]
        t_prev_list = [vec_t]
        for init_order in range(1, order):
            vec_t = timesteps[init_order].expand((x.shape[0],))
            x = self.multistep_dpm_solver_update(x, model_prev_list, t_prev_list, vec_t, init_order)
            model_prev_list.append(self.model_fn(x, vec_t))
            t_prev_list.append(vec_t)
        for step in range(order, steps + 1):
            vec_t = timesteps[step].expand((x.shape[0],))
            step_order = min(order, steps + 1 - step) if (lower_order_final and steps < 15) else order
            x = self.multistep_dpm_solver_update(x, model_prev_list, t_prev_list, vec_t, step_order)
            for i in range(order - 1):
                t_prev_list[i] = t_prev_list[i + 1]
                model_prev_list[i] = model_prev_list[i + 1]
            t_prev_list[-1] = vec_t
            if step < steps:
                model_prev_list[-1] = self.model_fn(x, vec_t)
        return x


def oracle_encode(name, omodel):
    """x0 noised to where case `name` starts, by the oracle's own q_sample / noise schedule."""
    _, sampler, S, t_enc, _, _ = CASES[name]
    x0, noise = start_inputs()
    if sampler == "dpm":
        ns = OD.NoiseScheduleVP("discrete", alphas_cumprod=omodel.alphas_cumprod)
        t = torch.tensor([dpm_t_start(S, t_enc)], dtype=torch.float64)
        a, b = float(ns.marginal_alpha(t)), float(ns.marginal_std(t))
        return (a * torch.tensor(x0, dtype=torch.float64) + b * torch.tensor(noise, dtype=torch.float64)).to(torch.float32)
    t = int(O.make_ddim_timesteps(S, omodel.num_timesteps)[t_enc - 1])
    return omodel.q_sample(torch.tensor(x0), torch.full((B,), t, dtype=torch.int64), torch.tensor(noise))


def oracle_partial(name, omodel, ctx_dim):
    """Final latent of case `name`: the oracle's own samplers on the last t_enc steps, from oracle_encode()."""
    _, sampler, S, t_enc, scale, extra = CASES[name]
    _, c, uc = V.tiny_inputs(ctx_dim)
    x_enc = oracle_encode(name, omodel)
    calls = omodel.calls
    if sampler == "dpm":
        ns = OD.NoiseScheduleVP("discrete", alphas_cumprod=omodel.alphas_cumprod)
        fn = OD.model_wrapper(lambda x, t, cc: omodel.apply_model(x, t, cc), ns, torch.tensor(c), torch.tensor(uc), float(scale))
        solver = PartialDPMSolver(fn, ns, predict_x0=True)
        out = solver.sample(x_enc, steps=t_enc, t_start=dpm_t_start(S, t_enc))
        assert solver.nfe == t_enc and omodel.calls - calls == t_enc
        return out
    kw = {}
    if t_enc != S:
        kw["timesteps"] = t_enc + 1
        assert int(min((t_enc + 1) / S, 1) * S) - 1 == t_enc, (S, t_enc)      # the reference's prefix rule keeps t_enc steps
    if extra == "eta":
        it = iter(V.step_noises(t_enc))
        kw.update(eta=0.6, noise_fn=lambda shp: next(it))
    elif extra == "mask":
        m, xb = V.blend_inputs()
        kw.update(mask=m, x0=xb, blend_noises=V.step_noises(t_enc, seed=79))
    out, inter = O.sample(omodel, S, B, SHAPE, c, x_enc, sampler, unconditional_guidance_scale=scale,
                          unconditional_conditioning=uc, **kw)
    assert omodel.calls - calls == t_enc + (sampler == "plms"), (omodel.calls - calls, t_enc)
    return out


def product_sampler(name, model):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    return {"plms": PLMSSampler, "ddim": DDIMSampler, "dpm": DPMSolverSampler}[CASES[name][1]](model)


def product_encode(name, model, dev):
    """(sampler, x_enc): the product's stochastic_encode of the case's (x0, noise)."""
    _, kind, S, t_enc, _, extra = CASES[name]
    x0, noise = start_inputs()
    d = lambda a: torch.tensor(a, device=dev)
    sampler = product_sampler(name, model)
    if kind == "dpm":
        return sampler, sampler.stochastic_encode(d(x0), dpm_t_start(S, t_enc), noise=d(noise))
    sampler.make_schedule(S, ddim_eta=0.6 if extra == "eta" else 0., verbose=False)
    return sampler, sampler.stochastic_encode(d(x0), t_enc, noise=d(noise))


def product_decode(name, sampler, x_enc, ctx_dim, dev):
    """The remaining steps of case `name` from x_enc: decode (DPM-Solver: sample(t_start=))."""
    _, kind, S, t_enc, scale, extra = CASES[name]
    _, c, uc = V.tiny_inputs(ctx_dim)
    d = lambda a: torch.tensor(a, device=dev)
    if kind == "dpm":
        return sampler.sample(t_enc, B, SHAPE, conditioning=d(c), x_T=x_enc, unconditional_guidance_scale=scale,
                              unconditional_conditioning=d(uc), verbose=False, t_start=dpm_t_start(S, t_enc))[0]
    kw = {}
    if extra == "eta":
        kw.update(step_noises=V.step_noises(t_enc))
    elif extra == "mask":
        m, xb = V.blend_inputs()
        kw.update(mask=d(m), x0=d(xb), blend_noises=V.step_noises(t_enc, seed=79))
    return sampler.decode(x_enc, d(c), t_enc, unconditional_guidance_scale=scale, unconditional_conditioning=d(uc), **kw)[0]


def product_partial(name, model, ctx_dim, dev):
    """The same case through the product: stochastic_encode + decode."""
    sampler, x_enc = product_encode(name, model, dev)
    return product_decode(name, sampler, x_enc, ctx_dim, dev)
