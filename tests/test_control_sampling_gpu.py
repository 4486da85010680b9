"""Controlled sampling end to end: four-step DDIM / PLMS / DPM-Solver runs of the tiny LDM at guidance scale 5 inside
ControlledDiffusion.control(), against the oracle's own samplers on the controlled ModelOracle (tests/_control_util.py); a
v-prediction model, guidance rescale, guess mode; and the pipeline entry point against the sampler-level run.  The tolerance is
the project's trajectory tolerance, rel-L2 <= 1e-2."""
import functools

import numpy as np
import pytest
import torch

import _control_util as CU
import _rescale_util as R
import _vpred_util as V
from _util import check
from oracle import dpm_solver as OD
from oracle import ldm as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S, SCALE = 4, 5.0
TRAJ_TOL = 1e-2


@functools.lru_cache(maxsize=None)
def _setup(param="eps"):
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.ldm.models.diffusion.controlled import ControlledDiffusion
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from minddiffusion_amd.ldm.modules.diffusionmodules.controlnet import ControlNet
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    ocfg = dict(TINY_UNET, num_heads=-1)
    up, cp = O.init_params(ocfg, seed=V.TINY_SEED), CU.init_control_params(ocfg, seed=V.TINY_SEED + 10)
    net, cn = UNetModel(**TINY_UNET).load_state_dict(up), ControlNet(**TINY_UNET).load_state_dict(cp)
    model = LatentDiffusion(net, linear_start=0.00085, linear_end=0.0120, timesteps=1000, parameterization=param)
    return ocfg, model, cn, ControlledDiffusion(model, cn), CU.ControlOracle(ocfg, up, cp)


@functools.lru_cache(maxsize=None)
def _hint():
    return CU.blocky_hint(np.random.RandomState(404), V.B, 3, 8 * V.H, 8 * V.W)


def _oracle_model(param="eps", scale=1.0, uncond=True, phi=None):
    orc = _setup(param)[4]
    if param == "v":
        om = V.VModelOracle(CU.ControlledUNet(orc, _hint(), V.B, scale, uncond), conditioning_key="crossattn")
    else:
        om = CU.ControlModelOracle(orc, _hint(), V.B, scale, uncond)
    return om if phi is None else R.RescaleModelOracle(om, phi, SCALE, V.B)


def _oracle_run(sampler, om, ctx_dim):
    x_T, c, uc = V.tiny_inputs(ctx_dim)
    if sampler == "dpm":
        return OD.sample(om, S, V.B, (4, V.H, V.W), c, x_T, unconditional_guidance_scale=SCALE, unconditional_conditioning=uc)[0]
    return O.sample(om, S, V.B, (4, V.H, V.W), c, x_T, sampler, unconditional_guidance_scale=SCALE,
                    unconditional_conditioning=uc)[0]


def _product_run(sampler, cm, ctx_dim, scale=1.0, uncond=True, **kw):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    x_T, c, uc = V.tiny_inputs(ctx_dim)
    d = lambda a: torch.tensor(a, device=DEV)
    cls = {"plms": PLMSSampler, "ddim": DDIMSampler, "dpm": DPMSolverSampler}[sampler]
    with cm.control(d(_hint()), scale=scale, uncond=uncond):
        out = cls(cm).sample(S, V.B, (4, V.H, V.W), conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=SCALE,
                             unconditional_conditioning=d(uc), verbose=False, **kw)[0]
    assert cm._scope is None
    return out


@pytest.mark.parametrize("sampler", ["ddim", "plms", "dpm"])
def test_controlled_trajectories_match_the_oracle(sampler):
    ocfg, _, cn, cm, _ = _setup()
    evals = cm.evals
    got = _product_run(sampler, cm, ocfg["context_dim"])
    assert cm.evals - evals >= S and cm.last_control_batch == 2 * V.B         # one ControlNet evaluation per model call
    check(f"control.traj[{sampler}]", got, _oracle_run(sampler, _oracle_model(), ocfg["context_dim"]), rel_l2=TRAJ_TOL)


def test_the_control_moves_the_trajectory():
    """The oracle-side distance between the controlled and the plain run: far above the tolerance the runs above are held to."""
    ocfg, model, _, cm, orc = _setup()
    plain = _oracle_run("ddim", O.ModelOracle(orc.unet), ocfg["context_dim"])
    ctl = _oracle_run("ddim", _oracle_model(), ocfg["context_dim"])
    assert CU.rel_l2(ctl.numpy(), plain.numpy()) >= 10 * TRAJ_TOL


def test_guess_mode_trajectory_and_scales():
    ocfg, _, cn, cm, _ = _setup()
    scale = [0.5, 1.5]
    got = _product_run("ddim", cm, ocfg["context_dim"], scale=scale, uncond=False)
    assert cm.last_control_batch == V.B          # the ControlNet ran on the conditional half only
    check("control.traj[guess]", got, _oracle_run("ddim", _oracle_model(scale=scale, uncond=False), ocfg["context_dim"]),
          rel_l2=TRAJ_TOL)


def test_v_prediction_model():
    ocfg, _, _, cm, _ = _setup("v")
    got = _product_run("ddim", cm, ocfg["context_dim"])
    check("control.traj[v]", got, _oracle_run("ddim", _oracle_model("v"), ocfg["context_dim"]), rel_l2=TRAJ_TOL)


def test_guidance_rescale():
    ocfg, _, _, cm, _ = _setup()
    got = _product_run("ddim", cm, ocfg["context_dim"], guidance_rescale=0.7)
    check("control.traj[rescale]", got, _oracle_run("ddim", _oracle_model(phi=0.7), ocfg["context_dim"]), rel_l2=TRAJ_TOL)


@pytest.mark.parametrize("kind", ["ddim", "dpm_solver"])
def test_the_pipeline_call_is_the_sampler_level_run(kind):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    ocfg, model, cn, cm, _ = _setup()
    _, c, uc = V.tiny_inputs(ocfg["context_dim"])
    c16, uc16 = (torch.tensor(a, device=DEV).to(torch.float16) for a in (c, uc))
    hint = torch.tensor(_hint())
    seeds = [11, 12]
    pipe = DiffusionPipeline(model, kind)
    cp = pipe.controlled(cn)
    assert cp.model.inner is model and cp.model.controlnet is cn and type(cp.sampler) is type(pipe.sampler)
    got = cp(c=c16, uc=uc16, H=8 * V.H, W=8 * V.W, steps=S, scale=SCALE, control_image=hint, control_scale=[0.5, 1.5],
             control_uncond=False, seeds=seeds)
    with cm.control(hint.to(DEV), scale=[0.5, 1.5], uncond=False):
        ref = type(cp.sampler)(cm).sample(S=S, conditioning=c16, batch_size=V.B, shape=[4, V.H, V.W], verbose=False,
                                         unconditional_guidance_scale=SCALE, unconditional_conditioning=uc16, eta=0.0,
                                         seeds=seeds)[0]
    assert torch.equal(got, ref)
    # without control_image the controlled pipeline does what the plain one does
    assert torch.equal(cp(c=c16, uc=uc16, H=8 * V.H, W=8 * V.W, steps=S, scale=SCALE, seeds=seeds),
                       pipe(c=c16, uc=uc16, H=8 * V.H, W=8 * V.W, steps=S, scale=SCALE, seeds=seeds))
    assert not torch.equal(got, cp(c=c16, uc=uc16, H=8 * V.H, W=8 * V.W, steps=S, scale=SCALE, seeds=seeds))
    # img2img takes the hint too, through the same scope
    z0 = torch.tensor(np.random.RandomState(5).randn(V.B, 4, V.H, V.W).astype(np.float32), device=DEV)
    a = cp.img2img(init_latent=z0, strength=0.75, c=c16, uc=uc16, steps=S, scale=SCALE, seeds=seeds, control_image=hint[:1])
    b = cp.img2img(init_latent=z0, strength=0.75, c=c16, uc=uc16, steps=S, scale=SCALE, seeds=seeds)
    assert torch.isfinite(a).all() and not torch.equal(a, b)
    assert torch.equal(b, pipe.img2img(init_latent=z0, strength=0.75, c=c16, uc=uc16, steps=S, scale=SCALE, seeds=seeds))
