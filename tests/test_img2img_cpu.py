"""img2img -- the parts that need no GPU: the host-side argument checks of mdx_q_sample_f32 / mdx_vae_encode_noised_f32, the
t_enc / t_start arithmetic and refusals of stochastic_encode / decode / DiffusionPipeline.img2img, and the oracle side of the
partial runs the GPU trajectory tests compare against (tests/_img2img_util.py)."""
import ctypes

import numpy as np
import pytest
import torch

import _img2img_util as I
import _vpred_util as V
from oracle import ldm as O


def _ldm(**kw):
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    return LatentDiffusion(object(), linear_start=0.00085, linear_end=0.0120, timesteps=1000, **kw)


def test_q_sample_argument_validation_without_gpu():
    """Every refusal of mdx_q_sample_f32 happens on the host, before any launch (error code + message)."""
    from minddiffusion_amd import _lib
    lib = _lib.load()
    n = 2 * 4 * 35 * 4                     # bytes of one [2, 4, 5, 7] fp32 tensor
    X0, NZ, MK, IM, OUT = (4096 + k * 2 * n for k in range(5))   # disjoint non-null addresses: nothing is dereferenced

    def call(x0=X0, noise=NZ, mask=None, mask_c=0, img=None, out=OUT, B=2, C=4, HW=35):
        return lib.mdx_q_sample_f32(x0, noise, 0.8, 0.6, mask, mask_c, img, out, B, C, HW, None)

    def refused(msg, **kw):
        assert call(**kw) == -1
        err = lib.mdx_last_error()
        assert b"mdx_q_sample_f32" in err and msg in err, err

    refused(b"null pointer", x0=None)
    refused(b"null pointer", noise=None)
    refused(b"null pointer", out=None)
    refused(b"mask needs img", mask=MK, mask_c=1)
    for mc in (0, 2, 3, 5, -1):
        refused(b"mask_c must be 1 or C", mask=MK, mask_c=mc, img=IM)
    refused(b"bad extents", B=0)
    refused(b"bad extents", C=0)
    refused(b"bad extents", HW=-3)
    # out may be img itself, and overlap nothing else
    refused(b"may alias img", out=X0)
    refused(b"may alias img", out=NZ + 16)
    refused(b"may alias img", mask=MK, mask_c=4, img=IM, out=MK)
    refused(b"may alias img", mask=MK, mask_c=1, img=IM, out=IM + 4)
    assert _lib.SIGNATURES["mdx_q_sample_f32"][1][5] is ctypes.c_int       # mask_c


def test_vae_encode_noised_argument_validation_without_gpu():
    from minddiffusion_amd import _lib
    lib = _lib.load()
    P = 4096

    def call(mom=P, ld=8, noise=2 * P, z0=3 * P, xt=4 * P, B=2, zc=4, HW=35):
        return lib.mdx_vae_encode_noised_f32(mom, ld, None, 0.18215, 0.8, 0.6, noise, z0, xt, B, zc, HW, None)

    def refused(msg, **kw):
        assert call(**kw) == -1
        err = lib.mdx_last_error()
        assert b"mdx_vae_encode_noised_f32" in err and msg in err, err

    refused(b"null pointer", mom=None)
    refused(b"bad extents", ld=7)
    refused(b"bad extents", B=0)
    refused(b"bad extents", zc=0)
    refused(b"bad extents", HW=0)
    refused(b"no output", z0=None, xt=None)
    refused(b"needs a noise tensor", noise=None)
    refused(b"different tensors", z0=P * 3, xt=P * 3)


# ------------------------------------------------------------------------------------------------ samplers: arithmetic, refusals
def _samplers(model):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    return DDIMSampler(model), PLMSSampler(model)


def test_q_coefficients_are_the_level_of_the_first_step_that_runs():
    model = _ldm()
    ac = np.asarray(model.alphas_cumprod, np.float64)
    for s in _samplers(model):
        s.make_schedule(10, verbose=False)
        for t_enc in (1, 5, 10):
            a, b = s.q_coefficients(t_enc)
            t = int(s.ddim_timesteps[t_enc - 1])
            assert np.float32(s.ddim_alphas[t_enc - 1]) == np.float32(ac[t])
            assert abs(a - np.sqrt(ac[t])) <= 1e-6 and abs(b - np.sqrt(1 - ac[t])) <= 1e-6
        a, b = s.q_coefficients(10)          # strength 1: the top of the grid, not an index past it
        assert int(s.ddim_timesteps[9]) == 901 and abs(a * a + b * b - 1.0) <= 1e-6
        a, b = s.q_coefficients(37, use_original_steps=True)
        assert abs(a - np.sqrt(ac[36])) <= 1e-6
        for bad in (0, 11, -1, 2.5, True):
            with pytest.raises(ValueError, match="t_start"):
                s.q_coefficients(bad)
        with pytest.raises(ValueError, match="t_start"):
            s.q_coefficients(1001, use_original_steps=True)


def test_stochastic_encode_and_decode_need_a_schedule_and_a_valid_t_start():
    from minddiffusion_amd._lib import MdxError
    model = _ldm()
    x = torch.zeros(1, 4, 8, 8)
    for s in _samplers(model):
        with pytest.raises(MdxError, match="make_schedule"):
            s.stochastic_encode(x, 3)
        with pytest.raises(MdxError, match="make_schedule"):
            s.decode(x, None, 3)
        s.make_schedule(5, verbose=False)
        for bad in (0, 6):
            with pytest.raises(ValueError, match="t_start"):
                s.stochastic_encode(x, bad)
            with pytest.raises(ValueError, match="t_start"):
                s.decode(x, None, bad)
        with pytest.raises(MdxError, match="CUDA"):
            s.stochastic_encode(x, 3)                     # no CPU fallback
        with pytest.raises(TypeError, match="unexpected"):
            s.decode(x, None, 3, eta=0.5)


def test_dpm_solver_t_start_plan_and_refusals():
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP, multistep_2m_plan
    model = _ldm()
    ns = NoiseScheduleVP("discrete", alphas_cumprod=np.asarray(model.alphas_cumprod, np.float64))
    full = multistep_2m_plan(ns, 10)
    assert multistep_2m_plan(ns, 10, t_start=1.0) == full and multistep_2m_plan(ns, 10, t_start=None) == full
    # the last 6 of the 10-step grid's own intervals
    part = multistep_2m_plan(ns, 6, t_start=I.dpm_t_start(10, 6))
    np.testing.assert_allclose([p["t"] for p in part], [p["t"] for p in full[4:]], rtol=0, atol=1e-12)
    np.testing.assert_allclose(part[-1]["t_next"], 1e-3, rtol=0, atol=1e-15)
    assert part[0]["order"] == 1 and part[1]["order"] == 2
    one = multistep_2m_plan(ns, 1, order=1, t_start=I.dpm_t_start(8, 1))
    assert len(one) == 1 and one[0]["order"] == 1 and one[0]["c1"] == 0.0
    s = DPMSolverSampler(model)
    a, b = s.q_coefficients(0.6004)
    assert abs(a - float(ns.marginal_alpha(0.6004))) <= 1e-12 and abs(a * a + b * b - 1.0) <= 1e-9
    for bad in (0.0, 1e-3, 1.0001, -0.5):
        with pytest.raises(ValueError, match="t_start"):
            s.q_coefficients(bad)
        with pytest.raises(ValueError, match="t_start"):
            s.sample(3, 1, (4, 8, 8), conditioning=torch.zeros(1, 7, 64), t_start=bad)
    with pytest.raises(NotImplementedError):
        s.sample(3, 1, (4, 8, 8), conditioning=torch.zeros(1, 7, 64), t_start=0.5, mask=torch.ones(1, 1, 8, 8),
                 x0=torch.zeros(1, 4, 8, 8))


# ------------------------------------------------------------------------------------------------ pipeline refusals
def _pipe(sampler):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    return DiffusionPipeline(_ldm(), sampler, device="cpu")


def test_img2img_refusals(monkeypatch):
    from minddiffusion_amd import distributed
    from minddiffusion_amd._lib import MdxError
    lat, img = torch.zeros(1, 4, 8, 8), torch.zeros(1, 3, 16, 16)
    c = torch.zeros(1, 7, 64)
    for sampler in ("ddim", "plms", "dpm_solver"):
        p = _pipe(sampler)
        for bad in (0.0, -0.1, 1.01, float("nan")):
            with pytest.raises(ValueError, match="strength"):
                p.img2img(init_latent=lat, strength=bad, c=c)
        with pytest.raises(ValueError, match="strength"):
            p.img2img(init_latent=lat, strength=0.01, steps=50, c=c)        # t_enc = int(0.5) = 0
        with pytest.raises(ValueError, match="exactly one"):
            p.img2img(c=c)
        with pytest.raises(ValueError, match="exactly one"):
            p.img2img(init_image=img, init_latent=lat, c=c)
        with pytest.raises(ValueError, match="guidance_rescale"):
            p.img2img(init_latent=lat, c=c, guidance_rescale=1.5)
        with pytest.raises(MdxError, match="prompts"):
            p.img2img(init_latent=lat)
    with pytest.raises(NotImplementedError, match="mask"):
        _pipe("dpm_solver").img2img(init_latent=lat, c=c, mask=torch.ones(1, 1, 8, 8))
    with pytest.raises(MdxError, match="first_stage_model"):
        _pipe("ddim").img2img(init_image=img, c=c)                           # no VAE attached
    monkeypatch.setattr(distributed, "world", lambda: (0, 2))
    with pytest.raises(MdxError, match="single rank"):
        _pipe("ddim").img2img(init_latent=lat, c=c)


@pytest.mark.parametrize("strength,steps,t_enc", [(0.75, 50, 37), (1.0, 50, 50), (0.5, 5, 2), (0.3, 10, 3), (0.02, 50, 1)])
def test_img2img_t_enc_arithmetic(monkeypatch, strength, steps, t_enc):
    """t_enc = int(strength * steps) reaches the sampler as stochastic_encode's t_enc (DPM-Solver: as the continuous time the
    last t_enc of `steps` uniform intervals start at)."""
    seen = {}

    class Stop(Exception):
        pass

    def spy(self, x0, t, noise=None, **kw):
        seen["t"], seen["noise"] = t, noise
        raise Stop
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import _SamplerBase
    monkeypatch.setattr(_SamplerBase, "stochastic_encode", spy)
    monkeypatch.setattr(DPMSolverSampler, "stochastic_encode", spy)
    lat, c = torch.zeros(1, 4, 8, 8), torch.zeros(1, 7, 64)
    for sampler in ("ddim", "plms", "dpm_solver"):
        with pytest.raises(Stop):
            _pipe(sampler).img2img(init_latent=lat, strength=strength, steps=steps, c=c, seed=5)
        if sampler == "dpm_solver":
            assert abs(seen["t"] - (1e-3 + 0.999 * t_enc / steps)) <= 1e-12
        else:
            assert seen["t"] == t_enc
        # the forward-process draw is RandomState(seed), as start_noise()
        assert np.array_equal(seen["noise"].numpy(), np.random.RandomState(5).randn(1, 4, 8, 8).astype(np.float32))


# ------------------------------------------------------------------------------------------------ oracle side of the partial runs
def test_partial_dpm_solver_with_t_start_T_is_the_oracles_own_sample():
    from oracle import dpm_solver as OD
    from minddiffusion_amd.configs import TINY_UNET
    params = O.init_params(dict(TINY_UNET, num_heads=-1), seed=V.TINY_SEED)
    om = I.oracle_model("eps", TINY_UNET, params)
    x_T, c, uc = V.tiny_inputs(TINY_UNET["context_dim"])
    ref, _ = OD.sample(om, 4, V.B, I.SHAPE, c, x_T, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    ns = OD.NoiseScheduleVP("discrete", alphas_cumprod=om.alphas_cumprod)
    fn = OD.model_wrapper(lambda x, t, cc: om.apply_model(x, t, cc), ns, torch.tensor(c), torch.tensor(uc), 3.0)
    got = I.PartialDPMSolver(fn, ns).sample(torch.tensor(x_T), steps=4, t_start=1.0)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("name", sorted(I.CASES))
def test_partial_run_cases_are_inside_the_bound_on_the_oracle_itself(name):
    """The GPU trajectory bound (rel-L2 <= 1e-2, max|d| <= 1e-2 max|ref|) is only meaningful for cases on which the oracle's
    own fp32 and emulate_fp16() runs stay inside it.  oracle_partial also asserts that the reference's prefix rule keeps
    exactly t_enc steps and that the model is called t_enc (DDIM, DPM-Solver) / t_enc + 1 (PLMS) times."""
    from _util import metrics
    from minddiffusion_amd.configs import TINY_UNET
    params = O.init_params(dict(TINY_UNET, num_heads=-1), seed=V.TINY_SEED)
    om = I.oracle_model(I.CASES[name][0], TINY_UNET, params)
    ref = I.oracle_partial(name, om, TINY_UNET["context_dim"])
    with O.emulate_fp16():
        emu = I.oracle_partial(name, om, TINY_UNET["context_dim"])
    m = metrics(emu, ref)
    print("ORACLE_FP16_VS_FP32", name, m)
    assert m["finite"] and m["rel_l2"] <= 1e-2 and m["max_abs"] <= 1e-2 * m["ref_max"], m
