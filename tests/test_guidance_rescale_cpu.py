"""Guidance rescale (`guidance_rescale`, CFG rescale of the SD 2.x samplers) -- the parts that need no GPU: the host-side
refusals of mdx_sampler_step_rescale_f32, the RescaleModelOracle the GPU trajectory tests compare against, and the keyword
validation of the samplers and the pipeline."""
import ctypes

import numpy as np
import pytest
import torch

import _rescale_util as R
import _vpred_util as V
from oracle import ldm as O


def test_sampler_step_rescale_argument_validation_without_gpu():
    """Every refusal of mdx_sampler_step_rescale_f32 happens on the host, before any launch (error code + message)."""
    from minddiffusion_amd import _lib
    lib = _lib.load()
    coef = (ctypes.c_float * 4)(1.0, 0.0, 0.0, 0.0)
    P = 16     # any non-null address: nothing is dereferenced on the device before the checks pass

    def call(x=P, out_u=P, out_c=P, out_ld=8, pred=1, coef4=coef, sigma=0.0, x_prev=P, phi=0.7, C=4, H=5, W=7):
        c4 = None if coef4 is None else ctypes.cast(coef4, ctypes.c_void_p)
        return lib.mdx_sampler_step_rescale_f32(x, None, out_u, out_c, out_ld, 7.5, pred, 0.8, 0.6, None, None, None, c4,
                                                0.5, 0.5, 0.5, 0.5, sigma, None, None, x_prev, None, phi, None, 2, C, H, W,
                                                None)

    def refused(msg, **kw):
        assert call(**kw) == -1
        err = lib.mdx_last_error()
        assert b"mdx_sampler_step_rescale_f32" in err and msg in err, err

    for phi in (-0.1, 1.5, float("nan"), float("inf")):
        refused(b"guidance_rescale", phi=phi)
        refused(b"guidance_rescale", phi=phi, out_u=None)        # also where no rescale kernel would be launched
    refused(b"C * H * W >= 2", C=1, H=1, W=1)
    refused(b"C * H * W >= 2", C=1, H=1, W=1, phi=0.0)
    # inherited from the entry it extends
    refused(b"pred_type", pred=2)
    refused(b"null pointer", x=None)
    refused(b"null pointer", out_c=None)
    refused(b"null pointer", coef4=None)
    refused(b"null pointer", x_prev=None)
    refused(b"bad extents", out_ld=3)
    refused(b"needs a noise tensor", sigma=0.3)
    c = (ctypes.c_float * 4)(1.0, 0.5, 0.0, 0.0)
    refused(b"without its eps history", coef4=c)
    refused(b"without its eps history", coef4=c, phi=0.0)
    sig = _lib.SIGNATURES["mdx_sampler_step_rescale_f32"][1]
    assert sig[:22] == _lib.SIGNATURES["mdx_sampler_step_pred_f32"][1][:22]
    assert sig[22] is ctypes.c_float and sig[23] is ctypes.c_void_p      # guidance_rescale, factor_out


class _LinearUNet:
    """Stands in for the oracle UNet: a deterministic map whose conditional and unconditional outputs differ in shape (not
    only in size), so that std(out_c) / std(m) is not trivially 1 / scale."""

    def __call__(self, x, t, context=None, y=None):
        x = torch.as_tensor(x, dtype=torch.float32)
        g = torch.as_tensor(context, dtype=torch.float32).mean(dim=(1, 2)).reshape(-1, 1, 1, 1)
        return (0.3 * x.flip(-1) - 0.2 * x + g * x.flip(-2)
                + 0.01 * torch.as_tensor(t, dtype=torch.float32).reshape(-1, 1, 1, 1) / 1000.0)


def _linear_inputs():
    rng = np.random.RandomState(0)
    x = rng.randn(2, 4, 5, 7).astype(np.float32)
    c = (0.4 + 0.1 * rng.randn(2, 3, 6)).astype(np.float32)
    uc = np.repeat((-0.2 + 0.1 * rng.randn(1, 3, 6)).astype(np.float32), 2, 0)
    return x, c, uc


@pytest.mark.parametrize("v", [False, True])
def test_rescale_oracle_one_ddim_step_is_the_closed_form(v):
    net, scale, phi = _LinearUNet(), 3.0, 0.7
    base = V.VModelOracle(net) if v else O.ModelOracle(net)
    om = R.RescaleModelOracle(base, phi, scale, 2)
    x, c, uc = _linear_inputs()
    got, inter = O.sample(om, 1, 2, (4, 5, 7), c, x, "ddim", unconditional_guidance_scale=scale,
                          unconditional_conditioning=uc)
    t = int(O.make_ddim_timesteps(1, 1000)[0])
    tt = torch.full((2,), t, dtype=torch.int64)
    f64 = lambda a: np.asarray(a, np.float64)
    o_u, o_c = f64(net(x, tt, uc)), f64(net(x, tt, c))
    m = o_u + scale * (o_c - o_u)
    s_c = o_c.reshape(2, -1).std(axis=1, ddof=1)
    s_m = m.reshape(2, -1).std(axis=1, ddof=1)
    f = phi * s_c / s_m + (1 - phi)
    assert np.all(np.abs(f - 1) > 0.05) and abs(f[0] - f[1]) > 1e-3, f     # the factor does something, per sample
    np.testing.assert_allclose(om.factors[0], f, rtol=1e-6)
    m = f.reshape(2, 1, 1, 1) * m
    ac = f64(om.alphas_cumprod)
    a, b, a_prev = np.sqrt(ac[t]), np.sqrt(1.0 - ac[t]), ac[0]
    e = a * m + b * f64(x) if v else m
    p = (f64(x) - b * e) / a
    ref = np.sqrt(a_prev) * p + np.sqrt(1.0 - a_prev) * e
    assert np.abs(got.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    assert np.abs(inter["pred_x0"][-1].numpy() - p).max() <= 1e-5 * np.abs(ref).max()


def test_rescale_oracle_phi_one_restores_the_conditional_std_and_phi_zero_is_the_plain_oracle():
    net, scale = _LinearUNet(), 7.5
    x, c, uc = _linear_inputs()
    tt = torch.full((4,), 500, dtype=torch.int64)
    x2, c2 = torch.tensor(np.concatenate([x, x])), torch.tensor(np.concatenate([uc, c]))
    om = R.RescaleModelOracle(O.ModelOracle(net), 1.0, scale, 2)
    m2 = om.apply_model(x2, tt, c2)
    assert torch.equal(m2[:2], m2[2:])
    s_m = m2[2:].double().reshape(2, -1).std(dim=1)                                  # torch.std is unbiased
    s_c = net(x, tt[:2], c).double().reshape(2, -1).std(dim=1)
    assert float(((s_m - s_c).abs() / s_c).max()) <= 1e-6
    # an undoubled batch is not a guidance batch: untouched
    assert torch.equal(om.apply_model(torch.tensor(x), tt[:2], torch.tensor(c)), net(x, tt[:2], c))
    for v in (False, True):
        base = V.VModelOracle(net) if v else O.ModelOracle(net)
        kw = dict(unconditional_guidance_scale=scale, unconditional_conditioning=uc)
        want, _ = O.sample(base, 4, 2, (4, 5, 7), c, x, "plms", **kw)
        got, _ = O.sample(R.RescaleModelOracle(base, 0.0, scale, 2), 4, 2, (4, 5, 7), c, x, "plms", **kw)
        if not v:
            assert torch.equal(got, want)
        else:   # a (u + s (c - u)) + b x instead of (a u + b x) + s ((a c + b x) - (a u + b x)): equal up to fp32 rounding
            assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.fixture(scope="module")
def tiny_bases():
    from minddiffusion_amd.configs import TINY_UNET
    cfg = dict(TINY_UNET, num_heads=-1)
    net = O.UNetOracle(cfg, O.init_params(cfg, seed=V.TINY_SEED))
    return {"v": V.VModelOracle(net), "eps": O.ModelOracle(net)}, cfg


@pytest.fixture(scope="module")
def unrescaled(tiny_bases):
    bases, cfg = tiny_bases
    cache = {}

    def get(kind, name):
        if (kind, name) not in cache:
            cache[kind, name] = V.oracle_trajectory(name, bases[kind], cfg["context_dim"])
        return cache[kind, name]
    return get


@pytest.mark.parametrize("phi", R.PHIS)
@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("kind", ["v", "eps"])
def test_rescaled_cases_are_inside_the_bound_on_the_oracle_itself(tiny_bases, unrescaled, kind, name, phi):
    """The GPU trajectory bound (rel-L2 <= 1e-2, max|d| <= 1e-2 max|ref|) is only meaningful for inputs on which the
    oracle's own fp32 and emulate_fp16() runs of the rescaled case stay inside it (_vpred_util's seeds do), and only
    discriminates if the rescaled end point is far from the unrescaled one."""
    from _util import metrics
    bases, cfg = tiny_bases
    ref = R.oracle_trajectory(name, bases[kind], cfg["context_dim"], phi)
    with O.emulate_fp16():
        emu = R.oracle_trajectory(name, bases[kind], cfg["context_dim"], phi)
    m = metrics(emu, ref)
    far = metrics(unrescaled(kind, name), ref)["rel_l2"]
    print("ORACLE_FP16_VS_FP32", kind, name, phi, m, "unrescaled_rel_l2", far)
    assert m["finite"] and m["rel_l2"] <= 1e-2 and m["max_abs"] <= 1e-2 * m["ref_max"], m
    assert far > 0.1, far


def _ldm(**kw):
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    return LatentDiffusion(object(), linear_start=0.00085, linear_end=0.0120, timesteps=1000, **kw)


@pytest.mark.parametrize("bad", [1.5, -0.1, float("nan")])
def test_samplers_and_pipeline_refuse_a_guidance_rescale_outside_0_1(bad):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model = _ldm(parameterization="v")
    c = torch.zeros(2, 3, 8)
    for cls in (DDIMSampler, PLMSSampler, DPMSolverSampler):
        with pytest.raises(ValueError, match="guidance_rescale"):
            cls(model).sample(2, 2, (4, 8, 8), conditioning=c, verbose=False, guidance_rescale=bad)
    for cls in (DDIMSampler, PLMSSampler):
        with pytest.raises(ValueError, match="guidance_rescale"):
            cls(model).plms_sampling(c, (2, 4, 8, 8), verbose=False, guidance_rescale=bad)
    with pytest.raises(ValueError, match="guidance_rescale"):
        DiffusionPipeline(model, "ddim", device="cpu")(c=c, uc=c, H=64, W=64, steps=2, guidance_rescale=bad)
