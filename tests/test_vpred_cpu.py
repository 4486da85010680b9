"""v-prediction (`parameterization: "v"`, the SD 2.x 768-v checkpoints) -- the parts that need no GPU: the
LatentDiffusion surface, the host-side argument checks of mdx_sampler_step_pred_f32, and the VModelOracle the GPU
trajectory tests compare against."""
import ctypes

import numpy as np
import pytest
import torch

import _vpred_util as V
from oracle import ldm as O


def _ldm(**kw):
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    return LatentDiffusion(object(), linear_start=0.00085, linear_end=0.0120, timesteps=1000, **kw)


def test_latent_diffusion_accepts_v_and_still_rejects_unknown():
    from minddiffusion_amd.configs import SD2_768V_LDM, SD2_LDM
    assert _ldm(parameterization="v").parameterization == "v"
    assert _ldm().parameterization == "eps" and _ldm(parameterization="x0").parameterization == "x0"
    with pytest.raises(AssertionError):
        _ldm(parameterization="score")
    assert SD2_768V_LDM == dict(SD2_LDM, parameterization="v", image_size=96)
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    m = LatentDiffusion(object(), **SD2_768V_LDM)
    assert (m.parameterization, m.image_size, m.scale_factor) == ("v", 96, SD2_LDM["scale_factor"])


@pytest.mark.parametrize("t", [0, 500, 999])
def test_v_helpers_invert_each_other(t):
    """x_t = a x0 + b n, v = a n - b x0  =>  a x_t - b v = (a^2 + b^2) x0 = x0 and a v + b x_t = n, to fp32 rounding
    (1e-5 relative, the bound test_sampler_step uses for the same kind of arithmetic)."""
    m = _ldm(parameterization="v")
    rng = np.random.RandomState(t)
    x0, n = torch.tensor(rng.randn(3, 4, 5, 7).astype(np.float32)), torch.tensor(rng.randn(3, 4, 5, 7).astype(np.float32))
    tt = torch.full((3,), t, dtype=torch.long)
    x_t, v = m.q_sample(x0, tt, n), m.get_v(x0, n, tt)
    a, b = float(m.sqrt_alphas_cumprod[t]), float(m.sqrt_one_minus_alphas_cumprod[t])
    np.testing.assert_allclose(v.numpy(), a * n.numpy() - b * x0.numpy(), rtol=1e-5, atol=1e-6)
    rel = lambda got, ref: float((got - ref).norm() / ref.norm())
    assert rel(m.predict_start_from_z_and_v(x_t, tt, v), x0) <= 1e-5
    assert rel(m.predict_eps_from_z_and_v(x_t, tt, v), n) <= 1e-5
    # a per-sample t vector picks per-sample coefficients
    t3 = torch.tensor([0, 500, 999])
    x3, v3 = m.q_sample(x0, t3, n), m.get_v(x0, n, t3)
    assert rel(m.predict_start_from_z_and_v(x3, t3, v3), x0) <= 1e-5
    assert rel(m.predict_eps_from_z_and_v(x3, t3, v3), n) <= 1e-5


def test_sampler_step_pred_argument_validation_without_gpu():
    """Every refusal of mdx_sampler_step_pred_f32 happens on the host, before any launch (error code + message)."""
    from minddiffusion_amd import _lib
    lib = _lib.load()
    coef = (ctypes.c_float * 4)(1.0, 0.0, 0.0, 0.0)
    P = 16     # any non-null address: nothing is dereferenced on the device before the checks pass

    def call(x=P, x_model=None, out_u=None, out_c=P, out_ld=8, pred=1, olds=(None, None, None), coef4=coef, sigma=0.0,
             noise=None, x_prev=P, C=4):
        c4 = None if coef4 is None else ctypes.cast(coef4, ctypes.c_void_p)
        return lib.mdx_sampler_step_pred_f32(x, x_model, out_u, out_c, out_ld, 1.0, pred, 0.8, 0.6, olds[0], olds[1],
                                             olds[2], c4, 0.5, 0.5, 0.5, 0.5, sigma, noise, None, x_prev, None, 2, C, 5, 7,
                                             None)

    def refused(msg, **kw):
        assert call(**kw) == -1
        err = lib.mdx_last_error()
        assert b"mdx_sampler_step_pred_f32" in err and msg in err, err

    refused(b"pred_type", pred=2)
    refused(b"pred_type", pred=-1)
    refused(b"null pointer", x=None)
    refused(b"null pointer", out_c=None)
    refused(b"null pointer", coef4=None)
    refused(b"null pointer", x_prev=None)
    refused(b"bad extents", out_ld=3)
    refused(b"needs a noise tensor", sigma=0.3)
    for k in (1, 2, 3):
        c = (ctypes.c_float * 4)(1.0, 0.0, 0.0, 0.0)
        c[k] = 0.5
        refused(b"without its eps history", coef4=c)
        refused(b"without its eps history", coef4=c, pred=0)
    # the old entry names itself in the same refusals
    assert lib.mdx_sampler_step_f32(P, None, P, 3, 1.0, None, None, None, ctypes.cast(coef, ctypes.c_void_p), 0.5, 0.5, 0.5,
                                    0.5, 0.0, None, None, P, None, 2, 4, 5, 7, None) == -1
    assert b"mdx_sampler_step_f32: bad extents" in lib.mdx_last_error()
    assert _lib.SIGNATURES["mdx_sampler_step_pred_f32"][1][6] is ctypes.c_int      # pred_type
    from minddiffusion_amd import ops
    assert (ops.PRED_EPS, ops.PRED_V) == (0, 1)


class _LinearUNet:
    """Stands in for the oracle UNet: any deterministic map will do for checking the wrapper's algebra."""

    def __call__(self, x, t, context=None, y=None):
        x = torch.as_tensor(x, dtype=torch.float32)
        return 0.3 * x.flip(-1) - 0.2 * x + 0.01 * torch.as_tensor(t, dtype=torch.float32).reshape(-1, 1, 1, 1) / 1000.0


def test_vmodel_oracle_one_ddim_step_is_the_closed_form():
    """O.sample's unchanged eps DDIM step on VModelOracle = sqrt(a_prev) (a x - b v) + sqrt(1 - a_prev) (a v + b x), float64."""
    om = V.VModelOracle(_LinearUNet())
    assert om.parameterization == "v"
    x = np.random.RandomState(0).randn(2, 4, 5, 7).astype(np.float32)
    got, inter = O.sample(om, 1, 2, (4, 5, 7), None, x, "ddim")
    t = int(O.make_ddim_timesteps(1, 1000)[0])
    v = om.raw_v(torch.tensor(x), torch.full((2,), t, dtype=torch.int64)).numpy().astype(np.float64)
    ac = np.asarray(om.alphas_cumprod, np.float64)
    a, b, a_prev = np.sqrt(ac[t]), np.sqrt(1.0 - ac[t]), ac[0]
    x64 = x.astype(np.float64)
    ref = np.sqrt(a_prev) * (a * x64 - b * v) + np.sqrt(1.0 - a_prev) * (a * v + b * x64)
    assert np.abs(got.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    np.testing.assert_allclose(inter["pred_x0"][-1].numpy(), a * x64 - b * v, rtol=0, atol=1e-5 * np.abs(ref).max())
    # a fractional model-input time takes (a, b) from NoiseScheduleVP at t / 1000 + 1 / 1000: on the grid both tables agree
    a_i, b_i = om.ab(torch.tensor([500]))
    a_f, b_f = om.ab(torch.tensor([500.0]))
    assert abs(float(a_i) - float(a_f)) <= 1e-6 and abs(float(b_i) - float(b_f)) <= 1e-6


@pytest.mark.parametrize("name", sorted(V.TRAJECTORIES))
def test_trajectory_cases_are_inside_the_bound_on_the_oracle_itself(name):
    """The GPU trajectory bound (rel-L2 <= 1e-2, max|d| <= 1e-2 max|ref|) is only meaningful for inputs on which the
    oracle's own fp32 and emulate_fp16() runs of the v case stay inside it; the seeds of _vpred_util were picked so."""
    from _util import metrics
    from minddiffusion_amd.configs import TINY_UNET
    cfg = dict(TINY_UNET, num_heads=-1)
    params = O.init_params(cfg, seed=V.TINY_SEED)
    om = V.VModelOracle(O.UNetOracle(cfg, params))
    ref = V.oracle_trajectory(name, om, cfg["context_dim"])
    with O.emulate_fp16():
        emu = V.oracle_trajectory(name, om, cfg["context_dim"])
    m = metrics(emu, ref)
    print("ORACLE_FP16_VS_FP32", name, m)
    assert m["finite"] and m["rel_l2"] <= 1e-2 and m["max_abs"] <= 1e-2 * m["ref_max"], m
