"""DiffusionPipeline.hires on the GPU, on the tiny UNet and tiny VAE the img2img tests use: base 64 x 64 -> 128 x 128 (latents
8 x 8 -> 16 x 16, the second pass on 8 x 8 windows), 4 steps, strength 0.5; and a 64 x 128 -> 64 x 256 wrap_x case.  Every
equality is torch.equal: hires is a composition of entry points that exist, and with seeds its one fused launch promises the
bits of the three it replaces.  (The tiny VAE downsamples by 2, not 8: a base latent of 8 x 8 decodes to 16 x 16 pixels, so the
callable-upscaler case, which has to see a [B, 3, 64, 64] image, starts from a 32 x 32 latent.)"""
import numpy as np
import pytest
import torch

import _vpred_util as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS, STRENGTH, SCALE = 4, 0.5, 3.0
SEEDS = [101, 2 ** 40 + 7, 5]


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def _with_vae(model):
    from oracle import vae as OV
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
    dd = dict(TINY_VAE_DDCONFIG)
    vae = AutoencoderKL(ddconfig=dd, embed_dim=4, device=DEV)
    vae.load_state_dict(OV.init_params(dd, seed=8))
    model.first_stage_model = vae
    return model


@pytest.fixture(scope="module")
def models():
    eps, cfg, _ = V.tiny_eps_model(scale_factor=0.18215)
    v, _, _ = V.tiny_eps_model(parameterization="v", scale_factor=0.18215)
    return {"eps": _with_vae(eps), "v": _with_vae(v), "ctx": cfg["context_dim"]}


def _cond(ctx_dim, B):
    rng = np.random.RandomState(41)
    c = torch.tensor(rng.randn(B, V.T, ctx_dim).astype(np.float32))
    uc = torch.tensor(np.repeat(rng.randn(1, V.T, ctx_dim).astype(np.float32), B, 0))
    return c, uc


def _pipe(model, kind):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    return DiffusionPipeline(model, kind, device=DEV)


@pytest.mark.parametrize("kind", ["ddim", "plms", "dpm_solver"])
def test_hires_is_the_hand_composition(models, ops, kind):
    """First pass == pipe(...); with seeds (the fused launch) and with seed= (ops.resample + stochastic_encode) the result is
    pipe(...) -> ops.resample -> second.img2img(init_latent=...)."""
    pipe = _pipe(models["eps"], kind)
    c, uc = _cond(models["ctx"], 2)
    second = pipe.windowed(window=64)
    for rnd in (dict(seeds=SEEDS[:2]), dict(seed=9)):
        kw = dict(c=c, uc=uc, steps=STEPS, scale=SCALE, **rnd)
        got, base = pipe.hires(H=128, W=128, base=(64, 64), upscaler="latent-bicubic", strength=STRENGTH, return_base=True, **kw)
        assert tuple(base.shape) == (2, 4, 8, 8) and tuple(got.shape) == (2, 4, 16, 16) and bool(torch.isfinite(got).all())
        zb = pipe(H=64, W=64, **kw)
        assert torch.equal(base, zb)
        z_up = ops.resample(zb, (16, 16), "bicubic")
        want = second.img2img(init_latent=z_up, strength=STRENGTH, **kw)
        assert torch.equal(got, want), (kind, rnd)
        # an explicit second pipeline, and hires_steps: the second pass on its own grid
        got8 = pipe.hires(H=128, W=128, base=(64, 64), strength=0.25, hires_steps=8, second=second, **kw)
        assert torch.equal(got8, second.img2img(init_latent=z_up, strength=0.25, **dict(kw, steps=8)))
    # the second pass did run on windows, and its pipeline is kept
    kept = pipe._hires_kept[(64, 64)]
    assert kept.model.evals > 0 and kept.model.window == (8, 8)
    assert not torch.equal(got, torch.zeros_like(got))


def test_hires_v_prediction_scale_list_and_guidance_rescale(models, ops):
    pipe = _pipe(models["v"], "ddim")
    c, uc = _cond(models["ctx"], 2)
    kw = dict(c=c, uc=uc, steps=STEPS, scale=[2.0, 4.5], guidance_rescale=0.7, seeds=SEEDS[:2])
    got, base = pipe.hires(H=128, W=128, base=(64, 64), upscaler="latent-bilinear", strength=STRENGTH, return_base=True, **kw)
    zb = pipe(H=64, W=64, **kw)
    assert torch.equal(base, zb)
    want = pipe.windowed(window=64).img2img(init_latent=ops.resample(zb, (16, 16), "bilinear"), strength=STRENGTH, **kw)
    assert torch.equal(got, want)
    assert not torch.equal(got, pipe.hires(H=128, W=128, base=(64, 64), upscaler="latent-bilinear", strength=STRENGTH,
                                           **dict(kw, guidance_rescale=0.0)))


@pytest.mark.parametrize("upscaler,mode", [("image-bicubic", "bicubic"), ("image-lanczos3", "lanczos3")])
def test_hires_image_modes_are_decode_clamp_resample_img2img(models, ops, upscaler, mode):
    model = models["eps"]
    pipe = _pipe(model, "ddim")
    c, uc = _cond(models["ctx"], 2)
    kw = dict(c=c, uc=uc, steps=STEPS, scale=SCALE, seeds=SEEDS[:2])
    got = pipe.hires(H=128, W=128, base=(64, 64), upscaler=upscaler, strength=STRENGTH, **kw)
    zb = pipe(H=64, W=64, **kw)
    img = torch.clamp(model.decode_first_stage(zb).to(torch.float32), -1.0, 1.0).contiguous()
    assert tuple(img.shape) == (2, 3, 16, 16)                       # (the tiny VAE's factor is 2)
    big = ops.resample(img, (32, 32), mode)
    want = pipe.windowed(window=64).img2img(init_image=big, strength=STRENGTH, **kw)
    assert tuple(got.shape) == (2, 4, 16, 16) and torch.equal(got, want)
    dec = pipe.hires(H=128, W=128, base=(64, 64), upscaler=upscaler, strength=STRENGTH, decode=True, **kw)
    assert tuple(dec.shape) == (2, 3, 32, 32) and float(dec.min()) >= 0.0 and float(dec.max()) <= 1.0


def test_hires_callable_upscaler_is_called_once_with_the_decoded_image(models, ops):
    pipe = _pipe(models["eps"], "ddim")
    c, uc = _cond(models["ctx"], 1)
    calls = []

    def up(img):
        calls.append(tuple(img.shape))
        assert img.is_cuda and img.dtype == torch.float32 and float(img.min()) >= -1.0 and float(img.max()) <= 1.0
        return ops.resample(img, (128, 128), "bilinear")
    kw = dict(c=c, uc=uc, steps=STEPS, scale=SCALE, seeds=SEEDS[:1])
    got = pipe.hires(H=512, W=512, base=(256, 256), upscaler=up, strength=STRENGTH, second=pipe, **kw)
    assert calls == [(1, 3, 64, 64)] and tuple(got.shape) == (1, 4, 64, 64)
    zb = pipe(H=256, W=256, **kw)
    img = torch.clamp(models["eps"].decode_first_stage(zb).to(torch.float32), -1.0, 1.0).contiguous()
    assert torch.equal(got, pipe.img2img(init_image=ops.resample(img, (128, 128), "bilinear"), strength=STRENGTH, **kw))
    from minddiffusion_amd._lib import MdxError
    with pytest.raises(MdxError, match="upscaler returned"):
        pipe.hires(H=512, W=512, base=(256, 256), upscaler=lambda img: img, strength=STRENGTH, second=pipe, **kw)


def test_hires_seed_isolation(models):
    """Row b of a batch of 3 is the same request run alone, bit for bit: what every seeded entry point promises."""
    pipe = _pipe(models["eps"], "ddim")
    c, uc = _cond(models["ctx"], 3)
    kw = dict(H=128, W=128, base=(64, 64), steps=STEPS, scale=SCALE, strength=STRENGTH, eta=0.5)
    for upscaler in ("latent-bicubic", "image-bicubic"):
        whole = pipe.hires(c=c, uc=uc, seeds=SEEDS, upscaler=upscaler, **kw)
        for b in range(3):
            alone = pipe.hires(c=c[b:b + 1], uc=uc[b:b + 1], seeds=SEEDS[b:b + 1], upscaler=upscaler, **kw)
            assert torch.equal(whole[b:b + 1], alone), (upscaler, b)
    assert not torch.equal(whole[0], whole[1])


def test_hires_on_a_wrap_x_pipeline(models, ops):
    """64 x 128 -> 64 x 256 on pipe.windowed(window=64, wrap_x=True): the first pass on the inner model, the upscale wrapped --
    rolling the base latent by k columns rolls the upscaled one by 2 k -- and the second pass on the panorama's windows."""
    pipe = _pipe(models["eps"], "ddim")
    pano = pipe.windowed(window=64, wrap_x=True)
    c, uc = _cond(models["ctx"], 1)
    kw = dict(c=c, uc=uc, steps=STEPS, scale=SCALE, seeds=SEEDS[:1])
    got, base = pano.hires(H=64, W=256, base=(64, 128), strength=STRENGTH, return_base=True, **kw)
    assert tuple(base.shape) == (1, 4, 8, 16) and tuple(got.shape) == (1, 4, 8, 32) and bool(torch.isfinite(got).all())
    assert torch.equal(base, pipe(H=64, W=128, **kw))                # the inner, un-windowed model
    up = pano.upscale_latent(base, 64, 256)
    assert torch.equal(up, ops.resample(base, (8, 32), "bicubic", wrap_x=True))
    for k in (1, 5):
        assert torch.equal(pano.upscale_latent(torch.roll(base, k, -1), 64, 256), torch.roll(up, 2 * k, -1))
    assert not torch.equal(up, pipe.upscale_latent(base, 64, 256))   # a pipeline that does not wrap replicates the edge
    assert torch.equal(got, pano.img2img(init_latent=up, strength=STRENGTH, **kw))
    assert pano.model.evals > 0
