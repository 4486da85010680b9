"""AutoencoderKL.enable_tiling and DiffusionPipeline.enable_vae_tiling on the GPU, on the tiny VAE (factor 2): forwarding of a
canvas that fits one tile, the tiled decode as the numpy blend of an untiled VAE's decode of the same tile batches (bit for
bit, chunk padding included, wrapped or not), tiled decode and encode against the float64 blend of per-tile oracle results at
the tiny VAE's own tolerances, the distance to the global decode (logged, not bounded: GroupNorm sees one tile by design), and
the pipeline wiring.

Tolerances: test_vae_gpu.py's for the tiny decoder and encoder, rel-L2 <= 5e-3 and max|d| <= 5e-2 -- a blend is a convex
combination of per-tile results, so it cannot exceed the per-tile max-abs bound; the encoder's moments are additionally rounded
to fp16 once more after the average, half an fp16 ulp (2^-11 relative) on values of order 1, far inside the bound."""
import numpy as np
import pytest
import torch

import _tile_util as T
import _vpred_util as V
from _util import check
from oracle import vae as OV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE, OVERLAP, F = 16, 4, 2             # latent pixels; F: the tiny VAE's image pixels per latent pixel
STRIDE = TILE - OVERLAP
SEED = 8


def _dd():
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    return dict(TINY_VAE_DDCONFIG)


def _vae():
    from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
    vae = AutoencoderKL(ddconfig=_dd(), embed_dim=4, device=DEV)
    vae.load_state_dict(OV.init_params(_dd(), seed=SEED))
    return vae


@pytest.fixture(scope="module")
def params():
    return OV.init_params(_dd(), seed=SEED)


@pytest.fixture(scope="module")
def plain():
    """An untiled VAE on the same parameters: the reference's decoder and encoder calls."""
    return _vae()


def _latent(shape=(2, 4, 16, 40), seed=21):
    return torch.tensor(np.random.RandomState(seed).randn(*shape).astype(np.float32), device=DEV)


def _grid(h, w, wrap):
    """(oy, ox, th, tw) of the latent canvas h x w, restated: a tile larger than the canvas becomes its extent."""
    th, tw = min(TILE, h), min(TILE, w)
    return T.offsets(h, th, min(STRIDE, h)), T.offsets(w, tw, min(STRIDE, w), wrap and w > tw), th, tw


def _decode_ref(plain, z, m, wrap=False, mode="raw"):
    """The composition: torch slicing, the untiled VAE's decode on chunks of exactly m tiles, the numpy blend."""
    _, _, h, w = z.shape
    oy, ox, th, tw = _grid(h, w, wrap)
    tiles = T.run_chunks(plain.decode, T.gather_ref(z, oy, ox, th, tw), m)
    ref, _ = T.blend_ref(tiles.cpu().numpy(), [F * o for o in oy], [F * o for o in ox], F * h, F * w, F * OVERLAP, F * OVERLAP,
                         mode)
    return torch.from_numpy(ref)


# ------------------------------------------------------------------------------------------------ forwarding
def test_a_canvas_that_fits_one_tile_takes_the_plain_path(plain):
    vae = _vae().enable_tiling(tile=TILE, overlap=OVERLAP)
    for shape in ((2, 4, 16, 16), (1, 4, 8, 12)):
        z = _latent(shape, seed=3)
        want = plain.decode(z)
        assert torch.equal(vae.decode(z), want) and torch.equal(vae.decode(z, wrap_x=True), want)
        assert torch.equal(vae.decode_unit(z), torch.clamp((want + 1.0) / 2.0, 0.0, 1.0))
        x = torch.clamp(want, -1.0, 1.0).contiguous()
        assert torch.equal(vae.encode(x, sample=False), plain.encode(x, sample=False))
    assert sorted(vae.decoder._plans) == [(1, 8, 12), (2, 16, 16)]        # the plain plans, at the canvas' own batch
    off = _vae()
    assert torch.equal(off.decode_unit(z), torch.clamp((plain.decode(z) + 1.0) / 2.0, 0.0, 1.0))


# ------------------------------------------------------------------------------------------------ composition, bit for bit
@pytest.mark.parametrize("wrap,m", [(False, 6), (False, 4), (True, 8), (True, 3)])
def test_tiled_decode_is_the_blend_of_the_tile_decodes(plain, wrap, m):
    """z [2, 4, 16, 40]: 3 tiles per row (4 wrapped), 6 (8) in all.  m = 6 / 8: one chunk, no padding; m = 4: chunks of 4 and
    2 + 2 repeats; m = 3 on 8 tiles: 3, 3 and 2 + 1 repeat."""
    vae = _vae().enable_tiling(tile=TILE, overlap=OVERLAP, max_tile_batch=m)
    z = _latent()
    oy, ox, _, _ = _grid(16, 40, wrap)
    assert 2 * len(oy) * len(ox) == (8 if wrap else 6)
    got = vae.decode(z, wrap_x=wrap)
    assert tuple(got.shape) == (2, 3, 32, 80)
    assert torch.equal(got.cpu(), _decode_ref(plain, z, m, wrap))
    unit = vae.decode_unit(z, wrap_x=wrap)
    assert torch.equal(unit.cpu(), _decode_ref(plain, z, m, wrap, "unit")) and torch.equal(unit, torch.clamp((got + 1.0) / 2.0, 0.0, 1.0))
    # a second canvas size and batch: the same single plan
    z2 = _latent((1, 4, 24, 32), seed=22)
    got2 = vae.decode(z2, wrap_x=wrap)
    assert tuple(got2.shape) == (1, 3, 48, 64) and torch.equal(got2.cpu(), _decode_ref(plain, z2, m, wrap))
    assert list(vae.decoder._plans) == [(m, TILE, TILE)]
    assert not torch.equal(got, plain.decode(z))                          # (tiling is not the global decode)


def test_wrap_differs_from_the_clamped_grid_only_by_its_grid(plain):
    vae = _vae().enable_tiling(tile=TILE, overlap=OVERLAP)
    z = _latent()
    assert not torch.equal(vae.decode(z, wrap_x=True), vae.decode(z))


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("wrap", [False, True])
def test_tiled_decode_vs_the_float64_blend_of_oracle_tiles(params, wrap):
    vae = _vae().enable_tiling(tile=TILE, overlap=OVERLAP, max_tile_batch=4)
    z = _latent()
    oy, ox, th, tw = _grid(16, 40, wrap)
    tiles = OV.decode(params, T.gather_ref(z.cpu(), oy, ox, th, tw), _dd()).numpy()
    ref = T.blend_ref64(tiles, [F * o for o in oy], [F * o for o in ox], 32, 80, F * OVERLAP, F * OVERLAP)
    check(f"tiled_vae_decode_wrap{int(wrap)}", vae.decode(z, wrap_x=wrap), ref, rel_l2=5e-3, max_abs=5e-2)


@pytest.mark.parametrize("wrap", [False, True])
def test_tiled_encode_vs_the_float64_mean_of_oracle_moments(params, wrap):
    vae = _vae().enable_tiling(tile=TILE, overlap=OVERLAP, max_tile_batch=4)
    rng = np.random.RandomState(31)
    x = torch.tensor(np.clip(rng.randn(2, 3, 32, 80) * 0.5, -1, 1).astype(np.float32))
    noise = rng.randn(2, 4, 16, 40).astype(np.float32)
    oy, ox, th, tw = _grid(16, 40, wrap)
    img_tiles = T.gather_ref(x, [F * o for o in oy], [F * o for o in ox], F * th, F * tw)
    mom = T.blend_ref64(OV.encode_moments(params, img_tiles, _dd()).numpy(), oy, ox, 16, 40, OVERLAP, OVERLAP)
    mean, logvar = mom[:, :4], np.clip(mom[:, 4:], -30.0, 20.0)
    xd = x.to(DEV)
    tag = f"tiled_vae_encode_wrap{int(wrap)}"
    mode = vae.encode(xd, sample=False, wrap_x=wrap)
    assert tuple(mode.shape) == (2, 4, 16, 40)
    check(tag + "_mode", mode, mean, rel_l2=5e-3, max_abs=5e-2)
    got = vae.encode(xd, noise=torch.tensor(noise, device=DEV), wrap_x=wrap)
    check(tag + "_sampled", got, mean + np.exp(0.5 * logvar) * noise, rel_l2=5e-3, max_abs=5e-2)
    # the three encode entries share the moments: z0 of encode_noised and the latent channels of encode_concat
    z0, xt = vae.encode_noised(xd, 0.5, 0.8, 0.6, torch.tensor(noise, device=DEV), sample=False, wrap_x=wrap)
    check(tag + "_noised_z0", z0, 0.5 * mean, rel_l2=5e-3, max_abs=5e-2)
    cc = vae.encode_concat(xd, torch.zeros(1, 1, 32, 80), 0.5, sample=False, wrap_x=wrap)
    assert tuple(cc.shape) == (2, 5, 16, 40) and torch.equal(cc[:, 1:], z0)
    assert list(vae.encoder._plans) == [(4, F * TILE, F * TILE)]


def test_distance_to_the_global_decode_is_logged(params):
    """Not bounded: GroupNorm statistics are per tile by design.  docs/PARITY.md records the figure."""
    vae = _vae().enable_tiling(tile=TILE, overlap=OVERLAP)
    z = _latent()
    m = check("tiled_vae_decode_vs_global_decode", vae.decode(z), OV.decode(params, z.cpu(), _dd()))
    assert m["finite"]


# ------------------------------------------------------------------------------------------------ the pipeline
def _model():
    model, cfg, _ = V.tiny_eps_model(scale_factor=0.18215)
    model.first_stage_model = _vae()
    return model, cfg["context_dim"]


def _cond(ctx_dim, B=2):
    rng = np.random.RandomState(41)
    return (torch.tensor(rng.randn(B, V.T, ctx_dim).astype(np.float32)),
            torch.tensor(np.repeat(rng.randn(1, V.T, ctx_dim).astype(np.float32), B, 0)))


def test_pipeline_vae_tiling(plain):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model, ctx = _model()
    pipe = DiffusionPipeline(model, "ddim", device=DEV)
    c, uc = _cond(ctx)
    kw = dict(c=c, uc=uc, steps=2, scale=3.0, seeds=[101, 5], H=128, W=320)       # latents 16 x 40, images 32 x 80 (factor 2)
    wp, wpw = pipe.windowed(window=128), pipe.windowed(window=128, wrap_x=True, seam_pad=64)
    before = wp(decode=True, **kw)
    before_w = wpw(decode=True, **kw)
    assert pipe.enable_vae_tiling(tile=TILE, overlap=OVERLAP) is pipe
    vae = model.first_stage_model
    assert wp.model.first_stage_model is vae and wpw.model.first_stage_model is vae and vae.tiling["max_tile_batch"] == 8
    inv = 1. / model.scale_factor
    # clamped canvas
    z = wp(**kw)
    assert tuple(z.shape) == (2, 4, 16, 40)
    img = wp(decode=True, **kw)
    assert tuple(img.shape) == (2, 3, 32, 80)
    assert torch.equal(img.cpu(), _decode_ref(plain, inv * z, 8, False, "unit"))
    assert not torch.equal(img, before)
    # wrapped canvas: the VAE takes the wrapped grid, nothing is padded
    zw = wpw(**kw)
    imgw = wpw(decode=True, **kw)
    assert tuple(imgw.shape) == (2, 3, 32, 80)
    assert torch.equal(imgw, vae.decode_unit(inv * zw, wrap_x=True))
    assert torch.equal(imgw.cpu(), _decode_ref(plain, inv * zw, 8, True, "unit"))
    assert not torch.equal(imgw, vae.decode_unit(inv * zw)) and not torch.equal(imgw, before_w)
    assert list(vae.decoder._plans)[-1] == (8, TILE, TILE)
    # img2img starts from the tiled encode_noised
    rng = np.random.RandomState(51)
    x = torch.tensor(np.clip(rng.randn(2, 3, 32, 80) * 0.5, -1, 1).astype(np.float32))
    noise, post = (torch.tensor(rng.randn(2, 4, 16, 40).astype(np.float32), device=DEV) for _ in range(2))
    ikw = dict(strength=0.5, c=c, uc=uc, steps=4, scale=3.0, noise=noise)
    got = wp.img2img(init_image=x, post_noise=post, **ikw)
    z0, _ = vae.encode_noised(x.to(DEV), model.scale_factor, 1.0, 0.0, noise, post_noise=post)
    assert torch.equal(got, wp.img2img(init_latent=z0, **ikw))
    z0_plain, _ = plain.encode_noised(x.to(DEV), model.scale_factor, 1.0, 0.0, noise, post_noise=post)
    assert not torch.equal(z0, z0_plain)
    assert list(vae.encoder._plans) == [(8, F * TILE, F * TILE)]
    # off again: what a pipeline that never enabled it gives
    assert pipe.disable_vae_tiling() is pipe and vae.tiling is None
    assert torch.equal(wp(decode=True, **kw), before) and torch.equal(wpw(decode=True, **kw), before_w)
    fresh_model, _ = _model()
    fresh = DiffusionPipeline(fresh_model, "ddim", device=DEV)
    assert torch.equal(fresh.windowed(window=128)(decode=True, **kw), before)
    assert torch.equal(fresh.windowed(window=128, wrap_x=True, seam_pad=64)(decode=True, **kw), before_w)
    assert torch.equal(fresh.windowed(window=128).img2img(init_image=x, post_noise=post, **ikw),
                       wp.img2img(init_image=x, post_noise=post, **ikw))


def test_enable_vae_tiling_needs_a_vae():
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model, _, _ = V.tiny_eps_model()
    with pytest.raises(MdxError, match="enable_vae_tiling"):
        DiffusionPipeline(model, "ddim", device=DEV).enable_vae_tiling()
