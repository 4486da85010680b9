"""Shared helpers of the inpainting tests (test_inpaint_cpu.py / test_inpaint_gpu.py).

numpy / float64 restatements of what the four kernels of csrc/inpaint.hip compute -- the integer nearest rule, make_batch_sd of
wukong-huahua/inpaint.py:39-63, alpha = max(m, G * m), the composite -- the tiny hybrid model the pipeline tests run, and the oracle
side of the end-to-end comparison, which needs nothing changed under oracle/.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import dpm_solver as OD
from oracle import ldm as O
from oracle import vae as OV

SCALE_FACTOR = 0.18215
UNET_SEED, VAE_SEED = 6, 8          # the seeds tests/test_unet_gpu.py and tests/test_img2img_gpu.py use for these two networks


# ------------------------------------------------------------------------------------------------ restatements
def binarise(mask):
    """inpaint.py:51-52: >= 0.5 is the hole."""
    return (np.asarray(mask, np.float32) >= np.float32(0.5)).astype(np.float32)


def nearest_index(n_out, n_in):
    """Source index of every output index: (i * n_in) // n_out, in integers (ResizeNearestNeighbor, align_corners=False)."""
    return (np.arange(n_out, dtype=np.int64) * n_in) // n_out


def resize_nearest(m, h, w):
    """[.., H, W] -> [.., h, w] by the integer rule."""
    return m[..., nearest_index(h, m.shape[-2])[:, None], nearest_index(w, m.shape[-1])[None, :]]


def make_batch_sd(image, mask, num_samples):
    """inpaint.py:39-63 on arrays: image [1, 3, H, W] in [-1, 1], mask [1, 1, H, W] in [0, 1] -> the repeated image, binarised
    mask and masked image."""
    m = binarise(mask)
    masked = image * (m < 0.5)
    rep = lambda a: np.repeat(a, num_samples, axis=0)
    return {"image": rep(image), "mask": rep(m), "masked_image": rep(masked.astype(np.float32))}


def feather_ref(mask, weights):
    """float64 alpha = max(m, G * m): replicate pad, rows then columns, with the given (fp32) taps."""
    m = torch.tensor(binarise(mask), dtype=torch.float64)
    wts = torch.tensor(np.asarray(weights), dtype=torch.float64)
    r = (wts.numel() - 1) // 2
    g = F.conv2d(F.pad(m, (r, r, r, r), mode="replicate"), wts.reshape(1, 1, 1, -1))
    g = F.conv2d(g, wts.reshape(1, 1, -1, 1))
    return torch.maximum(m, g).numpy()


def composite_ref(decoded, image, alpha):
    """float64 clamp((alpha d + (1 - alpha) img + 1) / 2, 0, 1); alpha None: 1."""
    d = np.asarray(decoded, np.float64)
    if alpha is not None:
        a = np.asarray(alpha, np.float64)
        d = a * d + (1.0 - a) * np.asarray(image, np.float64)
    return np.clip((d + 1.0) / 2.0, 0.0, 1.0)


# ------------------------------------------------------------------------------------------------ the tiny hybrid model
B, S, SCALE = 2, 5, 7.5
IMG, LAT, T = 16, 8, 6              # 16 x 16 images, the tiny VAE halves them


def tiny_cfg(in_channels=9):
    from minddiffusion_amd.configs import TINY_UNET
    return dict(TINY_UNET, in_channels=in_channels)


def tiny_params(in_channels=9):
    return O.init_params(dict(tiny_cfg(in_channels), num_heads=-1), seed=UNET_SEED)


def vae_params():
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    return OV.init_params(dict(TINY_VAE_DDCONFIG), seed=VAE_SEED)


def tiny_model(dev, in_channels=9):
    """LatentInpaintDiffusion (9 channels) or LatentDiffusion (4) around the seeded tiny UNet, the tiny VAE attached."""
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion, LatentInpaintDiffusion
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    net = UNetModel(**tiny_cfg(in_channels))
    net.load_state_dict(tiny_params(in_channels))
    kw = dict(linear_start=0.00085, linear_end=0.0120, timesteps=1000, scale_factor=SCALE_FACTOR)
    model = LatentInpaintDiffusion(unet_config=net, **kw) if in_channels == 9 else LatentDiffusion(net, **kw)
    vae = AutoencoderKL(ddconfig=dict(TINY_VAE_DDCONFIG), embed_dim=4, device=dev)
    vae.load_state_dict(vae_params())
    model.first_stage_model = vae
    return model


def pipe_inputs(seed=41):
    """Two different images, a soft-valued mask per sample (values on both sides of 0.5: the binarisation matters), the posterior
    and forward draws, the two contexts (the unconditional one a repeated row)."""
    rng = np.random.RandomState(seed)
    image = np.clip(0.5 * rng.randn(B, 3, IMG, IMG), -1, 1).astype(np.float32)
    mask = np.zeros((B, 1, IMG, IMG), np.float32)
    mask[0, 0, 4:12, 2:9] = 0.9
    mask[0, 0, 0:3, 12:16] = 0.4          # below the threshold: not a hole
    mask[1, 0, 6:16, 5:14] = 0.5          # the threshold itself is a hole
    post, noise = (rng.randn(B, 4, LAT, LAT).astype(np.float32) for _ in range(2))
    ctx = tiny_cfg()["context_dim"]
    c = rng.randn(B, T, ctx).astype(np.float32)
    uc = np.repeat(rng.randn(1, T, ctx).astype(np.float32), B, 0)
    return {k: torch.tensor(v) for k, v in dict(image=image, mask=mask, post=post, noise=noise, c=c, uc=uc).items()}


# ------------------------------------------------------------------------------------------------ the oracle side
def oracle_model(in_channels=9):
    return O.ModelOracle(O.UNetOracle(dict(tiny_cfg(in_channels), num_heads=-1), tiny_params(in_channels)))


def oracle_c_concat(image, mask, post):
    """inpaint.py:76-85 on the oracle's VAE: cat(nearest-resized binarised mask, scale_factor * encode(masked image))."""
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    m = binarise(mask)
    masked = (np.asarray(image, np.float32) * (m < 0.5)).astype(np.float32)
    z = SCALE_FACTOR * OV.encode(vae_params(), masked, post, dict(TINY_VAE_DDCONFIG)).numpy()
    m_lat = np.broadcast_to(resize_nearest(m, z.shape[2], z.shape[3]), (z.shape[0], 1) + z.shape[2:])
    return np.concatenate([m_lat, z], 1).astype(np.float32)


def oracle_decode(z):
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    return OV.decode(vae_params(), torch.as_tensor(z, dtype=torch.float32) / SCALE_FACTOR, dict(TINY_VAE_DDCONFIG)).numpy()


def oracle_dpm_hybrid(omodel, steps, c_cat, c, uc, x_T, scale, uc_cat=None):
    """The oracle's DPM-Solver++ on hybrid conditioning: model_wrapper concatenates [uncond; cond] for the text context, the lambda
    does the same for c_concat (WK plms.py:191-201: every key)."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
    cat2 = torch.cat([t(c_cat if uc_cat is None else uc_cat), t(c_cat)])
    ns = OD.NoiseScheduleVP("discrete", alphas_cumprod=omodel.alphas_cumprod)
    fn = OD.model_wrapper(lambda x, tt, cc: omodel.apply_model(x, tt, {"c_concat": cat2, "c_crossattn": cc}), ns, t(c), t(uc),
                          float(scale))
    return OD.DPM_Solver(fn, ns, predict_x0=True).sample(t(x_T), steps=steps, order=2, lower_order_final=True)
