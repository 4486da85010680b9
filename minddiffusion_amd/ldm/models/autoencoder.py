"""AutoencoderKL -- mirror of the reference's ldm/models/autoencoder.py (:22-78): ``decode(z)`` =
``decoder(post_quant_conv(z))`` and ``encode(x)`` = a sample of the diagonal Gaussian given by
``quant_conv(encoder(x))`` (the inpainting / img2img pre-processing, wukong-huahua/inpaint.py:79-81).

Attach to ``LatentDiffusion.first_stage_model`` and ``decode_first_stage`` / ``DiffusionPipeline`` produce images:

    vae = AutoencoderKL(ddconfig=SD_VAE_DDCONFIG, embed_dim=4)
    vae.load_state_dict(params)            # reference names: post_quant_conv.*, decoder.*
    model.first_stage_model = vae
"""
import numpy as np
import torch

from ... import ops
from ..modules.diffusionmodules.model import Decoder, Encoder


def _int_pair(v, what):
    """An int or an (h, w) pair of ints (no bools, no floats) as (h, w)."""
    from ..._lib import MdxError
    pair = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if len(pair) != 2 or any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) for a in pair):
        raise MdxError(f"AutoencoderKL.enable_tiling: {what} must be an int or an (h, w) pair of ints, got {v!r}")
    return int(pair[0]), int(pair[1])


class AutoencoderKL:
    def __init__(self, ddconfig, embed_dim, ckpt_path=None, ignore_keys=(), image_key="image", colorize_nlabels=None,
                 monitor=None, use_fp16=False, device=None, use_graph=True):
        assert ddconfig["double_z"]
        self.embed_dim = embed_dim
        self.ddconfig = dict(ddconfig)
        self.decoder = Decoder(device=device, use_graph=use_graph, **ddconfig)
        self.encoder = Encoder(device=device, use_graph=use_graph, **ddconfig)
        self.generator = None          # torch.Generator for encode()'s noise (None: the default generator)
        self.tiling = None             # enable_tiling(): {"tile", "overlap", "max_tile_batch"}; None: every canvas is one image
        self._tile_grids = {}
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    def init_from_ckpt(self, path, ignore_keys=()):
        """autoencoder.py:44-54: read a MindSpore .ckpt (minddiffusion_amd/ms_checkpoint.py), drop keys that start with
        one of `ignore_keys`, load.  Accepts a bare VAE checkpoint or a whole LatentDiffusion one (first_stage_model.*)."""
        from ...ms_checkpoint import VAE_PREFIX, load_checkpoint
        sd = load_checkpoint(path)
        if any(k.startswith(VAE_PREFIX) for k in sd):
            sd = {k[len(VAE_PREFIX):]: v for k, v in sd.items() if k.startswith(VAE_PREFIX)}
        sd = {k: v for k, v in sd.items() if not any(k.startswith(ik) for ik in ignore_keys)}
        # Keys this model does not own (loss.*, discriminator.* of a training checkpoint ...) are reported, not fatal -- the
        # reference's load_param_into_net ignores them and the CLI prints the list (autoencoder.py:44-54); MISSING keys of a
        # checkpoint that carries an encoder still raise.
        own = self.parameter_shapes()
        self.unexpected_keys = sorted(k for k in sd if k not in own)
        if self.unexpected_keys:
            import warnings
            warnings.warn(f"AutoencoderKL.init_from_ckpt: {len(self.unexpected_keys)} checkpoint keys are not parameters of this "
                          f"model and were ignored: {self.unexpected_keys[:8]}{' ...' if len(self.unexpected_keys) > 8 else ''}")
        sd = {k: v for k, v in sd.items() if k in own}
        self.load_state_dict(sd, strict="encoder.conv_in.weight" in sd)
        return self

    def parameter_shapes(self):
        zc = self.ddconfig["z_channels"]
        s = {"post_quant_conv.weight": (zc, self.embed_dim, 1, 1), "post_quant_conv.bias": (zc,)}
        s.update(self.decoder.parameter_shapes("decoder."))
        s["quant_conv.weight"] = (2 * self.embed_dim, 2 * zc, 1, 1)
        s["quant_conv.bias"] = (2 * self.embed_dim,)
        s.update(self.encoder.parameter_shapes("encoder."))
        return s

    def load_state_dict(self, params, strict=True):
        """Reference names: post_quant_conv.*, decoder.*, quant_conv.*, encoder.*.  A decode-only checkpoint (no encoder.*)
        loads with strict=False; encode() then raises.  strict also rejects keys this model does not own."""
        from ...weights import check_state_dict
        if strict:
            check_state_dict(self.parameter_shapes(), params, True, "AutoencoderKL.load_state_dict")
        self.decoder.load_state_dict(params, prefix="decoder.",
                                     post_quant=(params["post_quant_conv.weight"], params["post_quant_conv.bias"]),
                                     strict=strict)
        if "encoder.conv_in.weight" in params:
            self.encoder.load_state_dict(params, prefix="encoder.",
                                         quant=(params["quant_conv.weight"], params["quant_conv.bias"]), strict=strict)
        elif strict:
            from ..._lib import MdxError
            raise MdxError("AutoencoderKL.load_state_dict: encoder.* parameters missing (pass strict=False for decode only)")

    # ------------------------------------------------------------------ tiling
    @property
    def factor(self):
        """Image pixels per latent pixel and axis: 2^(levels - 1), 8 for the SD VAE, 2 for the tiny test VAE."""
        return 1 << (len(self.ddconfig["ch_mult"]) - 1)

    def enable_tiling(self, tile=64, overlap=16, max_tile_batch=8):
        """Decode and encode canvases larger than one tile as overlapping tiles, blended with min-ramp weights over the
        overlap.  tile / overlap: latent pixels, ints or (h, w) pairs, 0 <= overlap < tile; the stride is tile - overlap.
        max_tile_batch: the batch every decoder / encoder call of a tiled canvas has (the last chunk repeats its last tile), so
        one plan per tile shape serves every canvas size and batch.  A canvas that fits one tile on both axes takes the plain
        path.  GroupNorm and the mid attention see one tile: the result is close to the global one, not equal to it."""
        from ..._lib import MdxError
        th, tw = _int_pair(tile, "tile")
        oh, ow = _int_pair(overlap, "overlap")
        if th < 1 or tw < 1 or not (0 <= oh < th and 0 <= ow < tw):
            raise MdxError(f"AutoencoderKL.enable_tiling: need 0 <= overlap < tile per axis, got tile {(th, tw)}, overlap "
                           f"{(oh, ow)}")
        if isinstance(max_tile_batch, bool) or not isinstance(max_tile_batch, (int, np.integer)) or max_tile_batch < 1:
            raise MdxError(f"AutoencoderKL.enable_tiling: max_tile_batch must be an int >= 1, got {max_tile_batch!r}")
        if max(oh, ow, 1) * self.factor > 4096:
            raise MdxError(f"AutoencoderKL.enable_tiling: overlap {(oh, ow)} x factor {self.factor} exceeds the blend's ramp "
                           f"limit of 4096 image pixels")
        self.tiling = {"tile": (th, tw), "overlap": (oh, ow), "max_tile_batch": int(max_tile_batch)}
        self._tile_grids = {}
        return self

    def disable_tiling(self):
        self.tiling = None
        self._tile_grids = {}
        return self

    def _tiles_for(self, h, w, wrap_x):
        """None when tiling is off or the latent canvas h x w fits one tile on both axes; else the cached grids of the canvas:
        lat / img (ops.WindowGrid on the latent and on the image canvas: the same grid times `factor`), rows (all N tiles),
        ramp_lat / ramp_img (ry, rx).  A tile larger than the canvas on an axis becomes the canvas extent."""
        if self.tiling is None:
            return None
        (th, tw), (oh, ow) = self.tiling["tile"], self.tiling["overlap"]
        if h <= th and w <= tw:
            return None
        key = (int(h), int(w), bool(wrap_x))
        if key not in self._tile_grids:
            f = self.factor
            sh, sw = min(th - oh, h), min(tw - ow, w)
            th, tw = min(th, h), min(tw, w)
            wrap = bool(wrap_x) and w > tw
            lat = ops.WindowGrid((h, w), (th, tw), (sh, sw), wrap_x=wrap)
            img = ops.WindowGrid((f * h, f * w), (f * th, f * tw), (f * sh, f * sw), wrap_x=wrap)
            assert img.host.tolist() == [f * o for o in lat.host.tolist()]
            self._tile_grids[key] = {"lat": lat, "img": img, "rows": ops.WindowRows(list(range(lat.N))),
                                     "ramp_lat": (max(1, oh), max(1, ow)), "ramp_img": (max(1, f * oh), max(1, f * ow)),
                                     "weights": {}}
        return self._tile_grids[key]

    def _run_tiles(self, net, tiles, stage_shape, dtype):
        """`net` on tiles [T, ...] in chunks of exactly max_tile_batch rows -- chunk c holds rows c m .. min((c + 1) m, T) - 1
        and the last chunk repeats its last row up to m -- its outputs (the plan's own buffer, overwritten by the next chunk)
        staged into one [T, *stage_shape] tensor."""
        m, T = self.tiling["max_tile_batch"], int(tiles.shape[0])
        staged = torch.empty((T,) + tuple(stage_shape), dtype=dtype, device=tiles.device)
        for c0 in range(0, T, m):
            chunk = tiles[c0:c0 + m]
            n = int(chunk.shape[0])
            if n < m:
                chunk = torch.cat([chunk, chunk[-1:].expand(m - n, *chunk.shape[1:])])
            staged[c0:c0 + n].copy_(net(chunk)[:n])
        return staged

    def _decode_tiled(self, z, wrap_x, mode):
        z = z.to(torch.float32).contiguous()
        t = self._tiles_for(int(z.shape[2]), int(z.shape[3]), wrap_x)
        if t is None:
            return None
        lat, img = t["lat"], t["img"]
        tiles = ops.window_gather_rows(z, lat, t["rows"])
        staged = self._run_tiles(self.decoder, tiles, (self.decoder.out_ch, img.h, img.w), torch.float32)
        return ops.tile_blend(staged, img, t["ramp_img"], mode=mode)

    def decode(self, z, wrap_x=False):
        """autoencoder.py:65-68.  Returns a fresh tensor (the decoder's own output buffer is reused by the next call).  With
        tiling on and a canvas larger than one tile: the tiles gathered, decoded in chunks and blended by ONE
        mdx_tile_blend_f32 launch; wrap_x: the tiles wrap around the canvas' right edge (a 360-degree panorama)."""
        if self.tiling is not None:
            out = self._decode_tiled(z, wrap_x, "raw")
            if out is not None:
                return out
        return self.decoder(z).clone()

    def decode_unit(self, z, wrap_x=False):
        """clamp((decode(z) + 1) / 2, 0, 1): the image in [0, 1]; tiled, the conversion is part of the blend launch."""
        if self.tiling is not None:
            out = self._decode_tiled(z, wrap_x, "unit")
            if out is not None:
                return out
        return torch.clamp((self.decoder(z) + 1.0) / 2.0, 0.0, 1.0)

    def _latent_hw(self, B, H, W):
        """(h, w) of the latent of images [B, 3, H, W], without building a whole-canvas plan for a tiled canvas."""
        f = self.factor
        if self.tiling is not None and H % f == 0 and W % f == 0:
            th, tw = self.tiling["tile"]
            if H // f > th or W // f > tw:
                return H // f, W // f
        return self.encoder._plan(B, H, W).out_hw

    def _moments(self, x, wrap_x=False):
        """(moments NHWC fp16 [B, h * w, mom_pad] = [mean | logvar | pad], (h, w)): the encoder on x, or -- with tiling on and a
        canvas larger than one tile -- on its image tiles in chunks, the tiles' moments averaged onto the latent canvas with
        the min-ramp weights at latent resolution (mdx_window_average_f16 / mdx_window_average_regions_f16 on a wrapped grid)."""
        B, _, H, W = x.shape
        f = self.factor
        t = None
        if self.tiling is not None:
            if H % f or W % f:
                from ..._lib import MdxError
                raise MdxError(f"AutoencoderKL: image {H}x{W} is not divisible by {f}")
            t = self._tiles_for(H // f, W // f, wrap_x)
        if t is None:
            mom = self.encoder(x)
            return mom, self.encoder._plans[(B, H, W)].out_hw
        lat, img = t["lat"], t["img"]
        x = x.to(torch.float32).contiguous()
        tiles = ops.window_gather_rows(x, img, t["rows"])
        staged = self._run_tiles(self.encoder, tiles, (lat.h * lat.w, self.encoder.mom_pad), torch.float16)
        if x.device not in t["weights"]:
            t["weights"][x.device] = ops.ramp_weights((lat.h, lat.w), t["ramp_lat"]).to(x.device)
        wts = t["weights"][x.device]
        C = 2 * self.embed_dim
        if lat.wrap_x:
            mom = ops.window_average_regions(staged, lat, C, plan=None, weights=wts)
        else:
            mom = ops.window_average(staged, lat, C, weights=wts)
        return mom, (lat.Hc, lat.Wc)

    def encode(self, x, noise=None, sample=True, wrap_x=False):
        """autoencoder.py:70-78: mean, logvar = split(quant_conv(encoder(x))); logvar clipped to [-30, 20];
        returns mean + exp(0.5 logvar) * N(0, 1)  ([B, embed_dim, H/8, W/8] fp32).  `noise` injects the draw (tests);
        sample=False returns the mode.  wrap_x: with tiling on, the tiles wrap around the x axis."""
        mom, (h, w) = self._moments(x, wrap_x)
        B = x.shape[0]
        zc = self.embed_dim
        out = torch.empty((B, zc, h, w), dtype=torch.float32, device=mom.device)
        if sample and noise is None:
            noise = torch.randn(out.shape, device=mom.device, dtype=torch.float32, generator=self.generator)
        if noise is not None:
            noise = noise.to(device=mom.device, dtype=torch.float32).contiguous()
        return ops.vae_gaussian_sample(mom, zc, noise if sample else None, out)

    def latent_shape(self, image_shape):
        """[B, embed_dim, h, w] of encode()'s result for images [B, 3, H, W]: the encoder plan's own output size (the
        downsampling factor is 2^(levels - 1): 8 for the SD VAE, 2 for the tiny test VAE)."""
        B, _, H, W = image_shape
        h, w = self._latent_hw(B, H, W)
        return (B, self.embed_dim, h, w)

    def encode_noised(self, x, scale_factor, a, b, noise, post_noise=None, sample=True, wrap_x=False):
        """img2img start: the encoder, then ONE launch (mdx_vae_encode_noised_f32) that draws the posterior sample as encode()
        does, scales it (z0 = scale_factor * z, LatentDiffusion.get_first_stage_encoding) and noises it
        (x_t = a * z0 + b * noise, the samplers' stochastic_encode).  noise: N(0, 1) of latent_shape(x.shape); post_noise /
        sample: encode()'s `noise` / `sample`.  Returns (z0, x_t), fresh tensors."""
        mom, hw = self._moments(x, wrap_x)
        shape = (int(x.shape[0]), self.embed_dim) + tuple(hw)
        z0 = torch.empty(shape, dtype=torch.float32, device=mom.device)
        x_t = torch.empty_like(z0)
        if sample and post_noise is None:
            post_noise = torch.randn(shape, device=mom.device, dtype=torch.float32, generator=self.generator)
        to_dev = lambda t: torch.as_tensor(t).to(device=mom.device, dtype=torch.float32).contiguous()
        return ops.vae_encode_noised(mom, self.embed_dim, to_dev(post_noise) if sample else None, scale_factor, a, b,
                                     to_dev(noise), z0, x_t)

    def encode_concat(self, masked_image, mask, scale_factor, post_noise=None, sample=True, wrap_x=False):
        """Inpainting conditioning (inpaint.py:76-85): the encoder on the masked image, then ONE launch (mdx_inpaint_concat_f32)
        that writes c_concat [B, 1 + embed_dim, h, w] = cat(mask at the latent grid, scale_factor * posterior sample).  mask
        [1 | B, 1, H, W], >= 0.5 = hole, resized by the integer nearest rule; post_noise / sample: encode()'s `noise` / `sample`.
        The latent channels are encode_noised's z0 bit for bit.  A fresh tensor."""
        mom, hw = self._moments(masked_image, wrap_x)
        shape = (int(masked_image.shape[0]), self.embed_dim) + tuple(hw)
        if sample and post_noise is None:
            post_noise = torch.randn(shape, device=mom.device, dtype=torch.float32, generator=self.generator)
        to_dev = lambda t: torch.as_tensor(t).to(device=mom.device, dtype=torch.float32).contiguous()
        return ops.inpaint_concat(mom, self.embed_dim, to_dev(post_noise) if sample else None, scale_factor, to_dev(mask),
                                  shape[2:])
