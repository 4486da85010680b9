#!/usr/bin/env python3
"""Canonical text of what every model's load_state_dict packs, built on the host (device="cpu", seeded numpy parameters): run it
on two commits and diff the output to show that a change to the loading code left every packed byte as it was.

Per case:
    shape <name> <shape>                     parameter_shapes(), in order
    w <name> <dtype> <shape> <sha256>        one line per entry of model.w, in insertion order
    emb_off / emb_total                      the time-embedding column table of the UNets
    lora_base / lora_site / lora_merge       with enable_lora: the fp32 merge sources, where each target lives in w, and the
                                             arguments of every merge launch (ops.lora_merge is recorded, not run)

    python tools/weights_fingerprint.py [--only SUBSTR] > fingerprint.txt
"""
import argparse
import contextlib
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minddiffusion_amd import ops  # noqa: E402

UNET320 = dict(image_size=32, in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[1], num_res_blocks=1,
               channel_mult=[1, 2], num_head_channels=64, use_spatial_transformer=True, use_linear_in_transformer=True,
               transformer_depth=1, context_dim=1024, legacy=False)


def sha(t):
    if t is None:
        return "-"
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def tensor_line(name, t):
    return f"{name} {str(t.dtype).replace('torch.', '')} {tuple(t.shape)} {sha(t)}"


@contextlib.contextmanager
def settings(env=None, options=None):
    """Environment variables and ops options for the duration of one load."""
    env, options = env or {}, options or {}
    keep_env = {k: os.environ.get(k) for k in env}
    keep_opt = {k: ops.get_option(k) for k in options}
    os.environ.update(env)
    for k, v in options.items():
        ops.set_option(k, v)
    try:
        yield
    finally:
        for k, v in keep_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        for k, v in keep_opt.items():
            ops.set_option(k, v)


class Case:
    """One model, the parameters it is loaded from and how.  `shapes` = the ordered names the class owns; `weights` = the
    (label, w dict) pairs the load leaves behind."""

    def __init__(self, model, params, shapes=None, load=None, weights=None, env=None, options=None):
        self.name, self.model, self.params = "", model, params
        self.shapes = model.parameter_shapes() if shapes is None else shapes
        self._load = load or (lambda m, p, **kw: m.load_state_dict(p, **kw))
        self._weights = weights or (lambda m: [("", m.w)])
        self.env, self.options = env, options

    def load(self, params=None, **kw):
        """Load (the case's parameters unless others are given); returns the recorded LoRA merge launches."""
        merges = []

        def record(base, dst, layout, A=None, B=None, scale=1.0, **site):
            merges.append(f"lora_merge base={sha(base)} A={sha(A)} B={sha(B)} scale={scale!r}")
        keep, ops.lora_merge = ops.lora_merge, record
        try:
            with settings(self.env, self.options):
                self._load(self.model, self.params if params is None else params, **kw)
        finally:
            ops.lora_merge = keep
        return merges

    def weights(self):
        return self._weights(self.model)


def _numpy_params(shapes, seed=0):
    from minddiffusion_amd.weights import synthetic_unet_params_numpy
    return synthetic_unet_params_numpy(shapes, seed)


def _unet(cfg, as_torch=False, adapter=False, **kw):
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    net = UNetModel(device="cpu", **cfg)
    params = _numpy_params(net.parameter_shapes())
    if adapter:
        from _lora_util import make_adapter
        params.update(make_adapter(net.lora_parameter_shapes(), 3))
    if as_torch:
        params = {k: torch.from_numpy(v) for k, v in params.items()}
    return Case(net, params, **kw)


def _glide(upsampler, subpixel):
    from test_host_cpu import TINY_GLIDE
    from oracle import glide as OG
    from minddiffusion_amd.glide.diffusion_creator import create_model, create_upsample_model
    otiny = dict(OG.BASE_OPTIONS, image_size=16, model_channels=64, num_res_blocks=1, channel_mult=(1, 2),
                 attention_resolutions=(1, 2), text_ctx=16, xf_width=64, xf_layers=2, xf_heads=1, n_vocab=100)
    options = {"unet_subpixel_upsample": subpixel}
    if not upsampler:
        return Case(create_model(device="cpu", **TINY_GLIDE), OG.init_params(otiny, seed=0), options=options)
    up = create_upsample_model(device="cpu", low_size=8, **dict(TINY_GLIDE, image_size=32, channel_mult=(1, 1, 2)))
    return Case(up, OG.init_params(dict(otiny, in_channels=6, image_size=32, channel_mult=(1, 1, 2)), seed=1), options=options)


def _vae(what, **ddconfig):
    """AutoencoderKL, or one half loaded the way AutoencoderKL loads it from a dict whose keys carry a prefix."""
    from oracle import vae as OV
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
    from minddiffusion_amd.ldm.modules.diffusionmodules.model import Decoder, Encoder
    dd = dict(TINY_VAE_DDCONFIG, **ddconfig)
    vp = OV.init_params(dd, seed=len(ddconfig))
    if what == "vae":
        return Case(AutoencoderKL(ddconfig=dd, embed_dim=4, device="cpu"), vp,
                    weights=lambda m: [("decoder ", m.decoder.w), ("encoder ", m.encoder.w)])
    if what == "bare decoder":
        return Case(Decoder(device="cpu", **dd), {k[len("decoder."):]: v for k, v in vp.items() if k.startswith("decoder.")})
    pre = "first_stage_model."
    half, arg, conv = (Decoder, "post_quant", "post_quant_conv") if what == "decoder" else (Encoder, "quant", "quant_conv")
    net = half(device="cpu", **dd)
    return Case(net, {pre + k: v for k, v in vp.items()}, shapes=net.parameter_shapes(pre + what + "."),
                load=lambda m, p, **kw: m.load_state_dict(p, prefix=pre + what + ".",
                                                          **{arg: (p[pre + conv + ".weight"], p[pre + conv + ".bias"])}, **kw))


def _text(frozen):
    from oracle import text_encoder as OT
    from minddiffusion_amd.ldm.modules.encoders.modules import FrozenCLIPEmbedder_ZH
    from minddiffusion_amd.ldm.modules.encoders.text_encoder import TextEncoder
    tcfg = dict(OT.SD2_TEXT, vocab_size=100, width=128, layers=3, heads=2)
    tp = OT.init_params(tcfg, seed=1)
    if frozen:
        emb = FrozenCLIPEmbedder_ZH(max_length=tcfg["context_length"], device="cpu", vocab_size=100, width=128, layers=3, heads=2)
        return Case(emb, tp, weights=lambda m: [("", m.transformer.w)])
    enc = TextEncoder(context_length=tcfg["context_length"], vocab_size=100, output_dim=128, width=128, layers=3, heads=2,
                      device="cpu")
    return Case(enc, {k[len("transformer."):]: v for k, v in tp.items()})


def _srgan(factor, prelu, dtype):
    from test_srgan_cpu import synthetic_params
    from minddiffusion_amd.glide.model.srgan import Generator
    p = synthetic_params(factor, seed=factor, prelu=prelu)
    if dtype == np.float64:     # values that float32 cannot hold, so that both roundings of the load are exercised
        rng = np.random.RandomState(17)
        p = {k: v.astype(np.float64) * (1.0 + 1e-9 * rng.standard_normal(v.shape)) for k, v in p.items()}
    gen = Generator(factor, device="cpu")
    return Case(gen, p, shapes=gen.parameter_shapes(prelu))


def case_table():
    """name -> function that builds the Case (models and parameters are built only when asked for)."""
    from test_host_cpu import UNET_VARIANTS
    from minddiffusion_amd.configs import TINY_UNET
    t = {"unet320": lambda: _unet(UNET320),
         "unet320 MDX_UNET_LN_FOLD=0": lambda: _unet(UNET320, env={"MDX_UNET_LN_FOLD": "0"}),
         "unet320 MDX_UNET_QKV_MERGE=0": lambda: _unet(UNET320, env={"MDX_UNET_QKV_MERGE": "0"}),
         "unet320 subpixel off": lambda: _unet(UNET320, options={"unet_subpixel_upsample": 0}),
         "unet320 lora": lambda: _unet(dict(UNET320, enable_lora=True)),
         "unet320 lora + adapter": lambda: _unet(dict(UNET320, enable_lora=True), adapter=True),
         "tiny_unet": lambda: _unet(TINY_UNET),
         "tiny_unet torch tensors": lambda: _unet(TINY_UNET, as_torch=True),
         "tiny_unet lora + adapter": lambda: _unet(dict(TINY_UNET, enable_lora=True), adapter=True),
         # inner = 96: no LayerNorm fold, the [q | k] + v fallback
         "unet96 inner % 64 != 0": lambda: _unet(dict(TINY_UNET, model_channels=96, num_head_channels=32))}
    for name in sorted(UNET_VARIANTS):
        t[f"tiny_unet variant {name}"] = lambda name=name: _unet(dict(TINY_UNET, **UNET_VARIANTS[name]))
    for sub in (1, 0):
        tag = "" if sub else " subpixel off"
        t["tiny_glide base" + tag] = lambda sub=sub: _glide(False, sub)
        t["tiny_glide upsampler" + tag] = lambda sub=sub: _glide(True, sub)
    t["tiny_vae"] = lambda: _vae("vae")
    t["tiny_vae attn"] = lambda: _vae("vae", attn_resolutions=[16])
    t["tiny_vae decoder post_quant prefix"] = lambda: _vae("decoder")
    t["tiny_vae encoder quant prefix"] = lambda: _vae("encoder")
    t["tiny_vae decoder no post_quant"] = lambda: _vae("bare decoder")
    t["tiny_text_encoder"] = lambda: _text(False)
    t["frozen_embedder"] = lambda: _text(True)
    for factor, prelu, dtype in ((2, "a", np.float32), (4, "w", np.float32), (2, "w", np.float64), (4, "a", np.float64)):
        t[f"srgan x{factor} .{prelu} {np.dtype(dtype).name}"] = lambda a=(factor, prelu, dtype): _srgan(*a)
    return t


def build_case(name, table=None):
    case = (table or case_table())[name]()
    case.name = name
    return case


def _site_line(name, site, w):
    """One entry of UNetModel._lora_sites: tensors print as the w entry whose storage they view, plus the offset."""
    where = {t.untyped_storage().data_ptr(): k for k, t in w.items()}
    parts = []
    for k, v in site.items():
        if isinstance(v, torch.Tensor):
            v = f"{where.get(v.untyped_storage().data_ptr(), '?')}+{v.storage_offset()}"
        parts.append(f"{k}={v}")
    return f"lora_site {name}: " + " ".join(parts)


def fingerprint(case):
    out = [f"==== {case.name}"]
    out += [f"shape {k} {tuple(v)}" for k, v in case.shapes.items()]
    merges = case.load()
    m = case.model
    for label, w in case.weights():
        out += [tensor_line(f"w {label}{k}", t) for k, t in w.items()]
    if hasattr(m, "_emb_off"):
        out.append("emb_off " + " ".join(f"{k}={v}" for k, v in m._emb_off.items()))
        out.append(f"emb_total {m._emb_total}")
    if getattr(m, "enable_lora", False):
        out += [tensor_line(f"lora_base {k}", t) for k, t in m._lora_base.items()]
        for name, sites in m._lora_sites.items():
            out += [_site_line(name, s, m.w) for s in sites]
        out += merges
        if m._lora:
            out += [f"lora {k} A={sha(a)} B={sha(b)}" for k, (a, b) in m._lora.items()]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default="", help="only the cases whose name contains this")
    args = ap.parse_args()
    table = case_table()
    for name in table:
        if args.only in name:
            print("\n".join(fingerprint(build_case(name, table))))


if __name__ == "__main__":
    main()
