#!/usr/bin/env python3
"""Canonical text of what the planners emit, built on the host (device="cpu", nothing is launched): run it on two commits and
diff the output to show that a change to the planning code left every plan as it was.

Per plan, layer 1 (from the plan's own records):
    op   <i>: kind | flops | launches | info          one line per entry of P.meta
    desc <i>: every mdx_gemm_desc field in header order (also the context-plan descriptors: they are part of P.descs)
    tail / head <i>: the same for the fused SpatialTransformer descriptors
    marks: op index of the guidance-duplicate checkpoints (P.ck), temb_ops, n_text, n_emb
layer 2: P.main (then P.ctxops and the guidance-duplicate body) replayed against a recording stand-in for the library -- every C
call's name and arguments, which reaches what only lives in closures (attention strides, norm arguments, small ops).  Functions
that launch (the *_f16 / *_f32 entry points, which take a stream) are logged and return 0; host-only queries are forwarded.

Pointers print as the ordinal of their first appearance in the plan (0 stays 0): aliasing, buffer reuse and view offsets stay
visible, addresses do not.

    python tools/plan_fingerprint.py [--only SUBSTR] [--no-replay] > fingerprint.txt
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from minddiffusion_amd import _lib, ops  # noqa: E402

_PTR = ctypes.c_void_p
_DESC_TYPES = (_lib.GemmDesc, _lib.StTailDesc, _lib.StHeadDesc)


class Pointers:
    """address -> ordinal of first appearance."""

    def __init__(self):
        self.seen = {}

    def __call__(self, v):
        v = int(v or 0)
        if v == 0:
            return "0"
        return "p%d" % self.seen.setdefault(v, len(self.seen) + 1)


def _num(v):
    return repr(round(v, 9)) if isinstance(v, float) else str(v)


def desc_fields(d, ptr):
    """Every field of a ctypes descriptor in declaration (= header) order, pointers normalised by `ptr`."""
    out = []
    for name, ctype in d._fields_:
        v = getattr(d, name)
        out.append(f"{name}={ptr(v) if ctype is _PTR else _num(v)}")
    return " ".join(out)


def gemm_desc_sequence(descs, ptr=None):
    """The pointer-normalised field lines of a list of GEMM descriptors (one normaliser for the whole list)."""
    ptr = ptr or Pointers()
    return [desc_fields(d, ptr) for d in descs]


class Recorder:
    """Stands in for the loaded library while a plan is replayed on the host."""

    def __init__(self, real, ptr, log):
        self._real, self._ptr, self._log = real, ptr, log

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if not name.endswith(("_f16", "_f32")):
            return real
        argtypes = _lib.SIGNATURES[name][1]

        def call(*args):
            parts = []
            for a, ct in zip(args, argtypes):
                obj = getattr(a, "_obj", None)      # ctypes.byref(descriptor)
                if isinstance(obj, _DESC_TYPES):
                    parts.append("{" + desc_fields(obj, self._ptr) + "}")
                elif ct is _PTR:
                    parts.append(self._ptr(a.value if isinstance(a, _PTR) else a))
                else:
                    parts.append(_num(a))
            self._log.append(f"{name}({', '.join(parts)})")
            return 0
        return call


def replay(op_list, ptr):
    """Run the closures of an op list with the library replaced by a Recorder; returns the call log."""
    log = []
    keep = (_lib.load, ops._chk, ops._stream)
    rec = Recorder(_lib.load(), ptr, log)
    _lib.load, ops._chk, ops._stream = (lambda: rec), (lambda *a, **k: None), (lambda: None)
    try:
        for i, op in enumerate(op_list):
            n = len(log)
            try:
                op()
            except Exception as e:     # an op kind the host cannot replay: say so instead of hiding it
                log.append(f"UNREPLAYABLE {type(e).__name__}: {e}")
            if len(log) == n:
                log.append("(host op)")
            log[n:] = [f"{i}: {line}" for line in log[n:]]
    finally:
        _lib.load, ops._chk, ops._stream = keep
    return log


def fingerprint(name, P, do_replay=True, extra_lists=()):
    ptr = Pointers()
    out = [f"==== {name}"]
    meta = getattr(P, "meta", None) or []
    for i, m in enumerate(meta):
        out.append(f"op {i}: {m['kind']} | {m['flops']} | {m['launches']} | {m['info']}")
    for i, line in enumerate(gemm_desc_sequence(P.descs, ptr)):
        out.append(f"desc {i}: {line}")
    for kind in ("tails", "heads_fused"):
        for i, d in enumerate(getattr(P, kind, None) or []):
            out.append(f"{kind} {i}: {desc_fields(d, ptr)}")
    ck = getattr(P, "ck", None)
    if ck:
        out.append("ck: " + " ".join(f"{k}={P.main.index(ck[k])}" for k in ("conv_in", "op", "op2") if ck.get(k) is not None))
    out.append("marks: " + " ".join(f"{k}={getattr(P, k)}" for k in ("temb_ops", "n_text", "n_emb") if hasattr(P, k)))
    out.append(f"len(main)={len(P.main)} len(meta)={len(meta)} arena={P.arena.total}")
    if do_replay:
        for label, ops_list in (("main", P.main), ("ctxops", getattr(P, "ctxops", None))) + tuple(extra_lists):
            if ops_list:
                out.append(f"-- calls of {label}")
                out += replay(ops_list, ptr)
    return out


# ------------------------------------------------------------------ the fixed list of plans
def _unet(cfg):
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from minddiffusion_amd.weights import synthetic_unet_params_numpy
    net = UNetModel(device="cpu", **cfg)
    return net.load_state_dict(synthetic_unet_params_numpy(net.parameter_shapes(), 0))


def plans():
    """Yields (name, plan, extra op lists)."""
    from test_host_cpu import TINY_GLIDE, UNET_VARIANTS
    from minddiffusion_amd.configs import SMALL_WUKONG_UNET, TINY_UNET, TINY_VAE_DDCONFIG
    net = _unet(TINY_UNET)
    for shape in ((2, 8, 8), (3, 8, 12), (4, 8, 8)):
        yield f"tiny_unet {shape}", net._plan(*shape), ()
    yield "tiny_unet selfctx (2, 8, 8)", net._plan(2, 8, 8, _selfctx=True), ()
    for name in sorted(UNET_VARIANTS):
        yield f"variant {name} (2, 8, 8)", _unet(dict(TINY_UNET, **UNET_VARIANTS[name]))._plan(2, 8, 8), ()
    old = ops.get_option("unet_cfg_dup")
    ops.set_option("unet_cfg_dup", 4)
    try:
        wk = _unet(SMALL_WUKONG_UNET)
        yield "small_wukong (2, 8, 8)", wk._plan(2, 8, 8), ()
        P4 = wk._plan(4, 8, 8)
        yield "small_wukong (4, 8, 8) + dup_body", P4, (("dup_body", wk._dup_body(P4)),)
        P4 = net._plan(4, 8, 8)
        yield "tiny_unet (4, 8, 8) dup_body only", P4, (("dup_body", net._dup_body(P4)),)
    finally:
        ops.set_option("unet_cfg_dup", old)
    # the 320-channel build of test_unet_plan_fuses_the_320_channel_transformer_blocks, under its option sets
    cfg320 = dict(image_size=32, in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[1, 2],
                  num_res_blocks=1, channel_mult=[1, 2], num_head_channels=64, use_spatial_transformer=True,
                  use_linear_in_transformer=True, transformer_depth=1, context_dim=1024, legacy=False)
    option_sets = {"default": {},
                   "unfused+gn_proj_fuse": dict(unet_st_tail=0, unet_st_head=0, unet_gn_proj_fuse=1024),
                   "unfused": dict(unet_st_tail=0, unet_st_head=0, unet_gn_proj_fuse=0),
                   "unfused-xattn": dict(unet_st_tail=0, unet_st_head=0, unet_gn_proj_fuse=0, unet_xattn_fuse=0),
                   "gn_proj_fuse": dict(unet_gn_proj_fuse=1024),
                   "no_xattn": dict(unet_gn_proj_fuse=0, unet_xattn_fuse=0)}
    for oname, opts in option_sets.items():
        keep = {k: ops.get_option(k) for k in opts}
        try:
            for k, v in opts.items():
                ops.set_option(k, v)
            yield f"unet320 [{oname}] (2, 64, 64)", _unet(cfg320)._plan(2, 64, 64), ()
        finally:
            for k, v in keep.items():
                ops.set_option(k, v)
    yield "unet320 [default] (2, 16, 16)", _unet(cfg320)._plan(2, 16, 16), ()

    from oracle import glide as OG
    from minddiffusion_amd.glide.diffusion_creator import create_model, create_upsample_model
    otiny = dict(OG.BASE_OPTIONS, image_size=16, model_channels=64, num_res_blocks=1, channel_mult=(1, 2),
                 attention_resolutions=(1, 2), text_ctx=16, xf_width=64, xf_layers=2, xf_heads=1, n_vocab=100)
    g = create_model(device="cpu", **TINY_GLIDE)
    g.load_state_dict(OG.init_params(otiny, seed=0))
    yield "tiny_glide base (4, 16, 16)", g._plan(4, 16, 16), ()
    yield "tiny_glide text_plan(3)", g._text_plan(3), ()
    up = create_upsample_model(device="cpu", low_size=8, **dict(TINY_GLIDE, image_size=32, channel_mult=(1, 1, 2)))
    up.load_state_dict(OG.init_params(dict(otiny, in_channels=6, image_size=32, channel_mult=(1, 1, 2)), seed=1))
    yield "tiny_glide upsampler (2, 32, 32)", up._plan(2, 32, 32), ()

    from oracle import vae as OV
    from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
    vae = AutoencoderKL(ddconfig=dict(TINY_VAE_DDCONFIG), embed_dim=4, device="cpu")
    vae.load_state_dict(OV.init_params(dict(TINY_VAE_DDCONFIG), seed=0))
    yield "tiny_vae decoder (2, 16, 16)", vae.decoder._plan(2, 16, 16), ()
    yield "tiny_vae encoder (2, 32, 32)", vae.encoder._plan(2, 32, 32), ()

    from oracle import text_encoder as OT
    from minddiffusion_amd.ldm.modules.encoders.text_encoder import TextEncoder
    tcfg = dict(OT.SD2_TEXT, vocab_size=100, width=128, layers=3, heads=2)
    enc = TextEncoder(context_length=tcfg["context_length"], vocab_size=100, output_dim=128, width=128, layers=3, heads=2,
                      device="cpu")
    enc.load_state_dict(OT.init_params(tcfg, seed=1), prefix="transformer.")
    yield "tiny_text_encoder (2)", enc._plan(2), ()

    from test_srgan_cpu import synthetic_params
    from minddiffusion_amd.glide.model.srgan import Generator
    gen = Generator(4, device="cpu")
    gen.load_state_dict(synthetic_params(4, seed=0))
    yield "srgan x4 (1, 16, 16)", gen._plan(1, 16, 16), ()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default="", help="only the plans whose name contains this")
    ap.add_argument("--no-replay", action="store_true", help="descriptor / meta layer only")
    args = ap.parse_args()
    torch.manual_seed(0)
    np.random.seed(0)
    for name, P, extra in plans():
        if args.only in name:
            print("\n".join(fingerprint(name, P, not args.no_replay, extra)))


if __name__ == "__main__":
    main()
