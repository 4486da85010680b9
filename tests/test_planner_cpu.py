"""The shared plan builder (minddiffusion_amd/planner.py) on the host: nothing is launched."""
import os
import sys

import torch

from minddiffusion_amd import ops
from minddiffusion_amd.planner import PlanBuilder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from plan_fingerprint import gemm_desc_sequence  # noqa: E402

f16, f32 = torch.float16, torch.float32


def _dense_args(cin=64, nout=64):
    w = ops.pack_gemm_weight(torch.zeros((nout, cin), dtype=f16))
    return w, torch.zeros(nout, dtype=f32)


def test_a_buffer_handed_out_again_is_nobodys_producer():
    pb = PlanBuilder("cpu", 2, track_producers=True)
    w, b = _dense_args()
    x = pb.get((2, 64, 64))
    y = pb.dense(x, 2, 64, 64, 64, w, bias=b)
    d = pb.descs[-1]
    assert pb.producer[y.data_ptr()] is d and pb.op_index[__import__("ctypes").addressof(d)] == 0
    pb.release(y)
    z = pb.get((2, 64, 64))                 # exact-size bucket: the same storage comes back
    assert z.data_ptr() == y.data_ptr() and z.data_ptr() not in pb.producer
    # ... and a GroupNorm planned on it sees no producer, while one planned on a live GEMM output does
    y2 = pb.dense(x, 2, 64, 64, 64, w, bias=b)
    g = torch.ones(64, dtype=f32)
    pb.gn(z, None, g, g, 1e-5, True, pb.get((2, 64, 64)))
    pb.gn(y2, None, g, g, 1e-5, True, pb.get((2, 64, 64)))
    assert pb.gn_calls[0]["prod"] == (None, None) and pb.gn_calls[1]["prod"][0] is pb.descs[-1]


def _tiny_plans():
    from test_host_cpu import TINY_GLIDE
    from oracle import glide as OG, vae as OV
    from minddiffusion_amd.configs import TINY_UNET, TINY_VAE_DDCONFIG
    from minddiffusion_amd.glide.diffusion_creator import create_model
    from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from minddiffusion_amd.weights import synthetic_unet_params_numpy
    net = UNetModel(device="cpu", **TINY_UNET)
    net.load_state_dict(synthetic_unet_params_numpy(net.parameter_shapes(), 0))
    otiny = dict(OG.BASE_OPTIONS, image_size=16, model_channels=64, num_res_blocks=1, channel_mult=(1, 2),
                 attention_resolutions=(1, 2), text_ctx=16, xf_width=64, xf_layers=2, xf_heads=1, n_vocab=100)
    glide = create_model(device="cpu", **TINY_GLIDE)
    glide.load_state_dict(OG.init_params(otiny, seed=0))
    vae = AutoencoderKL(ddconfig=dict(TINY_VAE_DDCONFIG), embed_dim=4, device="cpu")
    vae.load_state_dict(OV.init_params(dict(TINY_VAE_DDCONFIG), seed=0))
    return glide, {"unet": net._plan(2, 8, 8), "glide": glide._plan(4, 16, 16), "glide_text": glide._text_plan(3),
                   "vae_dec": vae.decoder._plan(2, 16, 16), "vae_enc": vae.encoder._plan(2, 32, 32)}


def test_finished_plans_share_one_sufficient_workspace_and_untracked_ones_wire_no_statistics():
    glide, plans = _tiny_plans()
    for name, P in plans.items():
        assert len(P.main) == len(P.meta) > 0, name
        ws, nbytes = P.gemm_ws.data_ptr(), P.gemm_ws.numel() * 4
        for d in P.descs:
            assert d.workspace == ws and d.workspace_bytes == nbytes, name
            assert ops.gemm_workspace_bytes(d) <= d.workspace_bytes, name
        gemms = [m for m in P.meta if m["kind"] == "gemm" and "desc" in m]
        assert gemms and all(" split=" in m["info"] and m["launches"] in (1, 2) for m in gemms), name
    for name in ("glide_text", "vae_dec", "vae_enc"):       # built without producer tracking
        assert not any(d.colstats_out for d in plans[name].descs), name


def test_glide_text_prefix_and_text_plan_record_the_same_gemm_descriptors():
    """Host-side guard of the bit identity tests/test_glide_gpu.py asserts on the device: the step plan's text prefix and the
    whole-loop table pass at the same row count are the same sequence of launches (pointers as ordinals of first appearance;
    the shared workspace is each plan's own and sized for different launches, so its size is left out)."""
    glide, plans = _tiny_plans()
    P = plans["glide"]
    T = glide._text_plan(P.B)
    prefix = [m["desc"] for m in P.meta[:P.n_text] if "desc" in m]
    assert all(m["text"] for m in P.meta[:P.n_text]) and not any(m["text"] for m in P.meta[P.n_text:])
    assert len(prefix) == len(T.descs) > 0 and all(d.splitk == 1 for d in prefix + list(T.descs))

    def fields(descs):
        return [" ".join(f for f in line.split() if not f.startswith("workspace_bytes=")) for line in gemm_desc_sequence(descs)]
    # the step plan writes the encoder_kv rows into the blocks' [text | image] key / value buffers, the table pass into
    # tables of their own: compare the transformer launches in full and the encoder_kv launches up to their output strides
    n_xf = 5 * glide.xf_layers          # qk, v, proj, fc, fc2 per layer
    assert fields(prefix[:n_xf]) == fields(T.descs[:n_xf])
    for a, b in zip(prefix[n_xf:], T.descs[n_xf:]):
        assert (a.N, a.B, a.H, a.W, a.c1, a.out_mode, a.epilogue, a.splitk) == (b.N, b.B, b.H, b.W, b.c1, b.out_mode, b.epilogue, b.splitk)
        assert a.a and b.a and bool(a.bias) and bool(b.bias)
