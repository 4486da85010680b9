"""GPU parity of the SRGAN post-upscaler (glide/model/srgan.py): the two 9x9 kernels, the PReLU / depth-to-space epilogue of
mdx_gemm_f16 on every launch form a 3x3 conv resolves to, the HALO activation gate, the whole Generator against the fp32
reference of tests/test_srgan_cpu.py, graph replay, the GLIDE pipeline's upscale=True and sr_image.

Tolerances (fp16 storage, fp32 accumulation vs all-fp32): single launches on fp16-rounded operands rel-L2 <= 1e-3; the
Generator (37 convs) rel-L2 <= 2.5e-3 at 32^2 / 64^2 and <= 3e-3 at 256^2 -> 1024^2 (started from the VAE decoder's 5e-3 / 1e-2;
measured 0.74-1.13e-3 and 1.23e-3, docs/PARITY.md)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import check
from test_srgan_cpu import ref_generator, synthetic_params, torch_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def h16(t):
    return t.to(torch.float16).to(torch.float32)


def _prelu(x, a):
    return torch.where(x > 0, x, a.view(1, -1, 1, 1) * x)


# ---------------------------------------------------------------------------------------------------- 9x9 kernels
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(16, 16), (40, 24), (256, 256)])
def test_conv_in(B, H, W):
    from minddiffusion_amd import ops
    rng = np.random.RandomState(B * 1000 + H + W)
    x = torch.tensor(rng.uniform(-1, 1, (B, 3, H, W)).astype(np.float32))
    w = torch.tensor((rng.standard_normal((64, 3, 9, 9)) * (2.0 / 243) ** 0.5).astype(np.float32))
    b = torch.tensor(rng.uniform(-0.1, 0.1, 64).astype(np.float32))
    a = torch.tensor(rng.uniform(-0.3, 0.5, 64).astype(np.float32))
    ref = _prelu(F.conv2d(h16(x), h16(w), b, padding=4), a)
    got = ops.srgan_conv_in(x.to(DEV), w.to(torch.float16).to(DEV), b.to(DEV), a.to(DEV))
    check(f"srgan_conv_in_B{B}_{H}x{W}", got.permute(0, 3, 1, 2), ref, rel_l2=1e-3)


@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (3, 16, 16), (1, 40, 24), (3, 40, 24), (1, 256, 256), (3, 256, 256),
                                   (2, 1024, 1024)])
def test_conv_out(B, H, W):
    from minddiffusion_amd import ops
    rng = np.random.RandomState(B * 7 + H + 3 * W)
    x = torch.tensor(rng.standard_normal((B, 64, H, W)).astype(np.float32)).to(torch.float16)
    w = torch.tensor((rng.standard_normal((3, 64, 9, 9)) * 0.5 * (2.0 / 5184) ** 0.5).astype(np.float32))
    b = torch.tensor(rng.uniform(-0.1, 0.1, 3).astype(np.float32))
    pre = F.conv2d(x.float(), h16(w), b, padding=4)
    assert 0.2 <= float(pre.std()) <= 3.0
    got = ops.srgan_conv_out(x.permute(0, 2, 3, 1).contiguous().to(DEV), w.to(torch.float16).to(DEV), b.to(DEV), B, H, W)
    check(f"srgan_conv_out_B{B}_{H}x{W}", got, torch.tanh(pre), rel_l2=1e-3)


# ---------------------------------------------------------------------------------------------------- 3x3 epilogues
def _conv3_case(seed, B, H, W, N):
    rng = np.random.RandomState(seed)
    x = torch.tensor(rng.standard_normal((B, 64, H, W)).astype(np.float32)).to(torch.float16)
    w = torch.tensor((rng.standard_normal((N, 64, 3, 3)) * (2.0 / 576) ** 0.5).astype(np.float32)).to(torch.float16)
    b = torch.tensor(rng.uniform(-0.3, 0.3, N).astype(np.float32))
    a = torch.tensor(rng.uniform(-0.3, 0.5, 64).astype(np.float32))
    r = torch.tensor(rng.standard_normal((B, 64, H, W)).astype(np.float32)).to(torch.float16)
    return x, w, b, a, r


def _run3(x, w, b, N, forms, **kw):
    """Runs the conv with every override in `forms` and returns {form name: (kernel form, output)}."""
    from minddiffusion_amd import ops
    B, _, H, W = x.shape
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    wd = ops.pack_conv_weight(w.float().to(DEV))
    res = {}
    for name, ov in forms.items():
        args = dict(kw, **ov)
        if "residual" in args:
            args["residual"] = args["residual"].permute(0, 2, 3, 1).contiguous().to(DEV)
            args["residual_ld"] = 64
        if "act_slope" in args:
            args["act_slope"] = args["act_slope"].to(DEV)
        out_mode = args.get("out_mode", ops.OUT_ROWMAJOR)
        if out_mode == ops.OUT_D2S2:
            out = torch.full((B, 2 * H, 2 * W, N // 4), float("nan"), dtype=torch.float16, device=DEV)
            ld = N // 4
        else:
            out = torch.full((B * H * W, N), float("nan"), dtype=torch.float16, device=DEV)
            ld = N
        d = ops.make_gemm_desc(xd, wd, N, B, H, W, 64, out, ld, bias=b.to(DEV), ksize=3, **args)
        need = ops.gemm_workspace_bytes(d)
        if need:
            ws = ops.new_gemm_workspace(need, DEV)
            d.workspace, d.workspace_bytes = ws.data_ptr(), need
        q = ops.gemm_query(d)
        ops.gemm_run(d)
        torch.cuda.synchronize()
        res[name] = (q, out)
    return res


# the overrides of a 3x3 conv launch: auto, 64- / 128-row tiles, 64-column tiles, split K (slabs + reduce launch)
FORMS = {"auto": {}, "m64": {"tile_m": 64}, "m128": {"tile_m": 128}, "m128n64": {"tile_m": 128, "tile_n": 64},
         "split3": {"tile_m": 64, "splitk": 3}}


@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (3, 40, 24), (2, 64, 64)])
@pytest.mark.parametrize("with_res", [False, True])
def test_conv3_prelu(B, H, W, with_res):
    from minddiffusion_amd import ops
    x, w, b, a, r = _conv3_case(B + H + with_res, B, H, W, 64)
    ref = _prelu(F.conv2d(x.float(), w.float(), b, padding=1), a)
    if with_res:
        ref = ref + r.float()                           # residual AFTER the activation (srgan.py:113)
    kw = dict(epilogue=ops.EPI_PRELU, act_slope=a)
    if with_res:
        kw["residual"] = r
    for name, (q, out) in _run3(x, w, b, 64, FORMS, **kw).items():
        assert q[3] == 0, (name, q)                      # PReLU runs on the generic kernel (HALO / conv8p / lean dense exclude it)
        got = out.view(B, H, W, 64).permute(0, 3, 1, 2)
        check(f"conv3_prelu_{'res_' if with_res else ''}B{B}_{H}x{W}_{name}", got, ref, rel_l2=1e-3)


@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (3, 40, 24), (2, 64, 64)])
def test_conv3_d2s_prelu(B, H, W):
    from minddiffusion_amd import ops
    from test_srgan_cpu import ref_depth_to_space
    x, w, b, a, _ = _conv3_case(5 * B + H, B, H, W, 256)
    ref = _prelu(ref_depth_to_space(F.conv2d(x.float(), w.float(), b, padding=1)), a)     # DCR weight rows = identity
    for name, (q, out) in _run3(x, w, b, 256, FORMS, epilogue=ops.EPI_PRELU, act_slope=a, out_mode=ops.OUT_D2S2).items():
        assert q[3] == 0, (name, q)
        check(f"conv3_d2s_prelu_B{B}_{H}x{W}_{name}", out.permute(0, 3, 1, 2), ref, rel_l2=1e-3)


@pytest.mark.parametrize("epi", ["gelu", "quickgelu"])
def test_conv3_gelu_is_activated_on_halo_shapes(epi):
    """A 3x3 conv with GELU / QuickGELU at a shape the HALO kernel takes for the plain epilogue: the launch must store the
    activated output (the HALO store loop has no activation: the launch resolves to a form that has one)."""
    from minddiffusion_amd import ops
    B, H, W = 2, 32, 32
    x, w, b, _, _ = _conv3_case(11, B, H, W, 64)
    pre = F.conv2d(x.float(), w.float(), b, padding=1)
    if epi == "gelu":
        ref = 0.5 * pre * (1 + torch.tanh(0.7978845608028654 * (pre + 0.044715 * pre ** 3)))
        e = ops.EPI_GELU
    else:
        ref = pre * torch.sigmoid(1.702 * pre)
        e = ops.EPI_QUICKGELU
    plain = _run3(x, w, b, 64, {"auto": {}, "m128": {"tile_m": 128}})
    assert plain["m128"][0][3] == 1, plain["m128"][0]     # the plain conv of this shape does run on HALO
    for name, (q, out) in _run3(x, w, b, 64, {"auto": {}, "m128": {"tile_m": 128}, "m64": {"tile_m": 64}}, epilogue=e).items():
        got = out.view(B, H, W, 64).permute(0, 3, 1, 2)
        check(f"conv3_{epi}_B{B}_{H}x{W}_{name}", got, ref, rel_l2=1e-3)


# ---------------------------------------------------------------------------------------------------- Generator
def _generator(factor, seed, use_graph=True):
    from minddiffusion_amd.glide.model.srgan import Generator
    p = synthetic_params(factor, seed=seed)
    g = Generator(factor, device=DEV, use_graph=use_graph)
    g.load_state_dict(p)
    return g, torch_params(p)


def _image(B, H, W, seed):
    rng = np.random.RandomState(seed)
    return torch.tensor(np.tanh(rng.standard_normal((B, 3, H, W)) * 0.8).astype(np.float32))


@pytest.mark.parametrize("factor,B,S", [(2, 3, 32), (4, 3, 32), (2, 2, 64), (4, 2, 64)])
def test_generator_small(factor, B, S):
    g, tp = _generator(factor, seed=factor + S)
    x = _image(B, S, S, seed=S)
    pre = ref_generator(tp, x, factor, pre_tanh=True)
    assert 0.2 <= float(pre.std()) <= 3.0, float(pre.std())
    got = g(x.to(DEV))
    assert got.shape == (B, 3, factor * S, factor * S)
    check(f"srgan_x{factor}_B{B}_{S}", got, torch.tanh(pre), rel_l2=2.5e-3)


def test_generator_256_to_1024():
    from minddiffusion_amd.glide.model.srgan_util import get_img
    g, tp = _generator(4, seed=42)
    x = _image(2, 256, 256, seed=43)
    pre = ref_generator(tp, x, 4, pre_tanh=True)
    assert 0.2 <= float(pre.std()) <= 3.0, float(pre.std())
    ref = torch.tanh(pre)
    got = g(x.to(DEV)).cpu()
    m = check("srgan_x4_B2_256", got, ref, rel_l2=3e-3)
    u_got, u_ref = get_img(got).astype(np.int32), get_img(ref).astype(np.int32)
    frac = float((np.abs(u_got - u_ref) <= 1).mean())
    print("SRGAN uint8 within one level:", frac, m)
    assert frac >= 0.99, frac


def test_graph_replay_equals_eager_and_plans_per_shape():
    g, _ = _generator(2, seed=7)
    ge, _ = _generator(2, seed=7, use_graph=False)
    x = _image(2, 32, 32, seed=8).to(DEV)
    a = g(x).clone()
    b = g(x).clone()                                      # second call: graph replay
    assert g._plans[(2, 32, 32)].graph is not None
    e = ge(x).clone()
    assert torch.equal(a, b) and torch.equal(a, e)
    x3 = _image(3, 24, 40, seed=9).to(DEV)
    c = g(x3)
    assert c.shape == (3, 3, 48, 80) and len(g._plans) == 2
    assert torch.equal(g(x).clone(), a)


def test_pipeline_upscale():
    from minddiffusion_amd.glide.pipeline import GlidePipeline
    from test_distributed_gpu import _glide_models
    from minddiffusion_amd.glide.model.srgan import Generator
    P = 2
    dm, sr = _glide_models(P)
    gen = Generator(4, device=DEV)
    gen.load_state_dict(synthetic_params(4, seed=12))
    rng = np.random.RandomState(41)
    tok, msk = rng.randint(1, 99, (P, 16)).astype(np.int32), np.ones((P, 16), np.int32)
    plain = GlidePipeline(dm, sr, text_ctx=16, vocab_len=100)(tokens=tok, mask=msk, seed=5).clone()
    pipe = GlidePipeline(dm, sr, text_ctx=16, vocab_len=100, srgan=gen)
    same = pipe(tokens=tok, mask=msk, seed=5).clone()
    assert torch.equal(same, plain)
    up = pipe(tokens=tok, mask=msk, seed=5, upscale=True)
    S = plain.shape[-1]
    assert up.shape == (P, 3, 4 * S, 4 * S)
    assert torch.equal(pipe.last_up256, plain)
    assert torch.equal(up, gen(pipe.last_up256.contiguous()))


def test_sr_image_round_trip(tmp_path):
    from PIL import Image
    from minddiffusion_amd.glide.model import srgan_util
    p = synthetic_params(4, seed=21)
    sr = srgan_util.SRGAN(4, params=p, device=DEV)
    rng = np.random.RandomState(22)
    img = rng.randint(0, 256, (24, 40, 3)).astype(np.uint8)
    src, dst = str(tmp_path / "lr.png"), str(tmp_path / "hr.png")
    Image.fromarray(img).save(src)
    sr.sr_image(src, dst)
    out = np.array(Image.open(dst))
    assert out.shape == (96, 160, 3) and out.dtype == np.uint8
    x = torch.tensor((img / 127.5 - 1.0).transpose(2, 0, 1)[None].astype(np.float32))
    ref = ref_generator(torch_params(p), x, 4)[0].numpy()
    want = ((np.clip(ref, -1, 1) + 1) / 2 * 255).transpose(1, 2, 0).astype(np.uint8)
    assert float((np.abs(out.astype(np.int32) - want.astype(np.int32)) <= 1).mean()) >= 0.99
