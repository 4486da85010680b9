"""Long prompts on the GPU: a text context of several 77-token CLIP windows ([B, n * 77, D]) through the two fused cross-attention
paths and everything above them.

  * mdx_st_tail_f16 (csrc/stchain.hip, stage S3): contexts past 96 keys run 96-key chunks with online softmax.  Against
    `chain_ref(round16=True)` of tests/test_stchain_gpu.py at that file's own bars (rel_l2 1e-3, max_rel 6e-3); a context of at
    most 96 keys keeps the bits of the commit before (tests/golden/st_tail_parent.npz).
  * the cross-attention epilogue of the lean dense kernel (csrc/dense.hip): more than two 64-key tiles, re-staged pair by pair;
    `torch.equal` against projection + mdx_attention_f16, as tests/test_kernels_gpu.py::test_dense_with_cross_attention_epilogue.
  * UNetModel(max_context_len=) / set_max_context_len, TextEncoder on [B, n, 77] ids, pad_conditioning + DiffusionPipeline.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from _guard import assert_footprint, guarded, poisoned
from _util import check, h16
from oracle import ldm as O
from oracle import text_encoder as OT
from test_stchain_gpu import chain_ref, make_case, run_fused, unfused_chain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS = dict(rel_l2=1e-3, max_rel=6e-3)      # tests/test_stchain_gpu.py's bars against the fp16-storage restatement


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.float16)


def cap_of(n):
    return (n + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------ mdx_st_tail_f16
B, TOKENS, C = 1, 64, 320


@functools.lru_cache(maxsize=None)
def tail_case(heads, ctx_len, ctx_cap, outlier=None):
    """(w, x, fp16-storage reference): computed once per case, shared by the tests that read it (nobody writes to it)."""
    w, x = make_case(100 + heads + ctx_len, B, TOKENS, C, heads, ctx_len, 1024 if heads == 5 else 768, ctx_cap=ctx_cap)
    if outlier is not None:
        x["k"][:, outlier] *= 12.0
        x["k"][:, 3] *= -9.0
        x["k"] = h16(x["k"])
    return w, x, chain_ref(w, x, B, TOKENS, C, heads, ctx_len, True)


@pytest.mark.parametrize("heads", [5, 8])
@pytest.mark.parametrize("ctx_len,ctx_cap", [(96, 96), (97, 104), (154, 160), (192, 192), (231, 232), (77, 240)])
def test_st_tail_chunk_boundaries(ops, heads, ctx_len, ctx_cap):
    """96: the last one-chunk length; 97: one key in chunk 2; 192: an exact chunk boundary; 154 / 231: two and three CLIP windows;
    77 keys in a capacity-240 buffer: a short prompt in a long plan (the one-chunk form, V^T row stride 240)."""
    w, x, ref = tail_case(heads, ctx_len, ctx_cap)
    for stage, name in ((4, "xattn"), (0, "out")):
        got, _ = run_fused(ops, w, x, B, TOKENS, C, heads, ctx_len, 64, stage, ctx_cap=ctx_cap)
        check(f"st_tail_long_h{heads}_ctx{ctx_len}_cap{ctx_cap}_{name}", got, ref[stage], **BARS)


def test_st_tail_two_chunks_in_32_row_blocks(ops):
    w, x, ref = tail_case(5, 154, 160)
    for stage, name in ((4, "xattn"), (0, "out")):
        got, _ = run_fused(ops, w, x, B, TOKENS, C, 5, 154, 32, stage, ctx_cap=160)
        check(f"st_tail_long_r32_ctx154_{name}", got, ref[stage], **BARS)


@pytest.mark.parametrize("outlier", [50, 120])
def test_st_tail_running_maximum(ops, outlier):
    """One key's logits far above the rest (tests/test_stchain_gpu.py::test_st_tail_attention_outlier_keys) at 154 keys: in chunk 1
    (key 50) the running maximum never moves after the first chunk, so no rescale fires; in chunk 2 (key 120) the rescale fires
    with a large step and chunk 1's contribution all but vanishes."""
    w, x, ref = tail_case(5, 154, 160, outlier)
    got, _ = run_fused(ops, w, x, B, TOKENS, C, 5, 154, 64, 4, ctx_cap=160)
    check(f"st_tail_long_outlier_key{outlier}_xattn", got, ref[4], **BARS)
    got, _ = run_fused(ops, w, x, B, TOKENS, C, 5, 154, 64, 0, ctx_cap=160)
    check(f"st_tail_long_outlier_key{outlier}_out", got, ref[0], **BARS)


def test_st_tail_multi_chunk_distance_next_to_the_unfused_chain(ops):
    """For docs/PARITY.md: distance of the fused tail and of the unfused launches (projection + mdx_attention_f16, itself online
    softmax) to the same fp16-storage reference on the same 154-key inputs.  The fused tail is held to the file's bars."""
    w, x, ref = tail_case(5, 154, 160)
    un = unfused_chain(ops, w, x, B, TOKENS, C, 5, 154, ctx_cap=160)
    got, _ = run_fused(ops, w, x, B, TOKENS, C, 5, 154, 64, 0, ctx_cap=160)
    check("unfused_chain_ctx154_out_vs_fp16ref", un, ref[0])
    check("st_tail_long_ctx154_out_vs_fp16ref", got, ref[0], **BARS)


@pytest.mark.parametrize("heads", [5, 8])
@pytest.mark.parametrize("tile_rows", [64, 32])
def test_st_tail_one_chunk_keeps_the_parent_bits(ops, heads, tile_rows):
    """tests/golden/st_tail_parent.npz (make_st_tail_parent_golden.py): a 77-key context in a capacity-80 buffer gives the bits
    the commit before the chunk loop gave, on the same device."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_st_tail_parent_golden as G
    gold = np.load(os.path.join(ROOT, "tests", "golden", "st_tail_parent.npz"))
    w, x = G.case_inputs(heads)
    got, _ = run_fused(ops, w, x, G.B, G.TOKENS, G.C, heads, G.CTX_LEN, tile_rows, 0, ctx_cap=G.CAP)
    assert torch.equal(got.cpu(), torch.from_numpy(gold[f"h{heads}_r{tile_rows}"])), "the one-chunk path changed its bits"


@pytest.mark.parametrize("tile_rows", [32, 64])
def test_warmer_schedule_matches_the_compute_waves_at_two_chunks(ops, tile_rows):
    """Twin of tests/test_stchain_gpu.py::test_warmer_schedules_match_the_compute_waves at 154 keys in a capacity-160 buffer: the
    chunk loop adds no block barrier."""
    from minddiffusion_amd import _lib
    lib = _lib.load()
    heads, ctx_len = 5, 154
    w, x = make_case(5, 1, 128, C, heads, ctx_len, 1024, ctx_cap=160)
    dbg, _ = run_fused(ops, w, x, 1, 128, C, heads, ctx_len, tile_rows, stage=100, ctx_cap=160)
    n_tail = int(dbg.view(torch.int32).reshape(-1)[0])
    assert n_tail == lib.mdx_st_tail_sched_barriers(C, tile_rows), (n_tail, lib.mdx_st_tail_sched_barriers(C, tile_rows))


def test_st_tail_footprint_at_capacity_160(ops):
    """Output rows inside a sentinel-guarded allocation, K / V^T inside NaN-filled ones (zero between ctx_len and the capacity, as
    the product fills them): nothing outside the output is written, the context buffers are unchanged, and the result depends on
    nothing outside the operands."""
    heads, ctx_len, cap = 8, 154, 160
    w, x, ref = tail_case(heads, ctx_len, cap)
    stream, vec = ops.pack_st_tail(*(dev16(w[n]) for n in ("o1", "q2", "o2", "ff1", "ff2", "po")),
                                   *(torch.from_numpy(w[n]).to(DEV) for n in ("bo1", "g2", "be2", "bo2", "g3", "be3", "b1", "b2", "bpo")))
    t = {n: dev16(x[n]) for n in ("attn_o", "tok", "x_in")}
    kbuf, kd = poisoned(x["k"][:, :ctx_len], dtype=torch.float16, zero_shape=(B, cap, C), device=DEV)
    vbuf, vd = poisoned(x["vt"][:, :, :ctx_len], strides=(C * cap, cap, 1), dtype=torch.float16, zero_shape=(B, C, cap), device=DEV)
    kd, vd = kbuf.as_strided((B, cap, C), (cap * C, C, 1), kd.storage_offset()), vbuf.as_strided((B, C, cap), (C * cap, cap, 1), vd.storage_offset())
    k0, v0 = kbuf.clone(), vbuf.clone()
    obuf, out = guarded((B * TOKENS, C), device=DEV)
    d = ops.make_st_tail_desc(t["attn_o"], t["tok"], t["x_in"], out, kd, vd, stream, vec, B, TOKENS, C, heads, C // heads, ctx_len, cap,
                              tile_rows=64)
    ops.st_tail_run(d)
    assert_footprint(obuf, out, "st_tail_cap160", written=True)
    assert torch.equal(kbuf.view(torch.int16), k0.view(torch.int16)) and torch.equal(vbuf.view(torch.int16), v0.view(torch.int16))
    check("st_tail_cap160_footprint_out", out, ref[0], **BARS)


# ------------------------------------------------------------------------------------------------ dense cross-attention epilogue
def _xattn_case(ops, Bx, T, Cx, L, tile_m, lnfold, outlier=None, guard=False):
    """The form of tests/test_kernels_gpu.py::test_dense_with_cross_attention_epilogue; returns (fused, two launches, fp32 torch)."""
    heads = Cx // 64
    cap = cap_of(L)
    rng = np.random.RandomState(Bx * T + Cx + L)
    x = h16(rng.standard_normal((Bx * T, Cx)))
    wq = h16(rng.standard_normal((Cx, Cx)) / math.sqrt(Cx))
    k = h16(0.7 * rng.standard_normal((Bx, L, Cx)))
    v = h16(rng.standard_normal((Bx, L, Cx)))
    if outlier is not None:
        k[:, outlier] = h16(k[:, outlier] * 12.0)
    vt = np.ascontiguousarray(v.transpose(0, 2, 1))
    if guard:
        kbuf, kv = poisoned(k, dtype=torch.float16, zero_shape=(Bx, cap, Cx), device=DEV)
        vbuf, vv = poisoned(vt, strides=(Cx * cap, cap, 1), dtype=torch.float16, zero_shape=(Bx, Cx, cap), device=DEV)
        kd = kbuf.as_strided((Bx, cap, Cx), (cap * Cx, Cx, 1), kv.storage_offset())
        vtd = vbuf.as_strided((Bx, Cx, cap), (Cx * cap, cap, 1), vv.storage_offset())
    else:
        kd = torch.zeros((Bx, cap, Cx), dtype=torch.float16, device=DEV)
        kd[:, :L] = dev16(k)
        vtd = torch.zeros((Bx, Cx, cap), dtype=torch.float16, device=DEV)
        vtd[:, :, :L] = dev16(vt)
        kbuf, vbuf = kd, vtd
    xd = dev16(x)
    scale = 64 ** -0.5
    kw = {}
    if lnfold:
        g = (1.0 + 0.1 * rng.standard_normal(Cx)).astype(np.float32)
        bt = (0.1 * rng.standard_normal(Cx)).astype(np.float32)
        xt = torch.tensor(x).float()
        xn = (xt - xt.mean(1, keepdim=True)) / torch.sqrt(xt.var(1, unbiased=False, keepdim=True) + 1e-5) * torch.tensor(g) + torch.tensor(bt)
        qref = xn @ torch.tensor(wq).float().T
        wg, sv, cb = ops.fold_layernorm(torch.tensor(wq).to(DEV), torch.tensor(g).to(DEV), torch.tensor(bt).to(DEV))
        wd = ops.pack_gemm_weight(wg)
        nt = Cx // 64
        st = torch.zeros((Bx * T, nt, 2), dtype=torch.float32, device=DEV)
        xs = xd.float().reshape(Bx * T, nt, 64)
        st[:, :, 0], st[:, :, 1] = xs.sum(2), (xs * xs).sum(2)
        kw = dict(ln_stats=st, ln_s=sv, bias=cb)
    else:
        qref = torch.tensor(x).float() @ torch.tensor(wq).float().T
        wd = ops.pack_gemm_weight(dev16(wq))
    qh = qref.reshape(Bx, T, heads, 64).permute(0, 2, 1, 3)
    kh = torch.tensor(k).float().reshape(Bx, L, heads, 64).permute(0, 2, 1, 3)
    vh = torch.tensor(v).float().reshape(Bx, L, heads, 64).permute(0, 2, 1, 3)
    ref = torch.matmul(torch.softmax(torch.matmul(qh, kh.transpose(2, 3)) * scale, -1), vh).permute(0, 2, 1, 3).reshape(Bx * T, Cx)
    q = torch.empty((Bx * T, Cx), dtype=torch.float16, device=DEV)
    ops.gemm_run(ops.make_gemm_desc(xd, wd, Cx, Bx, T, 1, Cx, q, Cx, tile_n=64, splitk=1, tile_m=tile_m, **kw))
    two = torch.empty((Bx * T, Cx), dtype=torch.float16, device=DEV)
    ops.attention(q.data_ptr(), kd.data_ptr(), vtd.data_ptr(), two.data_ptr(), Bx, heads, 64, T, L, scale,
                  T * Cx, Cx, cap * Cx, Cx, Cx * cap, cap, T * Cx, Cx)
    torch.cuda.synchronize()
    k0, v0 = kbuf.clone(), vbuf.clone()
    if guard:
        obuf, one = guarded((Bx * T, Cx), strides=(Cx + 8, 1), device=DEV)
    else:
        obuf = one = torch.full((Bx * T, Cx), float("nan"), dtype=torch.float16, device=DEV)
    d1 = ops.make_gemm_desc(xd, wd, Cx, Bx, T, 1, Cx, one, one.stride(0), tile_n=64, splitk=1, tile_m=tile_m, xattn_k=kd, xattn_vt=vtd,
                            xattn_len=L, xattn_cap=cap, xattn_scale=scale, **kw)
    qq = ops.gemm_query(d1)
    assert qq[3] == 2 and qq[1] == 64 and qq[2] == 1, qq
    ops.gemm_run(d1)
    torch.cuda.synchronize()
    if guard:
        assert_footprint(obuf, one, f"dense_xattn_L{L}", written=True)
    assert torch.equal(kbuf.view(torch.int16), k0.view(torch.int16)) and torch.equal(vbuf.view(torch.int16), v0.view(torch.int16))
    return one, two, ref


@pytest.mark.parametrize("Bx,T,Cx,L,tile_m,lnfold", [
    (1, 128, 64, 129, 0, False),      # one key in the third tile: the first re-staged pair holds a single masked tile
    (2, 128, 128, 154, 0, True),      # two CLIP windows, the LayerNorm-fold consumer form the planner emits
    (1, 64, 192, 231, 64, False),     # three windows = four tiles, 64-row tiles (two waves only stage)
    (1, 128, 64, 256, 0, False),      # four full tiles: no masked tile
    (1, 128, 64, 192, 0, False),      # three full tiles: an odd count, unmasked
])
def test_dense_cross_attention_epilogue_past_two_tiles(ops, Bx, T, Cx, L, tile_m, lnfold):
    one, two, ref = _xattn_case(ops, Bx, T, Cx, L, tile_m, lnfold)
    assert torch.equal(one, two), f"fused cross-attention differs from projection + mdx_attention_f16: max |d| = {(one.float() - two.float()).abs().max().item():.3e}"
    check(f"dense_xattn_long_B{Bx}_T{T}_C{Cx}_L{L}_tm{tile_m}_ln{int(lnfold)}", one, ref, rel_l2=3e-3, max_abs=3e-2)


def test_dense_cross_attention_epilogue_outlier_in_tile_3(ops):
    """A dominating key in the third tile (key 140 of 154): the lazy rescale fires after the re-staging hand-over."""
    one, two, ref = _xattn_case(ops, 1, 128, 64, 154, 0, False, outlier=140)
    assert torch.equal(one, two)
    check("dense_xattn_long_outlier_key140", one, ref, rel_l2=3e-3, max_abs=3e-2)


def test_dense_cross_attention_epilogue_footprint_at_154_keys(ops):
    one, two, ref = _xattn_case(ops, 2, 128, 128, 154, 0, False, guard=True)
    assert torch.equal(one, two)
    check("dense_xattn_long_footprint_L154", one, ref, rel_l2=3e-3, max_abs=3e-2)


# ------------------------------------------------------------------------------------------------ UNet
def _ocfg(cfg):
    c = dict(cfg)
    c.setdefault("num_heads", -1)
    c.setdefault("num_head_channels", -1)
    return c


def _net(cfg, params, graph, **kw):
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    net = UNetModel(**cfg, **kw)
    net.use_graph = graph
    net.load_state_dict(params)
    return net


def _inputs(Bn, H, W, T, D, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(Bn, 4, H, W).astype(np.float32), rng.randn(Bn, T, D).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _tiny():
    from minddiffusion_amd.configs import TINY_UNET
    cfg = dict(TINY_UNET)
    params = O.init_params(_ocfg(cfg), seed=4)
    return cfg, params, O.UNetOracle(_ocfg(cfg), params)


@functools.lru_cache(maxsize=None)
def _tiny_refs():
    cfg, params, oracle = _tiny()
    refs = {}
    for T in (154, 77, 231):
        x, ctx = _inputs(2, 8, 8, T, cfg["context_dim"], seed=10 + T)
        refs[T] = (x, ctx, oracle(x, torch.full((2,), 250.0), ctx))
    return refs


@pytest.mark.parametrize("graph", [False, True])
def test_tiny_unet_long_contexts_through_one_net(ops, graph):
    """Two windows, one, three, two again through one net built with max_context_len=240 (head dim 64: the cross-attention rides on
    its query projection), each against the oracle; the two 154-token evaluations agree bit for bit, and so does the same evaluation
    with the epilogue off (projection + mdx_attention_f16)."""
    cfg, params, _ = _tiny()
    net = _net(cfg, params, graph, max_context_len=240)
    assert net.max_context_len == 240
    assert any("+cross-attention" in m["info"] for m in net._plan(2, 8, 8).meta), "the tiny UNet should fuse at capacity 240"
    outs = []
    for T in (154, 77, 231, 154):
        x, ctx, ref = _tiny_refs()[T]
        got = net(torch.tensor(x, device=DEV), torch.full((2,), 250.0, device=DEV), torch.tensor(ctx, device=DEV))
        check(f"long_context_tiny_T{T}_graph{int(graph)}", got, ref, rel_l2=5e-3)
        outs.append(got.clone())
    assert torch.equal(outs[0], outs[3])
    old = ops.get_option("unet_xattn_fuse")
    ops.set_option("unet_xattn_fuse", 0)
    try:
        net0 = _net(cfg, params, graph, max_context_len=240)
        assert not any("+cross-attention" in m["info"] for m in net0._plan(2, 8, 8).meta)
        x, ctx, _ = _tiny_refs()[154]
        two = net0(torch.tensor(x, device=DEV), torch.full((2,), 250.0, device=DEV), torch.tensor(ctx, device=DEV))
    finally:
        ops.set_option("unet_xattn_fuse", old)
    assert torch.equal(two, outs[0]), "the fused long cross-attention changes the UNet's bits"


def test_wukong_style_unet_runs_the_fused_tail_at_154_tokens():
    from minddiffusion_amd.configs import SMALL_WUKONG_UNET
    cfg = dict(SMALL_WUKONG_UNET)
    params = O.init_params(_ocfg(cfg), seed=21)
    net = _net(cfg, params, True, max_context_len=160)
    assert net._plan(2, 64, 64).tails, "B = 2 at 64 x 64 (256 row blocks) should plan the fused tail at capacity 160"
    x, ctx = _inputs(2, 64, 64, 154, cfg["context_dim"], seed=31)
    ts = np.full((2,), 437.0, np.float32)
    got = net(torch.tensor(x, device=DEV), torch.tensor(ts, device=DEV), torch.tensor(ctx, device=DEV))
    check("long_context_wukong_style_64x64_T154", got, O.UNetOracle(_ocfg(cfg), params)(x, torch.tensor(ts), ctx), rel_l2=5e-3,
          max_abs=5e-2)


def test_default_unet_refuses_154_tokens_until_the_capacity_is_raised():
    from minddiffusion_amd._lib import MdxError
    cfg, params, _ = _tiny()
    net = _net(cfg, params, True)
    x, ctx, ref = _tiny_refs()[154]
    args = (torch.tensor(x, device=DEV), torch.full((2,), 250.0, device=DEV), torch.tensor(ctx, device=DEV))
    with pytest.raises(MdxError, match="max_context_len"):
        net(*args)
    net.set_max_context_len(154)
    assert net.max_context_len == 160
    check("long_context_tiny_after_set_max_context_len", net(*args), ref, rel_l2=5e-3)


# ------------------------------------------------------------------------------------------------ text encoder
def test_text_encoder_takes_windows_of_a_long_prompt():
    from minddiffusion_amd.ldm.modules.encoders.text_encoder import TextEncoder
    cfg = dict(OT.SD2_TEXT, vocab_size=100, width=128, layers=3, heads=2, act="gelu_tanh")
    params = OT.init_params(cfg, seed=1)
    enc = TextEncoder(context_length=77, vocab_size=100, output_dim=128, width=128, layers=3, heads=2, act="gelu_tanh", device=DEV,
                      ln_eps=cfg.get("ln_eps", 1e-5))
    enc.load_state_dict(params, prefix="transformer.")
    tok = np.random.RandomState(3).randint(0, 100, (2, 3, 77))
    ref = np.concatenate([np.asarray(OT.encode_tokens(params, tok[:, i], cfg)) for i in range(3)], axis=1)
    got = enc(tok)
    assert tuple(got.shape) == (2, 231, 128) and got.dtype == torch.float16
    check("text_encoder_windows_2x3x77", got, ref, rel_l2=5e-3, max_abs=5e-2)
    flat = enc(tok[:, 0])
    assert tuple(flat.shape) == (2, 77, 128) and torch.equal(flat, enc(tok[:, 0]))


# ------------------------------------------------------------------------------------------------ pipeline
def _pipeline(sampler):
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from minddiffusion_amd.pipeline import DiffusionPipeline
    cfg, params, oracle = _tiny()
    net = _net(cfg, params, True)
    model = LatentDiffusion(net, linear_start=0.00085, linear_end=0.0120, timesteps=1000)
    return DiffusionPipeline(model, sampler=sampler), O.ModelOracle(oracle), cfg["context_dim"]


def _conditioning(D):
    rng = np.random.RandomState(55)
    return (rng.randn(2, 154, D).astype(np.float32), rng.randn(1, 77, D).astype(np.float32), rng.randn(1, 77, D).astype(np.float32),
            rng.randn(2, 4, 8, 8).astype(np.float32))


@pytest.mark.parametrize("sampler", ["ddim", "plms"])
def test_pipeline_two_steps_with_a_long_c_and_a_short_uc(sampler):
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.modules.encoders import pad_conditioning
    pipe, omodel, D = _pipeline(sampler)
    c, uc, empty, x_T = _conditioning(D)
    with pytest.raises(MdxError, match="pad_conditioning"):
        pipe(c=torch.tensor(c), uc=torch.tensor(uc), H=64, W=64, steps=2, scale=3.0, x_T=torch.tensor(x_T))
    c2, uc2 = pad_conditioning(torch.tensor(c), torch.tensor(uc), torch.tensor(empty))
    assert tuple(c2.shape) == (2, 154, D) and tuple(uc2.shape) == (1, 154, D)
    got = pipe(c=c2, uc=uc2, H=64, W=64, steps=2, scale=3.0, x_T=torch.tensor(x_T))
    assert pipe.model.unet.max_context_len == 160      # raised from 80 to the next multiple of 80
    ref, _ = O.sample(omodel, 2, 2, (4, 8, 8), c2.numpy(), x_T, sampler, unconditional_guidance_scale=3.0,
                      unconditional_conditioning=np.repeat(uc2.numpy(), 2, 0))
    check(f"long_context_pipeline_{sampler}_S2", got, ref, rel_l2=1e-2, max_rel=1e-2)


def test_pipeline_img2img_with_a_long_c_and_a_short_uc():
    from minddiffusion_amd.ldm.modules.encoders import pad_conditioning
    pipe, omodel, D = _pipeline("ddim")
    c, uc, empty, z0 = _conditioning(D)
    noise = np.random.RandomState(56).randn(2, 4, 8, 8).astype(np.float32)
    c2, uc2 = pad_conditioning(torch.tensor(c), torch.tensor(uc), torch.tensor(empty))
    S, t_enc = 4, 2
    got = pipe.img2img(init_latent=torch.tensor(z0), strength=0.5, c=c2, uc=uc2, steps=S, scale=3.0, noise=torch.tensor(noise, device=DEV))
    t = int(O.make_ddim_timesteps(S, omodel.num_timesteps)[t_enc - 1])
    x_enc = omodel.q_sample(torch.tensor(z0), torch.full((2,), t, dtype=torch.int64), torch.tensor(noise))
    assert int(min((t_enc + 1) / S, 1) * S) - 1 == t_enc
    ref, _ = O.sample(omodel, S, 2, (4, 8, 8), c2.numpy(), x_enc, "ddim", unconditional_guidance_scale=3.0,
                      unconditional_conditioning=np.repeat(uc2.numpy(), 2, 0), timesteps=t_enc + 1)
    check("long_context_pipeline_img2img_ddim", got, ref, rel_l2=1e-2, max_rel=1e-2)
