"""Write footprints and input independence of the MFMA kernel families: mdx_gemm_f16 in its launch forms (generic, lean dense,
128 x 160 tile, HALO 8 x 16 / HALO8 / weight-streaming convs, conv8p and its sub-pixel form, transposed / split / depth-to-space
stores), the attention kernels, mdx_st_head_f16 / mdx_st_tail_f16 and the two SRGAN 9 x 9 convs.

Every case is an ordinary parity test -- the launch against a float64 reference computed from the same fp16-rounded operands, at the
tolerance the project already states for that kernel -- run the way the product runs it and no existing test does:
  * every output (out, out2, stats_out, colstats_out, debug_out, the split-K / split-KV workspace) sits inside a sentinel-filled
    allocation (tests/_guard.py) with a leading dimension larger than its logical width; after the launch every element outside the
    logical output must still hold the sentinel bit for bit, and every element inside must have been written;
  * every input sits inside a NaN-filled allocation, with NaN in its stride gaps; memory a header requires to be finite (vt columns
    Nk .. vt_ld - 1, context rows ctx_len .. ctx_cap - 1) is zero as the product leaves it.  A result that depends on anything
    outside the logical operands is not finite and fails `check`;
  * the workspace is exactly as large as the library asks (ops.gemm_workspace_bytes / the documented split-KV size), and the arrival
    counters (caller-owned here) must be back at zero.
Each GEMM / conv case asserts through ops.gemm_query that it runs the launch form it means to test.  The case table lives in
tests/_footprint_cases.py (no device access: tests/test_footprint_cpu.py resolves every row on the host).
"""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _guard as G
from _footprint_cases import CASES, CONV_CASES, DENSE_CASES, TRANSPOSED_CASES, expected_query, make_desc, out_hw, out_ld, width  # noqa: F401
from _util import check, h16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS_PAD = 2 * 256 * 192      # fp32 elements around a workspace: two of the largest tile's partials


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def options(ops, **kw):
    keep = {k: ops.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            ops.set_option(k, v)
        yield
    finally:
        for k, v in keep.items():
            ops.set_option(k, v)


def seed_of(*parts):
    return sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(map(str, parts)))) % (2 ** 31)


def dev(a, dtype=torch.float16):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def pin(a, shape=None, strides=None, dtype=torch.float16, **kw):
    """A poisoned device input (tests/_guard.py): returns the view; the view keeps the allocation alive."""
    return G.poisoned(np.asarray(a), shape, strides, dtype=dtype, device=DEV, **kw)[1]


def gelu_tanh(x):
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


@contextlib.contextmanager
def guarded_workspace(ops, nbytes):
    """An fp32 workspace of EXACTLY nbytes inside a sentinel-filled allocation, with caller-owned arrival counters -- MDX_GEMM_WS_HEAD
    zeroed bytes, guarded the same way -- bound to it (include/mdx.h mdx_gemm_bind_counters) and released on exit.
    Yields (workspace buffer, workspace view, counters buffer, counters view as int32)."""
    from minddiffusion_amd import _lib
    lib = _lib.load()
    assert nbytes % 4 == 0
    buf, ws = G.guarded((nbytes // 4,), torch.float32, pad=WS_PAD, device=DEV)
    cbuf, cview = G.guarded((16384 // 4,), torch.float32, device=DEV)
    cview.zero_()
    _lib.check(lib.mdx_gemm_bind_counters(ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(cview.data_ptr())), "mdx_gemm_bind_counters")
    try:
        yield buf, ws, cbuf, cview
    finally:
        torch.cuda.synchronize()
        lib.mdx_gemm_release_workspace(ctypes.c_void_p(ws.data_ptr()))


# --------------------------------------------------------------------------- mdx_gemm_f16: operands, reference, launch
def conv_ref(x_nhwc, w, ks, stride, up, asym):
    """float64 conv of NHWC rows x [B, H, W, Cin] with w [N, Cin, ks, ks] -> [B, Ho, Wo, N] (torch CPU, float64)."""
    x = torch.from_numpy(x_nhwc.astype(np.float64)).permute(0, 3, 1, 2)
    if up:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    pad = 1 if ks == 3 else 0
    if asym:
        x, pad = F.pad(x, (0, 1, 0, 1)), 0
    y = F.conv2d(x, torch.from_numpy(w.astype(np.float64)), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1).numpy()


def colstats_blocks(o, rows, form):
    """o [B, Ho, Wo, N] (the stored fp16 output, float64) cut into the row blocks colstats_out describes: [blocks, rows, N]."""
    B, Ho, Wo, N = o.shape
    if form in ("halo", "conv8p"):
        ph = rows // 16
        return o.reshape(B, Ho // ph, ph, Wo // 16, 16, N).transpose(0, 1, 3, 2, 4, 5).reshape(-1, rows, N)
    return o.reshape(-1, rows, N)


def run_gemm_case(ops, c):
    name = "footprint_" + c["id"]
    rng = np.random.RandomState(seed_of(c["id"]))
    B, H, W, c1, c2, N, ks = c["B"], c["H"], c["W"], c["c1"], c["c2"], c["N"], c["ks"]
    cin = c1 + c2
    K = ks * ks * cin
    Ho, Wo = out_hw(c)
    T = Ho * Wo
    M = B * T
    wd, ld = width(c), out_ld(c)
    x = h16(rng.standard_normal((B, H, W, cin)))
    w = h16(rng.standard_normal((N, cin, ks, ks)) / math.sqrt(K))
    bias = rng.standard_normal(N).astype(np.float32)
    t = {}
    t["a"] = pin(x[..., :c1])                     # dense [B][H][W][c1]: nothing but NaN in front of sample 0 and behind the last sample
    if c2:
        t["a2"] = pin(x[..., c1:])
    wt = torch.from_numpy(w).to(DEV)
    bt = torch.from_numpy(bias).to(DEV)
    y = conv_ref(x, w, ks, c["stride"], c["up"], c["asym"]).reshape(M, N)
    if c["lnfold"]:      # x rows are the raw token rows; the launch gets gamma (.) W, S and W beta + b
        g = (1.0 + 0.3 * rng.standard_normal(cin)).astype(np.float32)
        be = (0.3 * rng.standard_normal(cin)).astype(np.float32)
        xr = x.reshape(M, cin).astype(np.float64)
        y = layer_norm(xr, g.astype(np.float64), be.astype(np.float64), 1e-5) @ w.reshape(N, cin).astype(np.float64).T
        xs = xr.reshape(M, cin // 64, 64)
        t["ln_stats"] = pin(np.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).astype(np.float32), dtype=torch.float32)
        wg, s, cb = ops.fold_layernorm(wt.reshape(N, cin), dev(g, torch.float32), dev(be, torch.float32), bt)
        wt, bt = wg.reshape(N, cin, 1, 1), cb
        t["ln_s"] = pin(s.cpu().numpy(), dtype=torch.float32)
    if c["epi"] == "geglu":
        unit = c["geglu_unit"] or 64
        wt = ops.geglu_interleave(wt[:N // 2], wt[N // 2:], unit)
        bt = ops.geglu_interleave(bt[:N // 2], bt[N // 2:], unit)
        if c["lnfold"]:
            t["ln_s"] = pin(ops.geglu_interleave(s[:N // 2], s[N // 2:], unit).cpu().numpy(), dtype=torch.float32)
    # packed weights come from the product's own packers, unpoisoned
    if c["w_frag"]:
        t["w"] = ops.pack_conv_weight_frag(wt)
    elif ks == 3:
        t["w"] = ops.pack_conv_weight(wt)
    else:
        t["w"] = ops.pack_gemm_weight(wt.reshape(N, cin))
    if c["w_sub"]:
        t["w_sub"] = ops.pack_subpixel_conv_weight(wt)
    if c["bias"]:
        t["bias"] = pin(bt.cpu().numpy(), dtype=torch.float32)
        y = y + bias.astype(np.float64)
    if c["skip"]:
        xs_ = h16(rng.standard_normal((B, H, W, c["skip"])))
        ws_ = h16(rng.standard_normal((N, c["skip"], 1, 1)) / math.sqrt(c["skip"]))
        t["skip_a"] = pin(xs_)
        t["skip_w"] = ops.pack_conv_weight(torch.from_numpy(ws_).to(DEV))
        y = y + conv_ref(xs_, ws_, 1, 1, 0, 0).reshape(M, N)
    if c["rowbias"]:
        rb = rng.standard_normal((B, N)).astype(np.float32)
        t["rowbias"] = pin(rb, (B, N), (N + 12, 1), dtype=torch.float32)
        y = (y.reshape(B, T, N) + rb.astype(np.float64)[:, None, :]).reshape(M, N)
    if c["epi"] == "gelu":
        y = gelu_tanh(y)
    elif c["epi"] == "qgelu":
        y = y / (1.0 + np.exp(-1.702 * y))
    elif c["epi"] == "geglu":
        y = y[:, :N // 2] * gelu_tanh(y[:, N // 2:])
    elif c["epi"] == "prelu":
        nsl = wd if c["mode"] == "d2s" else N
        slope = rng.uniform(0.05, 0.5, nsl).astype(np.float32)
        t["act_slope"] = pin(slope, dtype=torch.float32)
        y = np.where(y > 0, y, y * np.tile(slope.astype(np.float64), N // nsl)[None, :])
    if c["residual"]:
        res = h16(rng.standard_normal((M, wd)))
        t["residual"] = pin(res, (M, wd), (wd + 16, 1))
        y = y + res.astype(np.float64)

    # ---- guarded outputs
    guards = []                                    # (buffer, payload view(s), label)
    ctx = c["ctx"]
    if c["mode"] == "T":                           # out[(b * N + n) * out_ld + tok], written at column offset ctx of [B][N][out_ld]
        buf, full = G.guarded((B, N, ld), device=DEV)
        out_view, t["out"] = full[:, :, ctx:ctx + T], full[:, :, ctx:]
        ref_out = y.reshape(B, T, N).transpose(0, 2, 1)
    elif c["mode"] == "d2s":
        C = wd
        buf, full = G.guarded((B, 2 * Ho, 2 * Wo, C), strides=(4 * T * ld, 2 * Wo * ld, ld, 1), device=DEV)
        out_view, t["out"] = full, full
        ref_out = y.reshape(B, Ho, Wo, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * Ho, 2 * Wo, C)
    else:                                          # [B][ctx + T][ld] (ctx > 0: the q | k rows behind live text keys, out_bs)
        buf, full = G.guarded((B, ctx + T, wd), strides=((ctx + T) * ld, ld, 1), device=DEV)
        out_view, t["out"] = full[:, ctx:], full[:, ctx:]
        ref_out = y[:, :wd].reshape(B, T, wd)
    guards.append((buf, out_view, "out"))
    if c["n_split"]:
        n2 = N - c["n_split"]
        buf2, full2 = G.guarded((B, n2, ctx + T), device=DEV)
        out2_view, t["out2"] = full2[:, :, ctx:], full2[:, :, ctx:]
        guards.append((buf2, out2_view, "out2"))
    if c["stats_out"]:
        sbuf, t["stats_out"] = G.guarded((M, N // 64, 2), torch.float32, device=DEV)
        guards.append((sbuf, t["stats_out"], "stats_out"))

    with contextlib.ExitStack() as stack:
        if c["lean"] is not None:
            stack.enter_context(options(ops, gemm_lean_dense=c["lean"]))
        d = make_desc(ops, c, t)
        need = ops.gemm_workspace_bytes(d)
        counters = None
        if need:
            wbuf, ws, tbuf, counters = stack.enter_context(guarded_workspace(ops, need))
            d.workspace, d.workspace_bytes = ws.data_ptr(), need
            guards.append((wbuf, ws, "workspace"))
        q = ops.gemm_query(d)
        rows = 0
        if c["colstats"]:
            rows = q[5]
            assert rows > 0 and M % rows == 0, q
            cbuf, t["colstats_out"] = G.guarded((M // rows, N, 2), torch.float32, device=DEV)
            d.colstats_out, d.colstats_cap = t["colstats_out"].data_ptr(), M // rows      # room for exactly the row blocks produced
            guards.append((cbuf, t["colstats_out"], "colstats_out"))
            q = ops.gemm_query(d)
        exp = expected_query(c)
        assert all(q[k] == v for k, v in exp.items()), f"{name}: resolved to {q}, expected {exp}"
        if c["splitk"] > 1 or c["id"].startswith("conv8p_tail_split"):
            assert need > 0, f"{name}: a split launch that asks for no workspace"
        ops.gemm_run(d)
        for gbuf, gview, label in guards:
            # (the partials of a workspace need not cover it: tile-padded layouts leave holes)
            G.assert_footprint(gbuf, gview, f"{name}:{label}", written=label != "workspace")
        if counters is not None:      # every launch leaves its tickets zero, and takes them inside the 16 KiB it was given
            G.assert_footprint(tbuf, counters, f"{name}:counters")
            assert int(counters.view(torch.int32).abs().sum()) == 0, f"{name}: arrival counters not back at zero"
        m = check(name, out_view, ref_out, rel_l2=c["tol"], form=c["form"], query=list(q))
        if c["n_split"]:
            check(name + "_out2", out2_view, y[:, wd:].reshape(B, T, N - wd).transpose(0, 2, 1), rel_l2=c["tol"], form=c["form"])
        stored = out_view.double().cpu().numpy()
        if c["stats_out"]:
            o = stored.reshape(M, N // 64, 64)
            check(name + "_stats", t["stats_out"], np.stack([o.sum(-1), (o * o).sum(-1)], -1), rel_l2=1e-5)
        if c["colstats"]:
            blk = colstats_blocks(stored.reshape(B, Ho, Wo, N), rows, c["form"])
            check(name + "_colstats_sum", t["colstats_out"][..., 0], blk.sum(1), rel_l2=1e-5)
            check(name + "_colstats_sumsq", t["colstats_out"][..., 1], (blk * blk).sum(1), rel_l2=1e-5)
    return m


@pytest.mark.parametrize("c", DENSE_CASES, ids=lambda c: c["id"])
def test_dense_footprint(ops, c):
    run_gemm_case(ops, c)


@pytest.mark.parametrize("c", TRANSPOSED_CASES, ids=lambda c: c["id"])
def test_transposed_and_split_store_footprint(ops, c):
    run_gemm_case(ops, c)


@pytest.mark.parametrize("c", CONV_CASES, ids=lambda c: c["id"])
def test_conv_footprint(ops, c):
    run_gemm_case(ops, c)


# --------------------------------------------------------------------------- attention
def attn_ref(q, k, v, heads, causal=False):
    B, Nq, C = q.shape
    D = C // heads
    qh, kh, vh = (torch.from_numpy(a.astype(np.float64)).reshape(B, -1, heads, D).permute(0, 2, 1, 3) for a in (q, k, v))
    s = qh @ kh.transpose(2, 3) * D ** -0.5
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(Nq, Nq, dtype=torch.bool), 1), float("-inf"))
    return (torch.softmax(s, -1) @ vh).permute(0, 2, 1, 3).reshape(B, Nq, C).numpy()


def attn_operands(rng, B, heads, D, Nq, Nk):
    """q, k (numpy) and the poisoned device operands: q | k from ONE fused [B][N][2 C] buffer with a padded leading dimension when
    Nq == Nk (self-attention), two such buffers otherwise; V^T with vt_ld = Nk rounded up to 8, plus 8: zero-filled columns
    Nk .. vt_ld - 1 (include/mdx.h requires them finite), NaN beyond."""
    C = heads * D
    q = h16(0.5 * rng.standard_normal((B, Nq, C)))
    k = h16(0.5 * rng.standard_normal((B, Nk, C)))
    v = h16(rng.standard_normal((B, Nk, C)))
    ldq = 2 * C + 8
    if Nq == Nk:
        fused = pin(np.concatenate([q, k], -1), (B, Nq, 2 * C), (Nq * ldq + 64, ldq, 1))
        qd, kd = fused[:, :, :C], fused[:, :, C:]
    else:
        qd = pin(q, (B, Nq, C), (Nq * ldq + 64, ldq, 1))
        kd = pin(k, (B, Nk, C), (Nk * ldq + 64, ldq, 1))[:, :, :]
    vt_ld = (Nk + 7) // 8 * 8 + 8
    vtd = pin(v.transpose(0, 2, 1), (B, C, Nk), (C * vt_ld + 64, vt_ld, 1), zero_shape=(B, C, vt_ld))
    return q, k, v, qd, kd, vtd, vt_ld


def launch_attention(ops, qd, kd, vtd, vt_ld, B, heads, D, Nq, Nk, causal=False, ws=None, splits=0):
    C = heads * D
    o_ld = C + 8
    obuf, o = G.guarded((B, Nq, C), strides=(Nq * o_ld + 64, o_ld, 1), device=DEV)
    ops.attention(qd.data_ptr(), kd.data_ptr(), vtd.data_ptr(), o.data_ptr(), B, heads, D, Nq, Nk, D ** -0.5, qd.stride(0), qd.stride(1),
                  kd.stride(0), kd.stride(1), vtd.stride(0), vt_ld, o.stride(0), o_ld, causal=causal, ws=ws, kv_splits=splits)
    return obuf, o


ATTN_SHAPES = [(1, 1), (100, 77), (129, 200), (100, 200), (129, 1), (1, 77), (100, 100)]


@pytest.mark.parametrize("Nq,Nk", ATTN_SHAPES)
@pytest.mark.parametrize("D,heads", [(40, 2), (64, 1), (80, 2), (160, 1)])
def test_attention_footprint(ops, D, heads, Nq, Nk):
    B = 2
    rng = np.random.RandomState(seed_of("attn", D, Nq, Nk))
    q, k, v, qd, kd, vtd, vt_ld = attn_operands(rng, B, heads, D, Nq, Nk)
    name = f"footprint_attention_d{D}_h{heads}_q{Nq}_k{Nk}"
    obuf, o = launch_attention(ops, qd, kd, vtd, vt_ld, B, heads, D, Nq, Nk)
    G.assert_footprint(obuf, o, name, written=True)
    check(name, o, attn_ref(q, k, v, heads), rel_l2=2e-3, max_abs=2e-2)


@pytest.mark.parametrize("N", [1, 77, 100, 129, 200])
@pytest.mark.parametrize("D,heads", [(40, 2), (64, 2), (80, 1), (160, 1)])
def test_attention_causal_footprint(ops, D, heads, N):
    B = 2
    rng = np.random.RandomState(seed_of("causal", D, N))
    q, k, v, qd, kd, vtd, vt_ld = attn_operands(rng, B, heads, D, N, N)
    name = f"footprint_attention_causal_d{D}_h{heads}_n{N}"
    obuf, o = launch_attention(ops, qd, kd, vtd, vt_ld, B, heads, D, N, N, causal=True)
    G.assert_footprint(obuf, o, name, written=True)
    check(name, o, attn_ref(q, k, v, heads, causal=True), rel_l2=2e-3, max_abs=2e-2)


@pytest.mark.parametrize("D,heads,Nq", [(40, 2, 100), (64, 1, 129), (80, 2, 1), (64, 2, 256)])
def test_attention_pipelined_form_footprint(ops, D, heads, Nq):
    """attn_pipe_kernel: whole key tiles only (Nk % 64 == 0, at least two), D <= 80 -- Nk = 256."""
    B, Nk = 2, 256
    rng = np.random.RandomState(seed_of("pipe", D, Nq))
    q, k, v, qd, kd, vtd, vt_ld = attn_operands(rng, B, heads, D, Nq, Nk)
    name = f"footprint_attention_pipe_d{D}_h{heads}_q{Nq}_k{Nk}"
    with options(ops, attn_pipe=1):
        obuf, o = launch_attention(ops, qd, kd, vtd, vt_ld, B, heads, D, Nq, Nk)
        G.assert_footprint(obuf, o, name, written=True)
    check(name, o, attn_ref(q, k, v, heads), rel_l2=2e-3, max_abs=2e-2)


def splitkv_bytes(B, heads, D, Nq, splits):
    return 65536 + ((Nq + 127) // 128) * heads * B * splits * (128 * D * 2 + 1024)      # include/mdx.h, mdx_attention_splitkv_f16


def splitkv_workspace(nbytes):
    """(buf, fp32 view, uint8 view) of a guarded workspace of nbytes: only the 64 KiB of arrival counters at its head are zeroed
    (what "zero on the first use" protects); the partial area starts as sentinel, so that a launch given a PREFIX of it as its
    workspace shows any partial it parks behind that prefix."""
    wbuf, ws = G.guarded((nbytes // 4,), torch.float32, pad=WS_PAD, device=DEV)
    ws[:65536 // 4].zero_()
    return wbuf, ws, ws.view(torch.uint8)


# (3 splits need six key tiles of 64: Nk = 330, the nearest accepted to the 200 of the unsplit cases; 2 splits run at Nk = 200)
@pytest.mark.parametrize("pipe", [0, 1])
@pytest.mark.parametrize("D,heads,Nq,Nk,splits,Nq2,Nk2,splits2", [
    (64, 2, 129, 200, 2, 100, 330, 3), (40, 2, 100, 330, 3, 129, 200, 2), (160, 1, 129, 200, 2, 1, 330, 3), (80, 1, 1, 256, 2, 100, 384, 3)])
def test_attention_split_kv_footprint(ops, D, heads, Nq, Nk, splits, Nq2, Nk2, splits2, pipe):
    """mdx_attention_splitkv_f16, two launches of different shapes in turn on one workspace, each given EXACTLY the documented size of
    its own launch: the smaller one runs first on a prefix of the allocation (everything behind the prefix must stay sentinel), the
    larger one on all of it; the arrival counters at the head are zero after each (the second launch starts from what the first left)."""
    B = 2
    launches = sorted([(splitkv_bytes(B, heads, D, Nq, splits), Nq, Nk, splits), (splitkv_bytes(B, heads, D, Nq2, splits2), Nq2, Nk2, splits2)])
    wbuf, ws, wsb = splitkv_workspace(launches[-1][0])
    assert wsb.numel() == launches[-1][0]
    with options(ops, attn_pipe=pipe):
        for need, nq, nk, s in launches:
            rng = np.random.RandomState(seed_of("splitkv", D, nq, nk, s))
            q, k, v, qd, kd, vtd, vt_ld = attn_operands(rng, B, heads, D, nq, nk)
            name = f"footprint_attention_splitkv{s}_pipe{pipe}_d{D}_h{heads}_q{nq}_k{nk}"
            obuf, o = launch_attention(ops, qd, kd, vtd, vt_ld, B, heads, D, nq, nk, ws=wsb[:need], splits=s)
            G.assert_footprint(obuf, o, name, written=True)
            G.assert_footprint(wbuf, ws[:need // 4], name + ":workspace")
            assert int(wsb[:65536].view(torch.int32).abs().sum()) == 0, f"{name}: arrival counters not back at zero"
            check(name, o, attn_ref(q, k, v, heads), rel_l2=2e-3, max_abs=2e-2)


@pytest.mark.parametrize("D,heads,Nq,Nk", [(64, 1, 100, 3072), (80, 2, 129, 3100)])
def test_attention_auto_split_kv_on_the_librarys_own_size(ops, D, heads, Nq, Nk):
    """kv_splits = 0: the library chooses the split, and ops.attention_ws_bytes says how much workspace that needs -- the launch runs on
    exactly that many guarded bytes.  The automatic policy splits only launches with at least 48 key tiles (two splits of 24): Nk = 3072
    and a ragged 3100 are the smallest such shapes; B = 1 leaves the items far below the chip's block slots."""
    B = 1
    need = ops.attention_ws_bytes(B, heads, D, Nq, Nk)
    assert need > 65536, "the automatic policy should split this launch"
    wbuf, ws, wsb = splitkv_workspace(need)
    assert wsb.numel() == need
    rng = np.random.RandomState(seed_of("splitkv_auto", D, Nq, Nk))
    q, k, v, qd, kd, vtd, vt_ld = attn_operands(rng, B, heads, D, Nq, Nk)
    name = f"footprint_attention_splitkv_auto_d{D}_h{heads}_q{Nq}_k{Nk}"
    obuf, o = launch_attention(ops, qd, kd, vtd, vt_ld, B, heads, D, Nq, Nk, ws=wsb, splits=0)
    G.assert_footprint(obuf, o, name, written=True)
    G.assert_footprint(wbuf, ws, name + ":workspace")
    written = int((ws[65536 // 4:] != G.SENT).sum())
    assert written > 0, f"{name}: no partial reached the workspace -- the launch did not split"
    assert int(wsb[:65536].view(torch.int32).abs().sum()) == 0, f"{name}: arrival counters not back at zero"
    check(name, o, attn_ref(q, k, v, heads), rel_l2=2e-3, max_abs=2e-2)


@pytest.mark.parametrize("T,tile_m,heads,L,lnfold", [(64, 64, 2, 77, False), (128, 128, 1, 77, True), (64, 64, 1, 1, True), (128, 0, 2, 33, False)])
def test_cross_attention_epilogue_footprint(ops, T, tile_m, heads, L, lnfold):
    """mdx_gemm_desc.xattn_k: the attention as the epilogue of the lean dense kernel's query projection (one head per 64-column tile).
    Keys [B][cap][C]: rows L .. cap - 1 are NOT attended to and hold NaN; V^T columns L .. cap - 1 are zero (the arithmetic is that of
    mdx_attention_f16, whose header requires them finite)."""
    B, D = 2, 64
    C = heads * D
    cap = (L + 7) // 8 * 8 + 8
    rng = np.random.RandomState(seed_of("xattn", T, heads, L))
    x = h16(rng.standard_normal((B * T, C)))
    wq = h16(rng.standard_normal((C, C)) / math.sqrt(C))
    k = h16(0.7 * rng.standard_normal((B, L, C)))
    v = h16(rng.standard_normal((B, L, C)))
    kd = pin(k, (B, L, C), (cap * C, C, 1))
    vtd = pin(v.transpose(0, 2, 1), (B, C, L), (C * cap, cap, 1), zero_shape=(B, C, cap))
    kw = {}
    if lnfold:
        g = (1.0 + 0.1 * rng.standard_normal(C)).astype(np.float32)
        bt = (0.1 * rng.standard_normal(C)).astype(np.float32)
        qref = layer_norm(x.astype(np.float64), g.astype(np.float64), bt.astype(np.float64), 1e-5) @ wq.astype(np.float64).T
        wg, sv, cb = ops.fold_layernorm(dev(wq), dev(g, torch.float32), dev(bt, torch.float32))
        wp = ops.pack_gemm_weight(wg)
        xs = x.astype(np.float64).reshape(B * T, C // 64, 64)
        kw = dict(ln_stats=pin(np.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).astype(np.float32), dtype=torch.float32),
                  ln_s=pin(sv.cpu().numpy(), dtype=torch.float32), bias=pin(cb.cpu().numpy(), dtype=torch.float32))
    else:
        qref = x.astype(np.float64) @ wq.astype(np.float64).T
        wp = ops.pack_gemm_weight(dev(wq))
    ref = attn_ref(h16(qref).reshape(B, T, C), k, v, heads).reshape(B * T, C)      # (the kernel attends with the fp16-rounded q)
    ld = C + 8
    obuf, out = G.guarded((B * T, C), strides=(ld, 1), device=DEV)
    name = f"footprint_xattn_T{T}_tm{tile_m}_h{heads}_L{L}_ln{int(lnfold)}"
    with options(ops, gemm_lean_dense=1):
        d = ops.make_gemm_desc(pin(x), wp, C, B, T, 1, C, out, ld, tile_n=64, splitk=1, tile_m=tile_m, xattn_k=kd, xattn_vt=vtd,
                               xattn_len=L, xattn_cap=cap, xattn_scale=D ** -0.5, **kw)
        qq = ops.gemm_query(d)
        assert qq[3] == 2 and qq[1] == 64 and qq[2] == 1 and (tile_m == 0 or qq[0] == tile_m), qq
        ops.gemm_run(d)
        G.assert_footprint(obuf, out, name, written=True)
    check(name, out, ref, rel_l2=2e-3, max_abs=2e-2)


# --------------------------------------------------------------------------- fused transformer kernels
@pytest.mark.parametrize("heads", [5, 8])
@pytest.mark.parametrize("tile_rows", [32, 64])
def test_st_tail_footprint(ops, heads, tile_rows):
    """mdx_st_tail_f16 at 64 tokens per sample, 33 of 80 context rows: out, colstats_out and every debug tap guarded; context key rows
    33 .. 79 and V^T columns 33 .. 79 are zero as the cached-context GEMMs leave them (the header requires them finite), NaN beyond."""
    from test_stchain_gpu import STAGE_NAMES, chain_ref, make_case
    B, tokens, C, ctx_len, cap = 2, 64, 320, 33, 80
    assert ops.st_tail_supported(C, heads, C // heads, tokens, tile_rows)
    w, x = make_case(40 + heads, B, tokens, C, heads, ctx_len, 1024 if heads == 5 else 768, ctx_cap=cap)
    ref16 = chain_ref(w, x, B, tokens, C, heads, ctx_len, True)
    M = B * tokens
    stream, vec = ops.pack_st_tail(*(dev(w[n]) for n in ("o1", "q2", "o2", "ff1", "ff2", "po")),
                                   *(dev(w[n], torch.float32) for n in ("bo1", "g2", "be2", "bo2", "g3", "be3", "b1", "b2", "bpo")))
    ins = {n: pin(x[n]) for n in ("attn_o", "tok", "x_in")}
    kd = pin(x["k"][:, :ctx_len], (B, ctx_len, C), (cap * C, C, 1), zero_shape=(B, cap, C))
    vtd = pin(x["vt"][:, :, :ctx_len], (B, C, ctx_len), (C * cap, cap, 1), zero_shape=(B, C, cap))
    for stage in (0, 1, 4, 7):
        name = f"footprint_st_tail_h{heads}_r{tile_rows}_{STAGE_NAMES[stage]}"
        obuf, out = G.guarded((M, C), device=DEV)
        cbuf, cs = G.guarded((M // tile_rows, C, 2), torch.float32, device=DEV)
        dbuf, dbg = G.guarded((M, C), device=DEV)
        d = ops.make_st_tail_desc(ins["attn_o"], ins["tok"], ins["x_in"], out, kd, vtd, stream, vec, B, tokens, C, heads, C // heads,
                                  ctx_len, cap, tile_rows=tile_rows, colstats_out=cs, debug_out=dbg if stage else None, debug_stage=stage)
        ops.st_tail_run(d)
        if stage:      # the launch stops after the tap: out and colstats_out stay untouched
            G.assert_footprint(dbuf, dbg, name + ":debug_out", written=True)
            G.assert_footprint(obuf, torch.zeros_like(obuf, dtype=torch.bool), name + ":out")
            G.assert_footprint(cbuf, torch.zeros_like(cbuf, dtype=torch.bool), name + ":colstats_out")
            check(name, dbg, ref16[stage], rel_l2=1e-3, max_rel=6e-3)
        else:
            G.assert_footprint(obuf, out, name + ":out", written=True)
            G.assert_footprint(cbuf, cs, name + ":colstats_out", written=True)
            G.assert_footprint(dbuf, torch.zeros_like(dbuf, dtype=torch.bool), name + ":debug_out")
            check(name, out, ref16[0], rel_l2=1e-3, max_rel=6e-3)
            blk = out.double().cpu().numpy().reshape(-1, tile_rows, C)
            check(name + "_colstats_sum", cs[..., 0], blk.sum(1), rel_l2=1e-5)
            check(name + "_colstats_sumsq", cs[..., 1], (blk * blk).sum(1), rel_l2=1e-5)


@pytest.mark.parametrize("tile_rows", [32, 64])
@pytest.mark.parametrize("tokens", [64, 128])
def test_st_head_footprint(ops, tokens, tile_rows):
    """mdx_st_head_f16, B = 2: tok, qk, vt (vt_ld = tokens + 8: columns tokens .. vt_ld - 1 must survive) and the debug taps guarded."""
    from test_stchain_gpu import head_ref, make_head_case
    B, C, stat_rows = 2, 320, 32
    assert ops.st_head_supported(C, tokens, tile_rows)
    w, x = make_head_case(50 + tokens, B, tokens, C)
    ref16 = head_ref(w, x, B, tokens, C, True)
    M, nrb, vt_ld = B * tokens, tokens // stat_rows, tokens + 8
    stream, vec = ops.pack_st_head(*(dev(w[n]) for n in ("pi", "q", "k", "v")), *(dev(w[n], torch.float32) for n in ("gn_g", "gn_b", "bpi", "g1", "be1")))
    blk = x.astype(np.float64).reshape(B * nrb, stat_rows, C)
    cs = pin(np.stack([blk.sum(1), (blk * blk).sum(1)], 2).astype(np.float32), dtype=torch.float32)
    xd = pin(x)
    for stage in (0, 1, 3):
        name = f"footprint_st_head_t{tokens}_r{tile_rows}_stage{stage}"
        tbuf, tok = G.guarded((M, C), device=DEV)
        qbuf, qk = G.guarded((M, 2 * C), device=DEV)
        vbuf, vt = G.guarded((B, C, tokens), strides=(C * vt_ld, vt_ld, 1), device=DEV)
        dbuf, dbg = G.guarded((M, C), device=DEV)
        d = ops.make_st_head_desc(xd, cs, nrb, stream, vec, tok, qk, vt, vt_ld, B, tokens, C, tile_rows=tile_rows,
                                  debug_out=dbg if stage else None, debug_stage=stage)
        ops.st_head_run(d)
        if stage:
            G.assert_footprint(dbuf, dbg, name + ":debug_out", written=True)
            for b_, lab in ((tbuf, "tok"), (qbuf, "qk"), (vbuf, "vt")):
                G.assert_footprint(b_, torch.zeros_like(b_, dtype=torch.bool), f"{name}:{lab}")
            check(name, dbg, ref16[stage], rel_l2=1e-3, max_rel=6e-3)
        else:
            G.assert_footprint(tbuf, tok, name + ":tok", written=True)
            G.assert_footprint(qbuf, qk, name + ":qk", written=True)
            G.assert_footprint(vbuf, vt, name + ":vt", written=True)
            G.assert_footprint(dbuf, torch.zeros_like(dbuf, dtype=torch.bool), name + ":debug_out")
            check(name + "_tok", tok, ref16[2], rel_l2=1e-3, max_rel=6e-3)
            check(name + "_q", qk[:, :C], ref16["q"], rel_l2=1e-3, max_rel=6e-3)
            check(name + "_k", qk[:, C:], ref16["k"], rel_l2=1e-3, max_rel=6e-3)
            check(name + "_vt", vt, ref16["v"].reshape(B, tokens, C).transpose(0, 2, 1), rel_l2=1e-3, max_rel=6e-3)


# --------------------------------------------------------------------------- SRGAN 9 x 9 convs
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(17, 9), (40, 24), (33, 65)])
def test_srgan_conv_footprint(ops, B, H, W):
    """srgan_conv_in (fp32 NCHW -> PReLU -> fp16 NHWC) and srgan_conv_out (fp16 NHWC -> tanh -> fp32 NCHW) at sizes with pixels past
    the 32 x 16 and 32 x 64 tiles in both directions; inputs between NaN pads, both outputs guarded."""
    rng = np.random.RandomState(seed_of("srgan", B, H, W))
    x = h16(rng.uniform(-1, 1, (B, 3, H, W)))      # (conv_in rounds its input to fp16: fp16-exact values make the operands identical)
    w1 = h16(rng.standard_normal((64, 3, 9, 9)) / math.sqrt(243))
    b1 = (0.1 * rng.standard_normal(64)).astype(np.float32)
    sl = rng.uniform(0.05, 0.5, 64).astype(np.float32)
    y = F.conv2d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w1.astype(np.float64)), torch.from_numpy(b1.astype(np.float64)), padding=4)
    y = torch.where(y > 0, y, y * torch.from_numpy(sl.astype(np.float64))[None, :, None, None]).permute(0, 2, 3, 1).numpy()
    name = f"footprint_srgan_conv_in_B{B}_{H}x{W}"
    obuf, out = G.guarded((B, H, W, 64), device=DEV)
    ops.srgan_conv_in(pin(x, dtype=torch.float32), dev(w1), pin(b1, dtype=torch.float32), pin(sl, dtype=torch.float32), out=out)
    G.assert_footprint(obuf, out, name, written=True)
    check(name, out, y, rel_l2=1e-3)

    f = h16(rng.standard_normal((B, H, W, 64)))
    w3 = h16(rng.standard_normal((3, 64, 9, 9)) / math.sqrt(64 * 81))
    b3 = (0.1 * rng.standard_normal(3)).astype(np.float32)
    z = torch.tanh(F.conv2d(torch.from_numpy(f.astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(w3.astype(np.float64)),
                            torch.from_numpy(b3.astype(np.float64)), padding=4)).numpy()
    name = f"footprint_srgan_conv_out_B{B}_{H}x{W}"
    obuf, out = G.guarded((B, 3, H, W), torch.float32, device=DEV)
    ops.srgan_conv_out(pin(f), dev(w3), pin(b3, dtype=torch.float32), B, H, W, out=out)
    G.assert_footprint(obuf, out, name, written=True)
    check(name, out, z, rel_l2=1e-3)
