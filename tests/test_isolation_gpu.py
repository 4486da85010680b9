"""Sample isolation on the GPU (tests/_isolation.py): at batch 3, every output of sample r -- r = 0, 1 (neighbours on both sides)
and 2 (the end of the batch) -- is torch.equal across four launches that differ only in the OTHER samples' per-sample inputs:
as given, re-drawn at another scale and offset, all NaN, all +Inf.  No tolerance anywhere; value parity against float64 stays with
the kernel tests.  Weights, biases, gamma / beta and the LayerNorm-fold S[n] are shared and stay finite.

The launch forms are the ones production batches resolve to and the tiny session test (tests/test_session_gpu.py) never reaches:
M tiles that straddle samples, ticket and slab split-K, HALO patches, the eight-wave conv core with its tail split, column
statistics per sample, every attention form, the fused cross-attention epilogue, the SpatialTransformer chain kernels, the table
and slot sampler steps.  Every case asserts the form it claims to run (mdx_gemm_query, mdx_groupnorm_query, the forcing options).

Not asserted, on purpose: equality across row positions (conv8p's tail round and the split policies add a sample's products in
another order at another position), equality across batch sizes, and the guidance-duplicate prefix (its precondition is equal
halves: both halves of a pair are perturbed together here).
"""
import contextlib
import math

import numpy as np
import pytest
import torch

import _isolation as I
from _util import h16
from test_norm_regimes_gpu import GN_CASES      # GroupNorm forms 0-4, the two-source concat, FiLM, the colstats geometries

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3
ROWS = (0, 1, 2)


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.float16)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.float32)


def zeros16(*shape):
    return torch.zeros(shape, dtype=torch.float16, device=DEV)


def zeros32(*shape):
    return torch.zeros(shape, dtype=torch.float32, device=DEV)


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
    return sum(map(ord, "/".join(map(str, parts)))) % (2 ** 31)


def per_b(outs, b):
    """own() of a run that returns tensors with the sample index on axis 0."""
    return [t[b] for t in outs]


def launch(ops, d, expect):
    """Workspace, the launch form the case claims (indices into mdx_gemm_query's answer), launch, wait."""
    ws = ops.new_gemm_workspace(max(ops.gemm_workspace_bytes(d), 16), DEV)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    q = ops.gemm_query(d)
    assert all(q[i] == v for i, v in expect.items()), f"resolved to {q}, the case wants {expect}"
    ops.gemm_run(d)
    torch.cuda.synchronize()            # the workspace, and its counters' binding, end with this call
    return q


# --------------------------------------------------------------------------- dense GEMM
# T = 80 tokens per sample, M = 240: 64- and 128-row tiles straddle samples (64 | 16 + 48 | 32 + 32 | 48 + 16 ...), the last tile
# is ragged.  K = N = 320; K = 1280 where a split needs depth (20 K tiles: 3 splits reduce in the kernel by ticket, a request for
# 8 resolves to 7 non-empty splits of 3 K tiles through the slab reduce kernel).
# form: (gemm_lean_dense, tile_m, tile_n, splitk asked, K, splits resolved, in-kernel reduce)
DENSE_FORMS = {f"{'lean' if lean else 'gen'}_{tm}x{tn}": (lean, tm, tn, 1, 320, 1, 0)
               for lean in (0, 1) for tm, tn in ((64, 64), (64, 128), (128, 64), (128, 128))}
_TILES = list(DENSE_FORMS)
DENSE_FORMS.update(lean_128x160=(1, 128, 160, 1, 320, 1, 0), gen_ticket3=(0, 128, 128, 3, 1280, 3, 1),
                   lean_ticket3=(1, 128, 128, 3, 1280, 3, 1), gen_slab8=(0, 64, 64, 8, 1280, 7, 0))
_GEN = [f for f in DENSE_FORMS if f.startswith("gen")]
_WIDE = [f for f in DENSE_FORMS if DENSE_FORMS[f][2] >= 128 and f != "lean_128x160"]      # GEGLU pairs columns inside a 128-wide tile
# epilogue -> the forms that carry it (dense.hip mdx_dense_takes_desc: the lean kernel has no rowbias / out_bs / transposed store;
# the 128 x 160 tile has bias / residual / GEGLU packed at 80 / the LayerNorm-fold consumer only)
DENSE_FEATS = {
    "res_stats": _TILES + ["gen_ticket3", "lean_ticket3", "gen_slab8"],
    "res": ["lean_128x160"],
    "rowbias": _GEN,
    "colstats": _TILES + ["gen_ticket3", "lean_ticket3", "gen_slab8"],
    "geglu": _WIDE + ["lean_128x160"],
    "lnfold": list(DENSE_FORMS),
    "lnfold_geglu": _WIDE + ["lean_128x160"],
    "lnfold_nsplit": _TILES + ["gen_ticket3", "lean_ticket3", "gen_slab8"],
    "nsplit": _TILES + ["gen_ticket3", "lean_ticket3", "gen_slab8"],
    "transposed": _GEN,
    "out_bs": _GEN,
    "twosrc": _TILES + ["gen_ticket3", "lean_ticket3"],
}
DENSE_CASES = [(feat, form) for feat, forms in DENSE_FEATS.items() for form in forms]


def dense_case(ops, feat, form):
    """(inputs, per_sample, run) of one dense launch: 3 samples of T tokens."""
    lean, tm, tn, sk, K, ns, ticket = DENSE_FORMS[form]
    T = 128 if feat == "colstats" else 80        # a column-statistics row block never straddles samples: T % tile_m == 0
    M = B * T
    N = 640 if feat.endswith("geglu") else 960 if feat.endswith("nsplit") else 320
    rng = np.random.RandomState(seed_of("dense", feat, form))
    a = h16(rng.standard_normal((M, K)))
    wd = dev16(h16(rng.standard_normal((N, K)) / math.sqrt(K)))
    bias = dev32(rng.standard_normal(N))
    takes_lean = lean and feat not in ("rowbias", "transposed", "out_bs") and (ns == 1 or ticket)
    if feat == "transposed" and ns > 1:
        ticket = 0                                  # a transposed store reduces through the slabs
    expect = {0: tm, 1: tn, 2: ns, 3: 2 if takes_lean else 0, 6: ticket}
    kw = dict(splitk=sk, tile_m=tm, tile_n=tn, bias=bias)
    inputs, per = {"a": dev16(a)}, {"a": {"rows": T}}
    if feat in ("res_stats", "res", "twosrc"):
        inputs["res"], per["res"] = dev16(h16(rng.standard_normal((M, N)))), {"rows": T}
    if feat == "twosrc":                            # K-segmented A: [a | a2], whole 64-channel K tiles per source
        c1 = K * 3 // 5
        inputs["a"], inputs["a2"], per["a2"] = dev16(a[:, :c1]), dev16(a[:, c1:]), {"rows": T}
    if feat == "rowbias":                           # a different time-embedding row per sample, a column slice of a wider tensor
        inputs["emb"], per["emb"] = dev32(rng.standard_normal((B, 400))), {"axis": 0}
    if feat.startswith("lnfold"):                   # the consumer: raw rows + the producer's per-64-column {sum, sumsq}
        g, be = dev32(1 + 0.3 * rng.standard_normal(K)), dev32(0.3 * rng.standard_normal(K))
        xs = a.astype(np.float64).reshape(M, K // 64, 64)
        inputs["st"], per["st"] = dev32(np.stack([xs.sum(-1), (xs * xs).sum(-1)], -1)), {"rows": T}
        wd, s, bias = ops.fold_layernorm(wd, g, be, bias)       # gamma-scaled weights, S[n], W beta + b
        kw.update(bias=bias, ln_s=s)
    if feat.endswith("geglu"):                      # weights, bias and S[n] packed value | gate per tile
        unit = 80 if tn == 160 else 64
        il = lambda t: ops.geglu_interleave(t[:N // 2], t[N // 2:], unit)
        wd = il(wd)
        kw.update(bias=il(kw["bias"]), epilogue=ops.EPI_GEGLU, geglu_unit=80 if tn == 160 else 0)
        if "ln_s" in kw:
            kw["ln_s"] = il(kw["ln_s"])
    wp = ops.pack_gemm_weight(wd)

    def run(inp):
        k = dict(kw)
        if feat.endswith("nsplit"):                 # q | k row-major and V^T from one launch
            C = N // 3
            out, vt = zeros16(B, T, 2 * C), zeros16(B, C, T)
            outs, k = [out, vt], dict(k, out2=vt, out2_ld=T, n_split=2 * C)
            ld = 2 * C
        elif feat == "transposed":
            out = zeros16(B, N, T)
            outs, ld, k = [out], T, dict(k, out_mode=ops.OUT_TRANSPOSED)
        elif feat == "out_bs":                      # a token sub-range of a larger [B][100][N] buffer
            big = zeros16(B, 100, N)
            out, outs, ld, k = big[:, 12:], [big], N, dict(k, out_bs=100 * N)
        else:
            out = zeros16(B, T, N // 2 if feat.endswith("geglu") else N)
            outs, ld = [out], out.shape[-1]
        if "res" in inp:
            k.update(residual=inp["res"], residual_ld=N)
        if feat in ("res_stats", "twosrc"):
            st = zeros32(B, T, N // 64, 2)
            outs, k = outs + [st], dict(k, stats_out=st)
        if feat == "twosrc":
            k.update(a2=inp["a2"], c2=inp["a2"].shape[1])
        if feat == "rowbias":
            k.update(rowbias=inp["emb"][:, 40:40 + N], rowbias_ld=400)
        if "st" in inp:
            k.update(ln_stats=inp["st"])
        cs = None
        if feat == "colstats":
            cs = zeros32(B * T // 64, N, 2)
            k.update(colstats_out=cs)
        d = ops.make_gemm_desc(inp["a"], wp, N, B, T, 1, inp["a"].shape[1], out, ld, **k)
        q = launch(ops, d, expect)
        if cs is not None:                          # row blocks as the query reports them
            assert q[5] > 0 and T % q[5] == 0, q
            nrb = T // q[5]
            outs = outs + [cs[:B * nrb].view(B, nrb, N, 2)]
            assert not bool(cs[B * nrb:].any())
        return outs

    return inputs, per, lambda inp: _with(ops, run, inp, gemm_lean_dense=lean)


def _with(ops, run, inp, **opts):
    with options(ops, **opts):
        return run(inp)


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("feat,form", DENSE_CASES, ids=[f"{a}-{b}" for a, b in DENSE_CASES])
def test_dense_gemm(ops, feat, form, r):
    inputs, per, run = dense_case(ops, feat, form)
    I.assert_isolated(f"iso_dense_{feat}_{form}", run, inputs, per, r, per_b, seed=seed_of(feat, form, r))


# --------------------------------------------------------------------------- convolutions
def pack_conv(ops, w):
    return ops.pack_conv_weight(torch.from_numpy(np.ascontiguousarray(w)).to(DEV))


# id: (B, H, W, Cin, Cout, descriptor fields, features, what mdx_gemm_query must report {index: value})
#   features: e = bias + time-embedding row + residual, c = column statistics, s2 = fused skip 1x1 over two sources (128 + 64),
#   s1 = over one source (64), f = fragment-major (streamed) weights, u = the sub-pixel weights, g = fused input GroupNorm
#   (statistics in 64-row blocks), w0 = no split-K workspace
CONV_CASES = {
    "generic_6x10": (3, 6, 10, 64, 72, dict(), "e", {3: 0}),                                   # ragged extent, N tail
    "generic_stride2_8x8": (3, 8, 8, 128, 128, dict(stride=2), "e", {3: 0}),
    "generic_nearest2x_8x8": (3, 8, 8, 128, 128, dict(upsample=1), "e", {3: 0}),
    # two samples per 128-row tile: r = 0 / 1 share a tile, the last tile is half empty (no column statistics in this form: 5: 0)
    "halo8": (3, 8, 8, 128, 192, dict(splitk=1), "e", {0: 128, 2: 1, 3: 1, 5: 0}),
    "halo8_split2": (3, 8, 8, 128, 192, dict(splitk=2), "e", {0: 128, 2: 2, 3: 1, 5: 0}),
    "halo8_stream": (2, 8, 8, 128, 192, dict(splitk=1, tile_m=128, tile_n=64, w_frag=1), "ef", {0: 128, 1: 64, 2: 1, 3: 1}),
    "halo8_stream_split2": (2, 8, 8, 128, 192, dict(splitk=2, tile_m=128, tile_n=64, w_frag=1), "ef", {0: 128, 1: 64, 2: 2, 3: 1}),
    "halo16": (3, 16, 16, 128, 192, dict(splitk=1), "ec", {0: 128, 2: 1, 3: 1, 5: 128}),
    "halo16_split2": (3, 16, 16, 128, 192, dict(splitk=2), "ec", {0: 128, 2: 2, 3: 1}),
    "halo16_skip": (3, 16, 16, 128, 192, dict(splitk=1), "ecs2", {0: 128, 2: 1, 3: 1, 5: 128}),
    "halo16_skip_split2": (3, 16, 16, 128, 192, dict(splitk=2), "ecs2", {0: 128, 2: 2, 3: 1}),
    # the eight-wave core, one 16 x 16 patch per sample.  Without a workspace no tile splits: 64-column tiles make 9 tiles, 8 in
    # the whole-tile order + 1 odd; with one, every tile of the partly filled round splits along the 64-channel chunks
    "conv8p_whole": (3, 16, 16, 128, 160, dict(tile_m=256, stages=8, tile_n=64), "ecw0", {0: 256, 1: 64, 2: 1, 3: 1, 5: 256}),
    "conv8p_tail_split": (3, 16, 16, 128, 160, dict(tile_m=256, stages=8, tile_n=160), "ecs1", {0: 256, 1: 160, 3: 1, 5: 256}),
    "conv8p_subpixel": (3, 16, 16, 64, 64, dict(tile_m=256, stages=8, upsample=1), "u", {0: 256, 3: 1}),
    "halo16_fused_gn": (3, 16, 16, 128, 128, dict(splitk=1, tile_n=64), "g", {1: 64, 3: 1}),
}


def conv_case(ops, cid):
    Bc, H, W, Cin, Cout, fields, feats, expect = CONV_CASES[cid]
    rng = np.random.RandomState(seed_of("conv", cid))
    HW = H * W
    up, stride = fields.get("upsample", 0), fields.get("stride", 1)
    HoWo = HW * (4 if up else 1) // (stride * stride)
    wt = h16(rng.standard_normal((Cout, Cin, 3, 3)) / math.sqrt(9 * Cin))
    wp = ops.pack_conv_weight_frag(torch.from_numpy(wt).to(DEV)) if "f" in feats else pack_conv(ops, wt)
    kw = dict(fields, ksize=3, bias=dev32(rng.standard_normal(Cout)))
    x = h16(rng.standard_normal((Bc, HW, Cin)) * 1.5 + 0.3)
    inputs, per = {"x": dev16(x)}, {"x": {"axis": 0}}
    if "e" in feats:
        inputs.update(emb=dev32(rng.standard_normal((Bc, Cout + 24))), res=dev16(h16(rng.standard_normal((Bc, HoWo, Cout)))))
        per.update(emb={"axis": 0}, res={"axis": 0})
    if "u" in feats:
        kw["w_sub"] = ops.pack_subpixel_conv_weight(torch.from_numpy(wt).to(DEV))
    nskip = 2 if "s2" in feats else 1 if "s1" in feats else 0
    if nskip:
        cs_ = (128, 64) if nskip == 2 else (64,)
        kw.update(skip_w=pack_conv(ops, h16(rng.standard_normal((Cout, sum(cs_), 1, 1)) / math.sqrt(sum(cs_)))), skip_c1=cs_[0],
                  skip_c2=cs_[1] if nskip == 2 else 0)
        for i, c in enumerate(cs_):
            inputs[f"skip{i}"], per[f"skip{i}"] = dev16(h16(rng.standard_normal((Bc, HW, c)))), {"axis": 0}
    if "g" in feats:
        blk = x.astype(np.float64).reshape(Bc * HW // 64, 64, Cin)
        inputs["gn_cs"], per["gn_cs"] = dev32(np.stack([blk.sum(1), (blk * blk).sum(1)], 2)), {"rows": HW // 64}
        kw.update(gn_nrb=HW // 64, gn_gamma=dev32(1 + 0.2 * rng.standard_normal(Cin)), gn_beta=dev32(0.1 * rng.standard_normal(Cin)),
                  gn_eps=1e-5, gn_silu=1)

    def run(inp):
        k = dict(kw)
        out = zeros16(Bc, HoWo, Cout)
        outs = [out]
        if "e" in feats:
            k.update(rowbias=inp["emb"][:, 16:16 + Cout], rowbias_ld=Cout + 24, residual=inp["res"], residual_ld=Cout)
        if nskip:
            k.update(skip_a=inp["skip0"], skip_a2=inp.get("skip1"))
        if "g" in feats:
            k.update(gn_colstats=inp["gn_cs"])
        cs = None
        if "c" in feats:
            cs = zeros32(Bc * HoWo // 128, Cout, 2)
            k.update(colstats_out=cs)
        d = ops.make_gemm_desc(inp["x"], wp, Cout, Bc, H, W, Cin, out, Cout, **k)
        if "w0" in feats:
            q = ops.gemm_query(d)
            assert all(q[i] == v for i, v in expect.items()), (q, expect)
            ops.gemm_run(d)
        else:
            if cid == "conv8p_tail_split":
                assert ops.gemm_workspace_bytes(d) > 0      # the plan splits the tail round: partials go through the workspace
            q = launch(ops, d, expect)
        if cs is not None:
            assert q[5] > 0 and HoWo % q[5] == 0, q
            nrb = HoWo // q[5]
            outs.append(cs[:Bc * nrb].view(Bc, nrb, Cout, 2))
        return outs

    return Bc, inputs, per, run


CONV_ROWS = [(cid, r) for cid in CONV_CASES for r in range(CONV_CASES[cid][0])]


@pytest.mark.parametrize("cid,r", CONV_ROWS, ids=[f"{c}-{r}" for c, r in CONV_ROWS])
def test_convolutions(ops, cid, r):
    _, inputs, per, run = conv_case(ops, cid)
    I.assert_isolated(f"iso_conv_{cid}", run, inputs, per, r, per_b, seed=seed_of(cid, r))


@pytest.mark.parametrize("r", ROWS)
def test_dense_with_fused_input_groupnorm(ops, r):
    """mdx_gemm_desc.gn_colstats on a dense launch, the batch-3 row of the kernel test: 576 tokens, 10 channels per group, 64 x 64
    tiles, the normalisation applied to the A fragments from per-sample statistics."""
    HW, Cin, N, rows = 576, 320, 320, 64
    rng = np.random.RandomState(seed_of("dense_gn"))
    x = h16(rng.standard_normal((B, HW, Cin)) * (0.5 + rng.rand(Cin)) + rng.standard_normal(Cin))
    blk = x.astype(np.float64).reshape(B * HW // rows, rows, Cin)
    inputs = {"x": dev16(x), "cs": dev32(np.stack([blk.sum(1), (blk * blk).sum(1)], 2))}
    per = {"x": {"axis": 0}, "cs": {"rows": HW // rows}}
    wp = ops.pack_gemm_weight(dev16(h16(rng.standard_normal((N, Cin)) / math.sqrt(Cin))))
    bias, g, bt = dev32(rng.standard_normal(N)), dev32(1 + 0.2 * rng.standard_normal(Cin)), dev32(0.1 * rng.standard_normal(Cin))

    def run(inp):
        out = zeros16(B, HW, N)
        d = ops.make_gemm_desc(inp["x"], wp, N, B, HW, 1, Cin, out, N, bias=bias, tile_m=64, tile_n=64, gn_colstats=inp["cs"],
                               gn_nrb=HW // rows, gn_gamma=g, gn_beta=bt, gn_eps=1e-6, gn_silu=0)
        launch(ops, d, {0: 64, 1: 64, 3: 0})
        return [out]
    I.assert_isolated("iso_dense_fused_gn", run, inputs, per, r, per_b, seed=r)


# --------------------------------------------------------------------------- norms
# The cases run at batch 3 where that keeps their launch form; the three whose form is a function of the batch keep their own
# (fused_256: 16 samples of 4 pixels; colstats_boost: >= 1 MiB at batch 4) or restate the fields the batch moves.
GN_KEEP_B = {"fused_256": 16, "colstats_boost": 4}
GN_FIELDS_B3 = {"colstats_boost_below": dict(cw=5, nblk=22, pix=12)}      # 0.94 MiB: still below the boost


def sample_stats(rng, shape):
    """fp16-exact values, every sample with its own mean and std."""
    Bn = shape[0]
    std = (0.5 + 0.75 * np.arange(Bn)).reshape(Bn, *([1] * (len(shape) - 1)))
    mean = (0.9 * np.arange(Bn) - 0.6).reshape(std.shape)
    return h16(rng.standard_normal(shape) * std + mean)


def col_partials(x, nrb):
    """[B * nrb, C, 2] float64 {sum, sumsq} of x [B, HW, C] over nrb row blocks per sample, as a producer emits them."""
    Bn, HW, C = x.shape
    out = np.zeros((Bn, nrb, C, 2))
    for j, rows in enumerate(np.array_split(np.arange(HW), nrb)):
        out[:, j, :, 0] = x[:, rows].astype(np.float64).sum(1)
        out[:, j, :, 1] = (x[:, rows].astype(np.float64) ** 2).sum(1)
    return dev32(out.reshape(Bn * nrb, C, 2))


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: c[0])
def test_groupnorm_forms(ops, case, r):
    cid, _, H, W, C1, C2, opts, kind, form, fields = case
    Bn = GN_KEEP_B.get(cid, B)
    fields = fields if cid in GN_KEEP_B or case[1] == B else GN_FIELDS_B3.get(cid, fields)
    C, HW = C1 + C2, H * W
    rng = np.random.RandomState(seed_of("gn", cid))
    x = sample_stats(rng, (Bn, HW, C))
    g, b = dev32(rng.uniform(-3, 3, C)), dev32(rng.uniform(-3, 3, C))
    inputs, per = {"x1": dev16(x[:, :, :C1])}, {"x1": {"axis": 0}}
    nrb1 = nrb2 = 0
    if C2:
        inputs["x2"], per["x2"] = dev16(x[:, :, C1:]), {"axis": 0}
    if kind == "film":          # rows [scale | shift] of one tensor
        inputs["mod"], per["mod"] = dev32(rng.uniform(-1, 1, (Bn, 2 * C))), {"axis": 0}
    elif kind != "plain":
        _, nrb1, nrb2 = kind
        inputs["cs1"], per["cs1"] = col_partials(x[:, :, :C1], nrb1), {"rows": nrb1}
        if C2:
            inputs["cs2"], per["cs2"] = col_partials(x[:, :, C1:], nrb2), {"rows": nrb2}

    def run(inp):
        out = zeros16(Bn, HW, C)
        for act in (False, True):
            if kind == "plain":
                ops.groupnorm(inp["x1"], inp.get("x2"), g, b, 1e-5, act, out=out)
            elif kind == "film":
                ops.groupnorm_scaleshift(inp["x1"], inp.get("x2"), g, b, inp["mod"][:, :C], inp["mod"][:, C:], 2 * C, 1e-5, act, out=out)
            else:
                ops.groupnorm_colstats(inp["x1"], inp["cs1"], nrb1, inp.get("x2"), inp.get("cs2"), nrb2, g, b, 1e-5, act, out=out)
            yield out.clone()

    with options(ops, **opts):
        q = ops.groupnorm_query(C1, C2, Bn, HW, 32, colstats_nrb=nrb1)
        assert q["form"] == form and all(q[k] == v for k, v in fields.items()), f"{cid} at batch {Bn}: resolved to {q}"
        I.assert_isolated(f"iso_gn_{cid}", lambda inp: list(run(inp)), inputs, per, r, per_b, seed=seed_of(cid, r))


@pytest.mark.parametrize("r", ROWS)
def test_groupnorm_from_splitk_slabs(ops, r):
    """The slab form of gn_fused_kernel at 8 x 8, split 2: a 1 x 1 identity conv leaves its partial sums in the workspace and
    the GroupNorm launch folds them per sample."""
    H = W = 8
    C, HW = 320, 64
    rng = np.random.RandomState(seed_of("gn_slabs"))
    inputs = {"a": dev16(sample_stats(rng, (B, HW, C)))}
    wp = ops.pack_conv_weight(torch.eye(C, dtype=torch.float32, device=DEV).reshape(C, C, 1, 1))
    g, b = dev32(rng.uniform(-3, 3, C)), dev32(rng.uniform(-3, 3, C))

    def run(inp):
        conv_out, out = zeros16(B, HW, C), zeros16(B, HW, C)
        d = ops.make_gemm_desc(inp["a"], wp, C, B, H, W, C, conv_out, C, ksize=1, splitk=2)
        ws = ops.new_gemm_workspace(ops.gemm_workspace_bytes(d), DEV)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        d.defer_reduce = 1
        assert ops.gemm_query(d)[2] == 2 and ops.groupnorm_from_splitk_ok(d, 32), ops.gemm_query(d)
        ops.gemm_run(d)
        ops.groupnorm_from_splitk(d, g, b, 1e-5, True, out, 32)
        torch.cuda.synchronize()
        return [conv_out, out]
    I.assert_isolated("iso_gn_from_splitk_8x8_s2", run, inputs, {"a": {"axis": 0}}, r, per_b, seed=r)


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("C", [72, 1032])
def test_layernorm(ops, C, r):
    T = 5
    rng = np.random.RandomState(seed_of("ln", C))
    inputs = {"x": dev16(sample_stats(rng, (B, T, C)).reshape(B * T, C))}
    g, b = dev32(rng.uniform(-3, 3, C)), dev32(rng.uniform(-3, 3, C))
    run = lambda inp: [ops.layernorm(inp["x"], g, b, 1e-5).view(B, T, C)]
    I.assert_isolated(f"iso_ln_C{C}", run, inputs, {"x": {"rows": T}}, r, per_b, seed=seed_of(C, r))


# --------------------------------------------------------------------------- attention
HEADS = 2
HEAD_DIMS = (40, 64, 80, 160)
# form: (Nq, Nk, library options, kv splits, causal).  attn_pipe = 0 is attn_kernel (attn_occ3 picks its 3- or 2-blocks-per-CU build at
# D <= 64); attn_pipe = 1 takes a launch of full key tiles at D <= 80, attn8 = 2 forces the eight-wave form on 256-query blocks
# (neither has a D = 160 instantiation).  Nk = 200 ends inside a key tile: with K stored [B, Nk, C] the rows directly behind
# sample r's masked tail are sample r + 1's.
_A0 = dict(attn_pipe=0, attn8=0, attn_occ3=1)
ATTN_FORMS = {"attn_kernel": (100, 200, _A0, 0, False), "attn_kernel_occ2": (100, 200, dict(_A0, attn_occ3=0), 0, False),
              "pipelined": (100, 192, dict(_A0, attn_pipe=1), 0, False), "eight_wave": (256, 128, dict(_A0, attn8=2), 0, False),
              "split_kv": (100, 512, _A0, 2, False), "split_kv_pipelined": (100, 512, dict(_A0, attn_pipe=1), 2, False),
              "causal": (77, 77, _A0, 0, True)}
ATTN_CASES = [(f, D) for f in ATTN_FORMS for D in HEAD_DIMS
              if not (D == 160 and (ATTN_FORMS[f][2]["attn_pipe"] or ATTN_FORMS[f][2]["attn8"]))
              and not (D > 64 and not ATTN_FORMS[f][2]["attn_occ3"])]
_ATTN_WS = {}


def attn_inputs(rng, Nq, Nk, C):
    ld = (Nk + 7) // 8 * 8
    vt = np.zeros((B, C, ld), np.float32)
    vt[:, :, :Nk] = h16(rng.standard_normal((B, C, Nk)))
    inputs = {"q": dev16(h16(rng.standard_normal((B, Nq, C)))), "k": dev16(h16(rng.standard_normal((B, Nk, C)))), "vt": dev16(vt)}
    return inputs, {k: {"axis": 0} for k in inputs}, ld


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("form,D", ATTN_CASES, ids=[f"{f}-d{D}" for f, D in ATTN_CASES])
def test_attention(ops, form, D, r):
    Nq, Nk, opts, splits, causal = ATTN_FORMS[form]
    C = HEADS * D
    inputs, per, ld = attn_inputs(np.random.RandomState(seed_of("attn", form, D)), Nq, Nk, C)
    ws = None
    if splits:                  # ONE workspace for all launches of the form, never cleared: every launch leaves its counters at zero
        assert ops.attention_ws_bytes(B, HEADS, D, Nq, Nk) == 0      # the library would not split this shape: the count is forced
        key = (form, D)
        if key not in _ATTN_WS:
            items = (Nq + 127) // 128 * HEADS * B
            _ATTN_WS[key] = ops.attention_workspace(65536 + items * splits * (128 * D * 2 + 1024), DEV)
        ws = _ATTN_WS[key]

    def run(inp):
        out = zeros16(B, Nq, C)
        ops.attention(inp["q"].data_ptr(), inp["k"].data_ptr(), inp["vt"].data_ptr(), out.data_ptr(), B, HEADS, D, Nq, Nk, D ** -0.5,
                      Nq * C, C, Nk * C, C, C * ld, ld, Nq * C, C, causal=causal, ws=ws, kv_splits=splits)
        return [out]
    with options(ops, **opts):
        I.assert_isolated(f"iso_attn_{form}_d{D}", run, inputs, per, r, per_b, seed=seed_of(form, D, r))
    if ws is not None:
        torch.cuda.synchronize()
        assert int(ws[:65536].view(torch.int32).abs().sum()) == 0, "arrival counters not back at zero"


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_attention_fused_qk_layout(ops, D, r):
    """q and k as column slices of one [B, N, 2 C] projection buffer, V^T beside it: how the UNet calls it."""
    N, C = 100, HEADS * D
    rng = np.random.RandomState(seed_of("attn_qk", D))
    ld = (N + 7) // 8 * 8
    vt = np.zeros((B, C, ld), np.float32)
    vt[:, :, :N] = h16(rng.standard_normal((B, C, N)))
    inputs = {"qk": dev16(h16(rng.standard_normal((B, N, 2 * C)))), "vt": dev16(vt)}

    def run(inp):
        out = zeros16(B, N, C)
        p = inp["qk"].data_ptr()
        ops.attention(p, p + 2 * C, inp["vt"].data_ptr(), out.data_ptr(), B, HEADS, D, N, N, D ** -0.5, N * 2 * C, 2 * C, N * 2 * C, 2 * C,
                      C * ld, ld, N * C, C)
        return [out]
    with options(ops, attn_pipe=0, attn8=0):
        I.assert_isolated(f"iso_attn_fused_qk_d{D}", run, inputs, {"qk": {"axis": 0}, "vt": {"axis": 0}}, r, per_b, seed=seed_of(D, r))


# --------------------------------------------------------------------------- cross-attention as the epilogue of the query projection
# (tokens per sample, tile_m, keys, key capacity): tile_m needs tokens % tile_m == 0, so the 128-row tile runs at 128 tokens;
# 200 keys take the pair-by-pair staging of contexts beyond 128 keys
XATTN_CASES = [(64, 64, 77, 80), (128, 128, 77, 80), (64, 64, 200, 200), (128, 128, 200, 200)]


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("lnfold", [False, True], ids=["plain", "lnfold"])
@pytest.mark.parametrize("T,tile_m,L,cap", XATTN_CASES)
def test_cross_attention_epilogue(ops, T, tile_m, L, cap, lnfold, r):
    C = 128
    rng = np.random.RandomState(seed_of("xattn", T, L, lnfold))
    x = h16(rng.standard_normal((B * T, C)))
    k = np.zeros((B, cap, C), np.float32)
    vt = np.zeros((B, C, cap), np.float32)
    k[:, :L] = h16(0.7 * rng.standard_normal((B, L, C)))
    vt[:, :, :L] = h16(rng.standard_normal((B, C, L)))
    inputs = {"x": dev16(x), "k": dev16(k), "vt": dev16(vt)}
    per = {"x": {"rows": T}, "k": {"axis": 0}, "vt": {"axis": 0}}
    wq = dev16(h16(rng.standard_normal((C, C)) / math.sqrt(C)))
    kw = {}
    if lnfold:
        xs = x.astype(np.float64).reshape(B * T, C // 64, 64)
        inputs["st"], per["st"] = dev32(np.stack([xs.sum(-1), (xs * xs).sum(-1)], -1)), {"rows": T}
        wg, s, cb = ops.fold_layernorm(wq, dev32(1 + 0.1 * rng.standard_normal(C)), dev32(0.1 * rng.standard_normal(C)))
        wp, kw = ops.pack_gemm_weight(wg), dict(ln_s=s, bias=cb)
    else:
        wp = ops.pack_gemm_weight(wq)

    def run(inp):
        out = zeros16(B, T, C)
        k_ = dict(kw, ln_stats=inp["st"]) if lnfold else kw
        d = ops.make_gemm_desc(inp["x"], wp, C, B, T, 1, C, out, C, tile_n=64, splitk=1, tile_m=tile_m, xattn_k=inp["k"],
                               xattn_vt=inp["vt"], xattn_len=L, xattn_cap=cap, xattn_scale=64 ** -0.5, **k_)
        launch(ops, d, {0: tile_m, 1: 64, 2: 1, 3: 2})
        return [out]
    I.assert_isolated(f"iso_xattn_T{T}_L{L}_ln{int(lnfold)}", run, inputs, per, r, per_b, seed=seed_of(T, L, lnfold, r))


# --------------------------------------------------------------------------- the SpatialTransformer chain kernels
@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("tile_rows", [32, 64])
def test_st_head(ops, tile_rows, r):
    """GroupNorm (per-sample statistics from column partials) -> proj_in -> LayerNorm -> q | k | V^T: tok, q | k and V^T of r."""
    from test_stchain_gpu import make_head_case
    tokens, C, stat_rows = 64, 320, 32
    assert ops.st_head_supported(C, tokens, tile_rows)
    w, x = make_head_case(5, B, tokens, C)
    stream, vec = ops.pack_st_head(*(dev16(w[n]) for n in ("pi", "q", "k", "v")), *(dev32(w[n]) for n in ("gn_g", "gn_b", "bpi", "g1", "be1")))
    nrb = tokens // stat_rows
    inputs = {"x": dev16(x), "cs": col_partials(x.reshape(B, tokens, C), nrb)}

    def run(inp):
        tok, qk, vt = zeros16(B, tokens, C), zeros16(B, tokens, 2 * C), zeros16(B, C, tokens)
        ops.st_head_run(ops.make_st_head_desc(inp["x"], inp["cs"], nrb, stream, vec, tok, qk, vt, tokens, B, tokens, C, tile_rows=tile_rows))
        return [tok, qk, vt]
    I.assert_isolated(f"iso_st_head_r{tile_rows}", run, inputs, {"x": {"rows": tokens}, "cs": {"rows": nrb}}, r, per_b, seed=r)


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("ctx_len,ctx_cap", [(77, 80), (200, 200)], ids=["ctx77", "long200"])      # > 96 keys: the LONG instantiation
@pytest.mark.parametrize("heads", [5, 8])
@pytest.mark.parametrize("tile_rows", [32, 64])
def test_st_tail(ops, tile_rows, heads, ctx_len, ctx_cap, r):
    """The fused tail of a transformer block: the output rows and the column statistics of r's row blocks."""
    from test_stchain_gpu import make_case
    tokens, C = 64, 320
    assert ops.st_tail_supported(C, heads, C // heads, tokens, tile_rows)
    w, x = make_case(7 + heads, B, tokens, C, heads, ctx_len, 64, ctx_cap=ctx_cap)
    stream, vec = ops.pack_st_tail(*(dev16(w[n]) for n in ("o1", "q2", "o2", "ff1", "ff2", "po")),
                                   *(dev32(w[n]) for n in ("bo1", "g2", "be2", "bo2", "g3", "be3", "b1", "b2", "bpo")))
    inputs = {n: dev16(x[n]) for n in ("attn_o", "tok", "x_in", "k", "vt")}
    per = {n: {"rows": tokens} for n in ("attn_o", "tok", "x_in")}
    per.update(k={"axis": 0}, vt={"axis": 0})
    nrb = tokens // tile_rows

    def run(inp):
        out, cs = zeros16(B, tokens, C), zeros32(B, nrb, C, 2)
        d = ops.make_st_tail_desc(inp["attn_o"], inp["tok"], inp["x_in"], out, inp["k"], inp["vt"], stream, vec, B, tokens, C, heads,
                                  C // heads, ctx_len, ctx_cap, tile_rows=tile_rows, colstats_out=cs)
        ops.st_tail_run(d)
        return [out, cs]
    I.assert_isolated(f"iso_st_tail_r{tile_rows}_h{heads}_ctx{ctx_len}", run, inputs, per, r, per_b, seed=seed_of(heads, ctx_len, r))


# --------------------------------------------------------------------------- the sampler step: scalar, table and slot entries
LATENTS = {"4x8x8": (4, 8, 8), "4x5x5": (4, 5, 5)}      # 256 elements per sample (vector path), 100 (the scalar path)
COEF3 = (55 / 24, -59 / 24, 37 / 24, -9 / 24)
TICK, CAP = 5, 4


def nhwc8(e):
    """NCHW values -> the UNet's NHWC fp16 output layout [B][HW][8]; the pad channels hold a value that must not be read."""
    Bn, C, H, W = e.shape
    buf = np.full((Bn, H * W, 8), 1e4, np.float32)
    buf[:, :, :C] = e.transpose(0, 2, 3, 1).reshape(Bn, H * W, C)
    return dev16(buf)


def step_tensors(rng, shape):
    """x, the model's point, both halves of the model output (each sample at its own scale), three old eps, the noise."""
    full = (B,) + shape
    su = np.array([0.5, 1.0, 3.0], np.float32).reshape(B, 1, 1, 1)
    t = {k: dev32(rng.standard_normal(full)) for k in ("x", "xm", "old1", "old2", "old3", "noise")}
    t.update(vu=nhwc8(h16(su * rng.standard_normal(full))), vc=nhwc8(h16(np.roll(su, 1, 0) * rng.standard_normal(full))))
    return t, {k: {"axis": 0} for k in t}


def step_rows(ops, phis, shift=0.0):
    """[B, STEP_ROW]: every sample its own guidance scale, rescale, model point, multistep coefficients, schedule point, sigma."""
    t = np.zeros((B, ops.STEP_ROW), np.float32)
    for b in range(B):
        a_t, a_prev, sigma = 0.3 + 0.05 * b + shift, 0.5 + 0.04 * b + shift, 0.3 * (1 + 0.1 * b)
        t[b, ops.STEP_ACTIVE] = 1.0
        t[b, ops.STEP_CFG_SCALE], t[b, ops.STEP_RESCALE] = 1.5 + 2.0 * b + 10 * shift, phis[b]
        t[b, ops.STEP_SQRT_AT_MODEL], t[b, ops.STEP_SQRT_ONE_MINUS_AT_MODEL] = np.sqrt(0.4 + 0.03 * b), np.sqrt(0.6 - 0.03 * b)
        t[b, ops.STEP_C0:ops.STEP_C0 + 4] = [c * (1 + 0.125 * b) for c in COEF3]
        t[b, ops.STEP_SQRT_AT:ops.STEP_SIGMA + 1] = (np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_prev), np.sqrt(1 - a_prev - sigma ** 2), sigma)
    return dev32(t)


def step_outputs(x):
    return [torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x), zeros32(B, 1)]      # x_prev, pred_x0, e_t, factor


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("entry", ["step", "pred_eps", "pred_v", "rescale_eps", "rescale_v"])
@pytest.mark.parametrize("latent", sorted(LATENTS))
def test_sampler_step_scalar_entries(ops, latent, entry, r):
    """mdx_sampler_step_f32 / _pred_f32 / _rescale_f32: one set of scalars for the batch, so only the tensors are per sample; in
    the rescale entry one workgroup owns a sample and reduces its two standard deviations."""
    inputs, per = step_tensors(np.random.RandomState(seed_of("step", latent, entry)), LATENTS[latent])
    pred = ops.PRED_V if entry.endswith("_v") else ops.PRED_EPS
    upd = (math.sqrt(0.3), math.sqrt(0.7), math.sqrt(0.5), math.sqrt(0.5 - 0.09), 0.3)

    def run(i):
        xp, p0, et, f = step_outputs(i["x"])
        olds = [i["old1"], i["old2"], i["old3"]]
        if entry == "step":
            ops.sampler_step(i["x"], i["vu"], i["vc"], 8, 7.5, olds, COEF3, *upd, i["noise"], et, xp, p0)
        elif entry.startswith("pred"):
            ops.sampler_step_pred(i["x"], i["xm"], i["vu"], i["vc"], 8, 7.5, pred, math.sqrt(0.4), math.sqrt(0.6), olds, COEF3, *upd,
                                  i["noise"], et, xp, p0)
        else:
            ops.sampler_step_rescale(i["x"], i["xm"], i["vu"], i["vc"], 8, 7.5, pred, math.sqrt(0.4), math.sqrt(0.6), olds, COEF3, *upd,
                                     i["noise"], et, xp, p0, 0.7, f.view(B))
        return [xp, p0, et] + ([f] if entry.startswith("rescale") else [])
    I.assert_isolated(f"iso_sampler_{entry}_{latent}", run, inputs, per, r, per_b, seed=seed_of(latent, entry, r))


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("any_rescale", [0, 1])
@pytest.mark.parametrize("pred", [0, 1])
@pytest.mark.parametrize("latent", sorted(LATENTS))
def test_sampler_step_table(ops, latent, pred, any_rescale, r):
    """mdx_sampler_step_table_f32: the neighbours' table rows are perturbed with their tensors (another valid row, NaN, +Inf --
    the ACTIVE flag, the scales and the schedule point included).  With any_rescale every row rescales with its own phi."""
    inputs, per = step_tensors(np.random.RandomState(seed_of("table", latent, pred, any_rescale)), LATENTS[latent])
    phis = (0.3, 0.7, 1.0) if any_rescale else (0.0, 0.0, 0.0)
    inputs["table"], per["table"] = step_rows(ops, phis), {"axis": 0, "other": step_rows(ops, phis[::-1], shift=0.07)}

    def run(i):
        xp, p0, et, f = step_outputs(i["x"])
        ops.sampler_step_table(i["x"], i["xm"], i["vu"], i["vc"], pred, [i["old1"], i["old2"], i["old3"]], i["noise"], et, xp, p0,
                               i["table"], any_rescale, f.view(B))
        return [xp, p0, et] + ([f] if any_rescale else [])
    I.assert_isolated(f"iso_sampler_table_{latent}_p{pred}_r{any_rescale}", run, inputs, per, r, per_b,
                      seed=seed_of(latent, pred, any_rescale, r))


def slot_inputs():
    """Every slot active at tick 5 (positions 0, 2, 3 of capacity 4); the perturbed neighbours sit at position 4 == their length
    (ended), -1 (not started) and 1."""
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    inputs = {"start": i32([5, 3, 2]), "len": i32([4, 4, 4])}
    per = {"start": {"axis": 0, "other": i32([1, 6, 4])}, "len": {"axis": 0, "other": i32([4, 4, 3])}}
    return inputs, per, [0, 2, 3]


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("any_rescale", [0, 1])
@pytest.mark.parametrize("pred", [0, 1])
@pytest.mark.parametrize("latent", sorted(LATENTS))
def test_sampler_step_slots(ops, latent, pred, any_rescale, r):
    """mdx_sampler_step_slots_f32: the neighbours' schedule rows, slot_start and slot_len move with their tensors."""
    inputs, per = step_tensors(np.random.RandomState(seed_of("slots", latent, pred, any_rescale)), LATENTS[latent])
    slots, slots_per, pos = slot_inputs()
    inputs.update(slots)
    per.update(slots_per)
    phis = (0.3, 0.7, 1.0) if any_rescale else (0.0, 0.0, 0.0)
    own, decoy = step_rows(ops, phis), step_rows(ops, (0.5, 0.5, 0.5), shift=0.05)
    sched = torch.stack([decoy.roll(k + 1, 0) for k in range(CAP)], 1).contiguous()      # another request's row at every other position
    for b in range(B):
        sched[b, pos[b]] = own[b]
    inputs["sched"], per["sched"] = sched, {"axis": 0, "other": sched.roll(1, 1).roll(1, 0).contiguous()}

    def run(i):
        xp, p0, et, f = step_outputs(i["x"])
        ops.sampler_step_slots(i["x"], i["xm"], i["vu"], i["vc"], pred, [i["old1"], i["old2"], i["old3"]], i["noise"], et, xp, p0,
                               i["sched"], i["start"], i["len"], TICK, any_rescale, f.view(B))
        return [xp, p0, et] + ([f] if any_rescale else [])
    I.assert_isolated(f"iso_sampler_slots_{latent}_p{pred}_r{any_rescale}", run, inputs, per, r, per_b,
                      seed=seed_of(latent, pred, any_rescale, r))


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("latent", sorted(LATENTS))
def test_randn_slots_and_slot_gather(ops, latent, r):
    """mdx_randn_slots_f32 (the neighbours' seeds and slot positions move) and mdx_slot_gather_f32 (their rows and positions)."""
    shape = LATENTS[latent]
    n = int(np.prod(shape))
    inputs, per, _ = slot_inputs()
    inputs["seeds"], per["seeds"] = ops.seeds_tensor([11, -3, 1 << 40], DEV), {"axis": 0, "other": ops.seeds_tensor([5, 6, 7], DEV)}
    inputs["src"], per["src"] = dev32(np.random.RandomState(n).standard_normal((B, CAP, n))), {"axis": 0}

    def run(i):
        rnd, got = zeros32(B, *shape), zeros32(2 * B, n)
        ops.randn_slots(i["seeds"], ops.RNG_STEP, 3, i["start"], i["len"], TICK, rnd, scale=0.75)
        ops.slot_gather(i["src"], i["start"], i["len"], TICK, got, reps=2)
        return [rnd, got.view(2, B, n).transpose(0, 1)]
    I.assert_isolated(f"iso_slots_randn_gather_{latent}", run, inputs, per, r, per_b, seed=seed_of(latent, r))


# --------------------------------------------------------------------------- elementwise kernels with per-sample parameters
def moments8(rng, hw):
    """Encoder moments NHWC fp16 [B, hw, 8]: 4 means, 4 log-variances."""
    return dev16(h16(np.concatenate([rng.standard_normal((B, hw, 4)), 0.5 * rng.standard_normal((B, hw, 4))], 2)))


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("latent", sorted(LATENTS))
def test_q_sample_and_vae_encode_noised(ops, latent, r):
    shape = LATENTS[latent]
    full = (B,) + shape
    rng = np.random.RandomState(seed_of("qs", latent))
    inputs = {k: dev32(rng.standard_normal(full)) for k in ("x0", "noise", "img", "post")}
    inputs.update(mask=dev32((rng.rand(B, 1, *shape[1:]) > 0.5).astype(np.float32)), mom=moments8(rng, shape[1] * shape[2]))

    def run(i):
        blended = ops.q_sample(i["x0"], i["noise"], 0.8, 0.6, mask=i["mask"], img=i["img"])
        z0, xt = zeros32(*full), zeros32(*full)
        ops.vae_encode_noised(i["mom"], 4, i["post"], 0.18215, 0.8, 0.6, i["noise"], z0, xt)
        return [blended, ops.q_sample(i["x0"], i["noise"], 0.8, 0.6), z0, xt]
    I.assert_isolated(f"iso_q_sample_encode_{latent}", run, inputs, {k: {"axis": 0} for k in inputs}, r, per_b, seed=seed_of(latent, r))


@pytest.mark.parametrize("r", ROWS)
def test_inpaint_kernels(ops, r):
    """The four inpainting launches with a mask / alpha per sample (mask_b = alpha_b = B)."""
    H = W = 16
    rng = np.random.RandomState(seed_of("inpaint"))
    inputs = {"image": dev32(rng.uniform(-1, 1, (B, 3, H, W))), "decoded": dev32(rng.uniform(-1.2, 1.2, (B, 3, H, W))),
              "mask": dev32((rng.rand(B, 1, H, W) > 0.6).astype(np.float32)), "alpha": dev32(rng.rand(B, 1, H, W)),
              "mom": moments8(rng, 64), "post": dev32(rng.standard_normal((B, 4, 8, 8)))}

    def run(i):
        f32_, u8 = ops.inpaint_composite(i["decoded"], i["image"], i["alpha"], output="both")
        return [ops.inpaint_mask_image(i["image"], i["mask"]), ops.inpaint_concat(i["mom"], 4, i["post"], 0.18215, i["mask"], (8, 8)),
                ops.inpaint_resize_mask(i["mask"], (8, 8)), ops.mask_feather(i["mask"], 1.5), f32_, u8]
    I.assert_isolated("iso_inpaint", run, inputs, {k: {"axis": 0} for k in inputs}, r, per_b, seed=r)


@pytest.mark.parametrize("r", ROWS)
def test_glide_step_and_superres_input(ops, r):
    from minddiffusion_amd.glide.diffusion_creator import _Schedule
    H = W = 8
    rng = np.random.RandomState(seed_of("glide"))
    coef8 = _Schedule("squaredcos_cap_v2", 1000, "10").coef8(5)

    def buf(o):         # [B, 6, H, W] -> NHWC fp16 [B, HW, 8]
        t = np.zeros((B, H * W, 8), np.float32)
        t[:, :, :6] = o.transpose(0, 2, 3, 1).reshape(B, H * W, 6)
        return dev16(t)
    inputs = {"x": dev32(rng.standard_normal((B, 3, H, W))), "oc": buf(h16(rng.standard_normal((B, 6, H, W)))),
              "ou": buf(h16(rng.standard_normal((B, 6, H, W)))), "noise": dev32(rng.standard_normal((B, 3, H, W))),
              "hi": dev32(rng.standard_normal((B, 3, 16, 16))), "low": dev32(np.clip(0.5 * rng.standard_normal((B, 3, 4, 4)), -1, 1))}

    def run(i):
        outs = [torch.zeros_like(i["x"]) for _ in range(4)]
        ops.glide_step(i["x"], i["oc"], i["ou"], 8, 3.0, coef8, 0, 1.0, i["noise"], outs[0], outs[1])      # guided ancestral step
        ops.glide_step(i["x"], i["oc"], None, 8, 1.0, coef8, 1, 0.0, None, outs[2], outs[3])              # DDIM step
        return outs + [ops.glide_superres_input(i["hi"], i["low"])]
    I.assert_isolated("iso_glide", run, inputs, {k: {"axis": 0} for k in inputs}, r, per_b, seed=r)


@pytest.mark.parametrize("r", ROWS)
def test_timestep_embedding_and_dense_small(ops, r):
    """The time-embedding MLP at M = 3: one timestep per sample."""
    rng = np.random.RandomState(seed_of("temb"))
    w, b = dev16(h16(rng.standard_normal((1280, 320)) / math.sqrt(320))), dev32(rng.standard_normal(1280))
    inputs = {"t": dev32(np.array([981.0, 1.0, 500.5]))}
    per = {"t": {"axis": 0, "other": dev32(np.array([21.0, 640.0, 333.25]))}}

    def run(i):
        emb = ops.timestep_embedding(i["t"], 320)
        return [emb, ops.dense_small(emb, w, b, act_out=True)]
    I.assert_isolated("iso_temb_dense_small", run, inputs, per, r, per_b, seed=r)


# --------------------------------------------------------------------------- whole models
_NETS = {}


def unet(name, graph):
    """The constructor variants of tests/test_unet_gpu.py, built once per (variant, eager | captured graph)."""
    if (name, graph) not in _NETS:
        from minddiffusion_amd.configs import SMALL_WUKONG_UNET, TINY_UNET
        from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
        from oracle import ldm as O
        cfg = {"tiny": dict(TINY_UNET), "wukong_style": dict(SMALL_WUKONG_UNET),
               "depth2_updown": dict(TINY_UNET, transformer_depth=2, resblock_updown=True),
               "no_attention_at_level_0": dict(TINY_UNET, attention_resolutions=[2])}[name]
        ocfg = dict(cfg)
        ocfg.setdefault("num_heads", -1)
        ocfg.setdefault("num_head_channels", -1)
        net = UNetModel(**cfg)
        net.use_graph = graph
        net.load_state_dict(O.init_params(ocfg, seed=21))
        _NETS[name, graph] = net, cfg
    return _NETS[name, graph]


@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["tiny", "wukong_style", "depth2_updown", "no_attention_at_level_0"])
def test_unet_forward(name, graph, r):
    """One UNet evaluation at batch 3 on a 16 x 16 latent (256- and 64-token levels): x, t and the context rows of the
    neighbours move together."""
    net, cfg = unet(name, graph)
    rng = np.random.RandomState(seed_of("unet", name))
    inputs = {"x": dev32(rng.standard_normal((B, 4, 16, 16))), "t": dev32(np.array([940.0, 333.0, 7.0])),
              "ctx": dev32(rng.standard_normal((B, 9, cfg["context_dim"])))}
    per = {"x": {"axis": 0}, "ctx": {"axis": 0}, "t": {"axis": 0, "other": dev32(np.array([120.0, 801.0, 499.0]))}}
    run = lambda i: [net(i["x"], i["t"], i["ctx"])]
    I.assert_isolated(f"iso_unet_{name}_graph{int(graph)}", run, inputs, per, r, per_b, seed=seed_of(name, r))
    assert (net._plan(B, 16, 16).graph is not None) == graph, "the captured graph was not what ran"


# --------------------------------------------------------------------------- a request that overflows inside a running batch
@pytest.fixture(scope="module")
def tiny_models():
    import _vpred_util as V
    rng = np.random.RandomState(413)
    models = {"eps": V.tiny_eps_model()[0], "v": V.tiny_eps_model(parameterization="v")[0]}
    return models, dev32(rng.standard_normal((B, V.T, 64))), dev32(rng.standard_normal((B, V.T, 64)))


@pytest.mark.parametrize("phi", [0.0, 0.7], ids=["norescale", "rescale"])
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
@pytest.mark.parametrize("param", ["eps", "v"])
def test_an_overflowing_request_leaves_its_neighbours_alone(tiny_models, param, kind, phi):
    """Four steps at per-request guidance scales [1.5, 1e38, 7.5]: the middle request overflows at its first step and is Inf / NaN
    from then on -- in the UNet batch, in the step table launch, in the rescale reduction of its neighbours' launch.  Requests 0
    and 2 must end bit-equal to the run in which the middle request has scale 3."""
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    models, c, uc = tiny_models
    sampler = (DPMSolverSampler if kind == "dpm" else DDIMSampler)(models[param])

    def run(mid):
        return sampler.sample([4] * B, B, (4, 8, 8), conditioning=c, unconditional_conditioning=uc, seeds=[5, 7, 9],
                              unconditional_guidance_scale=[1.5, mid, 7.5], guidance_rescale=[phi, 0.0, phi], verbose=False)[0].clone()
    sane, wild = run(3.0), run(1e38)
    assert bool(torch.isfinite(sane).all()) and not bool(torch.isfinite(wild[1]).all()), "the middle request did not overflow"
    for b in (0, 2):
        assert bool(torch.isfinite(wild[b]).all()), (param, kind, phi, b)
        assert torch.equal(wild[b], sane[b]), (param, kind, phi, b, float((wild[b] - sane[b]).abs().max()))
    assert not torch.equal(sane[0], sane[2])
