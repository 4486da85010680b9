"""LoRA on the GPU: the merge kernel (mdx_lora_merge_f16) against the Python packers, the merged model buffers against a plain
model loaded with merged parameters, the output against the fp32 oracle on merged parameters, adapter hot swap under a captured
graph, and misuse.

Reference of every check: float64 W + s (B @ A), s = m * alpha / rank (the reference's LoRADense, wukong-huahua
ldm/modules/attention.py:118-126, merged).  Adapters are synthetic (tests/_lora_util.make_adapter), rank 4, alpha 4.

Folded layouts: gamma (.) W' is rounded to fp16 a second time, so a 1-ulp difference of W' can show as 2 ulp there (the product
moves by gamma ulp(W') < 2 ulp of the result, plus the rounding).  The 1-ulp condition is therefore asserted on W' itself (the
un-folded launches), and a folded launch must be BIT-EQUAL to ops.fold_layernorm of the kernel's own W' -- stricter than a ulp
bound -- with S against the float64 row sums of its own fp16 output (rel 1e-6) and cb against the float64 W' beta + b (rel 1e-5)
of that same W'; against a matrix merged in float64 cb is held to CB_INDEP (below)."""
import hashlib

import numpy as np
import pytest
import torch

from _lora_util import ALPHA, RANK, make_adapter, merged_params, one_ulp_condition, ulp_distance
from _util import check
from oracle import ldm as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f16, f32, f64 = torch.float16, torch.float32, torch.float64
# cb against a matrix merged in float64 instead of the kernel's own W': the two matrices differ by 1 ulp (<= 2^-10 of the element)
# in a share p of the elements, so the row sums W' beta differ by about sqrt(p) 2^-10 of their size.  At the cap of the merge
# condition, p = 2e-3, that is 4.4e-5; at the measured shares (2e-4 .. 5e-4) it is 1.4e-5 .. 2.2e-5, and 1.2e-5 is the largest
# value seen (test 1: up to 1.0e-5 at R = 16; model buffers: 3.5e-6 .. 1.2e-5).  The rel 1e-5 of the issue is asserted against
# float64 from the kernel's own W', where it is the accumulation error alone (<= 3e-8).
CB_INDEP = 4.4e-5
SENT = 0x7A5C       # sentinel bit pattern (a finite fp16) around and inside every destination


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def _guarded(n, guard=1024):
    buf = torch.full((n + 2 * guard,), SENT, dtype=torch.int16, device=DEV)
    return buf, buf[guard:guard + n].view(f16)


def _case(N, K, R, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    base = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    A = (torch.randn(max(R, 1), K, generator=g) / K ** 0.5)[:R].contiguous().to(DEV)
    B = (0.5 * torch.randn(N, max(R, 1), generator=g))[:, :R].contiguous().to(DEV)
    gamma = (1.0 + 0.1 * torch.randn(K, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(K, generator=g)).to(DEV)
    bias = (0.05 * torch.randn(N, generator=g)).to(DEV)
    scale = 0.75 * ALPHA / RANK
    ref = base.to(f64)
    if R:
        ref = ref + scale * (B.to(f64) @ A.to(f64))
    return base, (A if R else None), (B if R else None), gamma, beta, bias, scale, ref


def _to_f16(x64):
    """float64 -> fp16 with ONE rounding (torch converts through fp32; fix the rare double-rounding cases up)."""
    h = x64.to(f32).to(f16)
    # candidates: h and its neighbours; pick the nearest to x64 (ties cannot be decided wrongly by more than the tie itself)
    i = h.view(torch.int16).to(torch.int32)
    best, err = h, (h.to(f64) - x64).abs()
    for step in (-1, 1):
        c = (i + step).to(torch.int16).view(f16)
        e = (c.to(f64) - x64).abs()
        take = torch.isfinite(c.to(f32)) & (e < err)
        best, err = torch.where(take, c, best), torch.where(take, e, err)
    return best


SHAPES = [(64, 64), (320, 320), (320, 96), (1280, 768)]


@pytest.mark.parametrize("R", [0, 1, 4, 8, 16])      # 16: the ranks above 8 re-read A inside the row loop
@pytest.mark.parametrize("N,K", SHAPES)
def test_merge_kernel_against_packers(ops, N, K, R):
    base, A, B, gamma, beta, bias, scale, ref64 = _case(N, K, R, seed=1000 * R + N + K)
    ref16 = base.to(f16) if R == 0 else _to_f16(ref64)
    Np, Kp = (N + 63) // 64 * 64, (K + 63) // 64 * 64

    def run(layout, numel, **kw):
        buf, dst = _guarded(numel)
        ops.lora_merge(base, dst, layout, A=A, B=B, scale=scale, **kw)
        snap = buf.clone()
        ops.lora_merge(base, dst, layout, A=A, B=B, scale=scale, **kw)
        assert torch.equal(buf, snap), "two merges of the same inputs differ"
        assert bool((buf[:1024] == SENT).all()) and bool((buf[-1024:] == SENT).all()), "guard bytes were written"
        return buf[1024:-1024], dst

    def cmp(got, want, what):
        if R == 0:
            assert torch.equal(got, want), f"{what}: the pure re-pack differs from the packer"
        else:
            one_ulp_condition(got, want, 1, f"{what} N{N} K{K} R{R}")

    # ROWMAJOR with ld > K: the gap columns keep the sentinel
    ld = K + 16
    raw, dst = run(ops.LORA_ROWMAJOR, (N - 1) * ld + K, ld=ld)
    rows = torch.cat([dst, torch.zeros(ld - K, dtype=f16, device=DEV)]).view(N, ld)
    own = rows[:, :K].contiguous()                  # the kernel's own W'
    cmp(own, ref16, "rowmajor")
    gaps = torch.cat([raw, raw[:ld - K]]).view(N, ld)[:-1, K:]
    assert bool((gaps == SENT).all()), "ROWMAJOR wrote between the rows"

    # TILED, plain: padding exactly zero
    _, dst = run(ops.LORA_TILED, Np * Kp)
    cmp(dst, ops.pack_gemm_weight(ref16), "tiled")
    assert torch.equal(dst, ops.pack_gemm_weight(own)), "TILED and ROWMAJOR disagree on W'"

    # TILED, folded: bit-equal to fold_layernorm + pack_gemm_weight of the kernel's own W'
    S = torch.full((N + 2,), 7.0, device=DEV)
    cb = torch.full((N + 2,), 7.0, device=DEV)
    _, dst = run(ops.LORA_TILED, Np * Kp, gamma=gamma, beta=beta, bias=bias, S=S[1:], cb=cb[1:])
    wg, s_ref, cb_ref = ops.fold_layernorm(own, gamma, beta, bias)
    dfold = ulp_distance(dst, ops.pack_gemm_weight(wg))
    assert torch.equal(dst, ops.pack_gemm_weight(wg)), \
        f"folded weights differ from fold_layernorm of the merged matrix: {int((dfold != 0).sum())} elements, max {int(dfold.max())} ulp"
    assert S[0] == 7.0 and S[-1] == 7.0 and cb[0] == 7.0 and cb[-1] == 7.0
    got_wg = ops.unpack_gemm_weight(dst, N, K)
    s64 = got_wg.to(f64).sum(1)
    cb64 = own.to(f64) @ beta.to(f64) + bias.to(f64)
    rel = lambda a, b: float((a.to(f64) - b).norm() / b.norm())
    cb_indep = float("nan")
    if R:
        cb_indep = rel(cb[1:-1], _to_f16(ref64).to(f64) @ beta.to(f64) + bias.to(f64))
    print(f"LORA fold N{N} K{K} R{R}: S rel {rel(S[1:-1], s64):.2e}  cb rel {rel(cb[1:-1], cb64):.2e}  "
          f"cb rel vs float64-merged W' {cb_indep:.2e}")
    assert rel(S[1:-1], s64) <= 1e-6
    assert rel(cb[1:-1], cb64) <= 1e-5
    if R == 0:
        assert torch.equal(S[1:-1], s_ref)
        assert rel(cb[1:-1], cb_ref.to(f64)) <= 1e-5
    else:
        assert cb_indep <= CB_INDEP     # ... and against W' beta + b of the float64-merged matrix
        # vs the fold of the float64-merged matrix: same share of differing elements, at most 2 ulp (module docstring)
        one_ulp_condition(dst, ops.pack_gemm_weight(ops.fold_layernorm(ref16, gamma, beta, bias)[0]), 2, f"tiled folded N{N} K{K} R{R}")

    # TILED at rows N and 2N of a 3N destination (attn1.qkv): the other rows keep the sentinel; the last one owns the padding
    N3p = (3 * N + 63) // 64 * 64
    for slot in (1, 2):
        raw, dst = run(ops.LORA_TILED, N3p * Kp, dst_n0=slot * N, dst_N=3 * N)
        full = torch.full((3 * N, K), 0.0, dtype=f16, device=DEV)
        full[slot * N:(slot + 1) * N] = own
        want = ops.pack_gemm_weight(full)
        rowmask = torch.zeros((N3p, Kp), dtype=torch.bool, device=DEV)
        rowmask[slot * N:(slot + 1) * N] = True
        if slot == 2:
            rowmask[3 * N:] = True
        mask = _pack_mask(ops, rowmask)
        assert torch.equal(dst[mask], want[mask]), f"slot {slot}: rows differ"
        assert bool((raw[~mask] == SENT).all()), f"slot {slot}: bytes outside the target rows were written"

    # FRAG at a non-zero piece_offset inside a larger per-wave stream
    if N % 32 == 0 and K % 16 == 0:
        ks, stride, off = K // 16, 3 * (K // 16) + 5, K // 16 + 3
        raw, dst = run(ops.LORA_FRAG, N // 32 * stride * 512, dst_N=N, piece_stride=stride, piece_offset=off)
        view = raw.view(N // 32, stride, 512)
        assert torch.equal(dst.view(N // 32, stride, 512)[:, off:off + ks], ops.pack_frag_weight(own))
        assert bool((view[:, :off] == SENT).all()) and bool((view[:, off + ks:] == SENT).all())


def _pack_mask(ops, rowmask):
    """Row mask [Np, Kp] -> the same mask in the tile-major storage order (pack_gemm_weight permutes whole chunks of a row)."""
    return ops.pack_gemm_weight(rowmask.to(f16)) != 0


def test_merge_kernel_rejects_bad_arguments(ops):
    from minddiffusion_amd._lib import MdxError
    base = torch.zeros(64, 64, device=DEV)
    dst = torch.zeros(64 * 64, dtype=f16, device=DEV)
    with pytest.raises(MdxError):
        ops.lora_merge(base, dst[:-8], ops.LORA_TILED)                      # destination too small
    with pytest.raises(MdxError):
        ops.lora_merge(base, dst, ops.LORA_TILED, A=torch.zeros(4, 32, device=DEV), B=torch.zeros(64, 4, device=DEV))
    with pytest.raises(MdxError):
        ops.lora_merge(base, dst, ops.LORA_TILED, A=torch.zeros(65, 64, device=DEV), B=torch.zeros(64, 65, device=DEV))
    with pytest.raises(MdxError):
        ops.lora_merge(base, dst, 3)
    with pytest.raises(MdxError):
        ops.lora_merge(base, dst, ops.LORA_FRAG, piece_stride=4, piece_offset=2)
    assert not bool(dst.any())


# ------------------------------------------------------------------------------------------------ model buffers
def _cfgs(name):
    from minddiffusion_amd.configs import SMALL_WUKONG_UNET, TINY_UNET
    return dict({"tiny": TINY_UNET, "small_wukong": SMALL_WUKONG_UNET}[name])


def _ocfg(cfg):
    c = dict(cfg)
    c.setdefault("num_heads", -1)
    c.setdefault("num_head_channels", -1)
    return c


def _model(cfg, params, lora=False, graph=True):
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    net = UNetModel(**cfg, **(dict(enable_lora=True, lora_rank=RANK, lora_alpha=ALPHA) if lora else {}))
    net.use_graph = graph
    return net.load_state_dict(params)


_PARAMS = {}


def _params(name):
    """(base parameters, adapter 1, adapter 2) per configuration, made once and never modified."""
    if name not in _PARAMS:
        from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
        cfg = _cfgs(name)
        shapes = UNetModel(**cfg, enable_lora=True, lora_rank=RANK, lora_alpha=ALPHA, device="cpu").lora_parameter_shapes()
        _PARAMS[name] = (O.init_params(_ocfg(cfg), seed=3), make_adapter(shapes, 21), make_adapter(shapes, 22))
    return _PARAMS[name]


def _is_target(key):
    return any(s in key for s in (".attn1.qkv.", ".attn1.qk.", ".attn1.v.", ".attn2.q.", ".attn2.k.", ".attn2.v.", ".attn1.o.w",
                                  ".attn2.o.w", ".tail.stream", ".head.stream"))


def _own_cb(ops, net, key):
    """float64 W' beta of a folded consumer (`<block>.attn1.qkv.cb` or `<block>.attn2.q.cb`; neither has a bias) from the merged
    matrices the kernel produces for this model's base, adapter and scale in a row-major destination."""
    t, which = key[:-len(".cb")].rsplit(".attn", 1)
    names, norm = ((["attn1.to_q", "attn1.to_k", "attn1.to_v"], "norm1") if which == "1.qkv" else (["attn2.to_q"], "norm2"))
    scale = net._lora_mult * net.lora_alpha / net.lora_rank
    rows = []
    for n in names:
        base = net._lora_base[t + "." + n]
        A, B = net._lora[t + "." + n]
        rows.append(ops.lora_merge(base, torch.empty(base.numel(), dtype=f16, device=DEV), ops.LORA_ROWMAJOR, A=A, B=B,
                                   scale=scale).view(base.shape))
    return torch.cat(rows, 0).to(f64) @ net.w[t + "." + norm + ".b"].to(f64)


@pytest.mark.parametrize("merge", ["1", "0"])
@pytest.mark.parametrize("fold", ["1", "0"])
@pytest.mark.parametrize("name", ["small_wukong", "tiny"])
def test_model_buffers_match_a_plain_model_on_merged_parameters(ops, monkeypatch, name, fold, merge):
    monkeypatch.setenv("MDX_UNET_LN_FOLD", fold)
    monkeypatch.setenv("MDX_UNET_QKV_MERGE", merge)
    cfg = _cfgs(name)
    base, ad1, _ = _params(name)
    a = _model(cfg, base, lora=True)
    ptrs = {k: v.data_ptr() for k, v in a.w.items()}
    assert not a.lora_loaded
    a.load_lora_state_dict(ad1)
    assert a.lora_loaded
    b = _model(cfg, merged_params(base, ad1, ALPHA / RANK))
    plain = _model(cfg, base)
    assert set(a.w) == set(b.w)
    assert (name == "small_wukong") == any(k.endswith("tail.stream") for k in a.w)
    assert (name == "small_wukong") == any(k.endswith("head.stream") for k in a.w)
    assert any(k.endswith("attn1.qkv.w") for k in a.w) == (merge == "1")
    assert any(k.endswith("attn2.q.s") for k in a.w) == (fold == "1")
    shares, cb_rels = [], []
    for k in sorted(a.w):
        ta, tb = a.w[k], b.w[k]
        if not _is_target(k):
            assert torch.equal(ta, tb), k
        elif ta.dtype == f16:
            # folded weights (an `.s` next to the `.w`): up to 2 ulp, see the module docstring
            folded = k.endswith(".w") and (k[:-2] + ".s") in a.w
            shares.append(one_ulp_condition(ta, tb, 2 if folded else 1, k))
        elif k.endswith(".s"):      # the property the fold relies on: S = the row sums of the model's OWN fp16 weights
            wk = a.w[k[:-2] + ".w"]
            n = ta.numel()
            own = ops.unpack_gemm_weight(wk, n, wk.numel() // ((n + 63) // 64 * 64)).to(f64).sum(1)
            assert float((ta.to(f64) - own).norm() / own.norm()) <= 1e-6, k
        else:
            # cb = W' beta (+ b), as in the kernel test: rel 1e-5 against float64 from the merged matrix the kernel itself produces
            # (the same launch with a row-major destination), and against the plain model's, which folds the float64-merged matrix
            assert k.endswith(".cb"), k
            own = _own_cb(ops, a, k)
            r_own = float((ta.to(f64) - own).norm() / own.norm())
            r_plain = float((ta.to(f64) - tb.to(f64)).norm() / tb.to(f64).norm())
            cb_rels.append((r_own, r_plain))
            assert r_own <= 1e-5, f"{k}: cb is {r_own:.2e} from float64 W' beta"
            assert r_plain <= CB_INDEP, f"{k}: cb is {r_plain:.2e} from the plain model's"
    print(f"LORA model buffers {name} fold={fold} merge={merge}: worst differing share {max(shares):.3e}"
          + (f", worst cb rel {max(r[0] for r in cb_rels):.2e} (own W') / {max(r[1] for r in cb_rels):.2e} (plain model)" if cb_rels else ""))
    # hot states: scale 0 and unload both give the base model bit for bit, on the same buffers
    a.set_lora_scale(0.0)
    for k in a.w:
        assert torch.equal(a.w[k], plain.w[k]), f"scale 0: {k}"
    a.set_lora_scale(1.0)
    for k in a.w:
        if _is_target(k) and a.w[k].dtype == f16 and not k.endswith("stream"):
            assert not torch.equal(a.w[k], plain.w[k]), k
    a.unload_lora()
    assert not a.lora_loaded
    for k in a.w:
        assert torch.equal(a.w[k], plain.w[k]), f"unload: {k}"
    assert {k: v.data_ptr() for k, v in a.w.items()} == ptrs
    assert plain.weight_bytes() < a.weight_bytes()


# ------------------------------------------------------------------------------------------------ output against the oracle
def _inputs(B, H, W, T, D, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(B, 4, H, W).astype(np.float32), rng.randn(B, T, D).astype(np.float32)


_ORACLE = {}


def _oracle_outputs():
    """Oracle outputs on base / merged (m = 1) / merged (m = 0.5) parameters for the one input of the output test."""
    if not _ORACLE:
        cfg = _cfgs("small_wukong")
        base, ad1, _ = _params("small_wukong")
        x, ctx = _inputs(2, 16, 16, 9, cfg["context_dim"], seed=4)
        ts = np.array([731.0, 105.0], np.float32)
        _ORACLE["in"] = (x, ts, ctx)
        for key, m in (("base", None), ("m1", 1.0), ("m05", 0.5)):
            p = base if m is None else merged_params(base, ad1, m * ALPHA / RANK)
            _ORACLE[key] = O.UNetOracle(_ocfg(cfg), p)(x, torch.tensor(ts), ctx)
    return _ORACLE


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_unet_output_against_the_oracle_on_merged_parameters(ops, graph, fused):
    """fused: the planner's fused SpatialTransformer head / tail launches (which read head.stream / tail.stream) forced on at
    this small shape through the documented option; by default they start at 192 row blocks."""
    ref = _oracle_outputs()
    assert _rel(ref["m1"], ref["base"]) >= 5e-2 and _rel(ref["m05"], ref["base"]) >= 5e-2, "the adapter does not show in the oracle"
    cfg = _cfgs("small_wukong")
    base, ad1, _ = _params("small_wukong")
    x, ts, ctx = (torch.tensor(v, device=DEV) for v in ref["in"])
    keep = ops.get_option("unet_st_tail")
    try:
        if fused:
            ops.set_option("unet_st_tail", 32)
        net = _model(cfg, base, lora=True, graph=graph)
        got0 = net(x, ts, ctx).clone()
        check(f"lora_unet_base_graph{int(graph)}_fused{int(fused)}", got0, ref["base"], rel_l2=5e-3)
        net.load_lora_state_dict(ad1)
        got1 = net(x, ts, ctx).clone()
        check(f"lora_unet_m1_graph{int(graph)}_fused{int(fused)}", got1, ref["m1"], rel_l2=5e-3)
        assert _rel(got1, got0) >= 5e-2
        net.set_lora_scale(0.5)
        got05 = net(x, ts, ctx).clone()
        check(f"lora_unet_m05_graph{int(graph)}_fused{int(fused)}", got05, ref["m05"], rel_l2=5e-3)
        assert _rel(got05, got0) >= 5e-2
        net.unload_lora()
        assert torch.equal(net(x, ts, ctx), got0)
        P = net._plans[(2, 16, 16)]
        assert len(net._plans) == 1
        infos = [m["info"] for m in P.meta]
        assert any(i.startswith("st_tail") for i in infos) == fused
        assert any(i.startswith("st_head") for i in infos) == fused
        assert (P.graph is not None) == graph
    finally:
        ops.set_option("unet_st_tail", keep)


# ------------------------------------------------------------------------------------------------ hot swap under a graph
def _sample(net, x_T, c, uc):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    model = LatentDiffusion(net, linear_start=0.00085, linear_end=0.0120, timesteps=1000)
    out, _ = DDIMSampler(model).sample(4, 2, (4, 8, 8), conditioning=c, x_T=x_T, unconditional_guidance_scale=3.0,
                                       unconditional_conditioning=uc, verbose=False)
    torch.cuda.synchronize()
    return out.clone()


def test_adapter_hot_swap_keeps_plans_and_graphs(ops):
    cfg = _cfgs("tiny")
    base, ad1, ad2 = _params("tiny")
    rng = np.random.RandomState(9)
    x_T = torch.tensor(rng.randn(2, 4, 8, 8).astype(np.float32), device=DEV)
    c = torch.tensor(rng.randn(2, 7, 64).astype(np.float32), device=DEV)
    uc = torch.tensor(rng.randn(2, 7, 64).astype(np.float32), device=DEV)
    net = _model(cfg, base, lora=True).load_lora_state_dict(ad1)
    first = _sample(net, x_T, c, uc)
    plans = dict(net._plans)
    graphs = {k: (p.graph, p.dup_graph) for k, p in plans.items()}
    assert any(g is not None for pair in graphs.values() for g in pair), "the sampling run captured no graph"
    net.load_lora_state_dict(ad2)
    second = _sample(net, x_T, c, uc)           # the SAME context tensor objects: the cached K / V^T must not survive the swap
    assert set(net._plans) == set(plans) and all(net._plans[k] is plans[k] for k in plans), "the swap re-planned"
    for k, p in plans.items():
        assert (p.graph, p.dup_graph) == graphs[k] and p.graph is graphs[k][0] and p.dup_graph is graphs[k][1], "the swap re-captured"
    fresh = _model(cfg, base, lora=True).load_lora_state_dict(ad2)
    want = _sample(fresh, x_T, c, uc)
    assert torch.equal(second, want)
    assert not torch.equal(second, first)
    # The samplers build their [uncond ; cond] batch anew per sample(), so the UNet saw a new context OBJECT above.  A serving
    # loop that calls the UNet itself keeps one: the K / V^T it cached under adapter 2 must not be used under adapter 1.
    # (Checked by hand: without the cache reset in UNetModel._merge_lora this is the assertion that fails.)
    x = torch.tensor(rng.randn(4, 4, 8, 8).astype(np.float32), device=DEV)
    ts = torch.tensor([801.0, 801.0, 401.0, 401.0], device=DEV)
    ctx = torch.cat([uc, c], 0).contiguous()
    net(x, ts, ctx)
    plan, graph = net._plans[(4, 8, 8)], net._plans[(4, 8, 8)].graph
    assert graph is not None
    got = net.load_lora_state_dict(ad1)(x, ts, ctx).clone()
    assert net._plans[(4, 8, 8)] is plan and plan.graph is graph
    assert torch.equal(got, fresh.load_lora_state_dict(ad1)(x, ts, ctx)), "stale context projections after the swap"


# ------------------------------------------------------------------------------------------------ misuse
def _checksum(net):
    h = hashlib.sha256()
    for k in sorted(net.w):
        h.update(net.w[k].cpu().numpy().tobytes())
    return h.hexdigest()


def test_misuse_raises_and_leaves_the_weights_alone():
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    cfg = _cfgs("tiny")
    base, ad1, _ = _params("tiny")
    net = UNetModel(**cfg, enable_lora=True, lora_rank=RANK, lora_alpha=ALPHA)
    with pytest.raises(MdxError, match="load_state_dict"):
        net.load_lora_state_dict(ad1)
    net.load_state_dict(base)
    before = _checksum(net)
    k = next(iter(ad1))
    wrong_rank = {n: (v[:2] if n.endswith("lora_a") else v[:, :2]) for n, v in ad1.items()}
    with pytest.raises(ValueError, match="shape"):
        net.load_lora_state_dict(wrong_rank)
    with pytest.raises(ValueError, match="shape"):
        net.load_lora_state_dict(dict(ad1, **{k: ad1[k][:, :-8]}))
    with pytest.raises(KeyError, match="missing"):
        net.load_lora_state_dict({n: v for n, v in ad1.items() if n != k})
    assert _checksum(net) == before and not net.lora_loaded
    with pytest.raises(MdxError, match="enable_lora"):
        UNetModel(**cfg).load_state_dict(base).load_lora_state_dict(ad1)


# ------------------------------------------------------------------------------------------------ the other ways in
def _same_weights(a, b):
    assert set(a.w) == set(b.w)
    for k in a.w:
        assert torch.equal(a.w[k], b.w[k]), k


def test_one_dict_load_and_the_surface_above_the_unet(tmp_path):
    """load_state_dict with the adapter in the same dict, a later base-only load, LatentDiffusion.load_lora (dict with the
    checkpoint prefix, and a .ckpt path) / set_lora_scale / unload_lora: all bit-equal to the two-call flow."""
    from minddiffusion_amd import ms_checkpoint as C
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    cfg = _cfgs("tiny")
    base, ad1, _ = _params("tiny")
    two = _model(cfg, base, lora=True).load_lora_state_dict(ad1)
    one = _model(cfg, dict(base, **ad1), lora=True)
    assert one.lora_loaded
    _same_weights(one, two)
    with pytest.raises(KeyError, match="unexpected"):
        one.load_state_dict(dict(base, **ad1, **{"foo.tk_delta_lora_a": np.zeros((4, 4), np.float32)}))
    loose = _model(cfg, base, lora=True).load_state_dict(dict(base, **ad1, **{"foo.tk_delta_lora_a": np.zeros((4, 4), np.float32), "bar": np.zeros(1)}), strict=False)
    _same_weights(loose, two)
    plain = _model(cfg, base)
    one.load_state_dict(base)           # a new base load drops the adapter
    assert not one.lora_loaded
    _same_weights(one, plain)
    # the caller's tensors are not retained: overwriting them afterwards changes nothing
    dev_base = {k: torch.tensor(v, device=DEV) for k, v in base.items()}
    dev_ad = {k: torch.tensor(v, device=DEV) for k, v in ad1.items()}
    kept = _model(cfg, dev_base, lora=True).load_lora_state_dict(dev_ad)
    for name in kept._lora_base:            # the merge sources: fp32 device tensors that would pass through unconverted
        dev_base[name + ".weight"].fill_(3.0)
    for v in dev_ad.values():
        v.fill_(3.0)
    kept.set_lora_scale(0.5).set_lora_scale(1.0)
    _same_weights(kept, two)
    # LatentDiffusion
    ldm = LatentDiffusion(_model(cfg, base, lora=True), linear_start=0.00085, linear_end=0.0120, timesteps=1000)
    ldm.load_lora({C.UNET_PREFIX + k: v for k, v in ad1.items()})
    _same_weights(ldm.unet, two)
    ldm.set_lora_scale(0.5)
    _same_weights(ldm.unet, _model(cfg, base, lora=True).load_lora_state_dict(ad1).set_lora_scale(0.5))
    ldm.unload_lora()
    _same_weights(ldm.unet, plain)
    blob = {C.UNET_PREFIX + k: v for k, v in ad1.items()}
    blob[C.UNET_PREFIX + "out.0.gamma"] = np.ones(64, np.float32)
    C.save_checkpoint(blob, tmp_path / "lora.ckpt")
    ldm.set_lora_scale(1.0).load_lora(str(tmp_path / "lora.ckpt"))
    _same_weights(ldm.unet, two)
    ldm.unload_lora().load_lora(tmp_path / "lora.ckpt")
    _same_weights(ldm.unet, two)
