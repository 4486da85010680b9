"""GroupNorm / LayerNorm / LayerNorm-fold sites under the input regimes of tests/_norm_regimes.py, one launch form at a time.

Every site is compared with a float64 numpy reference computed from the same fp16-rounded values.  What the regimes add to the
ordinary `randn * 1.5 + 0.3` input: `eps` makes the epsilon a 25 % effect (run with 1e-5 AND 1e-6, so a dropped, hard-coded or
swapped eps fails one of them), the `offset*` regimes load the one-pass variance sum x^2 / n - mean^2, `const` leaves nothing
but the clamp and eps between the output and a NaN, `spike` lets one value own the variance.  Every GroupNorm case asserts the
launch form it means to test through mdx_groupnorm_query; every GroupNorm / LayerNorm output sits inside a larger buffer whose
sentinel bytes before and after it must survive.

Tolerances (stated by the project for the same kernels; tests/test_norm_regimes_cpu.py shows that a correct one-pass fp32 kernel
meets them with a 3 x margin at offset32): GroupNorm / LayerNorm rel-L2 1e-3, max_abs 2e-2 (FiLM 3e-2; not for `spike`);
LayerNorm fold 2e-3 (GEGLU 3e-3); constant and all-zero groups max_abs 4e-3 against act(beta) (fp16 rounding of |beta| <= 3 is
<= 2e-3, the statistic term <= 1 ulp of 4.0 x rstd <= 316 x |gamma| <= 3 < 5e-4); `offset128` on the one-pass GroupNorm forms:
finite and rel-L2 <= 4 * one_pass_floor + 5e-4 (the floor is emulated from the same input; 4 covers the spread between
accumulation orders, 5e-4 is fp16 output rounding); `offset128` on ln_kernel (two-pass): the ordinary 1e-3.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

import _guard as G
import _norm_regimes as R
from _util import check, h16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.float16)


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, torch.float32)


def guarded(shape):
    """(buffer, view): an fp16 output of `shape` in the middle of a sentinel-filled buffer (tests/_guard.py; the output starts as
    sentinel too, so an element the launch leaves out shows up as an error)."""
    return G.guarded(shape, torch.float16, device=DEV)


def assert_guard(buf, out, name):
    G.assert_footprint(buf, out, name)


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


def eps_values(regime):
    return (1e-5, 1e-6) if regime == "eps" else (1e-5,)


def gn_eps_values(regime):
    """GroupNorm also runs `const` with the SpatialTransformer's eps = 1e-6, where rstd of a zero-variance group reaches 1000 and
    the statistic term is at its largest.  The 4e-3 bound on those groups still holds: 1e-3 (fp16 rounding of |beta| < 4)
    + 1.4e-3 (mean off by <= 2 ulp of 4.0, x rstd <= 1000 x |gamma| <= 3) + 1e-3 (the kernel's x * a + shift at |shift| <= 12000:
    one fp32 rounding each for shift and the sum).  (The variance of a group == 4.0 cannot round below zero: sum = 4 n and
    sumsq = 16 n are exact, fl(n * fl(1 / n)) <= 1 in round-to-nearest, so mean = 4 (1 - d) with d >= 0 and
    sumsq / n - mean^2 = 16 d (1 - d) >= 0 -- these groups test eps and the apply arithmetic, not the `var < 0` clamp.)"""
    return (1e-5, 1e-6) if regime in ("eps", "const") else (1e-5,)


# --------------------------------------------------------------------------- GroupNorm: forms x regimes x SiLU
# id, B, H, W, C1, C2, library options, kind, form the query must report, further query fields it must report
GN_CASES = [
    ("two_launch_cap64", 1, 32, 32, 320, 0, {}, "plain", "two_launch", dict(nblk=64)),      # cpg 10: 1024 * 80 B > 64 KiB
    ("two_launch_ragged_2src", 2, 33, 31, 320, 320, {}, "plain", "two_launch", dict(nblk=64, pix=16)),      # 1023 = 63 * 16 + 15
    ("two_launch_cap256", 1, 128, 128, 64, 0, {}, "plain", "two_launch", dict(nblk=256)),
    ("fused_one_pass_8x8", 2, 8, 8, 1280, 0, {}, "plain", "fused_one_pass", dict(threads=1024)),
    ("fused_one_pass_2x2", 3, 2, 2, 1280, 0, {}, "plain", "fused_one_pass", dict(threads=1024)),
    ("fused_two_reads_8x8", 2, 8, 8, 1280, 0, dict(gn_prefetch=0), "plain", "fused", dict(threads=1024)),
    ("fused_two_reads_2x2", 3, 2, 2, 1280, 0, dict(gn_prefetch=0), "plain", "fused", dict(threads=1024)),
    ("fused_256", 16, 2, 2, 1280, 0, dict(gn_fused_small=1), "plain", "fused_256", dict(threads=256, ncb=32)),
    ("two_launch_forced", 2, 8, 8, 1280, 0, dict(gn_fused=0), "plain", "two_launch", {}),
    ("film_fused", 3, 8, 8, 192, 0, {}, "film", "fused_one_pass", {}),
    ("film_two_launch", 1, 32, 32, 320, 0, {}, "film", "two_launch", {}),
    ("colstats_nrb1", 2, 16, 16, 320, 0, {}, ("colstats", 1, 0), "colstats", dict(cw=5)),
    ("colstats_nrb3", 2, 16, 16, 320, 0, {}, ("colstats", 3, 0), "colstats", dict(cw=5)),
    ("colstats_nrb64", 2, 16, 16, 320, 0, {}, ("colstats", 64, 0), "colstats", dict(cw=5)),
    ("colstats_cpg60_2src", 2, 8, 8, 1280, 640, {}, ("colstats", 4, 2), "colstats", dict(cw=15)),
    ("colstats_wide", 2, 16, 16, 640, 0, dict(gn_wide_rows=1), ("colstats", 1, 0), "colstats", dict(cw=40, nblk=64)),
    # 2 x 256 x 640 fp16 is 0.625 MiB, below gn_boost_mb = 1: the default geometry; the boosted one needs >= 1 MiB (B = 4)
    ("colstats_boost_below", 2, 16, 16, 640, 0, dict(gn_boost_mb=1), ("colstats", 2, 0), "colstats", dict(cw=5, nblk=32)),
    ("colstats_boost", 4, 16, 16, 640, 0, dict(gn_boost_mb=1), ("colstats", 2, 0), "colstats", dict(cw=5, nblk=64, pix=4)),
]


def colstats_of(xs, nrb):
    """Column partials [B * nrb, Cx, 2] of xs [B, HW, Cx] as a producer would emit them for nrb row blocks per sample: float64
    sums of the fp16 values, stored as fp32 (isolates the consumer's fold + apply)."""
    B, HW, Cx = xs.shape
    xs = xs.astype(np.float64)
    out = np.zeros((B, nrb, Cx, 2))
    for j, rows in enumerate(np.array_split(np.arange(HW), nrb)):
        out[:, j, :, 0] = xs[:, rows].sum(1)
        out[:, j, :, 1] = (xs[:, rows] ** 2).sum(1)
    return dev32(out.reshape(B * nrb, Cx, 2).astype(np.float32))


def check_gn(name, regime, x, got, g, b, eps, groups, act, scale=None, shift=None, max_abs=2e-2):
    """got [B, HW, C] from the device against the float64 reference of x [B, C, HW], at the tolerances of the module docstring."""
    got = got.float().cpu().numpy().transpose(0, 2, 1)
    ref = R.gn_ref(x, g, b, eps, groups, act, scale, shift)
    if regime == "offset128":
        floor = R.one_pass_floor(x, groups, g, b, eps, act, scale, shift)
        bound = 4 * floor + 5e-4
        m = check(name, got, ref, one_pass_floor=floor, bound=bound)
        assert m["rel_l2"] <= bound, f"{name}: rel_l2 {m['rel_l2']:.3e} > 4 * {floor:.3e} + 5e-4"
    else:
        check(name, got, ref, rel_l2=1e-3, max_abs=None if regime == "spike" else max_abs)
    if regime == "const":
        B, C, HW = x.shape
        cpg = C // groups
        tgt = np.asarray(b, np.float64)[None, :].repeat(B, 0)
        if scale is not None:
            tgt = tgt * (1.0 + scale.astype(np.float64)) + shift.astype(np.float64)
        tgt = R.silu(tgt) if act else tgt
        for s in range(B):
            for gi in R.const_groups(s, groups):
                sl = slice(gi * cpg, (gi + 1) * cpg)
                d = float(np.abs(got[s, sl] - tgt[s, sl, None]).max())
                assert d <= 4e-3, f"{name}: constant group {gi} of sample {s} is off act(beta) by {d:.3e}"


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: c[0])
def test_groupnorm_forms(ops, case, regime):
    cid, B, H, W, C1, C2, opts, kind, form, fields = case
    C, HW, groups = C1 + C2, H * W, 32
    rng = np.random.RandomState(seed_of(cid, regime))
    x = R.regime(regime, rng, B, C, HW, groups)
    g, b = R.affine(rng, C)
    xn = np.ascontiguousarray(x.transpose(0, 2, 1))
    x1 = dev16(xn[:, :, :C1])
    x2 = dev16(xn[:, :, C1:]) if C2 else None
    gd, bd = dev32(g), dev32(b)
    scale = shift = mod = None
    cs1 = cs2 = None
    nrb1 = nrb2 = 0
    if kind == "film":      # rows [scale | shift] of one tensor, as GLIDE's emb_out chunk: mod_ld = 2 C > C
        scale, shift = rng.uniform(-1, 1, (B, C)).astype(np.float32), rng.uniform(-1, 1, (B, C)).astype(np.float32)
        mod = dev32(np.concatenate([scale, shift], 1))
    elif kind != "plain":
        _, nrb1, nrb2 = kind
        cs1 = colstats_of(xn[:, :, :C1], nrb1)
        cs2 = colstats_of(xn[:, :, C1:], nrb2) if C2 else None
    with options(ops, **opts):
        q = ops.groupnorm_query(C1, C2, B, HW, groups, colstats_nrb=nrb1)
        assert q["form"] == form and all(q[k] == v for k, v in fields.items()), f"{cid}: resolved to {q}"
        if cid == "two_launch_ragged_2src":
            assert HW % q["pix"] != 0
        for act in (False, True):
            for eps in gn_eps_values(regime):
                name = f"regime_gn_{cid}_{regime}_silu{int(act)}_eps{eps:g}"
                buf, out = guarded((B, HW, C))
                if kind == "plain":
                    ops.groupnorm(x1, x2, gd, bd, eps, act, out=out)
                elif kind == "film":
                    ops.groupnorm_scaleshift(x1, x2, gd, bd, mod[:, :C], mod[:, C:], 2 * C, eps, act, out=out)
                else:
                    ops.groupnorm_colstats(x1, cs1, nrb1, x2, cs2, nrb2, gd, bd, eps, act, out=out)
                assert_guard(buf, out, name)
                check_gn(name, regime, x, out, g, b, eps, groups, act, scale, shift, max_abs=3e-2 if kind == "film" else 2e-2)


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("H,W,splitk", [(8, 8, 2), (8, 8, 5), (16, 16, 2), (16, 16, 5)])
def test_groupnorm_from_splitk_slabs(ops, H, W, splitk, regime):
    """mdx_groupnorm_from_splitk_f16: a 1 x 1 conv with the identity as its weight makes the producer's output equal the regime
    input exactly (every slab holds exact partial sums), so the slabs carry the regime into the slab form of gn_fused_kernel."""
    B, C, HW, groups = 2, 320, H * W, 32
    rng = np.random.RandomState(seed_of("splitk", H, splitk, regime))
    x = R.regime(regime, rng, B, C, HW, groups)
    g, b = R.affine(rng, C)
    a = dev16(np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(B * HW, C))
    wp = ops.pack_conv_weight(torch.eye(C, dtype=torch.float32, device=DEV).reshape(C, C, 1, 1))
    gd, bd = dev32(g), dev32(b)
    for act in (False, True):
        for eps in gn_eps_values(regime):
            name = f"regime_gn_from_splitk{splitk}_{H}x{W}_{regime}_silu{int(act)}_eps{eps:g}"
            conv_out = torch.zeros((B * HW, C), dtype=torch.float16, device=DEV)
            d = ops.make_gemm_desc(a, wp, C, B, H, W, C, conv_out, C, ksize=1, splitk=splitk)
            need = ops.gemm_workspace_bytes(d)
            assert need > 0
            ws = ops.new_gemm_workspace(need, DEV)
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
            d.defer_reduce = 1
            assert ops.gemm_query(d)[2] == splitk and ops.groupnorm_from_splitk_ok(d, groups), ops.gemm_query(d)
            ops.gemm_run(d)
            buf, out = guarded((B, HW, C))
            ops.groupnorm_from_splitk(d, gd, bd, eps, act, out, groups)
            assert_guard(buf, out, name)
            assert torch.equal(conv_out, a), f"{name}: the identity conv's output is not its input"
            check_gn(name, regime, x, out, g, b, eps, groups, act)


def test_producers_emit_right_column_partials_under_an_offset(ops):
    """mdx_gemm_desc.colstats_out under an offset: a dense GEMM (zero-centred weights) and an 8 x 16-patch HALO conv with a bias of
    +-8 (alternating by column) store values of mean / std ~ 8; their column partials against float64 column sums of the fp16
    output they stored, at the rel-L2 1e-5 test_gemm_layernorm_fold asks of the row statistics."""
    rng = np.random.RandomState(17)
    for label, B, H, W, Cin, Cout, ks in (("dense", 2, 16, 16, 64, 128, 1), ("halo", 2, 16, 32, 128, 192, 3)):
        x = h16(rng.standard_normal((B, H * W, Cin)))
        w = h16(rng.standard_normal((Cout, Cin, ks, ks)) / math.sqrt(ks * ks * Cin))
        bias = dev32((8.0 * (1 - 2 * (np.arange(Cout) % 2))).astype(np.float32))
        a, wp = dev16(x), ops.pack_conv_weight(torch.from_numpy(w).to(DEV))
        out = torch.empty((B * H * W, Cout), dtype=torch.float16, device=DEV)
        d = ops.make_gemm_desc(a, wp, Cout, B, H, W, Cin, out, Cout, bias=bias, ksize=ks, splitk=1)
        q = ops.gemm_query(d)
        rows = q[5]
        assert rows > 0 and (H * W) % rows == 0 and (ks == 1 or (q[3] == 1 and rows == 128)), q
        nrb = H * W // rows
        cs = torch.full((B * nrb, Cout, 2), float("nan"), dtype=torch.float32, device=DEV)
        d.colstats_out, d.colstats_cap = cs.data_ptr(), B * nrb
        ops.gemm_run(d)
        torch.cuda.synchronize()
        o = out.double().cpu().view(B, H * W, Cout)
        assert 6.0 < float(o.abs().mean()) < 10.0
        if ks == 3:          # HALO patches: 8 rows x 16 columns of pixels
            img = o.view(B, H // 8, 8, W // 16, 16, Cout).permute(0, 1, 3, 2, 4, 5).reshape(B * nrb, 128, Cout)
        else:
            img = o.reshape(B * nrb, rows, Cout)
        check(f"regime_colstats_offset8_{label}_sum", cs[..., 0], img.sum(1), rel_l2=1e-5)
        check(f"regime_colstats_offset8_{label}_sumsq", cs[..., 1], (img * img).sum(1), rel_l2=1e-5)


# --------------------------------------------------------------------------- LayerNorm (ln_kernel<2 | 4 | 8>)
@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("C", [8, 72, 1024, 1032, 2048, 2056, 4096])
def test_layernorm_regimes(ops, C, regime):
    """Two-pass statistics: the offsets cost nothing, offset128 included (the ordinary 1e-3 pins that property)."""
    for rows in (1, 5, 130):
        rng = np.random.RandomState(seed_of("ln", C, rows, regime))
        x = R.regime_rows(regime, rng, rows, C)
        g, b = R.affine(rng, C)
        xd, gd, bd = dev16(x), dev32(g), dev32(b)
        for eps in eps_values(regime):
            name = f"regime_ln_{rows}x{C}_{regime}_eps{eps:g}"
            buf, out = guarded((rows, C))
            ops.layernorm(xd, gd, bd, eps, out=out)
            assert_guard(buf, out, name)
            got = out.float().cpu().numpy()
            check(name, got, R.ln_ref(x, g, b, eps), rel_l2=1e-3, max_abs=None if regime == "spike" else 2e-2)
            if regime == "const":
                for r in np.concatenate(R.const_rows(rows)):
                    d = float(np.abs(got[r] - b.astype(np.float64)).max())
                    assert d <= 4e-3, f"{name}: constant row {r} is off beta by {d:.3e}"


# --------------------------------------------------------------------------- LayerNorm fold
FOLD_REGIMES = ("unit", "eps", "offset8", "offset32", "const")


def fold_problem(ops, regime, rng, M, C, N):
    """Rows of the regime, their per-64-column {sum, sumsq} as a producer GEMM would have emitted them (float64 sums stored as
    fp32), LayerNorm parameters and a projection [N, C] + bias.  ref(eps) is float64 LN(x) W^T + b."""
    x = R.regime_rows(regime, rng, M, C)
    g, be = R.affine(rng, C)
    w = h16(rng.standard_normal((N, C)) / math.sqrt(C))
    bv = rng.standard_normal(N).astype(np.float32)
    xs = x.astype(np.float64).reshape(M, C // 64, 64)
    st = dev32(np.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).astype(np.float32))
    wg, s, cb = ops.fold_layernorm(dev16(w), dev32(g), dev32(be), dev32(bv))
    ref = lambda eps: R.ln_ref(x, g, be, eps) @ w.astype(np.float64).T + bv.astype(np.float64)
    wbeta = w.astype(np.float64) @ be.astype(np.float64) + bv.astype(np.float64)
    return x, st, (wg, s, cb), ref, wbeta


def check_fold(name, regime, got, ref, tol, wbeta=None, **kw):
    got = got.float().cpu().numpy() if isinstance(got, torch.Tensor) else got
    check(name, got, ref, rel_l2=tol, **kw)
    if regime == "const" and wbeta is not None:      # a constant row normalises to beta: its output is W beta + b
        rows = np.concatenate(R.const_rows(got.shape[0]))
        check(name + "_const_rows", got[rows], np.broadcast_to(wbeta, (len(rows), wbeta.shape[-1])), rel_l2=tol)


def run_desc(ops, d):
    need = ops.gemm_workspace_bytes(d)
    ws = ops.new_gemm_workspace(max(need, 16), DEV)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    q = ops.gemm_query(d)
    ops.gemm_run(d)
    torch.cuda.synchronize()
    return q


@pytest.mark.parametrize("regime", FOLD_REGIMES)
@pytest.mark.parametrize("lean", [1, 0, 4])      # option gemm_lean_dense: the product's lean kernel, the generic kernel, and prefetch level 3
                                                   # (row statistics folded in registers before the K loop: its own eps site in csrc/dense.hip)
@pytest.mark.parametrize("C,splitk", [(320, 1), (320, 4), (320, 5), (320, 8), (640, 1), (640, 4), (640, 8)])
def test_layernorm_fold_plain(ops, C, splitk, lean, regime):
    """The plain consumer: the register correction (no split), the in-kernel ticket reduce (4) and the reduce kernel (5, 8), on the
    lean dense kernel (as shipped, and with the row statistics prefetched) and on the generic one.  K = 320 has five 64-wide K tiles: the library refuses an explicit split of 8 there
    (checked: refused on the host, nothing launched), 5 is the split that reaches the reduce kernel at that K."""
    M, N = 128, 640
    if (C, splitk) == (320, 8):
        from minddiffusion_amd._lib import MdxError
        z16 = torch.zeros((M, N), dtype=torch.float16, device=DEV)
        z32 = torch.zeros((M, C // 64, 2), dtype=torch.float32, device=DEV)
        d = ops.make_gemm_desc(z16, z16, N, 1, M, 1, C, z16, N, bias=z32, splitk=splitk, ln_stats=z32, ln_s=z32)
        ws = ops.new_gemm_workspace(ops.gemm_workspace_bytes(d), DEV)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        assert not ops.gemm_check(d)
        with pytest.raises(MdxError):
            ops.gemm_query(d)
        return
    rng = np.random.RandomState(seed_of("fold", C, splitk, regime))
    x, st, (wg, s, cb), ref, wbeta = fold_problem(ops, regime, rng, M, C, N)
    xd, wp = dev16(x), ops.pack_gemm_weight(wg)
    with options(ops, gemm_lean_dense=lean):
        for eps in eps_values(regime):
            out = torch.full((M, N), float("nan"), dtype=torch.float16, device=DEV)
            q = run_desc(ops, ops.make_gemm_desc(xd, wp, N, 1, M, 1, C, out, N, bias=cb, splitk=splitk, ln_stats=st, ln_s=s, ln_eps=eps))
            if splitk == 1:
                assert q[2] == 1 and q[3] == (2 if lean else 0), q
            elif splitk == 4:
                assert q[2] > 1 and q[6] == 1 and q[3] == (2 if lean else 0), q
            else:
                assert q[2] > 4 and q[6] == 0, q
            check_fold(f"regime_lnfold_plain_C{C}_s{splitk}_lean{lean}_{regime}_eps{eps:g}", regime, out, ref(eps), 2e-3, wbeta,
                       resolved_splitk=q[2], in_kernel_reduce=q[6])


@pytest.mark.parametrize("regime", FOLD_REGIMES)
def test_layernorm_fold_geglu(ops, regime):
    M, C = 128, 320
    N = 8 * C
    rng = np.random.RandomState(seed_of("fold_geglu", regime))
    x, st, (wg, s, cb), ref, wbeta = fold_problem(ops, regime, rng, M, C, N)
    il = lambda t: ops.geglu_interleave(t[:N // 2], t[N // 2:], 64)
    xd, wp = dev16(x), ops.pack_gemm_weight(il(wg))

    def geglu(y):
        gate = y[:, N // 2:]
        return y[:, :N // 2] * (0.5 * gate * (1 + np.tanh(math.sqrt(2 / math.pi) * (gate + 0.044715 * gate ** 3))))
    for eps in eps_values(regime):
        out = torch.full((M, N // 2), float("nan"), dtype=torch.float16, device=DEV)
        run_desc(ops, ops.make_gemm_desc(xd, wp, N, 1, M, 1, C, out, N // 2, bias=il(cb), splitk=1, epilogue=ops.EPI_GEGLU,
                                         ln_stats=st, ln_s=il(s), ln_eps=eps))
        check_fold(f"regime_lnfold_geglu_{regime}_eps{eps:g}", regime, out, geglu(ref(eps)), 3e-3, geglu(wbeta[None, :])[0])


@pytest.mark.parametrize("regime", FOLD_REGIMES)
def test_layernorm_fold_merged_qkv(ops, regime):
    B, T, C = 2, 64, 320
    M = B * T
    rng = np.random.RandomState(seed_of("fold_qkv", regime))
    x, st, (wg, s, cb), ref, wbeta = fold_problem(ops, regime, rng, M, C, 3 * C)
    xd, wp = dev16(x), ops.pack_gemm_weight(wg)
    for eps in eps_values(regime):
        qk = torch.full((B, T, 2 * C), float("nan"), dtype=torch.float16, device=DEV)
        vt = torch.full((B, C, T), float("nan"), dtype=torch.float16, device=DEV)
        run_desc(ops, ops.make_gemm_desc(xd, wp, 3 * C, B, T, 1, C, qk, 2 * C, bias=cb, splitk=1, out2=vt, out2_ld=T, n_split=2 * C,
                                         ln_stats=st, ln_s=s, ln_eps=eps))
        full = ref(eps)
        check_fold(f"regime_lnfold_qk_{regime}_eps{eps:g}", regime, qk.reshape(M, 2 * C), full[:, :2 * C], 2e-3, wbeta[:2 * C])
        v = vt.float().cpu().numpy().transpose(0, 2, 1).reshape(M, C)
        check_fold(f"regime_lnfold_vt_{regime}_eps{eps:g}", regime, v, full[:, 2 * C:], 2e-3, wbeta[2 * C:])


@pytest.mark.parametrize("regime", FOLD_REGIMES)
def test_layernorm_fold_tile160(ops, regime):
    """The 128 x 160 tile's epilogue_w41, at the smallest LayerNorm-fold shape of tests/test_dense_tile160_gpu.py."""
    M, N, C = 256, 448, 320
    rng = np.random.RandomState(seed_of("fold_160", regime))
    x, st, (wg, s, cb), ref, wbeta = fold_problem(ops, regime, rng, M, C, N)
    xd, wp = dev16(x), ops.pack_gemm_weight(wg)
    for eps in eps_values(regime):
        out = torch.full((M, N), float("nan"), dtype=torch.float16, device=DEV)
        q = run_desc(ops, ops.make_gemm_desc(xd, wp, N, 1, M, 1, C, out, N, bias=cb, splitk=1, tile_m=128, tile_n=160,
                                             ln_stats=st, ln_s=s, ln_eps=eps))
        assert q[0] == 128 and q[1] == 160 and q[2] == 1 and q[3] == 2, q
        check_fold(f"regime_lnfold_tile160_{regime}_eps{eps:g}", regime, out, ref(eps), 2e-3, wbeta)


@pytest.mark.parametrize("regime", FOLD_REGIMES)
def test_layernorm_fold_cross_attention_epilogue(ops, regime):
    """mdx_gemm_desc.xattn_k on a LayerNorm-fold query projection, at the smallest fold shape of
    test_dense_with_cross_attention_epilogue (8 x 8 level: 64 tokens per sample, 64-row tiles), with that test's tolerances."""
    B, T, C, L, heads = 2, 64, 1280, 77, 20
    cap = (L + 7) // 8 * 8
    rng = np.random.RandomState(seed_of("fold_xattn", regime))
    x = R.regime_rows(regime, rng, B * T, C)
    g, be = R.affine(rng, C)
    wq = h16(rng.standard_normal((C, C)) / math.sqrt(C))
    k = h16(0.7 * rng.standard_normal((B, L, C)) / 3.0)      # (|gamma| <= 3 makes q three times the usual size)
    v = h16(rng.standard_normal((B, L, C)))
    kd = torch.zeros((B, cap, C), dtype=torch.float16, device=DEV)
    kd[:, :L] = dev16(k)
    vtd = torch.zeros((B, C, cap), dtype=torch.float16, device=DEV)
    vtd[:, :, :L] = dev16(np.ascontiguousarray(v.transpose(0, 2, 1)))
    xs = x.astype(np.float64).reshape(B * T, C // 64, 64)
    st = dev32(np.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).astype(np.float32))
    wg, s, cb = ops.fold_layernorm(dev16(wq), dev32(g), dev32(be))
    xd, wp = dev16(x), ops.pack_gemm_weight(wg)
    scale = 64 ** -0.5
    kh = k.astype(np.float64).reshape(B, L, heads, 64).transpose(0, 2, 1, 3)
    vh = v.astype(np.float64).reshape(B, L, heads, 64).transpose(0, 2, 1, 3)
    for eps in eps_values(regime):
        qh = (R.ln_ref(x, g, be, eps) @ wq.astype(np.float64).T).reshape(B, T, heads, 64).transpose(0, 2, 1, 3)
        sc = qh @ kh.transpose(0, 1, 3, 2) * scale
        p = np.exp(sc - sc.max(-1, keepdims=True))
        ref = ((p / p.sum(-1, keepdims=True)) @ vh).transpose(0, 2, 1, 3).reshape(B * T, C)
        out = torch.full((B * T, C), float("nan"), dtype=torch.float16, device=DEV)
        d = ops.make_gemm_desc(xd, wp, C, B, T, 1, C, out, C, tile_n=64, splitk=1, tile_m=64, xattn_k=kd, xattn_vt=vtd, xattn_len=L,
                               xattn_cap=cap, xattn_scale=scale, ln_stats=st, ln_s=s, bias=cb, ln_eps=eps)
        q = ops.gemm_query(d)
        assert q[3] == 2 and q[1] == 64 and q[2] == 1, q
        ops.gemm_run(d)
        torch.cuda.synchronize()
        check(f"regime_lnfold_xattn_{regime}_eps{eps:g}", out, ref, rel_l2=3e-3, max_abs=3e-2)


# --------------------------------------------------------------------------- st_head: the GroupNorm in front of proj_in
@pytest.mark.parametrize("gn_eps", [1e-5, 1e-6])
@pytest.mark.parametrize("regime", ["eps", "offset32"])
def test_st_head_groupnorm_regimes(ops, regime, gn_eps):
    """mdx_st_head_f16 folds the producer's column partials and normalises in LDS: its GroupNorm tap (debug stage 1) under the
    eps and offset32 regimes, against the fp16-storage restatement of tests/test_stchain_gpu.py at that file's tolerances.
    (The LayerNorms inside the chain kernels see values produced inside the kernel: out of scope here.)"""
    from test_stchain_gpu import group_norm_rows, make_head_case
    B, tokens, C, tile_rows, stat_rows = 2, 256, 320, 32, 64
    assert ops.st_head_supported(C, tokens, tile_rows)
    w, _ = make_head_case(5, B, tokens, C)
    rng = np.random.RandomState(seed_of("st_head", regime))
    x = np.ascontiguousarray(R.regime(regime, rng, B, C, tokens, 32).transpose(0, 2, 1)).reshape(B * tokens, C)
    ref = h16(group_norm_rows(x.astype(np.float64), B, tokens, C, w["gn_g"].astype(np.float64), w["gn_b"].astype(np.float64), gn_eps))
    M, nrb = B * tokens, tokens // stat_rows
    xd = dev16(x)
    stream, vec = ops.pack_st_head(*(dev16(w[n]) for n in ("pi", "q", "k", "v")), *(dev32(w[n]) for n in ("gn_g", "gn_b", "bpi", "g1", "be1")))
    cs = colstats_of(x.reshape(B, tokens, C), nrb)
    tok = torch.full((M, C), float("nan"), dtype=torch.float16, device=DEV)
    qk = torch.full((M, 2 * C), float("nan"), dtype=torch.float16, device=DEV)
    vt = torch.full((B, C, tokens), float("nan"), dtype=torch.float16, device=DEV)
    dbg = torch.full((M, C), float("nan"), dtype=torch.float16, device=DEV)
    d = ops.make_st_head_desc(xd, cs, nrb, stream, vec, tok, qk, vt, tokens, B, tokens, C, tile_rows=tile_rows, gn_eps=gn_eps,
                              debug_out=dbg, debug_stage=1)
    ops.st_head_run(d)
    torch.cuda.synchronize()
    check(f"regime_st_head_groupnorm_{regime}_eps{gn_eps:g}", dbg, ref, rel_l2=1e-3, max_rel=6e-3)
