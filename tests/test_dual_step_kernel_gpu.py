"""Three-branch guidance in the step launches: ops.sampler_step_dual (mdx_sampler_step_dual_f32) and ops.sampler_step_lin_dual
(mdx_sampler_step_lin_dual_f32), whose step 1 is  m = u + s_i (m - u) + s_t (c - m)  on the outputs [uu ; ui ; ci].

Reference and bounds.  float64 numpy on the very fp16 outputs and float32 operands the launch gets.  The bounds are the ones of
the forms being extended: rel-L2 1e-5 on x_prev / pred_x0 / e_t_out and 1e-5 relative on the rescale factor
(test_kernels_gpu.test_sampler_step, test_guidance_rescale_gpu); per element 32 * 2^-24 times the sum of the magnitudes of all
terms as they enter for the lin entry (test_dpm_step_kernel_gpu, test_dpm_sde_step_kernel_gpu: a count of roundings, at most 20
here -- the combine has 5 where the pair's has 3).  Thresholding is bit for bit against the numpy-float32 statement on the
launch's own model_pre_out, as there.

Alias identities: out_m = out_u (the same tensor) is the two-branch entry at cfg_scale = s_t and out_m = out_c the two-branch
entry at cfg_scale = s_i, torch.equal on every output -- so every dual kernel is pinned to one that is oracle-tested.
"""
import numpy as np
import pytest
import torch

import _rescale_util as R
from _util import check, metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, V = 0, 1
X0, NOISE = 0, 1
ULP = 32 * 2.0 ** -24
LD = 8
f32 = np.float32
# (2,4,8,8): test_sampler_step's; (3,3,3,3): N = 27 < 64 (the clamp of the statistics' prologue), N % 4 and HW % 4 != 0 (a seeded
# quad straddles channels, the last is partial); (2,4,5,7); (2,4,40,40): N = 6400 > 4096, a second trip of the OWNED loops
SHAPES = [(2, 4, 8, 8), (3, 3, 3, 3), (2, 4, 5, 7), (2, 4, 40, 40)]
SCALES = [(1.5, 7.5), (0.3, 12.0)]                      # (s_i, s_t)
COEF = {0: (1., 0., 0., 0.), 1: (1.5, -0.5, 0., 0.), 3: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}
AM, SM = float(f32(0.83)), float(f32(0.5577))


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops
    return ops


def inputs(shape, seed):
    """NCHW fp32 operands and the three NHWC fp16 outputs (each sample and branch its own spread, so rescale factors differ;
    the pad channels hold a value that must not be read)."""
    B, C, H, W = shape
    rng = np.random.RandomState(seed)
    t = {k: rng.randn(*shape).astype(f32) for k in ("x", "xm", "o1", "o2", "o3", "noise", "h1", "h2")}
    for j, k in enumerate(("u", "m", "c")):
        s = np.array([(0.5, 1.0, 2.0)[(b + j) % 3] for b in range(B)], f32).reshape(B, 1, 1)
        o = np.full((B, H * W, LD), 1e4, np.float16)
        o[..., :C] = (s * rng.randn(B, H * W, C) + 0.1).astype(np.float16)
        t[k] = o
    return t


def nchw(o, shape):
    B, C, H, W = shape
    return o[..., :C].astype(np.float64).reshape(B, H * W, C).transpose(0, 2, 1).reshape(shape)


def dev(a):
    return None if a is None else torch.tensor(a, device=DEV)


def combine(t, shape, s_i, s_t, swap=False):
    """(m, |m| bound terms) of the three-branch combine in float64; swap: the middle and unconditional outputs exchanged."""
    u, m, c = (nchw(t[k], shape) for k in (("m", "u", "c") if swap else ("u", "m", "c")))
    return u + s_i * (m - u) + s_t * (c - m), np.abs(u) + abs(s_i) * (np.abs(m) + np.abs(u)) + abs(s_t) * (np.abs(c) + np.abs(m))


def same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


# ------------------------------------------------------------------------------------------------ the eps entry
def eps_scalars(sigma):
    a_t, a_prev = f32(0.3), f32(0.5)
    return tuple(float(v) for v in (np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_prev), np.sqrt(1 - a_prev - f32(sigma) ** 2), f32(sigma)))


def eps_launch(ops, t, shape, pred, order, sigma, phi, s_t, mid=None, s_i=None, alias=None, separate_xm=True):
    """One launch on fresh tensors.  mid: None = the two-branch entry (ops.sampler_step_rescale); "m" | "u" | "c" = the dual
    entry with that output as out_m ("u" / "c": the SAME tensor as out_u / out_c).  alias: "x" | "xm": x_prev IS that input."""
    d = {k: dev(v) for k, v in t.items()}
    x, xm = d["x"], d["xm"] if separate_xm else None
    olds = [d[k] for k in ("o1", "o2", "o3")][:order]
    e, p, fac = torch.empty_like(x), torch.empty_like(x), torch.full((shape[0],), -7., device=DEV)
    x_prev = {None: torch.empty_like(x), "x": x, "xm": xm}[alias]
    common = (pred, AM, SM, olds, COEF[order], *eps_scalars(sigma), d["noise"] if sigma else None, e, x_prev, p)
    if mid is None:
        ops.sampler_step_rescale(x, xm, d["u"], d["c"], LD, s_t, *common, phi, fac)
    else:
        ops.sampler_step_dual(x, xm, d["u"], d[mid], d["c"], LD, s_t, s_i, *common, guidance_rescale=phi, factor_out=fac)
    torch.cuda.synchronize()
    return dict(x_prev=x_prev, pred_x0=p, e_t=e, fac=fac)


def eps_reference(t, shape, pred, order, sigma, phi, s_i, s_t, swap=False):
    f64 = np.float64
    m, _ = combine(t, shape, s_i, s_t, swap)
    f = R.rescale_factor(nchw(t["c"], shape), m, phi) if phi else np.ones(shape[0])
    m = f.reshape(-1, 1, 1, 1) * m
    e_t = AM * m + SM * t["xm"].astype(f64) if pred == V else m
    coef = COEF[order]
    ep = coef[0] * e_t + sum(c * t[k].astype(f64) for c, k in zip(coef[1:], ("o1", "o2", "o3")[:order]))
    s_at, s_1mat, s_ap, dirc, sg = eps_scalars(sigma)
    px0 = (t["x"].astype(f64) - s_1mat * ep) / s_at
    return dict(x_prev=s_ap * px0 + dirc * ep + sg * t["noise"].astype(f64), pred_x0=px0, e_t=e_t, fac=f)


EPS_FORMS = [(pred, order, sigma) for pred in (EPS, V) for order in (0, 1, 3) for sigma in (0., 0.4)]


@pytest.mark.parametrize("phi", [0., 0.7], ids=["spread", "owned"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_eps_entry_against_float64(ops, shape, phi):
    t = inputs(shape, seed=shape[2] + 3)
    for n, (pred, order, sigma) in enumerate(EPS_FORMS):
        s_i, s_t = SCALES[n == 5]
        got = eps_launch(ops, t, shape, pred, order, sigma, phi, s_t, "m", s_i)
        ref = eps_reference(t, shape, pred, order, sigma, phi, s_i, s_t)
        tag = f"dual_eps_{shape}_p{pred}_o{order}_s{sigma}_phi{phi}"
        fg = got["fac"].cpu().numpy().astype(np.float64)
        print("FACTOR", tag, fg.tolist(), ref["fac"].tolist())
        if phi:
            assert np.all(np.abs(fg - ref["fac"]) <= 1e-5 * np.abs(ref["fac"])), (tag, fg, ref["fac"])
            assert np.ptp(ref["fac"]) > 0                   # a sample mix-up shows
        else:
            assert np.array_equal(fg, np.ones(shape[0]))
        for k in ("x_prev", "pred_x0", "e_t"):
            check(f"{tag}_{k}", got[k], ref[k], rel_l2=1e-5)
        # the test tells the branches apart: with the middle and the unconditional output exchanged the reference is far off
        swapped = eps_reference(t, shape, pred, order, sigma, phi, s_i, s_t, swap=True)
        assert metrics(got["x_prev"], swapped["x_prev"])["rel_l2"] > 1e-2


@pytest.mark.parametrize("phi", [0., 0.7], ids=["spread", "owned"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_eps_entry_alias_identities(ops, shape, phi):
    t = inputs(shape, seed=shape[3] + 11)
    s_i, s_t = SCALES[0]
    for pred, order, sigma in EPS_FORMS:
        what = f"{shape} p{pred} o{order} s{sigma} phi{phi}"
        same(eps_launch(ops, t, shape, pred, order, sigma, phi, s_t, "u", s_i),
             eps_launch(ops, t, shape, pred, order, sigma, phi, s_t), what + " out_m = out_u")
        same(eps_launch(ops, t, shape, pred, order, sigma, phi, s_t, "c", s_i),
             eps_launch(ops, t, shape, pred, order, sigma, phi, s_i), what + " out_m = out_c")


@pytest.mark.parametrize("phi", [0., 0.7], ids=["spread", "owned"])
def test_eps_entry_x_prev_may_be_x_or_x_model(ops, phi):
    shape = SHAPES[3]
    t = inputs(shape, seed=5)
    s_i, s_t = SCALES[0]
    plain = eps_launch(ops, t, shape, V, 3, 0.4, phi, s_t, "m", s_i)
    for alias in ("x", "xm"):
        same(plain, eps_launch(ops, t, shape, V, 3, 0.4, phi, s_t, "m", s_i, alias=alias), f"x_prev is {alias}")


def test_eps_entry_without_out_m_is_the_two_branch_entry(ops):
    shape = SHAPES[2]
    t = inputs(shape, seed=6)
    d = {k: dev(v) for k, v in t.items()}
    for phi in (0., 0.7):
        outs = []
        for dual in (False, True):
            e, p, xp = (torch.empty_like(d["x"]) for _ in range(3))
            fac = torch.full((shape[0],), -7., device=DEV)
            common = (V, AM, SM, [d["o1"]], COEF[1], *eps_scalars(0.), None, e, xp, p)
            if dual:
                ops.sampler_step_dual(d["x"], d["xm"], d["u"], None, d["c"], LD, 7.5, float("nan"), *common,
                                      guidance_rescale=phi, factor_out=fac)
            else:
                ops.sampler_step_rescale(d["x"], d["xm"], d["u"], d["c"], LD, 7.5, *common, phi, fac)
            outs.append(dict(e=e, p=p, xp=xp, fac=fac))
        same(outs[0], outs[1], f"out_m None, phi {phi}")


# ------------------------------------------------------------------------------------------------ the lin entry
LIN_C = tuple(float(f32(v)) for v in (0.4, 0.1, -0.2))
LIN_A, CN, MAX_VAL, DRAW = float(f32(0.8)), float(f32(0.37)), 0.5, 3
SEEDS = [11, 2 ** 40 + 5, -3]


def lin_launch(ops, t, shape, pred, value, noise, phi, thr, s_t, mid=None, s_i=None, alias=None):
    """noise: None | "tensor" | "seeded".  mid as in eps_launch (None: ops.sampler_step_lin_noise).  alias: "x_base" | "x_model"."""
    B = shape[0]
    d = {k: dev(v) for k, v in t.items()}
    x_base, x_model = d["x"], d["xm"]
    model_out, pre = torch.empty_like(x_base), torch.empty_like(x_base)
    thr_out, fac = torch.full((B,), -7., device=DEV), torch.full((B,), -7., device=DEV)
    x_out = {None: torch.empty_like(x_base), "x_base": x_base, "x_model": x_model}[alias]
    seeds = ops.seeds_tensor(SEEDS[:B], DEV)
    nz = dict(noise=d["noise"] if noise == "tensor" else None, seeds=seeds if noise == "seeded" else None, draw=DRAW)
    if noise == "seeded_as_tensor":                        # the generator's bits, handed over as a tensor
        nz = dict(noise=ops.randn_seeded(seeds, ops.RNG_STEP, DRAW, tuple(shape[1:])), seeds=None, draw=DRAW)
    tail = (pred, phi, value, AM, SM, d["h1"], d["h2"], LIN_A, *LIN_C, model_out, x_out, CN if noise else 0.)
    kw = dict(thresholding=thr, max_val=MAX_VAL, model_pre_out=pre, thr_out=thr_out, factor_out=fac, **nz)
    if mid is None:
        ops.sampler_step_lin_noise(x_base, x_model, d["u"], d["c"], s_t, *tail, **kw)
    else:
        ops.sampler_step_lin_dual(x_base, x_model, d["u"], d[mid], d["c"], s_t, s_i, *tail, **kw)
    torch.cuda.synchronize()
    return dict(model_out=model_out, pre=pre, x_out=x_out, thr=thr_out, fac=fac)


def within(name, got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{name}: worst error / bound = {worst:.4f}")
    assert np.all(err <= bound), f"{name}: {int((err > bound).sum())} elements beyond the bound, worst {worst:.3f} x"


def lin_check(ops, name, t, shape, pred, value, noise, phi, thr, s_i, s_t, got, swap=False):
    """The float64 statement of steps 1-8 with its bound; returns the worst error / bound of x_out (swap: nothing asserted)."""
    g = {k: v.cpu().numpy() for k, v in got.items()}
    m, mag = combine(t, shape, s_i, s_t, swap)
    if phi and not swap:
        f64 = R.rescale_factor(nchw(t["c"], shape), m, phi)
        assert np.all(np.abs(g["fac"] - f64) <= 1e-5 * np.abs(f64)), (name, g["fac"], f64)
    elif not phi:
        assert np.array_equal(g["fac"], np.ones(shape[0], f32))
    fb = g["fac"].astype(np.float64).reshape(-1, 1, 1, 1)       # the launch's own factor, held to the formula above
    m, mag = m * fb, mag * np.abs(fb)
    xm = t["xm"].astype(np.float64)
    if pred == V:
        m, mag = AM * m + SM * xm, AM * mag + SM * np.abs(xm)
    if value == X0:
        m, mag = (xm - SM * m) / AM, (np.abs(xm) + SM * mag) / AM
    z = 0.
    if noise == "tensor":
        z = t["noise"].astype(np.float64)
    elif noise == "seeded":
        z = ops.randn_seeded(ops.seeds_tensor(SEEDS[:shape[0]], DEV), ops.RNG_STEP, DRAW, tuple(shape[1:])).cpu().numpy().astype(np.float64)
    cn = CN if noise else 0.
    rest = LIN_A * t["x"].astype(np.float64) + LIN_C[1] * t["h1"].astype(np.float64) + LIN_C[2] * t["h2"].astype(np.float64) + cn * z
    rmag = LIN_A * np.abs(t["x"]) + abs(LIN_C[1]) * np.abs(t["h1"]) + abs(LIN_C[2]) * np.abs(t["h2"]) + abs(cn) * np.abs(z)
    if swap:
        return float(np.max(np.abs(g["x_out"] - (LIN_C[0] * m + rest)) / (ULP * (LIN_C[0] * mag + rmag))))
    within(f"{name} pre", g["pre"], m, ULP * mag)
    if thr:
        N = int(np.prod(shape[1:]))
        k = int((N - 1) * 0.995)
        for b in range(shape[0]):
            srt = np.sort(np.abs(g["pre"][b]).ravel())
            s = f32(srt[k] + f32(f32(srt[k + 1] - srt[k]) * f32(0.995)))
            s = max(s, f32(MAX_VAL))
            assert g["thr"][b] == s, (name, b, g["thr"][b], s)
            assert np.array_equal(g["model_out"][b], (np.clip(g["pre"][b], -s, s) / s).astype(f32)), (name, b)
        val, vmag = g["model_out"].astype(np.float64), np.abs(g["model_out"])
    else:
        assert np.array_equal(g["thr"], np.full(shape[0], -7., f32))
        assert np.array_equal(g["pre"].view(np.uint32), g["model_out"].view(np.uint32))
        val, vmag = m, mag
    within(f"{name} x_out", g["x_out"], LIN_C[0] * val + rest, ULP * (LIN_C[0] * vmag + rmag))
    return 0.


LIN_FORMS = [(pred, value, noise, thr) for pred in (EPS, V) for value in (X0, NOISE) for noise in (None, "tensor", "seeded")
             for thr in ((False, True) if value == X0 else (False,))]


@pytest.mark.parametrize("phi", [0., 0.7], ids=["phi0", "phi0.7"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_lin_entry_against_float64(ops, shape, phi):
    t = inputs(shape, seed=shape[2] + 17)
    for n, (pred, value, noise, thr) in enumerate(LIN_FORMS):
        s_i, s_t = SCALES[n == 7]
        name = f"dual_lin_{shape}_p{pred}_v{value}_{noise}_phi{phi}_thr{int(thr)}"
        got = lin_launch(ops, t, shape, pred, value, noise, phi, thr, s_t, "m", s_i)
        lin_check(ops, name, t, shape, pred, value, noise, phi, thr, s_i, s_t, got)
        if not thr:     # branch order: against the reference with the middle and unconditional outputs exchanged it is far out
            assert lin_check(ops, name, t, shape, pred, value, noise, phi, thr, s_i, s_t, got, swap=True) > 100.


@pytest.mark.parametrize("phi", [0., 0.7], ids=["phi0", "phi0.7"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_lin_entry_alias_identities(ops, shape, phi):
    t = inputs(shape, seed=shape[3] + 23)
    s_i, s_t = SCALES[0]
    for pred, value, noise, thr in LIN_FORMS:
        what = f"{shape} p{pred} v{value} {noise} phi{phi} thr{int(thr)}"
        same(lin_launch(ops, t, shape, pred, value, noise, phi, thr, s_t, "u", s_i),
             lin_launch(ops, t, shape, pred, value, noise, phi, thr, s_t), what + " out_m = out_u")
        same(lin_launch(ops, t, shape, pred, value, noise, phi, thr, s_t, "c", s_i),
             lin_launch(ops, t, shape, pred, value, noise, phi, thr, s_i), what + " out_m = out_c")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_lin_entry_forms_agree(ops, shape):
    t = inputs(shape, seed=shape[2] + 29)
    s_i, s_t = SCALES[0]
    for pred, value, phi, thr in [(EPS, X0, 0., False), (V, X0, 0.7, False), (V, X0, 0., True), (EPS, NOISE, 0.7, False),
                                  (EPS, X0, 0.7, True)]:
        # the generator's bits: drawn in the launch, or handed over as a tensor
        same(lin_launch(ops, t, shape, pred, value, "seeded", phi, thr, s_t, "m", s_i),
             lin_launch(ops, t, shape, pred, value, "seeded_as_tensor", phi, thr, s_t, "m", s_i),
             f"{shape} p{pred} v{value} phi{phi} thr{int(thr)}: seeded against tensor noise")
    # OWNED with phi == 0 (thresholding on) against SPREAD, where lin_value has one spelling: eps prediction
    for noise in (None, "tensor", "seeded"):
        owned = lin_launch(ops, t, shape, EPS, X0, noise, 0., True, s_t, "m", s_i)
        spread = lin_launch(ops, t, shape, EPS, X0, noise, 0., False, s_t, "m", s_i)
        assert torch.equal(owned["pre"], spread["model_out"]), f"{shape} {noise}: owned and spread values differ"
        assert torch.equal(owned["fac"], spread["fac"])


@pytest.mark.parametrize("alias", ["x_base", "x_model"])
def test_lin_entry_x_out_may_be_an_input(ops, alias):
    shape = SHAPES[3]
    t = inputs(shape, seed=31)
    s_i, s_t = SCALES[0]
    for noise, phi, thr in [(None, 0., False), ("seeded", 0., False), ("tensor", 0.7, False), ("seeded", 0.7, True)]:
        same(lin_launch(ops, t, shape, V, X0, noise, phi, thr, s_t, "m", s_i),
             lin_launch(ops, t, shape, V, X0, noise, phi, thr, s_t, "m", s_i, alias=alias), f"{noise} phi{phi} thr{thr} x_out is {alias}")


# ------------------------------------------------------------------------------------------------ refusals
def _eps_args(shape):
    t = {k: dev(v) for k, v in inputs(shape, seed=1).items()}
    outs = {k: torch.empty_like(t["x"]) for k in ("e", "xp", "p")}
    return t, outs


def _eps_call(ops, t, outs, u="u", m="m", s_i=1.5, phi=0., fac=None, **over):
    o = dict(outs, **over)
    ops.sampler_step_dual(t["x"], t["xm"], None if u is None else t[u], m if isinstance(m, torch.Tensor) else t[m], t["c"], LD, 7.5,
                          s_i, EPS, 1., 0., [], COEF[0], *eps_scalars(0.), None, o["e"], o["xp"], o["p"], guidance_rescale=phi,
                          factor_out=fac)


def _lin_call(ops, t, u="u", m="m", s_i=1.5, **over):
    o = {k: torch.empty_like(t["x"]) for k in ("model_out", "x_out", "pre")}
    o.update(thr=torch.empty(t["x"].shape[0], device=DEV), fac=torch.empty(t["x"].shape[0], device=DEV))
    o.update(over)
    ops.sampler_step_lin_dual(t["x"], t["xm"], None if u is None else t[u], m if isinstance(m, torch.Tensor) else t[m], t["c"], 7.5,
                              s_i, EPS, 0., X0, AM, SM, None, None, LIN_A, 0.5, 0., 0., o["model_out"], o["x_out"],
                              thresholding=True, max_val=1., model_pre_out=o["pre"], thr_out=o["thr"], factor_out=o["fac"])


def _overlapping(shape):
    """An fp16 out_m and an fp32 [B, C, H, W] tensor and a [B] fp32 tensor on the same bytes."""
    B, C, H, W = shape
    n = max(B * H * W * LD * 2, B * C * H * W * 4)
    buf = torch.zeros(n, dtype=torch.uint8, device=DEV)
    out_m = buf[:B * H * W * LD * 2].view(torch.float16).view(B, H * W, LD)
    return out_m, buf[:B * C * H * W * 4].view(torch.float32).view(shape), buf[:B * 4].view(torch.float32)


def test_refusals_name_what_they_refuse(ops):
    from minddiffusion_amd._lib import MdxError
    shape = SHAPES[2]
    t, outs = _eps_args(shape)
    with pytest.raises(MdxError, match="mdx_sampler_step_dual_f32: out_m without out_u"):
        _eps_call(ops, t, outs, u=None)
    with pytest.raises(MdxError, match="mdx_sampler_step_lin_dual_f32: out_m without out_u"):
        _lin_call(ops, t, u=None)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(MdxError, match="mdx_sampler_step_dual_f32: mid_scale .* is not finite"):
            _eps_call(ops, t, outs, s_i=bad)
        with pytest.raises(MdxError, match="mdx_sampler_step_lin_dual_f32: mid_scale .* is not finite"):
            _lin_call(ops, t, s_i=bad)
    out_m, over32, overB = _overlapping(shape)
    for key, name in (("e", "e_t_out"), ("xp", "x_prev"), ("p", "pred_x0")):
        with pytest.raises(MdxError, match=f"mdx_sampler_step_dual_f32: {name} overlaps out_m"):
            _eps_call(ops, t, outs, m=out_m, **{key: over32})
    with pytest.raises(MdxError, match="mdx_sampler_step_dual_f32: factor_out overlaps out_m"):
        _eps_call(ops, t, outs, m=out_m, phi=0.7, fac=overB)
    for key, name in (("model_out", "model_out"), ("x_out", "x_out"), ("pre", "model_pre_out")):
        with pytest.raises(MdxError, match=f"mdx_sampler_step_lin_dual_f32: {name} overlaps out_m"):
            _lin_call(ops, t, m=out_m, **{key: over32})
    for key, name in (("thr", "thr_out"), ("fac", "factor_out")):
        with pytest.raises(MdxError, match=f"mdx_sampler_step_lin_dual_f32: {name} overlaps out_m"):
            _lin_call(ops, t, m=out_m, **{key: overB})
    # the wrappers' own checks: out_m has out_c's dtype, shape and ld, and comes with a scale
    with pytest.raises(MdxError, match="out_m"):
        _eps_call(ops, t, outs, m=t["m"].to(torch.float32))
    with pytest.raises(MdxError, match="out_m: expected out_c's shape"):
        _lin_call(ops, t, m=t["m"][:, :-1].contiguous())
    with pytest.raises(MdxError, match="out_m needs a mid_scale"):
        _eps_call(ops, t, outs, s_i=None)
    torch.cuda.synchronize()
