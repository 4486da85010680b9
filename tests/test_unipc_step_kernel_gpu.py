"""ops.sampler_step_pc (mdx_sampler_step_pc_f32): the model value of one evaluation, the corrected latent
xc = Ac x_base + d0 val + d1 h1 + d2 h2 + d3 h3 and the predicted latent xp = Ap xc + e0 val + e1 h1 + e2 h2, in both launch forms.

Reference and bound, as tests/test_dpm_step_kernel_gpu.py derives them: float64 numpy on the very fp16 model outputs and the
float32-rounded scalars the launch gets; per element 32 * 2^-24 times the sum of the magnitudes of all terms as they enter.  The
count of roundings is at most 25 here (value 10: combine 3, rescale 1, v -> eps 3, data prediction 3; corrector 6: two products,
one sum, three fused terms; predictor 5: two products, one sum, two fused terms; the stored xc is one of them), each at most
2^-24 of a partial result no larger than that sum.  For x_pred_out the magnitude of xc is the corrector's sum times |Ap|.

Where the launch overlaps mdx_sampler_step_lin_f32 -- corrector off, or d3 == 0 -- it is held to that entry's bits."""
import ctypes

import numpy as np
import pytest
import torch

import _guard as G
import test_dpm_step_kernel_gpu as K

pytestmark = pytest.mark.gpu
DEV, f32 = K.DEV, np.float32
EPS, V, X0, NOISE, ULP, SHAPES, LD, AM, SM = K.EPS, K.V, K.X0, K.NOISE, K.ULP, K.SHAPES, K.LD, K.AM, K.SM
HIST = ("h1", "h2", "h3")
r32 = lambda vs: tuple(float(f32(v)) for v in vs)
CORR = r32((0.93, 0.41, -0.27, 0.09, -0.031))         # Ac, d0, d1, d2, d3
PRED = r32((0.88, 0.35, -0.19, 0.044))                # Ap, e0, e1, e2


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops
    return ops


def inputs(shape, seed):
    t = K.inputs(shape, seed)
    t["h3"] = np.random.RandomState(seed + 1000).randn(*shape).astype(f32)
    return t


def coefficients(n_hist, corrector=True):
    """(corrector | None, predictor) reading n_hist histories: the coefficients beyond are exactly 0."""
    corr = tuple(v if j < 2 + n_hist else 0. for j, v in enumerate(CORR)) if corrector else None
    pred = tuple(v if j < 2 + min(n_hist, 2) else 0. for j, v in enumerate(PRED))
    return corr, pred


def reference(t, shape, pred, value, with_u, cfg, corr, predc, f):
    """model value, corrected and predicted latent with their bounds, float64."""
    val, vb, _, _ = K.reference(t, shape, pred, value, with_u, cfg, AM, SM, 0., (1., 0., 0.), f, "x_model")
    mag = vb / ULP
    h = [t[k].astype(np.float64) for k in HIST]
    if corr is None:
        xc, cmag = t["x_model"].astype(np.float64), np.abs(t["x_model"]).astype(np.float64)
    else:
        xb = t["x_base"].astype(np.float64)
        xc = corr[0] * xb + corr[1] * val + sum(d * hh for d, hh in zip(corr[2:], h))
        cmag = abs(corr[0]) * np.abs(xb) + abs(corr[1]) * mag + sum(abs(d) * np.abs(hh) for d, hh in zip(corr[2:], h))
    xp = predc[0] * xc + predc[1] * val + sum(e * hh for e, hh in zip(predc[2:], h))
    pmag = abs(predc[0]) * cmag + abs(predc[1]) * mag + sum(abs(e) * np.abs(hh) for e, hh in zip(predc[2:], h))
    return val, vb, xc, ULP * cmag, xp, ULP * pmag


def launch(ops, t, shape, pred, value, with_u, cfg, corr, predc, phi=0., thresholding=False, max_val=1., alias=False,
           nan_skipped=False):
    """One launch on fresh device tensors; the outputs as numpy.  alias: x_corr_out IS x_base and x_pred_out IS x_model.
    nan_skipped: every input whose term is skipped points to NaN-filled memory."""
    B = shape[0]
    d = {k: torch.tensor(v, device=DEV) for k, v in t.items()}
    nan = torch.full(shape, float("nan"), device=DEV)
    used = [(corr is not None and corr[2 + j] != 0.) or (j < 2 and predc[2 + j] != 0.) for j in range(3)]
    hist = [d[k] if u else (nan if nan_skipped else None) for k, u in zip(HIST, used)]
    x_base = d["x_base"] if corr is not None and corr[0] != 0. else (nan.clone() if nan_skipped else None)
    if alias and x_base is None:
        x_base = torch.empty(shape, device=DEV)
    x_model = d["x_model"].clone()
    model_out, pre = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
    thr, fac = torch.full((B,), -7., device=DEV), torch.full((B,), -7., device=DEV)
    xc = x_base if alias else torch.empty(shape, device=DEV)
    xp = x_model if alias else torch.empty(shape, device=DEV)
    ops.sampler_step_pc(x_base, x_model, d["out_u"] if with_u else None, d["out_c"], cfg, pred, phi, value, AM, SM, *hist, corr,
                        predc, model_out, xc, xp, thresholding=thresholding, max_val=max_val, model_pre_out=pre, thr_out=thr,
                        factor_out=fac)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(model_out=model_out, pre=pre, xc=xc, xp=xp, thr=thr, fac=fac).items()}


def lin(ops, t, shape, pred, value, with_u, cfg, x_base_key, A, c, phi=0., thresholding=False, max_val=1.):
    """ops.sampler_step_lin on the same inputs, x_model = t["x_model"]."""
    B = shape[0]
    d = {k: torch.tensor(v, device=DEV) for k, v in t.items()}
    model_out, pre, x_out = (torch.empty(shape, device=DEV) for _ in range(3))
    thr, fac = torch.full((B,), -7., device=DEV), torch.full((B,), -7., device=DEV)
    ops.sampler_step_lin(d[x_base_key], d["x_model"], d["out_u"] if with_u else None, d["out_c"], cfg, pred, phi, value, AM, SM,
                         d["h1"] if c[1] != 0. else None, d["h2"] if c[2] != 0. else None, A, c[0], c[1], c[2], model_out, x_out,
                         thresholding=thresholding, max_val=max_val, model_pre_out=pre, thr_out=thr, factor_out=fac)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(model_out=model_out, pre=pre, x_out=x_out, thr=thr, fac=fac).items()}


def same_bits(a, b, what):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


# name -> (pred, value, with_u, guidance scale, histories read, corrector, phi)
CASES = {
    "eps_x0_nou_h0_first": (EPS, X0, False, 1.0, 0, False, 0.),
    "eps_x0_u_h1": (EPS, X0, True, 7.5, 1, True, 0.),
    "v_x0_u_h2": (V, X0, True, 3.0, 2, True, 0.),
    "v_x0_u_h3": (V, X0, True, 3.0, 3, True, 0.),
    "eps_eps_nou_h3": (EPS, NOISE, False, 1.0, 3, True, 0.),
    "v_eps_u_h2": (V, NOISE, True, 4.0, 2, True, 0.),
    "eps_eps_u_h2_nocorr": (EPS, NOISE, True, 5.0, 2, False, 0.),
    "v_x0_nou_h0": (V, X0, False, 1.0, 0, True, 0.),
    "eps_x0_u_h3_rescale_half": (EPS, X0, True, 7.5, 3, True, 0.5),
    "v_eps_u_h3_rescale_one": (V, NOISE, True, 4.0, 3, True, 1.0),
    "v_x0_u_h1_rescale_half_nocorr": (V, X0, True, 4.0, 1, False, 0.5),
    "eps_eps_u_h0_rescale_one": (EPS, NOISE, True, 3.0, 0, True, 1.0),
}


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("case", sorted(CASES))
def test_value_corrector_and_predictor(ops, shape, case):
    import _rescale_util as R
    pred, value, with_u, cfg, n_hist, corrector, phi = CASES[case]
    cfg = float(f32(cfg))
    corr, predc = coefficients(n_hist, corrector)
    t = inputs(shape, seed=len(case) + shape[2])
    got = launch(ops, t, shape, pred, value, with_u, cfg, corr, predc, phi=phi)
    if phi:
        oc, ou = K.nchw(t["out_c"], shape), K.nchw(t["out_u"], shape)
        f64 = R.rescale_factor(oc, ou + cfg * (oc - ou), phi)
        assert np.all(np.abs(got["fac"] - f64) <= 1e-5 * np.abs(f64)), (got["fac"], f64)
    else:
        assert np.array_equal(got["fac"], np.ones(shape[0], f32))
    val, vb, xc, cb, xp, pb = reference(t, shape, pred, value, with_u, cfg, corr, predc, got["fac"])
    K.within(f"{case} {shape} model_out", got["model_out"], val, vb)
    if corr is None:
        same_bits(got["xc"], t["x_model"], "x_corr_out without a corrector")
    else:
        K.within(f"{case} {shape} x_corr_out", got["xc"], xc, cb)
    K.within(f"{case} {shape} x_pred_out", got["xp"], xp, pb)
    same_bits(got["pre"], got["model_out"], "model_pre_out")
    assert np.array_equal(got["thr"], np.full(shape[0], -7., f32))       # written with thresholding only


FORMS = {"spread": {}, "rescale": dict(phi=0.7), "threshold_0.4": dict(thresholding=True, max_val=0.4),
         "threshold_100": dict(thresholding=True, max_val=100.), "rescale_threshold": dict(phi=0.7, thresholding=True, max_val=0.4)}


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("pred", [EPS, V])
def test_bits_of_the_lin_launch(ops, shape, form, pred):
    """Corrector off: the lin launch on (x_model, Ap, e).  Corrector on with d3 == 0: the lin launch on (x_base, Ac, d0 .. d2)."""
    kw, cfg = FORMS[form], float(f32(5.0))
    t = inputs(shape, seed=31 + shape[3])
    _, predc = coefficients(2)
    off = launch(ops, t, shape, pred, X0, True, cfg, None, predc, **kw)
    ref = lin(ops, t, shape, pred, X0, True, cfg, "x_model", predc[0], predc[1:], **kw)
    same_bits(off["xc"], t["x_model"], "x_corr_out")
    for k, r in (("model_out", "model_out"), ("pre", "pre"), ("thr", "thr"), ("fac", "fac"), ("xp", "x_out")):
        same_bits(off[k], ref[r], f"corrector off, {k}")
    corr, _ = coefficients(2)
    assert corr[4] == 0. and corr[3] != 0.
    on = launch(ops, t, shape, pred, X0, True, cfg, corr, predc, **kw)
    ref = lin(ops, t, shape, pred, X0, True, cfg, "x_base", corr[0], corr[1:4], **kw)
    for k, r in (("model_out", "model_out"), ("pre", "pre"), ("thr", "thr"), ("fac", "fac"), ("xc", "x_out")):
        same_bits(on[k], ref[r], f"corrector on, {k}")
    if "thresholding" in kw:
        assert np.all(on["thr"] > f32(0.4)) if kw["max_val"] == 0.4 else np.all(on["thr"] == f32(100.))
    # the noise form has no thresholding; spread and rescale still overlap the lin launch
    if "thresholding" not in kw:
        off = launch(ops, t, shape, pred, NOISE, True, cfg, None, predc, **kw)
        ref = lin(ops, t, shape, pred, NOISE, True, cfg, "x_model", predc[0], predc[1:], **kw)
        for k, r in (("model_out", "model_out"), ("fac", "fac"), ("xp", "x_out")):
            same_bits(off[k], ref[r], f"noise form, corrector off, {k}")


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("corrector", [True, False])
def test_both_aliases_together(ops, form, corrector):
    """x_corr_out = x_base and x_pred_out = x_model in one launch: the bits of the launch with outputs of their own."""
    shape, kw = SHAPES[1], FORMS[form]
    t = inputs(shape, seed=5)
    corr, predc = coefficients(3, corrector)
    plain = launch(ops, t, shape, V, X0, True, 3.0, corr, predc, **kw)
    aliased = launch(ops, t, shape, V, X0, True, 3.0, corr, predc, alias=True, **kw)
    for k in ("xc", "xp", "model_out", "pre", "fac", "thr"):
        same_bits(plain[k], aliased[k], k)


@pytest.mark.parametrize("form", ["spread", "rescale", "threshold_0.4"])
@pytest.mark.parametrize("n_hist,corrector", [(0, True), (1, True), (2, True), (2, False), (0, False)])
def test_a_zero_coefficient_skips_its_tensor(ops, form, n_hist, corrector):
    shape, kw = SHAPES[0], FORMS[form]
    t = inputs(shape, seed=9)
    corr, predc = coefficients(n_hist, corrector)
    plain = launch(ops, t, shape, EPS, X0, True, 3.0, corr, predc, **kw)
    skipped = launch(ops, t, shape, EPS, X0, True, 3.0, corr, predc, nan_skipped=True, **kw)
    for k in ("xc", "xp", "model_out"):
        assert np.isfinite(skipped[k]).all(), k
        same_bits(plain[k], skipped[k], k)
    # Ac == 0 / Ap == 0 skip the latent they would scale (denoise_to_zero's record: the data prediction is the result)
    z = launch(ops, t, shape, EPS, X0, True, 3.0, (0.,) + CORR[1:], (0., 1., 0., 0.), nan_skipped=True, **kw)
    same_bits(z["xp"], z["model_out"], "Ap = 0, e0 = 1")
    assert np.isfinite(z["xc"]).all()


@pytest.mark.parametrize("form", ["spread", "rescale", "threshold_0.4"])
def test_a_row_of_a_batch_is_the_batch_1_launch(ops, form):
    shape, kw = SHAPES[0], FORMS[form]
    t = inputs(shape, seed=17)
    corr, predc = coefficients(3)
    batch = launch(ops, t, shape, V, X0, True, 3.0, corr, predc, **kw)
    for b in range(shape[0]):
        row = launch(ops, {k: v[b:b + 1] for k, v in t.items()}, (1,) + shape[1:], V, X0, True, 3.0, corr, predc, **kw)
        for k in ("xc", "xp", "model_out", "fac", "thr"):
            same_bits(batch[k][b:b + 1], row[k], (k, b))


@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
@pytest.mark.parametrize("form", ["spread", "rescale", "threshold_0.4"])
def test_only_the_outputs_are_written(ops, shape, form):
    B, kw = shape[0], FORMS[form]
    t = inputs(shape, seed=2)
    outs = {k: G.guarded(shape, torch.float32) for k in ("model_out", "xc", "xp", "pre")}
    small = {k: G.guarded((B,), torch.float32) for k in ("thr", "fac")}
    ins = {k: G.poisoned(t[k]) for k in ("x_base", "x_model") + HIST}
    halves = {k: G.poisoned(t[k]) for k in ("out_u", "out_c")}
    before = {k: v[0].clone() for k, v in {**ins, **halves}.items()}
    ops.sampler_step_pc(ins["x_base"][1], ins["x_model"][1], halves["out_u"][1], halves["out_c"][1], 3.0, V, kw.get("phi", 0.), X0,
                        AM, SM, ins["h1"][1], ins["h2"][1], ins["h3"][1], CORR, PRED, outs["model_out"][1], outs["xc"][1],
                        outs["xp"][1], thresholding="thresholding" in kw, max_val=0.4, model_pre_out=outs["pre"][1],
                        thr_out=small["thr"][1], factor_out=small["fac"][1])
    for k, (buf, view) in outs.items():
        G.assert_footprint(buf, view, f"{form} {k}", written=True)
        assert torch.isfinite(view).all(), k
    G.assert_footprint(*small["fac"], f"{form} factor_out", written=True)
    if "thresholding" in kw:
        G.assert_footprint(*small["thr"], f"{form} thr_out", written=True)
    else:
        assert bool((small["thr"][0] == G.SENT).all())
    for k, (buf, _) in {**ins, **halves}.items():          # inputs: untouched, bit for bit
        kind = torch.int32 if buf.dtype == torch.float32 else torch.int16
        assert torch.equal(buf.view(kind), before[k].view(kind)), k


def test_refusals(ops):
    from minddiffusion_amd._lib import MdxError
    shape = SHAPES[0]
    t = inputs(shape, seed=1)
    d = {k: torch.tensor(v, device=DEV) for k, v in t.items()}
    mo, xc, xp, pre = (torch.full(shape, 5., device=DEV) for _ in range(4))
    thr, fac = torch.full((3,), 5., device=DEV), torch.full((3,), 5., device=DEV)

    def call(match, **kw):
        a = dict(x_base=d["x_base"], x_model=d["x_model"], out_u=d["out_u"], out_c=d["out_c"], cfg_scale=3.0, pred_type=EPS,
                 guidance_rescale=0., value_type=X0, alpha_m=AM, sigma_m=SM, h1=d["h1"], h2=d["h2"], h3=d["h3"], corrector=CORR,
                 predictor=PRED, model_out=mo, x_corr_out=xc, x_pred_out=xp, thresholding=False, max_val=1., model_pre_out=pre,
                 thr_out=thr, factor_out=fac)
        a.update(kw)
        with pytest.raises(MdxError, match=match):
            ops.sampler_step_pc(**a)

    # everything the lin entry refuses
    call("out_c, model_out and x_out are required", out_c=None)
    call("out_c, model_out and x_out are required", model_out=None)
    call("x_corr_out and x_pred_out are required", x_corr_out=None)
    call("x_corr_out and x_pred_out are required", x_pred_out=None)
    call("x_model is required", x_model=None)
    call("unknown pred_type", pred_type=2)
    call("unknown value_type", value_type=2)
    call("alpha_m == 0", alpha_m=0.)
    call("thresholding acts on a data prediction", thresholding=True, value_type=NOISE)
    for bad in (0., -1., float("inf"), float("nan")):
        call("max_val", thresholding=True, max_val=bad)
    for bad in (-0.1, 1.5, float("nan")):
        call("guidance_rescale", guidance_rescale=bad)
    # a coefficient without its history, in either form
    call("non-zero history coefficient", h1=None)
    call("non-zero history coefficient", h2=None)
    call("non-zero history coefficient", h3=None)
    call("non-zero history coefficient", h1=None, corrector=None)                        # e1 alone needs h1
    call("non-zero history coefficient", h2=None, predictor=PRED[:3] + (0.,))            # d2 alone needs h2
    call("has_corrector without x_base", x_base=None)
    # overlaps: only x_corr_out == x_base and x_pred_out == x_model pass
    call("x_corr_out overlaps x_pred_out", x_pred_out=xc)
    call("x_corr_out overlaps x_model", x_corr_out=d["x_model"])
    call("x_pred_out overlaps x_base", x_pred_out=d["x_base"])
    call("x_corr_out overlaps h3", x_corr_out=d["h3"])
    call("x_pred_out overlaps h1", x_pred_out=d["h1"])
    call("model_out overlaps h3", model_out=d["h3"])
    call("model_out overlaps x_base", model_out=d["x_base"])
    call("x_corr_out overlaps model_out", x_corr_out=mo)
    call("x_pred_out overlaps model_pre_out", model_pre_out=xp)
    call("x_pred_out overlaps out_c", x_pred_out=d["out_c"].view(torch.float32).reshape(-1)[:420].reshape(shape))
    flat = torch.zeros(421, device=DEV)
    call("x_corr_out overlaps x_base", x_base=flat[:420].reshape(shape), x_corr_out=flat[1:].reshape(shape))
    call("x_pred_out overlaps x_model", x_model=flat[:420].reshape(shape), x_pred_out=flat[1:].reshape(shape))
    # the wrapper's own checks: the library sees pointers only
    call("h3: expected", h3=d["h3"][:2])
    call("x_base: expected", x_base=d["x_base"][:2])
    call("x_pred_out: expected torch.float32", x_pred_out=xp.half())
    call("corrector is None or", corrector=CORR[:4])
    call("thr_out: needs 3 elements", thr_out=thr[:2])
    one = (2, 1, 1, 1)
    z = lambda: torch.zeros(one, device=DEV)
    h = torch.zeros((2, 1, LD), dtype=torch.float16, device=DEV)
    with pytest.raises(MdxError, match="two order statistics"):
        ops.sampler_step_pc(None, z(), None, h, 1., EPS, 0., X0, 1., 0.5, None, None, None, None, (1., 1., 0., 0.), z(), z(), z(),
                            thresholding=True)
    with pytest.raises(MdxError, match="per-sample std"):
        ops.sampler_step_pc(None, z(), h.clone(), h, 1., EPS, 0.5, X0, 1., 0.5, None, None, None, None, (1., 1., 0., 0.), z(), z(),
                            z())
    torch.cuda.synchronize()
    for o in (mo, xc, xp, pre, thr, fac):              # refused before any launch
        assert bool((o == 5.).all())
    # a skipped input is not read and may lie anywhere: model_out over an h3 with d3 == 0, no x_base without a corrector
    ops.sampler_step_pc(d["x_base"], d["x_model"], None, d["out_c"], 1., EPS, 0., X0, AM, SM, d["h1"], d["h2"], d["h3"],
                        CORR[:4] + (0.,), PRED, d["h3"], xc, xp)
    ops.sampler_step_pc(None, d["x_model"], None, d["out_c"], 1., EPS, 0., X0, AM, SM, None, None, None, None, (0.9, 0.3, 0., 0.),
                        mo, xc, xp)
    torch.cuda.synchronize()


def test_extents_are_refused_by_the_entry_itself():
    """With pointers it never dereferences: the refusal precedes any launch."""
    from minddiffusion_amd import _lib
    buf = torch.zeros(16, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    fn = _lib.load().mdx_sampler_step_pc_f32
    tail = lambda dims: (p, p, None, p, 8, 1., 0, 0., 0, 1., .5, 0, 1., None, None, None, 0, 0., 0., 0., 0., 0., 1., 1., 0., 0., p,
                         p, p, None, None, None, *dims, None)
    rc = fn(*tail((1, 4, 32768, 16384)))
    assert rc != 0
    with pytest.raises(_lib.MdxError, match="exceeds 31 bits"):
        _lib.check(rc, "mdx_sampler_step_pc_f32")
    for dims in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, -1, 8), (1, 4, 8, 0)):
        assert fn(*tail(dims)) != 0
    args = list(tail((1, 4, 2, 2)))
    args[4] = 3
    assert fn(*args) != 0       # out_ld < C
