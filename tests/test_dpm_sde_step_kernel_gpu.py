"""ops.sampler_step_lin_noise (mdx_sampler_step_lin_noise_f32): ops.sampler_step_lin's launch with step 8,
x_out = (A x_base + c0 val + c1 h1 + c2 h2) + cn z, z from a tensor or drawn inside the launch from per-sample seeds.

Cases, inputs, the float64 reference and the bound are tests/test_dpm_step_kernel_gpu.py's: 32 * 2^-24 times the sum of the
magnitudes of all terms as they enter, with |cn z| added as a term -- the count there is 17 roundings, step 8 adds two (the
product and the sum, one if fused), still under the 32.  Shapes: HW = 35 (a generator quad straddles two channels of the NHWC
model output), N = 105 (the last quad of a sample is partial), N = 4884 (a second trip of the one-workgroup-per-sample form)
and a latent-sized one.  Everything the seeded form promises is an equality of bits: with the tensor form fed
ops.randn_seeded's output, between a row of a batch and the B = 1 launch with its seed, and with ops.sampler_step_lin at cn = 0."""
import ctypes

import numpy as np
import pytest
import torch

import _guard as G
import _rescale_util as R
import test_dpm_step_kernel_gpu as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
SHAPES = [(3, 4, 5, 7), (2, 3, 5, 7), (2, 4, 33, 37), (1, 4, 64, 64)]
CN = float(f32(0.37))
DRAW = 5
SEEDS = [11, (1 << 63) + 5, -3]
FORMS = {"spread": ("v_x0_u_h2_xmodel", False), "rescale": ("v_x0_u_h2_xmodel_rescale", False),
         "threshold": ("eps_x0_u_h1", True), "rescale_threshold": ("v_x0_u_h2_xmodel_rescale", True)}
X0_CASES = sorted(k for k, v in K.CASES.items() if v[1] == K.X0)


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops
    return ops


def seeds_for(ops, B):
    return ops.seeds_tensor(SEEDS[:B], DEV)


def z_for(shape, seed=77):
    return np.random.RandomState(seed).randn(*shape).astype(f32)


def launch(ops, t, shape, case, cn=CN, noise=None, seeds=None, draw=DRAW, thresholding=False, max_val=0.5, alias=None,
           entry="noise"):
    """One launch on fresh device tensors, outputs as numpy.  noise: numpy / tensor or None; seeds: device tensor or None;
    alias: "x_base" | "x_model" -- x_out IS that input; entry "lin": ops.sampler_step_lin (no step 8)."""
    pred, value, with_u, cfg, A, c, phi, xmk = K.scalars(case)
    B = shape[0]
    d = {k: torch.tensor(v, device=DEV) for k, v in t.items()}
    x_base = d["x_base"].clone()
    x_model = d[xmk].clone() if xmk != "x_base" else None
    h1 = d["h1"] if c[1] != 0. else None
    h2 = d["h2"] if c[2] != 0. else None
    model_out, pre = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
    thr, fac = torch.full((B,), -7., device=DEV), torch.full((B,), -7., device=DEV)
    x_out = {None: torch.empty(shape, device=DEV), "x_base": x_base, "x_model": x_base if x_model is None else x_model}[alias]
    args = (x_base, x_model, d["out_u"] if with_u else None, d["out_c"], cfg, pred, phi, value, K.AM, K.SM, h1, h2, A, c[0], c[1],
            c[2], model_out, x_out)
    kw = dict(thresholding=thresholding, max_val=max_val, model_pre_out=pre, thr_out=thr, factor_out=fac)
    if entry == "lin":
        ops.sampler_step_lin(*args, **kw)
    else:
        if noise is not None and not isinstance(noise, torch.Tensor):
            noise = torch.tensor(noise, device=DEV)
        ops.sampler_step_lin_noise(*args, cn, noise=noise, seeds=seeds, stream=ops.RNG_STEP, draw=draw, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(model_out=model_out, pre=pre, x_out=x_out, thr=thr, fac=fac).items()}


def same_bits(a, b, keys=("x_out", "model_out", "pre", "thr", "fac")):
    for k in keys:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# ------------------------------------------------------------------------------------------------ tensor form vs float64
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("case", sorted(K.CASES))
def test_tensor_form_against_float64(ops, shape, case):
    pred, value, with_u, cfg, A, c, phi, xmk = K.scalars(case)
    t = K.inputs(shape, seed=len(case) + shape[2])
    z = z_for(shape)
    got = launch(ops, t, shape, case, noise=z)
    if phi:
        oc, ou = K.nchw(t["out_c"], shape), K.nchw(t["out_u"], shape)
        f64 = R.rescale_factor(oc, ou + cfg * (oc - ou), phi)
        assert np.all(np.abs(got["fac"] - f64) <= 1e-5 * np.abs(f64)), (got["fac"], f64)
    else:
        assert np.array_equal(got["fac"], np.ones(shape[0], f32))
    val, vb, x, xb = K.reference(t, shape, pred, value, with_u, cfg, K.AM, K.SM, A, c, got["fac"], xmk)
    K.within(f"{case} {shape} model_out", got["model_out"], val, vb)
    K.within(f"{case} {shape} x_out with noise", got["x_out"], x + CN * z.astype(np.float64), xb + K.ULP * np.abs(CN * z))
    # the noise is in: without the term the result is off by |cn z|, far beyond the bound
    assert np.abs(got["x_out"] - x).max() > 100 * xb.max()
    assert np.array_equal(got["pre"].view(np.uint32), got["model_out"].view(np.uint32))
    assert np.array_equal(got["thr"], np.full(shape[0], -7., f32))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("case", ["eps_x0_u_h1", "v_x0_u_h2_xmodel", "v_x0_u_h2_xmodel_rescale"])
def test_tensor_form_with_thresholding(ops, shape, case):
    """Step 8 in the finishing pass: the selection and the clamp exact on the launch's own model_pre_out (as the lin entry's
    test has it), the linear form with the noise within the bound."""
    pred, value, with_u, cfg, A, c, phi, xmk = K.scalars(case)
    t = K.inputs(shape, seed=21)
    z = z_for(shape)
    for max_val in (0.5, 50.0):
        got = launch(ops, t, shape, case, noise=z, thresholding=True, max_val=max_val)
        val, vb, _, _ = K.reference(t, shape, pred, value, with_u, cfg, K.AM, K.SM, A, c, got["fac"], xmk)
        K.within(f"{case} {shape} model_pre_out", got["pre"], val, vb)
        s, clipped, _, _ = K.numpy_threshold(got["pre"], max_val)
        assert np.array_equal(got["thr"].view(np.uint32), s.view(np.uint32))
        assert np.array_equal(got["model_out"].view(np.uint32), clipped.view(np.uint32))
        mo, d = got["model_out"].astype(np.float64), lambda k: t[k].astype(np.float64)
        x = c[0] * mo + A * d("x_base") + c[1] * d("h1") + c[2] * d("h2") + CN * z.astype(np.float64)
        xb = K.ULP * (abs(c[0]) * np.abs(mo) + abs(A) * np.abs(d("x_base")) + abs(c[1]) * np.abs(d("h1"))
                      + abs(c[2]) * np.abs(d("h2")) + np.abs(CN * z))
        K.within(f"{case} {shape} thresholded x_out with noise", got["x_out"], x, xb)


# ------------------------------------------------------------------------------------------------ the seeded form
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("case", sorted(K.CASES))
def test_seeded_form_is_the_tensor_form_on_randn_seeded(ops, shape, case):
    t = K.inputs(shape, seed=len(case) + shape[3])
    seeds = seeds_for(ops, shape[0])
    z = ops.randn_seeded(seeds, ops.RNG_STEP, DRAW, shape[1:])
    thresholds = (False, True) if case in X0_CASES else (False,)
    for thresholding in thresholds:
        tensor = launch(ops, t, shape, case, noise=z, thresholding=thresholding)
        seeded = launch(ops, t, shape, case, seeds=seeds, thresholding=thresholding)
        same_bits(tensor, seeded)
        other = launch(ops, t, shape, case, seeds=seeds, draw=DRAW + 1, thresholding=thresholding)
        assert not np.array_equal(other["x_out"], seeded["x_out"])        # the draw counter is read
        same_bits(other, seeded, keys=("model_out", "pre", "thr", "fac"))
    zn = z.cpu().numpy()
    assert abs(float(zn.mean())) < 0.2 and 0.8 < float(zn.std()) < 1.2


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("shape", SHAPES[:3], ids=str)
def test_cn_zero_is_the_lin_entry(ops, shape, form):
    """cn == 0 forwards: ops.sampler_step_lin's bits, with both sources given and both full of NaN patterns."""
    case, thresholding = FORMS[form]
    t = K.inputs(shape, seed=4)
    nan = torch.full(shape, float("nan"), device=DEV)
    nan_seeds = torch.full((shape[0],), float("nan"), device=DEV, dtype=torch.float64).view(torch.int64)
    plain = launch(ops, t, shape, case, thresholding=thresholding, entry="lin")
    zero = launch(ops, t, shape, case, cn=0., noise=nan, seeds=nan_seeds, thresholding=thresholding)
    assert np.isfinite(zero["x_out"]).all()
    same_bits(plain, zero, keys=("x_out", "model_out", "pre", "fac") + (("thr",) if thresholding else ()))
    neither = launch(ops, t, shape, case, cn=0., thresholding=thresholding)
    same_bits(plain, neither, keys=("x_out", "model_out"))


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("chw", [(4, 5, 7), (3, 5, 7), (4, 33, 37)], ids=str)
def test_a_row_does_not_depend_on_its_batch(ops, chw, form):
    """Row b of a B = 3 launch is the B = 1 launch with seeds[b], bit for bit (the rescale factor and the threshold are per
    sample, the noise is keyed by the sample's seed and counted from the sample's start)."""
    case, thresholding = FORMS[form]
    shape = (3,) + chw
    t = K.inputs(shape, seed=6)
    seeds = seeds_for(ops, 3)
    whole = launch(ops, t, shape, case, seeds=seeds, thresholding=thresholding)
    for b in range(3):
        row = launch(ops, {k: v[b:b + 1] for k, v in t.items()}, (1,) + chw, case, seeds=seeds[b:b + 1], thresholding=thresholding)
        for k in ("x_out", "model_out", "fac") + (("thr",) if thresholding else ()):
            assert np.array_equal(whole[k][b:b + 1].view(np.uint32), row[k].view(np.uint32)), (b, k)
    # the same inputs under another sample's seed give another row: the seed is read per sample
    swapped = launch(ops, {k: v[:1] for k, v in t.items()}, (1,) + chw, case, seeds=seeds[1:2], thresholding=thresholding)
    assert not np.array_equal(whole["x_out"][:1], swapped["x_out"])
    assert np.array_equal(whole["model_out"][:1].view(np.uint32), swapped["model_out"].view(np.uint32))


@pytest.mark.parametrize("alias", ["x_base", "x_model"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_x_out_may_be_an_input(ops, form, alias):
    case, thresholding = FORMS[form]
    shape = SHAPES[2]
    t = K.inputs(shape, seed=5)
    seeds = seeds_for(ops, shape[0])
    for src in (dict(seeds=seeds), dict(noise=z_for(shape))):
        plain = launch(ops, t, shape, case, thresholding=thresholding, **src)
        aliased = launch(ops, t, shape, case, thresholding=thresholding, alias=alias, **src)
        same_bits(plain, aliased, keys=("x_out", "model_out", "pre", "fac") + (("thr",) if thresholding else ()))


# ------------------------------------------------------------------------------------------------ footprint
@pytest.mark.parametrize("shape", SHAPES[:3], ids=str)
@pytest.mark.parametrize("source", ["noise", "seeds"])
@pytest.mark.parametrize("form", ["spread", "rescale", "threshold"])
def test_only_the_outputs_are_written(ops, shape, form, source):
    B, C, H, W = shape
    t = K.inputs(shape, seed=2)
    t["noise"] = z_for(shape)
    outs = {k: G.guarded(shape, torch.float32) for k in ("model_out", "x_out", "pre")}
    small = {k: G.guarded((B,), torch.float32) for k in ("thr", "fac")}
    ins = {k: G.poisoned(t[k]) for k in ("x_base", "x_model", "h1", "h2", "noise")}
    halves = {k: G.poisoned(t[k]) for k in ("out_u", "out_c")}
    before = {k: v[0].clone() for k, v in {**ins, **halves}.items()}
    seeds = seeds_for(ops, B)
    seeds_before = seeds.clone()
    ops.sampler_step_lin_noise(ins["x_base"][1], ins["x_model"][1], halves["out_u"][1], halves["out_c"][1], 3.0, K.V,
                               0.7 if form == "rescale" else 0., K.X0, K.AM, K.SM, ins["h1"][1], ins["h2"][1], 0.9, 0.3, -0.2, 0.1,
                               outs["model_out"][1], outs["x_out"][1], CN, noise=ins["noise"][1] if source == "noise" else None,
                               seeds=seeds if source == "seeds" else None, draw=DRAW, thresholding=form == "threshold",
                               max_val=0.5, model_pre_out=outs["pre"][1], thr_out=small["thr"][1], factor_out=small["fac"][1])
    for k, (buf, view) in outs.items():
        G.assert_footprint(buf, view, f"{form} {source} {k}", written=True)
        assert torch.isfinite(view).all(), k
    G.assert_footprint(*small["fac"], f"{form} factor_out", written=True)
    if form == "threshold":
        G.assert_footprint(*small["thr"], f"{form} thr_out", written=True)
    else:
        assert bool((small["thr"][0] == G.SENT).all())
    for k, (buf, _) in {**ins, **halves}.items():          # inputs: untouched, bit for bit
        kind = torch.int32 if buf.dtype == torch.float32 else torch.int16
        assert torch.equal(buf.view(kind), before[k].view(kind)), k
    assert torch.equal(seeds, seeds_before)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ops):
    from minddiffusion_amd import _lib
    from minddiffusion_amd._lib import MdxError
    shape = SHAPES[0]
    t = K.inputs(shape, seed=1)
    d = {k: torch.tensor(v, device=DEV) for k, v in t.items()}
    z = torch.tensor(z_for(shape), device=DEV)
    seeds = seeds_for(ops, 3)
    mo, xo, pre = (torch.full(shape, 5., device=DEV) for _ in range(3))
    thr, fac = torch.full((3,), 5., device=DEV), torch.full((3,), 5., device=DEV)

    def call(match, **kw):
        a = dict(x_base=d["x_base"], x_model=d["x_model"], out_u=d["out_u"], out_c=d["out_c"], cfg_scale=3.0, pred_type=K.EPS,
                 guidance_rescale=0., value_type=K.X0, alpha_m=K.AM, sigma_m=K.SM, h1=d["h1"], h2=d["h2"], A=0.9, c0=0.3, c1=0.2,
                 c2=0.1, model_out=mo, x_out=xo, cn=CN, noise=z, seeds=None, stream=ops.RNG_STEP, draw=0, thresholding=False,
                 max_val=1., model_pre_out=pre, thr_out=thr, factor_out=fac)
        a.update(kw)
        with pytest.raises(MdxError, match=match):
            ops.sampler_step_lin_noise(**a)

    for bad in (float("nan"), float("inf"), float("-inf")):
        call("cn .* is not finite", cn=bad)
        call("cn .* is not finite", cn=bad, noise=None)
    call("exactly one noise source.*both", seeds=seeds)
    call("exactly one noise source.*neither", noise=None)
    call("stream must be in", stream=1 << 31)
    call("stream must be in", stream=-1)
    call("draw in", draw=1 << 32)
    call("noise: expected", noise=z[:2])
    call("noise: expected torch.float32", noise=z.double())
    call("seeds must be a", noise=None, seeds=seeds[:2])
    call("seeds", noise=None, seeds=seeds.to(torch.int32))
    for name, out in (("model_out", "model_out"), ("x_out", "x_out"), ("model_pre_out", "model_pre_out")):
        call(f"{name} overlaps noise", **{out: z})
    flat = torch.zeros(421, device=DEV)
    call("x_out overlaps noise", noise=flat[:420].reshape(shape), x_out=flat[1:].reshape(shape))
    # everything the lin entry refuses, under this entry's name
    call("mdx_sampler_step_lin_noise_f32: unknown pred_type", pred_type=2)
    call("non-zero history coefficient", h1=None)
    call("alpha_m == 0", alpha_m=0.)
    call("thresholding acts on a data prediction", thresholding=True, value_type=K.NOISE)
    call("guidance_rescale", guidance_rescale=1.5)
    call("model_out overlaps h1", model_out=d["h1"])
    call("out_c, model_out and x_out are required", x_out=None)
    call("unknown pred_type", pred_type=2, cn=0.)               # ... and at cn == 0 too
    # the library's own refusal of a stream with the top bit (the wrapper above refuses it first)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = _lib.load().mdx_sampler_step_lin_noise_f32(p(d["x_base"]), p(d["x_model"]), None, p(d["out_c"]), K.LD, 1., 0, 0., 0, K.AM,
                                                    K.SM, 0, 1., None, None, 0.9, 0.3, 0., 0., p(mo), p(xo), None, None, None, CN,
                                                    None, p(seeds), 1 << 31, 0, *shape, None)
    assert rc != 0
    with pytest.raises(MdxError, match="stream .* is not below 2\\^31"):
        _lib.check(rc, "mdx_sampler_step_lin_noise_f32")
    torch.cuda.synchronize()
    for o in (mo, xo, pre, thr, fac):              # refused before any launch
        assert bool((o == 5.).all())
    # cn == 0 reads neither source: a noise that overlaps an output passes, and so do both sources at once
    ops.sampler_step_lin_noise(d["x_base"], None, None, d["out_c"], 1., K.EPS, 0., K.X0, K.AM, K.SM, None, None, 0.9, 0.3, 0., 0.,
                               mo, xo, 0., noise=xo, seeds=seeds)
    torch.cuda.synchronize()
