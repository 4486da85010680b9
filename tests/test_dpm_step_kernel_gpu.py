"""ops.sampler_step_lin (mdx_sampler_step_lin_f32): the model value of one evaluation and the linear form
x_out = A x_base + c0 val + c1 h1 + c2 h2, in both launch forms.

Reference and bound.  The reference is float64 numpy on the very fp16 model outputs and the float32-rounded scalars the launch
gets.  The bound per element is 32 * 2^-24 times the sum of the magnitudes of all terms as they enter (products taken in
absolute value): a count of roundings -- at most 17 between the fp16 inputs and x_out (combine 3, rescale 1, v -> eps 3, data
prediction 3, linear form 7), each at most 2^-24 of a partial result that is no larger than that sum -- not a measurement.
The rescale factor f of the reference is the launch's own factor_out (it is held to the float64 formula at 1e-5, the bound of
tests/test_guidance_rescale_gpu.py for the same reduction).

Thresholding is checked bit for bit: thr_out against the numpy-float32 statement of the formula on the sorted |model_pre_out|,
model_out against clip(pre, -s, s) / s."""
import numpy as np
import pytest
import torch

import _guard as G
import _rescale_util as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, V = 0, 1
X0, NOISE = 0, 1
ULP = 32 * 2.0 ** -24
SHAPES = [(3, 4, 5, 7), (2, 4, 33, 37), (1, 4, 64, 64)]
LD = 8
f32 = np.float32


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops
    return ops


def inputs(shape, seed):
    """NCHW fp32 x_base, x_model, h1, h2 and NHWC fp16 out_u, out_c (channels C .. LD - 1 NaN: they are not the launch's)."""
    B, C, H, W = shape
    rng = np.random.RandomState(seed)
    t = {k: rng.randn(*shape).astype(f32) for k in ("x_base", "x_model", "h1", "h2")}
    for k in ("out_u", "out_c"):
        o = np.full((B, H * W, LD), np.nan, np.float16)
        o[..., :C] = (rng.randn(B, H * W, C) * 0.7 + 0.1).astype(np.float16)
        t[k] = o
    return t


def nchw(o, shape):
    B, C, H, W = shape
    return o[..., :C].astype(np.float64).reshape(B, H * W, C).transpose(0, 2, 1).reshape(shape)


def reference(t, shape, pred, value, with_u, cfg, am, sm, A, c, f, x_model_key):
    """(val, |val| bound, x_out, |x_out| bound) in float64; f: [B] rescale factors (1 without rescale)."""
    oc, xm = nchw(t["out_c"], shape), t[x_model_key].astype(np.float64)
    m, mag = oc, np.abs(oc)
    if with_u:
        ou = nchw(t["out_u"], shape)
        m = ou + cfg * (oc - ou)
        mag = np.abs(ou) + abs(cfg) * (np.abs(oc) + np.abs(ou))
    fb = np.asarray(f, np.float64).reshape(-1, 1, 1, 1)
    m, mag = m * fb, mag * np.abs(fb)
    if pred == V:
        m, mag = am * m + sm * xm, abs(am) * mag + abs(sm) * np.abs(xm)
    if value == X0:
        m, mag = (xm - sm * m) / am, (np.abs(xm) + abs(sm) * mag) / abs(am)
    x = c[0] * m + A * t["x_base"].astype(np.float64) + c[1] * t["h1"].astype(np.float64) + c[2] * t["h2"].astype(np.float64)
    xmag = abs(c[0]) * mag + abs(A) * np.abs(t["x_base"]) + abs(c[1]) * np.abs(t["h1"]) + abs(c[2]) * np.abs(t["h2"])
    return m, ULP * mag, x, ULP * xmag


def launch(ops, t, shape, pred, value, with_u, cfg, am, sm, A, c, phi=0., x_model_key="x_base", thresholding=False, max_val=1.,
           alias=None, nan_skipped=False):
    """One launch on fresh device tensors; returns the outputs as numpy.  alias: "x_base" | "x_model" -- x_out IS that input.
    nan_skipped: every input whose term is skipped points to NaN-filled memory."""
    B = shape[0]
    d = {k: torch.tensor(v, device=DEV) for k, v in t.items()}
    nan = torch.full(shape, float("nan"), device=DEV)
    x_model = d[x_model_key].clone() if x_model_key != "x_base" else None
    x_base = d["x_base"].clone()
    if nan_skipped and A == 0. and x_model is not None:
        x_base = nan
    h1 = d["h1"] if c[1] != 0. else (nan if nan_skipped else None)
    h2 = d["h2"] if c[2] != 0. else (nan if nan_skipped else None)
    model_out, pre = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
    thr, fac = torch.full((B,), -7., device=DEV), torch.full((B,), -7., device=DEV)
    x_out = {None: torch.empty(shape, device=DEV), "x_base": x_base, "x_model": x_base if x_model is None else x_model}[alias]
    ops.sampler_step_lin(x_base, x_model, d["out_u"] if with_u else None, d["out_c"], cfg, pred, phi, value, am, sm, h1, h2, A,
                         c[0], c[1], c[2], model_out, x_out, thresholding=thresholding, max_val=max_val, model_pre_out=pre,
                         thr_out=thr, factor_out=fac)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(model_out=model_out, pre=pre, x_out=x_out, thr=thr, fac=fac).items()}


def within(name, got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{name}: worst error / bound = {worst:.4f}")
    assert np.all(err <= bound), f"{name}: {int((err > bound).sum())} elements beyond the bound, worst {worst:.3f} x"


AM, SM = float(f32(0.83)), float(f32(0.5577))
# name -> (pred, value, with_u, guidance scale, A, (c0, c1, c2), phi, x_model)
CASES = {
    "eps_x0_nou_h0": (EPS, X0, False, 1.0, 0.91, (0.21, 0., 0.), 0., "x_base"),
    "eps_x0_u_h1": (EPS, X0, True, 7.5, 0.91, (0.33, -0.12, 0.), 0., "x_base"),
    "v_x0_u_h2_xmodel": (V, X0, True, 3.0, 0.77, (0.5, -0.4, 0.13), 0., "x_model"),
    "v_eps_u_h2": (V, NOISE, True, 3.0, 0.97, (-0.2, 0.11, -0.03), 0., "x_base"),
    "eps_eps_nou_h1_xmodel": (EPS, NOISE, False, 1.0, 0.97, (-0.2, 0.11, 0.), 0., "x_model"),
    "v_x0_nou_A0": (V, X0, False, 1.0, 0., (1.0, 0., 0.), 0., "x_base"),
    "eps_x0_u_A0_xmodel": (EPS, X0, True, 5.0, 0., (1.0, 0., 0.), 0., "x_model"),
    "eps_x0_u_h1_rescale": (EPS, X0, True, 7.5, 0.91, (0.33, -0.12, 0.), 0.7, "x_base"),
    "v_eps_u_h2_xmodel_rescale": (V, NOISE, True, 4.0, 0.8, (0.4, 0.1, -0.2), 1.0, "x_model"),
    "v_x0_u_h2_xmodel_rescale": (V, X0, True, 4.0, 0.8, (0.4, 0.1, -0.2), 0.5, "x_model"),
}


def scalars(case):
    pred, value, with_u, cfg, A, c, phi, xmk = CASES[case]
    return pred, value, with_u, float(f32(cfg)), float(f32(A)), tuple(float(f32(v)) for v in c), phi, xmk


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("case", sorted(CASES))
def test_value_and_linear_form(ops, shape, case):
    pred, value, with_u, cfg, A, c, phi, xmk = scalars(case)
    t = inputs(shape, seed=len(case) + shape[2])
    got = launch(ops, t, shape, pred, value, with_u, cfg, AM, SM, A, c, phi=phi, x_model_key=xmk)
    if phi:
        oc, ou = nchw(t["out_c"], shape), nchw(t["out_u"], shape)
        f64 = R.rescale_factor(oc, ou + cfg * (oc - ou), phi)
        assert np.all(np.abs(got["fac"] - f64) <= 1e-5 * np.abs(f64)), (got["fac"], f64)
        assert shape[0] == 1 or np.ptp(f64) > 0         # the samples' factors differ: a sample mix-up shows
    else:
        assert np.array_equal(got["fac"], np.ones(shape[0], f32))
    val, vb, x, xb = reference(t, shape, pred, value, with_u, cfg, AM, SM, A, c, got["fac"], xmk)
    within(f"{case} {shape} model_out", got["model_out"], val, vb)
    within(f"{case} {shape} x_out", got["x_out"], x, xb)
    assert np.array_equal(got["pre"].view(np.uint32), got["model_out"].view(np.uint32))
    assert np.array_equal(got["thr"], np.full(shape[0], -7., f32))       # written with thresholding only


@pytest.mark.parametrize("alias", ["x_base", "x_model"])
@pytest.mark.parametrize("case", ["v_x0_u_h2_xmodel", "v_x0_u_h2_xmodel_rescale", "eps_x0_u_h1"])
def test_x_out_may_be_an_input(ops, case, alias):
    """Bit-equal to the launch with an x_out of its own, in the spread and the owned form."""
    shape = SHAPES[1]
    pred, value, with_u, cfg, A, c, phi, xmk = scalars(case)
    t = inputs(shape, seed=5)
    kw = dict(phi=phi, x_model_key=xmk)
    plain = launch(ops, t, shape, pred, value, with_u, cfg, AM, SM, A, c, **kw)
    aliased = launch(ops, t, shape, pred, value, with_u, cfg, AM, SM, A, c, alias=alias, **kw)
    for k in ("x_out", "model_out", "fac"):
        assert np.array_equal(plain[k].view(np.uint32), aliased[k].view(np.uint32)), k
    thr = launch(ops, t, shape, pred, value, with_u, cfg, AM, SM, A, c, thresholding=True, max_val=0.5, **kw)
    thr_aliased = launch(ops, t, shape, pred, value, with_u, cfg, AM, SM, A, c, thresholding=True, max_val=0.5, alias=alias, **kw)
    for k in ("x_out", "model_out", "pre", "thr"):
        assert np.array_equal(thr[k].view(np.uint32), thr_aliased[k].view(np.uint32)), k


@pytest.mark.parametrize("case", ["eps_x0_nou_h0", "eps_x0_u_A0_xmodel", "eps_x0_u_h1_rescale"])
def test_a_zero_coefficient_skips_its_tensor(ops, case):
    shape = SHAPES[0]
    pred, value, with_u, cfg, A, c, phi, xmk = scalars(case)
    t = inputs(shape, seed=9)
    plain = launch(ops, t, shape, pred, value, with_u, cfg, AM, SM, A, c, phi=phi, x_model_key=xmk)
    skipped = launch(ops, t, shape, pred, value, with_u, cfg, AM, SM, A, c, phi=phi, x_model_key=xmk, nan_skipped=True)
    assert np.isfinite(skipped["x_out"]).all()
    for k in ("x_out", "model_out"):
        assert np.array_equal(plain[k].view(np.uint32), skipped[k].view(np.uint32)), k


# ------------------------------------------------------------------------------------------------ thresholding
def threshold_patterns(shape, seed):
    """x_model per sample such that the data prediction IS x_model (out_c = 0, alpha_m = 1): a constant sample, heavy ties,
    zeros and subnormals under two large values, subnormals only, and plain noise, dealt round robin over a batch of 5."""
    _, C, H, W = shape
    N = C * H * W
    rng = np.random.RandomState(seed)
    const = np.full(N, -0.75, f32)
    ties = (np.round(rng.randn(N) * 2) / 2).astype(f32)                       # multiples of 0.5, the top ones many times over
    tiny = np.zeros(N, f32)
    tiny[rng.rand(N) < 0.3] = -0.0
    sub = rng.rand(N) < 0.4
    tiny[sub] = (rng.randint(1, 1 << 22, int(sub.sum())).astype(np.uint32)).view(f32) * rng.choice([-1, 1], int(sub.sum()))
    only_sub = tiny.copy()
    tiny[rng.choice(N, 2, replace=False)] = [1.5, -2.25]
    noise = (rng.randn(N) * np.exp(rng.randn(N))).astype(f32)
    return np.stack([const, ties, tiny.astype(f32), only_sub.astype(f32), noise]).reshape((5, C, H, W))


def numpy_threshold(pre, max_val):
    """The reference's definition, every operation in float32: (s [B], clip(pre, -s, s) / s)."""
    B = pre.shape[0]
    srt = np.sort(np.abs(pre.reshape(B, -1)), axis=1)
    k = int((srt.shape[1] - 1) * 0.995)
    a, b = srt[:, k], srt[:, k + 1]
    s = a + (b - a) * f32(0.995)
    assert s.dtype == f32
    s = np.maximum(s, f32(max_val))
    sb = s.reshape(-1, 1, 1, 1)
    return s, np.clip(pre, -sb, sb) / sb, a, b


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("max_val", [1e-42, 0.4, 100.0])
def test_threshold_patterns_bit_for_bit(ops, shape, max_val):
    shape5 = (5,) + shape[1:]
    pats = threshold_patterns(shape, seed=shape[3])
    t = inputs(shape5, seed=3)
    t["x_model"] = pats
    t["out_c"][..., :shape[1]] = 0.
    A, c = float(f32(0.9)), (float(f32(0.3)), float(f32(-0.2)), 0.)
    got = launch(ops, t, shape5, EPS, X0, False, 1.0, 1.0, SM, A, c, x_model_key="x_model", thresholding=True, max_val=max_val)
    assert np.array_equal(got["pre"].view(np.uint32), pats.view(np.uint32))       # (x_m - sigma * 0) / 1
    s, clipped, a, b = numpy_threshold(got["pre"], max_val)
    print(f"{shape} max_val {max_val}: a {a}, b {b}, s {s}")
    assert np.array_equal(got["thr"].view(np.uint32), s.view(np.uint32)), (got["thr"], s)
    assert np.array_equal(got["model_out"].view(np.uint32), clipped.view(np.uint32))
    # both ends of the selection are in the cases: the two order statistics tie / differ; s / max_val wins
    assert (a == b).any() and (a < b).any()
    if max_val == 0.4:
        assert (s > f32(max_val)).any() and (s == f32(max_val)).any()
    x = c[0] * got["model_out"].astype(np.float64) + A * t["x_base"].astype(np.float64) + c[1] * t["h1"].astype(np.float64)
    xb = ULP * (abs(c[0]) * np.abs(got["model_out"]) + abs(A) * np.abs(t["x_base"]) + abs(c[1]) * np.abs(t["h1"]))
    within(f"threshold {shape} x_out", got["x_out"], x, xb)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("case", ["eps_x0_u_h1", "v_x0_u_h2_xmodel", "v_x0_u_h2_xmodel_rescale"])
def test_threshold_on_model_outputs(ops, shape, case):
    """The whole chain with thresholding on: model_pre_out within the bound of the reference, and the selection, the clamp and
    the linear form exact / within the bound on the launch's own model_pre_out."""
    pred, value, with_u, cfg, A, c, phi, xmk = scalars(case)
    t = inputs(shape, seed=21)
    for max_val in (0.5, 50.0):
        got = launch(ops, t, shape, pred, value, with_u, cfg, AM, SM, A, c, phi=phi, x_model_key=xmk, thresholding=True,
                     max_val=max_val)
        val, vb, _, _ = reference(t, shape, pred, value, with_u, cfg, AM, SM, A, c, got["fac"], xmk)
        within(f"{case} {shape} model_pre_out", got["pre"], val, vb)
        s, clipped, _, _ = numpy_threshold(got["pre"], max_val)
        assert np.array_equal(got["thr"].view(np.uint32), s.view(np.uint32))
        assert np.array_equal(got["model_out"].view(np.uint32), clipped.view(np.uint32))
        assert (s > f32(max_val)).all() if max_val == 0.5 else (s == f32(max_val)).all()
        mo = got["model_out"].astype(np.float64)
        x = c[0] * mo + A * t["x_base"].astype(np.float64) + c[1] * t["h1"].astype(np.float64) + c[2] * t["h2"].astype(np.float64)
        xb = ULP * (abs(c[0]) * np.abs(mo) + abs(A) * np.abs(t["x_base"]) + abs(c[1]) * np.abs(t["h1"]) + abs(c[2]) * np.abs(t["h2"]))
        within(f"{case} {shape} thresholded x_out", got["x_out"], x, xb)


# ------------------------------------------------------------------------------------------------ against the existing step
@pytest.mark.parametrize("pred,phi", [(EPS, 0.), (V, 0.), (EPS, 0.7), (V, 0.7)])
@pytest.mark.parametrize("second_order", [False, True])
def test_a_2m_row_agrees_with_the_existing_step(ops, pred, phi, second_order):
    """ops.sampler_update with a DPM-Solver++(2M) row's scalars (schedule.dpm_step_scalars) and the new entry with the same
    row as (A, c0, c1) compute the same update: both within the bound of the float64 reference, so within twice the bound of
    each other."""
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP, multistep_2m_plan
    from minddiffusion_amd.ldm.models.diffusion.schedule import PLMS_AB, dpm_model_point, dpm_step_scalars
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2
    row = multistep_2m_plan(NoiseScheduleVP("discrete", betas=betas), 10)[4 if second_order else 0]
    assert (row["c1"] != 0.) == second_order
    shape, cfg = SHAPES[1], float(f32(7.5))
    t = inputs(shape, seed=13)
    d = {k: torch.tensor(v, device=DEV) for k, v in t.items()}
    am, sm = (float(v) for v in dpm_model_point(row))
    x_prev, pred_x0 = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
    update = tuple(float(v) for v in dpm_step_scalars(row))
    ops.sampler_update(d["x_base"], d["out_u"], d["out_c"], cfg, pred, [], PLMS_AB[0],
                       update + (d["h1"] if second_order else None, None, x_prev, pred_x0), phi, None, am, sm)
    A, c = float(f32(row["A"])), (float(f32(row["c0"])), float(f32(row["c1"])), 0.)
    got = launch(ops, t, shape, pred, X0, True, cfg, am, sm, A, c, phi=phi)
    val, vb, x, xb = reference(t, shape, pred, X0, True, cfg, am, sm, A, c, got["fac"], "x_base")
    within("new entry x_out", got["x_out"], x, xb)
    # the existing step forms sqrt_a_prev * x0 + dir_coef * e with sqrt_a_prev = A alpha + c0 and dir_coef = A sigma rounded to
    # float32 on the host: two more roundings of terms the sum of magnitudes already holds
    xb_old = xb + ULP * (abs(A) * (abs(am) * np.abs(val) + abs(sm) * np.abs((t["x_base"] - am * val) / sm)))
    within("existing step x_prev", x_prev.cpu().numpy(), x, xb_old)
    within("existing step pred_x0", pred_x0.cpu().numpy(), val, vb)
    assert np.all(np.abs(got["x_out"].astype(np.float64) - x_prev.cpu().numpy()) <= xb + xb_old)
    assert np.all(np.abs(got["model_out"].astype(np.float64) - pred_x0.cpu().numpy()) <= 2 * vb)


# ------------------------------------------------------------------------------------------------ footprint
@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
@pytest.mark.parametrize("form", ["spread", "rescale", "threshold"])
def test_only_the_outputs_are_written(ops, shape, form):
    B, C, H, W = shape
    t = inputs(shape, seed=2)
    outs = {k: G.guarded(shape, torch.float32) for k in ("model_out", "x_out", "pre")}
    small = {k: G.guarded((B,), torch.float32) for k in ("thr", "fac")}
    ins = {k: G.poisoned(t[k]) for k in ("x_base", "x_model", "h1", "h2")}
    halves = {k: G.poisoned(t[k]) for k in ("out_u", "out_c")}
    before = {k: v[0].clone() for k, v in {**ins, **halves}.items()}
    ops.sampler_step_lin(ins["x_base"][1], ins["x_model"][1], halves["out_u"][1], halves["out_c"][1], 3.0, V,
                         0.7 if form == "rescale" else 0., X0, AM, SM, ins["h1"][1], ins["h2"][1], 0.9, 0.3, -0.2, 0.1,
                         outs["model_out"][1], outs["x_out"][1], thresholding=form == "threshold", max_val=0.5,
                         model_pre_out=outs["pre"][1], thr_out=small["thr"][1], factor_out=small["fac"][1])
    for k, (buf, view) in outs.items():
        G.assert_footprint(buf, view, f"{form} {k}", written=True)
        assert torch.isfinite(view).all(), k
    G.assert_footprint(*small["fac"], f"{form} factor_out", written=True)
    if form == "threshold":
        G.assert_footprint(*small["thr"], f"{form} thr_out", written=True)
    else:
        assert bool((small["thr"][0] == G.SENT).all())
    for k, (buf, _) in {**ins, **halves}.items():          # inputs: untouched, bit for bit
        kind = torch.int32 if buf.dtype == torch.float32 else torch.int16
        assert torch.equal(buf.view(kind), before[k].view(kind)), k


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ops):
    from minddiffusion_amd._lib import MdxError
    shape = SHAPES[0]
    t = inputs(shape, seed=1)
    d = {k: torch.tensor(v, device=DEV) for k, v in t.items()}
    mo, xo, pre = (torch.full(shape, 5., device=DEV) for _ in range(3))
    thr, fac = torch.full((3,), 5., device=DEV), torch.full((3,), 5., device=DEV)

    def call(match, **kw):
        a = dict(x_base=d["x_base"], x_model=d["x_model"], out_u=d["out_u"], out_c=d["out_c"], cfg_scale=3.0, pred_type=EPS,
                 guidance_rescale=0., value_type=X0, alpha_m=AM, sigma_m=SM, h1=d["h1"], h2=d["h2"], A=0.9, c0=0.3, c1=0.2,
                 c2=0.1, model_out=mo, x_out=xo, thresholding=False, max_val=1., model_pre_out=pre, thr_out=thr, factor_out=fac)
        a.update(kw)
        with pytest.raises(MdxError, match=match):
            ops.sampler_step_lin(**a)

    call("out_c, model_out and x_out are required", out_c=None)
    call("out_c, model_out and x_out are required", model_out=None)
    call("out_c, model_out and x_out are required", x_out=None)
    call("non-zero history coefficient", h1=None)
    call("non-zero history coefficient", h2=None)
    call("unknown pred_type", pred_type=2)
    call("unknown value_type", value_type=2)
    call("alpha_m == 0", alpha_m=0.)
    call("thresholding acts on a data prediction", thresholding=True, value_type=NOISE)
    for bad in (0., -1., float("inf"), float("nan")):
        call("max_val", thresholding=True, max_val=bad)
    for bad in (-0.1, 1.5, float("nan")):
        call("guidance_rescale", guidance_rescale=bad)
    call("model_out overlaps h1", model_out=d["h1"])
    call("model_out overlaps x_base", model_out=d["x_base"])
    call("x_out overlaps out_c", x_out=d["out_c"].view(torch.float32).reshape(-1)[:420].reshape(shape))
    call("x_out overlaps h2", x_out=d["h2"])
    call("model_pre_out overlaps x_model", model_pre_out=d["x_model"])
    call("model_out overlaps x_out", x_out=mo)
    call("model_out overlaps model_pre_out", model_pre_out=mo)
    # one element per sample: no two order statistics, no std
    one = (2, 1, 1, 1)
    z = lambda: torch.zeros(one, device=DEV)
    h = torch.zeros((2, 1, LD), dtype=torch.float16, device=DEV)
    with pytest.raises(MdxError, match="two order statistics"):
        ops.sampler_step_lin(z(), None, None, h, 1., EPS, 0., X0, 1., 0.5, None, None, 1., 1., 0., 0., z(), z(), thresholding=True)
    with pytest.raises(MdxError, match="per-sample std"):
        ops.sampler_step_lin(z(), None, h.clone(), h, 1., EPS, 0.5, X0, 1., 0.5, None, None, 1., 1., 0., 0., z(), z())
    # the wrapper's own checks: the library sees pointers only
    call("x_model: expected", x_model=d["x_model"][:2])
    call("model_out: expected torch.float32", model_out=mo.half())
    call("out_u: expected NHWC", out_u=d["out_u"][:, :-1].contiguous())
    call("thr_out: needs 3 elements", thr_out=thr[:2])
    torch.cuda.synchronize()
    for o in (mo, xo, pre, thr, fac):              # refused before any launch
        assert bool((o == 5.).all())
    # a shifted x_out overlaps x_base without being it
    flat = torch.zeros(421, device=DEV)
    with pytest.raises(MdxError, match="x_out overlaps x_base"):
        ops.sampler_step_lin(flat[:420].reshape(shape), d["x_model"], None, d["out_c"], 1., EPS, 0., X0, AM, SM, None, None, 0.9,
                             0.3, 0., 0., mo, flat[1:].reshape(shape))
    # a skipped input is not read and may lie anywhere: model_out over an h1 with c1 == 0 passes
    ops.sampler_step_lin(d["x_base"], None, None, d["out_c"], 1., EPS, 0., X0, AM, SM, d["h1"], None, 0.9, 0.3, 0., 0., d["h1"], xo)
    torch.cuda.synchronize()


def test_sample_extent_above_31_bits_is_refused():
    """The entry itself, with pointers it never dereferences: the refusal precedes any launch."""
    import ctypes
    from minddiffusion_amd import _lib
    buf = torch.zeros(16, device=DEV)
    p = ctypes.c_void_p(buf.data_ptr())
    rc = _lib.load().mdx_sampler_step_lin_f32(p, p, None, p, 8, 1., 0, 0., 0, 1., .5, 0, 1., None, None, 1., 1., 0., 0., p, p,
                                              None, None, None, 1, 4, 32768, 16384, None)
    assert rc != 0
    with pytest.raises(_lib.MdxError, match="exceeds 31 bits"):
        _lib.check(rc, "mdx_sampler_step_lin_f32")
    for dims in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, -1, 8), (1, 4, 8, 0)):
        assert _lib.load().mdx_sampler_step_lin_f32(p, p, None, p, 8, 1., 0, 0., 0, 1., .5, 0, 1., None, None, 1., 1., 0., 0., p,
                                                    p, None, None, None, *dims, None) != 0
    assert _lib.load().mdx_sampler_step_lin_f32(p, p, None, p, 3, 1., 0, 0., 0, 1., .5, 0, 1., None, None, 1., 1., 0., 0., p, p,
                                                None, None, None, 1, 4, 2, 2, None) != 0      # out_ld < C
    assert _lib.load().mdx_sampler_step_lin_f32(None, p, None, p, 8, 1., 0, 0., 0, 1., .5, 0, 1., None, None, 1., 1., 0., 0., p,
                                                p, None, None, None, 1, 4, 2, 2, None) != 0     # NULL x_base
