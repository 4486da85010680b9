"""Guidance rescale on the GPU: mdx_sampler_step_rescale_f32 against numpy, its bit-identity and aliasing contracts, and the
three samplers with `guidance_rescale` against RescaleModelOracle (tests/_rescale_util.py).

Tolerances: the kernel is fp32 arithmetic on given inputs -> rel-L2 1e-5 on x_prev / pred_x0 / e_t_out (the bound of the other
step tests) and 1e-5 relative on the factors (fp32 sums of <= 36 864 centred values, reduced per thread, wave and workgroup).
Trajectories: the project's bound for 5 / 10-step tiny-UNet runs, rel-L2 <= 1e-2 and max|d| <= 1e-2 max|ref|;
test_guidance_rescale_cpu.py checks that the oracle's own fp32 and fp16-emulated runs of every case stay inside it.
"""
import numpy as np
import pytest
import torch

import _rescale_util as R
import _vpred_util as V
from _util import check, h16
from oracle import ldm as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def dev32(a):
    return torch.tensor(np.asarray(a, np.float32), device=DEV)


def out_buf(e, ld=8):
    """NCHW values -> the UNet's NHWC fp16 output layout [B][HW][ld]; the pad channels hold a value that must not be read
    (one of them inside the statistics would wreck the std)."""
    B, C, H, W = e.shape
    buf = np.full((B, H * W, ld), 1e4, np.float32)
    buf[:, :, :C] = e.transpose(0, 2, 3, 1).reshape(B, H * W, C)
    return torch.tensor(buf, dtype=torch.float16, device=DEV)


COEF = {0: (1, 0, 0, 0), 1: (1.5, -0.5, 0, 0), 3: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}
# each sample its own output scales, and another for out_u than for out_c (f does not change when both are scaled alike):
# the factors differ, so a sample-index mix-up shows
SAMPLE_SCALE = (0.5, 1.0, 3.0)
SHAPES = {
    "3x4x5x7": (3, 4, 5, 7),        # 140 elements per sample: fewer than a workgroup, not a multiple of a wave
    "2x4x33x37": (2, 4, 33, 37),    # 4 884 per sample: several ragged trips
    "1x4x96x96": (1, 4, 96, 96),    # the 768-v latent
}


def _reference(a, phi):
    """numpy (fp32 / fp16-rounded inputs, float64 arithmetic) result of one step: (x_prev, pred_x0, e_t, f)."""
    f64 = np.float64
    vu, vc = a["vu"].astype(f64), a["vc"].astype(f64)
    m = vu + f64(a["scale"]) * (vc - vu)
    f = R.rescale_factor(vc, m, phi)
    m = f.reshape(-1, 1, 1, 1) * m
    e_t = f64(a["am"]) * m + f64(a["bm"]) * a["xm"].astype(f64) if a["pred"] == 1 else m
    coef = a["coef"]
    ep = coef[0] * e_t + sum(c * o.astype(f64) for c, o in zip(coef[1:], a["olds"]))
    s_at, s_1mat, s_ap, dirc, sigma = (f64(v) for v in a["scalars"])
    px0 = (a["x"].astype(f64) - s_1mat * ep) / s_at
    xp = s_ap * px0 + dirc * ep + (sigma * a["noise"].astype(f64) if a["noise"] is not None else 0.0)
    return xp, px0, e_t, f


def _case(shape, pred, order, sigma, separate_xm, seed, scale=7.5, outputs=None):
    """Inputs of one step.  outputs: (vu, vc) to use instead of per-sample-scaled N(0,1) draws."""
    rng = np.random.RandomState(seed)
    B = shape[0]
    x = rng.standard_normal(shape).astype(np.float32)
    xm = rng.standard_normal(shape).astype(np.float32) if separate_xm else x
    if outputs is None:
        su = np.array([SAMPLE_SCALE[b % 3] for b in range(B)], np.float32).reshape(B, 1, 1, 1)
        sc = np.array([SAMPLE_SCALE[(b + 1) % 3] for b in range(B)], np.float32).reshape(B, 1, 1, 1)
        outputs = su * rng.standard_normal(shape), sc * rng.standard_normal(shape)
    vu, vc = h16(outputs[0]), h16(outputs[1])
    olds = [rng.standard_normal(shape).astype(np.float32) for _ in range(order)]
    noise = rng.standard_normal(shape).astype(np.float32)
    a_t, a_prev = np.float32(0.3), np.float32(0.5)
    # the model's own point: another timestep than the update's when x_model is a distinct tensor (the PLMS first step)
    am, bm = (np.float32(np.sqrt(0.4)), np.float32(np.sqrt(0.6))) if separate_xm else (np.sqrt(a_t), np.sqrt(1 - a_t))
    dirc = np.sqrt(1 - a_prev - np.float32(sigma) ** 2)
    return dict(x=x, xm=xm, vu=vu, vc=vc, olds=olds, coef=COEF[order], scale=scale, am=am, bm=bm, pred=pred,
                scalars=(np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_prev), dirc, np.float32(sigma)),
                noise=noise if sigma else None)


def _launch(ops, a, phi, entry="rescale", no_u=False, x_prev=None, x_t=None, xm_t=None):
    """Run the new entry (or, entry="pred", ops.sampler_step_pred on the same inputs).  x_t / xm_t / x_prev: preallocated
    device tensors (to alias them).  Returns (x_prev, pred_x0, e_t, f)."""
    xd = dev32(a["x"]) if x_t is None else x_t
    xmd = xm_t if xm_t is not None else (None if a["xm"] is a["x"] else dev32(a["xm"]))
    e_out, p_out = torch.empty_like(xd), torch.empty_like(xd)
    x_out = torch.empty_like(xd) if x_prev is None else x_prev
    f_out = torch.full((xd.shape[0],), -7.0, device=DEV)
    args = (xd, xmd, None if no_u else out_buf(a["vu"]), out_buf(a["vc"]), 8, a["scale"], a["pred"], a["am"], a["bm"],
            [dev32(o) for o in a["olds"]], a["coef"], *a["scalars"], None if a["noise"] is None else dev32(a["noise"]),
            e_out, x_out, p_out)
    if entry == "pred":
        ops.sampler_step_pred(*args)
    else:
        ops.sampler_step_rescale(*args, phi, f_out)
    torch.cuda.synchronize()
    return x_out, p_out, e_out, f_out


def _check_step(tag, got, ref):
    f_got, f_ref = got[3].cpu().numpy().astype(np.float64), ref[3]
    f_err = float(np.abs(f_got - f_ref).max() / np.abs(f_ref).max()) if len(f_ref) else 0.0
    print("FACTOR", tag, "got", f_got.tolist(), "ref", f_ref.tolist(), "max_rel_err", f_err)
    assert np.all(np.abs(f_got - f_ref) <= 1e-5 * np.abs(f_ref)), (tag, f_got, f_ref)
    check(tag + "_x", got[0], ref[0], rel_l2=1e-5, factor_rel_err=f_err)
    check(tag + "_p", got[1], ref[1], rel_l2=1e-5)
    check(tag + "_e", got[2], ref[2], rel_l2=1e-5)


@pytest.mark.parametrize("phi", R.PHIS)
@pytest.mark.parametrize("separate_xm", [False, True])
@pytest.mark.parametrize("sigma", [0.0, 0.3])
@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("pred", [0, 1])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_sampler_step_rescale_vs_numpy(ops, shape, pred, order, sigma, separate_xm, phi):
    a = _case(SHAPES[shape], pred, order, sigma, separate_xm, seed=order + 4 * pred + 8 * int(separate_xm))
    ref = _reference(a, phi)
    if len(ref[3]) > 1:
        assert np.ptp(ref[3]) > 1e-3          # the samples' factors do differ
    _check_step(f"step_rescale_{shape}_pred{pred}_o{order}_s{sigma}_xm{int(separate_xm)}_phi{phi}", _launch(ops, a, phi), ref)


@pytest.mark.parametrize("phi", R.PHIS)
@pytest.mark.parametrize("pred", [0, 1])
def test_outputs_on_an_offset_far_above_their_spread(ops, pred, phi):
    """out_c = 3 + 0.05 N(0,1), out_u = 3 + 0.05 N(0,1) at scale 7.5: a one-pass fp32 E[x^2] - E[x]^2 is about 1e-4 off here,
    a centred form is not."""
    shape = SHAPES["2x4x33x37"]
    rng = np.random.RandomState(21)
    outs = 3.0 + 0.05 * rng.standard_normal(shape), 3.0 + 0.05 * rng.standard_normal(shape)
    a = _case(shape, pred, 1, 0.3, True, seed=22, scale=7.5, outputs=outs)
    _check_step(f"step_rescale_offset_pred{pred}_phi{phi}", _launch(ops, a, phi), _reference(a, phi))


@pytest.mark.parametrize("pred", [0, 1])
def test_constant_outputs_give_factor_one(ops, pred):
    """out_u == out_c == a constant: std(m) = 0, f = 1, and the outputs are the pred entry's."""
    shape = SHAPES["3x4x5x7"]
    const = np.full(shape, 0.375, np.float32)
    a = _case(shape, pred, 1, 0.3, True, seed=23, outputs=(const, const))
    got = _launch(ops, a, 0.7)
    want = _launch(ops, a, None, entry="pred")
    assert torch.equal(got[3], torch.ones_like(got[3]))
    for g, w, name in zip(got[:3], want[:3], "xpe"):
        assert bool(torch.isfinite(g).all())
        print("CONSTANT", pred, name, "max|d|", float((g - w).abs().max()))
        assert torch.equal(g, w), name


@pytest.mark.parametrize("pred", [0, 1])
def test_no_rescale_is_bit_identical_to_the_pred_entry(ops, pred):
    """guidance_rescale = 0, and out_u = NULL with any guidance_rescale: ops.sampler_step_pred's results, factor_out = 1."""
    a = _case(SHAPES["3x4x5x7"], pred, 3, 0.3, True, seed=24)
    for phi, no_u in ((0.0, False), (0.0, True), (0.7, True), (1.0, True)):
        want = _launch(ops, a, None, entry="pred", no_u=no_u)
        got = _launch(ops, a, phi, no_u=no_u)
        assert all(torch.equal(g, w) for g, w in zip(got[:3], want[:3])), (phi, no_u)
        assert torch.equal(got[3], torch.ones_like(got[3])), (phi, no_u)
    rescaled = _launch(ops, a, 0.7)
    assert not torch.equal(rescaled[0], _launch(ops, a, None, entry="pred")[0])


def test_sampler_step_rescale_aliasing(ops):
    """x_prev == x_model (the second call of the PLMS first step) and x_prev == x give exactly the non-aliased results."""
    eq = lambda got, ref: all(torch.equal(g, r) for g, r in zip(got, ref))
    for shape in ("3x4x5x7", "2x4x33x37"):
        a = _case(SHAPES[shape], 1, 1, 0.3, True, seed=25)
        ref = _launch(ops, a, 0.7)
        xm_t = dev32(a["xm"])
        got = _launch(ops, a, 0.7, xm_t=xm_t, x_prev=xm_t)
        assert got[0] is xm_t and eq(got, ref)
        x_t = dev32(a["x"])
        got = _launch(ops, a, 0.7, x_t=x_t, x_prev=x_t)
        assert got[0] is x_t and eq(got, ref)
        # x_model == NULL with x_prev == x: both aliases at once
        b = _case(SHAPES[shape], 1, 1, 0.3, False, seed=25)
        ref = _launch(ops, b, 0.7)
        x_t = dev32(b["x"])
        assert eq(_launch(ops, b, 0.7, x_t=x_t, x_prev=x_t), ref)


# --------------------------------------------------------------------------------------- samplers vs RescaleModelOracle
@pytest.fixture(scope="module")
def tiny():
    """One tiny UNet (hipGraph on) read as a v model and as an eps model, and the oracles over the same weights."""
    v_model, cfg, params = V.tiny_eps_model(parameterization="v")
    eps_model, _, _ = V.tiny_eps_model()
    net = O.UNetOracle(dict(cfg, num_heads=-1), params)
    return {"v": (v_model, V.VModelOracle(net)), "eps": (eps_model, O.ModelOracle(net))}, cfg


@pytest.mark.parametrize("phi", R.PHIS)
@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("kind", ["v", "eps"])
def test_rescaled_trajectory_vs_oracle(tiny, kind, name, phi):
    models, cfg = tiny
    model, base = models[kind]
    got = R.product_trajectory(name, model, cfg["context_dim"], DEV, guidance_rescale=phi)
    ref = R.oracle_trajectory(name, base, cfg["context_dim"], phi)
    check(f"tiny_{kind}_rescale{phi}_{name}", got, ref, rel_l2=1e-2, max_rel=1e-2)


@pytest.mark.parametrize("kind", ["v", "eps"])
def test_zero_rescale_and_unguided_runs_never_reach_the_new_entry(tiny, ops, monkeypatch, kind):
    """guidance_rescale = 0.0, and runs without guidance at any guidance_rescale, make the calls they always made."""
    models, cfg = tiny
    model = models[kind][0]
    guided, unguided = ("ddim_S5_scale3.0", "plms_S5_scale3.0", "dpm_S10_scale7.5"), ("ddim_S4_scale1.0", "dpm_S15_scale1.0")
    want = {name: V.product_trajectory(name, model, cfg["context_dim"], DEV) for name in guided + unguided}

    def refuse(*a, **k):
        raise AssertionError("no rescale: must not go through ops.sampler_step_rescale")
    monkeypatch.setattr(ops, "sampler_step_rescale", refuse)
    for name in guided:
        assert torch.equal(R.product_trajectory(name, model, cfg["context_dim"], DEV, guidance_rescale=0.0), want[name]), name
    for name in unguided:
        assert torch.equal(R.product_trajectory(name, model, cfg["context_dim"], DEV, guidance_rescale=0.7), want[name]), name


@pytest.mark.parametrize("name", ["ddim_S5_scale3.0", "plms_S5_scale3.0"])
def test_rescale_with_an_identity_score_corrector(tiny, name):
    """The rescale belongs to the combine that produces e_t (pass 1), so an identity corrector changes nothing but the fp16
    round trip of e_t; modify_score is called once per model evaluation."""
    models, cfg = tiny
    model = models["eps"][0]

    class Identity:
        calls = 0

        def modify_score(self, model, e_t, x, t, c, **kw):
            self.calls += 1
            return e_t
    corr = Identity()
    plain = R.product_trajectory(name, model, cfg["context_dim"], DEV, guidance_rescale=0.7)
    got = R.product_trajectory(name, model, cfg["context_dim"], DEV, guidance_rescale=0.7, score_corrector=corr)
    assert corr.calls == V.TRAJECTORIES[name][1] + int(name.startswith("plms"))
    check(f"tiny_eps_rescale0.7_corrector_{name}", got, plain, rel_l2=1e-2)


def test_pipeline_forwards_guidance_rescale(tiny):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.pipeline import DiffusionPipeline
    models, cfg = tiny
    model, base = models["v"]
    x_T, c, uc = V.tiny_inputs(cfg["context_dim"])
    c16, uc16 = torch.tensor(c, device=DEV).half(), torch.tensor(uc, device=DEV).half()    # the pipeline hands fp16 contexts on
    got = DiffusionPipeline(model, "ddim", device=DEV)(c=torch.tensor(c), uc=torch.tensor(uc), H=64, W=64, steps=5, scale=3.0,
                                                       x_T=torch.tensor(x_T), guidance_rescale=0.7)
    direct, _ = DDIMSampler(model).sample(5, V.B, (4, V.H, V.W), conditioning=c16, x_T=torch.tensor(x_T, device=DEV),
                                          unconditional_guidance_scale=3.0, unconditional_conditioning=uc16, verbose=False,
                                          guidance_rescale=0.7)
    assert torch.equal(got, direct)
    unrescaled = DiffusionPipeline(model, "ddim", device=DEV)(c=torch.tensor(c), uc=torch.tensor(uc), H=64, W=64, steps=5,
                                                              scale=3.0, x_T=torch.tensor(x_T))
    assert not torch.equal(got, unrescaled)
    check("tiny_v_rescale0.7_pipeline_ddim_S5", got, R.oracle_trajectory("ddim_S5_scale3.0", base, cfg["context_dim"], 0.7),
          rel_l2=1e-2, max_rel=1e-2)
