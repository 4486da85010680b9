"""v-prediction on the GPU: mdx_sampler_step_pred_f32 against numpy, its aliasing and bit-identity contracts, and the three
samplers on a `parameterization: "v"` model against VModelOracle (tests/_vpred_util.py).

Tolerances: the kernel is fp32 elementwise arithmetic on given inputs -> rel-L2 1e-5 (test_sampler_step's bound).
Trajectories: the project's bound for 5 / 10-step tiny-UNet runs, rel-L2 <= 1e-2 and max|d| <= 1e-2 max|ref| (see
test_unet_gpu.py); test_vpred_cpu.py checks that the oracle's own fp32 and fp16-emulated runs of every case stay inside it.
"""
import os

import numpy as np
import pytest
import torch

import _vpred_util as V
from _util import check, h16
from oracle import ldm as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def dev32(a):
    return torch.tensor(np.asarray(a, np.float32), device=DEV)


def out_buf(e, ld=8):
    """NCHW values -> the UNet's NHWC fp16 output layout [B][HW][ld]; the pad channels hold a value that must not be read."""
    B, C, H, W = e.shape
    buf = np.full((B, H * W, ld), 1e4, np.float32)
    buf[:, :, :C] = e.transpose(0, 2, 3, 1).reshape(B, H * W, C)
    return torch.tensor(buf, dtype=torch.float16, device=DEV)


COEF = {0: (1, 0, 0, 0), 1: (1.5, -0.5, 0, 0), 3: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}


def _case(shape, cfg, order, sigma, separate_xm, seed):
    """Inputs and the numpy (fp32 inputs, float64 arithmetic) result of one MDX_PRED_V step."""
    rng = np.random.RandomState(seed)
    B, C, H, W = shape
    x = rng.standard_normal(shape).astype(np.float32)
    xm = rng.standard_normal(shape).astype(np.float32) if separate_xm else x
    vu, vc = h16(rng.standard_normal(shape)), h16(rng.standard_normal(shape))
    olds = [rng.standard_normal(shape).astype(np.float32) for _ in range(order)]
    noise = rng.standard_normal(shape).astype(np.float32)
    scale = 7.5
    a_t, a_prev = np.float32(0.3), np.float32(0.5)
    # the model's own point: another timestep than the update's when x_model is a distinct tensor (the PLMS first step)
    am, bm = (np.float32(np.sqrt(0.4)), np.float32(np.sqrt(0.6))) if separate_xm else (np.sqrt(a_t), np.sqrt(1 - a_t))
    f = np.float64
    m = vu.astype(f) + scale * (vc.astype(f) - vu.astype(f)) if cfg else vc.astype(f)
    e_t = f(am) * m + f(bm) * xm.astype(f)
    ep = COEF[order][0] * e_t + sum(c * o.astype(f) for c, o in zip(COEF[order][1:], olds))
    px0 = (x.astype(f) - f(np.sqrt(1 - a_t)) * ep) / f(np.sqrt(a_t))
    dirc = np.sqrt(1 - a_prev - np.float32(sigma) ** 2)
    xp = f(np.sqrt(a_prev)) * px0 + f(dirc) * ep + f(np.float32(sigma)) * noise.astype(f)
    args = dict(x=x, xm=xm, vu=vu if cfg else None, vc=vc, olds=olds, coef=COEF[order], scale=scale, am=am, bm=bm,
                scalars=(np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_prev), dirc, np.float32(sigma)),
                noise=noise if sigma else None)
    return args, (xp, px0, e_t)


def _launch(ops, a, pred=1, xm="given", x_prev=None, x_t=None, xm_t=None):
    """Run the new entry; xm: "given" (a distinct device tensor, or None when the case shares x) | None.
    x_t / xm_t / x_prev: preallocated device tensors (to alias them)."""
    xd = dev32(a["x"]) if x_t is None else x_t
    if xm_t is not None:
        xmd = xm_t
    elif xm is None or a["xm"] is a["x"]:
        xmd = None
    else:
        xmd = dev32(a["xm"])
    e_out, p_out = torch.empty_like(xd), torch.empty_like(xd)
    x_out = torch.empty_like(xd) if x_prev is None else x_prev
    ops.sampler_step_pred(xd, xmd, None if a["vu"] is None else out_buf(a["vu"]), out_buf(a["vc"]), 8, a["scale"], pred,
                          a["am"], a["bm"], [dev32(o) for o in a["olds"]], a["coef"], *a["scalars"],
                          None if a["noise"] is None else dev32(a["noise"]), e_out, x_out, p_out)
    torch.cuda.synchronize()
    return x_out, p_out, e_out


SMALL = (2, 4, 5, 7)      # 280 elements: a ragged last block, and a C * HW boundary (140) inside block 0


@pytest.mark.parametrize("separate_xm", [False, True])
@pytest.mark.parametrize("sigma", [0.0, 0.3])
@pytest.mark.parametrize("order", [0, 1, 3])
@pytest.mark.parametrize("cfg", [True, False])
def test_sampler_step_pred_vs_numpy(ops, cfg, order, sigma, separate_xm):
    a, (xp, px0, e_t) = _case(SMALL, cfg, order, sigma, separate_xm, seed=order + 2 * int(cfg))
    x_out, p_out, e_out = _launch(ops, a)
    tag = f"sampler_step_pred_cfg{int(cfg)}_o{order}_s{sigma}_xm{int(separate_xm)}"
    check(tag + "_x", x_out, xp, rel_l2=1e-5)
    check(tag + "_p", p_out, px0, rel_l2=1e-5)
    check(tag + "_e", e_out, e_t, rel_l2=1e-5)


def test_sampler_step_pred_grid_stride_loop(ops):
    """2 x 4 x 264 x 264 = 557 568 elements > 2048 blocks x 256 threads: the grid-stride loop takes a second pass."""
    a, (xp, px0, e_t) = _case((2, 4, 264, 264), True, 3, 0.3, True, seed=9)
    x_out, p_out, e_out = _launch(ops, a)
    check("sampler_step_pred_264x264_x", x_out, xp, rel_l2=1e-5)
    check("sampler_step_pred_264x264_p", p_out, px0, rel_l2=1e-5)
    check("sampler_step_pred_264x264_e", e_out, e_t, rel_l2=1e-5)


def test_sampler_step_pred_aliasing(ops):
    """x_prev == x_model (the second call of the PLMS first step) and x_prev == x give exactly the non-aliased results."""
    a, _ = _case(SMALL, True, 1, 0.3, True, seed=4)
    x_ref, p_ref, e_ref = _launch(ops, a)
    xm_t = dev32(a["xm"])
    x_out, p_out, e_out = _launch(ops, a, xm_t=xm_t, x_prev=xm_t)
    assert x_out is xm_t and torch.equal(x_out, x_ref) and torch.equal(p_out, p_ref) and torch.equal(e_out, e_ref)
    x_t = dev32(a["x"])
    x_out, p_out, e_out = _launch(ops, a, x_t=x_t, x_prev=x_t)
    assert x_out is x_t and torch.equal(x_out, x_ref) and torch.equal(p_out, p_ref) and torch.equal(e_out, e_ref)
    # x_model == NULL with x_prev == x: both aliases at once
    b, _ = _case(SMALL, True, 1, 0.3, False, seed=4)
    x_ref, p_ref, e_ref = _launch(ops, b)
    x_t = dev32(b["x"])
    x_out, p_out, e_out = _launch(ops, b, x_t=x_t, x_prev=x_t)
    assert torch.equal(x_out, x_ref) and torch.equal(p_out, p_ref) and torch.equal(e_out, e_ref)


def test_pred_eps_entry_is_bit_identical_to_sampler_step(ops):
    """CFG / order 3 / noise: MDX_PRED_EPS through the new entry == ops.sampler_step, bit for bit (x_model NULL or not)."""
    a, _ = _case(SMALL, True, 3, 0.3, True, seed=5)
    xd = dev32(a["x"])
    e0, x0, p0 = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)
    ops.sampler_step(xd, out_buf(a["vu"]), out_buf(a["vc"]), 8, a["scale"], [dev32(o) for o in a["olds"]], a["coef"],
                     *a["scalars"], dev32(a["noise"]), e0, x0, p0)
    for xm in (None, "given"):
        x1, p1, e1 = _launch(ops, a, pred=ops.PRED_EPS, xm=xm)
        assert torch.equal(x1, x0) and torch.equal(p1, p0) and torch.equal(e1, e0)
    x2, _, _ = _launch(ops, a, pred=ops.PRED_V)
    assert not torch.equal(x2, x0)


def test_eps_sampler_runs_do_not_depend_on_the_new_entry(ops, monkeypatch):
    """An "eps" model never reaches mdx_sampler_step_pred_f32: all three samplers keep calling the old entry, whose host code
    fills MDX_PRED_EPS into the same kernel body it always launched."""
    def refuse(*a, **k):
        raise AssertionError("an eps model must go through ops.sampler_step")
    model, cfg, _ = V.tiny_eps_model()
    want = {name: V.product_trajectory(name, model, cfg["context_dim"], DEV) for name in V.EPS_IDENTITY_CASES}
    monkeypatch.setattr(ops, "sampler_step_pred", refuse)
    for name in V.EPS_IDENTITY_CASES:
        assert torch.equal(V.product_trajectory(name, model, cfg["context_dim"], DEV), want[name]), name


def test_eps_sampler_runs_are_bit_identical_to_the_parent_commit():
    """tests/golden/vpred_eps_parent.npz: the final latents of short "eps" tiny-UNet runs of all three samplers (hipGraph on),
    recorded on an MI355X with the library of the commit before mdx_sampler_step_pred_f32 existed
    (tests/golden/make_vpred_eps_golden.py says how to record it again)."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "vpred_eps_parent.npz"))
    model, cfg, _ = V.tiny_eps_model()
    assert sorted(gold.files) == sorted(V.EPS_IDENTITY_CASES)
    for name in V.EPS_IDENTITY_CASES:
        got = V.product_trajectory(name, model, cfg["context_dim"], DEV)
        assert torch.equal(got.cpu(), torch.tensor(gold[name])), name


def test_closed_form_pred_x0(ops):
    """coef = (1, 0, 0, 0), x_model = x, a^2 + b^2 = 1 at the update's own point: pred_x0 = a x - b v."""
    rng = np.random.RandomState(6)
    x = rng.standard_normal(SMALL).astype(np.float32)
    v = h16(rng.standard_normal(SMALL))
    a, b = np.float32(np.sqrt(0.3)), np.float32(np.sqrt(0.7))
    xd = dev32(x)
    x_out, p_out = torch.empty_like(xd), torch.empty_like(xd)
    ops.sampler_step_pred(xd, None, None, out_buf(v), 8, 1.0, ops.PRED_V, a, b, [], (1, 0, 0, 0), a, b, 1.0, 0.0, 0.0, None,
                          None, x_out, p_out)
    check("sampler_step_pred_closed_form_pred_x0", p_out, np.float64(a) * x - np.float64(b) * v, rel_l2=1e-5)
    check("sampler_step_pred_closed_form_x_prev", x_out, np.float64(a) * x - np.float64(b) * v, rel_l2=1e-5)


# --------------------------------------------------------------------------------------------- samplers vs VModelOracle
@pytest.fixture(scope="module")
def tiny_v():
    """One tiny UNet (hipGraph on) as a v model, and the oracle that reads the same weights' output as v."""
    model, cfg, params = V.tiny_eps_model(parameterization="v")
    assert model.parameterization == "v"
    om = V.VModelOracle(O.UNetOracle(dict(cfg, num_heads=-1), params))
    return model, om, cfg


@pytest.fixture(scope="module")
def oracle_refs(tiny_v):
    """Each case's oracle end point, computed once and shared."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = V.oracle_trajectory(name, tiny_v[1], tiny_v[2]["context_dim"])
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(V.TRAJECTORIES))
def test_v_trajectory_vs_oracle(tiny_v, oracle_refs, name):
    model, _, cfg = tiny_v
    got = V.product_trajectory(name, model, cfg["context_dim"], DEV)
    check(f"tiny_v_{name}", got, oracle_refs(name), rel_l2=1e-2, max_rel=1e-2)


def test_v_model_is_not_the_eps_model(tiny_v, oracle_refs):
    """The same weights read as eps end somewhere else entirely: the trajectory bound above does discriminate."""
    model, _, cfg = tiny_v
    model.parameterization = "eps"
    try:
        eps = V.product_trajectory("ddim_S5_scale3.0", model, cfg["context_dim"], DEV)
    finally:
        model.parameterization = "v"
    ref = oracle_refs("ddim_S5_scale3.0")
    assert float((eps.cpu() - ref).norm() / ref.norm()) > 0.1


class _ApplyModelOnly:
    """A model object in the reference's calling convention only: apply_model(x, t, cond) -> NCHW v, plus the schedule."""

    def __init__(self, ldm):
        self._ldm = ldm
        self.parameterization = "v"
        for k in ("num_timesteps", "betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod",
                  "sqrt_one_minus_alphas_cumprod"):
            setattr(self, k, getattr(ldm, k))
        self.calls = 0

    def apply_model(self, x, t, cond):
        self.calls += 1
        return self._ldm.apply_model(x, t, cond)


@pytest.mark.parametrize("name", ["ddim_S5_scale3.0", "plms_S5_scale3.0", "dpm_S10_scale7.5"])
def test_v_generic_apply_model_path(tiny_v, oracle_refs, name):
    model, _, cfg = tiny_v
    generic = _ApplyModelOnly(model)
    got = V.product_trajectory(name, generic, cfg["context_dim"], DEV)
    S = V.TRAJECTORIES[name][1]
    assert generic.calls == S + (name.startswith("plms"))
    check(f"tiny_v_generic_{name}", got, oracle_refs(name), rel_l2=1e-2, max_rel=1e-2)
    fast = V.product_trajectory(name, model, cfg["context_dim"], DEV)
    check(f"tiny_v_generic_vs_fast_{name}", got, fast, rel_l2=1e-2, max_rel=1e-2)


def test_v_pipeline_needs_no_change(tiny_v, oracle_refs):
    """DiffusionPipeline only hands the model to a sampler, which reads model.parameterization."""
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model, _, cfg = tiny_v
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    x_T, c, uc = V.tiny_inputs(cfg["context_dim"])
    c16, uc16 = torch.tensor(c, device=DEV).half(), torch.tensor(uc, device=DEV).half()    # the pipeline hands fp16 contexts on
    got = DiffusionPipeline(model, "ddim", device=DEV)(c=torch.tensor(c), uc=torch.tensor(uc), H=64, W=64, steps=5, scale=3.0,
                                                       x_T=torch.tensor(x_T))
    direct, _ = DDIMSampler(model).sample(5, V.B, (4, V.H, V.W), conditioning=c16, x_T=torch.tensor(x_T, device=DEV),
                                          unconditional_guidance_scale=3.0, unconditional_conditioning=uc16, verbose=False)
    assert torch.equal(got, direct)
    check("tiny_v_pipeline_ddim_S5", got, oracle_refs("ddim_S5_scale3.0"), rel_l2=1e-2, max_rel=1e-2)


def test_score_corrector_still_needs_eps(tiny_v):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    model, _, cfg = tiny_v
    x_T, c, _ = V.tiny_inputs(cfg["context_dim"])

    class Corrector:
        def modify_score(self, *a, **k):
            raise RuntimeError("must not be reached")
    with pytest.raises(AssertionError, match="eps"):
        DDIMSampler(model).sample(2, V.B, (4, V.H, V.W), conditioning=torch.tensor(c, device=DEV),
                                  x_T=torch.tensor(x_T, device=DEV), verbose=False, score_corrector=Corrector())


@pytest.mark.parametrize("sampler", ["ddim", "plms"])
def test_one_step_run_of_an_eps_model(sampler):
    """S = 1: the timestep grid has one element, whose flipped view keeps a negative stride (torch refuses such an array, so
    plms_sampling copies it).  Any parameterization took that path; "eps" on the tiny UNet against the oracle, t = 1, so the
    bound is a single UNet call's (rel-L2 5e-3, test_unet_gpu.py)."""
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    model, cfg, params = V.tiny_eps_model()
    om = O.ModelOracle(O.UNetOracle(dict(cfg, num_heads=-1), params))
    x_T, c, uc = V.tiny_inputs(cfg["context_dim"])
    ref, _ = O.sample(om, 1, V.B, (4, V.H, V.W), c, x_T, sampler, unconditional_guidance_scale=3.0,
                      unconditional_conditioning=uc)
    cls = DDIMSampler if sampler == "ddim" else PLMSSampler
    d = lambda a: torch.tensor(a, device=DEV)
    got, inter = cls(model).sample(1, V.B, (4, V.H, V.W), conditioning=d(c), x_T=d(x_T), unconditional_guidance_scale=3.0,
                                   unconditional_conditioning=d(uc), verbose=False)
    assert len(inter["x_inter"]) == 2
    check(f"tiny_eps_{sampler}_S1", got, ref, rel_l2=5e-3)


def test_sd2_768v_single_ddim_step():
    """SD2_UNET + SD2_768V_LDM on a 96x96 latent, B = 1: the FIRST step of a 2-step DDIM run (t = 501, a = 0.52, b = 0.85, so
    the conversion carries the result) through the sampler, the per-run time-embedding table and the hipGraph, against one
    get_x_prev_and_pred_x0 (plms.py:210-228, as oracle.ldm.sample applies it) on VModelOracle's output -- one 2.15-TFLOP oracle
    evaluation on the host.  Tolerance: test_sd2_768_single_step's.  The same run read as "eps" must fall outside it."""
    from _util import metrics
    from minddiffusion_amd.configs import SD2_768V_LDM, SD2_UNET
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    torch.set_num_threads(min(32, os.cpu_count() or 8))
    params = O.init_params(O.SD2_UNET, seed=1)
    net = UNetModel(**SD2_UNET)
    net.use_graph = True
    net.load_state_dict(params)
    model = LatentDiffusion(unet_config=net, **SD2_768V_LDM)
    assert model.parameterization == "v" and model.image_size == 96
    om = V.VModelOracle(O.UNetOracle(O.SD2_UNET, params))
    x_T = np.random.RandomState(43).randn(1, 4, 96, 96).astype(np.float32)
    c = np.random.RandomState(2).randn(1, 77, 1024).astype(np.float32)
    ts = O.make_ddim_timesteps(2, om.num_timesteps)                       # [1, 501]
    _, alphas, alphas_prev = O.make_ddim_sampling_parameters(om.alphas_cumprod, ts, 0.0)
    a_t, a_prev = torch.tensor(alphas[1]), torch.tensor(alphas_prev[1])
    x = torch.tensor(x_T)
    e = om.apply_model(x, torch.full((1,), int(ts[1]), dtype=torch.int64), torch.tensor(c))
    ref_p = (x - (1.0 - a_t).sqrt() * e) / a_t.sqrt()
    ref_x = a_prev.sqrt() * ref_p + (1.0 - a_prev).sqrt() * e

    def first_step():
        _, inter = DDIMSampler(model).sample(2, 1, (4, 96, 96), conditioning=torch.tensor(c, device=DEV),
                                             x_T=torch.tensor(x_T, device=DEV), verbose=False, log_every_t=1)
        assert len(inter["x_inter"]) == 3
        return inter["x_inter"][1], inter["pred_x0"][1]
    got_x, got_p = first_step()
    check("sd2_768v_single_ddim_step_B1_96x96", got_x, ref_x, rel_l2=5e-3, max_abs=5e-2)
    check("sd2_768v_single_ddim_step_B1_96x96_pred_x0", got_p, ref_p, rel_l2=5e-3, max_abs=5e-2)
    model.parameterization = "eps"
    eps_x, _ = first_step()
    assert metrics(eps_x, ref_x)["rel_l2"] > 5e-2
