"""img2img on the GPU: mdx_q_sample_f32 and mdx_vae_encode_noised_f32 against float64 numpy and their bit-level contracts,
the identity of decode(t_start = S) with sample(), partial runs of all three samplers against the oracle
(tests/_img2img_util.py), the launch count of the masked path, and DiffusionPipeline.img2img end to end.

Tolerances: the kernels are fp32 elementwise arithmetic on given inputs -> rel-L2 1e-5 (test_sampler_step's bound).
Trajectories: the project's bound for short tiny-UNet runs, rel-L2 <= 1e-2 and max|d| <= 1e-2 max|ref|; test_img2img_cpu.py
checks that the oracle's own fp32 and fp16-emulated runs of every case stay inside it.
"""
import os

import numpy as np
import pytest
import torch

import _img2img_util as I
import _vpred_util as V
from _util import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from minddiffusion_amd import ops as _ops
    return _ops


def dev32(a, misaligned=False):
    """Device copy of `a`; misaligned: a contiguous view that starts one float past a 16-byte boundary."""
    a = np.ascontiguousarray(a, np.float32)
    if not misaligned:
        return torch.tensor(a, device=DEV)
    flat = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    view = flat[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ mdx_q_sample_f32
A, Bc = np.float32(0.8366), np.float32(0.5478)
# 3x4x5x7: odd HW, less than a wave per channel plane; 2x4x33x37: HW % 4 != 0, several blocks; 1x4x64x64: the latent size,
# float4 path (scalar when misaligned).
SHAPES = [(3, 4, 5, 7), (2, 4, 33, 37), (1, 4, 64, 64)]
# larger than one pass of the capped grid: 4096 blocks x 64 lanes x 4 floats = 1 048 576 elements on the float4 path, 262 144
# on the scalar one (which misaligned or HW % 4 != 0 inputs take)
BIG_VEC, BIG_SCALAR = (2, 4, 384, 384), (1, 4, 257, 257)


def _q_case(shape, mask_mode, mask_kind, seed):
    """Inputs and the float64 result.  Every sample has its own values (mask included), so a batch-index mix-up shows."""
    rng = np.random.RandomState(seed)
    Bn, C, Hh, Ww = shape
    x0, nz, img = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    f = np.float64
    q = f(A) * x0.astype(f) + f(Bc) * nz.astype(f)
    if mask_mode == 0:
        return dict(x0=x0, nz=nz, img=None, mask=None), q
    mshape = (Bn, 1 if mask_mode == 1 else C, Hh, Ww)
    m = rng.rand(*mshape)
    m = (m > 0.5).astype(np.float32) if mask_kind == "binary" else m.astype(np.float32)
    return dict(x0=x0, nz=nz, img=img, mask=m), m.astype(f) * q + (1.0 - m.astype(f)) * img.astype(f)


def _q_launch(ops, a, misaligned=False, out=None, img_t=None, ab=(A, Bc)):
    d = lambda v: None if v is None else dev32(v, misaligned)
    img = d(a["img"]) if img_t is None else img_t
    if out is None:
        out = dev32(np.zeros(a["x0"].shape, np.float32), misaligned)
    res = ops.q_sample(d(a["x0"]), d(a["nz"]), ab[0], ab[1], out=out, mask=d(a["mask"]), img=img)
    torch.cuda.synchronize()
    assert res is out
    return out


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("mask_mode", [0, 1, "C"])
@pytest.mark.parametrize("shape", SHAPES)
def test_q_sample_vs_numpy(ops, shape, mask_mode, misaligned):
    kinds = ("binary", "fractional") if mask_mode else ("none",)
    for k, kind in enumerate(kinds):
        a, ref = _q_case(shape, mask_mode, kind, seed=11 + k)
        got = _q_launch(ops, a, misaligned)
        check(f"q_sample_{'x'.join(map(str, shape))}_mask{mask_mode}_{kind}_mis{int(misaligned)}", got, ref, rel_l2=1e-5)


@pytest.mark.parametrize("shape,misaligned", [(BIG_VEC, False), (BIG_SCALAR, False), (BIG_SCALAR, True)])
def test_q_sample_grid_stride_loop(ops, shape, misaligned):
    """More elements than one pass of the capped grid covers, on the float4 and on the scalar path (one mask plane per sample:
    the index arithmetic of the later passes)."""
    a, ref = _q_case(shape, 1, "fractional", seed=13)
    got = _q_launch(ops, a, misaligned)
    check(f"q_sample_{'x'.join(map(str, shape))}_mis{int(misaligned)}", got, ref, rel_l2=1e-5)


@pytest.mark.parametrize("shape,misaligned", [((1, 4, 64, 64), False), ((1, 4, 64, 64), True), ((3, 4, 5, 7), False)])
@pytest.mark.parametrize("mask_mode", [1, "C"])
def test_q_sample_bit_level_contracts(ops, shape, misaligned, mask_mode):
    """m == 0 -> out is img bit for bit; m == 1 -> out is the unmasked launch's q; a = 1, b = 0 without a mask -> x0."""
    a, _ = _q_case(shape, mask_mode, "binary", seed=17)
    q = _q_launch(ops, dict(a, mask=None, img=None), misaligned)
    got = _q_launch(ops, a, misaligned)
    m = torch.tensor(np.broadcast_to(a["mask"], shape).copy(), device=DEV)
    img = torch.tensor(a["img"], device=DEV)
    assert 0 < int((m == 0).sum()) < m.numel()
    assert torch.equal(bits(got)[m == 0], bits(img)[m == 0])
    assert torch.equal(got[m == 1], q[m == 1])
    same = _q_launch(ops, dict(a, mask=None, img=None), misaligned, ab=(1.0, 0.0))
    assert torch.equal(same, torch.tensor(a["x0"], device=DEV))
    # all-ones / all-zeros masks: the whole tensor
    ones = _q_launch(ops, dict(a, mask=np.ones_like(a["mask"])), misaligned)
    zeros = _q_launch(ops, dict(a, mask=np.zeros_like(a["mask"])), misaligned)
    assert torch.equal(ones, q) and torch.equal(bits(zeros), bits(img))


@pytest.mark.parametrize("shape,misaligned", [((1, 4, 64, 64), False), ((2, 4, 33, 37), False), ((1, 4, 64, 64), True)])
def test_q_sample_out_aliasing_img(ops, shape, misaligned):
    a, _ = _q_case(shape, 1, "fractional", seed=19)
    want = _q_launch(ops, a, misaligned)
    img_t = dev32(a["img"], misaligned)
    got = _q_launch(ops, a, misaligned, out=img_t, img_t=img_t)
    assert got is img_t and torch.equal(got, want)


def test_q_sample_wrapper_refuses_bad_tensors(ops):
    from minddiffusion_amd._lib import MdxError
    x = torch.zeros(2, 4, 5, 7, device=DEV)
    with pytest.raises(MdxError, match="noise"):
        ops.q_sample(x, torch.zeros(2, 4, 5, 8, device=DEV), 1.0, 0.0)
    with pytest.raises(MdxError, match="mask"):
        ops.q_sample(x, x.clone(), 1.0, 0.0, mask=torch.zeros(1, 1, 5, 7, device=DEV), img=x.clone())
    with pytest.raises(MdxError, match="mask_c"):
        ops.q_sample(x, x.clone(), 1.0, 0.0, mask=torch.zeros(2, 2, 5, 7, device=DEV), img=x.clone())
    with pytest.raises(MdxError, match="may alias img"):
        ops.q_sample(x, x.clone(), 1.0, 0.0, out=x)
    with pytest.raises(MdxError, match="GPU"):
        ops.q_sample(x.cpu(), x.clone(), 1.0, 0.0)


# ------------------------------------------------------------------------------------------------ mdx_vae_encode_noised_f32
SCALE = np.float32(0.18215)


def _enc_case(shape, seed):
    """Moments in an ld = 8 NHWC fp16 buffer: zc = 3 mean and 3 logvar channels, two pad channels holding 1e4 (never read);
    logvar values beyond both clip ends ([-30, 20])."""
    rng = np.random.RandomState(seed)
    Bn, zc, Hh, Ww = shape
    HW = Hh * Ww
    mean = rng.standard_normal((Bn, HW, zc)).astype(np.float16)
    logvar = (3.0 * rng.standard_normal((Bn, HW, zc))).astype(np.float16)
    logvar[:, 0::5, 0], logvar[:, 1::5, 1], logvar[:, 2::5, 2] = -40.0, 30.0, 25.0
    buf = np.full((Bn, HW, 8), 1e4, np.float16)
    buf[:, :, :zc], buf[:, :, zc:2 * zc] = mean, logvar
    pn, nz = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    f = np.float64
    nchw = lambda t: t.astype(f).transpose(0, 2, 1).reshape(shape)
    std = np.exp(0.5 * np.clip(nchw(logvar), -30.0, 20.0))
    z = {True: nchw(mean) + std * pn.astype(f), False: nchw(mean)}
    return dict(mom=torch.tensor(buf, device=DEV), pn=pn, nz=nz), z


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 3, 8, 8), (1, 3, 33, 36)])
def test_vae_encode_noised_vs_numpy_and_its_two_ties(ops, shape, misaligned):
    a, z = _enc_case(shape, seed=23)
    f = np.float64
    empty = lambda: dev32(np.zeros(shape, np.float32), misaligned)
    pn, nz = dev32(a["pn"], misaligned), dev32(a["nz"], misaligned)
    tag = f"vae_encode_noised_{'x'.join(map(str, shape))}_mis{int(misaligned)}"
    for sample in (True, False):
        z0, xt = ops.vae_encode_noised(a["mom"], 3, pn if sample else None, SCALE, A, Bc, nz, empty(), empty())
        ref0 = f(SCALE) * z[sample]
        check(f"{tag}_sample{int(sample)}_z0", z0, ref0, rel_l2=1e-5)
        check(f"{tag}_sample{int(sample)}_xt", xt, f(A) * ref0 + f(Bc) * a["nz"].astype(f), rel_l2=1e-5)
        # tie 2: xt is mdx_q_sample_f32 of z0_out
        assert torch.equal(xt, ops.q_sample(z0.contiguous(), nz, A, Bc))
        # each output alone
        only0, none = ops.vae_encode_noised(a["mom"], 3, pn if sample else None, SCALE, A, Bc, None, empty(), None)
        assert none is None and torch.equal(only0, z0)
        none, onlyt = ops.vae_encode_noised(a["mom"], 3, pn if sample else None, SCALE, A, Bc, nz, None, empty())
        assert none is None and torch.equal(onlyt, xt)
        # tie 1: scale_factor = 1, no xt_out -> mdx_vae_gaussian_sample_f32's output
        z1, _ = ops.vae_encode_noised(a["mom"], 3, pn if sample else None, 1.0, A, Bc, None, empty(), None)
        g = ops.vae_gaussian_sample(a["mom"], 3, pn if sample else None, empty())
        torch.cuda.synchronize()
        assert torch.equal(z1, g)


# ------------------------------------------------------------------------------------------------ identity with the existing path
@pytest.fixture(scope="module")
def tiny():
    """One tiny UNet (hipGraph on) as an eps model and as a v model over the same weights, with their oracles."""
    model, cfg, params = V.tiny_eps_model()
    vmodel, _, _ = V.tiny_eps_model(parameterization="v")
    return {"eps": model, "v": vmodel, "cfg": cfg,
            "o_eps": I.oracle_model("eps", cfg, params), "o_v": I.oracle_model("v", cfg, params)}


@pytest.mark.parametrize("kind", ["ddim", "plms"])
def test_decode_from_the_top_is_sample(tiny, kind):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    cls = DDIMSampler if kind == "ddim" else PLMSSampler
    x_T, c, uc = V.tiny_inputs(tiny["cfg"]["context_dim"])
    d = lambda a: torch.tensor(a, device=DEV)
    S = 5
    for eta, extra in ((0., {}), (0.6, {"step_noises": V.step_noises(S)})) if kind == "ddim" else ((0., {}),):
        want, winter = cls(tiny["eps"]).sample(S, V.B, I.SHAPE, conditioning=d(c), x_T=d(x_T), eta=eta,
                                               unconditional_guidance_scale=3.0, unconditional_conditioning=d(uc),
                                               verbose=False, **extra)
        s = cls(tiny["eps"])
        s.make_schedule(S, ddim_eta=eta, verbose=False)
        got, ginter = s.decode(d(x_T), d(c), S, unconditional_guidance_scale=3.0, unconditional_conditioning=d(uc), **extra)
        assert torch.equal(got, want)
        assert len(ginter["x_inter"]) == len(winter["x_inter"]) and torch.equal(ginter["pred_x0"][-1], winter["pred_x0"][-1])


def test_dpm_solver_t_start_T_is_the_full_run(tiny):
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    x_T, c, uc = V.tiny_inputs(tiny["cfg"]["context_dim"])
    d = lambda a: torch.tensor(a, device=DEV)
    run = lambda **kw: DPMSolverSampler(tiny["eps"]).sample(6, V.B, I.SHAPE, conditioning=d(c), x_T=d(x_T),
                                                            unconditional_guidance_scale=3.0,
                                                            unconditional_conditioning=d(uc), verbose=False, **kw)[0]
    assert torch.equal(run(t_start=1.0), run()) and torch.equal(run(t_start=None), run())


def test_eps_sampler_runs_still_reproduce_the_parent_golden():
    """tests/golden/vpred_eps_parent.npz (see test_vpred_gpu.py): the runs without t_start are the runs they always were."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "vpred_eps_parent.npz"))
    model, cfg, _ = V.tiny_eps_model()
    for name in V.EPS_IDENTITY_CASES:
        got = V.product_trajectory(name, model, cfg["context_dim"], DEV)
        assert torch.equal(got.cpu(), torch.tensor(gold[name])), name


# ------------------------------------------------------------------------------------------------ partial runs vs the oracle
@pytest.mark.parametrize("name", sorted(I.CASES))
def test_partial_run_vs_oracle(tiny, name):
    param = I.CASES[name][0]
    model, om, ctx = tiny[param], tiny["o_" + param], tiny["cfg"]["context_dim"]
    sampler, x_enc = I.product_encode(name, model, DEV)
    check(f"img2img_encode_{name}", x_enc, I.oracle_encode(name, om), rel_l2=1e-5)
    got = I.product_decode(name, sampler, x_enc, ctx, DEV)
    check(f"img2img_{name}", got, I.oracle_partial(name, om, ctx), rel_l2=1e-2, max_rel=1e-2)


def test_stochastic_encode_returns_a_fresh_tensor_and_draws_from_the_generator(tiny):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    x0 = torch.tensor(I.start_inputs()[0], device=DEV)
    keep = x0.clone()
    g = torch.Generator(device=DEV)
    s = DDIMSampler(tiny["eps"], generator=g)
    s.make_schedule(10, verbose=False)
    g.manual_seed(7)
    one = s.stochastic_encode(x0, 4)
    g.manual_seed(7)
    two = s.stochastic_encode(x0, 4)
    assert one.data_ptr() != x0.data_ptr() and torch.equal(x0, keep) and torch.equal(one, two)
    g.manual_seed(7)
    n = torch.randn(x0.shape, device=DEV, dtype=torch.float32, generator=g)
    assert torch.equal(one, s.stochastic_encode(x0, 4, noise=n))


@pytest.mark.parametrize("name", ["eps_plms_S8_t4_mask", "eps_ddim_S8_t4_mask"])
def test_masked_decode_makes_one_q_sample_launch_per_step(tiny, ops, monkeypatch, name):
    """The mask / x0 blend of decode() is ops.q_sample, once per step, and never the torch expression of model.q_sample."""
    model, ctx = tiny["eps"], tiny["cfg"]["context_dim"]
    sampler, x_enc = I.product_encode(name, model, DEV)
    count = {"ops": 0, "model": 0}
    real_ops, real_model = ops.q_sample, model.q_sample

    def ops_q(*a, **k):
        count["ops"] += 1
        assert k["out"] is k["img"] and k["mask"] is not None
        return real_ops(*a, **k)

    def model_q(*a, **k):
        count["model"] += 1
        return real_model(*a, **k)
    monkeypatch.setattr(ops, "q_sample", ops_q)
    monkeypatch.setattr(model, "q_sample", model_q, raising=False)
    I.product_decode(name, sampler, x_enc, ctx, DEV)
    assert count == {"ops": I.CASES[name][3], "model": 0}
    # sample(mask=) keeps the torch expression: moving it is not part of this change
    count.update(ops=0, model=0)
    V.product_trajectory("plms_S5_blend", model, ctx, DEV)
    assert count == {"ops": 0, "model": 5}


# ------------------------------------------------------------------------------------------------ pipeline end to end
@pytest.fixture(scope="module")
def tiny_pipeline_model(tiny):
    """The tiny UNet with the tiny VAE attached (it downsamples by 2: a 16 x 16 image is an 8 x 8 latent)."""
    from oracle import vae as OV
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
    dd = dict(TINY_VAE_DDCONFIG)
    vae = AutoencoderKL(ddconfig=dd, embed_dim=4, device=DEV)
    vae.load_state_dict(OV.init_params(dd, seed=8))
    model, _, _ = V.tiny_eps_model(scale_factor=0.18215)
    model.first_stage_model = vae
    return model


def _pipe_inputs(ctx_dim):
    rng = np.random.RandomState(31)
    image = np.clip(0.5 * rng.randn(2, 3, 16, 16), -1, 1).astype(np.float32)
    noise, post = rng.randn(2, 4, 8, 8).astype(np.float32), rng.randn(2, 4, 8, 8).astype(np.float32)
    _, c, uc = V.tiny_inputs(ctx_dim)
    return torch.tensor(image), torch.tensor(noise), torch.tensor(post), torch.tensor(c), torch.tensor(uc)


@pytest.mark.parametrize("kind", ["ddim", "plms", "dpm_solver"])
def test_pipeline_img2img_is_the_hand_composition(tiny, tiny_pipeline_model, kind):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model = tiny_pipeline_model
    image, noise, post, c, uc = _pipe_inputs(tiny["cfg"]["context_dim"])
    steps, strength, scale = 8, 0.5, 3.0
    t_enc = 4
    pipe = DiffusionPipeline(model, kind, device=DEV)
    got = pipe.img2img(init_image=image, strength=strength, c=c, uc=uc, steps=steps, scale=scale, noise=noise,
                       post_noise=post)
    assert tuple(got.shape) == (2, 4, 8, 8)
    # by hand: encode, scale, noise, run the remaining steps
    d = lambda t: t.to(DEV)
    z0 = model.get_first_stage_encoding(model.first_stage_model.encode(d(image), noise=d(post)))
    c16, uc16 = d(c).half(), d(uc).half()
    s = type(pipe.sampler)(model)

    def remaining(z):
        if kind == "dpm_solver":
            t_start = I.dpm_t_start(steps, t_enc)
            x_enc = s.stochastic_encode(z, t_start, noise=d(noise))
            return s.sample(t_enc, 2, (4, 8, 8), conditioning=c16, x_T=x_enc, unconditional_guidance_scale=scale,
                            unconditional_conditioning=uc16, verbose=False, t_start=t_start)[0]
        s.make_schedule(steps, ddim_eta=0., verbose=False)
        x_enc = s.stochastic_encode(z, t_enc, noise=d(noise))
        return s.decode(x_enc, c16, t_enc, unconditional_guidance_scale=scale, unconditional_conditioning=uc16)[0]
    assert torch.equal(got, remaining(z0))
    # init_latent= is the same composition run from the latent
    z = torch.tensor(I.start_inputs()[0])
    from_latent = pipe.img2img(init_latent=z, strength=strength, c=c, uc=uc, steps=steps, scale=scale, noise=noise)
    assert torch.equal(from_latent, remaining(d(z)))


def test_pipeline_img2img_seed_mask_and_decode(tiny, tiny_pipeline_model):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model = tiny_pipeline_model
    image, _, _, c, uc = _pipe_inputs(tiny["cfg"]["context_dim"])
    pipe = DiffusionPipeline(model, "ddim", device=DEV)
    kw = dict(init_image=image, strength=0.6, c=c, uc=uc, steps=5, scale=3.0)
    one, two, other = pipe.img2img(seed=3, **kw), pipe.img2img(seed=3, **kw), pipe.img2img(seed=4, **kw)
    assert torch.equal(one, two) and not torch.equal(one, other)
    # both draws come from the seed: numpy RandomState(seed) / RandomState(seed + 1) at the latent's shape
    draw = lambda sd: torch.from_numpy(np.random.RandomState(sd).randn(2, 4, 8, 8).astype(np.float32))
    assert torch.equal(one, pipe.img2img(noise=draw(3), post_noise=draw(4), **kw))
    mode = pipe.img2img(seed=3, sample_posterior=False, **kw)
    assert not torch.equal(mode, one)
    # decode=True: images in [0, 1] of the input's size
    out = pipe.img2img(seed=3, decode=True, **kw)
    assert tuple(out.shape) == (2, 3, 16, 16) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    assert bool(torch.isfinite(out).all())
    # mask (1 = keep the init image): the encoded z0 is the x0 of the blend -- against the hand composition
    mask = torch.zeros(2, 1, 8, 8)
    mask[:, :, :, :4] = 1.0
    g = torch.Generator(device=DEV)
    pipe.sampler.generator = g
    g.manual_seed(9)
    masked = pipe.img2img(seed=3, mask=mask.to(DEV), **kw)
    z0 = model.get_first_stage_encoding(model.first_stage_model.encode(image.to(DEV), noise=draw(4).to(DEV)))
    s = type(pipe.sampler)(model, generator=g)
    s.make_schedule(5, verbose=False)
    g.manual_seed(9)
    want = s.decode(s.stochastic_encode(z0, 3, noise=draw(3).to(DEV)), c.to(DEV).half(), 3, unconditional_guidance_scale=3.0,
                    unconditional_conditioning=uc.to(DEV).half(), mask=mask.to(DEV), x0=z0)[0]
    assert torch.equal(masked, want) and not torch.equal(masked, one)
