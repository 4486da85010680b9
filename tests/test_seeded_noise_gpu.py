"""Per-sample seeded noise on the GPU: mdx_philox_u32 / mdx_randn_f32 (csrc/rng.hip) against the numpy restatement of
tests/_seeded_util.py -- never against themselves -- and the seeds= keyword of the samplers and the pipeline.

The kernel shapes sit where the indexing can break: fewer elements than one Philox call, odd tails, more than one sample per
wave, exactly one wave of float4 lanes and one element more, and one tensor large enough that the grid-stride loop takes a
second trip (4096 workgroups x 64 lanes x 4 elements = 2^20 < 3 * (2^19 + 4))."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _guard as G
import _seeded_default_runs as DR
import _seeded_util as R
import _vpred_util as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

SEEDS = [0, 1, 1 << 32, (1 << 63) + 5, -1]
SHAPES = [(1, 1), (1, 3), (1, 4), (3, 5), (2, 7), (3, 64 * 4), (2, 64 * 4 + 1)]
BIG = (3, (1 << 19) + 4)
# absolute bound on a normal against the float64 restatement, derived from the arithmetic and not from a run: |z| <= r < 6.8,
# a few ulp each from logf, sqrtf, sincospif and the products is ~3e-6 at that magnitude; 1e-5 leaves a factor of three
NORMAL_ATOL = 1e-5
# two runs of one sample in different batches take different launch plans; each is within 1e-2 of the oracle (test_unet_gpu.py)
BATCH_REL_L2 = 2e-2

_memo = {}


def ref_words(seed, stream, draw, n):
    key = ("w", seed, stream, draw, n)
    if key not in _memo:
        _memo[key] = R.philox_u32(seed, stream, draw, n)
    return _memo[key]


def ref_randn(seed, stream, draw, n, scale=1.0, dropout=0.0):
    key = ("z", seed, stream, draw, n, scale, dropout)
    if key not in _memo:
        _memo[key] = R.randn([seed], stream, draw, n, scale, dropout)[0]
    return _memo[key]


def seed_rows(B, k):
    """B of the five seeds, starting at the k-th: over k = 0..4 every seed meets every row of every shape."""
    return [SEEDS[(k + i) % len(SEEDS)] for i in range(B)]


def dev_seeds(seeds):
    from minddiffusion_amd import ops
    return ops.seeds_tensor(seeds, DEV)


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ kernel: bits
@pytest.mark.parametrize("B,n", SHAPES + [BIG])
def test_philox_words_equal_the_restatement(B, n):
    from minddiffusion_amd import ops
    for k in range(len(SEEDS) if (B, n) != BIG else 1):
        seeds = seed_rows(B, k + 2 if (B, n) == BIG else k)
        for stream, draw in ((0, 0), (3, 70000)):
            got = as_u32(ops.philox_u32(dev_seeds(seeds), stream, draw, (n,)))
            want = np.stack([ref_words(s, stream, draw, n) for s in seeds])
            assert np.array_equal(got, want), (seeds, stream, draw)


def test_known_answer_rows():
    """seed 0, stream 0, draw 0: elements 0..3 are Random123's first philox4x32-10 vector."""
    from minddiffusion_amd import ops
    got = as_u32(ops.philox_u32(dev_seeds([0]), 0, 0, (4,)))[0]
    assert [int(w) for w in got] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


# ------------------------------------------------------------------------------------------------ kernel: normals
def test_normals_are_within_the_derived_bound_of_the_float64_restatement():
    from minddiffusion_amd import ops
    worst = 0.0
    for B, n in SHAPES + [BIG]:
        for k in range(len(SEEDS) if (B, n) != BIG else 1):
            seeds = seed_rows(B, k + 2 if (B, n) == BIG else k)
            got = ops.randn_seeded(dev_seeds(seeds), R.RNG_STEP, 2, (n,)).cpu().numpy().astype(np.float64)
            want = np.stack([ref_randn(s, R.RNG_STEP, 2, n) for s in seeds])
            assert np.isfinite(got).all()
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"largest |kernel - float64 restatement| over all cases: {worst:.3e}")
    assert worst <= NORMAL_ATOL


def test_scale_is_one_float32_multiply():
    from minddiffusion_amd import ops
    for B, n in ((3, 256), (2, 257)):
        st = dev_seeds(seed_rows(B, 1))
        one = ops.randn_seeded(st, 0, 0, (n,)).cpu().numpy()
        scaled = ops.randn_seeded(st, 0, 0, (n,), scale=0.37).cpu().numpy()
        assert np.array_equal(scaled, np.float32(0.37) * one)


# ------------------------------------------------------------------------------------------------ kernel: the two forms agree
@pytest.mark.parametrize("dropout", [0.0, 0.25])
def test_vector_and_scalar_forms_write_the_same_bits(dropout):
    from minddiffusion_amd import ops
    for B, n in ((3, 256), (2, 1024), (3, 8)):
        st = dev_seeds(seed_rows(B, 3))
        aligned = ops.randn_seeded(st, 1, 5, (n,), dropout=dropout)
        assert aligned.data_ptr() % 16 == 0
        flat = torch.zeros(B * n + 8, device=DEV)
        shifted = flat[1:1 + B * n].view(B, n)                      # starts one float later: the scalar form
        assert shifted.data_ptr() % 16 == 4
        ops.randn_seeded(st, 1, 5, (n,), dropout=dropout, out=shifted)
        assert torch.equal(aligned, shifted)
        wa = ops.philox_u32(st, 1, 5, (n,))
        ws = torch.zeros(B * n + 8, device=DEV, dtype=torch.int32)[1:1 + B * n].view(B, n)
        ops.philox_u32(st, 1, 5, (n,), out=ws)
        assert torch.equal(wa, ws)


@pytest.mark.parametrize("n", [1, 3, 5, 7, 257, 1023])
def test_an_odd_length_is_a_prefix_of_the_next_multiple_of_four(n):
    from minddiffusion_amd import ops
    st = dev_seeds(seed_rows(3, 2))
    n4 = (n + 3) // 4 * 4
    for dropout in (0.0, 0.25):
        assert torch.equal(ops.randn_seeded(st, 2, 1, (n,), dropout=dropout),
                           ops.randn_seeded(st, 2, 1, (n4,), dropout=dropout)[:, :n])
    assert torch.equal(ops.philox_u32(st, 2, 1, (n,)), ops.philox_u32(st, 2, 1, (n4,))[:, :n])


# ------------------------------------------------------------------------------------------------ kernel: batch invariance
@pytest.mark.parametrize("shape", [(256,), (257,), (4, 8, 8), (3, 5, 7)])
def test_a_row_depends_on_its_own_seed_only(shape):
    from minddiffusion_amd import ops
    a, b, c = 5, (1 << 63) + 5, -1
    for kw in ({}, {"scale": 0.8, "dropout": 0.25}):
        abc = ops.randn_seeded(dev_seeds([a, b, c]), 1, 3, shape, **kw)
        alone = ops.randn_seeded(dev_seeds([b]), 1, 3, shape, **kw)
        ba = ops.randn_seeded(dev_seeds([b, a]), 1, 3, shape, **kw)
        assert tuple(abc.shape) == (3,) + shape
        assert torch.equal(abc[1], alone[0]) and torch.equal(abc[1], ba[0]) and torch.equal(abc[0], ba[1])
        assert not torch.equal(abc[0], abc[1])


# ------------------------------------------------------------------------------------------------ kernel: dropout
def test_dropout_zeroes_what_the_restatement_zeroes():
    from minddiffusion_amd import ops
    worst = 0.0
    for B, n in SHAPES + [(2, 4096)]:
        seeds = seed_rows(B, 0)
        st = dev_seeds(seeds)
        got = ops.randn_seeded(st, R.RNG_STEP, 1, (n,), dropout=0.25).cpu().numpy().astype(np.float64)
        want = np.stack([ref_randn(s, R.RNG_STEP, 1, n, 1.0, 0.25) for s in seeds])
        assert np.array_equal(got == 0.0, want == 0.0)
        worst = max(worst, float(np.abs(got - want).max()))
        assert torch.equal(ops.randn_seeded(st, R.RNG_STEP, 1, (n,), dropout=0.0), ops.randn_seeded(st, R.RNG_STEP, 1, (n,)))
    zeros = float((got == 0.0).mean())
    print(f"dropout 0.25: largest |kernel - restatement| {worst:.3e}, zero fraction of the 2 x 4096 case {zeros:.4f}")
    assert worst <= NORMAL_ATOL
    assert abs(zeros - 0.25) <= 5.0 * np.sqrt(0.25 * 0.75 / 8192)


# ------------------------------------------------------------------------------------------------ kernel: footprint, refusals
@pytest.mark.parametrize("B,n", [(3, 256), (3, 5), (2, 257)])
def test_nothing_outside_the_output_is_written(B, n):
    from minddiffusion_amd import ops
    st = dev_seeds(seed_rows(B, 0))
    for dropout in (0.0, 0.25):
        buf, view = G.guarded((B, n), dtype=torch.float32, device=DEV)
        ops.randn_seeded(st, 0, 0, (n,), dropout=dropout, out=view)
        G.assert_footprint(buf, view, f"mdx_randn_f32 {B}x{n} p={dropout}", written=True)
    buf = torch.full((4096 + B * n + 4096,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    view = buf[4096:4096 + B * n].view(B, n)
    ops.philox_u32(st, 0, 0, (n,), out=view)
    torch.cuda.synchronize()
    assert bool((buf[:4096] == 0x5A5A5A5A).all()) and bool((buf[4096 + B * n:] == 0x5A5A5A5A).all())
    assert np.array_equal(as_u32(view), np.stack([ref_words(s, 0, 0, n) for s in seed_rows(B, 0)]))


def test_bad_arguments_are_refused_without_a_launch():
    from minddiffusion_amd import _lib
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd import ops
    lib = _lib.load()
    st = dev_seeds([1, 2])
    out = torch.full((2, 64), G.SENT, device=DEV)
    sp, op = ctypes.c_void_p(st.data_ptr()), ctypes.c_void_p(out.data_ptr())
    for rc in (lib.mdx_randn_f32(sp, 0, 0, 1.0, 0.0, op, 2, 0, None),
               lib.mdx_randn_f32(sp, 0, 0, 1.0, 1.0, op, 2, 64, None),
               lib.mdx_randn_f32(None, 0, 0, 1.0, 0.0, op, 2, 64, None),
               lib.mdx_randn_f32(sp, 0, 0, 1.0, 0.0, op, 2, (1 << 34) + 4, None),
               lib.mdx_randn_f32(sp, 0, 0, float("inf"), 0.0, op, 2, 64, None),
               lib.mdx_philox_u32(sp, 0, 0, op, 2, 0, None),
               lib.mdx_philox_u32(None, 0, 0, op, 2, 64, None),
               lib.mdx_philox_u32(sp, 0, 0, op, 2, (1 << 34) + 4, None)):
        assert rc == -1                                               # MDX_E_INVALID
    torch.cuda.synchronize()
    assert bool((out == G.SENT).all())
    with pytest.raises(MdxError, match="dropout_p"):
        ops.randn_seeded(st, 0, 0, (64,), dropout=1.0)
    with pytest.raises(MdxError, match="stream"):
        ops.randn_seeded(st, 1 << 31, 0, (64,))
    with pytest.raises(MdxError, match="out has shape"):
        ops.randn_seeded(st, 0, 0, (64,), out=torch.empty(2, 63, device=DEV))


# ------------------------------------------------------------------------------------------------ samplers
S = 4
LATENT = (4, 8, 8)


@pytest.fixture(scope="module")
def tiny():
    model, cfg, _ = V.tiny_eps_model()
    rng = np.random.RandomState(401)
    ctx = cfg["context_dim"]
    c = torch.tensor(rng.randn(3, V.T, ctx).astype(np.float32), device=DEV)
    uc = torch.tensor(np.repeat(rng.randn(1, V.T, ctx).astype(np.float32), 3, 0), device=DEV)
    return {"model": model, "cfg": cfg, "c": c, "uc": uc}


def _samplers():
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    return {"plms": (PLMSSampler, {}), "ddim_eta1": (DDIMSampler, {"eta": 1.0}), "dpm": (DPMSolverSampler, {}),
            "ddim_eta1_temp_drop": (DDIMSampler, {"eta": 1.0, "temperature": 0.8, "noise_dropout": 0.25})}


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("extra", ["plain", "temperature", "blend", "blend_decode"])
def test_seeded_run_equals_the_run_with_the_same_draws_injected(tiny, extra):
    """Pins the (stream, draw) bookkeeping: x_T is (RNG_X_T, 0), the k-th step noise (RNG_STEP, k), the blend at loop index i
    (RNG_BLEND, i).  The injected path's parity with the oracle is tested elsewhere, so the seeded path inherits it."""
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    seeds = [5, (1 << 63) + 5]
    st = dev_seeds(seeds)
    c, uc = tiny["c"][:2], tiny["uc"][:2]
    x_T = ops.randn_seeded(st, ops.RNG_X_T, 0, LATENT)
    steps = [ops.randn_seeded(st, ops.RNG_STEP, k, LATENT) for k in range(S)]
    kw = dict(conditioning=c, unconditional_guidance_scale=3.0, unconditional_conditioning=uc, verbose=False, eta=1.0)
    inj = {}
    if extra == "temperature":
        kw["temperature"] = 0.8
    if extra in ("blend", "blend_decode"):
        rng = np.random.RandomState(78)
        kw["mask"] = torch.tensor((rng.rand(2, 1, 8, 8) > 0.5).astype(np.float32), device=DEV)
        kw["x0"] = torch.tensor(rng.randn(2, *LATENT).astype(np.float32), device=DEV)
        inj["blend_noises"] = [ops.randn_seeded(st, ops.RNG_BLEND, i, LATENT) for i in range(S)]
    if extra == "blend_decode":
        t_enc = 3
        del kw["verbose"], kw["eta"]
        cond = kw.pop("conditioning")
        a, b = DDIMSampler(tiny["model"]), DDIMSampler(tiny["model"])
        for s in (a, b):
            s.make_schedule(S, ddim_eta=1.0, verbose=False)
        xa = a.stochastic_encode(kw["x0"], t_enc, seeds=seeds)
        xb = b.stochastic_encode(kw["x0"], t_enc, noise=ops.randn_seeded(st, ops.RNG_ENCODE, 0, LATENT))
        assert torch.equal(xa, xb)
        seeded = a.decode(xa, cond, t_enc, seeds=seeds, **kw)[0]
        injected = b.decode(xb, cond, t_enc, step_noises=steps, **inj, **kw)[0]
    else:
        seeded, inter = DDIMSampler(tiny["model"]).sample(S, 2, LATENT, seeds=seeds, **kw)
        assert torch.equal(inter["x_inter"][0], x_T)
        injected = DDIMSampler(tiny["model"]).sample(S, 2, LATENT, x_T=x_T, step_noises=steps, **inj, **kw)[0]
    assert bool(torch.isfinite(seeded).all())
    assert torch.equal(seeded, injected)


@pytest.mark.parametrize("kind", ["plms", "ddim_eta1", "dpm", "ddim_eta1_temp_drop"])
def test_a_sample_does_not_depend_on_the_batch_it_is_served_in(tiny, kind, monkeypatch):
    """seeds [5, 7, 9] at batch 3 against seed [7] at batch 1: every draw of that sample is bit-identical (x_T first), and the
    final latents differ only by the different launch plans of the two UNet batches."""
    from minddiffusion_amd import ops
    cls, kw = _samplers()[kind]
    drawn = []
    real = ops.randn_seeded

    def spy(*a, **k):
        out = real(*a, **k)
        drawn.append(out.clone())
        return out
    monkeypatch.setattr(ops, "randn_seeded", spy)
    common = dict(unconditional_guidance_scale=3.0, verbose=False, **kw)
    three = cls(tiny["model"]).sample(S, 3, LATENT, conditioning=tiny["c"], unconditional_conditioning=tiny["uc"],
                                      seeds=[5, 7, 9], **common)[0]
    d3, drawn[:] = list(drawn), []
    one = cls(tiny["model"]).sample(S, 1, LATENT, conditioning=tiny["c"][1:2], unconditional_conditioning=tiny["uc"][1:2],
                                    seeds=[7], **common)[0]
    d1 = list(drawn)
    assert len(d3) == len(d1) == (1 + S if kind.startswith("ddim_eta1") else 1)
    for a, b in zip(d3, d1):
        assert torch.equal(a[1], b[0])
    assert torch.equal(d1[0], real(dev_seeds([7]), ops.RNG_X_T, 0, LATENT))
    err = rel_l2(three[1], one[0])
    print(f"{kind}: sample of seed 7 at batch 3 vs batch 1, rel-L2 {err:.3e}")
    assert err <= BATCH_REL_L2


def test_default_runs_are_bit_identical_to_the_parent_commit(tiny):
    """tests/golden/seeded_parent.npz: seeds=None runs (x_T, step noise and dropout mask from a seeded torch generator),
    recorded before the samplers took seeds=.  This one passes before and after."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "seeded_parent.npz"))
    got = DR.default_runs(tiny["model"], tiny["cfg"]["context_dim"], DEV)
    assert sorted(gold.files) == sorted(got)
    for name, t in got.items():
        assert np.array_equal(t.cpu().numpy(), gold[name]), name


# ------------------------------------------------------------------------------------------------ pipeline
def test_pipeline_sample_does_not_depend_on_its_batch(tiny, monkeypatch):
    from minddiffusion_amd import ops
    from minddiffusion_amd.pipeline import DiffusionPipeline
    drawn = []
    real = ops.randn_seeded
    monkeypatch.setattr(ops, "randn_seeded", lambda *a, **k: drawn.append(real(*a, **k)) or drawn[-1])
    pipe = DiffusionPipeline(tiny["model"], "ddim", device=DEV)
    kw = dict(H=64, W=64, steps=S, scale=3.0, eta=1.0)
    two = pipe(c=tiny["c"][:2].cpu(), uc=tiny["uc"][:2].cpu(), seeds=[3, 4], **kw)
    d2, drawn[:] = [t.clone() for t in drawn], []
    one = pipe(c=tiny["c"][1:2].cpu(), uc=tiny["uc"][1:2].cpu(), seeds=[4], **kw)
    assert len(d2) == len(drawn) == 1 + S
    for a, b in zip(d2, drawn):
        assert torch.equal(a[1], b[0])
    err = rel_l2(two[1], one[0])
    print(f"pipeline: seed 4 at batch 2 vs batch 1, rel-L2 {err:.3e}")
    assert err <= BATCH_REL_L2
    # seed= keeps its meaning when seeds is None
    assert torch.equal(pipe(c=tiny["c"][:2].cpu(), uc=tiny["uc"][:2].cpu(), seed=6, H=64, W=64, steps=S, scale=3.0),
                       pipe(c=tiny["c"][:2].cpu(), uc=tiny["uc"][:2].cpu(), x_T=pipe.start_noise(2, [4, 8, 8], 6), H=64, W=64,
                            steps=S, scale=3.0))


@pytest.mark.parametrize("kind", ["ddim", "dpm_solver"])
def test_pipeline_img2img_with_seeds(tiny, kind, monkeypatch):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    pipe = DiffusionPipeline(tiny["model"], kind, device=DEV)
    z = torch.tensor(np.random.RandomState(17).randn(2, *LATENT).astype(np.float32))
    kw = dict(init_latent=z, strength=0.5, c=tiny["c"][:2].cpu(), uc=tiny["uc"][:2].cpu(), steps=2 * S, scale=3.0)
    encoded = []
    name = "sample" if kind == "dpm_solver" else "decode"
    real = getattr(pipe.sampler, name)

    def spy(*a, **k):
        encoded.append((k["x_T"] if kind == "dpm_solver" else a[0]).clone())
        return real(*a, **k)
    monkeypatch.setattr(pipe.sampler, name, spy)
    one, two, other = pipe.img2img(seeds=[3, 4], **kw), pipe.img2img(seeds=[3, 4], **kw), pipe.img2img(seeds=[8, 4], **kw)
    assert torch.equal(one, two) and bool(torch.isfinite(one).all())
    assert torch.equal(encoded[0], encoded[1])
    assert torch.equal(encoded[2][1], encoded[0][1]) and not torch.equal(encoded[2][0], encoded[0][0])
    assert not torch.equal(other[0], one[0])
