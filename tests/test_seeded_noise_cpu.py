"""Per-sample seeded noise, the part that needs no GPU: the numpy restatement (tests/_seeded_util.py) against the published
Random123 known answers and against the statistics of N(0, 1), and the seeds= plumbing of the samplers and the pipeline."""
import types

import numpy as np
import pytest
import torch

import _seeded_util as R

MDX_E_INVALID = -1     # include/mdx.h


# ------------------------------------------------------------------------------------------------ the generator
# Random123 kat_vectors, philox4x32-10: counter ; key -> output
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,expected", KNOWN_ANSWERS)
def test_restatement_reproduces_the_random123_known_answers(counter, key, expected):
    got = tuple(int(w) for w in R.philox4x32_10(counter, key))
    assert got == expected, [hex(w) for w in got]


def test_element_layout_of_the_restatement():
    """seed 0, stream 0, draw 0: elements 0..3 are the first known answer; a tail shorter than four is its prefix; the key is
    (low word, high word) of the seed's 64-bit pattern and -1 is 2^64 - 1."""
    assert [int(w) for w in R.philox_u32(0, 0, 0, 4)] == list(KNOWN_ANSWERS[0][2])
    assert [int(w) for w in R.philox_u32(0, 0, 0, 3)] == list(KNOWN_ANSWERS[0][2][:3])
    full = R.philox4x32_10((1, 7, 3, 0), (0xffffffff, 0xffffffff))
    assert [int(w) for w in R.philox_u32(-1, 3, 7, 8)[4:]] == [int(w) for w in full]
    assert np.array_equal(R.philox_u32(-1, 3, 7, 8), R.philox_u32((1 << 64) - 1, 3, 7, 8))
    full = R.philox4x32_10((0, 0, 0, 0), (5, 0x80000000))
    assert [int(w) for w in R.philox_u32((1 << 63) + 5, 0, 0, 4)] == [int(w) for w in full]


N = 1 << 20


@pytest.fixture(scope="module")
def draws():
    """2^20 reference normals of seed 11 on streams 0 and 1, and of seed 12 on stream 0 -- computed once."""
    return {"s11_0": R.normals64(11, 0, 0, N), "s11_1": R.normals64(11, 1, 0, N), "s12_0": R.normals64(12, 0, 0, N)}


def test_uniforms_are_strictly_inside_the_open_interval():
    u = R.uniform(R.philox_u32(11, 0, 0, N))
    assert u.dtype == np.float32 and float(u.min()) > 0.0 and float(u.max()) < 1.0
    edge = R.uniform(np.array([0, 0xffffffff], np.uint64))
    assert float(edge[0]) == 2.0 ** -24 and float(edge[1]) == 1.0 - 2.0 ** -24


def test_reference_normals_have_the_moments_of_n01(draws):
    """Five standard errors of each estimator at N = 2^20: mean 1/sqrt(N), variance sqrt(2/N), excess kurtosis sqrt(24/N)."""
    z = draws["s11_0"]
    assert np.isfinite(z).all()
    m, v = float(z.mean()), float(z.var())
    kurt = float(((z - m) ** 4).mean() / v ** 2 - 3.0)
    print(f"mean {m:.3e}  var - 1 {v - 1:.3e}  excess kurtosis {kurt:.3e}")
    assert abs(m) <= 5.0 / np.sqrt(N)
    assert abs(v - 1.0) <= 5.0 * np.sqrt(2.0 / N)
    assert abs(kurt) <= 5.0 * np.sqrt(24.0 / N)


def test_streams_and_neighbouring_seeds_are_uncorrelated(draws):
    for a, b in (("s11_0", "s11_1"), ("s11_0", "s12_0")):
        r = float(np.corrcoef(draws[a], draws[b])[0, 1])
        print(f"corr({a}, {b}) = {r:.3e}")
        assert abs(r) <= 5.0 / np.sqrt(N)


def test_dropout_rule_of_the_restatement():
    keep = R.keep_mask(11, R.RNG_STEP, 0, N, 0.25)
    assert abs(float(keep.mean()) - 0.75) <= 5.0 * np.sqrt(0.25 * 0.75 / N)
    z = R.randn([11], R.RNG_STEP, 0, 4096, dropout=0.25)[0]
    base = R.normals64(11, R.RNG_STEP, 0, 4096)
    assert np.array_equal(z == 0.0, ~keep[:4096])
    np.testing.assert_allclose(z[keep[:4096]], base[keep[:4096]] / 0.75, rtol=1e-7, atol=0)


# ------------------------------------------------------------------------------------------------ host-side refusals and helpers
def test_rng_entries_refuse_bad_arguments_without_a_launch():
    """Every refusal happens on the host, before any launch: nothing is dereferenced, so made-up addresses do."""
    from minddiffusion_amd import _lib
    lib = _lib.load()
    SEEDS, OUT = 4096, 1 << 20

    def randn(seeds=SEEDS, out=OUT, B=2, n=64, scale=1.0, p=0.0):
        return lib.mdx_randn_f32(seeds, 0, 0, scale, p, out, B, n, None)

    def u32(seeds=SEEDS, out=OUT, B=2, n=64):
        return lib.mdx_philox_u32(seeds, 0, 0, out, B, n, None)
    for rc in (randn(seeds=None), randn(out=None), randn(B=0), randn(n=0), randn(n=-4), randn(n=(1 << 34) + 1), randn(p=1.0),
               randn(p=-0.1), randn(p=float("nan")), randn(scale=float("inf")), randn(scale=float("nan")),
               u32(seeds=None), u32(out=None), u32(B=0), u32(n=0), u32(n=(1 << 34) + 4)):
        assert rc == MDX_E_INVALID


def test_seeds_tensor_accepts_the_whole_64_bit_range():
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    t = ops.seeds_tensor([0, 1, 1 << 32, (1 << 63) + 5, -1, (1 << 64) - 1, -(1 << 63)], "cpu")
    assert t.dtype == torch.int64
    assert t.tolist() == [0, 1, 1 << 32, -(1 << 63) + 5, -1, -1, -(1 << 63)]
    assert ops.seeds_tensor(np.array([3, 4]), "cpu").tolist() == [3, 4]
    assert ops.seeds_tensor(torch.tensor([3, 4], dtype=torch.int32), "cpu").dtype == torch.int64
    for bad in ([1 << 64], [-(1 << 63) - 1], [1.5], [True], torch.zeros(2), torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(MdxError, match="seeds"):
            ops.seeds_tensor(bad, "cpu")
    assert (ops.RNG_X_T, ops.RNG_STEP, ops.RNG_BLEND, ops.RNG_ENCODE, ops.RNG_POSTERIOR) == (0, 1, 2, 3, 4)


# ------------------------------------------------------------------------------------------------ sampler and pipeline plumbing
def _ldm():
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    return LatentDiffusion(object(), linear_start=0.00085, linear_end=0.0120, timesteps=1000)


def test_two_sources_for_one_draw_are_refused():
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    c = torch.zeros(2, 7, 64)
    g = torch.Generator().manual_seed(0)
    nz = [torch.zeros(2, 4, 8, 8)] * 3
    for cls in (PLMSSampler, DDIMSampler, DPMSolverSampler):
        with pytest.raises(ValueError, match="generator"):
            cls(_ldm(), generator=g).sample(4, 2, (4, 8, 8), conditioning=c, seeds=[1, 2], verbose=False)
    for cls in (PLMSSampler, DDIMSampler):
        for kw in ("step_noises", "blend_noises", "dropout_masks"):
            with pytest.raises(ValueError, match=kw):
                cls(_ldm()).sample(4, 2, (4, 8, 8), conditioning=c, seeds=[1, 2], verbose=False, **{kw: nz})
        s = cls(_ldm())
        s.make_schedule(4, verbose=False)
        with pytest.raises(ValueError, match="step_noises"):
            s.decode(torch.zeros(2, 4, 8, 8), c, 2, seeds=[1, 2], step_noises=nz)


class _StubSampler:
    """Records what DiffusionPipeline hands its sampler."""

    def __init__(self):
        self.calls = []

    def sample(self, **kw):
        self.calls.append(kw)
        b = kw["batch_size"]
        return torch.zeros(b, 4, 8, 8), None


def _stub_pipe():
    from minddiffusion_amd.pipeline import DiffusionPipeline
    unet = types.SimpleNamespace(context_dim=64, max_context_len=80, device=torch.device("cpu"))
    model = types.SimpleNamespace(unet=unet)
    return DiffusionPipeline(model, _StubSampler(), device="cpu")


def test_pipeline_refuses_a_wrong_number_of_seeds():
    from minddiffusion_amd._lib import MdxError
    p = _stub_pipe()
    c = torch.zeros(4, 7, 64)
    with pytest.raises(MdxError, match="3 seeds for a global batch of 4"):
        p(c=c, uc=torch.zeros(4, 7, 64), H=64, W=64, steps=2, seeds=[1, 2, 3])
    with pytest.raises(MdxError, match="5 seeds for a global batch of 4"):
        p.img2img(init_latent=torch.zeros(4, 4, 8, 8), c=c, steps=4, seeds=torch.arange(5))
    assert p.sampler.calls == []


def test_pipeline_without_seeds_passes_no_seeds_keyword():
    p = _stub_pipe()
    p(c=torch.zeros(2, 7, 64), uc=torch.zeros(2, 7, 64), H=64, W=64, steps=2)
    assert "seeds" not in p.sampler.calls[0]
    assert torch.equal(p.sampler.calls[0]["x_T"], p.start_noise(2, [4, 8, 8], 42))


@pytest.mark.parametrize("rank", [0, 1])
def test_each_rank_hands_its_sampler_its_own_slice_of_the_seeds(monkeypatch, rank):
    """World (rank, 2), global batch 4: the sampler gets seeds[lo:hi] of D.shard_bounds; rank 1 draws nothing itself (the
    global x_T is rank 0's and arrives with the one broadcast, here a stand-in)."""
    from minddiffusion_amd import distributed as D
    from minddiffusion_amd import pipeline as P
    B, seeds = 4, [11, (1 << 63) + 5, -1, 7]
    sent = {}

    def fake_broadcast(c, uc, x_T, global_batch, ctx_shape, latent_shape, device, **kw):
        sent.update(x_T=x_T, global_batch=global_batch)
        lo, hi = D.shard_bounds(global_batch, rank, 2)
        return torch.zeros(hi - lo, 7, 64), torch.zeros(hi - lo, 7, 64), torch.zeros(hi - lo, *latent_shape)

    made = []
    monkeypatch.setattr(D, "world", lambda: (rank, 2))
    monkeypatch.setattr(D, "broadcast_conditioning", fake_broadcast)
    monkeypatch.setattr(P.DiffusionPipeline, "seeded_noise",
                        lambda self, s, stream, shape: made.append((list(s), stream, tuple(shape))) or torch.zeros(len(s), *shape))
    p = _stub_pipe()
    p(c=torch.zeros(B, 7, 64) if rank == 0 else None, uc=torch.zeros(B, 7, 64) if rank == 0 else None, H=64, W=64, steps=2,
      batch_size=B, seeds=seeds)
    call = p.sampler.calls[0]
    assert call["seeds"] == seeds[B // 2 * rank:B // 2 * (rank + 1)] and call["batch_size"] == B // 2
    if rank == 0:
        assert made == [(seeds, 0, (4, 8, 8))] and tuple(sent["x_T"].shape) == (B, 4, 8, 8)
    else:
        assert made == [] and sent["x_T"] is None
        assert call["seeds"] == seeds[B // 2:]
