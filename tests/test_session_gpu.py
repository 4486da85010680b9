"""Sampling sessions end to end on the GPU: five requests with their own seeds, steps, guidance scales and rescales go through a
3-slot session -- four submitted at once, the fifth after two ticks have run -- so one lands in a slot vacated mid-run and one
starts on an odd tick (the DPM-Solver buffer parity).

The reference for the request that ran in slot b is the existing per-request path: sampler.sample(S=[S_r] * 3, ...) with the
request's conditioning, seed and parameters in row b (two other requests fill the other rows) -- the same batch size, so the same
launch plans, and the same guidance batch.  Every request's latent must be torch.equal to row b of that run, which also shows
that a request joining or leaving changes no bit of its neighbours.  No tolerance anywhere.
"""
import numpy as np
import pytest
import torch

import _vpred_util as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LATENT = (4, 8, 8)
SLOTS = 3
# DDIM takes steps from {1, 2, 4} (make_ddim_timesteps has no 3-step grid), DPM-Solver from {1, 3, 4}
STEPS = {"ddim": [4, 1, 2, 4, 2], "ddim_eta1": [4, 1, 2, 4, 2], "dpm": [4, 1, 3, 4, 3]}
SCALES = [1.5, 3.0, 7.5, 5.0, 2.0]
PHIS = [0.0, 0.7, 0.3, 0.0, 1.0]
SEEDS = [5, 7, 9, -11, (1 << 63) + 13]
RELEASE = [0, 0, 0, 0, 2]                     # the tick before which each request is submitted
KINDS = sorted(STEPS)


def packing(steps):
    """FIFO into the lowest free slot: (slot, start) of every request and the tick count."""
    free, placed = [0] * SLOTS, []
    for n, rel in zip(steps, RELEASE):
        start = max(min(free), rel)
        b = min(i for i in range(SLOTS) if free[i] <= start)
        placed.append((b, start))
        free[b] = start + n
    return placed, max(free)


@pytest.fixture(scope="module")
def tiny():
    v_model, cfg, _ = V.tiny_eps_model(parameterization="v")
    eps_model, _, _ = V.tiny_eps_model()
    rng = np.random.RandomState(411)
    d = lambda a: torch.tensor(a.astype(np.float32), device=DEV)
    return {"v": v_model, "eps": eps_model, "c": d(rng.randn(5, V.T, cfg["context_dim"])),
            "uc": d(rng.randn(5, V.T, cfg["context_dim"]))}


def pipeline(tiny, param, kind):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    return DiffusionPipeline(tiny[param], "dpm_solver" if kind == "dpm" else "ddim", device=DEV)


def requests(tiny, kind):
    eta = 1.0 if kind == "ddim_eta1" else 0.0
    return [dict(c=tiny["c"][r], uc=tiny["uc"][r], steps=STEPS[kind][r], scale=SCALES[r], guidance_rescale=PHIS[r], eta=eta,
                 seed=SEEDS[r]) for r in range(5)]


def run_session(tiny, param, kind):
    """(handles, session) of the five requests, the fifth submitted after two ticks."""
    sess = pipeline(tiny, param, kind).session(slots=SLOTS, H=64, W=64, context_len=V.T, max_steps=4)
    reqs = requests(tiny, kind)
    handles = [sess.submit(**r) for r in reqs[:4]]
    finished = sess.step() + sess.step()
    handles.append(sess.submit(**reqs[4]))
    finished += sess.run_until_idle()
    assert sorted(h.index for h, _ in finished) == list(range(5)) and all(lat is h.latent for h, lat in finished)
    return handles, sess


_REFERENCE = {}


def reference(tiny, param, kind, r, b):
    """Row b of the batch-3 per-request run whose row b is request r; computed once per (model, sampler, request, slot)."""
    key = (param, kind, r, b)
    if key not in _REFERENCE:
        from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
        from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
        who = [(r + 1) % 5, (r + 2) % 5]
        who.insert(b, r)                                            # request r in row b, two others around it
        sampler = (DPMSolverSampler if kind == "dpm" else DDIMSampler)(tiny[param])
        s_r = STEPS[kind][r]
        out = sampler.sample([s_r] * 3, 3, LATENT, conditioning=tiny["c"][who], unconditional_conditioning=tiny["uc"][who],
                             seeds=[SEEDS[i] for i in who], unconditional_guidance_scale=[SCALES[i] for i in who],
                             guidance_rescale=[PHIS[i] for i in who], eta=1.0 if kind == "ddim_eta1" else 0.0,
                             verbose=False)[0]
        _REFERENCE[key] = out[b].clone()
    return _REFERENCE[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("param", ["eps", "v"])
def test_every_request_equals_its_row_of_the_per_request_path(tiny, param, kind):
    handles, sess = run_session(tiny, param, kind)
    placed, ticks = packing(STEPS[kind])
    assert [(h.slot, h.start) for h in handles] == placed
    assert sess.tick_count == ticks == sess.unet_evals and sess.admissions == 5
    assert placed[3] == (1, 1)                                     # a slot vacated mid-run, entered on an odd tick
    assert any(start % 2 for _, start in placed) and any(start > 0 and b == placed[1][0] for b, start in placed)
    for r, h in enumerate(handles):
        assert h.done and tuple(h.latent.shape) == LATENT and bool(torch.isfinite(h.latent).all())
        want = reference(tiny, param, kind, r, h.slot)
        print(f"{param} {kind} request {r} (slot {h.slot}, tick {h.start}): max|d| {float((h.latent - want).abs().max()):.3e}")
        assert torch.equal(h.latent, want), (param, kind, r)
    assert not torch.equal(handles[0].latent, handles[3].latent)      # same steps, other seed / prompt / scale


def served(steps):
    """(slot of every request, tick count) when all are submitted at once."""
    free, slots = [0] * SLOTS, []
    for n in steps:
        slots.append(free.index(min(free)))
        free[slots[-1]] += n
    return slots, max(free)


@pytest.mark.parametrize("kind", ["ddim_eta1", "dpm"])
def test_serve_returns_results_in_request_order(tiny, kind):
    """All five at once through pipe.serve: the latents of the session run, in request order (requests 1 and 4 finish before
    request 0 and 3)."""
    handles, _ = run_session(tiny, "v", kind)
    pipe = pipeline(tiny, "v", kind)
    lat = pipe.serve(requests(tiny, kind), slots=SLOTS, H=64, W=64, output="latent")
    assert tuple(lat.shape) == (5,) + LATENT
    slots, ticks = served(STEPS[kind])
    assert pipe.last_session.tick_count == ticks
    for r, h in enumerate(handles):
        want = h.latent if slots[r] == h.slot else reference(tiny, "v", kind, r, slots[r])     # its slot is its UNet row
        assert torch.equal(lat[r], want), (kind, r)


def test_serve_images_have_the_shape_and_range_of_call(tiny):
    """The tiny VAE downsamples by 2: an 8 x 8 latent is a 16 x 16 image."""
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
    from minddiffusion_amd.pipeline import DiffusionPipeline
    from oracle import vae as OV
    dd = dict(TINY_VAE_DDCONFIG)
    vae = AutoencoderKL(ddconfig=dd, embed_dim=4, device=DEV)
    vae.load_state_dict(OV.init_params(dd, seed=8))
    model, _, _ = V.tiny_eps_model(scale_factor=0.18215)
    model.first_stage_model = vae
    pipe = DiffusionPipeline(model, "ddim", device=DEV)
    reqs = requests(tiny, "ddim")[:4]
    lat = pipe.serve(reqs, slots=2, H=64, W=64, output="latent")
    img = pipe.serve(reqs, slots=2, H=64, W=64, output="float")
    u8 = pipe.serve(reqs, slots=2, H=64, W=64, output="uint8")
    call = pipe(c=tiny["c"][:2].cpu(), uc=tiny["uc"][:2].cpu(), H=64, W=64, steps=2, scale=3.0, decode=True)
    assert tuple(img.shape) == (4,) + tuple(call.shape[1:]) == (4, 3, 16, 16) and img.dtype == call.dtype == torch.float32
    assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0 and float(img.max()) > float(img.min())
    assert torch.equal(img[:2], pipe._decoded(lat[:2])) and torch.equal(img[2:], pipe._decoded(lat[2:]))
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (4, 16, 16, 3)
    assert torch.equal(u8, (img * 255.0).to(torch.uint8).permute(0, 2, 3, 1))
    with pytest.raises(ValueError, match="output"):
        pipe.serve(reqs, output="png")


def test_refusals(tiny):
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.pipeline import DiffusionPipeline
    pipe = pipeline(tiny, "eps", "ddim")
    with pytest.raises(MdxError, match="PLMS evaluates the model twice"):
        pipe.session(slots=2, H=64, W=64, sampler="plms", context_len=V.T)
    with pytest.raises(MdxError, match="PLMS evaluates the model twice"):
        DiffusionPipeline(tiny["eps"], "plms", device=DEV).session(slots=2, H=64, W=64, context_len=V.T)
    sess = pipe.session(slots=2, H=64, W=64, context_len=V.T, max_steps=4)
    ok = dict(c=tiny["c"][0], uc=tiny["uc"][0], steps=2, scale=3.0, seed=1)
    with pytest.raises(ValueError, match="max_steps=4"):
        sess.submit(**dict(ok, steps=5))
    with pytest.raises(IndexError, match="choose S dividing"):           # no 3-step DDIM grid on 1000 training steps
        sess.submit(**dict(ok, steps=3))
    for k, v in (("mask", torch.ones(1, 1, 8, 8)), ("x0", torch.zeros(1, 4, 8, 8)), ("score_corrector", object()),
                 ("quantize_x0", True)):
        with pytest.raises(ValueError, match=f"{k} is not available in a session"):
            sess.submit(**dict(ok, **{k: v}))
    long_c = torch.zeros(V.T + 1, tiny["c"].shape[2])
    with pytest.raises(MdxError, match=f"{V.T + 1} context tokens"):
        sess.submit(**dict(ok, c=long_c))
    with pytest.raises(MdxError, match="only whole 77-token windows can be padded"):
        sess.submit(**dict(ok, c=tiny["c"][0][:3]))
    with pytest.raises(MdxError, match="width"):
        sess.submit(**dict(ok, c=tiny["c"][0][:, :-1]))
    with pytest.raises(MdxError, match="pass uc="):
        sess.submit(**dict(ok, uc=None))
    with pytest.raises(MdxError, match="either prompt= or c="):
        sess.submit(**dict(ok, prompt="a cat"))
    with pytest.raises(MdxError, match="text encoder"):
        sess.submit(prompt="a cat", steps=2)
    assert sess.scheduler.idle and sess.step() == [] and sess.tick_count == 0     # nothing was queued, nothing ran

    class Hybrid:
        conditioning_key = "hybrid"
    eps = tiny["eps"]
    wrapper = eps.model
    try:
        eps.model = Hybrid()
        with pytest.raises(MdxError, match="conditioning_key='hybrid'"):
            pipe.session(slots=2, H=64, W=64, context_len=V.T)
    finally:
        eps.model = wrapper
    with pytest.raises(ValueError, match="eta"):
        pipeline(tiny, "eps", "dpm").session(slots=2, H=64, W=64, context_len=V.T, max_steps=4).submit(**dict(ok, eta=0.5))


def test_an_empty_slot_evaluates_finite_numbers(tiny):
    """One request in three slots: the two empty slots ride along on zeros and the request equals its batch-3 reference."""
    sess = pipeline(tiny, "v", "ddim").session(slots=SLOTS, H=64, W=64, context_len=V.T, max_steps=4)
    h = sess.submit(**requests(tiny, "ddim")[0])
    sess.run_until_idle()
    assert bool(torch.isfinite(sess.x).all()) and not bool(sess.x[1:].any())
    assert torch.equal(h.latent, reference(tiny, "v", "ddim", 0, 0))


def test_a_shorter_context_is_padded_with_whole_empty_windows():
    """A 77-token request in a 154-token session runs on [c | empty]: the batch-3 run handed that context explicitly."""
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.pipeline import DiffusionPipeline
    model, cfg, _ = V.tiny_eps_model()                            # its own model: the session raises the UNet's context capacity
    rng = np.random.RandomState(412)
    d = lambda *s: torch.tensor(rng.randn(*s).astype(np.float32), device=DEV)
    c, uc, empty = d(1, 77, cfg["context_dim"]), d(1, 77, cfg["context_dim"]), d(1, 77, cfg["context_dim"])
    pipe = DiffusionPipeline(model, "ddim", device=DEV)
    with pytest.raises(MdxError, match="nothing to pad it with"):
        pipe.session(slots=SLOTS, H=64, W=64, context_len=154, max_steps=4).submit(c=c, uc=uc, steps=2, seed=3)
    sess = pipe.session(slots=SLOTS, H=64, W=64, context_len=154, max_steps=4, empty=empty)
    h = sess.submit(c=c[0], uc=uc, steps=2, scale=3.0, guidance_rescale=0.5, seed=3)
    sess.run_until_idle()
    pad = lambda t: torch.cat([t, empty], 1).expand(3, -1, -1).contiguous()
    want = DDIMSampler(model).sample([2] * 3, 3, LATENT, conditioning=pad(c), unconditional_conditioning=pad(uc),
                                     seeds=[3, 4, 5], unconditional_guidance_scale=[3.0] * 3, guidance_rescale=[0.5] * 3,
                                     verbose=False)[0]
    assert bool(torch.isfinite(h.latent).all()) and torch.equal(h.latent, want[0])
