"""img2img and masked-blend requests in a sampling session, end to end on the GPU: six requests per sampler kind -- plain
text-to-image ones, img2img ones of several (steps, strength) pairs, two of them with a keep_mask -- go through a 3-slot session,
five submitted at once and the sixth after two ticks.

The reference of an img2img request that ran in slot b is the aligned-batch path: pipe.img2img(init_latent=, strength=, steps=,
scale=[..], guidance_rescale=[..], seeds=[..], mask=) at batch 3 with the request's operands in row b (two other requests fill
the other rows; all rows take the request's steps and strength, since one grid serves that call).  The reference of a plain
request is sampler.sample at batch 3, as tests/test_session_gpu.py builds it.  Every latent must be torch.equal to row b of its
reference: no tolerance anywhere.
"""
import numpy as np
import pytest
import torch

import _vpred_util as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LATENT = (4, 8, 8)
SLOTS = 3
# (steps, strength or None for a plain request, keep_mask?) in submission order.  DDIM has grids for {1, 2, 4} steps; a partial
# run walks the last t_enc points of its `steps` grid, so any t_enc <= steps has rows.  ticks = t_enc = int(strength * steps).
#   ddim: ticks [2, 4, 1, 3, 4, 2] -> slots 0 1 2 | 2 at tick 1 (after the blending (2, 0.5)) | 0 at tick 2 (after the blending
#         (4, 0.5)) | 1 at tick 4
#   dpm:  ticks [1, 4, 3, 3, 4, 3] -> slots 0 1 2 | 0 at tick 1 | 2 at tick 3 | 0 at tick 4
_DDIM = [(4, 0.5, True), (4, None, False), (2, 0.5, True), (4, 0.75, False), (4, 1.0, False), (2, None, False)]
SPEC = {"ddim": _DDIM, "ddim_eta1": _DDIM,
        "dpm": [(4, 0.25, False), (4, None, False), (6, 0.5, False), (4, 0.75, False), (4, 1.0, False), (3, None, False)]}
SCALES = [1.5, 3.0, 7.5, 5.0, 2.0, 4.0]
PHIS = [0.0, 0.7, 0.3, 0.0, 1.0, 0.5]
SEEDS = [5, 7, 9, -11, (1 << 63) + 13, 21]
RELEASE = [0, 0, 0, 0, 0, 2]                  # the tick before which each request is submitted
MAX_STEPS = 6
KINDS = sorted(SPEC)
N = 6


def t_enc_of(steps, strength):
    return steps if strength is None else int(strength * steps)


def packing(ticks, release=RELEASE):
    """FIFO into the lowest free slot: (slot, start) of every request and the tick count."""
    free, placed = [0] * SLOTS, []
    for n, rel in zip(ticks, release):
        start = max(min(free), rel)
        b = min(i for i in range(SLOTS) if free[i] <= start)
        placed.append((b, start))
        free[b] = start + n
    return placed, max(free)


@pytest.fixture(scope="module")
def tiny():
    v_model, cfg, _ = V.tiny_eps_model(parameterization="v")
    eps_model, _, _ = V.tiny_eps_model()
    rng = np.random.RandomState(511)
    d = lambda a: torch.tensor(a.astype(np.float32), device=DEV)
    keep = rng.rand(N, 1, 8, 8)
    pick = rng.randint(0, 3, size=keep.shape)
    keep[pick == 0], keep[pick == 1] = 0.0, 1.0               # exact 0, exact 1 and fractions
    return {"v": v_model, "eps": eps_model, "c": d(rng.randn(N, V.T, cfg["context_dim"])),
            "uc": d(rng.randn(N, V.T, cfg["context_dim"])), "z0": d(rng.randn(N, *LATENT)), "keep": d(keep)}


def pipeline(tiny, param, kind):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    return DiffusionPipeline(tiny[param], "dpm_solver" if kind == "dpm" else "ddim", device=DEV)


def eta_of(kind):
    return 1.0 if kind == "ddim_eta1" else 0.0


def requests(tiny, kind):
    out = []
    for r, (steps, strength, keep) in enumerate(SPEC[kind]):
        req = dict(c=tiny["c"][r], uc=tiny["uc"][r], steps=steps, scale=SCALES[r], guidance_rescale=PHIS[r], eta=eta_of(kind),
                   seed=SEEDS[r])
        if strength is not None:
            req.update(init_latent=tiny["z0"][r], strength=strength)
        if keep:
            req.update(keep_mask=tiny["keep"][r])
        out.append(req)
    return out


def test_every_t_enc_has_rows():
    """A CPU call of request_rows per (steps, strength) pair used below: the sampler builds the partial run's rows."""
    from minddiffusion_amd.ldm.models.diffusion import session as S
    from test_per_request_cpu import StubModel
    for kind, spec in SPEC.items():
        for steps, strength, _ in spec:
            n = t_enc_of(steps, strength)
            rows, t_in = S.request_rows(StubModel(), "dpm_solver" if kind == "dpm" else "ddim", steps, 3.0, 0.0, eta_of(kind),
                                        None if strength is None else n)
            assert rows.shape[0] == n == t_in.shape[0] and 1 <= n <= MAX_STEPS
    assert [t_enc_of(s, g) for s, g, _ in SPEC["ddim"]] == [2, 4, 1, 3, 4, 2]
    assert [t_enc_of(s, g) for s, g, _ in SPEC["dpm"]] == [1, 4, 3, 3, 4, 3]


def run_session(tiny, param, kind, release=RELEASE):
    """(handles, session) of the six requests, each submitted before the tick RELEASE names."""
    sess = pipeline(tiny, param, kind).session(slots=SLOTS, H=64, W=64, context_len=V.T, max_steps=MAX_STEPS)
    reqs = requests(tiny, kind)
    handles, finished = [], []
    for tick in range(max(release) + 1):
        handles += [sess.submit(**reqs[r]) for r in range(N) if release[r] == tick]
        if tick < max(release):
            finished += sess.step()
    finished += sess.run_until_idle()
    assert sorted(h.index for h, _ in finished) == list(range(N)) and all(lat is h.latent for h, lat in finished)
    return handles, sess


_REFERENCE = {}


def reference(tiny, param, kind, r, b, plain=False):
    """Row b of the batch-3 aligned run whose row b is request r: pipe.img2img for an img2img request, sampler.sample for a
    plain one (plain=True: request r's seed and parameters as a txt2img run).  Once per (model, sampler, request, slot)."""
    key = (param, kind, r, b, plain)
    if key not in _REFERENCE:
        who = [(r + 1) % N, (r + 2) % N]
        who.insert(b, r)                                            # request r in row b, two others around it
        steps, strength, keep = SPEC[kind][r]
        pipe = pipeline(tiny, param, kind)
        lists = dict(scale=[SCALES[i] for i in who], guidance_rescale=[PHIS[i] for i in who], seeds=[SEEDS[i] for i in who])
        if strength is None or plain:
            out = pipe.sampler.sample([steps] * 3, 3, LATENT, conditioning=tiny["c"][who],
                                      unconditional_conditioning=tiny["uc"][who], seeds=lists["seeds"],
                                      unconditional_guidance_scale=lists["scale"], guidance_rescale=lists["guidance_rescale"],
                                      eta=eta_of(kind), verbose=False)[0]
        else:
            out = pipe.img2img(init_latent=tiny["z0"][who], strength=strength, steps=steps, eta=eta_of(kind),
                               mask=tiny["keep"][who] if keep else None, c=tiny["c"][who], uc=tiny["uc"][who], **lists)
        _REFERENCE[key] = out[b].clone()
    return _REFERENCE[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("param", ["eps", "v"])
def test_every_request_equals_its_row_of_the_aligned_batch(tiny, param, kind):
    handles, sess = run_session(tiny, param, kind)
    spec = SPEC[kind]
    ticks = [t_enc_of(s, g) for s, g, _ in spec]
    placed, total = packing(ticks)
    assert [(h.slot, h.start) for h in handles] == placed and [h.steps for h in handles] == ticks
    assert sess.tick_count == total == sess.unet_evals and sess.admissions == N
    # an img2img request enters a slot vacated mid-run on an odd tick
    assert placed[3] == ((2, 1) if kind != "dpm" else (0, 1)) and spec[3][1] is not None
    if kind == "dpm":
        assert sess.blend_on is None and sess.blend_launches == 0
    else:
        # slots 2 and 0 go from a blending tenant (requests 2 and 0) to one that does not blend (requests 3 and 4); the blend
        # runs on the ticks some active slot blends: 0 and 1
        assert placed[2][0] == placed[3][0] and spec[2][2] and not spec[3][2]
        assert placed[0][0] == placed[4][0] and spec[0][2] and not spec[4][2] and placed[4][1] == 2
        assert sess.blend_launches == 2 and sess.blend_on.tolist() == [0, 0, 0]
    for r, h in enumerate(handles):
        assert h.done and tuple(h.latent.shape) == LATENT and bool(torch.isfinite(h.latent).all())
        want = reference(tiny, param, kind, r, h.slot)
        print(f"{param} {kind} request {r} {spec[r]} (slot {h.slot}, tick {h.start}): "
              f"max|d| {float((h.latent - want).abs().max()):.3e}")
        assert torch.equal(h.latent, want), (param, kind, r)
    # strength 1.0 runs all its steps from a noised image, not from RNG_X_T noise: another result than the seed's txt2img run
    assert spec[4][:2] == (4, 1.0) and handles[4].steps == 4
    assert not torch.equal(handles[4].latent, reference(tiny, param, kind, 4, handles[4].slot, plain=True))


@pytest.mark.parametrize("kind", ["ddim_eta1", "dpm"])
def test_serve_returns_a_mixed_list_in_request_order(tiny, kind):
    """All six at once through pipe.serve(output='latent'): the latents of a session run with the same submissions, in request
    order, each torch.equal to its aligned-batch reference in the slot it got."""
    pipe = pipeline(tiny, "v", kind)
    lat = pipe.serve(requests(tiny, kind), slots=SLOTS, H=64, W=64, output="latent")
    assert tuple(lat.shape) == (N,) + LATENT
    handles, sess = run_session(tiny, "v", kind, release=[0] * N)
    placed, total = packing([t_enc_of(s, g) for s, g, _ in SPEC[kind]], [0] * N)
    assert pipe.last_session.tick_count == total == sess.tick_count and [(h.slot, h.start) for h in handles] == placed
    for r, h in enumerate(handles):
        assert torch.equal(lat[r], h.latent), (kind, r)
        assert torch.equal(lat[r], reference(tiny, "v", kind, r, h.slot)), (kind, r)


def test_a_session_without_blending_requests_makes_no_blend_launch(tiny, monkeypatch):
    from minddiffusion_amd import ops
    calls = []
    real = ops.slot_blend
    monkeypatch.setattr(ops, "slot_blend", lambda *a, **k: (calls.append(a[-1]), real(*a, **k))[1])
    sess = pipeline(tiny, "eps", "ddim").session(slots=SLOTS, H=64, W=64, context_len=V.T, max_steps=MAX_STEPS)
    reqs = requests(tiny, "ddim")
    for r in (1, 3, 4):                                              # plain, (4, 0.75) and (4, 1.0): no keep_mask
        sess.submit(**reqs[r])
    sess.run_until_idle()
    assert calls == [] and sess.blend_launches == 0 and sess.blend_on is None and sess.x0 is None
    h = sess.submit(**reqs[0])                                       # (4, 0.5) with a keep_mask: two ticks, two launches
    sess.run_until_idle()
    assert calls == [4, 5] and sess.blend_launches == 2 and h.start == 4 and sess.blend_on.tolist() == [1, 0, 0]
    assert torch.equal(h.latent, reference(tiny, "eps", "ddim", 0, 0))


def test_an_init_image_is_its_encoded_latent(tiny):
    """serve([{init_image=img}]) is torch.equal to serve([{init_latent=z0}]) with z0 the z0 output of vae.encode_noised(img[None])
    at batch 1 under the (seed, RNG_POSTERIOR, 0) draw: the header promises xt_out is mdx_q_sample_f32 of z0_out.  The tiny VAE
    downsamples by 2: a 16 x 16 image is an 8 x 8 latent."""
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
    from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
    from minddiffusion_amd.ldm.models.diffusion import session as S
    from minddiffusion_amd.pipeline import DiffusionPipeline
    from oracle import vae as OV
    dd = dict(TINY_VAE_DDCONFIG)
    vae = AutoencoderKL(ddconfig=dd, embed_dim=4, device=DEV)
    vae.load_state_dict(OV.init_params(dd, seed=8))
    model, _, _ = V.tiny_eps_model(scale_factor=0.18215)
    model.first_stage_model = vae
    pipe = DiffusionPipeline(model, "ddim", device=DEV)
    rng = np.random.RandomState(77)
    imgs = torch.tensor(np.clip(rng.randn(2, 3, 16, 16) * 0.5, -1, 1).astype(np.float32), device=DEV)
    base = [dict(c=tiny["c"][r], uc=tiny["uc"][r], steps=4, strength=(0.5, 0.75)[r], scale=SCALES[r], guidance_rescale=PHIS[r],
                 seed=SEEDS[r + 3]) for r in range(2)]
    base[0]["keep_mask"] = tiny["keep"][0]
    z0s = []
    for r in range(2):
        seed = ops.seeds_tensor([SEEDS[r + 3]], DEV)
        a, b = S.start_coefficients(model, "ddim", 4, int(base[r]["strength"] * 4))
        z0, _ = vae.encode_noised(imgs[r:r + 1], model.scale_factor, a, b, ops.randn_seeded(seed, ops.RNG_ENCODE, 0, LATENT),
                                  post_noise=ops.randn_seeded(seed, ops.RNG_POSTERIOR, 0, LATENT), sample=True)
        z0s.append(z0[0].clone())
    from_image = pipe.serve([dict(q, init_image=imgs[r]) for r, q in enumerate(base)], slots=2, H=64, W=64, output="latent")
    from_latent = pipe.serve([dict(q, init_latent=z0s[r]) for r, q in enumerate(base)], slots=2, H=64, W=64, output="latent")
    assert bool(torch.isfinite(from_image).all()) and torch.equal(from_image, from_latent)
    assert not torch.equal(from_image[0], from_image[1])
    # the posterior's mode is another start latent
    sess = pipe.session(slots=2, H=64, W=64, context_len=V.T, max_steps=4, sample_posterior=False)
    h = sess.submit(**dict(base[1], init_image=imgs[1][None]))
    sess.run_until_idle()
    assert bool(torch.isfinite(h.latent).all()) and not torch.equal(h.latent, from_image[1])
    with pytest.raises(MdxError, match="encodes to a latent"):
        sess.submit(**dict(base[1], init_image=torch.zeros(3, 32, 32, device=DEV)))
    with pytest.raises(ValueError, match="at most one"):
        sess.submit(**dict(base[1], init_image=imgs[1], init_latent=z0s[1]))
