"""img2img and masked-blend requests in a sampling session -- the parts that need no GPU: the validation of submit's new
keywords, the refusals that stay, the slot scheduler on a request that holds its slot for t_enc ticks, the rows of a partial run
against the samplers' own StepTable, and the host refusals and the C-ABI declaration of mdx_slot_blend_f32."""
import os
import re

import numpy as np
import pytest
import torch

from minddiffusion_amd import _lib, ops
from minddiffusion_amd._lib import MdxError
from minddiffusion_amd.ldm.models.diffusion import schedule as SCH
from minddiffusion_amd.ldm.models.diffusion import session as S
from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP
from test_per_request_cpu import StubModel
from test_session_cpu import Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (4, 8, 8)


def chk(sampler="ddim", steps=4, vae=None, **kw):
    return S.check_init(sampler, steps, SHAPE, vae, **kw)


def test_the_new_keywords_are_validated():
    z0, img, keep = torch.zeros(SHAPE), torch.zeros(3, 16, 16), torch.ones(1, 8, 8)
    assert chk() == (None, None, None, None)
    t_enc, lat, image, mask = chk(init_latent=z0[None], keep_mask=keep)
    assert t_enc == 3 and tuple(lat.shape) == SHAPE and image is None and tuple(mask.shape) == (1, 8, 8)    # strength 0.75
    assert chk(init_latent=z0, strength=0.5)[0] == 2 and chk(init_latent=z0, strength=1.0)[0] == 4
    assert tuple(chk(init_latent=z0, keep_mask=torch.ones(SHAPE))[3].shape) == SHAPE
    assert chk("dpm_solver", steps=6, init_latent=z0, strength=0.5)[0] == 3
    with pytest.raises(ValueError, match="at most one of init_latent and init_image"):
        chk(init_latent=z0, init_image=img)
    with pytest.raises(ValueError, match="strength needs an init"):
        chk(strength=0.5)
    with pytest.raises(ValueError, match="keep_mask needs an init"):
        chk(keep_mask=keep)
    for bad in (0.0, -0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"strength must be in \(0, 1\]"):
            chk(init_latent=z0, strength=bad)
    with pytest.raises(ValueError) as e:                                # t_enc == 0: the message of check_strength
        chk(init_latent=z0, strength=0.2)
    with pytest.raises(ValueError) as want:
        SCH.check_strength("submit", 0.2, 4)
    assert str(e.value) == str(want.value) and "leaves no step of 4 to run" in str(e.value)
    with pytest.raises(NotImplementedError, match="mask blending is implemented by PLMSSampler / DDIMSampler"):
        chk("dpm_solver", init_latent=z0, keep_mask=keep)
    for bad in (torch.zeros(4, 8, 9), torch.zeros(3, 8, 8), torch.zeros(2, 4, 8, 8), torch.zeros(8, 8), np.zeros(SHAPE)):
        with pytest.raises(MdxError, match="init_latent"):
            chk(init_latent=bad)
    for bad in (torch.ones(2, 8, 8), torch.ones(1, 8, 9), torch.ones(8, 8), torch.ones(2, 1, 8, 8)):
        with pytest.raises(MdxError, match="keep_mask"):
            chk(init_latent=z0, keep_mask=bad)
    with pytest.raises(MdxError, match="init_image= needs a VAE"):
        chk(init_image=img)
    with pytest.raises(MdxError, match="init_image= needs a VAE"):
        chk(init_image=img, vae=object())                               # no encode_noised

    class Vae:
        def encode_noised(self):
            pass

        def latent_shape(self, s):
            return (s[0], 4, s[2] // 2, s[3] // 2)

    assert tuple(chk(init_image=img[None], vae=Vae())[2].shape) == (3, 16, 16)
    with pytest.raises(MdxError, match="encodes to a latent"):
        chk(init_image=torch.zeros(3, 32, 32), vae=Vae())
    with pytest.raises(MdxError, match="init_image"):
        chk(init_image=torch.zeros(1, 16, 16), vae=Vae())


def test_the_pinned_refusals_stay():
    ok = dict(steps=4, scale=7.5, guidance_rescale=0.3, eta=0.0, seed=5)
    for k in ("mask", "x0"):                                            # refused by name; the sentence now says what to pass
        with pytest.raises(ValueError, match=f"{k} is not available in a session: .*init_latent.*keep_mask"):
            S.check_request("ddim", 50, **dict(ok, **{k: object()}))
    import inspect
    params = inspect.signature(S.SamplingSession.submit).parameters
    assert all(params[k].default is None for k in ("init_latent", "init_image", "strength", "keep_mask"))
    for k in ("strength", "init_latent", "keep_mask"):                  # not check_request's: check_init's
        with pytest.raises(TypeError, match="unexpected keyword"):
            S.check_request("ddim", 50, **dict(ok, **{k: 0.5}))


def test_an_img2img_request_holds_its_slot_for_t_enc_ticks():
    """(steps, strength) -> ticks: (4, 0.5) -> 2, plain 4 -> 4, (4, 0.75) -> 3, (2, 0.5) -> 1, in 2 slots."""
    model = StubModel()
    spec = [(4, 0.5), (4, None), (4, 0.75), (2, 0.5)]
    rec = Recorder()
    sch = S.SlotScheduler(2, rec)
    reqs = []
    for steps, strength in spec:
        t_enc = None if strength is None else chk(steps=steps, init_latent=torch.zeros(SHAPE), strength=strength)[0]
        rows, t_in = S.request_rows(model, "ddim", steps, 3.0, 0.0, 0.0, t_enc)
        reqs.append(sch.submit(len(rows), rows, t_in))
    assert [r.steps for r in reqs] == [2, 4, 3, 1]
    sch.run_until_idle()
    free, placed = [0, 0], []
    for r in reqs:                                                  # FIFO into the slot that frees first, from t_enc
        b = free.index(min(free))
        placed.append((b, free[b]))
        free[b] += r.steps
    assert [(r.slot, r.start) for r in reqs] == placed == [(0, 0), (1, 0), (0, 2), (1, 4)]
    assert sch.now == max(free) == 5
    assert [c[1] for c in rec.calls if c[0] == "tick"] == [0, 1, 2, 3, 4]
    assert rec.calls.index(("retire", 0, 0)) < rec.calls.index(("admit", 2, 0, 2))      # after 2 ticks, not 4


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_ddim_partial_rows_are_the_step_tables(eta):
    model = StubModel()
    sampler = DDIMSampler(model)
    for steps, t_enc, scale, phi in ((4, 2, 1.5, 0.0), (4, 3, 3.0, 0.7), (2, 1, 7.5, 0.3), (4, 4, 2.0, 1.0), (50, 30, 5.0, 0.0)):
        sampler.make_schedule(steps, ddim_eta=eta, verbose=False)
        grid = sampler.time_grid(False, None, t_enc)
        one, t_one, total = SCH.step_table([SCH.ddim_steps(sampler, grid, False)], [scale], [phi], True)
        rows, t_in = S.request_rows(model, "ddim", steps, scale, phi, eta, t_enc=t_enc)
        assert total == t_enc and rows.shape == (t_enc, ops.STEP_ROW) and rows.dtype == np.float32
        assert np.array_equal(rows.view(np.uint32), one.host()[:, 0].view(np.uint32))
        assert np.array_equal(t_in, t_one[:, 0]) and np.array_equal(t_in, np.flip(sampler.ddim_timesteps[:t_enc]))
        full, t_full = S.request_rows(model, "ddim", steps, scale, phi, eta)
        assert np.array_equal(full[steps - t_enc:].view(np.uint32), rows.view(np.uint32))    # the tail of the full run
        assert np.array_equal(t_full[steps - t_enc:], t_in)
        # the full form is what it was: the rows of the whole grid
        whole, t_whole, _ = SCH.step_table([SCH.ddim_steps(sampler, sampler.time_grid(False, None, None), False)], [scale],
                                           [phi], True)
        assert np.array_equal(full.view(np.uint32), whole.host()[:, 0].view(np.uint32)) and np.array_equal(t_full, t_whole[:, 0])
        # the start level and the blend coefficients: the sampler's own tables
        a, b = S.start_coefficients(model, "ddim", steps, t_enc, eta)
        assert (a, b) == sampler.q_coefficients(t_enc)
        ab = S.blend_coefficients(model, t_in)
        assert ab.dtype == np.float32 and ab.shape == (t_enc, 2)
        for i, t in enumerate(t_in):
            assert ab[i, 0] == sampler.sqrt_alphas_cumprod[int(t)] and ab[i, 1] == sampler.sqrt_one_minus_alphas_cumprod[int(t)]
    with pytest.raises(ValueError, match="t_enc"):
        S.request_rows(model, "ddim", 4, 2.0, t_enc=5)
    with pytest.raises(ValueError, match="t_enc"):
        S.request_rows(model, "ddim", 4, 2.0, t_enc=0)


def test_dpm_partial_rows_are_the_step_tables():
    model = StubModel()
    d = DPMSolverSampler(model)
    ns = NoiseScheduleVP("discrete", alphas_cumprod=d.alphas_cumprod)
    t_0 = 1.0 / d.alphas_cumprod.shape[0]
    for steps, t_enc, scale, phi in ((4, 3, 1.5, 0.0), (6, 3, 3.0, 0.7), (4, 4, 7.5, 0.3), (4, 1, 2.0, 1.0)):
        start = t_0 + (1.0 - t_0) * t_enc / steps
        one, t_one, total = SCH.step_table([SCH.dpm_steps(ns, t_enc, start)], [scale], [phi], True)
        rows, t_in = S.request_rows(model, "dpm_solver", steps, scale, phi, t_enc=t_enc)
        assert total == t_enc and rows.shape == (t_enc, ops.STEP_ROW)
        assert np.array_equal(rows.view(np.uint32), one.host()[:, 0].view(np.uint32)) and np.array_equal(t_in, t_one[:, 0])
        assert rows[0, ops.STEP_SIGMA] == 0          # c1 of a newcomer's first row: the previous prediction is not read
        assert S.start_coefficients(model, "dpm_solver", steps, t_enc) == d.q_coefficients(start)
        full, t_full = S.request_rows(model, "dpm_solver", steps, scale, phi)
        whole, t_whole, _ = SCH.step_table([SCH.dpm_steps(ns, steps)], [scale], [phi], True)
        assert np.array_equal(full.view(np.uint32), whole.host()[:, 0].view(np.uint32)) and np.array_equal(t_full, t_whole[:, 0])


def test_slot_blend_is_declared_and_refuses_on_the_host():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.S)
    args = re.search(r"\bint mdx_slot_blend_f32\s*\(([^)]*)\)", header).group(1)
    res, argtypes = _lib.SIGNATURES["mdx_slot_blend_f32"]
    assert res is _lib.c_int and len(argtypes) == len(args.split(",")) == 16 and argtypes[-1] is _lib.c_void_p
    assert argtypes[4] is _lib.c_uint and argtypes[5] is _lib.c_uint          # stream, draw0
    lib = _lib.load()
    names = ("x0", "keep", "img", "seeds", "stream", "draw0", "blend_ab", "blend_on", "slot_start", "slot_len", "cap", "tick",
             "B", "C", "HW", "s")
    good = dict(zip(names, (16, 16, 16, 16, 2, 0, 16, 16, 16, 16, 4, 0, 1, 4, 64, None)))
    call = lambda **kw: lib.mdx_slot_blend_f32(*[dict(good, **kw)[k] for k in names])
    # refused on the host, before any launch: no GPU is needed to see it
    for ptr in ("x0", "keep", "img", "seeds", "blend_ab", "blend_on", "slot_start", "slot_len"):
        assert call(**{ptr: None}) == -1 and b"mdx_slot_blend_f32: null pointer" in lib.mdx_last_error(), ptr
    for kw, word in ((dict(B=0), b"B=0"), (dict(B=65536), b"B=65536"), (dict(C=0), b"C=0"), (dict(HW=0), b"HW=0"),
                     (dict(C=1 << 20, HW=(1 << 14) + 1), b"C * HW <= 2^34")):
        assert call(**kw) == -1 and b"bad extents" in lib.mdx_last_error() and word in lib.mdx_last_error(), kw
    assert call(cap=0) == -1 and b"cap=0" in lib.mdx_last_error() and b"bad slot extents" in lib.mdx_last_error()
    assert call(tick=-1) == -1 and b"tick=-1" in lib.mdx_last_error() and b"bad slot extents" in lib.mdx_last_error()
    assert callable(ops.slot_blend)
