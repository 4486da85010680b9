"""Inpainting -- the parts that need no GPU: the host-side argument checks of the four entries of csrc/inpaint.hip (every refusal
names its entry and happens before any launch), the refusals of DiffusionPipeline.inpaint / inpaint_conditioning and of
DPMSolverSampler's dict conditioning, and the numpy restatements the GPU tests compare against (tests/_inpaint_util.py)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _inpaint_util as U

P = 1 << 20         # disjoint non-null addresses P, 2P, ...: nothing is dereferenced by a refused call


def _refuser(entry, call):
    from minddiffusion_amd import _lib
    lib = _lib.load()

    def refused(msg, **kw):
        assert call(lib, **kw) == -1
        err = lib.mdx_last_error()
        assert entry in err and msg in err, err
    return refused


def test_mask_image_argument_validation_without_gpu():
    def call(lib, image=P, mask=2 * P, mask_b=1, out=3 * P, B=2, C=3, HW=35):
        return lib.mdx_inpaint_mask_image_f32(image, mask, mask_b, out, B, C, HW, None)
    refused = _refuser(b"mdx_inpaint_mask_image_f32", call)
    refused(b"null pointer", image=None)
    refused(b"null pointer", mask=None)
    refused(b"null pointer", out=None)
    for kw in ({"B": 0}, {"C": 0}, {"HW": -3}):
        refused(b"bad extents", **kw)
    for mb in (0, 3, -1):
        refused(b"mask_b must be 1 or B", mask_b=mb)
    refused(b"out overlaps mask", out=2 * P + 16)


def test_concat_argument_validation_without_gpu():
    def call(lib, mom=P, ld=8, mask=2 * P, mask_b=1, H=6, W=10, out=3 * P, B=2, zc=4, h=3, w=5):
        return lib.mdx_inpaint_concat_f32(mom, ld, None, 0.18215, mask, mask_b, H, W, out, B, zc, h, w, None)
    refused = _refuser(b"mdx_inpaint_concat_f32", call)
    refused(b"null pointer", mom=None)
    refused(b"null pointer", mask=None)
    refused(b"null pointer", out=None)
    refused(b"bad extents", ld=7)                   # ld >= 2 zc
    for kw in ({"B": 0}, {"zc": -1}, {"h": 0}, {"w": 0}, {"H": 0}, {"W": -1}):
        refused(b"bad extents", **kw)
    refused(b"bad extents", H=1 << 16, W=1 << 16)   # a plane the int pixel index cannot hold
    for mb in (0, 3):
        refused(b"mask_b must be 1 or B", mask_b=mb)
    from minddiffusion_amd import _lib
    assert _lib.SIGNATURES["mdx_inpaint_concat_f32"][1][3] is ctypes.c_float       # scale_factor


def test_feather_argument_validation_without_gpu():
    def call(lib, mask=P, wts=2 * P, radius=3, out=3 * P, Bm=1, H=16, W=24):
        return lib.mdx_mask_feather_f32(mask, wts, radius, out, Bm, H, W, None)
    refused = _refuser(b"mdx_mask_feather_f32", call)
    refused(b"null pointer", mask=None)
    refused(b"null pointer", wts=None)
    refused(b"null pointer", out=None)
    for kw in ({"Bm": 0}, {"H": 0}, {"W": -2}):
        refused(b"bad extents", **kw)
    for r in (-1, 49, 1000):
        refused(b"radius must be in [0, 48]", radius=r)
    refused(b"out overlaps mask", out=P + 64)


def test_composite_argument_validation_without_gpu():
    def call(lib, dec=P, image=2 * P, alpha=3 * P, alpha_b=1, out_f32=4 * P, out_u8=5 * P, B=2, C=3, H=5, W=7):
        return lib.mdx_inpaint_composite_f32(dec, image, alpha, alpha_b, out_f32, out_u8, B, C, H, W, None)
    refused = _refuser(b"mdx_inpaint_composite_f32", call)
    refused(b"null pointer", dec=None)
    refused(b"null pointer", image=None)            # alpha needs the image
    refused(b"no output", out_f32=None, out_u8=None)
    for kw in ({"B": 0}, {"C": 0}, {"H": 0}, {"W": -1}):
        refused(b"bad extents", **kw)
    for ab in (0, 3):
        refused(b"alpha_b must be 1 or B", alpha_b=ab)
    refused(b"out_f32 overlaps an input", out_f32=P)
    refused(b"out_f32 overlaps an input", out_f32=2 * P + 4)
    refused(b"out_f32 overlaps an input", out_f32=3 * P)


# ------------------------------------------------------------------------------------------------ Python validation
def _ldm(**kw):
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    return LatentDiffusion(object(), linear_start=0.00085, linear_end=0.0120, timesteps=1000, **kw)


def _pipe(sampler, **kw):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    return DiffusionPipeline(_ldm(**kw), sampler, device="cpu")


def test_inpaint_refusals(monkeypatch):
    from minddiffusion_amd import distributed
    from minddiffusion_amd._lib import MdxError
    img, mask, c = torch.zeros(1, 3, 16, 16), torch.ones(1, 1, 16, 16), torch.zeros(2, 7, 64)
    for sampler in ("ddim", "plms", "dpm_solver"):
        p = _pipe(sampler)
        for bad in (0.0, -0.1, 1.01, float("nan")):
            with pytest.raises(ValueError, match="strength"):
                p.inpaint(img, mask, c=c, strength=bad)
        with pytest.raises(ValueError, match="strength"):
            p.inpaint(img, mask, c=c, strength=0.01, steps=30)              # t_enc = int(0.3) = 0
        for bad in ("u8", "pil", None):
            with pytest.raises(ValueError, match="output"):
                p.inpaint(img, mask, c=c, output=bad)
        with pytest.raises(ValueError, match="radius"):
            p.inpaint(img, mask, c=c, mask_blur=16.5)                       # ceil(3 sigma) = 50 > 48
        with pytest.raises(ValueError, match="mask_blur"):
            p.inpaint(img, mask, c=c, mask_blur=-1.0)
        with pytest.raises(ValueError, match="guidance_rescale"):
            p.inpaint(img, mask, c=c, guidance_rescale=1.5)
        with pytest.raises(MdxError, match="prompts"):
            p.inpaint(img, mask)
        # batches: image and mask are 1 or the conditioning's batch
        with pytest.raises(MdxError, match="3 images and 1 masks for a batch of 2"):
            p.inpaint(torch.zeros(3, 3, 16, 16), mask, c=c)
        with pytest.raises(MdxError, match="1 images and 3 masks for a batch of 2"):
            p.inpaint(img, torch.ones(3, 1, 16, 16), c=c)
        with pytest.raises(MdxError, match="2 images and 2 masks for a batch of 1"):
            p.inpaint(torch.zeros(2, 3, 16, 16), torch.ones(2, 1, 16, 16), c=c[:1])
        with pytest.raises(MdxError, match="mask is"):
            p.inpaint(img, torch.ones(1, 1, 16, 8), c=c)
        with pytest.raises(MdxError, match=r"\[B, 1, H, W\]"):
            p.inpaint(img, torch.ones(1, 3, 16, 16), c=c)
        with pytest.raises(MdxError, match="seeds"):
            p.inpaint(img, mask, c=c, seeds=[1, 2, 3])
    # a plain 4-channel model blends under the mask: DPM-Solver refuses, as img2img(mask=) does
    with pytest.raises(NotImplementedError, match="PLMSSampler"):
        _pipe("dpm_solver").inpaint(img, mask, c=c)
    for kw in ({}, {"conditioning_key": "hybrid"}):
        with pytest.raises(MdxError, match="first_stage_model"):
            _pipe("plms", **kw).inpaint(img, mask, c=c)                      # no VAE attached
        with pytest.raises(MdxError, match="first_stage_model"):
            _pipe("plms", **kw).inpaint_conditioning(img, mask)
    monkeypatch.setattr(distributed, "world", lambda: (0, 2))
    with pytest.raises(MdxError, match="single rank"):
        _pipe("plms").inpaint(img, mask, c=c)


def test_feather_weights_are_the_float64_gaussian():
    from minddiffusion_amd import ops
    for sigma, radius in ((1.0, 3), (2.0, 6), (0.4, 2), (16.0, 48)):
        r, w = ops.feather_weights(sigma)
        k = np.arange(-radius, radius + 1, dtype=np.float64)
        ref = np.exp(-0.5 * (k / sigma) ** 2)
        assert r == radius and w.dtype == np.float32 and np.array_equal(w, (ref / ref.sum()).astype(np.float32))
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= (2 * radius + 1) * 2.0 ** -24
    for bad in (0.0, -1.0, float("nan"), float("inf"), 16.1):
        with pytest.raises(ValueError, match="mask_blur"):
            ops.feather_weights(bad)


def test_dpm_solver_dict_conditioning_still_refuses_mask_and_cpu_tensors():
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    s = DPMSolverSampler(_ldm(conditioning_key="hybrid"))
    cond = {"c_concat": torch.zeros(1, 5, 8, 8), "c_crossattn": torch.zeros(1, 7, 64)}
    with pytest.raises(NotImplementedError):
        s.sample(3, 1, (4, 8, 8), conditioning=cond, unconditional_conditioning=cond, mask=torch.ones(1, 1, 8, 8),
                 x0=torch.zeros(1, 4, 8, 8))
    with pytest.raises(MdxError, match="CUDA"):                     # the dict was taken apart: its text context is checked
        s.sample(3, 1, (4, 8, 8), conditioning=cond, unconditional_conditioning=cond)


# ------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("ratio", [2, 8])
def test_integer_nearest_rule_is_interpolate_nearest_at_integer_ratios(ratio):
    rng = np.random.RandomState(3)
    for h, w in ((3, 5), (8, 8), (1, 7)):
        m = (rng.rand(2, 1, h * ratio, w * ratio) > 0.5).astype(np.float32)
        ref = F.interpolate(torch.tensor(m), size=(h, w), mode="nearest").numpy()
        assert np.array_equal(U.resize_nearest(m, h, w), ref)
        assert np.array_equal(U.nearest_index(h, h * ratio), np.arange(h) * ratio)


def test_integer_nearest_rule_at_a_non_integer_ratio():
    # 5 x 7 -> 2 x 3: rows (0 * 5) // 2, (1 * 5) // 2 = 0, 2; columns 0, 2, 4 -- every index inside the source
    assert U.nearest_index(2, 5).tolist() == [0, 2] and U.nearest_index(3, 7).tolist() == [0, 2, 4]
    for n_out in range(1, 40):
        for n_in in range(1, 40):
            idx = U.nearest_index(n_out, n_in)
            assert idx.min() >= 0 and idx.max() < n_in and np.all(np.diff(idx) >= 0)


def test_make_batch_sd_restatement():
    rng = np.random.RandomState(5)
    image = rng.uniform(-1, 1, (1, 3, 6, 10)).astype(np.float32)
    mask = rng.rand(1, 1, 6, 10).astype(np.float32)
    mask[0, 0, 0, :3] = (0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.0)
    b = U.make_batch_sd(image, mask, 3)
    assert b["image"].shape == (3, 3, 6, 10) and b["mask"].shape == (3, 1, 6, 10) and b["masked_image"].shape == (3, 3, 6, 10)
    assert set(np.unique(b["mask"])) == {0.0, 1.0} and b["mask"][0, 0, 0, :3].tolist() == [1.0, 0.0, 0.0]
    # the torch expression the mask-image kernel is held to, on the raw and on the binarised mask
    t = (torch.tensor(image) * (torch.tensor(mask) < 0.5)).numpy()
    assert np.array_equal(b["masked_image"][1], t[0])
    assert np.array_equal(b["masked_image"][2], (torch.tensor(image) * (torch.tensor(b["mask"][:1]) < 0.5)).numpy()[0])
    hole = b["mask"][0, 0] == 1
    assert np.all(b["masked_image"][0][:, hole] == 0) and np.array_equal(b["masked_image"][0][:, ~hole], image[0][:, ~hole])


@pytest.mark.parametrize("sigma", [1.0, 2.0, 5.0])
def test_alpha_is_one_on_the_hole_and_in_the_unit_interval(sigma):
    from minddiffusion_amd import ops
    rng = np.random.RandomState(7)
    mask = np.zeros((2, 1, 16, 24), np.float32)
    mask[0, 0, 4:9, 6:15] = 1.0
    mask[1, 0] = rng.rand(16, 24) > 0.7
    mask[1, 0, 0, 0] = mask[1, 0, 15, 23] = 1.0         # holes in the corners: the replicate edge
    _, w = ops.feather_weights(sigma)
    a = U.feather_ref(mask, w)
    m = U.binarise(mask)
    assert np.all(a[m == 1] == 1.0) and a.min() >= 0.0 and a.max() <= 1.0 + 1e-6
    assert np.all(a >= m) and np.any((a > 0) & (a < 1))          # the ramp is outside the hole only
    far = np.zeros_like(m[0, 0], bool)
    far[:, 20:] = True                                            # columns >= 20 are farther than ... only at sigma 1
    if sigma == 1.0:
        assert np.all(a[0, 0][far] == 0.0)                        # beyond the radius (3) of the hole's edge (column 14)
