"""Host side of the SRGAN post-upscaler (glide/model/srgan.py, srgan_util.py): the fp32 reference of the Generator (also used by
tests/test_srgan_gpu.py), BatchNorm folding, the depth-to-space index map of MDX_OUT_D2S2, the checkpoint loader and get_img.

The reference restates vision/Taichu-GLIDE/model/glide_text2im/model/srgan.py statement for statement in torch on the CPU:
unfolded BatchNorm (inference mode), per-channel PReLU, DCR depth-to-space written out (not pixel_shuffle), tanh."""
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

TRUNK = 16


# ---------------------------------------------------------------------------------------------------- fp32 reference
def ref_prelu(x, a):                                   # nn.PReLU(channel): x if x > 0 else a[c] * x
    return torch.where(x > 0, x, a.view(1, -1, 1, 1) * x)


def ref_bn(x, gamma, beta, mean, var, eps=1e-5):       # nn.BatchNorm2d, inference mode (moving statistics)
    v = lambda t: t.view(1, -1, 1, 1)
    return v(gamma) * (x - v(mean)) / torch.sqrt(v(var) + eps) + v(beta)


def ref_depth_to_space(x):                             # ops.DepthToSpace(2), DCR: out[n, c, 2h+i, 2w+j] = x[n, (2i+j) C + c, h, w]
    B, C4, H, W = x.shape
    C = C4 // 4
    return x.view(B, 2, 2, C, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, C, 2 * H, 2 * W)


def ref_generator(p, x, factor, pre_tanh=False):
    """srgan.py:75-117 in fp32.  p: name -> torch fp32 tensor (PReLU slopes as `.a`)."""
    conv = lambda t, k, pad: F.conv2d(t, p[k + ".weight"], p[k + ".bias"], padding=pad)
    c1 = ref_prelu(conv(x, "conv1.0", 4), p["conv1.1.a"])                             # srgan.py:83-85, 107
    t = c1
    for i in range(TRUNK):                                                             # srgan.py:88-91, 108
        q = f"trunk.{i}."
        bn = lambda u, b: ref_bn(u, p[q + b + ".gamma"], p[q + b + ".beta"], p[q + b + ".moving_mean"],
                                 p[q + b + ".moving_variance"])
        out = conv(t, q + "conv1", 1)                                                  # srgan.py:51
        out = bn(out, "bn1")                                                           # srgan.py:52
        out = ref_prelu(out, p[q + "prelu.a"])                                         # srgan.py:53
        out = conv(out, q + "conv2", 1)                                                # srgan.py:54
        out = bn(out, "bn2")                                                           # srgan.py:55
        t = out + t                                                                    # srgan.py:56
    c2 = ref_prelu(conv(t, "conv2.0", 1), p["conv2.1.a"])                              # srgan.py:94-96, 109
    out = c1 + c2                                                                      # srgan.py:110
    for j in range(int(math.log(factor, 2))):                                          # srgan.py:99-102, 111
        q = f"subpixel_conv.{j}."
        out = conv(out, q + "conv", 1)                                                 # srgan.py:68
        out = ref_depth_to_space(out)                                                  # srgan.py:69
        out = ref_prelu(out, p[q + "prelu.a"])                                         # srgan.py:70
    out = conv(out, "conv3", 4)                                                        # srgan.py:112
    return out if pre_tanh else torch.tanh(out)                                        # srgan.py:113


def synthetic_params(factor, seed=0, prelu="a"):
    """He-scaled convs (trunk scaled down so 16 residual adds stay O(1)), non-trivial BN statistics, PReLU slopes in
    [-0.3, 0.5].  numpy float32 arrays under the reference names."""
    from minddiffusion_amd.glide.model.srgan import Generator
    rng = np.random.RandomState(seed)
    shapes = Generator(factor, device="cpu").parameter_shapes(prelu)
    p = {}
    for k, shp in shapes.items():
        if k.endswith(".weight"):
            fan_in = shp[1] * shp[2] * shp[3]
            scale = math.sqrt(2.0 / fan_in) * (0.3 if k.startswith("trunk.") else 1.0)
            if k == "conv3.weight":
                scale *= 0.5
            p[k] = rng.standard_normal(shp) * scale
        elif k.endswith(".bias"):
            p[k] = rng.uniform(-0.1, 0.1, shp)
        elif k.endswith(".gamma"):
            p[k] = rng.uniform(0.5, 1.5, shp)
        elif k.endswith(".beta"):
            p[k] = rng.uniform(-0.2, 0.2, shp)
        elif k.endswith(".moving_mean"):
            p[k] = rng.uniform(-0.2, 0.2, shp)
        elif k.endswith(".moving_variance"):
            p[k] = rng.uniform(0.5, 2.0, shp)
        else:                                              # PReLU slope
            p[k] = rng.uniform(-0.3, 0.5, shp)
    return {k: v.astype(np.float32) for k, v in p.items()}


def torch_params(p):
    """name -> fp32 torch tensor (PReLU slopes renamed to `.a`)."""
    out = {}
    for k, v in p.items():
        if k.endswith(".w") and not k.endswith(".weight"):
            k = k[:-2] + ".a"
        t = torch.tensor(np.asarray(v, np.float32))
        out[k] = t
    return out


# ---------------------------------------------------------------------------------------------------- tests
def test_bn_fold_matches_unfolded_batchnorm():
    from minddiffusion_amd.glide.model.srgan import fold_batchnorm
    p = synthetic_params(4, seed=1)
    q = "trunk.3."
    x = torch.tensor(np.random.RandomState(2).standard_normal((2, 64, 7, 9)))
    t = {k: torch.tensor(v.astype(np.float64)) for k, v in p.items() if k.startswith(q)}
    ref = ref_bn(F.conv2d(x, t[q + "conv1.weight"], t[q + "conv1.bias"], padding=1), t[q + "bn1.gamma"], t[q + "bn1.beta"],
                 t[q + "bn1.moving_mean"], t[q + "bn1.moving_variance"])
    wf, bf = fold_batchnorm(p[q + "conv1.weight"], p[q + "conv1.bias"], p[q + "bn1.gamma"], p[q + "bn1.beta"],
                            p[q + "bn1.moving_mean"], p[q + "bn1.moving_variance"])
    got = F.conv2d(x, torch.tensor(wf), torch.tensor(bf), padding=1)
    assert float((got - ref).abs().max()) <= 1e-6


@pytest.mark.parametrize("C", [8, 64])
def test_d2s_weight_rows_and_store_index_equal_depth_to_space(C):
    """Conv output rows permuted by d2s_weight_rows, stored by the MDX_OUT_D2S2 index formula of include/mdx.h, equal the
    explicit DCR depth-to-space of the unpermuted conv output."""
    from minddiffusion_amd.glide.model.srgan import d2s_weight_rows
    rng = np.random.RandomState(C)
    B, H, W = 2, 3, 5
    y = rng.standard_normal((B, 4 * C, H, W)).astype(np.float32)           # conv output, reference channel order
    ref = ref_depth_to_space(torch.tensor(y)).numpy()                      # [B, C, 2H, 2W]
    rows = d2s_weight_rows(C)
    g = y[:, rows].transpose(0, 2, 3, 1).reshape(B * H * W, 4 * C)         # GEMM output: row m = (b, y, x), column n
    Ho, Wo = H, W
    out = np.full((B * 2 * Ho * 2 * Wo * C,), np.nan, np.float32)           # NHWC [B][2H][2W][C], out_ld = C
    for m in range(B * H * W):
        b, r = divmod(m, Ho * Wo)
        yy, xx = divmod(r, Wo)
        for n in range(0, 4 * C, 8):                                       # 8-column groups, as the epilogue stores them
            q, c = divmod(n, C)
            pix = (b * 2 * Ho + 2 * yy + q // 2) * (2 * Wo) + 2 * xx + q % 2
            out[pix * C + c: pix * C + c + 8] = g[m, n:n + 8]
    got = out.reshape(B, 2 * Ho, 2 * Wo, C).transpose(0, 3, 1, 2)
    assert np.array_equal(got, ref)
    # the DCR map is not pixel_shuffle's CRD map
    assert not np.array_equal(F.pixel_shuffle(torch.tensor(y), 2).numpy(), ref)


@pytest.mark.parametrize("spelling", ["a", "w"])
def test_checkpoint_round_trip(tmp_path, spelling, monkeypatch):
    from minddiffusion_amd import ms_checkpoint
    from minddiffusion_amd.glide.model import srgan_util
    from minddiffusion_amd.glide.model.srgan import Generator
    p = synthetic_params(4, seed=3, prelu=spelling)
    path = str(tmp_path / "srgan.ckpt")
    ms_checkpoint.save_checkpoint(p, path)
    seen = {}

    def fake_load(self, params, strict=True):          # the loader's output, before anything touches a device
        seen.update(params)
    monkeypatch.setattr(Generator, "load_state_dict", fake_load)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        srgan_util.SRGAN(4, path, device="cpu")
    want = Generator(4, device="cpu").normalize_keys(p)
    assert sorted(seen) == sorted(want)
    for k in want:
        assert np.array_equal(np.asarray(seen[k]), want[k]), k
    # an extra key warns
    p2 = dict(p, **{"discriminator.extra": np.zeros(3, np.float32)})
    ms_checkpoint.save_checkpoint(p2, path)
    with pytest.warns(UserWarning, match="discriminator.extra"):
        srgan_util.SRGAN(4, path, device="cpu")
    # a missing key raises, naming it
    monkeypatch.undo()
    from minddiffusion_amd._lib import MdxError
    p3 = {k: v for k, v in p.items() if k != "trunk.7.bn2.moving_variance"}
    ms_checkpoint.save_checkpoint(p3, path)
    with pytest.raises(MdxError, match="trunk.7.bn2.moving_variance"):
        srgan_util.SRGAN(4, path, device="cpu")
    p4 = {k: v for k, v in p.items() if k != f"trunk.2.prelu.{spelling}"}
    ms_checkpoint.save_checkpoint(p4, path)
    with pytest.raises(MdxError, match="trunk.2.prelu"):
        srgan_util.SRGAN(4, path, device="cpu")


def _f64_hitting(target):
    """A float64 x with (x + 1) * 127.5 == target exactly in float64 (an exact .5 after scaling)."""
    x = np.float64(target / 127.5 - 1.0)
    for _ in range(256):
        v = (x + 1.0) * 127.5
        if v == target:
            return x
        x = np.nextafter(x, np.inf if v < target else -np.inf)
    raise AssertionError(target)


def test_get_img_hand_computed():
    from minddiffusion_amd.glide.model.srgan_util import get_img
    # (x + 1) * 127.5 -> rint -> clip [0, 255]:  -1 -> 0, 1 -> 255, 0 -> 127.5 -> 128, -1e-4 -> 127.487 -> 127, -1.2 -> clip 0,
    # 1.3 -> clip 255; the zero image of batch 1 -> 128
    below0 = np.float32(-1e-4)
    vals = [np.float32(-1.0), np.float32(1.0), np.float32(0.0), below0, np.float32(-1.2), np.float32(1.3)]
    x = np.zeros((2, 3, 1, 3), np.float32)               # [B, 3, H = 1, W = 3]
    x.reshape(-1)[:6] = vals
    got = get_img(x)
    assert got.dtype == np.uint8 and got.shape == (1, 6, 3)       # [H, B * W, 3]
    want = np.full((1, 6, 3), 128, np.uint8)
    want[0, 0:3, 0] = [0, 255, 128]                      # batch 0, channel 0 along W
    want[0, 0:3, 1] = [127, 0, 255]                      # batch 0, channel 1
    assert np.array_equal(got, want), got
    # rint at exact halves rounds to EVEN: 126.5 -> 126 and 124.5 -> 124 (round-half-up would give 127 / 125), 125.5 -> 126
    h = np.zeros((1, 3, 1, 3), np.float64)
    h[0, 0, 0, :] = [_f64_hitting(126.5), _f64_hitting(124.5), _f64_hitting(125.5)]
    got = get_img(h)
    assert list(got[0, :, 0]) == [126, 124, 126], got[0, :, 0]


def test_parameter_shapes_match_reference_structure():
    from minddiffusion_amd.glide.model.srgan import Generator
    for f, nsub in ((2, 1), (4, 2), (8, 3)):
        s = Generator(f, device="cpu").parameter_shapes()
        assert len(s) == 3 + TRUNK * (4 + 8 + 1) + 3 + 3 * nsub + 2
        assert s["conv1.0.weight"] == (64, 3, 9, 9) and s["conv3.weight"] == (3, 64, 9, 9)
        assert s[f"subpixel_conv.{nsub - 1}.conv.weight"] == (256, 64, 3, 3)
        assert f"subpixel_conv.{nsub}.conv.weight" not in s
        assert s["trunk.15.bn2.moving_variance"] == (64,) and s["conv2.1.a"] == (64,)
    from minddiffusion_amd._lib import MdxError
    with pytest.raises(MdxError):
        Generator(3, device="cpu")


def test_reference_pre_tanh_spread_is_meaningful():
    """The synthetic weights keep tanh out of saturation (the GPU tests assert the same at their shapes)."""
    p = torch_params(synthetic_params(2, seed=5))
    x = torch.tensor(np.random.RandomState(6).uniform(-1, 1, (1, 3, 16, 16)).astype(np.float32))
    sd = float(ref_generator(p, x, 2, pre_tanh=True).std())
    assert 0.2 <= sd <= 3.0, sd
