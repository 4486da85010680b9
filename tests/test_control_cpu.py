"""ControlNet without a GPU: the host refusals of mdx_control_add_f16 through the C ABI, the declaration, the ControlNet's
parameter names and shapes, every wrapper / pipeline refusal, and the oracle side of the parity tests -- ControlOracle with zero
zero-convs IS the UNet oracle, and the distances that show a parity check can tell a dead hint path or a wrong residual order
from a right one."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _control_util as CU
from oracle import ldm as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the C ABI
def _desc(n_seg=2, nb=3, dst=(4096, 8192), epr=(64, 8), src=1 << 16, src_row=1 << 17, scale=1 << 18):
    from minddiffusion_amd import _lib
    d = _lib.ControlAddDesc()
    d.n_seg, d.nb = n_seg, nb
    for k, (p, e) in enumerate(zip(dst, epr)):
        d.dst[k], d.elems_per_row[k] = p, e
    d.src, d.src_row, d.scale = src, src_row, scale
    return d


def test_control_add_refuses_on_the_host_before_any_launch():
    from minddiffusion_amd import _lib
    lib = _lib.load()

    def refused(what, **kw):
        assert lib.mdx_control_add_f16(ctypes.byref(_desc(**kw)), None) == -1, kw
        msg = lib.mdx_last_error()
        assert msg.startswith(b"mdx_control_add_f16") and what in msg, (kw, msg)
    assert lib.mdx_control_add_f16(None, None) == -1 and b"null descriptor" in lib.mdx_last_error()
    refused(b"segments", n_seg=17)
    refused(b"segments", n_seg=0)
    refused(b"nb must be >= 1", nb=0)
    refused(b"nb must be >= 1", nb=-2)
    refused(b"not 16-byte aligned", dst=(4096, 8200))
    refused(b"null dst", dst=(4096, 0))
    refused(b"multiple of 8", epr=(64, 12))
    refused(b"multiple of 8", epr=(0, 8))
    refused(b"null src", src=0)
    refused(b"null src", src_row=0)
    refused(b"null src", scale=0)
    refused(b"misaligned", src=(1 << 16) + 4)
    refused(b"misaligned", src_row=(1 << 17) + 2)
    refused(b"misaligned", scale=(1 << 18) + 1)
    assert lib.mdx_silu_f16(None, 8, None) == -1 and b"mdx_silu_f16" in lib.mdx_last_error()
    assert lib.mdx_silu_f16(4096, 12, None) == -1 and lib.mdx_silu_f16(4104, 8, None) == -1


def test_the_entries_are_declared_as_the_header_declares_them():
    from minddiffusion_amd import _lib
    raw = open(os.path.join(ROOT, "include", "mdx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint mdx_control_add_f16\s*\(const mdx_control_add_desc\* d, mdx_stream_t s\)", header)
    assert re.search(r"\bint mdx_silu_f16\s*\(void\* x, size_t n, mdx_stream_t s\)", header)
    assert _lib.SIGNATURES["mdx_control_add_f16"][1] == [ctypes.POINTER(_lib.ControlAddDesc), _lib.c_void_p]
    assert _lib.SIGNATURES["mdx_silu_f16"][1] == [_lib.c_void_p, _lib.c_size_t, _lib.c_void_p]
    assert hasattr(_lib.load(), "mdx_control_add_f16") and hasattr(_lib.load(), "mdx_silu_f16")
    assert int(re.search(r"#define MDX_CONTROL_MAX_SEGS (\d+)", header).group(1)) == _lib.CONTROL_MAX_SEGS == 16
    # the ctypes struct follows the header's field order
    body = header[header.index("typedef struct mdx_control_add_desc {"):header.index("} mdx_control_add_desc;")]
    fields = re.findall(r"(\w+)(?:\[MDX_CONTROL_MAX_SEGS\])?;", body)
    assert fields == [f[0] for f in _lib.ControlAddDesc._fields_]


# ------------------------------------------------------------------------------------------------ the model class
def test_controlnet_parameter_shapes_for_the_sd2_unet():
    from minddiffusion_amd.configs import SD2_UNET
    from minddiffusion_amd.ldm.modules.diffusionmodules.controlnet import ControlNet
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    cn = ControlNet(hint_channels=3, device="cpu", **SD2_UNET)
    s = cn.parameter_shapes()
    assert s == CU.control_param_shapes(dict(O.SD2_UNET), 3)
    zero = sorted(k for k in s if k.startswith("zero_convs.") and k.endswith(".weight"))
    assert len(zero) == 12 and s["middle_block_out.0.conv.weight"] == (1280, 1280, 1, 1)
    widths = [s[f"zero_convs.{i}.0.conv.weight"][0] for i in range(12)]
    assert widths == [320, 320, 320, 320, 640, 640, 640, 1280, 1280, 1280, 1280, 1280]
    assert all(s[f"zero_convs.{i}.0.conv.weight"] == (w, w, 1, 1) and s[f"zero_convs.{i}.0.conv.bias"] == (w,)
               for i, w in enumerate(widths))
    hint = [s[f"input_hint_block.{2 * k}.conv.weight"] for k in range(8)]
    assert hint == [(16, 3, 3, 3), (16, 16, 3, 3), (32, 16, 3, 3), (32, 32, 3, 3), (96, 32, 3, 3), (96, 96, 3, 3),
                    (256, 96, 3, 3), (320, 256, 3, 3)]
    assert not any(k.startswith(("output_blocks.", "out.")) for k in s)
    # the encoder half carries the UNet's own names
    unet = UNetModel(device="cpu", **SD2_UNET).parameter_shapes()
    enc = {k: v for k, v in unet.items() if k.startswith(("input_blocks.", "middle_block.", "time_embed."))}
    assert enc and all(s[k] == v for k, v in enc.items())
    assert cn.output_blocks == [] and len(cn.input_blocks) == 12
    # the plain UNet's own names are what they were
    assert unet == O.unet_param_shapes(dict(O.SD2_UNET))


def test_controlnet_declines_lora_and_class_labels():
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.ldm.modules.diffusionmodules.controlnet import ControlNet
    with pytest.raises(MdxError, match="enable_lora"):
        ControlNet(device="cpu", **dict(TINY_UNET, enable_lora=True))
    with pytest.raises(MdxError, match="num_classes"):
        ControlNet(device="cpu", **dict(TINY_UNET, num_classes=10))
    with pytest.raises(MdxError, match="hint_channels"):
        ControlNet(hint_channels=9, device="cpu", **TINY_UNET)
    cn = ControlNet(device="cpu", **TINY_UNET)
    with pytest.raises(MdxError, match="forward_residuals"):
        cn.forward_nhwc(None, None)


def test_checkpoint_reader_strips_the_control_model_prefix(tmp_path):
    from minddiffusion_amd import ms_checkpoint as MS
    a, b = np.arange(6, dtype=np.float32).reshape(2, 3), np.ones(4, np.float32)
    path = str(tmp_path / "cn.ckpt")
    MS.save_checkpoint({"control_model.zero_convs.0.0.conv.bias": b, "control_model.input_hint_block.0.conv.weight": a,
                        "model.diffusion_model.out.2.conv.bias": b}, path)
    got = MS.load_controlnet_checkpoint(path)
    assert sorted(got) == ["input_hint_block.0.conv.weight", "zero_convs.0.0.conv.bias"]
    assert np.array_equal(got["input_hint_block.0.conv.weight"], a)
    MS.save_checkpoint({"zero_convs.0.0.conv.bias": b}, path)
    assert sorted(MS.load_controlnet_checkpoint(path)) == ["zero_convs.0.0.conv.bias"]


# ------------------------------------------------------------------------------------------------ wrapper / pipeline refusals
def _ldm(cfg=None, **kw):
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    net = UNetModel(device="cpu", **(cfg or TINY_UNET))
    return LatentDiffusion(net, linear_start=0.00085, linear_end=0.0120, timesteps=1000, **kw)


def _cn(cfg=None, **kw):
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.ldm.modules.diffusionmodules.controlnet import ControlNet
    return ControlNet(device="cpu", **dict(cfg or TINY_UNET, **kw))


def test_controlled_diffusion_refusals(monkeypatch):
    from minddiffusion_amd import distributed
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.ldm.models.diffusion.controlled import ControlledDiffusion
    from minddiffusion_amd.ldm.models.diffusion.session import SamplingSession
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    cm = ControlledDiffusion(_ldm(), _cn())
    assert cm.n_res == 5 and cm.is_controlled and cm.num_timesteps == 1000 and cm.unet is cm.inner.unet
    # a WindowedDiffusion inside or outside the wrapper, and a second wrapper
    with pytest.raises(MdxError, match="wrapper already"):
        ControlledDiffusion(WindowedDiffusion(_ldm(), window=(8, 8)), _cn())
    with pytest.raises(MdxError, match="not windowed"):
        WindowedDiffusion(cm, window=(8, 8))
    with pytest.raises(MdxError, match="wrapper already"):
        ControlledDiffusion(cm, _cn())
    # hybrid, concat and adm models
    for key in ("hybrid", "concat", "adm", None):
        with pytest.raises(MdxError, match="conditioning_key"):
            ControlledDiffusion(_ldm(conditioning_key=key), _cn())
    with pytest.raises(MdxError, match="conditioning_key"):
        ControlledDiffusion(_ldm(dict(TINY_UNET, num_classes=4)), _cn())
    # a ControlNet whose config differs from the UNet's in anything but hint_channels
    ControlledDiffusion(_ldm(), _cn(hint_channels=1))
    for kw, name in ((dict(model_channels=128), "model_channels"), (dict(context_dim=96), "context_dim"),
                     (dict(channel_mult=[1, 2, 4]), "channel_mult"), (dict(num_res_blocks=2), "num_res_blocks"),
                     (dict(in_channels=9), "in_channels"), (dict(use_linear_in_transformer=False), "use_linear")):
        with pytest.raises(MdxError, match=name):
            ControlledDiffusion(_ldm(), _cn(**kw))
    with pytest.raises(MdxError, match="must be a ControlNet"):
        ControlledDiffusion(_ldm(), _ldm().unet)
    # sessions
    with pytest.raises(MdxError, match="ControlledDiffusion"):
        SamplingSession(cm, 2, H=64, W=64, sampler="ddim")
    # the hint: its channel count, a size that is no multiple of 8, nesting, a non-finite scale
    with pytest.raises(MdxError, match="hint must be a tensor"):
        with cm.control(torch.zeros(1, 4, 64, 64)):
            pass
    with pytest.raises(MdxError, match="8 x a latent"):
        with cm.control(torch.zeros(1, 3, 60, 64)):
            pass
    with pytest.raises(MdxError, match="finite"):
        with cm.control(torch.zeros(1, 3, 64, 64), scale=float("nan")):
            pass
    with cm.control(torch.zeros(1, 3, 64, 64)):
        with pytest.raises(MdxError, match="already inside"):
            with cm.control(torch.zeros(1, 3, 64, 64)):
                pass
        # a hint whose size is not 8 x the latent of the call
        with pytest.raises(MdxError, match="8 x the latent"):
            cm._prepare(2, 16, 8, torch.device("cpu"))
        with pytest.raises(MdxError, match="does not fit"):
            cm._scope["hint"] = torch.zeros(3, 3, 64, 64)
            cm._prepare(4, 8, 8, torch.device("cpu"))
    assert cm._scope is None
    # several ranks
    monkeypatch.setattr(distributed, "world", lambda: (0, 2))
    with pytest.raises(MdxError, match="single rank"):
        ControlledDiffusion(_ldm(), _cn())


def test_row_maps_and_scale_tables_of_the_scope():
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.controlled import ControlledDiffusion
    cm = ControlledDiffusion(_ldm(), _cn())
    cpu = torch.device("cpu")
    hint = torch.rand(2, 3, 64, 64)
    with cm.control(hint, scale=[0.5, 1.5], uncond=True):
        e = cm._prepare(4, 8, 8, cpu)           # the guidance batch: the hint and the per-sample scales repeat over both halves
        assert e["rows"] == [0, 1, 2, 3] and e["nb_cn"] == 4 and tuple(e["hint"].shape) == (4, 3, 64, 64)
        assert torch.equal(e["hint"][:2], hint) and torch.equal(e["hint"][2:], hint)
        assert e["scale"].tolist() == [[0.5, 1.5, 0.5, 1.5]] * 5
        e = cm._prepare(2, 8, 8, cpu)           # no guidance: the caller's own tensor, so its in-place edits reach the ControlNet
        assert e["rows"] == [0, 1] and e["hint"] is hint
    with cm.control(hint, scale=[1, 2, 3, 4, 5], uncond=False):
        e = cm._prepare(4, 8, 8, cpu)           # guess mode: the unconditional rows are not touched, the ControlNet runs at b
        assert e["rows"] == [-1, -1, 0, 1] and e["nb_cn"] == 2 and e["half"] and e["hint"] is hint
        assert e["scale"][:, 0].tolist() == [1, 2, 3, 4, 5] and e["scale"].shape == (5, 4)
    with cm.control(hint[:1], uncond=False):
        assert cm._prepare(4, 8, 8, cpu)["rows"] == [-1, -1, 0, 1]          # a one-row hint: an even batch is the guidance batch
        assert cm._prepare(3, 8, 8, cpu)["rows"] == [0, 1, 2]
    with cm.control(hint[:1], uncond=True):
        assert cm._prepare(4, 8, 8, cpu)["rows"] == [0, 1, 2, 3]
    with cm.control(hint, scale=[1.0, 2.0, 3.0]):
        with pytest.raises(MdxError, match="scale has 3 entries"):
            cm._prepare(4, 8, 8, cpu)
    five = torch.rand(5, 3, 64, 64)
    with cm.control(five, scale=[1.0] * 5):
        with pytest.raises(MdxError, match="ambiguous"):
            cm._prepare(5, 8, 8, cpu)
    with cm.control(five, scale=np.ones((5, 5))):
        assert cm._prepare(5, 8, 8, cpu)["scale"].shape == (5, 5)


def test_pipeline_refusals(monkeypatch):
    from minddiffusion_amd import distributed
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.pipeline import DiffusionPipeline
    pipe = DiffusionPipeline(_ldm(), "ddim", device="cpu")
    c = torch.zeros(2, 6, 64)
    with pytest.raises(MdxError, match="needs a controlled pipeline"):
        pipe(c=c, uc=c, H=64, W=64, control_image=torch.zeros(2, 3, 64, 64))
    with pytest.raises(MdxError, match="needs a controlled pipeline"):
        pipe.img2img(init_latent=torch.zeros(2, 4, 8, 8), c=c, uc=c, control_image=torch.zeros(2, 3, 64, 64))
    cp = pipe.controlled(_cn())
    assert type(cp.sampler) is type(pipe.sampler) and cp.device == pipe.device and cp.model.inner is pipe.model
    assert DiffusionPipeline(_ldm(), "dpm_solver", device="cpu", solver=dict(order=3)).controlled(_cn())._solver() == {"order": 3}
    for call, name in ((lambda: cp.hires(c=c, uc=c), "hires"), (lambda: cp.session(), "session"),
                       (lambda: cp.serve([dict(c=c[0], uc=c[0])]), "serve"), (lambda: cp.windowed(), "windowed")):
        with pytest.raises(MdxError, match=f"{name}: not on a controlled pipeline"):
            call()
    with pytest.raises(MdxError, match="wrapper already"):
        pipe.windowed(window=64).controlled(_cn())
    with pytest.raises(MdxError, match="wrapper already"):
        cp.controlled(_cn())
    # a hint that is not at the image's size, or has the wrong batch
    cp._on_device = lambda c, uc, B: (c, uc)            # (no GPU here: the conditioning stays where it is)
    for bad in (torch.zeros(2, 3, 32, 64), torch.zeros(3, 3, 64, 64), torch.zeros(3, 64, 64)):
        with pytest.raises(MdxError, match="control_image is"):
            cp(c=c, uc=c, H=64, W=64, control_image=bad)
    monkeypatch.setattr(distributed, "world", lambda: (0, 2))
    with pytest.raises(MdxError, match="single rank"):
        cp(c=c, uc=c, H=64, W=64, control_image=torch.zeros(2, 3, 64, 64))


# ------------------------------------------------------------------------------------------------ the oracle side
CONFIGS = {"tiny": ("TINY_UNET", dict(num_heads=-1)), "small_wukong": ("SMALL_WUKONG_UNET", dict(num_head_channels=-1))}


def _oracle(name, seed, zero=False):
    from minddiffusion_amd import configs
    cname, extra = CONFIGS[name]
    cfg = dict(getattr(configs, cname), **extra)
    return cfg, CU.ControlOracle(cfg, O.init_params(cfg, seed=seed), CU.init_control_params(cfg, seed=seed + 10, zero=zero))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_zero_zero_convs_give_the_unet_oracle_exactly(name):
    cfg, orc = _oracle(name, 0, zero=True)
    x, t, c, hint = CU.inputs(cfg)
    ref = O.UNetOracle(cfg, O.init_params(cfg, seed=0))(x, t, c)
    assert torch.equal(orc.controlled(x, t, c, hint), ref)
    assert torch.equal(orc.unet_forward(x, t, c), ref)
    assert all(float(r.abs().max()) == 0.0 for r in orc.residuals(x, t, c, hint))


@pytest.mark.parametrize("seed", (0, 1))
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_parity_checks_can_tell_wrong_from_right(name, seed):
    """Oracle-side distances, each at least ten times the single-call tolerance (5e-3): control against none, two same-shaped
    residuals swapped, half the hint inverted.  A parity check at 5e-3 therefore fails on a dropped residual, a wrong order or
    a dead hint path.  (With HINT_GAIN = 1 the inverted hint moves eps by only ~4e-3.)"""
    cfg, orc = _oracle(name, seed)
    x, t, c, hint = CU.inputs(cfg)
    plain = orc.unet_forward(x, t, c).numpy()
    ctl = orc.controlled(x, t, c, hint).numpy()
    res = orc.residuals(x, t, c, hint)
    assert len(res) == orc.n_res == 5 and res[0].shape == res[1].shape       # input blocks 0 and 1 share a shape
    perm = [1, 0, 2, 3, 4]
    swapped = orc.controlled(x, t, c, hint, permute=perm).numpy()
    inv = hint.copy()
    inv[:, :, :, 32:] = 1.0 - inv[:, :, :, 32:]
    inverted = orc.controlled(x, t, c, inv).numpy()
    d = {"control_vs_plain": CU.rel_l2(ctl, plain), "swapped": CU.rel_l2(swapped, ctl), "hint_inverted": CU.rel_l2(inverted, ctl)}
    print("DISCRIMINATION", name, seed, d)
    assert all(v >= 0.05 for v in d.values()), d


def test_oracle_row_map_and_scales():
    cfg, orc = _oracle("tiny", 0)
    x, t, c, hint = CU.inputs(cfg)
    x2, t2, c2 = np.concatenate([x, x]), np.concatenate([t, t]), np.concatenate([c[::-1], c])
    guess = orc.controlled(x2, t2, c2, hint, uncond=False, guided=True)
    plain = orc.unet_forward(x2, t2, c2)
    both = orc.controlled(x2, t2, c2, hint, uncond=True, guided=True)
    assert torch.equal(guess[:2], plain[:2])                        # unconditional rows: no control at all
    # conditional rows: the controlled call on b rows (another batch size: the CPU library's sums differ in the last bits)
    close = lambda a, b: torch.allclose(a, b, rtol=0, atol=1e-5)
    assert close(guess[2:], orc.controlled(x, t, c, hint))
    assert close(both[2:], guess[2:]) and CU.rel_l2(both[:2].numpy(), plain[:2].numpy()) > 0.05
    half = orc.controlled(x, t, c, hint, scale=0.0)
    assert torch.equal(half, orc.unet_forward(x, t, c))
    per_row = orc.controlled(x, t, c, hint, scale=[0.0, 1.0])
    assert torch.equal(per_row[0], half[0]) and torch.equal(per_row[1], orc.controlled(x, t, c, hint)[1])
