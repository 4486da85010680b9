"""LoRA without a GPU: adapter parameter names and shapes, key validation, the config of the reference's LoRA YAML, the adapter
checkpoint reader, and the identity the merge rests on."""
import numpy as np
import pytest
import torch

from _lora_util import make_adapter, merged_params


def _net(cfg, **kw):
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    return UNetModel(**dict(cfg, **kw), device="cpu")


@pytest.mark.parametrize("name", ["TINY_UNET", "SMALL_WUKONG_UNET"])
def test_lora_parameter_shapes(name):
    from minddiffusion_amd import configs
    cfg = getattr(configs, name)
    net = _net(cfg, enable_lora=True, lora_rank=4, lora_alpha=4)
    base, lora = net.parameter_shapes(), net.lora_parameter_shapes()
    assert base == _net(cfg).parameter_shapes(), "enable_lora must not change the base parameters"
    dense = [k[:-len(".weight")] for k in base
             if any(k.endswith(f".{a}.{n}.weight") for a in ("attn1", "attn2") for n in ("to_q", "to_k", "to_v", "to_out.0"))]
    # both configurations: 2 levels with attention, one block each on the way down, the middle block, 2 x 2 on the way up
    assert len(dense) == 7 * 8 and len(lora) == 2 * len(dense)
    for d in dense:
        out, inn = base[d + ".weight"]
        assert lora[d + ".tk_delta_lora_a"] == (4, inn) and lora[d + ".tk_delta_lora_b"] == (out, 4)
    other = net.lora_parameter_shapes("mindpet_delta_")
    assert sorted(other.values()) == sorted(lora.values()) and all(".mindpet_delta_lora_" in k for k in other)
    assert _net(cfg, enable_lora=True, lora_rank=8).lora_parameter_shapes()[dense[0] + ".tk_delta_lora_a"][0] == 8
    with pytest.raises(ValueError):
        net.lora_parameter_shapes("delta_")


def test_adapter_key_validation():
    from minddiffusion_amd.configs import TINY_UNET
    net = _net(TINY_UNET, enable_lora=True)
    tk = make_adapter(net.lora_parameter_shapes(), 0)
    mp = {k.replace("tk_delta_", "mindpet_delta_"): v for k, v in tk.items()}
    canon = net._check_lora(tk, True, "t")
    assert set(canon) == set(tk)
    got = net._check_lora(mp, True, "t")            # the other prefix lands on the same canonical names
    assert set(got) == set(tk) and all(got[k] is tk[k] for k in tk)
    k0, k1 = sorted(tk)[:2]
    mixed = dict(tk)
    mixed[k0.replace("tk_delta_", "mindpet_delta_")] = mixed.pop(k0)
    with pytest.raises(KeyError, match="mix"):
        net._check_lora(mixed, True, "t")
    with pytest.raises(KeyError, match=r"1 missing.*" + k1.replace(".", r"\.")):
        net._check_lora({k: v for k, v in tk.items() if k != k1}, True, "t")
    with pytest.raises(KeyError, match="1 missing"):     # missing keys raise without strict as well
        net._check_lora({k: v for k, v in tk.items() if k != k1}, False, "t")
    extra = dict(tk, **{"middle_block.1.proj_in.tk_delta_lora_a": np.zeros((4, 128), np.float32), "foo": np.zeros(1)})
    with pytest.raises(KeyError, match="2 unexpected"):
        net._check_lora(extra, True, "t")
    assert set(net._check_lora(extra, False, "t")) == set(tk)
    with pytest.raises(KeyError, match="1 missing.*1 unexpected"):
        net._check_lora({("x" + k if k == k1 else k): v for k, v in tk.items()}, True, "t")
    with pytest.raises(ValueError, match="shape"):
        net._check_lora(dict(tk, **{k0: tk[k0][:2]}), True, "t")


def test_lora_keys_need_enable_lora():
    """Without enable_lora the adapter keys are unexpected keys like any other, checked before anything is packed."""
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.weights import synthetic_unet_params_numpy
    plain = _net(TINY_UNET)
    assert not plain.enable_lora and not plain.lora_loaded
    params = synthetic_unet_params_numpy(plain.parameter_shapes())
    adapter = make_adapter(_net(TINY_UNET, enable_lora=True).lora_parameter_shapes(), 0)
    with pytest.raises(KeyError, match=f"{len(adapter)} unexpected"):
        plain.load_state_dict(dict(params, **adapter))
    for call in (lambda: plain.load_lora_state_dict(adapter), plain.unload_lora, lambda: plain.set_lora_scale(0.5)):
        with pytest.raises(MdxError, match="enable_lora"):
            call()
    with pytest.raises(MdxError, match="load_state_dict"):
        _net(TINY_UNET, enable_lora=True).load_lora_state_dict(adapter)
    with pytest.raises(ValueError):
        _net(TINY_UNET, enable_lora=True, lora_rank=0)


def test_one_dict_load_checks_base_and_adapter_keys_before_packing():
    """load_state_dict of an enable_lora model splits the dict: base keys and adapter keys are each checked (missing always,
    unexpected under strict, mixed prefixes) before anything is packed, so these raise without a GPU."""
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.weights import synthetic_unet_params_numpy
    net = _net(TINY_UNET, enable_lora=True)
    params = synthetic_unet_params_numpy(net.parameter_shapes())
    adapter = make_adapter(net.lora_parameter_shapes(), 0)
    k0 = sorted(adapter)[0]
    with pytest.raises(KeyError, match="1 missing"):
        net.load_state_dict(dict(params, **{k: v for k, v in adapter.items() if k != k0}))
    with pytest.raises(KeyError, match="1 missing"):
        net.load_state_dict(dict(params, **{k: v for k, v in adapter.items() if k != k0}), strict=False)
    with pytest.raises(KeyError, match="1 unexpected"):
        net.load_state_dict(dict(params, **adapter, **{"foo.tk_delta_lora_a": np.zeros((4, 4), np.float32)}))
    mixed = dict(adapter)
    mixed[k0.replace("tk_delta_", "mindpet_delta_")] = mixed.pop(k0)
    with pytest.raises(KeyError, match="mix"):
        net.load_state_dict(dict(params, **mixed))
    with pytest.raises(ValueError, match="shape"):
        net.load_state_dict(dict(params, **dict(adapter, **{k0: adapter[k0][:2]})))
    with pytest.raises(KeyError, match="1 missing"):        # a base key missing, adapter complete
        net.load_state_dict(dict({k: v for k, v in params.items() if k != "out.0.gamma"}, **adapter))
    assert net.w is None and not net.lora_loaded


def test_instantiate_from_the_lora_yaml_params():
    """unet_config of wukong-huahua/configs/v1-inference-chinese-lora.yaml (settings, typed in)."""
    from minddiffusion_amd import configs
    from minddiffusion_amd.ldm.util import instantiate_from_config
    params = dict(image_size=32, in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1],
                  num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True, transformer_depth=1,
                  context_dim=768, use_checkpoint=True, legacy=False, use_fp16=True, enable_lora=True, lora_rank=4, lora_alpha=4)
    assert params == configs.WUKONG_LORA_UNET
    net = instantiate_from_config({"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel", "params": dict(params, device="cpu")})
    assert net.enable_lora and net.lora_rank == 4 and net.lora_alpha == 4
    shapes = net.lora_parameter_shapes()
    assert len(shapes) == 16 * 8 * 2
    # 3.19 MB of fp32: the "3.1M" adapter checkpoint of the reference's README
    assert sum(int(np.prod(s)) for s in shapes.values()) * 4 == 3188736


def test_load_lora_checkpoint(tmp_path):
    from minddiffusion_amd import ms_checkpoint as C
    from minddiffusion_amd.configs import TINY_UNET
    adapter = make_adapter(_net(TINY_UNET, enable_lora=True).lora_parameter_shapes(), 5)
    blob = {C.UNET_PREFIX + k: v for k, v in adapter.items()}
    blob[C.UNET_PREFIX + "out.0.gamma"] = np.ones(64, np.float32)           # another trainable parameter of the UNet
    blob[C.TEXT_PREFIX + "x.tk_delta_lora_a"] = np.ones((4, 8), np.float32)  # a LoRA-named key outside the UNet
    C.save_checkpoint(blob, tmp_path / "lora.ckpt")
    got = C.load_lora_checkpoint(tmp_path / "lora.ckpt")
    assert set(got) == set(adapter) and all(np.array_equal(got[k], adapter[k]) for k in adapter)
    C.save_checkpoint({C.UNET_PREFIX + "out.0.gamma": np.ones(64, np.float32)}, tmp_path / "plain.ckpt")
    with pytest.raises(ValueError, match="no LoRA"):
        C.load_lora_checkpoint(tmp_path / "plain.ckpt")


def test_merged_form_equals_the_side_branch():
    """x W^T + s (x A^T) B^T == x (W + s B A)^T in float64 (the LoRADense forward, attention.py:118-126, vs the merge)."""
    g = torch.Generator().manual_seed(0)
    x, W = torch.randn(37, 96, generator=g, dtype=torch.float64), torch.randn(80, 96, generator=g, dtype=torch.float64) / 96 ** 0.5
    A, B = torch.randn(4, 96, generator=g, dtype=torch.float64) / 96 ** 0.5, 0.5 * torch.randn(80, 4, generator=g, dtype=torch.float64)
    s = 0.75
    side = x @ W.T + s * (x @ A.T) @ B.T
    merged = x @ (W + s * (B @ A)).T
    assert float((side - merged).abs().max()) <= 1e-12 * float(side.abs().max())
    # ... and the helper the GPU tests build their reference with is that merge
    p = merged_params({"d.weight": W.numpy().astype(np.float32)},
                      {"d.tk_delta_lora_a": A.numpy().astype(np.float32), "d.tk_delta_lora_b": B.numpy().astype(np.float32)}, s)
    assert np.allclose(p["d.weight"], (W + s * (B @ A)).numpy(), atol=1e-6)
    # the adapter is as large as the base matrix, so it shows in every output
    assert 0.5 < float((s * (B @ A)).norm() / W.norm()) < 2.0
