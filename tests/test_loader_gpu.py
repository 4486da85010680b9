"""The shared weight loader on the device: a load with device="cuda" packs the same bits as the device="cpu" load of the same
parameters.  The loader decides the order of "move to the device" and "convert the dtype" for every class in one place; this
is the guard on that order."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import weights_fingerprint as WF  # noqa: E402

pytestmark = pytest.mark.gpu


def _same_bits(host, dev):
    assert list(host) == list(dev)
    for k in host:
        assert dev[k].is_cuda and dev[k].dtype == host[k].dtype and dev[k].shape == host[k].shape, k
        assert torch.equal(dev[k].cpu().view(torch.uint8), host[k].view(torch.uint8)), k


def test_unet320_device_load_equals_host_load():
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    case = WF.build_case("unet320")
    case.load()
    dev = UNetModel(device="cuda:0", **WF.UNET320).load_state_dict(case.params)
    assert any(k.endswith("head.stream") for k in dev.w) and any(k.endswith("qkv.cb") for k in dev.w)
    _same_bits(case.model.w, dev.w)
    assert dev._emb_off == case.model._emb_off and dev._emb_total == case.model._emb_total


def test_tiny_glide_device_load_equals_host_load():
    from test_host_cpu import TINY_GLIDE
    from minddiffusion_amd.glide.diffusion_creator import create_model
    case = WF.build_case("tiny_glide base")
    case.load()
    dev = create_model(device="cuda:0", **TINY_GLIDE).load_state_dict(case.params)
    _same_bits(case.model.w, dev.w)
