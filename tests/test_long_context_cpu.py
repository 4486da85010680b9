"""Long prompts on the host: cutting token ids into 77-token windows, bringing c and uc to one length, and what the UNet planner
emits for a context capacity above the default (plans are built on host tensors, nothing is launched: tests/test_host_cpu.py)."""
import numpy as np
import pytest
import torch

from minddiffusion_amd._lib import MdxError
from minddiffusion_amd.ldm.modules.encoders import chunk_token_ids, pad_conditioning

BOS, EOS = 98, 99


def window(body, pad=EOS):
    return [BOS] + list(body) + [EOS] + [pad] * (75 - len(body))


def test_chunk_token_ids_boundaries():
    ids = lambda n: list(range(1, n + 1))
    out = chunk_token_ids([[]], BOS, EOS)
    assert out.shape == (1, 1, 77) and out.dtype == np.int32 and out[0, 0].tolist() == window([])
    out = chunk_token_ids([ids(75)], BOS, EOS)                      # exactly one full window: bos, 75 ids, eos, no padding
    assert out.shape == (1, 1, 77) and out[0, 0].tolist() == [BOS] + ids(75) + [EOS]
    out = chunk_token_ids([ids(76)], BOS, EOS)                      # one id spills into a second window
    assert out.shape == (1, 2, 77) and out[0, 0].tolist() == window(ids(75)) and out[0, 1].tolist() == window([76])
    out = chunk_token_ids([ids(151)], BOS, EOS)
    assert out.shape == (1, 3, 77) and out[0, 2].tolist() == window([151]) and out[0, 1].tolist() == window(ids(150)[75:])


def test_chunk_token_ids_ragged_batch_and_padding():
    a, b, c = list(range(1, 81)), [5, 6, 7], []
    out = chunk_token_ids([a, np.array(b), c], BOS, EOS, pad=0)
    assert out.shape == (3, 2, 77)                                  # n is the batch maximum; shorter prompts get whole empty windows
    assert out[0, 0].tolist() == window(a[:75], 0) and out[0, 1].tolist() == window(a[75:], 0)
    assert out[1, 0].tolist() == window(b, 0) and out[1, 1].tolist() == window([], 0)
    assert out[2, 0].tolist() == window([], 0) and out[2, 1].tolist() == window([], 0)
    same = chunk_token_ids([a, b, c], BOS, EOS)                     # pad=None pads with eos
    assert same[1, 0].tolist() == window(b, EOS) and same[1, 0, 5:].tolist() == [EOS] * 72
    assert chunk_token_ids([a], BOS, EOS, body=40).shape == (1, 2, 42)
    with pytest.raises(MdxError):
        chunk_token_ids([], BOS, EOS)


def test_pad_conditioning():
    rng = np.random.RandomState(0)
    t = lambda *s: torch.tensor(rng.randn(*s).astype(np.float32))
    empty = t(1, 77, 8)
    c, uc = t(2, 231, 8), t(2, 77, 8)
    c2, uc2 = pad_conditioning(c, uc, empty)
    assert c2 is c and tuple(uc2.shape) == (2, 231, 8)
    assert torch.equal(uc2[:, :77], uc) and torch.equal(uc2[:, 77:154], empty.expand(2, 77, 8)) and torch.equal(uc2[:, 154:], empty.expand(2, 77, 8))
    c3, uc3 = pad_conditioning(uc, c, empty)                         # the other side shorter; a batch-1 uc stays batch 1
    assert uc3 is c and torch.equal(c3, uc2)
    one = pad_conditioning(c, t(1, 154, 8), empty)[1]
    assert tuple(one.shape) == (1, 231, 8) and torch.equal(one[:, 154:], empty)
    same = pad_conditioning(c, c2, None)                              # equal lengths: the identity, `empty` is not looked at
    assert same[0] is c and same[1] is c2
    with pytest.raises(MdxError, match="77"):
        pad_conditioning(t(2, 100, 8), uc, empty)
    with pytest.raises(MdxError, match="77"):
        pad_conditioning(c, t(2, 100, 8), empty)
    with pytest.raises(MdxError, match="empty"):
        pad_conditioning(c, uc, t(1, 76, 8))


def _host_net(cfg, **kw):
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from minddiffusion_amd.weights import synthetic_unet_params_numpy
    net = UNetModel(device="cpu", **cfg, **kw)
    net.load_state_dict(synthetic_unet_params_numpy(net.parameter_shapes(), 0))
    return net


def test_planner_keeps_both_fused_paths_at_capacity_160():
    import ctypes
    from minddiffusion_amd import _lib
    from minddiffusion_amd.configs import SMALL_WUKONG_UNET, TINY_UNET
    lib = _lib.load()
    net = _host_net(TINY_UNET, max_context_len=160)
    P = net._plan(2, 8, 8)
    assert sum("+cross-attention" in m["info"] for m in P.meta) == len(P.xattn_descs) > 0
    assert all(d.xattn_cap == 160 for d in P.xattn_descs)
    for d in P.descs:
        assert lib.mdx_gemm_check(ctypes.byref(d)) == 0, lib.mdx_last_error()
    for d in P.xattn_descs:                                           # the length a 154-token context sets passes the C-side check
        d.xattn_len = 154
        assert lib.mdx_gemm_check(ctypes.byref(d)) == 0, lib.mdx_last_error()
    wk = _host_net(SMALL_WUKONG_UNET, max_context_len=160)
    Pw = wk._plan(2, 64, 64)
    assert Pw.tails and all(t.ctx_cap == 160 for t in Pw.tails)
    assert any(m["info"].startswith("st_tail") for m in Pw.meta)


def test_default_capacity_plans_what_it_planned():
    """A net built with max_context_len=80 is the default-built net: same op list metadata (launch kinds, shapes, tiles, flops)."""
    from minddiffusion_amd.configs import SMALL_WUKONG_UNET, TINY_UNET
    for cfg, shape in ((TINY_UNET, (2, 8, 8)), (SMALL_WUKONG_UNET, (2, 64, 64))):
        a, b = _host_net(cfg), _host_net(cfg, max_context_len=80)
        assert a.max_context_len == b.max_context_len == 80
        Pa, Pb = a._plan(*shape), b._plan(*shape)
        assert [m["info"] for m in Pa.meta] == [m["info"] for m in Pb.meta]
        assert [(m["kind"], m["flops"], m["launches"]) for m in Pa.meta] == [(m["kind"], m["flops"], m["launches"]) for m in Pb.meta]


def test_set_max_context_len_drops_plans_only_when_the_value_changes():
    from minddiffusion_amd.configs import TINY_UNET
    net = _host_net(TINY_UNET)
    P = net._plan(2, 8, 8)
    assert net.set_max_context_len(77) is net and net.max_context_len == 80      # rounds up to a multiple of 8: unchanged
    assert net._plan(2, 8, 8) is P
    net.set_max_context_len(154)
    assert net.max_context_len == 160 and not net._plans and net._ctx_key is None
    P2 = net._plan(2, 8, 8)
    assert P2 is not P and tuple(P2.ctx_pad.shape)[1] == 160
    net.set_max_context_len(160)
    assert net._plan(2, 8, 8) is P2
    for bad in (0, 1025):
        with pytest.raises(MdxError, match="max_context_len"):
            net.set_max_context_len(bad)
    with pytest.raises(MdxError, match="max_context_len"):
        _host_net(TINY_UNET, max_context_len=2000)
