"""ff2 + proj_out of the last transformer block as ONE K-segmented dense launch (ops option unet_ff_proj_fuse, Planner.transformer;
ops.compose_ff_proj, csrc/dense.hip SEG).

The default gate (inner >= 640, M >= 128) leaves the tiny test models on their two launches, so the option is forced to 64 here: the
64-channel level of TINY_UNET then fuses wherever it has at least 128 token rows.  The bar is the oracle's, the one
test_tiny_unet_forward uses (rel-L2 5e-3, max |d| 5e-2); the fused-vs-unfused distance is printed as a PARITY line (docs/PARITY.md).
"""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

from _util import check, metrics
from oracle import ldm as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
DEV = "cuda:0"
gpu = pytest.mark.gpu

CFG320 = dict(image_size=32, in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[1, 2],
              num_res_blocks=1, channel_mult=[1, 2], num_head_channels=64, use_spatial_transformer=True,
              use_linear_in_transformer=True, transformer_depth=1, context_dim=1024, legacy=False)


@contextlib.contextmanager
def option(value):
    from minddiffusion_amd import ops
    keep = ops.get_option("unet_ff_proj_fuse")
    ops.set_option("unet_ff_proj_fuse", value)
    try:
        yield
    finally:
        ops.set_option("unet_ff_proj_fuse", keep)


def _cfg(**kw):
    from minddiffusion_amd.configs import TINY_UNET
    return dict(TINY_UNET, **kw)


def _ocfg(cfg):
    c = dict(cfg)
    c.setdefault("num_heads", -1)
    c.setdefault("num_head_channels", -1)
    return c


def _build(cfg, params, graph):
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    net = UNetModel(**cfg)
    net.use_graph = graph
    return net.load_state_dict(params)


def _fused_ops(P):
    return [m["info"] for m in P.meta if "ff2 + proj_out fused" in m["info"]]


@gpu
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("graph", [False, True])
def test_tiny_unet_with_the_fused_launch_against_the_oracle(graph, depth):
    """(2, 8, 8): 128 rows at the 64-channel level -- one 128-row tile or two 64-row ones; (1, 16, 16): 256 rows; (3, 8, 12): 288 rows,
    ragged against both tiles.  depth 2: only the last block's ff2 is folded into proj_out."""
    cfg = _cfg(transformer_depth=depth)
    params = O.init_params(_ocfg(cfg), seed=0)
    oracle = O.UNetOracle(_ocfg(cfg), params)
    with option(0):
        plain = _build(cfg, params, graph)
        outs0 = {}
        for (B, H, W, T, t) in ((2, 8, 8, 5, 981.0), (1, 16, 16, 77, 21.0), (3, 8, 12, 9, 500.0)):
            rng = np.random.RandomState(B + H)
            x, ctx = rng.randn(B, 4, H, W).astype(np.float32), rng.randn(B, T, cfg["context_dim"]).astype(np.float32)
            outs0[(B, H, W)] = (x, ctx, t, plain(torch.tensor(x, device=DEV), torch.full((B,), t, device=DEV), torch.tensor(ctx, device=DEV)).clone())
            assert not _fused_ops(plain._plan(B, H, W))
    with option(64):
        net = _build(cfg, params, graph)
        for (B, H, W), (x, ctx, t, out0) in outs0.items():
            got = net(torch.tensor(x, device=DEV), torch.full((B,), t, device=DEV), torch.tensor(ctx, device=DEV))
            P = net._plan(B, H, W)
            # the three SpatialTransformers of the 64-channel level (one on the way down, two on the way up) fuse; the 128-channel
            # level has fewer than 128 rows
            assert len(_fused_ops(P)) == 3, _fused_ops(P)
            assert len(P.descs) == len(plain._plan(B, H, W).descs) - 3
            if graph:
                assert P.graph is not None and not P.graph_failed
            ref = oracle(x, torch.full((B,), t), ctx)
            check(f"ff_proj_fuse_tiny_depth{depth}_graph{int(graph)}_B{B}_{H}x{W}", got, ref, rel_l2=5e-3, max_abs=5e-2)
            m = metrics(got, out0)
            print("PARITY", {"name": f"ff_proj_fuse_tiny_depth{depth}_graph{int(graph)}_B{B}_{H}x{W}_fused_vs_unfused", **m})
            got2 = net(torch.tensor(x, device=DEV), torch.full((B,), t, device=DEV), torch.tensor(ctx, device=DEV))
            assert torch.equal(got, got2)


@gpu
def test_zero_init_unet_with_the_fused_launch_is_exactly_zero():
    """The reference zero-inits proj_out (zero_module): W_p = 0 and b_p = 0 give Wc = 0 and bc = 0, the fused launch returns x."""
    cfg = _cfg()
    params = O.init_params(_ocfg(cfg), seed=1, zero_init=True)
    with option(64):
        net = _build(cfg, params, False)
        rng = np.random.RandomState(0)
        x, ctx = rng.randn(2, 4, 8, 8).astype(np.float32), rng.randn(2, 5, cfg["context_dim"]).astype(np.float32)
        got = net(torch.tensor(x, device=DEV), torch.full((2,), 981.0, device=DEV), torch.tensor(ctx, device=DEV))
        assert _fused_ops(net._plan(2, 8, 8))
        assert float(got.abs().max()) == 0.0


@gpu
def test_sd2_batch2_plan_has_eleven_descriptors_fewer_and_replays_as_a_graph():
    from minddiffusion_amd import ops
    from minddiffusion_amd.configs import SD2_UNET
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from minddiffusion_amd.weights import synthetic_unet_params_device
    net = UNetModel(**dict(SD2_UNET))
    net.load_state_dict(synthetic_unet_params_device(net.parameter_shapes(), seed=0, device=DEV))
    with option(0):
        n0 = len(net._plan(2, 64, 64).descs)
        net._plans.clear()
    assert ops.get_option("unet_ff_proj_fuse") == 640      # the shipped default
    P = net._plan(2, 64, 64)
    assert len(P.descs) == n0 - 11 and len(_fused_ops(P)) == 11, (n0, len(P.descs), _fused_ops(P))
    lean = 0
    for m in P.meta:
        if "ff2 + proj_out fused" in m["info"]:
            q = ops.gemm_query(m["desc"])
            # unsplit or reduced in the kernel: the lean dense kernel (a deeper split goes to slabs on the generic one)
            assert (q[3] == 2) == (q[2] == 1 or q[6] == 1), (m["info"], q)
            lean += q[3] == 2
    assert lean >= 10, lean      # every fused launch of the M = 2048 and M = 512 levels
    rng = np.random.RandomState(3)
    x = torch.tensor(rng.randn(2, 4, 64, 64).astype(np.float32), device=DEV)
    ctx = torch.tensor(rng.randn(2, 77, 1024).astype(np.float32), device=DEV)
    t = torch.full((2,), 500.0, device=DEV)
    net.use_graph = False
    eager = net(x, t, ctx).clone()
    net.use_graph = True
    got = net(x, t, ctx).clone()
    assert P.graph is not None and not P.graph_failed
    again = net(x, t, ctx)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, eager) and torch.equal(got, again)


def test_with_the_option_at_zero_the_planner_emits_the_parent_descriptor_sequence():
    """Host only (device="cpu", nothing is launched).  tests/golden/ff_proj_parent_unet320_descs.txt is tools/plan_fingerprint.py's
    gemm_desc_sequence of the 320-channel build at (2, 16, 16) on the commit before the option existed: its 640-channel level has
    128 rows and crosses the default gate."""
    from plan_fingerprint import _unet, gemm_desc_sequence
    parent = open(os.path.join(ROOT, "tests", "golden", "ff_proj_parent_unet320_descs.txt")).read().splitlines()
    with option(0):
        assert gemm_desc_sequence(_unet(CFG320)._plan(2, 16, 16).descs) == parent
    with option(640):
        P = _unet(CFG320)._plan(2, 16, 16)
        assert len(P.descs) == len(parent) - 4 and len(_fused_ops(P)) == 4
        fused = [m["desc"] for m in P.meta if "ff2 + proj_out fused" in m["info"]]
        assert all(d.c1 == 2560 and d.c2 == 640 and d.N == 640 and d.a2 and d.residual and d.bias for d in fused)
