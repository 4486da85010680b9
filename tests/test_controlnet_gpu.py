"""ControlNet on the GPU against ControlOracle (tests/_control_util.py): the hint block and the residuals, one controlled UNet
evaluation with every form of the scale table, guess mode, zero zero-convs, graph replays, the hint cache, and the wrapper
outside its scope.  Tiny configurations on 8 x 8 and 8 x 12 latents, with hipGraph capture on and off.  Tolerances are the
project's single-call ones: rel-L2 <= 5e-3, max-abs <= 5e-2 (fp16 storage / fp32 accumulation against the fp32 oracle)."""
import functools

import numpy as np
import pytest
import torch

import _control_util as CU
from _util import check
from oracle import ldm as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = dict(rel_l2=5e-3, max_abs=5e-2)
CONFIGS = {"tiny": ("TINY_UNET", dict(num_heads=-1)), "small_wukong": ("SMALL_WUKONG_UNET", dict(num_head_channels=-1))}
CASES = [(n, g) for n in sorted(CONFIGS) for g in (True, False)]


@functools.lru_cache(maxsize=None)
def _setup(name, graph, zero=False):
    from minddiffusion_amd import configs
    from minddiffusion_amd.ldm.models.diffusion.controlled import ControlledDiffusion
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from minddiffusion_amd.ldm.modules.diffusionmodules.controlnet import ControlNet
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    cname, extra = CONFIGS[name]
    cfg = getattr(configs, cname)
    ocfg = dict(cfg, **extra)
    up, cp = O.init_params(ocfg, seed=0), CU.init_control_params(ocfg, seed=10, zero=zero)
    net, cn = UNetModel(**cfg), ControlNet(**cfg)
    net.use_graph = cn.use_graph = graph
    net.load_state_dict(up)
    cn.load_state_dict(cp)
    model = LatentDiffusion(net, linear_start=0.00085, linear_end=0.0120, timesteps=1000)
    return ocfg, model, cn, ControlledDiffusion(model, cn), CU.ControlOracle(ocfg, up, cp)


@functools.lru_cache(maxsize=None)
def _inputs(name, B=2, H=8, W=8):
    from minddiffusion_amd import configs
    return CU.inputs(getattr(configs, CONFIGS[name][0]), B, H, W)


def _dev(*arrays):
    return [torch.tensor(np.asarray(a, dtype=np.float32), device=DEV) for a in arrays]


@functools.lru_cache(maxsize=None)
def _ref(name, scale=1.0, zero=False):
    """Oracle eps of the B = 2 case (hashable scale: a float or a tuple)."""
    orc = _setup(name, True, zero)[4]
    x, t, c, hint = _inputs(name)
    return orc.controlled(x, t, c, hint, scale=list(scale) if isinstance(scale, tuple) else scale).numpy()


@pytest.mark.parametrize("shape", [(2, 8, 8), (1, 8, 12)])
@pytest.mark.parametrize("name,graph", CASES)
def test_hint_features_and_residuals_match_the_oracle(name, graph, shape):
    ocfg, _, cn, _, orc = _setup(name, graph)
    B, H, W = shape
    x, t, c, hint = _inputs(name, B, H, W)
    dx, dt, dc, dh = _dev(x, t, c, hint)
    mc = ocfg["model_channels"]
    g = cn.hint_features(dh)
    assert tuple(g.shape) == (B, H * W, mc)
    check(f"control.hint[{name},{graph},{shape}]", CU.nchw(g, mc, H, W), orc.hint_features(hint), **TOL)
    res = cn.forward_residuals(dx, dt, dc, dh)
    want = orc.residuals(x, t, c, hint)
    assert len(res) == len(want) == 5
    for i, (r, w) in enumerate(zip(res, want)):
        ch, h, wd = int(w.shape[1]), int(w.shape[2]), int(w.shape[3])      # a swapped H / W shows on the 8 x 12 latent
        assert tuple(r.shape) == (B, h * wd, ch)
        check(f"control.residual{i}[{name},{graph},{shape}]", CU.nchw(r, ch, h, wd), w, **TOL)


@pytest.mark.parametrize("scale", [1.0, (0.5, 1.5), (1.0, 0.5, 1.5, 0.75, 1.25)], ids=["one", "per_row", "per_residual"])
@pytest.mark.parametrize("name,graph", CASES)
def test_controlled_eps_matches_the_oracle(name, graph, scale):
    _, model, cn, cm, _ = _setup(name, graph)
    x, t, c, hint = _inputs(name)
    dx, dt, dc, dh = _dev(x, t, c, hint)
    with cm.control(dh, scale=list(scale) if isinstance(scale, tuple) else scale):
        out = cm.apply_model_nhwc(dx, dt, dc)
    assert cm.last_control_batch == 2
    check(f"control.eps[{name},{graph},{scale}]", CU.nchw(out, 4, 8, 8), _ref(name, scale), **TOL)
    # the same op list but the one add: the plain plan is what it is without ControlNet
    plain, ctl = model.unet._plan(2, 8, 8), model.unet._plan(2, 8, 8, control=True)
    assert len(ctl.main) == len(plain.main) + 1 and not hasattr(plain, "control")


@pytest.mark.parametrize("name,graph", CASES)
def test_guess_mode_leaves_the_unconditional_rows_alone(name, graph):
    _, model, cn, cm, orc = _setup(name, graph)
    x, t, c, hint = _inputs(name)
    uc = np.random.RandomState(9).randn(*c.shape).astype(np.float32)
    x2, t2, c2 = np.concatenate([x, x]), np.concatenate([t, t]), np.concatenate([uc, c])
    dx, dt, dc, dh = _dev(x2, t2, c2, hint)
    cn._plans.pop((4, 8, 8), None)
    with cm.control(dh, uncond=False):
        out = CU.nchw(cm.apply_model_nhwc(dx, dt, dc, cfg_dup=True), 4, 8, 8)
    assert cm.last_control_batch == 2 and (2, 8, 8) in cn._plans and (4, 8, 8) not in cn._plans
    check(f"control.guess.uncond[{name},{graph}]", out[:2], orc.unet_forward(x2, t2, c2).numpy()[:2], **TOL)
    check(f"control.guess.cond[{name},{graph}]", out[2:], _ref(name), **TOL)
    with cm.control(dh, uncond=True):
        both = CU.nchw(cm.apply_model_nhwc(dx, dt, dc, cfg_dup=True), 4, 8, 8)
    assert cm.last_control_batch == 4
    check(f"control.both[{name},{graph}]", both, orc.controlled(x2, t2, c2, hint, guided=True).numpy(), **TOL)
    with cm.control(dh, uncond=False):              # and back: fewer source rows than the map of the call before named
        again = CU.nchw(cm.apply_model_nhwc(dx, dt, dc), 4, 8, 8)
    assert np.array_equal(again, out)


def test_zero_initialised_zero_convs_give_the_plain_output():
    _, model, cn, cm, orc = _setup("tiny", True, zero=True)
    x, t, c, hint = _inputs("tiny")
    dx, dt, dc, dh = _dev(x, t, c, hint)
    with cm.control(dh):
        out = CU.nchw(cm.apply_model_nhwc(dx, dt, dc), 4, 8, 8)
    check("control.zero_init", out, orc.unet_forward(x, t, c).numpy(), **TOL)
    assert all(float(r.abs().max()) == 0.0 for r in cn._plan(2, 8, 8).residuals)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_replays_give_equal_bits_and_a_scale_change_keeps_the_graph(name):
    _, model, cn, cm, _ = _setup(name, True)
    x, t, c, hint = _inputs(name)
    dx, dt, dc, dh = _dev(x, t, c, hint)
    with cm.control(dh):
        a = cm.apply_model_nhwc(dx, dt, dc).clone()
        b = cm.apply_model_nhwc(dx, dt, dc).clone()
    assert torch.equal(a, b)
    P, PC = model.unet._plans[(2, 8, 8, "control")], cn._plans[(2, 8, 8)]
    graphs = (P.graph, PC.graph)
    assert all(g is not None for g in graphs)
    writes = P.control.table_writes
    with cm.control(dh, scale=(0.5, 1.5)):
        s = cm.apply_model_nhwc(dx, dt, dc).clone()
    assert (P.graph, PC.graph) == graphs and model.unet._plans[(2, 8, 8, "control")] is P
    assert P.control.table_writes == writes             # the ControlNet's buffers did not move: no pointer upload either
    assert not torch.equal(s, a)
    check(f"control.rescaled[{name}]", CU.nchw(s, 4, 8, 8), _ref(name, (0.5, 1.5)), **TOL)


def test_the_hint_block_runs_once_per_hint():
    _, model, cn, cm, orc = _setup("tiny", True)
    x, t, c, hint = _inputs("tiny")
    dx, dt, dc, dh = _dev(x, t, c, hint)
    dh = dh.clone()                                     # a tensor object of this test's own
    runs = cn.hint_runs
    r0 = [r.clone() for r in cn.forward_residuals(dx, dt, dc, dh)]
    assert cn.hint_runs == runs + 1
    cn.forward_residuals(dx, dt, dc, dh)
    with cm.control(dh):
        cm.apply_model_nhwc(dx, dt, dc)
        cm.apply_model_nhwc(dx, dt, dc)
    assert cn.hint_runs == runs + 1                     # the same tensor, unchanged: the hint block did not run again
    dh[:, :, :, 32:] = 1.0 - dh[:, :, :, 32:]           # an in-place edit bumps the version counter
    edited = hint.copy()
    edited[:, :, :, 32:] = 1.0 - edited[:, :, :, 32:]
    r1 = cn.forward_residuals(dx, dt, dc, dh)
    assert cn.hint_runs == runs + 2 and not torch.equal(r1[0], r0[0])
    for i, (r, w) in enumerate(zip(r1, orc.residuals(x, t, c, edited))):
        check(f"control.hint_edit.residual{i}", CU.nchw(r, int(w.shape[1]), int(w.shape[2]), int(w.shape[3])), w, **TOL)
    same_values = dh.clone()                            # another object with the same values is another hint
    cn.forward_residuals(dx, dt, dc, same_values)
    assert cn.hint_runs == runs + 3


@pytest.mark.parametrize("name,graph", CASES)
def test_outside_the_scope_the_wrapper_is_the_inner_model(name, graph):
    _, model, cn, cm, _ = _setup(name, graph)
    x, t, c, hint = _inputs(name)
    dx, dt, dc, dh = _dev(x, t, c, hint)
    ref = model.apply_model_nhwc(dx, dt, dc).clone()
    with cm.control(dh):
        ctl = cm.apply_model_nhwc(dx, dt, dc).clone()
    got = cm.apply_model_nhwc(dx, dt, dc)
    assert torch.equal(got, ref) and not torch.equal(ctl, ref)
    tt = torch.tensor([500.0, 37.0], device=DEV)
    assert torch.equal(cm.time_embedding_table(tt), model.time_embedding_table(tt))
    with cm.control(dh):
        tab = cm.time_embedding_table(tt)
        eu = model.unet._emb_total
        assert tab.shape[1] == eu + cn._emb_total
        assert torch.equal(tab[:, :eu], model.time_embedding_table(tt)) and torch.equal(tab[:, eu:], cn.time_embedding_table(tt))
        via_table = cm.apply_model_nhwc(dx, dt, dc, temb=tab).clone()
    # (the table is the same arithmetic as the per-call time embedding, batched: held to the single-call tolerance)
    check(f"control.temb_table[{name},{graph}]", CU.nchw(via_table, 4, 8, 8), CU.nchw(ctl, 4, 8, 8), **TOL)
    assert torch.equal(cm.apply_model(dx, dt, dc), model.apply_model(dx, dt, dc))
