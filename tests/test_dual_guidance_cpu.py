"""Three-branch guidance (InstructPix2Pix) on the host, without a GPU: the batch GuidedModel lays out, which step entry the
dispatch picks, every refusal of the samplers and of pipe.edit, and the 8-channel loader."""
import types

import numpy as np
import pytest
import torch

UPDATE = (0.5, 0.6, 0.7, 0.8, 0.0, None, None, "x_prev", "pred_x0")


# ------------------------------------------------------------------------------------------------ the model call
def _model():
    table = []
    seen = []
    m = types.SimpleNamespace(unet=types.SimpleNamespace(num_classes=None), table=table, seen=seen,
                              time_embedding_table=lambda t: table.append(t.clone()) or torch.zeros(t.shape[0], 3))

    def apply_model_nhwc(x, t, c, temb=None):
        seen.append((x.clone(), t.clone(), c))
        return torch.arange(x.shape[0], dtype=torch.float32).reshape(-1, 1, 1).expand(-1, 64, 8).contiguous()
    m.apply_model_nhwc = apply_model_nhwc
    return m


def _guided(model, b=2, image_scale=1.5, t_steps=(801., 601., 401.), **over):
    from minddiffusion_amd.ldm.models.diffusion.guided import GuidedModel
    kw = dict(cond=torch.ones(b, 5, 6), uc=torch.zeros(b, 5, 6), c_cat=torch.full((b, 4, 8, 8), 2.0),
              uc_cat=torch.full((b, 4, 8, 8), 3.0))
    kw.update(over)
    return GuidedModel(model, b, (4, 8, 8), kw["cond"], kw["uc"], kw["c_cat"], kw["uc_cat"], 7.5, "cpu", list(t_steps),
                       image_scale=image_scale)


def test_guided_model_lays_out_three_branches_once():
    m = _model()
    g = _guided(m)
    assert g.dual and g.use_cfg and not g.same_halves and g.nb == 6 and g.out_m is None
    # x_in [3B, cx + ccat, h, w], the c_concat channels [uc_cat ; c_cat ; c_cat]
    assert tuple(g.x_in.shape) == (6, 8, 8, 8)
    want = torch.cat([torch.full((2, 4, 8, 8), 3.0), torch.full((4, 4, 8, 8), 2.0)])
    assert torch.equal(g.x_in[:, 4:], want)
    # the context [uc ; uc ; c], the timestep rows three times, one table for the run
    assert torch.equal(g.c_in, torch.cat([torch.zeros(4, 5, 6), torch.ones(2, 5, 6)]))
    assert tuple(g.t_all.shape) == (3, 6) and torch.equal(g.t_all[1], torch.full((6,), 601.))
    assert len(m.table) == 1 and m.table[0].tolist() == [801., 601., 401.]
    # a call: the latent into all three thirds, the c_concat channels untouched, (out_u, out_c) back and out_m exposed
    x = torch.randn(2, 4, 8, 8)
    out_u, out_c = g(x, 1)
    xin, t, c = m.seen[0]
    assert all(torch.equal(xin[k:k + 2, :4], x) for k in (0, 2, 4)) and torch.equal(xin[:, 4:], want)
    assert torch.equal(t, torch.full((6,), 601.)) and c is g.c_in
    assert out_u[:, 0, 0].tolist() == [0., 1.] and g.out_m[:, 0, 0].tolist() == [2., 3.] and out_c[:, 0, 0].tolist() == [4., 5.]
    # three branches whatever the scales are
    from minddiffusion_amd.ldm.models.diffusion.guided import GuidedModel
    g1 = GuidedModel(_model(), 2, (4, 8, 8), torch.ones(2, 5, 6), torch.zeros(2, 5, 6), torch.ones(2, 4, 8, 8),
                     torch.zeros(2, 4, 8, 8), 1.0, "cpu", [1.], image_scale=1.0)
    assert g1.nb == 6


def test_guided_model_without_image_scale_is_what_it_was():
    from minddiffusion_amd.ldm.models.diffusion.guided import GuidedModel
    a = GuidedModel(_model(), 2, (4, 8, 8), torch.ones(2, 5, 6), torch.zeros(2, 5, 6), torch.ones(2, 4, 8, 8),
                    torch.zeros(2, 4, 8, 8), 7.5, "cpu", [801., 601.])
    b = _guided(_model(), image_scale=None, c_cat=torch.ones(2, 4, 8, 8), uc_cat=torch.zeros(2, 4, 8, 8), t_steps=(801., 601.))
    assert not a.dual and a.out_m is None and a.nb == b.nb == 4
    for k in ("x_in", "c_in", "t_all"):
        assert torch.equal(getattr(a, k)[..., 4:, :, :] if k == "x_in" else getattr(a, k),
                           getattr(b, k)[..., 4:, :, :] if k == "x_in" else getattr(b, k)), k
    assert a.same_halves == b.same_halves and a.use_cfg == b.use_cfg


def test_guided_model_refusals():
    from minddiffusion_amd._lib import MdxError
    for over, name in ((dict(c_cat=None), "a c_concat"), (dict(uc_cat=None), "an unconditional c_concat"),
                       (dict(uc=None), "an unconditional c_crossattn")):
        with pytest.raises(MdxError, match=f"image guidance .* needs .*{name}"):
            _guided(_model(), **over)
    with pytest.raises(MdxError, match="per-request timesteps"):
        _guided(_model(), t_steps=np.zeros((3, 2), np.float32))
    with pytest.raises(MdxError, match="unconditional c_concat .* is not the c_concat's"):
        _guided(_model(), uc_cat=torch.zeros(2, 5, 8, 8))


# ------------------------------------------------------------------------------------------------ the step dispatch
def test_sampler_update_routes_to_the_dual_entry_only_with_out_m(monkeypatch):
    from minddiffusion_amd import ops
    calls = []
    for name in ("sampler_step", "sampler_step_pred", "sampler_step_rescale", "sampler_step_dual"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append((_n, a, k)))
    u = c = m = torch.zeros(2, 4, 4, 8)
    olds, coef = ["e1"], (1.5, -0.5, 0., 0.)
    ops.sampler_update("x", u, c, 7.5, ops.PRED_EPS, olds, coef, UPDATE)
    ops.sampler_update("x", u, c, 7.5, ops.PRED_EPS, olds, coef, UPDATE, out_m=None, mid_scale=None)
    assert [n for n, _, _ in calls] == ["sampler_step", "sampler_step"] and calls[0] == calls[1]
    del calls[:]
    ops.sampler_update("x", u, c, 7.5, ops.PRED_EPS, olds, coef, UPDATE, 0., "xm", 0.9, 0.1, out_m=m, mid_scale=1.5)
    ops.sampler_update("x", u, c, 7.5, ops.PRED_V, olds, coef, UPDATE, 0.7, "xm", 0.9, 0.1, out_m=m, mid_scale=1.5)
    assert calls == [("sampler_step_dual", ("x", "xm", u, m, c, 8, 7.5, 1.5, ops.PRED_EPS, 1., 0., olds, coef) + UPDATE,
                      {"guidance_rescale": 0.}),
                     ("sampler_step_dual", ("x", "xm", u, m, c, 8, 7.5, 1.5, ops.PRED_V, 0.9, 0.1, olds, coef) + UPDATE,
                      {"guidance_rescale": 0.7})]


def test_scalar_steps_hand_the_middle_output_on(monkeypatch):
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.schedule import ScalarSteps, Step
    seen = []
    monkeypatch.setattr(ops, "sampler_update", lambda *a, **k: seen.append((a, k)))
    plan = [Step(801., (0.9, 0.1), (1., 0., 0., 0.), (0.5, 0.6, 0.7, 0.8, 0.))]
    ScalarSteps(plan, 7.5, 0.).launch(0, "x", "u", "c", 0, [], None, None, "xp", "p0")
    assert seen[-1][1] == {}                                    # today's call, keyword for keyword
    ScalarSteps(plan, 7.5, 0., 1.5).launch(0, "x", "u", "c", 0, [], None, None, "xp", "p0", out_m="m")
    assert seen[-1][1] == {"out_m": "m", "mid_scale": 1.5} and seen[-1][0] == seen[0][0]
    with pytest.raises(MdxError, match="without an image_scale"):
        ScalarSteps(plan, 7.5, 0.).launch(0, "x", "u", "c", 0, [], None, None, "xp", "p0", out_m="m")


def test_the_entries_are_declared():
    from minddiffusion_amd import _lib
    for name, extra in (("mdx_sampler_step_dual_f32", "mdx_sampler_step_rescale_f32"),
                        ("mdx_sampler_step_lin_dual_f32", "mdx_sampler_step_lin_noise_f32")):
        two = _lib.SIGNATURES[extra][1]
        assert _lib.SIGNATURES[name] == (_lib.c_int, two[:-5] + [_lib.c_void_p, _lib.c_float] + two[-5:])


# ------------------------------------------------------------------------------------------------ sampler refusals
def _ldm(in_channels=8, cls="edit", **kw):
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.ldm.models.diffusion import ddpm
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    net = UNetModel(device="cpu", **dict(TINY_UNET, in_channels=in_channels))
    args = dict(linear_start=0.00085, linear_end=0.0120, timesteps=1000, **kw)
    if cls == "edit":
        return ddpm.LatentEditDiffusion(unet_config=net, **args)
    if cls == "inpaint":
        return ddpm.LatentInpaintDiffusion(unet_config=net, **args)
    return ddpm.LatentDiffusion(net, **args)


def _samplers(model):
    from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.plms import PLMSSampler
    return [PLMSSampler(model), DDIMSampler(model), DPMSolverSampler(model)]


def _dicts():
    return ({"c_concat": torch.ones(2, 4, 8, 8), "c_crossattn": torch.ones(2, 6, 64)},
            {"c_concat": torch.zeros(2, 4, 8, 8), "c_crossattn": torch.zeros(2, 6, 64)})


def _sample(s, cond, uc, S=4, scale=7.5, **kw):
    return s.sample(S, 2, (4, 8, 8), conditioning=cond, unconditional_conditioning=uc, unconditional_guidance_scale=scale,
                    verbose=False, image_guidance_scale=1.5, **kw)


def test_every_sampler_refuses_what_image_guidance_does_not_run_with(monkeypatch):
    from minddiffusion_amd import distributed
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    model = _ldm()
    cond, uc = _dicts()
    for s in _samplers(model):
        name = type(s).__name__
        # per-request lists of S, scale or rescale
        for kw in (dict(S=[4, 2]), dict(scale=[7.5, 5.0]), dict(guidance_rescale=[0., 0.5])):
            with pytest.raises(MdxError, match=f"{name}.sample: image_guidance_scale does not run with per-request lists"):
                _sample(s, cond, uc, **kw)
        # mask / x0
        for kw in (dict(mask=torch.ones(2, 1, 8, 8), x0=torch.zeros(2, 4, 8, 8)), dict(x0=torch.zeros(2, 4, 8, 8))):
            with pytest.raises(MdxError, match="image_guidance_scale does not run with mask= / x0="):
                _sample(s, cond, uc, **kw)
        # what the run needs: dicts on both sides with a c_concat each
        for c_, uc_, what in ((cond["c_crossattn"], uc, "conditioning as a dict"), (cond, uc["c_crossattn"],
                              "unconditional_conditioning as a dict"), (cond, None, "unconditional_conditioning as a dict"),
                              (cond, {"c_crossattn": uc["c_crossattn"]}, r"unconditional_conditioning\['c_concat'\]"),
                              ({"c_concat": cond["c_concat"]}, uc, r"conditioning\['c_crossattn'\]")):
            with pytest.raises(MdxError, match=f"image_guidance_scale needs {what}"):
                _sample(s, c_, uc_)
        # one float
        with pytest.raises(MdxError, match="image_guidance_scale is one float"):
            s.sample(4, 2, (4, 8, 8), conditioning=cond, unconditional_conditioning=uc, verbose=False, image_guidance_scale=[1.5, 1.0])
        with pytest.raises(ValueError, match="image_guidance_scale must be finite"):
            s.sample(4, 2, (4, 8, 8), conditioning=cond, unconditional_conditioning=uc, verbose=False, image_guidance_scale=float("nan"))
    # wrapper models
    windowed = WindowedDiffusion(_ldm(4, "plain"), window=(8, 8))
    controlled = types.SimpleNamespace(is_controlled=True, num_timesteps=1000, alphas_cumprod=model.alphas_cumprod,
                                       alphas_cumprod_prev=model.alphas_cumprod_prev, betas=model.betas)
    for wrapped, what in ((windowed, "WindowedDiffusion"), (controlled, "ControlledDiffusion")):
        for s in _samplers(wrapped):
            with pytest.raises(MdxError, match=f"image_guidance_scale does not run on a {what} model"):
                _sample(s, cond, uc)
    # the adaptive method, and the ported reference surface
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver.solver import DPM_Solver, model_wrapper
    with pytest.raises(MdxError, match="image_guidance_scale does not run with method='adaptive'"):
        _sample(DPMSolverSampler(model), cond, uc, method="adaptive")
    ns = NoiseScheduleVP("discrete", alphas_cumprod=np.asarray(model.alphas_cumprod, np.float64))
    with pytest.raises(MdxError, match="model_wrapper: image_guidance_scale is not carried"):
        model_wrapper(model, ns, image_guidance_scale=1.5)
    with pytest.raises(MdxError, match="DPM_Solver.sample: image_guidance_scale is not carried"):
        DPM_Solver(model_wrapper(model, ns), ns).sample(torch.zeros(2, 4, 8, 8), image_guidance_scale=1.5)
    # several ranks
    monkeypatch.setattr(distributed, "world", lambda: (0, 2))
    for s in _samplers(model):
        with pytest.raises(MdxError, match="image_guidance_scale runs on a single rank"):
            _sample(s, cond, uc)


def test_image_guidance_none_is_todays_path(monkeypatch):
    """None builds the objects a run builds today, keyword for keyword: GuidedModel and ScalarSteps see no new argument."""
    from minddiffusion_amd.ldm.models.diffusion import plms
    from minddiffusion_amd.ldm.models.diffusion.dpm_solver import sampler as dpm
    from minddiffusion_amd.ldm.models.diffusion.guided import check_image_guidance
    assert check_image_guidance("x", None, None, None, None, "anything", "mask", "x0") is None
    seen = []

    class Stop(Exception):
        pass

    def guided(*a, **k):
        seen.append(("guided", len(a), k))
        raise Stop

    def steps(*a, **k):
        seen.append(("steps", len(a), k))
        return types.SimpleNamespace(any_sigma=[False] * 8)
    for mod in (plms, dpm):
        monkeypatch.setattr(mod, "GuidedModel", guided)
        monkeypatch.setattr(mod, "ScalarSteps", steps)
        monkeypatch.setattr(mod, "split_conditioning", lambda model, c, uc, x_T=None: (c["c_crossattn"], uc["c_crossattn"],
                                                                                       c["c_concat"], uc["c_concat"], "cpu"))
        monkeypatch.setattr(mod, "start_latent", lambda *a: torch.zeros(2, 4, 8, 8))
    cond, uc = _dicts()
    for s in _samplers(_ldm()):
        for ig, want in ((None, {}), (1.5, {"image_scale": 1.5})):
            del seen[:]
            with pytest.raises(Stop):
                s.sample(4, 2, (4, 8, 8), conditioning=cond, unconditional_conditioning=uc, unconditional_guidance_scale=7.5,
                         verbose=False, **({} if ig is None else {"image_guidance_scale": ig}))
            assert seen == [("steps", 3, want), ("guided", 10, want)], (type(s).__name__, ig, seen)


def test_sessions_refuse_image_guidance():
    from minddiffusion_amd.ldm.models.diffusion.session import check_request
    for k in ("image_guidance_scale", "image_scale"):
        with pytest.raises(ValueError, match=f"submit: {k} is not available in a session: three-branch image guidance"):
            check_request("ddim", 50, 30, 7.5, 0., 0., 0, **{k: 1.5})
    check_request("ddim", 50, 30, 7.5, 0., 0., 0, image_guidance_scale=None)


# ------------------------------------------------------------------------------------------------ pipe.edit refusals
def test_pipeline_edit_refusals(monkeypatch):
    from minddiffusion_amd import distributed
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.pipeline import DiffusionPipeline
    c = torch.zeros(2, 6, 64)
    image = torch.zeros(2, 3, 16, 16)
    for model, what in ((_ldm(4, "plain"), "4 input channels under 'crossattn'"), (_ldm(9, "inpaint"), "9 input channels under 'hybrid'"),
                        (_ldm(8, "plain"), "8 input channels under 'crossattn'")):
        with pytest.raises(MdxError, match=f"DiffusionPipeline.edit: needs an InstructPix2Pix model .* this one has {what}"):
            DiffusionPipeline(model, "ddim", device="cpu").edit(image, c=c, uc=c)
    pipe = DiffusionPipeline(_ldm(), "ddim", device="cpu")
    for bad in (torch.zeros(2, 3, 12, 16), torch.zeros(2, 4, 16, 16), torch.zeros(3, 16, 16), "picture"):
        with pytest.raises(MdxError, match="edit: (image must be a tensor|the image's H and W)"):
            pipe.edit(bad, c=c, uc=c)
    with pytest.raises(MdxError, match="3 images for a batch of 2"):
        pipe.edit(torch.zeros(3, 3, 16, 16), c=c, uc=c)
    with pytest.raises(MdxError, match="needs the unconditional context uc"):
        pipe.edit(image, c=c)
    for kw, name in ((dict(steps=[3, 2]), "steps"), (dict(scale=[7.5, 5.]), "scale"), (dict(image_scale=[1.5, 1.]), "image_scale"),
                     (dict(guidance_rescale=[0., 0.5]), "guidance_rescale")):
        with pytest.raises(MdxError, match=f"edit: {name} is one value for the batch"):
            pipe.edit(image, c=c, uc=c, **kw)
    with pytest.raises(ValueError, match="output must be"):
        pipe.edit(image, c=c, uc=c, output="pil")
    with pytest.raises(ValueError, match="guidance_rescale must be in"):
        pipe.edit(image, c=c, uc=c, guidance_rescale=1.5)
    # derived pipelines
    plain = DiffusionPipeline(_ldm(4, "plain"), "ddim", device="cpu")
    with pytest.raises(MdxError, match="edit: not on a windowed pipeline"):
        plain.windowed(window=64).edit(image, c=c, uc=c)
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.ldm.modules.diffusionmodules.controlnet import ControlNet
    with pytest.raises(MdxError, match="edit: not on a controlled pipeline"):
        plain.controlled(ControlNet(device="cpu", **TINY_UNET)).edit(image, c=c, uc=c)
    first, second = plain._hires_pipelines(128, 128, (64, 64), None)
    assert first is plain and second._hires_derived
    derived = DiffusionPipeline(_ldm(), "ddim", device="cpu")
    derived._hires_derived = True
    with pytest.raises(MdxError, match="edit: not on a hires-derived pipeline"):
        derived.edit(image, c=c, uc=c)
    monkeypatch.setattr(distributed, "world", lambda: (0, 2))
    with pytest.raises(MdxError, match="edit: runs on a single rank"):
        pipe.edit(image, c=c, uc=c)


# ------------------------------------------------------------------------------------------------ model, config, loader
def test_edit_config_and_model_class():
    from minddiffusion_amd import configs
    from minddiffusion_amd._lib import MdxError
    assert configs.WUKONG_EDIT_UNET == dict(configs.WUKONG_UNET, in_channels=8)
    m = _ldm()
    assert m.model.conditioning_key == "hybrid" and m.unet.in_channels == 8
    with pytest.raises(MdxError, match="encode_edit_image: no VAE attached"):
        m.encode_edit_image(torch.zeros(1, 3, 16, 16))
    calls = []
    m.first_stage_model = types.SimpleNamespace(encode=lambda x, **k: calls.append(k) or "mode")
    assert m.encode_edit_image("image") == "mode" and calls == [{"sample": False}]      # the mode, not scaled


def test_the_loader_takes_the_8_channel_conv_in_by_shape():
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from minddiffusion_amd.weights import synthetic_unet_params_numpy
    cfg8 = dict(TINY_UNET, in_channels=8)
    shapes8 = UNetModel(device="cpu", **cfg8).parameter_shapes()
    shapes4 = UNetModel(device="cpu", **TINY_UNET).parameter_shapes()
    differ = sorted(k for k in shapes8 if tuple(shapes8[k]) != tuple(shapes4[k]))
    assert len(differ) == 1 and 8 in tuple(shapes8[differ[0]]) and 4 in tuple(shapes4[differ[0]]), differ     # conv_in alone
    UNetModel(device="cpu", **cfg8).load_state_dict(synthetic_unet_params_numpy(shapes8))
    with pytest.raises(Exception, match=differ[0].replace(".", r"\.")) as e:
        UNetModel(device="cpu", **cfg8).load_state_dict(synthetic_unet_params_numpy(shapes4))
    assert type(e.value).__name__ in ("ValueError", "MdxError", "LoaderMismatch"), type(e.value)
