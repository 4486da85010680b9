"""Host-side rules the three LDM samplers share, without a GPU: which fused step entry ops.sampler_update picks, and what
GuidedModel decides once per run (guidance batch, identical halves, the time-embedding table)."""
import types

import pytest
import torch

UPDATE = (0.5, 0.6, 0.7, 0.8, 0.0, None, None, "x_prev", "pred_x0")


@pytest.fixture
def entries(monkeypatch):
    from minddiffusion_amd import ops
    calls = []
    for name in ("sampler_step", "sampler_step_pred", "sampler_step_rescale"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name: calls.append((_n, a)))
    return calls


def test_sampler_update_picks_the_entry_and_hands_over_its_arguments(entries):
    from minddiffusion_amd import ops
    x, xm, u, c = "x", "xm", torch.zeros(2, 4, 4, 8), torch.zeros(2, 4, 4, 8)
    olds, coef = ["e1"], (1.5, -0.5, 0., 0.)
    # eps, no rescale -- and rescale without an unconditional half: the plain entry
    ops.sampler_update(x, u, c, 3.0, ops.PRED_EPS, olds, coef, UPDATE)
    ops.sampler_update(x, None, c, 1.0, ops.PRED_EPS, olds, coef, UPDATE, 0.7, xm, 0.9, 0.1)
    assert entries == [("sampler_step", (x, u, c, 8, 3.0, olds, coef) + UPDATE),
                       ("sampler_step", (x, None, c, 8, 1.0, olds, coef) + UPDATE)]
    del entries[:]
    # v: the pred entry, with the point the model was evaluated at -- also under a rescale that has nothing to combine
    ops.sampler_update(x, u, c, 3.0, ops.PRED_V, olds, coef, UPDATE, 0., xm, 0.9, 0.1)
    ops.sampler_update(x, None, c, 3.0, ops.PRED_V, olds, coef, UPDATE, 0.7, xm, 0.9, 0.1)
    assert entries == [("sampler_step_pred", (x, xm, u, c, 8, 3.0, ops.PRED_V, 0.9, 0.1, olds, coef) + UPDATE),
                       ("sampler_step_pred", (x, xm, None, c, 8, 3.0, ops.PRED_V, 0.9, 0.1, olds, coef) + UPDATE)]
    del entries[:]
    # rescale with guidance: the rescale entry; an eps output is not converted, whatever point is passed
    ops.sampler_update(x, u, c, 3.0, ops.PRED_EPS, olds, coef, UPDATE, 0.7, xm, 0.9, 0.1)
    ops.sampler_update(x, u, c, 3.0, ops.PRED_V, olds, coef, UPDATE, 0.7, xm, 0.9, 0.1)
    assert entries == [("sampler_step_rescale", (x, xm, u, c, 8, 3.0, ops.PRED_EPS, 1., 0., olds, coef) + UPDATE + (0.7,)),
                       ("sampler_step_rescale", (x, xm, u, c, 8, 3.0, ops.PRED_V, 0.9, 0.1, olds, coef) + UPDATE + (0.7,))]


def _model(num_classes=None):
    table = []
    unet = types.SimpleNamespace(num_classes=num_classes)
    return types.SimpleNamespace(unet=unet, table=table,
                                 time_embedding_table=lambda t: table.append(t.clone()) or torch.zeros(t.shape[0], 3))


def _guided(model, scale=3.0, uc=True, c_cat=None, uc_cat=None, b=2):
    from minddiffusion_amd.ldm.models.diffusion.guided import GuidedModel
    cond = torch.ones(b, 5, 6)
    return GuidedModel(model, b, (4, 8, 8), cond, torch.zeros(b, 5, 6) if uc else None, c_cat, uc_cat, scale, "cpu",
                       [801., 601., 401.])


def test_guided_model_builds_the_guidance_batch_once():
    g = _guided(_model())
    assert g.use_cfg and g.same_halves and g.nb == 4
    assert tuple(g.c_in.shape) == (4, 5, 6) and torch.equal(g.c_in[:2], torch.zeros(2, 5, 6))       # [uncond; cond]
    assert tuple(g.x_in.shape) == (4, 4, 8, 8) and tuple(g.t_all.shape) == (3, 4)
    assert torch.equal(g.t_all[1], torch.full((4,), 601.))
    for kw in (dict(scale=1.0), dict(uc=False)):        # no guidance: the latent goes to the UNet as it is
        g = _guided(_model(), **kw)
        assert not g.use_cfg and not g.same_halves and g.nb == 2 and g.x_in is None and tuple(g.c_in.shape) == (2, 5, 6)


def test_guided_model_writes_c_concat_once_and_knows_when_the_halves_differ():
    cc, ucc = torch.full((2, 5, 8, 8), 2.0), torch.full((2, 5, 8, 8), 3.0)
    g = _guided(_model(), c_cat=cc)
    assert g.same_halves and tuple(g.x_in.shape) == (4, 9, 8, 8) and torch.equal(g.x_in[:, 4:], torch.cat([cc, cc]))
    g = _guided(_model(), c_cat=cc, uc_cat=ucc)
    assert g.use_cfg and not g.same_halves and torch.equal(g.x_in[:, 4:], torch.cat([ucc, cc]))
    g = _guided(_model(), c_cat=cc, uc=False)
    assert not g.use_cfg and tuple(g.x_in.shape) == (2, 9, 8, 8) and torch.equal(g.x_in[:, 4:], cc)


def test_the_time_embedding_table_is_not_used_for_a_class_conditional_unet(monkeypatch):
    """label_emb(y) joins emb per call, so a table of the timestep-only part would drop it: every sampler skips the table."""
    m = _model()
    assert _guided(m).temb_all is not None and len(m.table) == 1 and m.table[0].tolist() == [801., 601., 401.]
    m = _model(num_classes=10)
    assert _guided(m).temb_all is None and m.table == []
    monkeypatch.setenv("MDX_SAMPLER_TEMB_TABLE", "0")
    m = _model()
    assert _guided(m).temb_all is None and m.table == []
