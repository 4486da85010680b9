"""Shared helpers of tests/test_step_table_gpu.py: one step's tensors come from test_guidance_rescale_gpu._case, the per-sample
scalars -- a row each, all different -- from rows_for(); run_table() launches mdx_sampler_step_table_f32 on the whole batch,
run_scalar() the scalar entry ops.sampler_update would pick for ONE row's scalars on that sample's batch-1 slice."""
import numpy as np
import torch

import test_guidance_rescale_gpu as GR
from _guard import SENT

DEV = GR.DEV
dev32, out_buf, COEF = GR.dev32, GR.out_buf, GR.COEF


def case(shape, pred, order, sigma, separate_xm, seed):
    """The tensors of one step (x, xm, vu, vc, olds, noise); the noise is there whatever sigma says: rows decide."""
    a = GR._case(shape, pred, order, 0.3, separate_xm, seed)
    a["sigma"] = sigma
    return a


def rows_for(a, phis, active=None, order=None):
    """One dict of scalars per sample, no two alike: guidance scale, schedule point, model point, multistep coefficients and
    sigma all move with b.  phis / active: per sample, repeated to the batch."""
    B = a["x"].shape[0]
    order = len(a["olds"]) if order is None else order
    f = np.float32
    rows = []
    for b in range(B):
        a_t, a_prev = f(0.3 + 0.05 * b), f(0.5 + 0.04 * b)
        sigma = f(a["sigma"] * (1.0 + 0.1 * b))          # (at most 0.42: 1 - a_prev - sigma^2 stays positive)
        coef = tuple(f(c * (1.0 + 0.125 * b)) for c in COEF[order])
        rows.append(dict(active=1.0 if active is None else float(active[b % len(active)]), scale=f(1.5 + 2.0 * b),
                         phi=f(phis[b % len(phis)]), am=f(np.sqrt(0.4 + 0.03 * b)), bm=f(np.sqrt(0.6 - 0.03 * b)), coef=coef,
                         update=(np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_prev), np.sqrt(1 - a_prev - sigma ** 2), sigma)))
    return rows


def table_of(ops, rows):
    t = np.zeros((len(rows), ops.STEP_ROW), np.float32)
    for b, r in enumerate(rows):
        t[b, ops.STEP_ACTIVE] = r["active"]
        t[b, ops.STEP_CFG_SCALE], t[b, ops.STEP_RESCALE] = r["scale"], r["phi"]
        t[b, ops.STEP_SQRT_AT_MODEL], t[b, ops.STEP_SQRT_ONE_MINUS_AT_MODEL] = r["am"], r["bm"]
        t[b, ops.STEP_C0:ops.STEP_C0 + 4] = r["coef"]
        t[b, ops.STEP_SQRT_AT:ops.STEP_SIGMA + 1] = r["update"]
    return torch.tensor(t, device=DEV)


def sentinel_like(x):
    return torch.full_like(x, SENT)


def run_table(ops, a, rows, any_rescale, no_u=False, x_t=None, xm_t=None, x_prev=None, outs=None, olds=None, noise=None):
    """(x_prev, pred_x0, e_t_out, factor_out) of one table launch; fresh outputs start as the sentinel.  x_t / xm_t / x_prev:
    preallocated device tensors (to alias them); outs: (x_prev, pred_x0, e_t_out, factor_out) to write into; olds / noise:
    device tensors to use instead of the case's."""
    xd = dev32(a["x"]) if x_t is None else x_t
    xmd = xm_t if xm_t is not None else (None if a["xm"] is a["x"] else dev32(a["xm"]))
    if outs is None:
        outs = (sentinel_like(xd) if x_prev is None else x_prev, sentinel_like(xd), sentinel_like(xd),
                torch.full((xd.shape[0],), SENT, device=DEV))
    x_out, p_out, e_out, f_out = outs
    ops.sampler_step_table(xd, xmd, None if no_u else out_buf(a["vu"]), out_buf(a["vc"]), a["pred"],
                           [dev32(o) for o in a["olds"]] if olds is None else olds,
                           dev32(a["noise"]) if noise is None else noise, e_out, x_out, p_out, table_of(ops, rows),
                           any_rescale, f_out)
    torch.cuda.synchronize()
    return x_out, p_out, e_out, f_out


def scalar_entry(pred, phi, has_u):
    """ops.sampler_update's choice."""
    return "rescale" if phi != 0 and has_u else "pred" if pred == 1 else "plain"


def run_scalar(ops, a, rows, b, no_u=False, drop=()):
    """The same four from the scalar entry for row b's scalars, on sample b alone.  drop: names among old1 / old2 / old3 /
    noise handed over as NULL (with their coefficient as the row has it, zero)."""
    r = rows[b]
    s = slice(b, b + 1)
    xd = dev32(a["x"][s])
    xmd = None if a["xm"] is a["x"] else dev32(a["xm"][s])
    olds = [dev32(o[s]) for k, o in enumerate(a["olds"]) if f"old{k + 1}" not in drop]
    noise = dev32(a["noise"][s]) if float(r["update"][4]) != 0 and "noise" not in drop else None
    x_out, p_out, e_out = (torch.empty_like(xd) for _ in range(3))
    f_out = torch.ones(1, device=DEV)
    ou, oc = None if no_u else out_buf(a["vu"][s]), out_buf(a["vc"][s])
    entry = scalar_entry(a["pred"], float(r["phi"]), not no_u)
    tail = (olds, r["coef"], *r["update"][:5], noise, e_out, x_out, p_out)
    if entry == "rescale":
        ops.sampler_step_rescale(xd, xmd, ou, oc, 8, r["scale"], a["pred"], r["am"], r["bm"], *tail, r["phi"], f_out)
    elif entry == "pred":
        ops.sampler_step_pred(xd, xmd, ou, oc, 8, r["scale"], a["pred"], r["am"], r["bm"], *tail)
    else:
        ops.sampler_step(xd, ou, oc, 8, r["scale"], *tail)
    torch.cuda.synchronize()
    return x_out, p_out, e_out, f_out


def assert_row_equals_scalar(got, want, b, tag):
    for g, w, name in zip(got, want, ("x_prev", "pred_x0", "e_t_out", "factor_out")):
        gb = g[b:b + 1]
        assert bool(torch.isfinite(gb).all()), (tag, b, name)
        assert torch.equal(gb, w), (tag, b, name, float((gb - w).abs().max()))
