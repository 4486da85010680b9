"""The single launches that tests/golden/step_family_parent.json pins (tests/test_step_family_bits_gpu.py and
tests/golden/make_step_family_parent_golden.py share them): every kernel instantiation of the fused sampler step family
(csrc/sampler_step.hip) at least once, on shapes at which a changed rounding in one launch form would show -- which the
whole-run goldens on a 2 x 4 x 8 x 8 latent (one trip of every loop, no partial quad) cannot see.  Built from the public
ops step functions only, so the file runs unchanged on the library that recorded the golden file and on every later one.

A case is ONE launch on seeded random inputs (numpy RandomState keyed by the case's name) and returns all of its output
tensors, each filled with FILL before the launch so that what a launch leaves unwritten (an inactive row) is pinned too.

Shapes (the model outputs are NHWC fp16 with out_ld = C + 3 > C):
  (3, 4, 5, 7)    140 elements per sample: fewer than a 1024-thread workgroup
  (2, 3, 5, 7)    105 elements: N % 4 == 1 and HW % 4 == 3, a partial last quad and quads that straddle channels
  (2, 4, 33, 37)  4884 elements > 4 * 1024: the owned loops take a second trip; HW is odd
"""
import hashlib
import zlib

import numpy as np
import torch

SHAPES = {"140": (3, 4, 5, 7), "105": (2, 3, 5, 7), "4884": (2, 4, 33, 37)}
LD_EXTRA = 3
FILL = -7.0
f32 = np.float32
PRED = {"eps": 0, "v": 1}          # ops.PRED_EPS, ops.PRED_V
VALUE = {"x0": 0, "epsval": 1}     # ops.VALUE_X0, ops.VALUE_EPS
AM, BM = float(f32(0.8)), float(f32(0.6))                      # the schedule point the model was evaluated at
UPDATE = tuple(float(f32(v)) for v in (0.83, 0.5577, 0.9, 0.41))  # sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef
SIGMA = float(f32(0.13))
ORDER3 = tuple(float(f32(v)) for v in (55 / 24, -59 / 24, 37 / 24, -9 / 24))
ORDER1 = tuple(float(f32(v)) for v in (1.5, -0.5, 0., 0.))
PHI = 0.7
SEEDS = [11, (1 << 63) + 5, -3]
DRAW = 5


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def _dev(a, dev, dtype=None):
    t = torch.tensor(a, device=dev)
    return t if dtype is None else t.to(dtype)


def _inputs(name, shape, dev):
    """x, x_model, three histories, noise [B, C, H, W] fp32; out_u / out_c NHWC fp16 on an offset (the rescale statistics
    then have something to cancel)."""
    B, C, H, W = shape
    r = _rng(name)
    t = {k: _dev(r.randn(*shape).astype(f32), dev) for k in ("x", "x_model", "old1", "old2", "old3", "noise")}
    for k in ("out_u", "out_c"):
        t[k] = _dev((0.3 + r.randn(B, H * W, C + LD_EXTRA)).astype(f32), dev, torch.float16)
    return t


def _outs(shape, dev, names):
    return {k: torch.full(shape if k not in ("factor_out", "thr_out") else (shape[0],), FILL, device=dev) for k in names}


# ------------------------------------------------------------------------------------------------ eps family, scalar entries
def _scalar(ops, dev, name, shape, pred, form):
    t = _inputs(name, shape, dev)
    ld = shape[1] + LD_EXTRA
    o = _outs(shape, dev, ("e_t_out", "x_prev", "pred_x0") + (("factor_out",) if form == "rescale" else ()))
    head = (t["x"], t["x_model"])
    if form == "plain_unguided_order0":
        ops.sampler_step_pred(*head, None, t["out_c"], ld, 1.0, pred, AM, BM, [], (1., 0., 0., 0.), *UPDATE, 0., None,
                              o["e_t_out"], o["x_prev"], o["pred_x0"])
    else:
        olds = [t["old1"], t["old2"], t["old3"]]
        args = (*head, t["out_u"], t["out_c"], ld, 3.5, pred, AM, BM, olds, ORDER3, *UPDATE, SIGMA, t["noise"], o["e_t_out"],
                o["x_prev"], o["pred_x0"])
        if form == "rescale":
            ops.sampler_step_rescale(*args, PHI, factor_out=o["factor_out"])
        else:
            ops.sampler_step_pred(*args)
    return o


# ------------------------------------------------------------------------------------------------ eps family, rows
def _row(ops, kind, rescale):
    """One MDX_STEP_ROW: "act" an order-3 step with noise (rescaled iff the launch rescales), "phi0" an order-1 step without
    noise or rescale at another guidance scale, "inactive" a finished request."""
    row = np.zeros(ops.STEP_ROW, f32)
    if kind == "inactive":
        return row
    act = kind == "act"
    row[ops.STEP_ACTIVE] = 1.
    row[ops.STEP_CFG_SCALE] = 3.5 if act else 1.75
    row[ops.STEP_RESCALE] = PHI if act and rescale else 0.
    row[ops.STEP_SQRT_AT_MODEL], row[ops.STEP_SQRT_ONE_MINUS_AT_MODEL] = AM, BM
    row[ops.STEP_C0:ops.STEP_C0 + 4] = ORDER3 if act else ORDER1
    row[ops.STEP_SQRT_AT:ops.STEP_SQRT_AT + 4] = UPDATE if act else (0.9, 0.4359, 0.95, 0.3)
    row[ops.STEP_SIGMA] = SIGMA if act else 0.
    return row


def _rows(ops, dev, name, shape, pred, entry, rescale, rot, alias):
    t = _inputs(name, shape, dev)
    B = shape[0]
    o = _outs(shape, dev, ("e_t_out", "x_prev", "pred_x0", "factor_out"))
    if alias:
        o["x_prev"] = t["x"]
    olds = [t["old1"], t["old2"], t["old3"]]
    head = (t["x"], t["x_model"], t["out_u"], t["out_c"], pred, olds, t["noise"], o["e_t_out"], o["x_prev"], o["pred_x0"])
    if entry == "table":
        kinds = [("act", "inactive", "phi0")[(b + rot) % 3] for b in range(B)]
        table = _dev(np.stack([_row(ops, k, rescale) for k in kinds]), dev)
        ops.sampler_step_table(*head, table, rescale, factor_out=o["factor_out"])
    else:           # slots: "outside" stands on no row of its request (its tick has passed the request's length)
        kinds = [("act", "outside", "phi0", "inactive")[(b + rot) % 4] for b in range(B)]
        cap, tick = 4, 6
        start = np.array([tick - 1 - b for b in range(B)], np.int32)          # slot b stands on row 1 + b
        length = np.array([1 + b if k == "outside" else cap for b, k in enumerate(kinds)], np.int32)
        sched = np.stack([np.stack([_row(ops, "phi0" if k == "act" else "act", rescale)] * cap) for k in kinds])
        for b, k in enumerate(kinds):
            sched[b, 1 + b] = _row(ops, "act" if k == "outside" else k, rescale)
        ops.sampler_step_slots(*head, _dev(sched, dev), _dev(start, dev), _dev(length, dev), tick, rescale,
                               factor_out=o["factor_out"])
    return o


# ------------------------------------------------------------------------------------------------ lin family
def _lin(ops, dev, name, shape, pred, value, form, noise, thresholding):
    t = _inputs(name, shape, dev)
    o = _outs(shape, dev, ("model_out", "x_out", "model_pre_out", "thr_out", "factor_out"))
    kw = dict(thresholding=thresholding, max_val=0.5, model_pre_out=o["model_pre_out"], thr_out=o["thr_out"],
              factor_out=o["factor_out"])
    if form == "bare":          # no guidance, no x_base term, no history
        args = (t["x"], t["x_model"], None, t["out_c"], 1.0, pred, 0., value, AM, BM, None, None, 0., 1.25, 0., 0.)
    else:
        args = (t["x"], t["x_model"], t["out_u"], t["out_c"], 3.5, pred, PHI if form == "owned" else 0., value, AM, BM,
                t["old1"], t["old2"], 0.9, -0.45, 0.3, -0.1)
    args += (o["model_out"], o["x_out"])
    if noise == "none":
        ops.sampler_step_lin(*args, **kw)
    elif noise == "tensor":
        ops.sampler_step_lin_noise(*args, 0.37, noise=t["noise"], **kw)
    else:
        ops.sampler_step_lin_noise(*args, 0.37, seeds=ops.seeds_tensor(SEEDS[:shape[0]], dev), draw=DRAW, **kw)
    return o


# ------------------------------------------------------------------------------------------------ slot_gather
def _gather(ops, dev, name, n):
    B, cap, tick, reps = 3, 4, 6, 2
    src = _dev(_rng(name).randn(B, cap, n).astype(f32), dev)
    start = _dev(np.array([5, 3, 6], np.int32), dev)
    length = _dev(np.array([4, 2, 4], np.int32), dev)        # slot 1 is outside its request
    out = torch.full((reps * B, n), FILL, device=dev)
    ops.slot_gather(src, start, length, tick, out, reps=reps)
    return {"out": out}


def cases():
    """name -> function (ops, device) -> {output name: device tensor}."""
    c = {}

    def add(name, fn, *args):
        c[name] = lambda ops, dev: fn(ops, dev, name, *args)

    for sk, shape in SHAPES.items():
        for pk, pred in PRED.items():
            for form in ("plain_unguided_order0", "plain_guided_order3_sigma", "rescale"):
                add(f"step_{form}_{pk}_{sk}", _scalar, shape, pred, form)
            for entry in ("table", "slots"):
                for rescale in (0, 1):
                    for rot in (0, 1):
                        add(f"{entry}_rescale{rescale}_rot{rot}_{pk}_{sk}", _rows, shape, pred, entry, rescale, rot, False)
                    add(f"{entry}_rescale{rescale}_alias_{pk}_{sk}", _rows, shape, pred, entry, rescale, 0, True)
            for vk, value in VALUE.items():
                add(f"lin_bare_{pk}_{vk}_{sk}", _lin, shape, pred, value, "bare", "none", False)
                for noise in ("none", "tensor", "seeded"):
                    for form in ("spread", "owned"):
                        add(f"lin_{form}_{noise}_{pk}_{vk}_{sk}", _lin, shape, pred, value, form, noise, False)
                    if vk == "x0":
                        add(f"lin_threshold_{noise}_{pk}_{vk}_{sk}", _lin, shape, pred, value, "spread", noise, True)
    add("slot_gather_n140", _gather, 140)
    add("slot_gather_n105", _gather, 105)
    return c


def digests(ops, dev):
    """name -> {output name: SHA-256 of the output's raw bytes}."""
    out = {}
    for name, fn in cases().items():
        got = fn(ops, dev)
        torch.cuda.synchronize()
        out[name] = {k: hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest() for k, v in sorted(got.items())}
    return out
