#!/usr/bin/env python3
"""What three-branch guidance (InstructPix2Pix, pipe.edit) costs per sampling step on the full configs.WUKONG_EDIT_UNET
(synthetic weights) at a 64 x 64 latent, B = 1.

  launch  microseconds per fused step launch, the dual entry (three model outputs) against the two-branch launch it extends,
          in three forms: eps SPREAD (PLMS Adams-Bashforth-4 step, no rescale), eps OWNED (the same with guidance_rescale = 0.7)
          and lin SPREAD (a second-order DPM-Solver data-prediction update).  Each form is captured as one hipGraph of --inner
          launches and replayed between two device events; all forms alternate inside every repetition; median of --reps, with
          the 10th and 90th percentile as the run-to-run spread.  The dual launch reads 1.5 x the fp16 model output and the
          same fp32 operands.
          --parent-lib PATH: a build of the PARENT commit's library.  Its three two-branch launches are captured too and
          alternate with this build's in the same repetitions (pair_parent_* against pair_*).
  eval    milliseconds per model evaluation with hipGraphs replayed, warm: the three-branch batch (UNet batch 3) against the
          guidance batch (UNet batch 2), alternated, median of --reps.

Each step runs in a child process under its own time limit; the parent prints one JSON line and writes --out.
"""
import argparse
import contextlib
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, C, H, W, T, LD = 1, 4, 64, 64, 77, 8


def _summary(v):
    v = sorted(v)
    q = lambda p: v[min(len(v) - 1, int(p * len(v)))]
    return dict(median=statistics.median(v), p10=q(0.1), p90=q(0.9), min=v[0])


@contextlib.contextmanager
def _library(path):
    """Route the ops wrappers to another build of the same C-ABI for the block (the two-branch entries are all it needs)."""
    from minddiffusion_amd import _lib
    if path is None:
        yield
        return
    other = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(other, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    head = _lib.load()
    _lib._lib = other
    try:
        yield
    finally:
        _lib._lib = head


def step_launch(reps, inner, parent_lib):
    import torch
    from minddiffusion_amd import ops
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(5)
    f32 = lambda: torch.randn(B, C, H, W, device=dev, generator=g)
    f16 = lambda: torch.randn(B, H * W, LD, device=dev, generator=g).to(torch.float16)
    x, o1, o2, o3, h1 = f32(), f32(), f32(), f32(), f32()
    u, m, c = f16(), f16(), f16()
    e_out, x_out, p_out = (torch.empty_like(x) for _ in range(3))
    ab4 = (55 / 24, -59 / 24, 37 / 24, -9 / 24)
    update = (0.8, 0.6, 0.85, 0.52, 0.0, None, e_out, x_out, p_out)

    def eps(phi, mid):
        return lambda: ops.sampler_update(x, u, c, 7.5, ops.PRED_EPS, [o1, o2, o3], ab4, update, phi, **mid)

    def lin(dual):
        tail = (ops.PRED_EPS, 0., ops.VALUE_X0, 0.8, 0.6, h1, None, 0.9, 0.3, -0.1, 0., p_out, x_out)
        if dual:
            return lambda: ops.sampler_step_lin_dual(x, x, u, m, c, 7.5, 1.5, *tail)
        return lambda: ops.sampler_step_lin(x, x, u, c, 7.5, *tail)
    mid = dict(out_m=m, mid_scale=1.5)
    pair = {"eps_spread": eps(0., {}), "eps_owned": eps(0.7, {}), "lin_spread": lin(False)}
    forms = {f"pair_{k}": (None, fn) for k, fn in pair.items()}
    forms.update({"dual_eps_spread": (None, eps(0., mid)), "dual_eps_owned": (None, eps(0.7, mid)),
                  "dual_lin_spread": (None, lin(True))})
    if parent_lib:
        forms.update({f"pair_parent_{k}": (parent_lib, fn) for k, fn in pair.items()})
    graphs = {}
    for name, (lib, fn) in forms.items():
        with _library(lib):
            fn()
            torch.cuda.synchronize()
            graphs[name] = ops.capture_graph([fn] * inner)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    us = {k: [] for k in graphs}
    for i in range(reps + 3):
        for name, gr in graphs.items():
            ev[0].record()
            gr.replay()
            ev[1].record()
            torch.cuda.synchronize()
            us[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / inner)
    out = {k: _summary(v[3:]) for k, v in us.items()}
    ratio = {k: out[f"dual_{k}"]["median"] / out[f"pair_{k}"]["median"] for k in pair}
    res = dict(step="launch", reps=reps, inner=inner, latent=[B, C, H, W], us=out, dual_over_pair=ratio,
               fp16_bytes_read=dict(pair=2 * B * H * W * LD * 2, dual=3 * B * H * W * LD * 2))
    if parent_lib:
        res["head_over_parent"] = {k: out[f"pair_{k}"]["median"] / out[f"pair_parent_{k}"]["median"] for k in pair}
    return res


def step_eval(reps):
    import torch
    from minddiffusion_amd.configs import SD2_LDM, WUKONG_EDIT_UNET
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentEditDiffusion
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from minddiffusion_amd.weights import synthetic_unet_params_device
    dev = "cuda:0"
    net = UNetModel(**WUKONG_EDIT_UNET)
    net.load_state_dict(synthetic_unet_params_device(net.parameter_shapes(), seed=0))
    model = LatentEditDiffusion(unet_config=net, **dict(SD2_LDM, conditioning_key="hybrid"))
    g = torch.Generator(device=dev).manual_seed(3)
    forms = {}
    for name, nb in (("pair_batch2", 2 * B), ("dual_batch3", 3 * B)):
        x = torch.randn(nb, 8, H, W, device=dev, generator=g)
        t = torch.full((nb,), 500.0, device=dev)
        ctx = torch.randn(nb, T, int(net.context_dim), device=dev, generator=g).to(torch.float16)
        forms[name] = lambda x=x, t=t, ctx=ctx: model.apply_model_nhwc(x, t, ctx)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {k: [] for k in forms}
    for i in range(reps + 3):           # three warm-up rounds: plans and captures
        for name, fn in forms.items():
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ms[name].append(ev[0].elapsed_time(ev[1]))
    out = {k: _summary(v[3:]) for k, v in ms.items()}
    return dict(step="eval", reps=reps, ms=out, dual_over_pair=out["dual_batch3"]["median"] / out["pair_batch2"]["median"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=50, help="launches per graph replay in the launch step")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library, for the two-branch launches")
    ap.add_argument("--step", choices=["launch", "eval"], help="run one step in this process (used by the parent)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_bench.json"))
    a = ap.parse_args()
    if a.step:
        res = step_launch(a.reps, a.inner, a.parent_lib) if a.step == "launch" else step_eval(a.reps)
        print("RESULT " + json.dumps(res))
        return 0
    result = {}
    for step in ("launch", "eval"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--inner", str(a.inner)]
        if a.parent_lib:
            cmd += ["--parent-lib", os.path.abspath(a.parent_lib)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"edit_bench: step {step} exceeded {a.timeout} s; stopping", file=sys.stderr)
            return 124
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"edit_bench: step {step} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        result[step] = json.loads(line[-1][len("RESULT "):])
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
