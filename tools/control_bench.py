#!/usr/bin/env python3
"""What ControlNet costs on the full SD2 UNet (configs.SD2_UNET, synthetic weights) at 512 x 512 (a 64 x 64 latent) and the
classifier-free-guidance batch of 2.

  eval   milliseconds per model evaluation with hipGraphs replayed, warm, median of --reps device-event timings, the four forms
         alternated inside every repetition: the plain UNet (LatentDiffusion.apply_model_nhwc), the wrapper outside its scope,
         controlled with uncond=True (ControlNet at batch 2) and with uncond=False (ControlNet at batch 1, "guess mode").
         Also: launches of a plain EAGER evaluation (UNetModel.last_launch_count) and of the control plan.
  add    the one mdx_control_add_f16 launch over the 13 residuals of that shape against 13 separate torch adds (dst.add_(src)),
         each captured as one hipGraph and replayed --inner times between two device events; median of --reps.  Bytes moved are
         computed from the shapes (2 reads + 1 write of every destination element).

Each step runs in a child process under its own time limit; the parent prints one JSON line and writes --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, T = 1, 64, 64, 77          # one sample under guidance: the UNet batch is [uncond ; cond] = 2


def _models():
    import torch
    from minddiffusion_amd.configs import SD2_LDM, SD2_UNET
    from minddiffusion_amd.ldm.models.diffusion.controlled import ControlledDiffusion
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from minddiffusion_amd.ldm.modules.diffusionmodules.controlnet import ControlNet
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from minddiffusion_amd.weights import synthetic_unet_params_device
    net, cn = UNetModel(**SD2_UNET), ControlNet(**SD2_UNET)
    net.load_state_dict(synthetic_unet_params_device(net.parameter_shapes(), seed=0))
    cn.load_state_dict(synthetic_unet_params_device(cn.parameter_shapes(), seed=1))
    model = LatentDiffusion(net, **SD2_LDM)
    torch.cuda.synchronize()
    return model, cn, ControlledDiffusion(model, cn)


def step_eval(reps):
    import torch
    model, cn, cm = _models()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(2 * B, 4, H, W, device=dev, generator=g)
    t = torch.full((2 * B,), 500.0, device=dev)
    c = torch.randn(2 * B, T, 1024, device=dev, generator=g).to(torch.float16)
    hint = (torch.rand(B, 3, 8 * H, 8 * W, device=dev, generator=g) > 0.5).to(torch.float32)
    unet = model.unet
    # launches of a plain eager evaluation: what the parent commit's plan launches must equal
    unet.use_graph = False
    model.apply_model_nhwc(x, t, c)
    plain_eager = unet.last_launch_count
    unet.use_graph = True
    forms = {
        "plain": lambda: model.apply_model_nhwc(x, t, c),
        "wrapper_outside_scope": lambda: cm.apply_model_nhwc(x, t, c),
    }
    scopes = {"control_uncond_true": True, "control_uncond_false": False}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k in list(forms) + list(scopes)}

    def timed(name, fn):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        times[name].append(ev[0].elapsed_time(ev[1]))
    for i in range(reps + 3):           # three warm-up rounds: plans, captures, the hint block
        for name, fn in forms.items():
            timed(name, fn)
        for name, uncond in scopes.items():
            with cm.control(hint, uncond=uncond):
                cm.apply_model_nhwc(x, t, c)          # (entering a scope prepares its tables: not part of a step)
                timed(name, lambda: cm.apply_model_nhwc(x, t, c))
    med = {k: statistics.median(v[3:]) for k, v in times.items()}
    lo = {k: min(v[3:]) for k, v in times.items()}
    pc = unet._plans[(2 * B, H, W, "control")]
    pp = unet._plans[(2 * B, H, W)]
    launches = lambda P: sum(m["launches"] for m in P.meta[P.temb_ops:])
    return dict(step="eval", reps=reps, ms_median=med, ms_min=lo, plain_eager_launch_count=plain_eager,
                plain_plan_launches=launches(pp), control_plan_launches=launches(pc),
                controlnet_plan_launches={str(k): launches(p) for k, p in cn._plans.items()},
                graphs=dict(plain=pp.graph is not None, control=pc.graph is not None), hint_runs=cn.hint_runs,
                control_over_plain=med["control_uncond_true"] / med["plain"],
                guess_over_plain=med["control_uncond_false"] / med["plain"])


def step_add(reps, inner):
    import torch
    from minddiffusion_amd import ops
    from minddiffusion_amd.configs import SD2_UNET
    from minddiffusion_amd.ldm.modules.diffusionmodules.controlnet import ControlNet
    dev = "cuda:0"
    cn = ControlNet(**SD2_UNET)
    chans, h, w, shapes = cn.block_channels(), H, W, []
    for blk, ch in zip(cn.input_blocks, chans):
        if blk[-1][0] in ("down", "resdown"):
            h, w = h // 2, w // 2
        shapes.append((h * w, ch))
    shapes.append(shapes[-1])           # the middle block's output
    nb = 2 * B
    g = torch.Generator(device=dev).manual_seed(4)
    dsts = [torch.randn(nb, n, ch, device=dev, generator=g).to(torch.float16) for n, ch in shapes]
    srcs = [torch.randn(nb, n, ch, device=dev, generator=g).to(torch.float16) * 0.01 for n, ch in shapes]
    halves = sum(t.numel() for t in dsts)
    ca = ops.ControlAdd(dsts)
    ca.set_sources(srcs, list(range(nb)))
    ca.set_scale(1.0)
    bodies = {"one_launch": [ca.run] * inner,
              "torch_13_adds": [(lambda d=d, s=s: d.add_(s)) for _ in range(inner) for d, s in zip(dsts, srcs)]}
    graphs = {}
    for name, body in bodies.items():
        for op in body[:len(body) // inner]:
            op()
        torch.cuda.synchronize()
        graphs[name] = ops.capture_graph(body)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    us = {k: [] for k in graphs}
    for i in range(reps + 3):
        for name, gr in graphs.items():
            ev[0].record()
            gr.replay()
            ev[1].record()
            torch.cuda.synchronize()
            us[name].append(ev[0].elapsed_time(ev[1]) * 1e3 / inner)
    med = {k: statistics.median(v[3:]) for k, v in us.items()}
    return dict(step="add", reps=reps, inner=inner, segments=len(dsts), halves_per_batch_row=halves // nb, batch_rows=nb,
                bytes_moved=6 * halves, us_median=med, us_min={k: min(v[3:]) for k, v in us.items()},
                GBps_one_launch=6 * halves / med["one_launch"] / 1e3, torch_over_one_launch=med["torch_13_adds"] / med["one_launch"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20, help="adds per graph replay in the add step")
    ap.add_argument("--step", choices=["eval", "add"], help="run one step in this process (used by the parent)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "control_bench.json"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step_eval(a.reps) if a.step == "eval" else step_add(a.reps, a.inner)))
        return 0
    result = {}
    for step in ("add", "eval"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--inner", str(a.inner)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"control_bench: step {step} exceeded {a.timeout} s; stopping", file=sys.stderr)
            return 124
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"control_bench: step {step} ended with status {r.returncode}; stopping", file=sys.stderr)
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
