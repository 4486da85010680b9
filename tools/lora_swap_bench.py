#!/usr/bin/env python3
"""Cost of switching the LoRA adapter of the full Wukong UNet (configs.WUKONG_LORA_UNET, synthetic weights).

  swap    UNetModel.load_lora_state_dict on a loaded enable_lora model: the in-place merge (mdx_lora_merge_f16, one launch per
          place a target matrix lives).  Device time between a hip event in front of the first merge launch and one behind the
          last, and host wall time of the whole call with the adapter given as host arrays (key check and upload of its 256
          tensors, 3 MB, included); warm, median of --reps.
  reload  what reaches the same state without the merge kernel: load_state_dict(merged parameters) on a plain model.  Wall
          time with the merged parameters ALREADY on the device (no upload: the packing alone), median of --reload-reps; it
          also discards every plan and captured graph (reported as plans_kept).

Each step runs in a child process under its own time limit; the parent prints one JSON line (and writes --out).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _setup(lora):
    import torch
    from minddiffusion_amd.configs import WUKONG_LORA_UNET, WUKONG_UNET
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from minddiffusion_amd.weights import synthetic_unet_params_device
    net = UNetModel(**(WUKONG_LORA_UNET if lora else WUKONG_UNET))
    params = synthetic_unet_params_device(net.parameter_shapes(), seed=0)
    shapes = UNetModel(**WUKONG_LORA_UNET).lora_parameter_shapes()
    adapters = []       # host numpy arrays, as a checkpoint reader delivers them: the timed call uploads them
    for seed in (1, 2):
        rng = np.random.RandomState(seed)
        adapters.append({k: (rng.standard_normal(s) * (s[1] ** -0.5 if k.endswith("lora_a") else 0.5)).astype(np.float32)
                         for k, s in shapes.items()})
    return net, params, adapters


def step_swap(reps):
    import torch
    net, params, adapters = _setup(True)
    net.load_state_dict(params)
    plain_bytes = sum(t.numel() * t.element_size() for t in net.w.values())
    x = torch.randn(2, 4, 64, 64, device="cuda:0")
    ctx = torch.randn(2, 77, 768, device="cuda:0")
    net(x, torch.tensor([500.0, 500.0], device="cuda:0"), ctx)        # a plan and a captured graph to keep
    plans = dict(net._plans)
    graphs = [p.graph for p in plans.values()]
    written = read = launches = 0
    for name, sites in net._lora_sites.items():
        n, k = net._lora_base[name].shape
        for s in sites:
            launches += 1
            read += 4 * n * k
            kp = (k + 63) // 64 * 64 if s["layout"] == 1 else k
            written += 2 * n * kp + (8 * n if "S" in s else 0)
    dev_ms, wall_ms = [], []
    merge = net._merge_lora
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed_merge():
        ev[0].record()
        merge()
        ev[1].record()
    net._merge_lora = timed_merge
    for i in range(reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net.load_lora_state_dict(adapters[i % 2])
        torch.cuda.synchronize()
        if i >= 3:
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            dev_ms.append(ev[0].elapsed_time(ev[1]))
    kept = all(net._plans.get(k) is p for k, p in plans.items()) and [p.graph for p in plans.values()] == graphs
    med = statistics.median(dev_ms)
    return dict(step="swap", reps=reps, merge_launches=launches, bytes_written=written, bytes_read=read,
                device_ms_median=med, device_ms_min=min(dev_ms), wall_ms_median=statistics.median(wall_ms),
                write_GBps=written / med / 1e6, traffic_GBps=(written + read) / med / 1e6, plans_kept=bool(kept),
                weight_bytes_plain=plain_bytes, weight_bytes_lora=net.weight_bytes(),
                lora_base_bytes=sum(t.numel() * 4 for t in net._lora_base.values()))


def step_reload(reps):
    import torch
    net, params, adapters = _setup(False)
    ad = adapters[0]
    merged = dict(params)
    for k, a in ad.items():
        if k.endswith("lora_a"):
            dense = k.rsplit(".", 1)[0]
            merged[dense + ".weight"] = params[dense + ".weight"] + torch.tensor(ad[k[:-1] + "b"] @ a, device="cuda:0")
    net.load_state_dict(params)
    x = torch.randn(2, 4, 64, 64, device="cuda:0")
    ctx = torch.randn(2, 77, 768, device="cuda:0")
    net(x, torch.tensor([500.0, 500.0], device="cuda:0"), ctx)
    plans = dict(net._plans)
    wall = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net.load_state_dict(merged)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    kept = bool(plans) and all(net._plans.get(k) is p for k, p in plans.items())
    return dict(step="reload", reps=reps, wall_ms_median=statistics.median(wall), wall_ms_min=min(wall), plans_kept=kept)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reload-reps", type=int, default=3)
    ap.add_argument("--step", choices=["swap", "reload"], help="run one step in this process (used by the parent)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", help="also write the JSON result to this file")
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step_swap(max(a.reps, 20)) if a.step == "swap" else step_reload(a.reload_reps)))
        return 0
    result = {}
    for step in ("swap", "reload"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps), "--reload-reps", str(a.reload_reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"lora_swap_bench: step {step} exceeded {a.timeout} s; stopping", file=sys.stderr)
            return 124
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f"lora_swap_bench: step {step} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode or 1
        result[step] = json.loads(line[-1][len("RESULT "):])
    result["reload_over_swap_wall"] = result["reload"]["wall_ms_median"] / result["swap"]["wall_ms_median"]
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
