#!/usr/bin/env python3
"""Launch cost of the masked forward-process blend of an img2img step, at the latent shapes the samplers run (a sibling of
tools/step_bench.py, same method).

  torch   the expression PLMSSampler.sample(mask=) evaluates every step (plms.py:153-157 through LatentDiffusion.q_sample):
              img_orig = a * x0 + b * noise;  img = img_orig * mask + (1. - mask) * img
          with a / b already on the device as [B, 1, 1, 1] tensors (the table look-up and the timestep vector of q_sample are
          left out: they cannot be captured, and leaving them out only favours this side)
  fused   ops.q_sample(x0, noise, a, b, out=img, mask=mask, img=img): mdx_q_sample_f32, one launch, in place

One process: `--launches` repetitions of each form are captured into a hipGraph (so the host's enqueue rate is not what is
measured), the two graphs are replayed alternately `--rounds` times after a warm-up, each replay between two hip events.
Reported per step: median over rounds of (replay time / launches).  Prints one JSON line (and writes --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((2, 4, 64, 64), (8, 4, 64, 64), (1, 4, 96, 96))      # 512^2 batch 2, 512^2 batch 8, 768^2 batch 1


def bench_shape(shape, launches, rounds, warmup):
    import torch
    from minddiffusion_amd import ops
    dev = "cuda:0"
    B, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(0)
    r32 = lambda: torch.randn(shape, device=dev, generator=g)
    x0, noise = r32(), r32()
    mask = (torch.rand((B, 1, H, W), device=dev, generator=g) > 0.5).float()
    a, b = 0.8366, 0.5478
    a_t, b_t = torch.full((B, 1, 1, 1), a, device=dev), torch.full((B, 1, 1, 1), b, device=dev)
    state = {"torch": r32(), "fused": None}
    state["fused"] = state["torch"].clone()

    def torch_form():
        img_orig = a_t * x0 + b_t * noise
        state["torch"] = img_orig * mask + (1. - mask) * state["torch"]

    def fused_form():
        ops.q_sample(x0, noise, a, b, out=state["fused"], mask=mask, img=state["fused"])
    entries = {"torch": torch_form, "fused": fused_form}
    graphs = {}
    for name, fn in entries.items():
        fn()
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(launches):
                fn()
    for _ in range(warmup):
        for gr in graphs.values():
            gr.replay()
    torch.cuda.synchronize()
    us = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, gr in graphs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            gr.replay()
            t1.record()
            t1.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / launches)
    res = {"shape": list(shape)}
    for name, v in us.items():
        res[name + "_us"] = round(statistics.median(v), 3)
        res[name + "_us_min"] = round(min(v), 3)
        res[name + "_us_max"] = round(max(v), 3)
    res["fused_minus_torch_us"] = round(res["fused_us"] - res["torch_us"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("q_sample_bench: needs a GPU")
    res = {"launches": a.launches, "rounds": a.rounds,
           "shapes": [bench_shape(s, a.launches, a.rounds, a.warmup) for s in SHAPES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
