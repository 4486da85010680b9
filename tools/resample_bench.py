#!/usr/bin/env python3
"""Launch cost of the resampling kernel (csrc/resample.hip), measured as tools/step_bench.py measures the sampler step: one
process, `--launches` launches of each entry captured into a hipGraph (so the host's enqueue rate is not what is measured), the
graphs replayed alternately `--rounds` times after a warm-up, each replay between two hip events; per launch, the median over
rounds of (replay time / launches).

  latent   2x4x64x64 -> 128x128, bicubic -- the enlargement of a hires run at batch 2:
             fused   the one mdx_resample_noised_f32 launch (seeded noise, z0 and xt written)
             three   the launches it replaces: mdx_resample_f32, mdx_randn_f32, mdx_q_sample_f32
  image    1x3x512x512 -> 1024x1024, bicubic and lanczos3 -- the plain resample of the image upscalers

Prints one JSON line and writes profiles/resample_bench.json (--out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from step_bench import time_entries  # noqa: E402


def bench_latent(launches, rounds, warmup):
    import torch
    from minddiffusion_amd import ops
    dev = "cuda:0"
    shape, size = (2, 4, 64, 64), (128, 128)
    x = torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    seeds = ops.seeds_tensor([100, 101], dev)
    oshape = shape[:2] + size
    z0, xt, noise = (torch.empty(oshape, device=dev) for _ in range(3))
    a, b, scale = 0.8366, 0.5478, 1.0

    def three():
        ops.resample(x, size, "bicubic", out=z0)
        ops.randn_seeded(seeds, ops.RNG_ENCODE, 0, oshape[1:], out=noise)
        return ops.q_sample(z0, noise, a, b, out=xt)
    entries = {"fused": lambda: ops.resample_noised(x, size, a, b, scale=scale, seeds=seeds, z0_out=z0, xt_out=xt),
               "three": three, "resample": lambda: ops.resample(x, size, "bicubic", out=z0)}
    res = time_entries(shape, entries, launches, rounds, warmup)
    res["to"] = list(size)
    res["saved_us"] = round(res["three_us"] - res["fused_us"], 3)
    return res


def bench_image(launches, rounds, warmup):
    import torch
    from minddiffusion_amd import ops
    dev = "cuda:0"
    shape, size = (1, 3, 512, 512), (1024, 1024)
    x = torch.rand(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2.0 - 1.0
    out = torch.empty(shape[:2] + size, device=dev)
    entries = {mode: (lambda m=mode: ops.resample(x, size, m, out=out)) for mode in ("nearest", "bicubic", "lanczos3")}
    res = time_entries(shape, entries, launches, rounds, warmup)
    res["to"] = list(size)
    moved = (x.numel() + out.numel()) * 4
    res["bicubic_GBps"] = round(moved / (res["bicubic_us"] * 1e-6) / 1e9, 1)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "resample_bench.py needs a GPU"
    res = {"tool": "resample_bench", "launches": a.launches, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0),
           "latent": bench_latent(a.launches, a.rounds, a.warmup),
           "image": bench_image(max(a.launches // 4, 10), a.rounds, a.warmup)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
