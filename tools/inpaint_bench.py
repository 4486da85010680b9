#!/usr/bin/env python3
"""Launch cost of the four kernels around an inpainting run (csrc/inpaint.hip) beside the torch expressions they replace, at the
reference CLI's shape: 4 x 3 x 512 x 512 images, one 512 x 512 mask, a 64 x 64 latent (a sibling of tools/step_bench.py).

  mask_image   image * (mask < 0.5)                                                       | ops.inpaint_mask_image
  concat       cat(F.interpolate(m, 64 x 64, nearest), scale * (mean + exp(0.5 clip(logvar)) * noise)) from the NHWC fp16 moments
                                                                                          | ops.inpaint_concat
  feather      maximum(m, conv2d(conv2d(pad(m, replicate), rows), columns)), sigma 4      | ops.mask_feather
  composite    v = clamp((a * x + (1 - a) * image + 1) / 2, 0, 1) and (v * 255).to(uint8).permute(0, 2, 3, 1).contiguous()
                                                                                          | ops.inpaint_composite(output="both")

Graph-free: every form is enqueued `--launches` times between two hip events on the current stream, `--rounds` times after a
warm-up, the two forms of a kernel alternating.  Reported: median over rounds of (elapsed / launches) in microseconds -- where
the device finishes a form faster than the host enqueues it, that is the host's enqueue time.  One JSON line (and --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def forms(B, H, W, h, w, sigma):
    import torch
    import torch.nn.functional as F
    from minddiffusion_amd import ops
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    image = torch.rand((B, 3, H, W), device=dev, generator=g) * 2 - 1
    x = torch.randn((B, 3, H, W), device=dev, generator=g)
    mask = (torch.rand((1, 1, H, W), device=dev, generator=g) > 0.7).float()
    alpha = torch.rand((1, 1, H, W), device=dev, generator=g)
    mom = torch.randn((B, h * w, 8), device=dev, generator=g).half()
    pn = torch.randn((B, 4, h, w), device=dev, generator=g)
    scale = 0.18215
    radius, wts = ops.feather_weights(sigma)
    wt = torch.from_numpy(wts).to(dev)
    rows, cols = wt.reshape(1, 1, 1, -1), wt.reshape(1, 1, -1, 1)

    def torch_concat():
        m = F.interpolate((mask >= 0.5).float(), size=(h, w), mode="nearest").expand(B, -1, -1, -1)
        nchw = mom[:, :, :8].float().permute(0, 2, 1).reshape(B, 8, h, w)
        z = nchw[:, :4] + torch.exp(0.5 * torch.clamp(nchw[:, 4:], -30.0, 20.0)) * pn
        return torch.cat([m, scale * z], 1)

    def torch_feather():
        m = (mask >= 0.5).float()
        gm = F.conv2d(F.conv2d(F.pad(m, (radius,) * 4, mode="replicate"), rows), cols)
        return torch.maximum(m, gm)

    def torch_composite():
        v = torch.clamp((alpha * x + (1 - alpha) * image + 1.0) / 2.0, 0.0, 1.0)
        return v, (v * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return {
        "mask_image": (lambda: image * (mask < 0.5), lambda: ops.inpaint_mask_image(image, mask)),
        "concat": (torch_concat, lambda: ops.inpaint_concat(mom, 4, pn, scale, mask, (h, w))),
        "feather": (torch_feather, lambda: ops.mask_feather(mask, sigma)),
        "composite": (torch_composite, lambda: ops.inpaint_composite(x, image, alpha, output="both")),
    }


def timed(fn, launches):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("inpaint_bench: needs a GPU")
    res = {"shape": [4, 3, 512, 512], "latent": [64, 64], "sigma": a.sigma, "launches": a.launches, "rounds": a.rounds,
           "graph": False, "kernels": {}}
    for name, (torch_form, fused_form) in forms(4, 512, 512, 64, 64, a.sigma).items():
        for _ in range(a.warmup):
            timed(torch_form, a.launches), timed(fused_form, a.launches)
        us = {"torch": [], "fused": []}
        for _ in range(a.rounds):
            us["torch"].append(timed(torch_form, a.launches))
            us["fused"].append(timed(fused_form, a.launches))
        res["kernels"][name] = {k + s: round(f(v), 2) for k, v in us.items()
                                for s, f in (("_us", statistics.median), ("_us_min", min), ("_us_max", max))}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
