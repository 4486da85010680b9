"""SRGAN post-upscaler throughput: SRGAN.sr_handle (the Generator's graph + the copy out of its plan buffer) at the Taichu-GLIDE CLI's shape (pics_generated = 8 images of 256^2, x4).
Synthetic weights (the timing does not depend on them).  Warm-up, then device-event timing over >= 1 s of back-to-back calls.

    python tools/srgan_bench.py [--factor 4] [--batch 8] [--size 256]

Useful FLOPs per image (srgan.py:75-117, H x W input, f = 2^L):
    conv_in   2 H W 64 243            trunk + conv2   33 x 2 H W 64 576
    sub-pixel j (0-based)  2 (4^j H W) 256 576        conv_out  2 (f^2 H W) 3 5184
HBM bytes from shapes: one read and one write of every tensor the plan stores (fp16 NHWC activations, fp32 image in / out)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def flops_per_image(H, W, f):
    L = {2: 1, 4: 2, 8: 3}[f]
    fl = 2 * H * W * 64 * 243 + 33 * 2 * H * W * 64 * 576
    fl += sum(2 * (4 ** j) * H * W * 256 * 576 for j in range(L))
    fl += 2 * f * f * H * W * 3 * 5184
    return fl


def hbm_bytes(B, H, W, f):
    L = {2: 1, 4: 2, 8: 3}[f]
    act = B * H * W * 64 * 2                              # one 64-channel fp16 tensor at the input resolution
    # conv_in: read image, write c1; 33 trunk / conv2 convs: read input (+ residual on 17 of them), write output
    b = B * 3 * H * W * 4 + act
    b += 33 * 2 * act + 17 * act
    for j in range(L):                                    # read 4^j act, write 4^(j+1) act
        b += (4 ** j) * act + (4 ** (j + 1)) * act
    b += (4 ** L) * act + B * 3 * f * f * H * W * 4       # conv_out: read the last tensor, write the fp32 image
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factor", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    a = ap.parse_args()
    import numpy as np
    import torch
    from minddiffusion_amd.glide.model import srgan_util
    from minddiffusion_amd.glide.model.srgan import Generator

    rng = np.random.RandomState(0)
    shapes = Generator(a.factor, device="cpu").parameter_shapes()
    params = {}
    for k, shp in shapes.items():
        if k.endswith(".moving_variance") or k.endswith(".gamma"):
            params[k] = rng.uniform(0.5, 1.5, shp).astype(np.float32)
        else:
            params[k] = (rng.standard_normal(shp) * 0.05).astype(np.float32)
    sr = srgan_util.SRGAN(a.factor, params=params, device="cuda:0")
    x = torch.rand((a.batch, 3, a.size, a.size), device="cuda:0") * 2 - 1
    for _ in range(3):
        sr.sr_handle(x)
    torch.cuda.synchronize()
    n = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            sr.sr_handle(x)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= a.min_seconds * 1e3:
            break
        n = max(n * 2, int(n * a.min_seconds * 1e3 / max(ms, 1e-3) * 1.2))
    per = ms / n
    fl = flops_per_image(a.size, a.size, a.factor) * a.batch
    by = hbm_bytes(a.batch, a.size, a.size, a.factor)
    P = sr.net._plan(a.batch, a.size, a.size)
    res = {"tool": "srgan_bench", "factor": a.factor, "batch": a.batch, "size": a.size, "calls": n, "ms_per_batch": round(per, 3),
           "images_per_s": round(a.batch / per * 1e3, 2), "useful_tflop_per_batch": round(fl / 1e12, 4),
           "useful_tf_per_s": round(fl / per / 1e9, 1), "hbm_gb_per_batch": round(by / 1e9, 3),
           "hbm_tb_per_s": round(by / per / 1e9, 3), "activation_gb": round(P.activation_bytes / 1e9, 3),
           "launches": len(P.main), "time": time.strftime("%Y-%m-%d %H:%M:%S")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
