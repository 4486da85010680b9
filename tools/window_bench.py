#!/usr/bin/env python3
"""What windowed evaluation costs around the UNet: the full-size SD2 UNet, a 64 x 256 latent canvas (a 512 x 2048
panorama) under guidance, so a canvas batch of 2; 64^2 windows at stride 32 -- 7 windows, one chunk, UNet batch 14 -- with the
UNet replaying its captured graph.  In one process:

  (a) windowed   WindowedDiffusion.apply_model_nhwc on the canvas: gather, the batch-14 UNet, average
  (b) plain      the inner model on a [14, 4, 64, 64] batch with the same per-window context: the UNet alone
  (c) launches   ops.window_gather and ops.window_average alone, by device events
  (d) native     for information, a run of its own (--native; with --out it is added to the record that is there): the inner
                 model on the canvas itself, [2, 4, 64, 256] -- its first self-attention runs over 16 384 tokens; an error
                 string if the plan cannot be built

(a) and (b) alternate, `--rounds` times after a warm-up of both (the method of tools/session_bench.py): per side the median over
the rounds of the wall time of `--iters` calls (default 20) that end in a device synchronise.  (a) - (b) is what the window launches, the
timestep rows and the host code of the wrapper add to one evaluation.  One JSON line (and --out).  No threshold."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--config", default="sd2", choices=["sd2", "tiny"], help="tiny: a rehearsal of the tool, not a measurement")
    ap.add_argument("--native", action="store_true", help="measure (d) alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("window_bench: needs the GPU (no timing is taken on a CPU)")
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import MdxError
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    dev = "cuda:0"
    if args.config == "sd2":
        import bench
        model, win, T = bench.build_model(dev, "sd2"), 64, 77
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _vpred_util as V
        model, win, T = V.tiny_eps_model()[0], 8, 6
    canvas = (win, 4 * win)
    unet = model.unet
    wm = WindowedDiffusion(model, (win, win), (win // 2, win // 2))
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((1, 4) + canvas, device=dev, generator=g)
    x_in = torch.cat([x, x]).contiguous()
    ctx = torch.randn((2, T, unet.context_dim), device=dev, generator=g).half()
    t = torch.full((2,), 500.0, device=dev)
    temb = model.time_embedding_table(t[:1])[0]
    med = statistics.median

    side = lambda v: {"ms_median": round(med(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    def write(res):
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")

    if args.native:
        res = {"tool": "window_bench", "config": args.config}
        if args.out and os.path.exists(args.out):
            res = json.loads(open(args.out).read())
        try:
            native = lambda: model.apply_model_nhwc(x_in, t, ctx, temb=temb, cfg_dup=True)
            assert bool(torch.isfinite(native()).all())
            timed(native)
            res["d_native_canvas_eval"] = dict(side([timed(native) for _ in range(args.rounds)]), process="a --native run of its "
                                               "own, added to the record of (a) - (c)", rounds=args.rounds, iters=args.iters)
        except MdxError as err:
            res["d_native_canvas_eval"] = {"error": str(err)[:300]}
        return write(res)

    def windowed():
        return wm.apply_model_nhwc(x_in, t, ctx, temb=temb, cfg_dup=True)

    out = windowed()                                   # warm-up: plans, graphs, code objects, the per-window context
    torch.cuda.synchronize()
    grid, chunks = wm.grid, list(wm.chunks)
    assert grid.N == 7 and chunks == [(0, 7)] and bool(torch.isfinite(out).all())
    xw = ops.window_gather(x_in, grid)                 # [14, 4, win, win]
    tw = t.repeat_interleave(grid.N)
    ctxw = wm._context(ctx, grid.N)                    # the buffer (a) hands the UNet: neither side re-projects it

    def plain():
        return model.apply_model_nhwc(xw, tw, ctxw, temb=temb, cfg_dup=True)

    e = plain().clone()
    torch.cuda.synchronize()
    composed_equal = bool(torch.equal(ops.window_average(e, grid, unet.final_channels), windowed()))

    timed(windowed), timed(plain)
    ms = {"windowed": [], "plain": []}
    for _ in range(args.rounds):
        for name, fn in (("windowed", windowed), ("plain", plain)):
            ms[name].append(timed(fn))

    def events(fn, iters=200):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters       # microseconds per call

    gat_out, avg_out = torch.empty_like(xw), torch.empty_like(out)
    us = {"window_gather": [], "window_average": []}
    for _ in range(max(args.rounds, 3)):
        us["window_gather"].append(events(lambda: ops.window_gather(x_in, grid, out=gat_out)))
        us["window_average"].append(events(lambda: ops.window_average(e, grid, unet.final_channels, out=avg_out)))

    res = {"tool": "window_bench", "config": args.config, "canvas_latent": [2, 4] + list(canvas), "window": win, "stride": win // 2,
           "windows": grid.N, "chunks": chunks, "unet_batch": 2 * grid.N, "rounds": args.rounds, "iters": args.iters,
           "unet_graph": bool(unet.use_graph), "windowed_equals_average_of_plain": composed_equal,
           "a_windowed_eval": side(ms["windowed"]), "b_plain_batch_eval": side(ms["plain"]),
           "c_launch_us": {k: {"median": round(med(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                           for k, v in us.items()}}
    res["a_minus_b_ms"] = round(res["a_windowed_eval"]["ms_median"] - res["b_plain_batch_eval"]["ms_median"], 4)
    res["a_over_b"] = round(res["a_windowed_eval"]["ms_median"] / res["b_plain_batch_eval"]["ms_median"], 4)
    write(res)


if __name__ == "__main__":
    main()
