#!/usr/bin/env python3
"""What regions and wrap-around windows cost around the UNet: the full-size SD2 UNet, a 64 x 256 latent canvas (a
512 x 2048 panorama) under guidance, so a canvas batch of 2; 64^2 windows at stride 32, the UNet replaying its captured graph.
In one process:

  (a) wrapped    WindowedDiffusion(wrap_x=True).apply_model_nhwc on the canvas -- 8 windows, UNet batch 16 -- against the inner
                 model on a plain [16, 4, 64, 64] batch with the same context rows
  (b) regions    a two-region evaluation on the clamped grid (7 windows) -- the background plus one region over a quarter of the
                 canvas -- against the plain batch of the same row count and the same context rows
  (c) launches   by device events: ops.window_gather_rows and ops.window_average_regions next to ops.window_gather and
                 ops.window_average, re-measured here on the same buffers
  (d) rows       the UNet rows evaluated with the active-pair pruning and without it (every region in every window)

Each pair of (a) and of (b) alternates, `--rounds` times after a warm-up of both (the method of tools/window_bench.py): per
side the median over the rounds of the wall time of `--iters` calls that end in a device synchronise.  One JSON line (and
--out).  No threshold."""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("window_regions_bench: needs the GPU (no timing is taken on a CPU)")
    from minddiffusion_amd import ops
    from minddiffusion_amd.ldm.models.diffusion.windowed import WindowedDiffusion
    dev = "cuda:0"
    if args.config == "sd2":
        import bench
        model, win, T = bench.build_model(dev, "sd2"), 64, 77
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _vpred_util as V
        model, win, T = V.tiny_eps_model()[0], 8, 6
    Hc, Wc = win, 4 * win
    unet = model.unet
    C = int(unet.final_channels)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((1, 4, Hc, Wc), device=dev, generator=g)
    x_in = torch.cat([x, x]).contiguous()
    ctxs = [torch.randn((2, T, unet.context_dim), device=dev, generator=g).half() for _ in range(2)]
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

    def alternate(a, b):
        timed(a), timed(b)
        ms = ([], [])
        for _ in range(args.rounds):
            ms[0].append(timed(a))
            ms[1].append(timed(b))
        ra, rb = side(ms[0]), side(ms[1])
        return {"windowed": ra, "plain_batch": rb, "minus_ms": round(ra["ms_median"] - rb["ms_median"], 4),
                "over": round(ra["ms_median"] / rb["ms_median"], 4)}

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

    stat = lambda v: {"median": round(med(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}

    # ---- (a) a wrapped evaluation: 8 windows, one chunk
    wrapped = WindowedDiffusion(model, (win, win), (win // 2, win // 2), max_unet_batch=16, wrap_x=True)
    call_a = lambda: wrapped.apply_model_nhwc(x_in, t, ctxs[0], temb=temb, cfg_dup=True)
    out_a = call_a()
    torch.cuda.synchronize()
    gw = wrapped.grid
    assert gw.wrap_x and gw.N == 8 and wrapped.chunks == [(0, 8)] and bool(torch.isfinite(out_a).all())
    xa = ops.window_gather_rows(x_in, gw, range(gw.N))
    ta, ctxa = t.repeat_interleave(gw.N), wrapped._context(ctxs[0], gw.N)
    plain_a = lambda: model.apply_model_nhwc(xa, ta, ctxa, temb=temb, cfg_dup=True)
    ea = plain_a().clone()
    torch.cuda.synchronize()
    equal_a = bool(torch.equal(ops.window_average_regions(ea, gw, C), call_a()))
    res_a = dict(alternate(call_a, plain_a), windows=gw.N, unet_batch=2 * gw.N, windowed_equals_average_of_plain=equal_a)

    # ---- (b) two regions on the clamped grid: the background and one region over a quarter of the canvas
    masks = torch.zeros(2, Hc, Wc)
    masks[1, :, Wc // 2:3 * Wc // 4] = 1.0
    masks[0] = 1.0 - masks[1]
    reg = WindowedDiffusion(model, (win, win), (win // 2, win // 2), max_unet_batch=32)
    with reg.regions(masks, ctxs):
        call_b = lambda: reg.apply_model_nhwc(x_in, t, ctxs[0], temb=temb, cfg_dup=True)
        out_b = call_b()
        torch.cuda.synchronize()
        gr, pairs = reg.grid, list(reg.pairs)
        assert len(reg.chunks) == 1 and bool(torch.isfinite(out_b).all())
        P = len(pairs)
        plan = reg._regions["plan"]
        xb = ops.window_gather_rows(x_in, gr, [k for k, _ in pairs])
        tb, ctxb = t.repeat_interleave(P), reg._region_context(ctxs[0], 0, P)
        plain_b = lambda: model.apply_model_nhwc(xb, tb, ctxb, temb=temb, cfg_dup=True)
        eb = plain_b().clone()
        torch.cuda.synchronize()
        equal_b = bool(torch.equal(ops.window_average_regions(eb, gr, C, plan=plan), call_b()))
        res_b = dict(alternate(call_b, plain_b), windows=gr.N, pairs=P, unet_batch=2 * P,
                     windowed_equals_average_of_plain=equal_b)

        # ---- (c) the launches alone, the new ones next to the existing ones on the clamped grid
        xw = ops.window_gather(x_in, gr)
        ew = eb.view(2, P, -1, eb.shape[2])[:, :gr.N].contiguous().view(2 * gr.N, -1, eb.shape[2])
        rows_all, rows_pairs = ops.WindowRows(range(gr.N)), ops.WindowRows([k for k, _ in pairs])
        gat, gat_p = torch.empty_like(xw), torch.empty_like(xb)
        avg = torch.empty_like(out_b)
        us = {"window_gather": [], "window_average": [], "window_gather_rows": [], "window_average_regions_R0": [],
              "window_gather_rows_pairs": [], "window_average_regions_R2": [], "window_gather_rows_wrapped": [],
              "window_average_regions_wrapped": []}
        rows_w, gat_w, avg_w = ops.WindowRows(range(gw.N)), torch.empty_like(xa), torch.empty_like(out_a)
        for _ in range(max(args.rounds, 3)):
            us["window_gather"].append(events(lambda: ops.window_gather(x_in, gr, out=gat)))
            us["window_gather_rows"].append(events(lambda: ops.window_gather_rows(x_in, gr, rows_all, out=gat)))
            us["window_gather_rows_pairs"].append(events(lambda: ops.window_gather_rows(x_in, gr, rows_pairs, out=gat_p)))
            us["window_gather_rows_wrapped"].append(events(lambda: ops.window_gather_rows(x_in, gw, rows_w, out=gat_w)))
            us["window_average"].append(events(lambda: ops.window_average(ew, gr, C, out=avg)))
            us["window_average_regions_R0"].append(events(lambda: ops.window_average_regions(ew, gr, C, out=avg)))
            us["window_average_regions_R2"].append(events(lambda: ops.window_average_regions(eb, gr, C, plan=plan, out=avg)))
            us["window_average_regions_wrapped"].append(events(lambda: ops.window_average_regions(ea, gw, C, out=avg_w)))

    res = {"tool": "window_regions_bench", "config": args.config, "canvas_latent": [2, 4, Hc, Wc], "window": win,
           "stride": win // 2, "rounds": args.rounds, "iters": args.iters, "unet_graph": bool(unet.use_graph),
           "a_wrapped_eval": res_a, "b_two_region_eval": res_b, "c_launch_us": {k: stat(v) for k, v in us.items()},
           "d_unet_rows": {"pruned": 2 * P, "unpruned": 2 * 2 * gr.N, "pairs": [list(p) for p in pairs]}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
