#!/usr/bin/env python3
"""Continuous batching against aligned batches: 16 requests whose step counts alternate between 20 and 50, on the
full-size SD2 UNet at 512 x 512 with 4 samples per UNet batch, DDIM, eta 0, served two ways in one process:

  (a) aligned   four calls of DiffusionPipeline.__call__ with steps=[20, 50, 20, 50]: every batch runs max(steps) iterations and a
                finished request is carried along -- the path as it was
  (b) session   pipe.serve(requests, slots=4): a request enters the lowest free slot on the tick it frees

The two alternate, `--rounds` times after a warm-up of both; reported per side: the UNet evaluations (counted, next to the count
the schedule predicts), the median wall time (host clock around work that ends in a device synchronise), requests per second
and the time per evaluation -- per step of (a), per tick of (b).  A last pass of (b), outside the medians, synchronises after every
tick and gives the median tick with and without an admission in it.  One JSON line (and --out).  No threshold."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [20, 50] * 8
SLOTS = 4
SCALE = 7.5


def expected_evals(steps, slots):
    aligned = sum(max(steps[i:i + slots]) for i in range(0, len(steps), slots))
    free = [0] * slots
    for n in steps:                          # FIFO into the slot that frees first
        free[free.index(min(free))] += n
    return aligned, max(free)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="sd2", choices=["sd2", "tiny"], help="tiny: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("session_bench: needs the GPU (no timing is taken on a CPU)")
    from minddiffusion_amd.pipeline import DiffusionPipeline
    dev = "cuda:0"
    if args.config == "sd2":
        import bench
        model, H = bench.build_model(dev, "sd2"), 512
        steps = STEPS
    else:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _vpred_util as V
        model, H = V.tiny_eps_model()[0], 64
        steps = [2, 4] * 8
    unet = model.unet
    T = 77 if args.config == "sd2" else 6
    g = torch.Generator(device=dev).manual_seed(0)
    c = torch.randn((len(steps), T, unet.context_dim), device=dev, generator=g).half()
    uc = torch.randn((1, T, unet.context_dim), device=dev, generator=g).half().expand(len(steps), -1, -1).contiguous()
    seeds = list(range(100, 100 + len(steps)))
    pipe = DiffusionPipeline(model, "ddim", device=dev)
    evals = {"n": 0}
    real = model.apply_model_nhwc

    def counted(*a, **k):
        evals["n"] += 1
        return real(*a, **k)
    model.apply_model_nhwc = counted

    def aligned():
        out = []
        for i in range(0, len(steps), SLOTS):
            s = slice(i, i + SLOTS)
            out.append(pipe(c=c[s], uc=uc[s], H=H, W=H, steps=steps[s], scale=[SCALE] * SLOTS, seeds=seeds[s]))
        return torch.cat(out)

    requests = [dict(c=c[r], uc=uc[r], steps=steps[r], scale=SCALE, seed=seeds[r]) for r in range(len(steps))]

    def session():
        return pipe.serve(requests, slots=SLOTS, H=H, W=H, output="latent")

    def timed(fn):
        evals["n"] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, evals["n"], out

    want_a, want_b = expected_evals(steps, SLOTS)
    _, n_a, lat_a = timed(aligned)                    # warm-up of both: plans, graphs, code objects
    _, n_b, lat_b = timed(session)
    assert (n_a, n_b) == (want_a, want_b), (n_a, n_b, want_a, want_b)
    assert bool(torch.isfinite(lat_a).all()) and bool(torch.isfinite(lat_b).all())
    # the first four requests start on tick 0 in slots 0..3, the rows they have in the first aligned batch: the same launches on
    # the same rows, so the same bits (the later ones run in other rows than their aligned batch gives them)
    first_batch_equal = bool(torch.equal(lat_a[:SLOTS], lat_b[:SLOTS]))
    wall = {"aligned": [], "session": []}
    for _ in range(args.rounds):
        for name, fn in (("aligned", aligned), ("session", session)):
            wall[name].append(timed(fn)[0])
    # where a tick's time goes: one more session, a synchronise after every tick
    sess = pipe.session(slots=SLOTS, H=H, W=H, context_len=T, max_steps=max(steps))
    for r in requests:
        sess.submit(**r)
    with_adm, without = [], []
    while not sess.scheduler.idle:
        before = sess.admissions
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sess.step()
        torch.cuda.synchronize()
        (with_adm if sess.admissions > before else without).append((time.perf_counter() - t0) * 1e3)
    med = statistics.median
    res = {"tool": "session_bench", "config": args.config, "slots": SLOTS, "steps": steps, "H": H, "rounds": args.rounds,
           "sampler": "ddim", "eta": 0.0}
    for name, n, want in (("aligned", n_a, want_a), ("session", n_b, want_b)):
        w = med(wall[name])
        res[name] = {"unet_evals": n, "unet_evals_expected": want, "wall_s_median": round(w, 4),
                     "wall_s_min": round(min(wall[name]), 4), "wall_s_max": round(max(wall[name]), 4),
                     "requests_per_s": round(len(steps) / w, 3), "ms_per_eval": round(w * 1e3 / n, 4)}
    res["session_over_aligned_ms_per_eval"] = round(res["session"]["ms_per_eval"] / res["aligned"]["ms_per_eval"], 4)
    res["session_over_aligned_requests_per_s"] = round(res["session"]["requests_per_s"] / res["aligned"]["requests_per_s"], 4)
    res["synced_tick_ms"] = {"with_admission_median": round(med(with_adm), 4), "with_admission_ticks": len(with_adm),
                             "without_admission_median": round(med(without), 4), "without_admission_ticks": len(without),
                             "first_tick": round(with_adm[0], 4)}
    res["first_four_requests_bit_equal_in_both"] = first_batch_equal
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
