#!/usr/bin/env python3
"""Continuous batching against aligned batches: 16 requests whose step counts alternate between 20 and 50, on the
full-size SD2 UNet at 512 x 512 with 4 samples per UNet batch, DDIM, eta 0, served two ways in one process:

  (a) aligned   four calls of DiffusionPipeline.__call__ with steps=[20, 50, 20, 50]: every batch runs max(steps) iterations and a
                finished request is carried along -- the path as it was
  (b) session   pipe.serve(requests, slots=4): a request enters the lowest free slot on the tick it frees

The two alternate, `--rounds` times after a warm-up of both; reported per side: the UNet evaluations (counted, next to the count
the schedule predicts), the median wall time (host clock around work that ends in a device synchronise), requests per second
and the time per evaluation -- per step of (a), per tick of (b).  A last pass of (b), outside the medians, synchronises after every
tick and gives the median tick with and without an admission in it.  One JSON line (and --out).  No threshold.

--mix (the default run is untouched): the same 16 requests, but half of them are img2img requests at strength 0.6 (init_latent=;
they hold their slot for int(0.6 * steps) ticks) and half of those carry a keep_mask, through `pipe.serve`.  Reported: the wall time
and requests per second of the mixed list; the median synchronised tick of a PLAIN session -- the launches of a session as it was
before img2img requests existed -- next to the median tick of the mixed session with and without a blending slot (ticks with an
admission aside); and the blend launch alone (ops.slot_blend, every slot blending) against the two launches it replaces
(ops.randn_slots(RNG_BLEND) then ops.q_sample(mask=)) at the session's latent shape, by device events, alternating."""
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


STRENGTH = 0.6


def mix(args, torch, pipe, requests, steps, H, T, timed):
    """The --mix measurements (module docstring).  Requests 2, 3, 6, 7, ... are img2img; of those every other pair member keeps
    a mask: both step counts appear with and without one."""
    from minddiffusion_amd import ops
    dev, med = pipe.device, statistics.median
    shape = (4, H // 8, H // 8)
    g = torch.Generator(device=dev).manual_seed(1)
    img2img = [r for r in range(len(steps)) if (r // 2) % 2 == 1]
    masked = [r for k, r in enumerate(img2img) if k % 4 in (0, 3)]
    mixed = []
    for r, q in enumerate(requests):
        q = dict(q)
        if r in img2img:
            q.update(init_latent=torch.randn(shape, device=dev, generator=g), strength=STRENGTH)
        if r in masked:
            q.update(keep_mask=(torch.rand((1,) + shape[1:], device=dev, generator=g) > 0.5).float())
        mixed.append(q)
    ticks = [int(STRENGTH * n) if r in img2img else n for r, n in enumerate(steps)]
    want = expected_evals(ticks, SLOTS)[1]
    serve = lambda: pipe.serve(mixed, slots=SLOTS, H=H, W=H, output="latent")
    _, n, lat = timed(serve)                           # warm-up: plans, graphs, code objects
    assert n == want == pipe.last_session.tick_count, (n, want)
    assert bool(torch.isfinite(lat).all()) and pipe.last_session.blend_launches > 0
    wall = [timed(serve)[0] for _ in range(args.rounds)]

    def synced_ticks(reqs):
        """One session, a synchronise after every tick: {(admission in it, a blending slot in it): [ms]}."""
        sess = pipe.session(slots=SLOTS, H=H, W=H, context_len=T, max_steps=max(steps))
        for q in reqs:
            sess.submit(**q)
        out = {}
        while not sess.scheduler.idle:
            adm, bl = sess.admissions, sess.blend_launches
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sess.step()
            torch.cuda.synchronize()
            out.setdefault((sess.admissions > adm, sess.blend_launches > bl), []).append((time.perf_counter() - t0) * 1e3)
        return out

    plain, mixed_t = {}, {}
    for measured in (False, True):                      # alternating; the first pass of each only warms its launches
        for acc, reqs in ((plain, requests), (mixed_t, mixed)):
            got = synced_ticks(reqs)
            if measured:
                acc.update(got)
    tick = lambda acc, k: {"median_ms": round(med(acc[k]), 4), "ticks": len(acc[k])} if acc.get(k) else None

    # the blend launch alone, every slot active and blending, against the two launches it replaces
    B, cap = SLOTS, 4
    z = lambda *s: torch.randn(s, device=dev, generator=g)
    x0, img_a, img_b, noise = z(B, *shape), z(B, *shape), z(B, *shape), torch.empty((B,) + shape, device=dev)
    keep = (torch.rand((B,) + shape, device=dev, generator=g) > 0.5).float()
    seeds = ops.seeds_tensor(list(range(B)), dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    start, length, on = i32([0] * B), i32([cap] * B), i32([1] * B)
    ab = torch.tensor([[[0.8, 0.6]] * cap] * B, device=dev)

    def one():
        ops.slot_blend(x0, keep, img_a, seeds, ops.RNG_BLEND, 0, ab, on, start, length, 1)

    def two():
        ops.randn_slots(seeds, ops.RNG_BLEND, 0, start, length, 1, noise)
        ops.q_sample(x0, noise, 0.8, 0.6, out=img_b, mask=keep, img=img_b)

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

    us = {"slot_blend": [], "randn_slots_then_q_sample": []}
    for _ in range(max(args.rounds, 3)):
        us["slot_blend"].append(events(one))
        us["randn_slots_then_q_sample"].append(events(two))
    w = med(wall)
    res = {"tool": "session_bench", "mode": "mix", "config": args.config, "slots": SLOTS, "steps": steps, "ticks": ticks, "H": H,
           "rounds": args.rounds, "sampler": "ddim", "eta": 0.0, "strength": STRENGTH, "img2img_requests": img2img,
           "keep_mask_requests": masked,
           "serve_mixed": {"unet_evals": n, "unet_evals_expected": want, "blend_launches": pipe.last_session.blend_launches,
                           "wall_s_median": round(w, 4), "wall_s_min": round(min(wall), 4), "wall_s_max": round(max(wall), 4),
                           "requests_per_s": round(len(steps) / w, 3), "ms_per_tick": round(w * 1e3 / n, 4)},
           "synced_tick_ms": {"plain_session_no_admission": tick(plain, (False, False)),
                              "mixed_session_no_admission_no_blend": tick(mixed_t, (False, False)),
                              "mixed_session_no_admission_blend": tick(mixed_t, (False, True)),
                              "mixed_session_admission": {"median_ms": round(med(mixed_t.get((True, False), [])
                                                                                   + mixed_t.get((True, True), [])), 4)}},
           "blend_launch_us": {k: {"median": round(med(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                               for k, v in us.items()},
           "blend_launch_shape": [B] + list(shape)}
    a, b = res["blend_launch_us"]["slot_blend"]["median"], res["blend_launch_us"]["randn_slots_then_q_sample"]["median"]
    res["blend_launch_us"]["one_over_two"] = round(a / b, 4)
    p, m = res["synced_tick_ms"]["plain_session_no_admission"], res["synced_tick_ms"]["mixed_session_no_admission_blend"]
    if p and m:
        res["synced_tick_ms"]["blend_tick_over_plain_tick"] = round(m["median_ms"] / p["median_ms"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="sd2", choices=["sd2", "tiny"], help="tiny: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=None)
    ap.add_argument("--mix", action="store_true", help="img2img and masked-blend requests in the list (see above)")
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

    if args.mix:
        res = mix(args, torch, pipe, requests, steps, H, T, timed)
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return

    want_a, want_b = expected_evals(steps, SLOTS)
    _, n_a, lat_a = timed(aligned)                   # warm-up of both: plans, graphs, code objects
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
