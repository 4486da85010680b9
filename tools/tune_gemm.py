#!/usr/bin/env python
"""Measure the (tile_m, splitk) candidates of every GEMM / conv shape of a UNet plan on the device and write the ones
that beat the cost model (gemm_plan.hip cost_model_tiling) into minddiffusion_amd/csrc/gemm_tuned.inc.

    python tools/tune_gemm.py --model sd2 --batch 2 --latent 64 [--merge] [--out minddiffusion_amd/csrc/gemm_tuned.inc]

Every candidate is timed as it runs inside a UNet evaluation: a 512 MiB fill evicts L2 and the Infinity Cache (cold
weights), then the plan's own two preceding ops run (--insitu: they leave the launch's activations where a real
evaluation finds them), then HIP events bracket the launch (main kernel + split-K reduce); median of --reps.
An entry is written only when the best candidate beats the model's own choice by --gain (default 4 %) and 0.5 us.
"""
import argparse
import ctypes
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# the baseline ("model") is whatever the library picks today: the committed table first, then the cost model --
# so a re-run only adds entries that beat the current choice

NS_CANDIDATES = [1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 20]


def variant(d):
    """Launch variant of a descriptor: gemm_plan.hip tuned_variant()."""
    return ((1 if d.c2 > 0 else 0) | (2048 if d.epilogue == 4 else d.epilogue << 1) | (8 if d.n_split else 0) | (16 if d.ln_stats else 0)
            | (32 if d.stats_out else 0) | (64 if d.out_mode == 1 else 0) | (128 if d.colstats_out else 0)
            | (256 if d.residual else 0) | (512 if d.rowbias else 0) | (1024 if d.out_mode == 2 else 0))


def time_desc(ops, d, flush, reps, pre=()):
    ts = []
    for r in range(reps):
        flush.fill_(r & 1)
        for op in pre:      # the plan's own predecessors: they leave this launch's activations where a real evaluation finds them
            op()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.gemm_run(d)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sd2", choices=["sd2", "wukong", "glide", "vae"])
    ap.add_argument("--batch", type=int, default=2, help="UNet batch (2 x images under CFG)")
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gain", type=float, default=0.04)
    ap.add_argument("--out", default=os.path.join(ROOT, "minddiffusion_amd", "csrc", "gemm_tuned.inc"))
    ap.add_argument("--out160", default=None, help="table of the 128 x 160 tile's rows (default: gemm_tuned160.inc beside --out)")
    ap.add_argument("--merge", action="store_true", help="keep the entries already in --out (other batches / models)")
    ap.add_argument("--log", default=None)
    ap.add_argument("--only-m", type=int, default=0, help="tune only the shapes with this M")
    ap.add_argument("--only-ks", type=int, default=0, help="tune only the shapes with this kernel size")
    ap.add_argument("--only-k", type=int, default=0, help="tune only the shapes with this K (ksize * ksize * Cin)")
    ap.add_argument("--tile160-only", action="store_true",
                    help="dense shapes only, and only the 128 x 160 tile (ring 2 | 3) against the present choice: the A/B of that form")
    ap.add_argument("--insitu", type=int, default=2,
                    help="run this many of the plan's preceding ops between the flush and the timed launch (0 = all cold)")
    args = ap.parse_args()
    import bench
    from minddiffusion_amd import ops
    from minddiffusion_amd._lib import GemmDesc
    dev = torch.device("cuda:0")
    B, h = args.batch, args.latent
    plans = []      # one forward each, so that every activation buffer holds sane values
    if args.model in ("sd2", "wukong"):
        net = bench.build_model(dev, args.model).unet
        ctx = torch.randn(B, 77, net.context_dim, device=dev, dtype=torch.float16)
        net.use_graph = False
        net.forward_nhwc(torch.randn(B, 4, h, h, device=dev), torch.full((B,), 500.0, device=dev), ctx)
        plans.append(net._plan(B, h, h))
    elif args.model == "glide":     # bench.py glide_256: base at UNet batch 2P (64x64), super-res at P (256x256)
        dm, sr = bench.build_glide(dev)
        Pn = bench.CONFIGS["glide_256"]["batch"]
        tok = torch.randint(1, 50000, (2 * Pn, 128), device=dev)
        msk = torch.ones((2 * Pn, 128), dtype=torch.bool, device=dev)
        for m in (dm.model, sr.model):
            m.use_graph = False
        dm.model.forward_nhwc(torch.randn(2 * Pn, 3, 64, 64, device=dev), torch.full((2 * Pn,), 500.0, device=dev), tok, msk)
        plans.append(dm.model._plan(2 * Pn, 64, 64))
        sr.model.forward_nhwc(torch.randn(Pn, 3, 256, 256, device=dev), torch.full((Pn,), 500.0, device=dev), tok[:Pn], msk[:Pn],
                              low_res=torch.randn(Pn, 3, 64, 64, device=dev))
        plans.append(sr.model._plan(Pn, 256, 256))
        B, h = Pn, 256
    else:                           # AutoencoderKL.decode of B latents (bench.py sd2_512_images / _e2e)
        vae = bench.build_vae(dev)
        vae.decode(torch.randn(B, 4, h, h, device=dev))
        plans.append(vae.decoder._plan(B, h, h))
    torch.cuda.synchronize()
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    shapes, pres = {}, {}
    for P in plans:
        for d in P.descs:
            if d.stride != 1 or d.upsample:
                continue
            M, N, K = d.B * d.H * d.W, d.N, d.ksize * d.ksize * (d.c1 + d.c2)
            shapes.setdefault((M, N, K, d.ksize, variant(d)), d)
        if args.insitu > 0:     # first op of the plan that issues each shape (closures carry their descriptor as a default)
            for i, fn in enumerate(P.main):
                dd = (getattr(fn, "__defaults__", None) or (None,))[0]
                if isinstance(dd, GemmDesc) and dd.stride == 1 and not dd.upsample:
                    key = (dd.B * dd.H * dd.W, dd.N, dd.ksize * dd.ksize * (dd.c1 + dd.c2), dd.ksize, variant(dd))
                    if key not in pres:
                        pres[key] = list(P.main[max(0, i - args.insitu):i])
                        shapes[key] = dd
    big_ws = ops.new_gemm_workspace(256 << 20, dev)
    # GEGLU weights are packed for ONE tile width (mdx_gemm_desc.geglu_unit): a candidate on the other width gets its own packing of
    # the plan's w / bias / S[n] (row permutations, cached per weight)
    ptr2t = {}
    if args.model in ("sd2", "wukong"):
        ptr2t = {t.data_ptr(): t for t in list(net.w.values()) + list(net._geglu80.values())}
    repacked = {}

    def set_geglu_unit(d, d0, unit):
        have = 80 if d0.geglu_unit == 80 else 64
        if unit == have:
            return True
        if d0.w not in ptr2t or (d0.bias and d0.bias not in ptr2t) or (d0.ln_s and d0.ln_s not in ptr2t):
            return False
        key = (d0.w, unit)
        if key not in repacked:
            N_, K_ = d0.N, d0.c1 + d0.c2
            w2 = ops.pack_gemm_weight(ops.geglu_repack(ops.unpack_gemm_weight(ptr2t[d0.w], N_, K_), have, unit))
            repacked[key] = (w2, ops.geglu_repack(ptr2t[d0.bias], have, unit) if d0.bias else None,
                             ops.geglu_repack(ptr2t[d0.ln_s], have, unit) if d0.ln_s else None)
        w2, b2, s2 = repacked[key]
        d.w, d.geglu_unit = w2.data_ptr(), (80 if unit == 80 else 0)
        if b2 is not None:
            d.bias = b2.data_ptr()
        if s2 is not None:
            d.ln_s = s2.data_ptr()
        return True
    lines, log = [], []
    for (M, N, K, ks, var), d0 in sorted(shapes.items()):
        if (args.only_m and M != args.only_m) or (args.only_ks and ks != args.only_ks) or (args.only_k and K != args.only_k):
            continue
        if d0.xattn_k:      # a query projection that carries its cross-attention: the planner fixes its tiles (one head per 64-column tile)
            continue
        kt = (K + 63) // 64
        halo = ks == 3 and d0.c2 == 0 and (d0.c1 % 64 == 0) and d0.W % 16 == 0 and d0.H % 8 == 0
        halo8 = ks == 3 and d0.c2 == 0 and (d0.c1 % 64 == 0) and d0.W == 8 and d0.H == 8   # bm = 128: HALO, bm = 64: generic

        def cand(bm, ns, bn=0, st=0):
            d = GemmDesc.from_buffer_copy(d0)
            d.tile_m, d.splitk, d.tile_n, d.stages = bm, ns, bn, st
            d.defer_reduce = 0      # time the launch with its own reduce
            if d.colstats_out:      # the plan's buffer is sized for the plan's row blocks: candidates get one that fits 64-row blocks
                d.colstats_out, d.colstats_cap = cs_scratch.data_ptr(), (M + 63) // 64
            d.workspace, d.workspace_bytes = big_ws.data_ptr(), big_ws.numel() * 4
            if d.epilogue == ops.EPI_GEGLU and bn and not set_geglu_unit(d, d0, 80 if bn == 160 else 64):
                raise RuntimeError("no tensors to repack the GEGLU weights from")
            return d
        pre = pres.get((M, N, K, ks, var), ())
        cs_scratch = torch.empty(((M + 63) // 64) * N * 2 + 16, dtype=torch.float32, device=dev) if d0.colstats_out else None
        auto = cand(0, 0)
        t_auto = time_desc(ops, auto, flush, args.reps, pre)
        best = (t_auto, 0, 0, 0, 0)
        bns = [128] if d0.epilogue == ops.EPI_GEGLU else ([64] if N < 128 else [128, 64])
        halo256 = halo and d0.H % 16 == 0
        # 8x8 images take the two-samples-per-tile HALO kernel whenever they are eligible (gemm_plan.hip lookup_tuned drops 64-row
        # rows for them), so 64-row generic tiles are not candidates there
        # the 128 x 160 tile of the lean dense kernel (four waves 4 x 1): every dense shape is offered it, unsplit, ring 2 | 3; the
        # library refuses the variants its epilogue does not carry (statistics, split stores, fused norms ...)
        if ks == 1 and d0.c2 == 0 and N >= 160:
            for st in (2, 3):
                try:
                    t = time_desc(ops, cand(128, 1, 160, st), flush, args.reps, pre)
                except Exception as e:
                    log.append(f"  skip M={M} N={N} K={K} bm=128 bn=160 ns=1 st={st}: {e}")
                    continue
                log.append(f"  M={M} N={N} K={K} v{var}: 128 x 160 ring {st}: {t:7.2f} us (present choice {t_auto:7.2f} us)")
                if t < best[0]:
                    best = (t, 128, 1, 160, st)
        elif args.tile160_only:
            continue
        for bm in (([128, 256] if halo256 else [128]) if (halo or halo8) else [128, 64]):
            if args.tile160_only:
                break
            for bn in bns:
                for ns in NS_CANDIDATES:
                    if ns > 1 and (kt // ns < 2 or ns * M * N * 4 > big_ws.numel() * 4):
                        continue
                    if (halo or (halo8 and bm == 128)) and ns > (d0.c1 // 64):
                        continue
                    # depth of the LDS ring; 10 | 11 = the same depths with eight waves per block (generic 128-row tiles)
                    generic = not halo and not (halo8 and bm == 128)
                    for st in (((2, 3, 4, 10, 11) if bm == 128 else (2, 3, 4, 5, 6)) if generic else (2, 3, 4)):
                        try:
                            t = time_desc(ops, cand(bm, ns, bn, st), flush, args.reps, pre)
                        except Exception as e:      # unsupported combination
                            log.append(f"  skip M={M} N={N} K={K} bm={bm} bn={bn} ns={ns} st={st}: {e}")
                            continue
                        if t < best[0]:
                            best = (t, bm, ns, bn, st)
        t_auto2 = time_desc(ops, auto, flush, args.reps, pre)     # re-measure the baseline: drift guard
        t_ref = min(t_auto, t_auto2)
        keep = best[1] and best[0] < t_ref * (1 - args.gain) and best[0] < t_ref - 0.5
        msg = (f"M={M:6d} N={N:6d} K={K:6d} k{ks} v{var:<4d} halo={int(halo)}: model {t_ref:7.2f} us | best bm={best[1]:3d} bn={best[3]:3d} ns={best[2]:2d} "
               f"st={best[4]} {best[0]:7.2f} us {'KEEP' if keep else ''}")
        print(msg, flush=True)
        log.append(msg)
        if keep:
            lines.append((M, N, K, ks, best[1], best[3], best[2], t_ref, best[0], var, best[4]))
    # Rows of the 128 x 160 tile go to a table of their own (gemm_tuned160.inc, consulted first by gemm_plan.hip lookup_tuned): the shape's
    # row in the main table stays and serves the descriptors that tile does not carry (GEGLU weights packed at 64 ...)
    lines160 = [l for l in lines if l[5] == 160]
    lines = [l for l in lines if l[5] != 160]
    out160 = args.out160 or os.path.join(os.path.dirname(args.out), "gemm_tuned160.inc")
    old160 = []
    if args.merge and os.path.exists(out160):
        for ln in open(out160):
            m = re.match(r"\s*\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\},", ln)
            if m and tuple(int(m.group(i)) for i in (1, 2, 3, 4, 8)) not in {l[:4] + (l[9] + 1,) for l in lines160}:
                old160.append(ln.rstrip("\n"))
    if lines160 or not args.merge:
        with open(out160, "w") as f:
            f.write("// generated by tools/tune_gemm.py -- rows of the 128 x 160 tile of the lean dense kernel, fields as in gemm_tuned.inc: "
                    "measured on MI355X, cold weights\n")
            for ln in old160:
                f.write(ln + "\n")
            for M, N, K, ks, bm, bn, ns, t0, t1, var, st in lines160:
                f.write(f"    {{{M}, {N}, {K}, {ks}, {bm}, {bn}, {ns}, {var + 1}, {st}}},   // {args.model} B={B} latent={h}: {t0:.1f} -> {t1:.1f} us\n")
        print(f"{len(lines160)} rows of the 128 x 160 tile written to {out160} ({len(old160)} kept)")
    if args.tile160_only:
        return
    old = []
    if args.merge and os.path.exists(args.out):
        for ln in open(args.out):
            m = re.match(r"\s*\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)(?:, (\d+))?(?:, \d+)?\},(.*)", ln)
            if m:
                key = (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(8) or 0))
                if key not in {l[:4] + (l[9] + 1,) for l in lines}:
                    old.append(ln.rstrip("\n"))
    with open(args.out, "w") as f:
        f.write("// generated by tools/tune_gemm.py -- {M, N, K, ksize, tile_m, tile_n (0 = default), splitk[, launch variant + 1[, LDS ring depth (0 = rule)]]}: measured on MI355X, cold weights\n")
        for ln in old:
            f.write(ln + "\n")
        for M, N, K, ks, bm, bn, ns, t0, t1, var, st in lines:
            f.write(f"    {{{M}, {N}, {K}, {ks}, {bm}, {bn}, {ns}, {var + 1}, {st}}},   // {args.model} B={B} latent={h}: {t0:.1f} -> {t1:.1f} us\n")
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(log) + "\n")
    print(f"{len(lines)} entries written to {args.out} ({len(old)} kept)")


if __name__ == "__main__":
    main()
