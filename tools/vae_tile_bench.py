#!/usr/bin/env python3
"""What the tiled VAE costs against the global one: the full-size SD VAE on a 64 x 256 latent (a 512 x 2048
panorama), batch 1, tile 64, overlap 16 -- 5 tiles (offsets 0 48 96 144 192), one chunk of max_tile_batch 8.  In one process:

  (a) decode   global AutoencoderKL.decode against the tiled one (gather, one batch-8 decoder call, one blend launch),
               alternating, `--rounds` times after a warm-up of both: per side the median over the rounds of the wall time of
               `--iters` calls that end in a device synchronise
  (b) encode   the same for encode(sample=False) of the 512 x 2048 image
  (c) blend    ops.tile_blend alone on the decode's image grid: `--blend-launches` launches captured into one graph, the graph
               replayed; device events around the replays, microseconds per launch
  (d) plans    activation_bytes of the plans involved, and how many decoder plans each VAE holds after decoding three canvas
               sizes (64 x 256, 64 x 128, 128 x 128)

One JSON line (and --out).  Reported, not gated: no threshold."""
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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--blend-launches", type=int, default=50)
    ap.add_argument("--config", default="sd", choices=["sd", "tiny"], help="tiny: a rehearsal of the tool, not a measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("vae_tile_bench: needs the GPU (no timing is taken on a CPU)")
    from minddiffusion_amd import ops
    dev = "cuda:0"
    if args.config == "sd":
        import bench
        build, tile, overlap = (lambda: bench.build_vae(dev)), 64, 16
    else:
        from minddiffusion_amd.configs import TINY_VAE_DDCONFIG
        from minddiffusion_amd.ldm.models.autoencoder import AutoencoderKL
        from oracle import vae as OV

        def build():
            vae = AutoencoderKL(ddconfig=dict(TINY_VAE_DDCONFIG), embed_dim=4, device=dev)
            vae.load_state_dict(OV.init_params(dict(TINY_VAE_DDCONFIG), seed=0))
            return vae
        tile, overlap = 16, 4
    plain, tiled = build(), build().enable_tiling(tile=tile, overlap=overlap, max_tile_batch=8)
    f = plain.factor
    canvases = [(tile, 4 * tile), (tile, 2 * tile), (2 * tile, 2 * tile)]
    g = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn((1, 4) + canvases[0], device=dev, generator=g)
    x = torch.rand((1, 3, f * canvases[0][0], f * canvases[0][1]), device=dev, generator=g) * 2.0 - 1.0
    med = statistics.median
    side = lambda v: {"ms_median": round(med(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.iters

    def pair(global_fn, tiled_fn):
        timed(global_fn), timed(tiled_fn)                    # warm-up: plans, graphs, code objects
        ms = {"global": [], "tiled": []}
        for _ in range(args.rounds):
            ms["global"].append(timed(global_fn))
            ms["tiled"].append(timed(tiled_fn))
        out = {k: side(v) for k, v in ms.items()}
        out["tiled_over_global"] = round(out["tiled"]["ms_median"] / out["global"]["ms_median"], 4)
        return out

    def distance(a, b):
        return round(float((a - b).norm() / b.norm()), 5)

    res = {"tool": "vae_tile_bench", "config": args.config, "latent": [1, 4] + list(canvases[0]), "tile": tile, "overlap": overlap,
           "max_tile_batch": 8, "rounds": args.rounds, "iters": args.iters}
    res["decode_rel_l2_tiled_vs_global"] = distance(tiled.decode(z), plain.decode(z))
    res["encode_rel_l2_tiled_vs_global"] = distance(tiled.encode(x, sample=False), plain.encode(x, sample=False))
    res["a_decode"] = pair(lambda: plain.decode(z), lambda: tiled.decode(z))
    res["b_encode"] = pair(lambda: plain.encode(x, sample=False), lambda: tiled.encode(x, sample=False))

    # (c) the blend launch alone, replayed from a captured graph
    t = tiled._tiles_for(canvases[0][0], canvases[0][1], False)
    img = t["img"]
    res["tiles"] = img.N
    tiles = torch.randn((img.N, 3, img.h, img.w), device=dev, generator=g)
    out = torch.empty((1, 3, img.Hc, img.Wc), device=dev)
    blend = lambda: ops.tile_blend(tiles, img, t["ramp_img"], out=out, mode="unit")
    blend()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.blend_launches):
            blend()
    us = []
    for _ in range(max(args.rounds, 3)):
        graph.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / (4 * args.blend_launches))
    moved = (tiles.numel() + out.numel()) * 4
    res["c_blend_us"] = {"median": round(med(us), 3), "min": round(min(us), 3), "max": round(max(us), 3),
                         "launches_per_graph": args.blend_launches, "bytes_read_and_written": moved,
                         "gbytes_per_s_at_median": round(moved / med(us) * 1e-3, 1)}

    # (d) plans
    for hw in canvases[1:]:
        zz = torch.randn((1, 4) + hw, device=dev, generator=g)
        plain.decode(zz), tiled.decode(zz)
    torch.cuda.synchronize()
    plans = lambda net: {"x".join(map(str, k)): int(p.activation_bytes) for k, p in net._plans.items()}
    res["d_plans"] = {"canvases_decoded": [list(c) for c in canvases],
                      "global_decoder_plans": len(plain.decoder._plans), "tiled_decoder_plans": len(tiled.decoder._plans),
                      "global_decoder_activation_bytes": plans(plain.decoder), "tiled_decoder_activation_bytes": plans(tiled.decoder),
                      "global_encoder_activation_bytes": plans(plain.encoder), "tiled_encoder_activation_bytes": plans(tiled.encoder)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
