#!/usr/bin/env python3
"""Launch cost of the fused sampler step with and without guidance rescale, at the latent shapes the samplers run.

  pred     mdx_sampler_step_pred_f32      (MDX_PRED_V, guidance on): the flat grid-stride kernel
  rescale  mdx_sampler_step_rescale_f32   (same arguments, guidance_rescale = 0.7): one workgroup per sample, statistics pass
           in front of the update

Both in the steady state of a PLMS run (order 3: three eps histories read, e_t / pred_x0 / x_prev written).  One process:
`--launches` launches of each entry are captured into a hipGraph (so the host's enqueue rate is not what is measured), the two
graphs are replayed alternately `--rounds` times after a warm-up, each replay between two hip events.  Reported per launch:
median over rounds of (replay time / launches), and rescale - pred, which is what a step gains by turning the rescale on.

--noise measures, the same way, what a stochastic step (eta > 0) spends on its noise tensor in front of the step launch:
  torch_t / torch_td    the torch sequence of the samplers without seeds: randn, * temperature (t), and with noise_dropout
                        rand, >=, cast, * keep, / (1 - p) on top (td): 2 and 7 launches
  seeded_t / seeded_td  the one mdx_randn_f32 launch of ops.randn_seeded(scale=temperature[, dropout=p])
--table measures the table-driven entry beside the scalar entries it stands in for, the same way and in the same process:
  table / table_rescale  mdx_sampler_step_table_f32 with any_rescale 0 / 1 on rows that repeat the scalar calls' arguments
                         (any_rescale 1: every row rescales, as in the scalar rescale launch)
--lin measures the DPM-Solver step launch (mdx_sampler_step_lin_f32, a third-order update) the same way beside pred / rescale:
  lin / lin_rescale                       the spread form / the owned form with guidance_rescale = 0.7
  lin_threshold / lin_rescale_threshold   the owned form with dynamic thresholding (the radix select), without / with rescale
  select_us = lin_rescale_threshold - lin_rescale: what the selection and the second pass over the sample cost
--sde measures the stochastic DPM-Solver step (mdx_sampler_step_lin_noise_f32, a 2M-SDE record: one stored model value read) the
same way, in the spread form and (`_rescale`) the owned form with guidance_rescale = 0.7:
  lin / lin_rescale                    mdx_sampler_step_lin_f32 alone, the deterministic record's launch
  seeded / seeded_rescale              the noise drawn inside the launch from per-sample seeds
  tensor / tensor_rescale              the noise read from a tensor (no launch for the tensor counted)
  three / three_rescale                the three launches the seeded launch replaces: ops.randn_seeded, the lin launch, an axpy
  draw_us = seeded - lin: what drawing inside the launch costs; saved_us = three - seeded
--pc measures the UniPC step launch (mdx_sampler_step_pc_f32, an order-3 record: corrector and next predictor) the same way
beside the DPM-Solver step launch of the same order, in the spread form and (`_rescale`) the owned form:
  lin / lin_rescale, pc / pc_rescale, and pc - lin per form
Prints one JSON line (and writes --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 4, 96, 96), (2, 4, 64, 64), (8, 4, 64, 64))      # 768^2 batch 1, 512^2 batch 2, 512^2 batch 8


def bench_shape(shape, launches, rounds, warmup):
    import torch
    from minddiffusion_amd import ops
    dev = "cuda:0"
    B, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(0)
    r32 = lambda: torch.randn(shape, device=dev, generator=g)
    x, olds = r32(), [r32(), r32(), r32()]
    out = torch.randn((2 * B, H * W, 8), device=dev, generator=g).half()       # [uncond; cond], NHWC, ld = 8
    out_u, out_c = out[:B], out[B:]
    e_out, x_prev, p_out = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    coef = (55 / 24, -59 / 24, 37 / 24, -9 / 24)
    args = (x, None, out_u, out_c, 8, 7.5, ops.PRED_V, 0.8, 0.6, olds, coef, 0.55, 0.83, 0.6, 0.8, 0.0, None, e_out, x_prev,
            p_out)
    entries = {"pred": lambda: ops.sampler_step_pred(*args), "rescale": lambda: ops.sampler_step_rescale(*args, 0.7)}
    res = time_entries(shape, entries, launches, rounds, warmup)
    res["extra_us"] = round(res["rescale_us"] - res["pred_us"], 3)
    return res


def bench_table(shape, launches, rounds, warmup):
    import numpy as np
    import torch
    from minddiffusion_amd import ops
    dev = "cuda:0"
    B, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(0)
    r32 = lambda: torch.randn(shape, device=dev, generator=g)
    x, olds = r32(), [r32(), r32(), r32()]
    out = torch.randn((2 * B, H * W, 8), device=dev, generator=g).half()
    out_u, out_c = out[:B], out[B:]
    e_out, x_prev, p_out = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    coef = (55 / 24, -59 / 24, 37 / 24, -9 / 24)
    args = (x, None, out_u, out_c, 8, 7.5, ops.PRED_V, 0.8, 0.6, olds, coef, 0.55, 0.83, 0.6, 0.8, 0.0, None, e_out, x_prev,
            p_out)
    row = np.zeros(ops.STEP_ROW, np.float32)
    row[:ops.STEP_SIGMA + 1] = (1.0, 7.5, 0.0, 0.8, 0.6) + coef + (0.55, 0.83, 0.6, 0.8, 0.0)
    plain = torch.tensor(np.tile(row, (B, 1)), device=dev)
    row[ops.STEP_RESCALE] = 0.7
    rescaled = torch.tensor(np.tile(row, (B, 1)), device=dev)
    table = lambda t, any_rescale: ops.sampler_step_table(x, None, out_u, out_c, ops.PRED_V, olds, None, e_out, x_prev, p_out,
                                                          t, any_rescale)
    entries = {"pred": lambda: ops.sampler_step_pred(*args), "table": lambda: table(plain, 0),
               "rescale": lambda: ops.sampler_step_rescale(*args, 0.7), "table_rescale": lambda: table(rescaled, 1)}
    res = time_entries(shape, entries, launches, rounds, warmup)
    res["table_minus_pred_us"] = round(res["table_us"] - res["pred_us"], 3)
    res["table_rescale_minus_rescale_us"] = round(res["table_rescale_us"] - res["rescale_us"], 3)
    return res


def bench_lin(shape, launches, rounds, warmup):
    """The DPM-Solver step launch beside the step it generalises: a third-order update (two stored model values read; the
    model value and x_out written) on a v model with guidance."""
    import torch
    from minddiffusion_amd import ops
    dev = "cuda:0"
    B, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(0)
    r32 = lambda: torch.randn(shape, device=dev, generator=g)
    x, h1, h2 = r32(), r32(), r32()
    out = torch.randn((2 * B, H * W, 8), device=dev, generator=g).half()
    out_u, out_c = out[:B], out[B:]
    m_out, x_out, p_out = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    args = (x, None, out_u, out_c, 8, 7.5, ops.PRED_V, 0.8, 0.6, [], (1., 0., 0., 0.), 0.8, 0.6, 0.9, 0.5, 0.1, h1, None, x_out, p_out)

    def lin(phi, thresholding):
        ops.sampler_step_lin(x, None, out_u, out_c, 7.5, ops.PRED_V, phi, ops.VALUE_X0, 0.8, 0.6, h1, h2, 0.9, 0.3, -0.2, 0.1,
                             m_out, x_out, thresholding=thresholding, max_val=1.0)
    entries = {"pred": lambda: ops.sampler_step_pred(*args), "lin": lambda: lin(0., False),
               "rescale": lambda: ops.sampler_step_rescale(*args, 0.7), "lin_rescale": lambda: lin(0.7, False),
               "lin_threshold": lambda: lin(0., True), "lin_rescale_threshold": lambda: lin(0.7, True)}
    res = time_entries(shape, entries, launches, rounds, warmup)
    res["select_us"] = round(res["lin_rescale_threshold_us"] - res["lin_rescale_us"], 3)
    return res


def bench_sde(shape, launches, rounds, warmup):
    """The stochastic step beside the deterministic one and beside the three launches it replaces."""
    import torch
    from minddiffusion_amd import ops
    dev = "cuda:0"
    B, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(0)
    r32 = lambda: torch.randn(shape, device=dev, generator=g)
    x, h1, z = r32(), r32(), r32()
    out = torch.randn((2 * B, H * W, 8), device=dev, generator=g).half()
    out_u, out_c = out[:B], out[B:]
    m_out, x_out, z_out = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    seeds = ops.seeds_tensor(list(range(100, 100 + B)), dev)
    cn, draw = 0.37, [0]

    def lin(phi):
        ops.sampler_step_lin(x, None, out_u, out_c, 7.5, ops.PRED_V, phi, ops.VALUE_X0, 0.8, 0.6, h1, None, 0.9, 0.3, -0.2, 0.,
                             m_out, x_out)

    def noisy(phi, **src):
        draw[0] += 1     # a new draw per launch, as in a run
        ops.sampler_step_lin_noise(x, None, out_u, out_c, 7.5, ops.PRED_V, phi, ops.VALUE_X0, 0.8, 0.6, h1, None, 0.9, 0.3, -0.2,
                                   0., m_out, x_out, cn, draw=draw[0], **src)

    def three(phi):
        draw[0] += 1
        ops.randn_seeded(seeds, ops.RNG_STEP, draw[0], shape[1:], out=z_out)
        lin(phi)
        x_out.add_(z_out, alpha=cn)
    entries = {}
    for tag, phi in (("", 0.), ("_rescale", 0.7)):
        entries["lin" + tag] = lambda phi=phi: lin(phi)
        entries["seeded" + tag] = lambda phi=phi: noisy(phi, seeds=seeds)
        entries["tensor" + tag] = lambda phi=phi: noisy(phi, noise=z)
        entries["three" + tag] = lambda phi=phi: three(phi)
    res = time_entries(shape, entries, launches, rounds, warmup)
    for tag in ("", "_rescale"):
        res["draw" + tag + "_us"] = round(res["seeded" + tag + "_us"] - res["lin" + tag + "_us"], 3)
        res["saved" + tag + "_us"] = round(res["three" + tag + "_us"] - res["seeded" + tag + "_us"], 3)
    return res


def bench_pc(shape, launches, rounds, warmup, with_pc=True):
    """The UniPC step launch (an order-3 record: the corrector reads three stored model values, the predictor two of them; the
    model value and both latents written) beside the DPM-Solver step launch of the same order.
    with_pc False: the lin entries alone (a library built before the pc entry)."""
    import torch
    from minddiffusion_amd import ops
    dev = "cuda:0"
    B, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(0)
    r32 = lambda: torch.randn(shape, device=dev, generator=g)
    x, xc, h1, h2, h3 = r32(), r32(), r32(), r32(), r32()
    out = torch.randn((2 * B, H * W, 8), device=dev, generator=g).half()
    out_u, out_c = out[:B], out[B:]
    m_out, x_out, xc_out = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)

    def lin(phi):
        ops.sampler_step_lin(x, None, out_u, out_c, 7.5, ops.PRED_V, phi, ops.VALUE_X0, 0.8, 0.6, h1, h2, 0.9, 0.3, -0.2, 0.1,
                             m_out, x_out)

    def pc(phi):
        ops.sampler_step_pc(xc, x, out_u, out_c, 7.5, ops.PRED_V, phi, ops.VALUE_X0, 0.8, 0.6, h1, h2, h3,
                            (0.9, 0.3, -0.2, 0.1, -0.03), (0.9, 0.3, -0.2, 0.1), m_out, xc_out, x_out)
    entries = {"lin": lambda: lin(0.), "lin_rescale": lambda: lin(0.7)}
    if with_pc:
        entries.update({"pc": lambda: pc(0.), "pc_rescale": lambda: pc(0.7)})
    res = time_entries(shape, entries, launches, rounds, warmup)
    if with_pc:
        res["pc_minus_lin_us"] = round(res["pc_us"] - res["lin_us"], 3)
        res["pc_rescale_minus_lin_rescale_us"] = round(res["pc_rescale_us"] - res["lin_rescale_us"], 3)
    return res


def bench_noise(shape, launches, rounds, warmup):
    import torch
    from minddiffusion_amd import ops
    dev = "cuda:0"
    temperature, p = 0.8, 0.25
    seeds = ops.seeds_tensor(list(range(100, 100 + shape[0])), dev)
    out = torch.empty(shape, device=dev)
    draw = [0]

    def torch_t():
        return torch.randn(shape, device=dev, dtype=torch.float32) * temperature

    def torch_td():      # the statements of the samplers' step() (ldm/models/diffusion/plms.py)
        noise = torch.randn(shape, device=dev, dtype=torch.float32) * temperature
        keep = (torch.rand(shape, device=dev) >= p).to(torch.float32)
        return noise * keep / (1. - p)

    def seeded(dropout):
        draw[0] += 1     # a new draw per launch, as in a run
        return ops.randn_seeded(seeds, ops.RNG_STEP, draw[0], shape[1:], scale=temperature, dropout=dropout, out=out)
    entries = {"torch_t": torch_t, "seeded_t": lambda: seeded(0.0), "torch_td": torch_td, "seeded_td": lambda: seeded(p)}
    res = time_entries(shape, entries, launches, rounds, warmup)
    res["saved_t_us"] = round(res["torch_t_us"] - res["seeded_t_us"], 3)
    res["saved_td_us"] = round(res["torch_td_us"] - res["seeded_td_us"], 3)
    return res


def time_entries(shape, entries, launches, rounds, warmup):
    import torch
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
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--noise", action="store_true", help="measure the stochastic step's noise preparation instead")
    ap.add_argument("--table", action="store_true", help="measure the table-driven entry beside the scalar entries instead")
    ap.add_argument("--lin", action="store_true", help="measure the DPM-Solver step launch (mdx_sampler_step_lin_f32) instead")
    ap.add_argument("--sde", action="store_true", help="measure the stochastic DPM-Solver step (mdx_sampler_step_lin_noise_f32) instead")
    ap.add_argument("--pc", action="store_true", help="measure the UniPC step launch (mdx_sampler_step_pc_f32) beside the lin launch instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("step_bench: needs a GPU")
    bench = (bench_noise if a.noise else bench_table if a.table else bench_lin if a.lin else bench_sde if a.sde else
             bench_pc if a.pc else bench_shape)
    res = {"launches": a.launches, "rounds": a.rounds, "shapes": [bench(s, a.launches, a.rounds, a.warmup) for s in SHAPES]}
    if a.noise:
        res["what"] = "noise preparation of a stochastic step, us per step"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
