"""Two ranks sharing ONE MI355X ("runnable with N ranks on 1 GPU"): the batch-sharded pipelines with the REAL
DDIM / PLMS samplers and the real (tiny) Taichu-GLIDE models -- every kernel through libmdx.so -- against single-process
runs of the same shards: bit for bit.  The process group is gloo (RCCL refuses two ranks on one device); the payload of
the one broadcast is staged through the host by distributed._broadcast, everything else is the production path."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from _util import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS, SCALE, B = 5, 5.0, 4

GL_TINY = dict(image_size=16, num_channels=64, num_res_blocks=1, channel_mult=(1, 2), num_heads=1, num_head_channels=64,
               num_heads_upsample=-1, attention_resolutions=(1, 2), dropout=0.0, text_ctx=16, xf_width=64, xf_layers=2,
               xf_heads=1, xf_final_ln=True, n_vocab=100, xf_padding=True, diffusion_steps=1000,
               noise_schedule="squaredcos_cap_v2", timestep_respacing="10", use_scale_shift_norm=True,
               resblock_updown=True, use_fp16=True, cache_text_emb=False)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ldm_model():
    from oracle import ldm as O
    from minddiffusion_amd.configs import TINY_UNET
    from minddiffusion_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from minddiffusion_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    cfg = dict(TINY_UNET)
    ocfg = dict(cfg)
    ocfg.setdefault("num_heads", -1)
    ocfg.setdefault("num_head_channels", -1)
    net = UNetModel(**cfg)
    net.load_state_dict(O.init_params(ocfg, seed=21))     # the oracle is only the seeded weight source here
    return LatentDiffusion(net, linear_start=0.00085, linear_end=0.0120, timesteps=1000), cfg["context_dim"]


def _ldm_inputs(ctx_dim):
    rng = np.random.RandomState(31)
    c = torch.from_numpy(rng.randn(B, 7, ctx_dim).astype(np.float16))
    uc = torch.from_numpy(rng.randn(1, 7, ctx_dim).astype(np.float16))
    x_T = torch.from_numpy(rng.randn(B, 4, 8, 8).astype(np.float32))
    return c, uc, x_T


def _glide_models(P):
    from oracle import glide as OG
    from minddiffusion_amd.glide.diffusion_creator import init_diffusion_model, init_super_res_model
    otiny = dict(OG.BASE_OPTIONS, image_size=16, model_channels=64, num_res_blocks=1, channel_mult=(1, 2),
                 attention_resolutions=(1, 2), text_ctx=16, xf_width=64, xf_layers=2, xf_heads=1, n_vocab=100,
                 timestep_respacing="10")
    dm = init_diffusion_model(options=GL_TINY, guidance_scale=3.0, shape=(2 * P, 3, 16, 16),
                              params=OG.init_params(otiny, seed=2))
    uopts = dict(GL_TINY, image_size=32, channel_mult=(1, 1, 2), noise_schedule="linear", timestep_respacing="fast27",
                 low_size=16)
    oup = dict(otiny, in_channels=6, image_size=32, channel_mult=(1, 1, 2), noise_schedule="linear",
               timestep_respacing="fast27")
    sr = init_super_res_model(options=uopts, shape=(P, 3, 32, 32), params=OG.init_params(oup, seed=4))
    return dm, sr


def _glide_prompts():
    rng = np.random.RandomState(41)
    return rng.randint(1, 99, (B, 16)).astype(np.int32), np.ones((B, 16), np.int32)


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0")
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    from minddiffusion_amd import distributed as D
    from minddiffusion_amd.pipeline import DiffusionPipeline
    from minddiffusion_amd.glide.pipeline import GlidePipeline
    torch.cuda.set_device(0)
    D.init_from_env(backend="gloo")
    r0 = lambda t: t if rank == 0 else None
    model, ctx_dim = _ldm_model()
    c, uc, x_T = _ldm_inputs(ctx_dim)
    for sampler in ("ddim", "plms"):
        pipe = DiffusionPipeline(model, sampler=sampler, device=DEV)
        out = pipe(c=r0(c), uc=r0(uc), x_T=r0(x_T), H=64, W=64, steps=STEPS, scale=SCALE, batch_size=B)
        torch.save(out.cpu(), os.path.join(out_dir, f"{sampler}_{rank}.pt"))
    dm, sr = _glide_models(B // world)
    tok, msk = _glide_prompts()
    gp = GlidePipeline(dm, sr, text_ctx=16, vocab_len=100)
    img = gp(tokens=r0(tok), mask=r0(msk), seed=5)
    torch.save(img.cpu(), os.path.join(out_dir, f"glide_{rank}.pt"))
    torch.save(torch.from_numpy(gp.last_uncond_tokens), os.path.join(out_dir, f"uncond_{rank}.pt"))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_real_samplers_equal_single_process(tmp_path):
    from minddiffusion_amd.pipeline import DiffusionPipeline
    from minddiffusion_amd.glide.pipeline import GlidePipeline
    out_dir = str(tmp_path)
    mp.spawn(_worker, args=(2, _free_port(), out_dir), nprocs=2, join=True)
    model, ctx_dim = _ldm_model()
    c, uc, x_T = _ldm_inputs(ctx_dim)
    per = B // 2
    for sampler in ("ddim", "plms"):
        pipe = DiffusionPipeline(model, sampler=sampler, device=DEV)
        for rank in range(2):
            lo, hi = rank * per, (rank + 1) * per
            ref = pipe(c=c[lo:hi], uc=uc, x_T=x_T[lo:hi], H=64, W=64, steps=STEPS, scale=SCALE).cpu()
            got = torch.load(os.path.join(out_dir, f"{sampler}_{rank}.pt"))
            assert torch.isfinite(got).all() and float(got.abs().max()) > 0
            assert torch.equal(got, ref), f"{sampler} rank {rank}: sharded run differs from the single-process shard"
        # and the un-sharded batch agrees to fp16 noise (a different batch size may pick other tiles / split-K factors)
        full = pipe(c=c, uc=uc, x_T=x_T, H=64, W=64, steps=STEPS, scale=SCALE).cpu()
        both = torch.cat([torch.load(os.path.join(out_dir, f"{sampler}_{r}.pt")) for r in range(2)], 0)
        check(f"two_rank_{sampler}_vs_full_batch", both, full, rel_l2=5e-3, max_rel=1e-2)
    u0, u1 = (torch.load(os.path.join(out_dir, f"uncond_{r}.pt")) for r in range(2))
    assert torch.equal(u0, u1) and tuple(u0.shape) == (10, 16)
    dm, sr = _glide_models(per)
    tok, msk = _glide_prompts()
    gp = GlidePipeline(dm, sr, text_ctx=16, vocab_len=100)
    for rank in range(2):
        lo, hi = rank * per, (rank + 1) * per
        x0, noises, up0 = gp.image_noise(5, lo, hi, 10)
        # single process, same shard: feed the broadcast's products by hand through the reference-shaped loops
        from minddiffusion_amd.glide.main_funcs import ddim_sample_loop, gaussian_p_sample_loop
        t2 = torch.from_numpy(np.concatenate([tok[lo:hi], tok[lo:hi]], 0))
        m2 = torch.from_numpy(np.concatenate([msk[lo:hi], msk[lo:hi]], 0))
        base = gaussian_p_sample_loop(dm, t2, m2, (2 * per, 3, 16, 16), 10, text_ctx=16, noise=torch.cat([x0, x0], 0),
                                      vocab_len=100, uncond_tokens=u0.numpy(), step_noises=noises)[:per]
        ref = ddim_sample_loop(sr, (per, 3, 32, 32), base, torch.from_numpy(tok[lo:hi]), torch.from_numpy(msk[lo:hi]), 27,
                               noise=up0).cpu()
        got = torch.load(os.path.join(out_dir, f"glide_{rank}.pt"))
        assert torch.isfinite(got).all() and tuple(got.shape) == (per, 3, 32, 32)
        assert torch.equal(got, ref), f"GLIDE rank {rank}: sharded run differs from the single-process shard"


def test_bench_two_ranks_contract():
    """bench.py's own N > 1 path (the driver launches it through torch.distributed.run on an 8-GPU node, which this box does
    not have): two ranks share the one GPU over gloo (MDX_DIST_BACKEND / MDX_BENCH_SHARE_GPU are test-only switches) and run
    the headline config for one timed trajectory each.  Checked: rank 0 prints exactly one JSON line, n_gpus = 2, the value is
    the whole-job rate (global batch 2 per step over the max-over-ranks time), weak scaling, no CPU baseline at N > 1 (the
    roofline checked here is part of the --full line)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MDX_DIST_BACKEND="gloo", MDX_BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
           "--full"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 1 and d["warmup"] == 1 and d["scaling"] == "weak" and d["higher_is_better"]
    assert d["config"]["global_batch"] == 2 and d["config"]["parallelism"].endswith("x2")
    assert abs(d["value"] - 2 / (d["ms_per_step"] * 1e-3)) < 1e-2 * d["value"]
    assert d["cpu_baseline"] is None and d["roofline"]["frac"] > 0
    # the N > 1 record proves itself: backend, world size, the ONE collective per trajectory and what it moved
    c = d["config"]
    assert c["dist_backend"] == "gloo" and c["rccl_world_size"] == 2 and c["broadcasts_per_step"] == 1
    assert c["broadcast_bytes"] > 2 * 77 * 1024 * 2 and c["broadcast_ms"] > 0
    assert 0 < c["per_rank_units_per_s"]["min"] <= c["per_rank_units_per_s"]["max"]


def test_bench_plain_run_contract(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W`: exactly K timed steps, the headline fields only (per-UNet-step ms,
    roofline, CPU baseline and the other configs take runs of their own and belong to --full), and --dump-outputs writes the
    latents the last timed step returned, float32."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "512x512 txt2img latents/sec (50-step DDIM)" and d["unit"] == "latents/s" and d["higher_is_better"]
    assert d["dtype"] == "f16" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert abs(d["value"] - 1 / (d["ms_per_step"] * 1e-3)) < 1e-2 * d["value"]
    assert d["config"]["hip_graph"] is True
    assert not {"per_unet_step_ms", "roofline", "cpu_baseline", "other_configs"} & set(d)
    assert sorted(os.listdir(tmp_path)) == ["latents.npy"]
    a = np.load(tmp_path / "latents.npy")
    assert a.dtype == np.float32 and a.shape == (1, 4, 64, 64) and np.isfinite(a).all() and a.std() > 0
