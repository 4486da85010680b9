"""Thin torch-tensor wrappers over the C-ABI (include/mdx.h).  torch supplies device memory and
the current HIP stream; all arithmetic happens in libmdx.so.  No CPU fallbacks."""
import ctypes
import math
import os
import weakref

import numpy as np
import torch

from . import _lib
from . import resample as _resample
from ._lib import GemmDesc, EPI_NONE, EPI_GEGLU, EPI_GELU, EPI_QUICKGELU, OUT_ROWMAJOR, OUT_TRANSPOSED  # noqa: F401
from ._lib import EPI_PRELU, OUT_D2S2  # noqa: F401

f16 = torch.float16
f32 = torch.float32


# Library-level options (experiment / tuning switches that used to be environment variables read inside the library):
# one explicit table instead of getenv() calls scattered through the code.
# -1 auto | 0 never | 32 | 64 rows per block of the fused SpatialTransformer tail (MDX_UNET_ST_TAIL presets it for A/B runs)
_OPTIONS = {"unet_st_tail": int(os.environ.get("MDX_UNET_ST_TAIL", "-1")),
            "unet_st_head": int(os.environ.get("MDX_UNET_ST_HEAD", "-1")),     # 0 = keep GroupNorm / proj_in / qkv unfused
            # 3x3 convs with at most this many output rows stream fragment-major weights to registers (0 = never)
            "unet_conv_stream": int(os.environ.get("MDX_UNET_CONV_STREAM", "128")),
            # GroupNorm inputs with > 64 row blocks per sample: 1 = pre-fold their column partials (mdx_colstats_fold_f32), 0 = the
            # two-launch statistics pass.  Measured round 3: GLIDE 256x256 7.57 -> 7.44 images/s with the fold, SDv2 96x96 equal
            "gn_colstats_fold": int(os.environ.get("MDX_GN_COLSTATS_FOLD", "0")),
            # GroupNorms of at most this many pixels per sample take over the split-K reduce of the conv in front of them
            # (mdx_groupnorm_from_splitk_f16).  Round 3, same box: 0 -> 4.437 ms per UNet step / 285 launches, 64 -> 4.422 / 274,
            # 256 -> 4.431 / 263 (round 2 had measured +0.7 %: the reduce kernels it replaces were cheaper then)
            "unet_gn_splitk_fuse": int(os.environ.get("MDX_UNET_GN_SPLITK_FUSE", "256")),
            # streamed convs: > 0 = 128-column tiles with the four waves side by side and this many K splits at most.  Measured
            # SLOWER (M = 128 convs 18.5 -> 20.4-23.6 us): off
            "unet_conv_stream_w4": int(os.environ.get("MDX_UNET_CONV_STREAM_W4", "0")),
            # 1 = a ResBlock's 1x1 skip_connection rides on its second 3x3 conv as extra K tiles (mdx_gemm_desc.skip_w)
            "unet_skip_fuse": int(os.environ.get("MDX_UNET_SKIP_FUSE", "1")),
            # GroupNorm + SiLU inside the consuming 3x3 conv at levels with at least this many output rows (0 = never)
            # (mdx_gemm_desc.gn_colstats).  Measured round 3 at UNet batch 2: 7 GroupNorm launches fewer (-0.10 ms) but the convs'
            # in-LDS normalisation pass costs as much (+0.10 ms): 4.603 -> 4.641 ms per step.  Off.
            "unet_gn_conv_fuse": int(os.environ.get("MDX_UNET_GN_CONV_FUSE", "0")),
            # 1 = when a plan is built, launches whose shape the measured tile table (csrc/gemm_tuned.inc) does not list are timed
            # once on the device (mdx_gemm_tune, a few ms per distinct shape) and keep the fastest form; answers live in tune_cache
            "unet_tune_first_use": int(os.environ.get("MDX_UNET_TUNE_FIRST_USE", "0")),
            # 1 = Upsample convs carry the sub-pixel weights (mdx_gemm_desc.w_sub: 4 Cin instead of 9 Cin products per output on the
            # un-upsampled tensor); the library uses them wherever the eight-wave conv core applies
            "unet_subpixel_upsample": int(os.environ.get("MDX_UNET_SUBPIXEL_UPSAMPLE", "1")),
            # SpatialTransformer.norm (GroupNorm without an activation) applied inside proj_in (mdx_gemm_desc.gn_colstats on a dense
            # launch: one packed fma per A fragment) at levels with at least this many tokens per sample (0 = never): no GroupNorm
            # launch, no normalised copy of the tensor.  Measured round 5 (tools/eval_ab.py, profiles/r05_gn_proj_fuse_ab.txt): at
            # 1024, SDv2 batch 2 233 ops instead of 238 at EQUAL time (4.2824 vs 4.2825 ms: every consumer block folds the statistics
            # before its first MFMA, which costs what the 7 us launch did), Wukong batch 16 +0.4 %, 96 x 96 batch 8 +0.5 %; at 256
            # (the levels whose GroupNorm launch doubles as a split-K reduce) +0.5 % / +1.0 % / +1.6 %.  Off.
            "unet_gn_proj_fuse": int(os.environ.get("MDX_UNET_GN_PROJ_FUSE", "0")),
            # (round 6) SDv2 (head dim 64): BasicTransformerBlock.attn2 -- to_q + the attention over the cached 77 context keys -- as ONE
            # launch, the attention as the epilogue of the query projection (mdx_gemm_desc.xattn_k); 0 = projection + attention launches
            "unet_xattn_fuse": int(os.environ.get("MDX_UNET_XATTN_FUSE", "1")),
            # (round 6) classifier-free guidance evaluates cat([x] * 2) with [uncond ; cond] contexts (plms.py:192-195): up to the
            # first cross-attention both halves are the same numbers.  From this batch on (0 = never) a sampler's guidance call runs
            # conv_in .. the first self-attention (and its output projection where that is a launch of its own) on ONE half and write the result to both (UNetModel._dup_body)
            "unet_cfg_dup": int(os.environ.get("MDX_UNET_CFG_DUP", "4")),
            # 1 = every cfg_dup call first compares the two halves of x (and of per-sample timesteps / temb rows) on the device and raises if
            # they differ: a host synchronisation per call, for bringing up a new sampler -- the shipped samplers build both halves
            # from one tensor
            "unet_cfg_dup_check": int(os.environ.get("MDX_UNET_CFG_DUP_CHECK", "0")),
            # The last ff2 of an unfused SpatialTransformer and its proj_out have no non-linearity between them: from this `inner`
            # on (0 = never; the launch must also have M >= 128) they run as ONE dense launch over the K-concatenated operand
            # [g | tok3] with the composite weight [W_p W_f2 | W_p] (compose_ff_proj; same FLOPs, same weight bytes, one launch and
            # one [M, C] round trip fewer; needs the K-segmented lean dense kernel).  The default keeps the tiny / small test
            # models (inner <= 320) on the launches their bit-exact fixtures were recorded with.  Measured at UNet batch 2 (profiles/ff_proj_fuse_*): per block
            # 30.3 -> 23.3 us (M = 2048), 31.8 -> 23.9 us (M = 512), 23.0 -> 14.4 us (M = 128); 227 -> 216 ops; bench.py six alternating
            # pairs 5.390-5.405 -> 5.490-5.501 latents/s (+1.9 %, ranges disjoint)
            "unet_ff_proj_fuse": int(os.environ.get("MDX_UNET_FF_PROJ_FUSE", "640")),
            # Taichu-GLIDE AttentionBlock (unet.py:267-297): 1 = q | k | v of the image tokens in ONE launch (q | k row-major into a
            # [B, text + image, 2 C] buffer, V transposed: mdx_gemm_desc.n_split with out_bs) instead of three -- 44 launches fewer
            # per base evaluation.  0 = three launches (A/B)
            "glide_qkv_merge": int(os.environ.get("MDX_GLIDE_QKV_MERGE", "1")),
            # Taichu-GLIDE AttentionBlock.norm (GroupNorm without an activation) applied inside the merged q | k | v projection
            # (mdx_gemm_desc.gn_colstats on a dense launch): 22 GroupNorm launches fewer per base evaluation
            "glide_gn_qkv_fuse": int(os.environ.get("MDX_GLIDE_GN_QKV_FUSE", "0"))}


def set_option(name, value):
    """Python-level planner options (unet_st_tail, unet_st_head) or, for any other name, a library option
    (include/mdx.h: mdx_set_option -- gemm_tuned, gemm_bm, gemm_splitk_fixup_max, ...)."""
    if name in _OPTIONS:
        _OPTIONS[name] = int(value)
        return
    _lib.check(_lib.load().mdx_set_option(name.encode(), int(value)), "mdx_set_option")


def get_option(name):
    if name in _OPTIONS:
        return _OPTIONS[name]
    out = ctypes.c_int(0)
    _lib.check(_lib.load().mdx_get_option(name.encode(), ctypes.byref(out)), "mdx_get_option")
    return int(out.value)


def capture_graph(ops_list):
    """Capture the calls of ops_list into one hipGraph and return it.  Python's cyclic garbage collector is held off for the
    duration: a collection in the middle of a capture can finalise an OLDER plan (its graph, its buffers) -- hipGraphExecDestroy /
    hipFree, calls the runtime refuses while a stream is capturing -- and an error inside a C++ destructor aborts the process
    (seen once in round 3: a full test run died in a text-encoder capture while 40 earlier plans were waiting for the collector)."""
    import gc
    g = torch.cuda.CUDAGraph()
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g):
            for op in ops_list:
                op()
    finally:
        if was_enabled:
            gc.enable()
    return g


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _chk(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.MdxError(f"{name}: tensor must live on the GPU (no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.MdxError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.MdxError(f"{name}: tensor must be contiguous")


def nchw_to_nhwc(x, cpad, out=None):
    """[B,C,H,W] fp32 -> [B,H*W,cpad] fp16 (zero-padded channels)."""
    _chk(x, f32, "x")
    B, C, H, W = x.shape
    if out is None:
        out = torch.empty((B, H * W, cpad), dtype=f16, device=x.device)
    _lib.check(_lib.load().mdx_nchw_to_nhwc_f16(_ptr(x), _ptr(out), B, C, H, W, cpad, _stream()), "mdx_nchw_to_nhwc_f16")
    return out


def nhwc_to_nchw(x, C, H, W, out=None):
    """[B,H*W,Cs] fp16 -> [B,C,H,W] fp32."""
    _chk(x, f16, "x")
    B, HW, Cs = x.shape
    assert HW == H * W
    if out is None:
        out = torch.empty((B, C, H, W), dtype=f32, device=x.device)
    _lib.check(_lib.load().mdx_nhwc_to_nchw_f32(_ptr(x), _ptr(out), B, C, H, W, Cs, _stream()), "mdx_nhwc_to_nchw_f32")
    return out


def groupnorm_ws_floats(B, HW, C, groups=32):
    return int(_lib.load().mdx_groupnorm_ws_floats(B, HW, C, groups))


def groupnorm(x1, x2, gamma, beta, eps, silu, ws=None, out=None, groups=32):
    """GroupNorm(groups)(cat(x1,x2)) [+SiLU]; x* [B,HW,C*] fp16, gamma/beta fp32."""
    _chk(x1, f16, "x1"); _chk(x2, f16, "x2"); _chk(gamma, f32, "gamma"); _chk(beta, f32, "beta")
    B, HW, C1 = x1.shape
    C2 = 0 if x2 is None else x2.shape[2]
    C = C1 + C2
    if ws is None:
        ws = torch.empty(groupnorm_ws_floats(B, HW, C, groups), dtype=f32, device=x1.device)
    if out is None:
        out = torch.empty((B, HW, C), dtype=f16, device=x1.device)
    _lib.check(_lib.load().mdx_groupnorm_f16(_ptr(x1), C1, _ptr(x2), C2, _ptr(gamma), _ptr(beta), _ptr(out), B, HW,
                                             groups, float(eps), int(bool(silu)), _ptr(ws), _stream()),
               "mdx_groupnorm_f16")
    return out


GN_FORMS = ("two_launch", "fused", "fused_one_pass", "fused_256", "colstats")


def groupnorm_query(C1, C2, B, HW, groups=32, colstats_nrb=0):
    """The launch form a GroupNorm of this shape resolves to under the current library options (mdx_groupnorm_query; host only):
    form is one of GN_FORMS; colstats_nrb > 0 asks about groupnorm_colstats."""
    out = (ctypes.c_int * 6)()
    _lib.check(_lib.load().mdx_groupnorm_query(int(C1), int(C2), int(B), int(HW), int(groups), int(colstats_nrb), out),
               "mdx_groupnorm_query")
    return dict(form=GN_FORMS[out[0]], cw=out[1], ncb=out[2], nblk=out[3], pix=out[4], threads=out[5])


class FoldedColStats:
    """Column partials with more than 64 row blocks per sample (include/mdx.h: mdx_colstats_fold_f32): `raw` [B * nrb, C, 2] is
    what the producer writes, `folded` [B * nrb2, C, 2] what the GroupNorm reads; groupnorm_colstats launches the fold."""

    def __init__(self, raw, nrb, batch):
        f = (nrb + 63) // 64
        self.raw, self.nrb, self.batch = raw, nrb, batch
        self.nrb2 = (nrb + f - 1) // f
        self.folded = torch.zeros((batch * self.nrb2, raw.shape[1], 2), dtype=f32, device=raw.device)

    def data_ptr(self):         # (the producer's descriptor points at the raw partials)
        return self.raw.data_ptr()

    def fold(self):
        _lib.check(_lib.load().mdx_colstats_fold_f32(_ptr(self.raw), self.nrb, _ptr(self.folded), self.nrb2, self.batch,
                                                     self.raw.shape[1], _stream()), "mdx_colstats_fold_f32")
        return self.folded, self.nrb2


def groupnorm_colstats(x1, cs1, nrb1, x2, cs2, nrb2, gamma, beta, eps, silu, out=None, groups=32, scale=None, shift=None,
                       mod_ld=0):
    """GroupNorm(groups)(cat(x1, x2)) [* (1 + scale) + shift] [+SiLU] with the statistics folded from the producers' column
    partials (mdx_gemm_desc.colstats_out): one launch, one read of x (plus one small fold launch per source with more than
    64 row blocks per sample)."""
    if isinstance(cs1, FoldedColStats):
        cs1, nrb1 = cs1.fold()
    if isinstance(cs2, FoldedColStats):
        cs2, nrb2 = cs2.fold()
    B, HW, C1 = x1.shape
    C2 = 0 if x2 is None else x2.shape[2]
    if out is None:
        out = torch.empty((B, HW, C1 + C2), dtype=f16, device=x1.device)
    _lib.check(_lib.load().mdx_groupnorm_colstats_f16(_ptr(x1), C1, _ptr(cs1), int(nrb1), _ptr(x2), C2, _ptr(cs2), int(nrb2),
                                                      _ptr(gamma), _ptr(beta), _ptr(scale), _ptr(shift), int(mod_ld),
                                                      _ptr(out), B, HW, groups, float(eps), int(bool(silu)), _stream()),
               "mdx_groupnorm_colstats_f16")
    return out


def groupnorm_from_splitk_ok(desc, groups=32):
    return bool(_lib.load().mdx_groupnorm_from_splitk_ok(ctypes.byref(desc), groups))


def groupnorm_from_splitk(desc, gamma, beta, eps, silu, out, groups=32):
    """GroupNorm fused with the split-K reduce of the conv / Dense `desc` (launched with defer_reduce = 1)."""
    _lib.check(_lib.load().mdx_groupnorm_from_splitk_f16(ctypes.byref(desc), _ptr(gamma), _ptr(beta), _ptr(out), groups,
                                                         float(eps), int(bool(silu)), _stream()),
               "mdx_groupnorm_from_splitk_f16")
    return out


def groupnorm_scaleshift(x1, x2, gamma, beta, scale, shift, mod_ld, eps, silu, ws=None, out=None, groups=32):
    """GLIDE ResBlock FiLM norm: silu?(GN(cat(x1,x2)) * (1 + scale[b]) + shift[b]); scale/shift fp32 views [B, C]."""
    _chk(x1, f16, "x1"); _chk(x2, f16, "x2")
    B, HW, C1 = x1.shape
    C2 = 0 if x2 is None else x2.shape[2]
    C = C1 + C2
    if ws is None:
        ws = torch.empty(groupnorm_ws_floats(B, HW, C, groups), dtype=f32, device=x1.device)
    if out is None:
        out = torch.empty((B, HW, C), dtype=f16, device=x1.device)
    _lib.check(_lib.load().mdx_groupnorm_scaleshift_f16(
        _ptr(x1), C1, _ptr(x2), C2, _ptr(gamma), _ptr(beta), _ptr(scale), _ptr(shift), int(mod_ld), _ptr(out), B, HW,
        groups, float(eps), int(bool(silu)), _ptr(ws), _stream()), "mdx_groupnorm_scaleshift_f16")
    return out


def avgpool2x2(x, B, H, W, C, out=None):
    if out is None:
        out = torch.empty((B, (H // 2) * (W // 2), C), dtype=f16, device=x.device)
    _lib.check(_lib.load().mdx_avgpool2x2_f16(_ptr(x), _ptr(out), B, H, W, C, _stream()), "mdx_avgpool2x2_f16")
    return out


def upsample_nearest2x(x, B, H, W, C, out=None):
    if out is None:
        out = torch.empty((B, 4 * H * W, C), dtype=f16, device=x.device)
    _lib.check(_lib.load().mdx_upsample_nearest2x_f16(_ptr(x), _ptr(out), B, H, W, C, _stream()),
               "mdx_upsample_nearest2x_f16")
    return out


def glide_text_embed(tokens, mask, tok_emb, pos, pad, out=None):
    """tokens/mask int32 [B,T]; tables fp16; -> [B,T,width] fp16."""
    B, T = tokens.shape
    width = pos.shape[1]
    if out is None:
        out = torch.empty((B, T, width), dtype=f16, device=tokens.device)
    _lib.check(_lib.load().mdx_glide_text_embed_f16(_ptr(tokens), _ptr(mask), _ptr(tok_emb), _ptr(pos), _ptr(pad),
                                                    _ptr(out), B, T, width, tok_emb.shape[0], _stream()),
               "mdx_glide_text_embed_f16")
    return out


def glide_superres_input(x, low, out=None):
    """x [B,3,S,S] fp32, low [B,3,s,s] fp32 -> NHWC fp16 [B, S*S, 8] = [x | bilinear(quantised low) | 0 0]."""
    B, _, S, _ = x.shape
    if out is None:
        out = torch.empty((B, S * S, 8), dtype=f16, device=x.device)
    _lib.check(_lib.load().mdx_glide_superres_input_f16(_ptr(x), _ptr(low), _ptr(out), B, S, low.shape[2], _stream()),
               "mdx_glide_superres_input_f16")
    return out


def glide_step(x, out_c, out_u, ld, scale, coef8, mode, noise_scale, noise, x_next, pred_x0):
    B, _, H, W = x.shape
    c8 = (ctypes.c_float * 8)(*[float(v) for v in coef8])
    _lib.check(_lib.load().mdx_glide_step_f32(_ptr(x), _ptr(out_c), _ptr(out_u), int(ld), float(scale),
                                              ctypes.cast(c8, ctypes.c_void_p), int(mode), float(noise_scale),
                                              _ptr(noise), _ptr(x_next), _ptr(pred_x0), B, H, W, _stream()),
               "mdx_glide_step_f32")


def glide_kv_slots(entries, device):
    """Device array of struct mdx_glide_kv_slot (include/mdx.h) from (src, dst, src_entry_bytes, dst_batch_bytes, src_pitch,
    dst_pitch, rows, row_bytes) tuples with tensor src / dst; returns (int64 tensor [n, 7] that holds the structs, n)."""
    import numpy as np
    rows = []
    for src, dst, seb, dbb, sp, dp, r, rb in entries:
        for v in (src.data_ptr(), dst.data_ptr(), seb, dbb, sp, dp, rb):
            if v % 16:
                raise _lib.MdxError("glide_kv_slots: pointers and byte counts must be multiples of 16")
        rows.append([src.data_ptr(), dst.data_ptr(), seb, dbb, sp, dp, (int(r) & 0xffffffff) | (int(rb) << 32)])
    return torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(device), len(rows)


def glide_kv_select(slots, nslots, entry0, entry_per_b, b0, nb, blocks_per_copy=8):
    _lib.check(_lib.load().mdx_glide_kv_select_f16(_ptr(slots), int(nslots), int(entry0), int(entry_per_b), int(b0), int(nb),
                                                   int(blocks_per_copy), _stream()), "mdx_glide_kv_select_f16")


def layernorm(x, gamma, beta, eps, out=None):
    _chk(x, f16, "x"); _chk(gamma, f32, "gamma"); _chk(beta, f32, "beta")
    C = x.shape[-1]
    rows = x.numel() // C
    if out is None:
        out = torch.empty_like(x)
    _lib.check(_lib.load().mdx_layernorm_f16(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), rows, C, float(eps), _stream()),
               "mdx_layernorm_f16")
    return out


def pack_gemm_weight(w2d):
    """[N, K] weight (K already in the kernel's K order) -> the packed fp16 storage mdx_gemm_f16 reads
    (include/mdx.h): N, K zero-padded to multiples of 64, tile-major [N/64][K/64][64][8 chunks][8], chunks
    pre-swizzled (position q of row r holds logical chunk q ^ ((r >> 1) & 7)).  Pure data movement, done once
    at weight-load time."""
    N, K = w2d.shape
    dev = w2d.device
    Np, Kp = (N + 63) // 64 * 64, (K + 63) // 64 * 64
    wp = torch.zeros((Np, Kp), dtype=f16, device=dev)
    wp[:N, :K] = w2d
    t = wp.view(Np // 64, 64, Kp // 64, 8, 8).permute(0, 2, 1, 3, 4)          # [panel, ktile, row, chunk, 8]
    r = torch.arange(64, device=dev)
    src = torch.arange(8, device=dev)[None, :] ^ ((r >> 1) & 7)[:, None]       # [row, position] -> logical chunk
    idx = src[None, None, :, :, None].expand(Np // 64, Kp // 64, 64, 8, 8)
    return torch.gather(t, 3, idx).contiguous().view(-1)


def conv_weight_k_order(w4d, cin_pad=None, cout_pad=None):
    """[Cout, Cin, kh, kw] -> [Cout_pad, K] in the kernel's K order: [cin/64][kh*kw][64] when Cin % 64 == 0
    (channel-chunk major, tap minor), else tap-major [kh*kw][Cin_pad]."""
    w4d = w4d.to(torch.float32)
    co, ci, kh, kw = w4d.shape
    cip = cin_pad or ci
    cop = cout_pad or co
    if cip % 64 == 0:
        assert cip == ci
        p = torch.zeros((cop, ci // 64, kh * kw, 64), dtype=torch.float32, device=w4d.device)
        p[:co] = w4d.reshape(co, ci // 64, 64, kh * kw).permute(0, 1, 3, 2)
        return p.reshape(cop, kh * kw * ci)
    p = torch.zeros((cop, kh * kw, cip), dtype=torch.float32, device=w4d.device)
    p[:co, :, :ci] = w4d.permute(0, 2, 3, 1).reshape(co, kh * kw, ci)
    return p.reshape(cop, kh * kw * cip)


def pack_conv_weight(w4d, cin_pad=None, cout_pad=None):
    return pack_gemm_weight(conv_weight_k_order(w4d, cin_pad, cout_pad))


def subpixel_conv_weight(w4d):
    """[Cout, Cin, 3, 3] of a conv that follows a nearest-2x upsample (Upsample.construct, openaimodel.py:57-60) -> the four
    2 x 2 convs of the LOW-resolution tensor it is equal to, [4 Cout, Cin, 2, 2] (parity (dy, dx) major): output pixel
    (2y + dy, 2x + dx) reads upsampled rows 2y + dy + ky - 1, i.e. source rows {y - 1, y, y} (dy = 0) or {y, y, y + 1} (dy = 1), so the
    taps that fall on one source row are summed (fp32, rounded to fp16 once by the packer): rows {w0, w1 + w2} / {w0 + w1, w2},
    columns likewise.  4 Cin instead of 9 Cin products per output."""
    w = w4d.to(torch.float32)
    rows = {0: (w[:, :, 0], w[:, :, 1] + w[:, :, 2]), 1: (w[:, :, 0] + w[:, :, 1], w[:, :, 2])}       # [Cout, Cin, 3 (kx)] each
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            taps = []
            for a in (0, 1):
                r = rows[dy][a]
                cols = (r[:, :, 0], r[:, :, 1] + r[:, :, 2]) if dx == 0 else (r[:, :, 0] + r[:, :, 1], r[:, :, 2])
                taps.append(torch.stack(cols, -1))                                                     # [Cout, Cin, 2 (b)]
            out.append(torch.stack(taps, 2))                                                           # [Cout, Cin, 2 (a), 2 (b)]
    return torch.cat(out, 0)


def pack_subpixel_conv_weight(w4d):
    """mdx_gemm_desc.w_sub (include/mdx.h): the packed per-parity 2 x 2 weights, logical [4 Cout][4 Cin] in the conv K order."""
    assert w4d.shape[0] % 64 == 0 and w4d.shape[1] % 64 == 0
    return pack_conv_weight(subpixel_conv_weight(w4d))


def pack_conv_weight_frag(w4d):
    """[Cout, Cin, 3, 3] -> the MFMA-fragment-major packing of mdx_gemm_desc.w_frag (Cout % 64 == 0, Cin % 64 == 0)."""
    co, ci = w4d.shape[0], w4d.shape[1]
    assert co % 64 == 0 and ci % 64 == 0
    return pack_frag_weight(conv_weight_k_order(w4d).to(f16)).reshape(-1)


def unpack_gemm_weight(packed, N, K):
    """Inverse of pack_gemm_weight: the tile-major, pre-swizzled storage -> [N, K] (plan-time re-packing of a conv that turns
    out to want the fragment-major form once its M is known)."""
    Np, Kp = (N + 63) // 64 * 64, (K + 63) // 64 * 64
    t = packed.view(Np // 64, Kp // 64, 64, 8, 8)
    r = torch.arange(64, device=packed.device)
    src = torch.arange(8, device=packed.device)[None, :] ^ ((r >> 1) & 7)[:, None]      # position -> logical chunk
    inv = torch.argsort(src, 1)                                                          # logical chunk -> position
    idx = inv[None, None, :, :, None].expand(Np // 64, Kp // 64, 64, 8, 8)
    return torch.gather(t, 3, idx).permute(0, 2, 1, 3, 4).reshape(Np, Kp)[:N, :K].contiguous()


def geglu_interleave(a, g, unit=64):
    """GEGLU packing of mdx_gemm_f16 (include/mdx.h, MDX_EPI_GEGLU / mdx_gemm_desc.geglu_unit): the 'a' rows and the gate rows of the
    projection ([half, ...] each: weight rows, bias or S[n] entries) -> [2 half, ...] with `unit` 'a' rows followed by their `unit` gate
    rows per 2 * unit-wide N tile.  unit 64: the 128-column tiles; 80: the 128 x 160 tile."""
    half = a.shape[0]
    assert g.shape == a.shape and half % unit == 0
    nt = half // unit
    return torch.stack([a.reshape(nt, unit, *a.shape[1:]), g.reshape(nt, unit, *a.shape[1:])], 1).reshape(2 * half, *a.shape[1:]).contiguous()


def geglu_deinterleave(t, unit=64):
    """Inverse of geglu_interleave: ([half, ...] 'a' rows, [half, ...] gate rows)."""
    half = t.shape[0] // 2
    assert t.shape[0] % (2 * unit) == 0
    x = t.reshape(half // unit, 2, unit, *t.shape[1:])
    return x[:, 0].reshape(half, *t.shape[1:]).contiguous(), x[:, 1].reshape(half, *t.shape[1:]).contiguous()


def geglu_repack(t, unit_from, unit_to):
    """A GEGLU-interleaved tensor (rows of the weight, bias, S[n]) from one packing unit to another: a row permutation, done once."""
    return geglu_interleave(*geglu_deinterleave(t, unit_from), unit_to)


def compose_ff_proj(w_p, b_p, w_f2, b_f2):
    """proj_out folded into the feed-forward's second Dense (option unet_ff_proj_fuse): with g the GEGLU hidden and tok3 the
    residual stream,  x + b_p + W_p (tok3 + b_f2 + W_f2 g) = x + bc + [g | tok3] [Wc | W_p]^T.  w_p [ch, inner] and w_f2
    [inner, 4 inner] are the stored fp16 matrices, b_p / b_f2 their fp32 biases.  Returns ([ch, 5 inner] fp16 = [Wc | W_p] with
    Wc = fp16(W_p W_f2), the product taken in fp64; bc = b_p + W_p b_f2 in fp32)."""
    wp64 = w_p.to(torch.float64)
    wc = (wp64 @ w_f2.to(torch.float64)).to(f16)
    bc = (b_p.to(torch.float64) + wp64 @ b_f2.to(torch.float64)).to(f32)
    return torch.cat([wc, w_p.to(f16)], 1).contiguous(), bc.contiguous()


def make_gemm_desc(a, w, N, B, H, W, c1, out, out_ld, a2=None, c2=0, bias=None, rowbias=None, rowbias_ld=0,
                   residual=None, residual_ld=0, ksize=1, stride=1, upsample=0, epilogue=EPI_NONE,
                   out_mode=OUT_ROWMAJOR, splitk=0, workspace=None, out_bs=0, out2=None, out2_ld=0, n_split=0, asym_pad=0,
                   stats_out=None, ln_stats=None, ln_s=None, ln_eps=1e-5, tile_m=0, tile_n=0, colstats_out=None, stages=0,
                   w_frag=0, skip_a=None, skip_a2=None, skip_c1=0, skip_c2=0, skip_w=None, gn_colstats=None, gn_nrb=0,
                   gn_gamma=None, gn_beta=None, gn_eps=1e-5, gn_silu=1, w_sub=None, xattn_k=None, xattn_vt=None, xattn_len=0,
                   xattn_cap=0, xattn_scale=0.0, act_slope=None, geglu_unit=0):
    d = GemmDesc()
    d.a = a.data_ptr()
    d.a2 = 0 if a2 is None else a2.data_ptr()
    d.c1, d.c2 = int(c1), int(c2)
    d.w = w.data_ptr()
    d.bias = 0 if bias is None else bias.data_ptr()
    d.rowbias = 0 if rowbias is None else rowbias.data_ptr()
    d.rowbias_ld = int(rowbias_ld)
    d.residual = 0 if residual is None else residual.data_ptr()
    d.residual_ld = int(residual_ld)
    d.out = out.data_ptr()
    d.out_ld = int(out_ld)
    d.B, d.H, d.W, d.N = int(B), int(H), int(W), int(N)
    d.ksize, d.stride, d.upsample = int(ksize), int(stride), int(upsample)
    d.epilogue, d.out_mode, d.splitk = int(epilogue), int(out_mode), int(splitk)
    d.workspace = 0 if workspace is None else workspace.data_ptr()
    d.workspace_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    d.out_bs = int(out_bs)
    d.out2 = 0 if out2 is None else out2.data_ptr()
    d.out2_ld, d.n_split, d.asym_pad = int(out2_ld), int(n_split), int(asym_pad)
    # LayerNorm fold (include/mdx.h): producer statistics / consumer correction
    d.stats_out = 0 if stats_out is None else stats_out.data_ptr()
    d.ln_stats = 0 if ln_stats is None else ln_stats.data_ptr()
    d.ln_s = 0 if ln_s is None else ln_s.data_ptr()
    d.ln_nt = 0 if ln_stats is None else (int(c1) + int(c2)) // 64
    d.ln_eps = float(ln_eps)
    d.tile_m, d.tile_n, d.stages, d.w_frag = int(tile_m), int(tile_n), int(stages), int(w_frag)
    d.gn_colstats = 0 if gn_colstats is None else gn_colstats.data_ptr()
    d.gn_gamma = 0 if gn_gamma is None else gn_gamma.data_ptr()
    d.gn_beta = 0 if gn_beta is None else gn_beta.data_ptr()
    d.gn_nrb, d.gn_silu, d.gn_eps = int(gn_nrb), int(gn_silu), float(gn_eps)
    d.skip_a = 0 if skip_a is None else skip_a.data_ptr()
    d.skip_a2 = 0 if skip_a2 is None else skip_a2.data_ptr()
    d.skip_c1, d.skip_c2 = int(skip_c1), int(skip_c2)
    d.skip_w = 0 if skip_w is None else skip_w.data_ptr()
    d.colstats_out = 0 if colstats_out is None else colstats_out.data_ptr()
    d.colstats_cap = 0 if colstats_out is None else int(colstats_out.shape[0])
    d.w_sub = 0 if w_sub is None else w_sub.data_ptr()
    if xattn_k is not None:      # cross-attention as the epilogue of the query projection (include/mdx.h)
        d.xattn_k, d.xattn_vt = xattn_k.data_ptr(), xattn_vt.data_ptr()
        d.xattn_len, d.xattn_cap, d.xattn_scale = int(xattn_len), int(xattn_cap), float(xattn_scale)
    if act_slope is not None:    # MDX_EPI_PRELU: per-channel slopes, fp32 [C], column n uses act_slope[n % C]
        d.act_slope, d.act_slope_n = act_slope.data_ptr(), int(act_slope.numel())
    d.geglu_unit = int(geglu_unit)      # GEGLU: packing unit of w / bias / ln_s (0 = 64; 80 = the 128 x 160 tile)
    # The C struct holds raw device pointers only.  The descriptor keeps its tensors alive (python-side attribute), so that an
    # argument built in the call expression -- `bias=interleave(cb)` -- is not handed back to the caching allocator, and to
    # whoever allocates next, between this call and the launch.
    d._tensors = tuple(t for t in (a, a2, w, bias, rowbias, residual, out, workspace, out2, stats_out, ln_stats, ln_s,
                                   colstats_out, skip_a, skip_a2, skip_w, gn_colstats, gn_gamma, gn_beta, w_sub, xattn_k,
                                   xattn_vt, act_slope) if t is not None)
    return d


def fold_layernorm(wt, gamma, beta, bias=None):
    """Host side of the LayerNorm fold (include/mdx.h, mdx_gemm_desc.ln_stats): for y = LN(x; gamma, beta) W^T + b returns
    (fp16 gamma (.) W [N, K], S fp32 [N], W beta + b fp32 [N]).  S is summed from the fp16-ROUNDED product, i.e. from
    exactly the numbers the MFMA multiplies, so the mean term cancels to accumulation noise."""
    w32 = wt.to(torch.float64)
    wg = (w32 * gamma.to(torch.float64)[None, :]).to(f16)
    s = wg.to(torch.float64).sum(1).to(f32).contiguous()
    cb = w32 @ beta.to(torch.float64)
    if bias is not None:
        cb = cb + bias.to(torch.float64)
    return wg.contiguous(), s, cb.to(f32).contiguous()


def gemm_workspace_bytes(desc):
    return int(_lib.load().mdx_gemm_workspace_bytes(ctypes.byref(desc)))


_WS_HEAD = 16384      # MDX_GEMM_WS_HEAD (include/mdx.h): bytes of arrival counters per workspace


def new_gemm_workspace(nbytes, device):
    """A split-K workspace for mdx_gemm_f16 (fp32) with its arrival counters: ONE zeroed torch allocation [16 KiB of counters |
    workspace], the counters bound to the workspace address (mdx_gemm_bind_counters) -- so libmdx.so allocates no device memory
    for launches on it (include/mdx.h, ownership rule) -- and unbound when the tensor dies (before the caching allocator can hand
    the address to anything else).  The workspace itself needs no initialisation."""
    import weakref
    base = torch.zeros((_WS_HEAD + max(int(nbytes), 16)) // 4 + 1, dtype=f32, device=device)
    ws = base[_WS_HEAD // 4:]
    lib = _lib.load()
    _lib.check(lib.mdx_gemm_bind_counters(ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(base.data_ptr())),
               "mdx_gemm_bind_counters")
    # unbind when the workspace tensor object dies (the plans hold exactly this object; its storage cannot be freed earlier)
    weakref.finalize(ws, lib.mdx_gemm_release_workspace, ctypes.c_void_p(ws.data_ptr()))
    return ws


def gemm_check(desc):
    """True when mdx_gemm_f16 would accept this descriptor as it stands (mdx_gemm_check: validation + launch resolution, no launch)."""
    return _lib.load().mdx_gemm_check(ctypes.byref(desc)) == 0


def gemm_query(desc):
    """(tile_m, tile_n, splitk, halo, from_tuned_table, colstats rows per block, in-kernel split-K reduce) mdx_gemm_f16
    would use for this descriptor (no launch)."""
    out = (ctypes.c_int * 7)()
    _lib.check(_lib.load().mdx_gemm_query(ctypes.byref(desc), out), "mdx_gemm_query")
    return tuple(int(v) for v in out)


# First-use tuning (include/mdx.h mdx_gemm_tune): the user-side cache.  key = gemm_shape_key(desc) -> (tile_m, tile_n, splitk,
# stages, us of the library's choice, us of the best form).  save_tune_cache / load_tune_cache keep it across processes.
tune_cache = {}
_tune_flush = {}


def gemm_shape_key(d):
    """What a launch form depends on: problem shape + launch variant (the tile table's key, gemm_plan.hip tuned_variant())."""
    var = ((1 if d.c2 > 0 else 0) | (d.epilogue << 1) | (8 if d.n_split else 0) | (16 if d.ln_stats else 0)
           | (32 if d.stats_out else 0) | (64 if d.out_mode == 1 else 0) | (128 if d.colstats_out else 0)
           | (256 if d.residual else 0) | (512 if d.rowbias else 0) | (1024 if d.skip_w else 0) | (2048 if d.gn_gamma else 0)
           | (4096 if d.w_sub else 0))      # (w_sub: the sub-pixel form of an Upsample conv resolves to another kernel)
    # B, H, W are part of the key: HALO eligibility, patch geometry (16-wide patches vs the 8 x 8 two-sample form) and the
    # eight-wave cores' tile counts depend on them, not only on M = B H W
    return (d.B * d.H * d.W, d.N, d.ksize * d.ksize * (d.c1 + d.c2), d.ksize, d.stride, d.upsample, var, d.B, d.H, d.W)


def gemm_tune(desc, reps=5, cold=True):
    """mdx_gemm_tune on the current stream: (tile_m, tile_n, splitk, stages, us_auto, us_best); zeros = keep the library's
    choice.  cold: a 512 MiB fill evicts L2 / Infinity Cache before every timed launch (weights arrive cold, as in a UNet
    evaluation).  SYNCHRONISES; overwrites desc.out."""
    flush, nbytes = None, 0
    if cold:
        dev = torch.cuda.current_device()
        if dev not in _tune_flush:
            _tune_flush[dev] = torch.empty(512 << 20, dtype=torch.uint8, device=f"cuda:{dev}")
        flush, nbytes = ctypes.c_void_p(_tune_flush[dev].data_ptr()), _tune_flush[dev].numel()
    best, us = (ctypes.c_int * 4)(), (ctypes.c_float * 2)()
    _lib.check(_lib.load().mdx_gemm_tune(ctypes.byref(desc), _stream(), flush, nbytes, int(reps), best, us), "mdx_gemm_tune")
    return tuple(int(v) for v in best) + (float(us[0]), float(us[1]))


def tune_untuned(descs, reps=5):
    """First-use pass of a planner: every descriptor whose shape neither the tile table nor tune_cache knows is measured once
    (descriptors tied to their launch form -- colstats_out, defer_reduce, w_frag -- and forced ones are left alone); the
    cached form is applied to every descriptor of that shape.  Returns the number of shapes measured."""
    measured = 0
    for d in descs:
        if (d.colstats_out or d.defer_reduce or d.w_frag or d.skip_w or d.gn_gamma or d.tile_m or d.tile_n or d.splitk
                or d.stages or d.geglu_unit):      # (geglu_unit: weights packed for the 128 x 160 tile the tile table chose)
            continue
        key = gemm_shape_key(d)
        if key not in tune_cache:
            if gemm_query(d)[4]:        # the measured table has this shape
                continue
            tune_cache[key] = gemm_tune(d, reps)
            measured += 1
        tm, tn, sk, stg = tune_cache[key][:4]
        old = (d.tile_m, d.tile_n, d.splitk, d.stages)
        d.tile_m, d.tile_n, d.splitk, d.stages = tm, tn, sk, stg
        if _lib.load().mdx_gemm_check(ctypes.byref(d)) != 0:      # a cached form this descriptor cannot take (e.g. a loaded cache)
            d.tile_m, d.tile_n, d.splitk, d.stages = old
    return measured


def release_tune_scratch():
    _tune_flush.clear()


TUNE_CACHE_VERSION = 2      # bump when gemm_shape_key changes: entries keyed the old way can never match and are dropped on load


def save_tune_cache(path):
    import json
    with open(path, "w") as f:
        json.dump({"version": TUNE_CACHE_VERSION, "key_fields": 10,
                   "entries": [[list(k), list(v)] for k, v in sorted(tune_cache.items())]}, f)


def load_tune_cache(path):
    """Returns the number of entries taken.  A file written under another key layout (no / other version, other key length) is
    ignored with a message: its keys would never match and every shape would silently be measured again."""
    import json
    import warnings
    with open(path) as f:
        data = json.load(f)
    if not isinstance(data, dict) or data.get("version") != TUNE_CACHE_VERSION:
        warnings.warn(f"load_tune_cache: {path} was written under another key layout (version "
                      f"{data.get('version') if isinstance(data, dict) else 'none'}, this build: {TUNE_CACHE_VERSION}); ignored")
        return 0
    n = 0
    for k, v in data["entries"]:
        if len(k) != 10:
            continue
        tune_cache[tuple(k)] = tuple(v)
        n += 1
    return n


def gemm_run(desc):
    _lib.check(_lib.load().mdx_gemm_f16(ctypes.byref(desc), _stream()), "mdx_gemm_f16")


def gemm(a, w, N, B, H, W, c1, out=None, **kw):
    """Convenience one-shot (tests): allocates output (row-major [M, out_cols]) and split-K workspace."""
    _chk(a, f16, "a"); _chk(w, f16, "w")
    ksize, stride, upsample = kw.get("ksize", 1), kw.get("stride", 1), kw.get("upsample", 0)
    Hs, Ws = (2 * H, 2 * W) if upsample else (H, W)
    pad = 1 if ksize == 3 else 0
    Ho = (Hs + 2 * pad - ksize) // stride + 1
    Wo = (Ws + 2 * pad - ksize) // stride + 1
    M = B * Ho * Wo
    epi = kw.get("epilogue", EPI_NONE)
    out_mode = kw.get("out_mode", OUT_ROWMAJOR)
    if out is None:
        if out_mode == OUT_TRANSPOSED:
            ld = kw.pop("out_ld", Ho * Wo)
            out = torch.zeros((B, N, ld), dtype=f16, device=a.device)
        elif out_mode == OUT_D2S2:
            ld = kw.pop("out_ld", N // 4)
            out = torch.empty((B, 2 * Ho, 2 * Wo, ld), dtype=f16, device=a.device)
        else:
            cols = N // 2 if epi == EPI_GEGLU else N
            ld = kw.pop("out_ld", cols)
            out = torch.empty((M, ld), dtype=f16, device=a.device)
    else:
        ld = kw.pop("out_ld")
    d = make_gemm_desc(a, w, N, B, H, W, c1, out, ld, **kw)
    if not d.workspace:
        need = gemm_workspace_bytes(d)
        if need:
            ws = new_gemm_workspace(need, a.device)
            d.workspace = ws.data_ptr()
            d.workspace_bytes = need
    gemm_run(d)
    return out


def attention(q_ptr, k_ptr, vt_ptr, o_ptr, B, heads, D, Nq, Nk, scale, q_bs, q_ld, k_bs, k_ld, vt_bs, vt_ld, o_bs, o_ld,
              causal=False, ws=None, kv_splits=0):
    """Raw-pointer form (q/k may be column slices of one fused projection buffer); see include/mdx.h.
    `ws`: a zero-initialised uint8 workspace tensor (attention_workspace) -> the split-KV form, `kv_splits` 0 = auto."""
    lib = _lib.load()
    if ws is not None and not causal:
        _lib.check(lib.mdx_attention_splitkv_f16(
            ctypes.c_void_p(q_ptr), q_bs, q_ld, ctypes.c_void_p(k_ptr), k_bs, k_ld, ctypes.c_void_p(vt_ptr), vt_bs, vt_ld,
            ctypes.c_void_p(o_ptr), o_bs, o_ld, B, heads, D, Nq, Nk, float(scale), int(kv_splits), ctypes.c_void_p(ws.data_ptr()),
            ws.numel() * ws.element_size(), _stream()), "mdx_attention_splitkv_f16")
        return
    fn = lib.mdx_attention_causal_f16 if causal else lib.mdx_attention_f16
    _lib.check(fn(ctypes.c_void_p(q_ptr), q_bs, q_ld, ctypes.c_void_p(k_ptr), k_bs, k_ld, ctypes.c_void_p(vt_ptr), vt_bs,
                  vt_ld, ctypes.c_void_p(o_ptr), o_bs, o_ld, B, heads, D, Nq, Nk, float(scale), _stream()),
               "mdx_attention_causal_f16" if causal else "mdx_attention_f16")


def attention_ws_bytes(B, heads, D, Nq, Nk):
    """Bytes of workspace the library's own split choice needs for this shape (0: it would not split)."""
    return int(_lib.load().mdx_attention_ws_bytes(B, heads, D, Nq, Nk))


def attention_workspace(nbytes, device):
    """Zeroed workspace for the split-KV attention: the arrival counters at its head must be zero on the first use and every
    launch leaves them zero, so ONE workspace serves all attention launches of a plan (one stream) in turn."""
    return torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def timestep_embedding(t, dim, max_period=10000.0, out=None):
    _chk(t, f32, "t")
    M = t.shape[0]
    if out is None:
        out = torch.empty((M, dim), dtype=f32, device=t.device)
    _lib.check(_lib.load().mdx_timestep_embedding_f32(_ptr(t), _ptr(out), M, dim, float(max_period), _stream()),
               "mdx_timestep_embedding_f32")
    return out


def dense_small(x, w, b, act_in=False, act_out=False, out=None):
    """out[M,N] = act_out(act_in(x) @ w^T + b); x/out fp32, w fp16 [N,K]."""
    _chk(x, f32, "x"); _chk(w, f16, "w"); _chk(b, f32, "b")
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=f32, device=x.device)
    _lib.check(_lib.load().mdx_dense_small_f32(_ptr(x), x.stride(0), _ptr(w), _ptr(b), _ptr(out), out.stride(0), M, N, K,
                                               int(act_in), int(act_out), _stream()), "mdx_dense_small_f32")
    return out


def _step_args(B, olds, coef=None, factor_out=None):
    """What the eps-family step wrappers share: the three history pointers (olds padded with None), the coef4 array (None for
    the entries whose coefficients live on the device; the caller keeps it alive over the call) and the factor_out check."""
    o = [_ptr(t) for t in list(olds) + [None] * (3 - len(olds))]
    c4 = None if coef is None else ctypes.cast((ctypes.c_float * 4)(*[float(v) for v in coef]), ctypes.c_void_p)
    if factor_out is not None:
        _chk(factor_out, f32, "factor_out")
        if factor_out.numel() < B:
            raise _lib.MdxError(f"factor_out: needs {B} elements, has {factor_out.numel()}")
    return o, c4


def sampler_step(x, eps_u, eps_c, eps_ld, cfg_scale, olds, coef, sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef,
                 sigma, noise, e_t_out, x_prev, pred_x0):
    """Fused CFG + multistep mix + DDIM update (see include/mdx.h)."""
    B, C, H, W = x.shape
    o, c4 = _step_args(B, olds, coef)
    _lib.check(_lib.load().mdx_sampler_step_f32(
        _ptr(x), _ptr(eps_u), _ptr(eps_c), int(eps_ld), float(cfg_scale), *o, c4, float(sqrt_at), float(sqrt_one_minus_at),
        float(sqrt_a_prev), float(dir_coef), float(sigma), _ptr(noise), _ptr(e_t_out), _ptr(x_prev), _ptr(pred_x0), B, C, H, W, _stream()),
        "mdx_sampler_step_f32")


PRED_EPS, PRED_V = 0, 1     # MDX_PRED_* of include/mdx.h


def sampler_step_pred(x, x_model, out_u, out_c, out_ld, cfg_scale, pred_type, sqrt_at_model, sqrt_one_minus_at_model,
                      olds, coef, sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma, noise, e_t_out, x_prev,
                      pred_x0):
    """sampler_step for a model whose output is eps (PRED_EPS) or v (PRED_V): the v -> eps conversion at the point
    (x_model, sqrt_at_model, sqrt_one_minus_at_model) the model was evaluated at is part of the same launch (see
    include/mdx.h).  x_model None = x."""
    B, C, H, W = x.shape
    o, c4 = _step_args(B, olds, coef)
    _lib.check(_lib.load().mdx_sampler_step_pred_f32(
        _ptr(x), _ptr(x_model), _ptr(out_u), _ptr(out_c), int(out_ld), float(cfg_scale), int(pred_type),
        float(sqrt_at_model), float(sqrt_one_minus_at_model), *o, c4, float(sqrt_at), float(sqrt_one_minus_at),
        float(sqrt_a_prev), float(dir_coef), float(sigma), _ptr(noise), _ptr(e_t_out), _ptr(x_prev), _ptr(pred_x0), B, C, H, W, _stream()),
        "mdx_sampler_step_pred_f32")


def sampler_step_rescale(x, x_model, out_u, out_c, out_ld, cfg_scale, pred_type, sqrt_at_model, sqrt_one_minus_at_model,
                         olds, coef, sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma, noise, e_t_out, x_prev,
                         pred_x0, guidance_rescale, factor_out=None):
    """sampler_step_pred with guidance rescale: the CFG-combined model output of sample b is scaled by
    f[b] = guidance_rescale * std(out_c[b]) / std(m[b]) + (1 - guidance_rescale) inside the same launch (see
    include/mdx.h).  factor_out: optional [B] fp32 tensor that receives f."""
    B, C, H, W = x.shape
    o, c4 = _step_args(B, olds, coef, factor_out)
    _lib.check(_lib.load().mdx_sampler_step_rescale_f32(
        _ptr(x), _ptr(x_model), _ptr(out_u), _ptr(out_c), int(out_ld), float(cfg_scale), int(pred_type),
        float(sqrt_at_model), float(sqrt_one_minus_at_model), *o, c4, float(sqrt_at), float(sqrt_one_minus_at),
        float(sqrt_a_prev), float(dir_coef), float(sigma), _ptr(noise), _ptr(e_t_out), _ptr(x_prev), _ptr(pred_x0), float(guidance_rescale), _ptr(factor_out),
        B, C, H, W, _stream()), "mdx_sampler_step_rescale_f32")


def _chk_out_m(fn, out_m, out_c, mid_scale):
    """The middle branch of three-branch guidance: out_c's dtype, shape and ld, and a scale to go with it."""
    _chk(out_m, f16, "out_m")
    if out_c is None or tuple(out_m.shape) != tuple(out_c.shape):
        raise _lib.MdxError(f"out_m: expected out_c's shape {None if out_c is None else tuple(out_c.shape)}, "
                            f"got {tuple(out_m.shape)}")
    if mid_scale is None:
        raise _lib.MdxError(f"{fn}: out_m needs a mid_scale")


def sampler_step_dual(x, x_model, out_u, out_m, out_c, out_ld, cfg_scale, mid_scale, pred_type, sqrt_at_model,
                      sqrt_one_minus_at_model, olds, coef, sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma, noise,
                      e_t_out, x_prev, pred_x0, guidance_rescale=0., factor_out=None):
    """sampler_step_rescale with three-branch guidance (mdx_sampler_step_dual_f32): the combined model output is
    out_u + mid_scale (out_m - out_u) + cfg_scale (out_c - out_m), in the same ONE launch; the rescale pulls it to
    std(out_c).  out_m: the middle output (empty text, image latent), with out_c's dtype, shape and ld; None is
    sampler_step_rescale, launch for launch."""
    B, C, H, W = x.shape
    o, c4 = _step_args(B, olds, coef, factor_out)
    if out_m is not None:
        _chk_out_m("sampler_step_dual", out_m, out_c, mid_scale)
    _lib.check(_lib.load().mdx_sampler_step_dual_f32(
        _ptr(x), _ptr(x_model), _ptr(out_u), _ptr(out_c), int(out_ld), float(cfg_scale), int(pred_type),
        float(sqrt_at_model), float(sqrt_one_minus_at_model), *o, c4, float(sqrt_at), float(sqrt_one_minus_at),
        float(sqrt_a_prev), float(dir_coef), float(sigma), _ptr(noise), _ptr(e_t_out), _ptr(x_prev), _ptr(pred_x0), float(guidance_rescale), _ptr(factor_out),
        _ptr(out_m), 0. if mid_scale is None else float(mid_scale), B, C, H, W, _stream()), "mdx_sampler_step_dual_f32")


def sampler_update(x, out_u, out_c, cfg_scale, pred_type, olds, coef, update, guidance_rescale=0., x_model=None,
                   sqrt_at_model=1., sqrt_one_minus_at_model=0., out_m=None, mid_scale=None):
    """The one fused step launch of every LDM sampler, through the entry that does no more than the step needs: the rescale
    entry iff guidance_rescale != 0 and there is an unconditional half to combine, else the pred entry iff the model output
    is v, else the plain entry (bit-identical where they overlap, include/mdx.h).  out_u / out_c: the halves of the model
    output (out_u None: no guidance); (x_model, sqrt_at_model, sqrt_one_minus_at_model): the point the model was evaluated
    at, read for a v output only (x_model None = x); update: (sqrt_at, sqrt_one_minus_at, sqrt_a_prev, dir_coef, sigma, noise,
    e_t_out, x_prev, pred_x0) of sampler_step.  out_m (with mid_scale): the middle output of three-branch guidance -- only then
    the dual entry, which carries rescale and v itself."""
    v = pred_type == PRED_V
    if out_m is not None:
        sampler_step_dual(x, x_model, out_u, out_m, out_c, out_c.shape[-1], cfg_scale, mid_scale, pred_type,
                          sqrt_at_model if v else 1., sqrt_one_minus_at_model if v else 0., olds, coef, *update,
                          guidance_rescale=guidance_rescale)
    elif guidance_rescale != 0. and out_u is not None:
        sampler_step_rescale(x, x_model, out_u, out_c, out_c.shape[-1], cfg_scale, pred_type, sqrt_at_model if v else 1.,
                             sqrt_one_minus_at_model if v else 0., olds, coef, *update, guidance_rescale)
    elif v:
        sampler_step_pred(x, x_model, out_u, out_c, out_c.shape[-1], cfg_scale, pred_type, sqrt_at_model,
                          sqrt_one_minus_at_model, olds, coef, *update)
    else:
        sampler_step(x, out_u, out_c, out_c.shape[-1], cfg_scale, olds, coef, *update)


STEP_ROW = 16               # MDX_STEP_* of include/mdx.h: the floats of one sample's row, and where each scalar sits in it
(STEP_ACTIVE, STEP_CFG_SCALE, STEP_RESCALE, STEP_SQRT_AT_MODEL, STEP_SQRT_ONE_MINUS_AT_MODEL, STEP_C0) = range(6)
(STEP_SQRT_AT, STEP_SQRT_ONE_MINUS_AT, STEP_SQRT_A_PREV, STEP_DIR_COEF, STEP_SIGMA) = range(9, 14)


def sampler_step_table(x, x_model, out_u, out_c, pred_type, olds, noise, e_t_out, x_prev, pred_x0, table, any_rescale,
                       factor_out=None):
    """The fused step with every per-sample scalar read from row b of `table` ([B, STEP_ROW] fp32 on the device, a slice of
    a larger tensor is fine): samples of one batch with their own guidance scale, guidance rescale and schedule point, an
    inactive row just carried over to x_prev (see include/mdx.h).  any_rescale: whether some active row has a non-zero
    guidance rescale.  The table's values are the builder's to check (StepTable); nothing here syncs."""
    B, C, H, W = x.shape
    _chk(table, f32, "table")
    if tuple(table.shape) != (B, STEP_ROW):
        raise _lib.MdxError(f"table: expected [{B}, {STEP_ROW}], got {tuple(table.shape)}")
    o, _ = _step_args(B, olds, factor_out=factor_out)
    _lib.check(_lib.load().mdx_sampler_step_table_f32(
        _ptr(x), _ptr(x_model), _ptr(out_u), _ptr(out_c), int(out_c.shape[-1]), int(pred_type), *o, _ptr(noise),
        _ptr(e_t_out), _ptr(x_prev), _ptr(pred_x0), _ptr(table), int(bool(any_rescale)), _ptr(factor_out), B, C, H, W, _stream()), "mdx_sampler_step_table_f32")


VALUE_X0, VALUE_EPS = 0, 1     # MDX_VALUE_* of include/mdx.h


def _step_lin_args(fn, x_base, x_model, out_u, out_c, cfg_scale, pred_type, guidance_rescale, value_type, alpha_m, sigma_m, h1,
                   h2, A, c0, c1, c2, model_out, x_out, thresholding, max_val, model_pre_out, thr_out, factor_out):
    """The checks of both step launches of the solver and the arguments they share, up to factor_out."""
    _chk(x_base, f32, "x_base")
    if x_base.dim() != 4:
        raise _lib.MdxError(f"x_base: expected [B, C, H, W], got {tuple(x_base.shape)}")
    B, C, H, W = x_base.shape
    if x_model is None:
        x_model = x_base
    if out_c is None or model_out is None or x_out is None:
        raise _lib.MdxError(f"{fn}: out_c, model_out and x_out are required")
    for name, t in (("x_model", x_model), ("h1", h1), ("h2", h2), ("model_out", model_out), ("x_out", x_out),
                    ("model_pre_out", model_pre_out)):
        _chk(t, f32, name)
        if t is not None and tuple(t.shape) != (B, C, H, W):
            raise _lib.MdxError(f"{name}: expected {(B, C, H, W)}, got {tuple(t.shape)}")
    ld = int(out_c.shape[-1])
    for name, t in (("out_u", out_u), ("out_c", out_c)):
        _chk(t, f16, name)
        if t is not None and (int(t.shape[-1]) != ld or t.numel() != B * H * W * ld or ld < C):
            raise _lib.MdxError(f"{name}: expected NHWC fp16 [{B}, {H * W}, {ld} >= {C}], got {tuple(t.shape)}")
    for name, t in (("thr_out", thr_out), ("factor_out", factor_out)):
        _chk(t, f32, name)
        if t is not None and t.numel() < B:
            raise _lib.MdxError(f"{name}: needs {B} elements, has {t.numel()}")
    return (_ptr(x_base), _ptr(x_model), _ptr(out_u), _ptr(out_c), ld, float(cfg_scale), int(pred_type), float(guidance_rescale),
            int(value_type), float(alpha_m), float(sigma_m), int(bool(thresholding)), float(max_val), _ptr(h1), _ptr(h2), float(A),
            float(c0), float(c1), float(c2), _ptr(model_out), _ptr(x_out), _ptr(model_pre_out), _ptr(thr_out), _ptr(factor_out))


def sampler_step_lin(x_base, x_model, out_u, out_c, cfg_scale, pred_type, guidance_rescale, value_type, alpha_m, sigma_m,
                     h1, h2, A, c0, c1, c2, model_out, x_out, thresholding=False, max_val=1., model_pre_out=None, thr_out=None,
                     factor_out=None):
    """The step launch of the whole DPM-Solver (see include/mdx.h): the model value `model_out` -- the data prediction
    (VALUE_X0, dynamically thresholded at `max_val` if `thresholding`) or the noise prediction (VALUE_EPS) from the UNet
    output halves out_u / out_c evaluated on x_model at the schedule point (alpha_m, sigma_m), after the CFG combine, the
    guidance rescale and the v -> eps conversion -- and x_out = A x_base + c0 model_out + c1 h1 + c2 h2, in ONE launch.  A term
    with a coefficient of exactly 0 is skipped (h1 / h2 may then be None).  x_out may be x_base and / or x_model; nothing else
    may overlap.  Optional outputs: model_pre_out (the value before thresholding), thr_out [B] (the threshold s), factor_out
    [B] (the rescale factor).  Every tensor's dtype, layout and extent is checked here: the library sees pointers only."""
    _lib.check(_lib.load().mdx_sampler_step_lin_f32(
        *_step_lin_args("sampler_step_lin", x_base, x_model, out_u, out_c, cfg_scale, pred_type, guidance_rescale, value_type,
                        alpha_m, sigma_m, h1, h2, A, c0, c1, c2, model_out, x_out, thresholding, max_val, model_pre_out, thr_out,
                        factor_out), *x_base.shape, _stream()), "mdx_sampler_step_lin_f32")


def _step_lin_noise_args(fn, x_base, noise, seeds, stream, draw):
    """The checks of the noise sources of a stochastic step launch; returns (noise, seeds, stream, draw) as the library takes them."""
    B = int(x_base.shape[0])
    _chk(noise, f32, "noise")
    if noise is not None and tuple(noise.shape) != tuple(x_base.shape):
        raise _lib.MdxError(f"noise: expected {tuple(x_base.shape)}, got {tuple(noise.shape)}")
    if seeds is not None:
        if not (isinstance(seeds, torch.Tensor) and tuple(seeds.shape) == (B,)):
            raise _lib.MdxError(f"{fn}: seeds must be a [{B}] int64 device tensor (ops.seeds_tensor)")
        _chk(seeds, torch.int64, "seeds")
    stream = RNG_STEP if stream is None else int(stream)
    if not (0 <= stream < (1 << 31) and 0 <= int(draw) < (1 << 32)):
        raise _lib.MdxError(f"{fn}: stream must be in [0, 2^31) and draw in [0, 2^32), got {stream!r}, {draw!r}")
    return _ptr(noise), _ptr(seeds), stream, int(draw)


def sampler_step_lin_noise(x_base, x_model, out_u, out_c, cfg_scale, pred_type, guidance_rescale, value_type, alpha_m, sigma_m,
                           h1, h2, A, c0, c1, c2, model_out, x_out, cn, noise=None, seeds=None, stream=None, draw=0,
                           thresholding=False, max_val=1., model_pre_out=None, thr_out=None, factor_out=None):
    """sampler_step_lin for a stochastic update (mdx_sampler_step_lin_noise_f32): the same launch with x_out += cn * z, z ~
    N(0, 1) from exactly one source -- `noise` [B, C, H, W] fp32, or `seeds` (ops.seeds_tensor, [B]): then z is drawn inside
    the launch, the bits randn_seeded(seeds, stream, draw, (C, H, W)) would store, and sample b's noise depends on seeds[b]
    alone.  stream: None = RNG_STEP.  cn == 0 is sampler_step_lin bit for bit and reads neither source.  noise may overlap no
    output."""
    args = _step_lin_args("sampler_step_lin_noise", x_base, x_model, out_u, out_c, cfg_scale, pred_type, guidance_rescale,
                          value_type, alpha_m, sigma_m, h1, h2, A, c0, c1, c2, model_out, x_out, thresholding, max_val,
                          model_pre_out, thr_out, factor_out)
    nz = _step_lin_noise_args("sampler_step_lin_noise", x_base, noise, seeds, stream, draw)
    _lib.check(_lib.load().mdx_sampler_step_lin_noise_f32(*args, float(cn), *nz, *x_base.shape, _stream()),
               "mdx_sampler_step_lin_noise_f32")


def sampler_step_lin_dual(x_base, x_model, out_u, out_m, out_c, cfg_scale, mid_scale, pred_type, guidance_rescale, value_type,
                          alpha_m, sigma_m, h1, h2, A, c0, c1, c2, model_out, x_out, cn=0., noise=None, seeds=None, stream=None,
                          draw=0, thresholding=False, max_val=1., model_pre_out=None, thr_out=None, factor_out=None):
    """sampler_step_lin_noise with three-branch guidance (mdx_sampler_step_lin_dual_f32): step 1 is
    out_u + mid_scale (out_m - out_u) + cfg_scale (out_c - out_m), everything after it unchanged, ONE launch.  out_m: the
    middle output (empty text, image latent), with out_c's dtype, shape and ld; it may overlap no output.  None is
    sampler_step_lin_noise, launch for launch."""
    args = _step_lin_args("sampler_step_lin_dual", x_base, x_model, out_u, out_c, cfg_scale, pred_type, guidance_rescale,
                          value_type, alpha_m, sigma_m, h1, h2, A, c0, c1, c2, model_out, x_out, thresholding, max_val,
                          model_pre_out, thr_out, factor_out)
    nz = _step_lin_noise_args("sampler_step_lin_dual", x_base, noise, seeds, stream, draw)
    if out_m is not None:
        _chk_out_m("sampler_step_lin_dual", out_m, out_c, mid_scale)
    _lib.check(_lib.load().mdx_sampler_step_lin_dual_f32(*args, float(cn), *nz, _ptr(out_m),
                                                         0. if mid_scale is None else float(mid_scale), *x_base.shape,
                                                         _stream()), "mdx_sampler_step_lin_dual_f32")


def sampler_step_pc(x_base, x_model, out_u, out_c, cfg_scale, pred_type, guidance_rescale, value_type, alpha_m, sigma_m,
                    h1, h2, h3, corrector, predictor, model_out, x_corr_out, x_pred_out, thresholding=False, max_val=1.,
                    model_pre_out=None, thr_out=None, factor_out=None):
    """The step launch of UniPC (mdx_sampler_step_pc_f32, see include/mdx.h): sampler_step_lin's model value `model_out`, then
    x_corr_out = Ac x_base + d0 model_out + d1 h1 + d2 h2 + d3 h3 with corrector = (Ac, d0, d1, d2, d3) -- or, with corrector
    None, x_model's bits -- and x_pred_out = Ap x_corr_out + e0 model_out + e1 h1 + e2 h2 with predictor = (Ap, e0, e1, e2), in
    ONE launch.  A term with a coefficient of exactly 0 is skipped (its tensor may be None; x_base may be None without a
    corrector).  x_corr_out may be x_base and x_pred_out may be x_model; nothing else may overlap."""
    if x_model is None:
        raise _lib.MdxError("sampler_step_pc: x_model is required")
    if x_corr_out is None or x_pred_out is None:
        raise _lib.MdxError("sampler_step_pc: x_corr_out and x_pred_out are required")
    for name, t in (("x_base", x_base), ("h3", h3), ("x_pred_out", x_pred_out)):
        _chk(t, f32, name)
        if t is not None and tuple(t.shape) != tuple(x_model.shape):
            raise _lib.MdxError(f"{name}: expected {tuple(x_model.shape)}, got {tuple(t.shape)}")
    if len(predictor) != 4 or (corrector is not None and len(corrector) != 5):
        raise _lib.MdxError("sampler_step_pc: corrector is None or (Ac, d0, d1, d2, d3), predictor is (Ap, e0, e1, e2)")
    Ac, d0, d1, d2, d3 = (0.,) * 5 if corrector is None else (float(v) for v in corrector)
    a = _step_lin_args("sampler_step_pc", x_model, x_model, out_u, out_c, cfg_scale, pred_type, guidance_rescale, value_type,
                       alpha_m, sigma_m, h1, h2, Ac, d0, d1, d2, model_out, x_corr_out, thresholding, max_val, model_pre_out,
                       thr_out, factor_out)
    _lib.check(_lib.load().mdx_sampler_step_pc_f32(
        _ptr(x_base), *a[1:15], _ptr(h3), int(corrector is not None), Ac, d0, d1, d2, float(d3),
        *(float(v) for v in predictor), a[19], a[20], _ptr(x_pred_out), *a[21:], *x_model.shape, _stream()),
        "mdx_sampler_step_pc_f32")


# ---- sampling sessions (include/mdx.h, "slots"): the samples of a batch are slots that requests enter and leave
def _chk_slots(B, slot_start, slot_len):
    for name, t in (("slot_start", slot_start), ("slot_len", slot_len)):
        _chk(t, torch.int32, name)
        if tuple(t.shape) != (B,):
            raise _lib.MdxError(f"{name}: expected [{B}] int32, got {tuple(t.shape)}")


def sampler_step_slots(x, x_model, out_u, out_c, pred_type, olds, noise, e_t_out, x_prev, pred_x0, sched, slot_start, slot_len,
                       tick, any_rescale, factor_out=None):
    """sampler_step_table with the row of sample b looked up per slot: sched [B, cap, STEP_ROW] fp32 holds the rows of the
    request in slot b, and at session tick `tick` the slot reads row tick - slot_start[b] if that lies in [0, slot_len[b]) and is
    an inactive row otherwise (see include/mdx.h).  any_rescale: whether some active slot's row has a non-zero guidance
    rescale -- the caller's host mirror knows; nothing here syncs."""
    B, C, H, W = x.shape
    _chk(sched, f32, "sched")
    if sched.dim() != 3 or sched.shape[0] != B or sched.shape[2] != STEP_ROW:
        raise _lib.MdxError(f"sched: expected [{B}, cap, {STEP_ROW}], got {tuple(sched.shape)}")
    _chk_slots(B, slot_start, slot_len)
    o, _ = _step_args(B, olds, factor_out=factor_out)
    _lib.check(_lib.load().mdx_sampler_step_slots_f32(
        _ptr(x), _ptr(x_model), _ptr(out_u), _ptr(out_c), int(out_c.shape[-1]), int(pred_type), *o, _ptr(noise), _ptr(e_t_out), _ptr(x_prev), _ptr(pred_x0), _ptr(sched), _ptr(slot_start), _ptr(slot_len),
        int(sched.shape[1]), int(tick), int(bool(any_rescale)), _ptr(factor_out), B, C, H, W, _stream()),
        "mdx_sampler_step_slots_f32")


def slot_gather(src, slot_start, slot_len, tick, out, reps=2):
    """out[r * B + b] = src[b, tick - slot_start[b]] for r < reps and every active slot b; the rows of the other slots are not
    written.  src [B, cap, n] fp32, out [reps * B, n] fp32.  One launch."""
    _chk(src, f32, "src"); _chk(out, f32, "out")
    if src.dim() != 3:
        raise _lib.MdxError(f"slot_gather: src must be [B, cap, n], got {tuple(src.shape)}")
    B, cap, n = (int(d) for d in src.shape)
    _chk_slots(B, slot_start, slot_len)
    if tuple(out.shape) != (int(reps) * B, n):
        raise _lib.MdxError(f"slot_gather: out has shape {tuple(out.shape)}, expected {(int(reps) * B, n)}")
    _lib.check(_lib.load().mdx_slot_gather_f32(_ptr(src), _ptr(slot_start), _ptr(slot_len), cap, int(tick), _ptr(out), B, n,
                                               int(reps), _stream()), "mdx_slot_gather_f32")
    return out


def probe_mfma(a, b):
    c = torch.empty((64, 16), dtype=f32, device=a.device)
    _lib.check(_lib.load().mdx_probe_mfma_32x32x16_f16(_ptr(a), _ptr(b), _ptr(c), _stream()), "mdx_probe_mfma")
    return c


def probe_mfma16(a, b):
    c = torch.empty((64, 4), dtype=f32, device=a.device)
    _lib.check(_lib.load().mdx_probe_mfma_16x16x32_f16(_ptr(a), _ptr(b), _ptr(c), _stream()), "mdx_probe_mfma16")
    return c


def pack_b_operand(src2d, out=None):
    """Row-major fp16 activation matrix [rows, K] (any row stride) -> packed B operand of mdx_gemm_f16."""
    rows, K = src2d.shape
    n = ((rows + 63) // 64) * ((K + 63) // 64) * 4096
    if out is None:
        out = torch.empty(n, dtype=f16, device=src2d.device)
    assert out.numel() >= n and src2d.stride(1) == 1
    _lib.check(_lib.load().mdx_pack_b_operand_f16(_ptr(src2d), src2d.stride(0), rows, K, _ptr(out), _stream()),
               "mdx_pack_b_operand_f16")
    return out


def softmax_rows(x2d, scale):
    """In place: x[r] = softmax(scale * x[r]) on fp16 scores [rows, cols]."""
    rows, cols = x2d.shape
    assert x2d.stride(1) == 1
    _lib.check(_lib.load().mdx_softmax_rows_f16(_ptr(x2d), x2d.stride(0), rows, cols, float(scale), _stream()),
               "mdx_softmax_rows_f16")
    return x2d


def srgan_conv_in(x, w, bias, slope, out=None):
    """SRGAN Generator.conv1 (srgan.py:83-85): fp32 NCHW image [B, 3, H, W] -> PReLU(conv9x9(x) + bias), NHWC fp16 [B, H, W, 64].
    w: fp16 [64, 3, 9, 9] (reference layout), bias / slope fp32 [64]."""
    _chk(x, f32, "x"); _chk(w, f16, "w"); _chk(bias, f32, "bias"); _chk(slope, f32, "slope")
    B, C, H, W = x.shape
    if out is None:
        out = torch.empty((B, H, W, 64), dtype=f16, device=x.device)
    _lib.check(_lib.load().mdx_srgan_conv_in_f16(_ptr(x), _ptr(w), _ptr(bias), _ptr(slope), _ptr(out), B, H, W, _stream()),
               "mdx_srgan_conv_in_f16")
    return out


def srgan_conv_out(x, w, bias, B, H, W, out=None):
    """SRGAN Generator.conv3 + tanh (srgan.py:115-116): NHWC fp16 [B, H, W, 64] -> tanh(conv9x9(x) + bias), fp32 NCHW [B, 3, H, W].
    w: fp16 [3, 64, 9, 9] (reference layout), bias fp32 [3]."""
    _chk(x, f16, "x"); _chk(w, f16, "w"); _chk(bias, f32, "bias")
    if out is None:
        out = torch.empty((B, 3, H, W), dtype=f32, device=x.device)
    _lib.check(_lib.load().mdx_srgan_conv_out_f32(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), B, H, W, _stream()),
               "mdx_srgan_conv_out_f32")
    return out


def vae_gaussian_sample(moments, zc, noise, out):
    """moments NHWC fp16 [B, HW, ld]; noise / out NCHW fp32 [B, zc, h, w] (noise None -> the mode)."""
    B, HW, ld = moments.shape
    _lib.check(_lib.load().mdx_vae_gaussian_sample_f32(_ptr(moments), ld, _ptr(noise), _ptr(out), B, zc, HW, _stream()),
               "mdx_vae_gaussian_sample_f32")
    return out


def _same_shape(ref, name, t):
    if t is not None and tuple(t.shape) != tuple(ref.shape):
        raise _lib.MdxError(f"{name}: shape {tuple(t.shape)}, expected {tuple(ref.shape)}")


def q_sample(x0, noise, a, b, out=None, mask=None, img=None):
    """out = a * x0 + b * noise (ddpm.py:197-200); with `mask` [B, 1 | C, H, W] the result is blended into the running latent
    `img`: out = mask * q + (1 - mask) * img (plms.py:153-157).  NCHW fp32; `out` may be `img` itself (in place) and no other
    input.  One launch (include/mdx.h: mdx_q_sample_f32)."""
    _chk(x0, f32, "x0"); _chk(noise, f32, "noise"); _chk(mask, f32, "mask"); _chk(img, f32, "img"); _chk(out, f32, "out")
    if x0.dim() != 4:
        raise _lib.MdxError(f"x0: expected [B, C, H, W], got shape {tuple(x0.shape)}")
    B, C, H, W = x0.shape
    if out is None:
        out = torch.empty_like(x0)
    _same_shape(x0, "noise", noise); _same_shape(x0, "img", img); _same_shape(x0, "out", out)
    mask_c = 0
    if mask is not None:
        if mask.dim() != 4 or mask.shape[0] != B or tuple(mask.shape[2:]) != (H, W):
            raise _lib.MdxError(f"mask: shape {tuple(mask.shape)}, expected [{B}, 1 or {C}, {H}, {W}]")
        mask_c = int(mask.shape[1])
    _lib.check(_lib.load().mdx_q_sample_f32(_ptr(x0), _ptr(noise), float(a), float(b), _ptr(mask), mask_c, _ptr(img),
                                            _ptr(out), B, C, H * W, _stream()), "mdx_q_sample_f32")
    return out


def vae_encode_noised(moments, zc, post_noise, scale_factor, a, b, noise, z0_out, xt_out):
    """Encoder moments NHWC fp16 [B, HW, ld] -> z0 = scale_factor * (mean + std * post_noise) and x_t = a * z0 + b * noise in
    one launch (include/mdx.h: mdx_vae_encode_noised_f32).  post_noise None: the mode; either output may be None."""
    _chk(moments, f16, "moments")
    for name, t in (("post_noise", post_noise), ("noise", noise), ("z0_out", z0_out), ("xt_out", xt_out)):
        _chk(t, f32, name)
    B, HW, ld = moments.shape
    ref = z0_out if z0_out is not None else xt_out
    if ref is not None:
        if ref.dim() != 4 or ref.shape[0] != B or ref.shape[1] != zc or ref.shape[2] * ref.shape[3] != HW:
            raise _lib.MdxError(f"vae_encode_noised: output shape {tuple(ref.shape)} does not match moments [{B}, {HW}, {ld}], "
                                f"zc = {zc}")
        for name, t in (("post_noise", post_noise), ("noise", noise), ("xt_out", xt_out)):
            _same_shape(ref, name, t)
    _lib.check(_lib.load().mdx_vae_encode_noised_f32(_ptr(moments), ld, _ptr(post_noise), float(scale_factor), float(a),
                                                     float(b), _ptr(noise), _ptr(z0_out), _ptr(xt_out), B, zc, HW, _stream()),
               "mdx_vae_encode_noised_f32")
    return z0_out, xt_out


# ---------------------------------------------------------------------------------------------------------------
# Inpainting: the work around the sampler (include/mdx.h: mdx_inpaint_* / mdx_mask_feather_f32, csrc/inpaint.hip).
# A mask value >= 0.5 is the hole; a mask (or alpha) of batch 1 is shared by the whole batch.
FEATHER_MAX_RADIUS = 48
_FEATHER_TAPS = {}


def _plane_mask(name, t, B, H, W):
    """[1 | B, 1, H, W] fp32 -> its batch."""
    _chk(t, f32, name)
    if t.dim() != 4 or t.shape[0] not in (1, B) or tuple(t.shape[1:]) != (1, H, W):
        raise _lib.MdxError(f"{name}: shape {tuple(t.shape)}, expected [1 or {B}, 1, {H}, {W}]")
    return int(t.shape[0])


def inpaint_mask_image(image, mask, out=None):
    """image * (mask < 0.5) (inpaint.py:55): image [B, C, H, W], mask [1 | B, 1, H, W], NCHW fp32.  One launch."""
    _chk(image, f32, "image"); _chk(out, f32, "out")
    if image.dim() != 4:
        raise _lib.MdxError(f"image: expected [B, C, H, W], got shape {tuple(image.shape)}")
    B, C, H, W = image.shape
    mask_b = _plane_mask("mask", mask, B, H, W)
    if out is None:
        out = torch.empty_like(image)
    _same_shape(image, "out", out)
    _lib.check(_lib.load().mdx_inpaint_mask_image_f32(_ptr(image), _ptr(mask), mask_b, _ptr(out), B, C, H * W, _stream()),
               "mdx_inpaint_mask_image_f32")
    return out


def inpaint_concat(moments, zc, post_noise, scale_factor, mask, hw, out=None):
    """c_concat [B, 1 + zc, h, w] of the hybrid UNet in one launch (inpaint.py:76-85): channel 0 the binarised mask
    [1 | B, 1, H, W] at the latent grid hw = (h, w) (nearest, integer arithmetic), channels 1.. scale_factor * the posterior
    sample of the encoder moments NHWC fp16 [B, h * w, ld] (post_noise [B, zc, h, w], None: the mode) -- bit for bit
    vae_encode_noised's z0."""
    _chk(moments, f16, "moments"); _chk(post_noise, f32, "post_noise"); _chk(out, f32, "out")
    B, HW, ld = moments.shape
    h, w = int(hw[0]), int(hw[1])
    if h * w != HW:
        raise _lib.MdxError(f"inpaint_concat: latent grid {h} x {w} does not match moments [{B}, {HW}, {ld}]")
    if mask.dim() != 4:
        raise _lib.MdxError(f"mask: expected [1 or {B}, 1, H, W], got shape {tuple(mask.shape)}")
    H, W = int(mask.shape[2]), int(mask.shape[3])
    mask_b = _plane_mask("mask", mask, B, H, W)
    if out is None:
        out = torch.empty((B, 1 + zc, h, w), dtype=f32, device=moments.device)
    elif tuple(out.shape) != (B, 1 + zc, h, w):
        raise _lib.MdxError(f"out: shape {tuple(out.shape)}, expected {(B, 1 + zc, h, w)}")
    if post_noise is not None and tuple(post_noise.shape) != (B, zc, h, w):
        raise _lib.MdxError(f"post_noise: shape {tuple(post_noise.shape)}, expected {(B, zc, h, w)}")
    _lib.check(_lib.load().mdx_inpaint_concat_f32(_ptr(moments), ld, _ptr(post_noise), float(scale_factor), _ptr(mask), mask_b,
                                                  H, W, _ptr(out), B, zc, h, w, _stream()), "mdx_inpaint_concat_f32")
    return out


def inpaint_resize_mask(mask, hw, out=None):
    """The binarised mask [Bm, 1, H, W] at the grid hw = (h, w), [Bm, 1, h, w]: channel 0 of inpaint_concat alone (zc = 0)."""
    if mask.dim() != 4:
        raise _lib.MdxError(f"mask: expected [B, 1, H, W], got shape {tuple(mask.shape)}")
    Bm, _, H, W = mask.shape
    _plane_mask("mask", mask, Bm, H, W); _chk(out, f32, "out")
    h, w = int(hw[0]), int(hw[1])
    if out is None:
        out = torch.empty((Bm, 1, h, w), dtype=f32, device=mask.device)
    elif tuple(out.shape) != (Bm, 1, h, w):
        raise _lib.MdxError(f"out: shape {tuple(out.shape)}, expected {(Bm, 1, h, w)}")
    _lib.check(_lib.load().mdx_inpaint_concat_f32(None, 0, None, 1.0, _ptr(mask), Bm, H, W, _ptr(out), Bm, 0, h, w, _stream()),
               "mdx_inpaint_concat_f32")
    return out


def feather_weights(sigma):
    """(radius, taps): radius = ceil(3 sigma), the 2 radius + 1 normalised Gaussian taps computed in float64, as fp32."""
    sigma = float(sigma)
    if not 0.0 < sigma < float("inf"):
        raise ValueError(f"mask_blur (the Gaussian's sigma, in pixels) must be positive and finite, got {sigma!r}")
    radius = int(math.ceil(3.0 * sigma))
    if radius > FEATHER_MAX_RADIUS:
        raise ValueError(f"mask_blur {sigma!r} needs a radius of {radius} pixels; the feather kernel takes at most "
                         f"{FEATHER_MAX_RADIUS} (sigma <= {FEATHER_MAX_RADIUS // 3})")
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    wts = np.exp(-0.5 * (k / sigma) ** 2)
    return radius, (wts / wts.sum()).astype(np.float32)


def mask_feather(mask, sigma, out=None):
    """alpha = max(m, G * m) [Bm, 1, H, W]: the binarised mask, widened outward by a separable Gaussian of `sigma` pixels with
    replicate edges (exactly 1 on the hole).  One launch."""
    _chk(mask, f32, "mask"); _chk(out, f32, "out")
    if mask.dim() != 4 or mask.shape[1] != 1:
        raise _lib.MdxError(f"mask: expected [B, 1, H, W], got shape {tuple(mask.shape)}")
    radius, wts = feather_weights(sigma)
    Bm, _, H, W = mask.shape
    if out is None:
        out = torch.empty_like(mask)
    _same_shape(mask, "out", out)
    key = (float(sigma), mask.device)
    if key not in _FEATHER_TAPS:        # the taps of a sigma are uploaded once per device
        _FEATHER_TAPS[key] = torch.from_numpy(wts).to(mask.device)
    wts = _FEATHER_TAPS[key]
    _lib.check(_lib.load().mdx_mask_feather_f32(_ptr(mask), _ptr(wts), radius, _ptr(out), Bm, H, W, _stream()),
               "mdx_mask_feather_f32")
    return out


def inpaint_composite(decoded, image=None, alpha=None, output="float", out_f32=None, out_u8=None):
    """The output stage after the decoder, one launch: clamp((alpha * decoded + (1 - alpha) * image + 1) / 2, 0, 1) as
    [B, C, H, W] fp32 (output "float"), as its truncation to [B, H, W, C] uint8 (output "uint8", inpaint.py:112-115), or as
    the pair (output "both").  alpha [1 | B, 1, H, W], None: 1 everywhere (image is then not needed).  out_f32 / out_u8: write
    into these instead of fresh tensors."""
    if output not in ("float", "uint8", "both"):
        raise ValueError(f"output must be 'float', 'uint8' or 'both', got {output!r}")
    _chk(decoded, f32, "decoded"); _chk(image, f32, "image")
    if decoded.dim() != 4:
        raise _lib.MdxError(f"decoded: expected [B, C, H, W], got shape {tuple(decoded.shape)}")
    B, C, H, W = decoded.shape
    alpha_b = 0
    if alpha is not None:
        if image is None:
            raise _lib.MdxError("inpaint_composite: alpha needs the image to composite with")
        _same_shape(decoded, "image", image)
        alpha_b = _plane_mask("alpha", alpha, B, H, W)
    _chk(out_f32, f32, "out_f32"); _chk(out_u8, torch.uint8, "out_u8")
    _same_shape(decoded, "out_f32", out_f32)
    if out_u8 is not None and tuple(out_u8.shape) != (B, H, W, C):
        raise _lib.MdxError(f"out_u8: shape {tuple(out_u8.shape)}, expected {(B, H, W, C)}")
    out_f = None if output == "uint8" else (torch.empty_like(decoded) if out_f32 is None else out_f32)
    out_u = None if output == "float" else (torch.empty((B, H, W, C), dtype=torch.uint8, device=decoded.device)
                                            if out_u8 is None else out_u8)
    _lib.check(_lib.load().mdx_inpaint_composite_f32(_ptr(decoded), _ptr(image), _ptr(alpha), alpha_b, _ptr(out_f), _ptr(out_u),
                                                     B, C, H, W, _stream()), "mdx_inpaint_composite_f32")
    return (out_f, out_u) if output == "both" else (out_f if out_u is None else out_u)


# ---------------------------------------------------------------------------------------------------------------
# Windowed UNet evaluation (include/mdx.h: mdx_window_gather_f32 / mdx_window_average_f16 and, for regions and wrap-around
# windows, mdx_window_gather_rows_f32 / mdx_window_average_regions_f16; csrc/window.hip).
def window_offsets(length, window, stride):
    """The offsets of one axis: 0, s, 2s, ... while o + w < L, then a last window at L - w (clamped, not padded);
    L == w: [0]."""
    length, window, stride = int(length), int(window), int(stride)
    if not 0 < window <= length:
        raise _lib.MdxError(f"window_offsets: a window of {window} on an axis of {length}")
    if not 0 < stride <= window:
        raise _lib.MdxError(f"window_offsets: stride {stride} must be in [1, window = {window}] (a larger one leaves pixels "
                            f"uncovered)")
    offs = []
    o = 0
    while o + window < length:
        offs.append(o)
        o += stride
    return offs + [length - window]


class _HostTable:
    """A host array the C entries validate and its device copy the kernels read, made on the first on(device), once."""

    def __init__(self, host):
        self.host = np.ascontiguousarray(host)
        self._ptr = ctypes.c_void_p(self.host.ctypes.data)       # (the array is written in place, never replaced)
        self._dev = {}

    def on(self, device):
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.host).to(device)
        return self._dev[device]

    def _host_ptr(self):
        return self._ptr


class WindowGrid(_HostTable):
    """The windows of one canvas: oy / ox (window_offsets per axis), window k = iy * nx + ix at (oy[iy], ox[ix]), and the
    int32 table [ny + nx] the kernels read -- on the host from construction, on a device from the first on(device), once.
    wrap_x: the x offsets are 0, s, 2s, ... while o < Wc (nx = ceil(Wc / s)) and a window at o covers the canvas columns
    (o + i) mod Wc, i < w: the left and the right edge of the canvas lie inside one window (a 360-degree panorama).  Rows never
    wrap.  A wrapped grid is read by window_gather_rows / window_average_regions only."""

    def __init__(self, canvas_hw, window_hw, stride_hw, wrap_x=False):
        (self.Hc, self.Wc), (self.h, self.w) = (int(v) for v in canvas_hw), (int(v) for v in window_hw)
        self.wrap_x = bool(wrap_x)
        self.oy = window_offsets(self.Hc, self.h, stride_hw[0])
        if self.wrap_x:
            window_offsets(self.Wc, self.w, stride_hw[1])            # (the same refusals: 0 < s <= w <= Wc)
            self.ox = list(range(0, self.Wc, int(stride_hw[1])))
        else:
            self.ox = window_offsets(self.Wc, self.w, stride_hw[1])
        self.ny, self.nx = len(self.oy), len(self.ox)
        self.N = self.ny * self.nx
        super().__init__(np.asarray(self.oy + self.ox, dtype=np.int32))

    def origin(self, k):
        return self.oy[k // self.nx], self.ox[k % self.nx]

    def columns(self, k):
        """The canvas columns of window k, in the window's own order (modulo Wc on a wrapped grid)."""
        return (self.ox[k % self.nx] + np.arange(self.w)) % self.Wc

    def coverage(self):
        """[Hc, Wc] int64: how many windows cover each canvas pixel (columns counted modulo Wc on a wrapped grid)."""
        cy, cx = np.zeros(self.Hc, np.int64), np.zeros(self.Wc, np.int64)
        for o in self.oy:
            cy[o:o + self.h] += 1
        for o in self.ox:
            cx[(o + np.arange(self.w)) % self.Wc] += 1
        return cy[:, None] * cx[None, :]


class _IntTable(_HostTable):
    """An int32 table of window, region or pair numbers."""

    def __init__(self, values):
        super().__init__(np.asarray(values, dtype=np.int32).reshape(-1))
        self.lo, self.hi = (int(self.host.min()), int(self.host.max())) if self.host.size else (0, -1)      # at construction

    def __len__(self):
        return int(self.host.shape[0])


class WindowRows(_IntTable):
    """A table of window numbers for window_gather_rows: any order, repeats allowed."""


class RegionPlan:
    """R regions on the canvas of `grid`: masks [R, Hc, Wc] fp32, finite, >= 0, their sum > 0 at every pixel, and the list of
    ACTIVE (window, region) pairs sorted by window then region -- (k, r) is active iff M_r is non-zero somewhere inside window
    k (wrap included) -- so a small region costs only the windows it touches, and a pixel with M_r > 0 has every covering
    window active for r (the denominator of the region mean is positive everywhere).  pair_window [P], pair_region [P] and the
    CSR index pair_first [N + 1] are held on the host (what the C entry validates) and, from on(device), on the device."""

    def __init__(self, grid, masks):
        m = torch.as_tensor(masks).detach().to("cpu", torch.float32)
        if m.dim() != 3 or tuple(m.shape[1:]) != (grid.Hc, grid.Wc) or m.shape[0] < 1:
            raise _lib.MdxError(f"RegionPlan: masks have shape {tuple(m.shape)}, expected [R >= 1, {grid.Hc}, {grid.Wc}]")
        a = np.ascontiguousarray(m.numpy())
        if not np.isfinite(a).all() or (a < 0).any():
            raise _lib.MdxError("RegionPlan: masks must be finite and >= 0")
        if not (a.sum(0, dtype=np.float64) > 0).all():
            raise _lib.MdxError("RegionPlan: the masks must sum to > 0 at every canvas pixel (a pixel no region claims has no "
                                "output)")
        self.grid, self.R = grid, int(a.shape[0])
        pw, pr, first = [], [], [0]
        for k in range(grid.N):
            oy = grid.oy[k // grid.nx]
            inside = a[:, oy:oy + grid.h][:, :, grid.columns(k)]
            for r in range(self.R):
                if inside[r].any():
                    pw.append(k)
                    pr.append(r)
            first.append(len(pw))
        self.pairs = list(zip(pw, pr))
        self.P = len(pw)
        self.pair_window, self.pair_region, self.pair_first = _IntTable(pw), _IntTable(pr), _IntTable(first)
        masks = _HostTable(a)
        self.masks_host, self.masks_on = masks.host, masks.on


def _clamped(grid, what):
    if grid.wrap_x:
        raise _lib.MdxError(f"{what}: a wrapped grid (wrap_x) is read by window_gather_rows / window_average_regions")


def _gather_dims(canvas, grid):
    """NB, C of a gather's canvas [NB, C, Hc, Wc]."""
    if canvas.dim() != 4 or tuple(canvas.shape[2:]) != (grid.Hc, grid.Wc):
        raise _lib.MdxError(f"canvas: shape {tuple(canvas.shape)}, expected [NB, C, {grid.Hc}, {grid.Wc}]")
    return int(canvas.shape[0]), int(canvas.shape[1])


def _window_out(out, shape, like):
    """The caller's `out` if it has `shape`, a fresh tensor of like's dtype and device without one."""
    if out is None:
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    if tuple(out.shape) != shape:
        raise _lib.MdxError(f"out: shape {tuple(out.shape)}, expected {shape}")
    return out


def _average_io(windows, grid, P, out, weights):
    """NB, ld, out of an average of P rows per canvas row: windows [NB * P, h * w, ld], weights [h, w] or None, out
    [NB, Hc * Wc, ld]."""
    if windows.dim() != 3 or windows.shape[0] % P or windows.shape[1] != grid.h * grid.w:
        raise _lib.MdxError(f"windows: shape {tuple(windows.shape)}, expected [NB * {P}, {grid.h * grid.w}, ld]")
    NB, ld = int(windows.shape[0]) // P, int(windows.shape[2])
    if weights is not None and tuple(weights.shape) != (grid.h, grid.w):
        raise _lib.MdxError(f"weights: shape {tuple(weights.shape)}, expected {(grid.h, grid.w)}")
    return NB, ld, _window_out(out, (NB, grid.Hc * grid.Wc, ld), windows)


def window_gather(canvas, grid, k0=0, n=None, out=None):
    """Windows k0 .. k0 + n - 1 of canvas [NB, C, Hc, Wc] fp32 as [NB * n, C, h, w], window kk of canvas row j in output row
    j * n + kk.  One launch."""
    _chk(canvas, f32, "canvas"); _chk(out, f32, "out")
    _clamped(grid, "window_gather")
    NB, C = _gather_dims(canvas, grid)
    k0 = int(k0)
    n = grid.N - k0 if n is None else int(n)
    if k0 < 0 or n < 1 or k0 + n > grid.N:
        raise _lib.MdxError(f"window_gather: windows [{k0}, {k0} + {n}) are not inside the grid of {grid.ny} x {grid.nx}")
    out = _window_out(out, (NB * n, C, grid.h, grid.w), canvas)
    _lib.check(_lib.load().mdx_window_gather_f32(_ptr(canvas), _ptr(out), _ptr(grid.on(canvas.device)), grid._host_ptr(), grid.ny,
                                                 grid.nx, k0, n, NB, C, grid.Hc, grid.Wc, grid.h, grid.w, _stream()),
               "mdx_window_gather_f32")
    return out


def window_average(windows, grid, C, out=None, weights=None):
    """The outputs of ALL windows, NHWC fp16 [NB * N, h * w, ld] in window_gather's row order, averaged onto the canvas
    [NB, Hc * Wc, ld] (include/mdx.h: the arithmetic is part of the contract).  weights: [h, w] fp32 > 0 on the device, None:
    uniform.  Channels [C, ld) of the result are 0.  One launch."""
    _chk(windows, f16, "windows"); _chk(out, f16, "out"); _chk(weights, f32, "weights")
    _clamped(grid, "window_average")
    NB, ld, out = _average_io(windows, grid, grid.N, out, weights)
    _lib.check(_lib.load().mdx_window_average_f16(_ptr(windows), _ptr(out), _ptr(weights), 0 if weights is None else weights.numel(),
                                                  _ptr(grid.on(windows.device)), grid._host_ptr(), grid.ny, grid.nx, NB, int(C), ld,
                                                  grid.Hc, grid.Wc, grid.h, grid.w, _stream()), "mdx_window_average_f16")
    return out


def window_gather_rows(canvas, grid, rows, out=None):
    """The windows rows[0 .. n) -- a WindowRows, or a sequence of window numbers; any order, repeats allowed -- of canvas
    [NB, C, Hc, Wc] fp32 as [NB * n, C, h, w], window rows[i] of canvas row j in output row j * n + i.  Reads a wrapped grid
    (grid.wrap_x) as well as a clamped one.  One launch."""
    _chk(canvas, f32, "canvas"); _chk(out, f32, "out")
    NB, C = _gather_dims(canvas, grid)
    if not isinstance(rows, WindowRows):
        rows = WindowRows(rows)
    n = len(rows)
    if n < 1 or rows.lo < 0 or rows.hi >= grid.N:              # (the C entry checks the host table itself, entry by entry)
        raise _lib.MdxError(f"window_gather_rows: rows {rows.host.tolist()} are not inside the grid of {grid.ny} x {grid.nx}")
    out = _window_out(out, (NB * n, C, grid.h, grid.w), canvas)
    _lib.check(_lib.load().mdx_window_gather_rows_f32(_ptr(canvas), _ptr(out), _ptr(grid.on(canvas.device)), grid._host_ptr(),
                                                      grid.ny, grid.nx, _ptr(rows.on(canvas.device)), rows._host_ptr(), n,
                                                      int(grid.wrap_x), NB, C, grid.Hc, grid.Wc, grid.h, grid.w, _stream()),
               "mdx_window_gather_rows_f32")
    return out


def window_average_regions(windows, grid, C, plan=None, out=None, weights=None):
    """The outputs of all P active pairs of `plan` (a RegionPlan on `grid`), NHWC fp16 [NB * P, h * w, ld], row j * P + p,
    averaged onto the canvas [NB, Hc * Wc, ld] with every term weighed by its region's mask at the pixel (times `weights`
    inside the window); include/mdx.h states the arithmetic.  plan None: no regions -- the pairs are the N windows -- which is
    window_average on a grid that may wrap.  One launch."""
    _chk(windows, f16, "windows"); _chk(out, f16, "out"); _chk(weights, f32, "weights")
    if plan is not None and plan.grid is not grid:
        raise _lib.MdxError("window_average_regions: the plan was made for another grid")
    P = grid.N if plan is None else plan.P
    NB, ld, out = _average_io(windows, grid, P, out, weights)
    dev = windows.device
    if plan is None:
        tables, masks, R = (None,) * 5, None, 0
    else:
        tables = (plan.pair_window._host_ptr(), _ptr(plan.pair_region.on(dev)), plan.pair_region._host_ptr(),
                  _ptr(plan.pair_first.on(dev)), plan.pair_first._host_ptr())
        masks, R = plan.masks_on(dev), plan.R
    _lib.check(_lib.load().mdx_window_average_regions_f16(
        _ptr(windows), _ptr(out), _ptr(weights), 0 if weights is None else weights.numel(), _ptr(grid.on(dev)), grid._host_ptr(),
        grid.ny, grid.nx, int(grid.wrap_x), *tables, P, _ptr(masks), R, NB, int(C), ld, grid.Hc, grid.Wc, grid.h, grid.w,
        _stream()), "mdx_window_average_regions_f16")
    return out


# Tiled VAE (include/mdx.h: mdx_tile_blend_f32, csrc/window.hip).
TILE_MODES = {"raw": 0, "unit": 1}          # MDX_TILE_RAW / MDX_TILE_UNIT


def ramp_weights(tile_hw, ramp_hw):
    """[h, w] fp32 min-ramp: min(y + 1, h - y, ramp_y) * min(x + 1, w - x, ramp_x) -- the weights mdx_tile_blend_f32 computes
    in its kernel, as a table for window_average(weights=) on the encode side of a tiled VAE."""
    (h, w), (ry, rx) = (int(v) for v in tile_hw), (int(v) for v in ramp_hw)
    if h < 1 or w < 1 or ry < 1 or rx < 1:
        raise _lib.MdxError(f"ramp_weights: tile {(h, w)} and ramps {(ry, rx)} must be positive")
    y, x = np.arange(h), np.arange(w)
    qy, qx = np.minimum(np.minimum(y + 1, h - y), ry), np.minimum(np.minimum(x + 1, w - x), rx)
    return torch.from_numpy((qy[:, None] * qx[None, :]).astype(np.float32))


def tile_blend(tiles, grid, ramp, out=None, mode="raw"):
    """Image tiles fp32 [NB * N, C, TH, TW] in window_gather's row order blended onto the canvas [NB, C, Hc, Wc] of `grid` -- a
    WindowGrid on the IMAGE canvas, in output pixels, wrapped or not -- with min-ramp weights; ramp: an int or (ramp_y, ramp_x),
    each in [1, 4096].  mode "raw": the blend; "unit": clamp((blend + 1) / 2, 0, 1) in the same launch.  include/mdx.h states
    the arithmetic.  One launch."""
    _chk(tiles, f32, "tiles"); _chk(out, f32, "out")
    if mode not in TILE_MODES:
        raise _lib.MdxError(f"tile_blend: mode must be one of {sorted(TILE_MODES)}, got {mode!r}")
    ry, rx = (ramp, ramp) if np.ndim(ramp) == 0 else ramp
    if tiles.dim() != 4 or tiles.shape[0] % grid.N or tuple(tiles.shape[2:]) != (grid.h, grid.w):
        raise _lib.MdxError(f"tiles: shape {tuple(tiles.shape)}, expected [NB * {grid.N}, C, {grid.h}, {grid.w}]")
    NB, C = int(tiles.shape[0]) // grid.N, int(tiles.shape[1])
    out = _window_out(out, (NB, C, grid.Hc, grid.Wc), tiles)
    _lib.check(_lib.load().mdx_tile_blend_f32(_ptr(tiles), _ptr(out), _ptr(grid.on(tiles.device)), grid._host_ptr(), grid.ny,
                                              grid.nx, int(grid.wrap_x), NB, C, grid.Hc, grid.Wc, grid.h, grid.w, int(ry), int(rx),
                                              TILE_MODES[mode], _stream()), "mdx_tile_blend_f32")
    return out


# ---------------------------------------------------------------------------------------------------------------
# Per-sample seeded noise (include/mdx.h: mdx_philox_u32 / mdx_randn_f32, csrc/rng.hip).  `stream` says what a draw is for,
# `draw` which one it is; these are the streams the samplers and the pipeline use (a stream is < 2^31: the top bit selects
# the dropout decisions of the same stream).
RNG_X_T = 0            # the start latent; draw 0
RNG_STEP = 1           # the k-th stochastic step (eta > 0) of a run; draw k
RNG_BLEND = 2          # the mask blend at loop index i; draw i
RNG_ENCODE = 3         # the forward noise of stochastic_encode / img2img; draw 0
RNG_POSTERIOR = 4      # the VAE posterior sample of img2img; draw 0


def seeds_tensor(seeds, device):
    """A sequence of Python ints in [-2^63, 2^64) (or an integer tensor) -> the int64 device tensor the kernels read.  A value
    of 2^63 and above is stored as its two's-complement pattern: seed 2^64 - 1 and seed -1 are the same seed."""
    if isinstance(seeds, torch.Tensor):
        if seeds.dtype.is_floating_point or seeds.dtype == torch.bool or seeds.dim() != 1:
            raise _lib.MdxError(f"seeds: expected a 1-d integer tensor, got {seeds.dtype} {tuple(seeds.shape)}")
        return seeds.to(device=device, dtype=torch.int64).contiguous()
    vals = []
    for s in seeds:
        if isinstance(s, bool) or int(s) != s:
            raise _lib.MdxError(f"seeds: {s!r} is not an integer")
        s = int(s)
        if not -(1 << 63) <= s < (1 << 64):
            raise _lib.MdxError(f"seeds: {s} is outside [-2^63, 2^64)")
        vals.append(s - (1 << 64) if s >= (1 << 63) else s)
    return torch.tensor(vals, dtype=torch.int64, device=device)


def _rng_args(name, seeds, stream, draw, sample_shape, out, dtype):
    if not (isinstance(seeds, torch.Tensor) and seeds.dim() == 1):
        raise _lib.MdxError(f"{name}: seeds must be a 1-d int64 device tensor (ops.seeds_tensor)")
    _chk(seeds, torch.int64, "seeds"); _chk(out, dtype, "out")
    if not (0 <= int(stream) < (1 << 31) and 0 <= int(draw) < (1 << 32)):
        raise _lib.MdxError(f"{name}: stream must be in [0, 2^31) and draw in [0, 2^32), got {stream!r}, {draw!r}")
    shape = (int(sample_shape),) if isinstance(sample_shape, int) else tuple(int(d) for d in sample_shape)
    B, n = int(seeds.shape[0]), 1
    for d in shape:
        n *= d
    if out is None:
        out = torch.empty((B,) + shape, dtype=dtype, device=seeds.device)
    elif tuple(out.shape) != (B,) + shape:
        raise _lib.MdxError(f"{name}: out has shape {tuple(out.shape)}, expected {(B,) + shape}")
    return out, B, n


def philox_u32(seeds, stream, draw, sample_shape, out=None):
    """The generator's raw 32-bit words, [B, *sample_shape] as int32 storage (bit patterns): element e of sample b is word
    e & 3 of Philox4x32-10(counter (e >> 2, draw, stream, 0), key seeds[b])."""
    out, B, n = _rng_args("philox_u32", seeds, stream, draw, sample_shape, out, torch.int32)
    _lib.check(_lib.load().mdx_philox_u32(_ptr(seeds), int(stream), int(draw), _ptr(out), B, n, _stream()), "mdx_philox_u32")
    return out


def randn_seeded(seeds, stream, draw, sample_shape, scale=1.0, dropout=0.0, out=None):
    """scale * N(0, 1) as [B, *sample_shape] fp32, sample b drawn from seeds[b] alone: the same (seed, stream, draw, element)
    gives the same bits whatever the batch, the row or the rank.  dropout p > 0: zero with probability p, the rest scaled by
    1 / (1 - p) (plms.py:224-225), decided by the same counter under stream | 2^31.  One launch."""
    out, B, n = _rng_args("randn_seeded", seeds, stream, draw, sample_shape, out, f32)
    _lib.check(_lib.load().mdx_randn_f32(_ptr(seeds), int(stream), int(draw), float(scale), float(dropout), _ptr(out), B, n,
                                         _stream()), "mdx_randn_f32")
    return out


def randn_slots(seeds, stream, draw0, slot_start, slot_len, tick, out, scale=1.0, dropout=0.0):
    """randn_seeded with the draw counter per session slot: sample b of `out` [B, *sample_shape] gets draw
    draw0 + (tick - slot_start[b]) while that position lies in [0, slot_len[b]) -- the bits randn_seeded(seeds[b:b+1], stream,
    that draw, ...) gives -- and is not written otherwise.  One launch."""
    if out is None:
        raise _lib.MdxError("randn_slots: pass out (the slots that are not active keep what it holds)")
    out, B, n = _rng_args("randn_slots", seeds, stream, draw0, tuple(out.shape[1:]), out, f32)
    _chk_slots(B, slot_start, slot_len)
    _lib.check(_lib.load().mdx_randn_slots_f32(_ptr(seeds), int(stream), int(draw0), float(scale), float(dropout), _ptr(out),
                                               _ptr(slot_start), _ptr(slot_len), int(tick), B, n, _stream()),
               "mdx_randn_slots_f32")
    return out


def slot_blend(x0, keep, img, seeds, stream, draw0, blend_ab, blend_on, slot_start, slot_len, tick):
    """The mask blend of decode()'s iterations per session slot, in place and in one launch: for every slot b that is active at
    `tick` and has blend_on[b] != 0, img[b] = keep[b] * q + (1 - keep[b]) * img[b] with q = a * x0[b] + b * noise, (a, b) =
    blend_ab[b, pos_b] and the noise drawn inside the kernel -- the bits of randn_seeded(seeds[b:b+1], stream, draw0 + pos_b)
    followed by q_sample(x0[b], noise, a, b, out=img[b], mask=keep[b], img=img[b]).  The other slots' rows of img are not
    touched.  x0, keep, img [B, C, H, W] fp32; blend_ab [B, cap, 2] fp32; blend_on [B] int32."""
    _chk(x0, f32, "x0"); _chk(keep, f32, "keep"); _chk(img, f32, "img"); _chk(blend_ab, f32, "blend_ab")
    _chk(seeds, torch.int64, "seeds"); _chk(blend_on, torch.int32, "blend_on")
    if img.dim() != 4:
        raise _lib.MdxError(f"slot_blend: img must be [B, C, H, W], got {tuple(img.shape)}")
    B, C, H, W = (int(d) for d in img.shape)
    _same_shape(img, "x0", x0); _same_shape(img, "keep", keep)
    if blend_ab.dim() != 3 or blend_ab.shape[0] != B or blend_ab.shape[2] != 2:
        raise _lib.MdxError(f"slot_blend: blend_ab must be [{B}, cap, 2], got {tuple(blend_ab.shape)}")
    if tuple(seeds.shape) != (B,) or tuple(blend_on.shape) != (B,):
        raise _lib.MdxError(f"slot_blend: seeds and blend_on must be [{B}], got {tuple(seeds.shape)}, {tuple(blend_on.shape)}")
    _chk_slots(B, slot_start, slot_len)
    if not (0 <= int(stream) < (1 << 31) and 0 <= int(draw0) < (1 << 32)):
        raise _lib.MdxError(f"slot_blend: stream must be in [0, 2^31) and draw0 in [0, 2^32), got {stream!r}, {draw0!r}")
    _lib.check(_lib.load().mdx_slot_blend_f32(_ptr(x0), _ptr(keep), _ptr(img), _ptr(seeds), int(stream), int(draw0),
                                              _ptr(blend_ab), _ptr(blend_on), _ptr(slot_start), _ptr(slot_len),
                                              int(blend_ab.shape[1]), int(tick), B, C, H * W, _stream()), "mdx_slot_blend_f32")
    return img


# ---------------------------------------------------------------------------------------------------------------
# Separable resampling (include/mdx.h: mdx_resample_f32 / mdx_resample_noised_f32, csrc/resample.hip; the tables:
# minddiffusion_amd/resample.py)
_TAP_TABLES = {}


def _tap_tables(n_in, n_out, mode, antialias, wrap, device):
    """(start int32 [n_out], w fp32 [n_out, T]) of one axis on `device`, uploaded once per (n_in, n_out, mode, antialias, wrap,
    device)."""
    key = (int(n_in), int(n_out), mode, bool(antialias), bool(wrap), torch.device(device))
    if key not in _TAP_TABLES:
        start, w = _resample.tap_table(n_in, n_out, mode, antialias, wrap)
        _TAP_TABLES[key] = (torch.from_numpy(start).to(device), torch.from_numpy(np.ascontiguousarray(w)).to(device))
    return _TAP_TABLES[key]


def _resample_args(name, x, size, mode, antialias, wrap_x):
    _chk(x, f32, "x")
    if x.dim() != 4:
        raise _lib.MdxError(f"{name}: x must be [B, C, H, W], got shape {tuple(x.shape)}")
    if mode not in _resample.MODES:
        raise _lib.MdxError(f"{name}: mode must be one of {_resample.MODES}, got {mode!r}")
    B, C, H, W = (int(d) for d in x.shape)
    Ho, Wo = int(size[0]), int(size[1])
    if Ho <= 0 or Wo <= 0:
        raise _lib.MdxError(f"{name}: size must be positive, got {tuple(size)}")
    try:
        ys, yw = _tap_tables(H, Ho, mode, Ho < H if antialias is None else antialias, False, x.device)
        xs, xw = _tap_tables(W, Wo, mode, Wo < W if antialias is None else antialias, wrap_x, x.device)
    except ValueError as e:
        raise _lib.MdxError(f"{name}: {e}") from None
    tables = (_ptr(ys), _ptr(yw), int(yw.shape[1]), _ptr(xs), _ptr(xw), int(xw.shape[1]), int(bool(wrap_x)))
    return (B, C, H, W, Ho, Wo), tables


def resample(x, size, mode="bicubic", antialias=None, wrap_x=False, out=None):
    """x [B, C, H, W] fp32 resampled to size = (H_out, W_out), one launch.  mode: "nearest" (the integer rule (i * n_in) // n_out),
    "bilinear", "bicubic" (F.interpolate(align_corners=False)'s definitions, antialias as torch's antialias=True) or "lanczos3"
    (always antialiased).  antialias None: on for an axis that shrinks, off otherwise.  wrap_x: columns wrap around (a panorama)
    instead of replicating the edge; rows always replicate.  An axis that keeps its size is copied bit for bit."""
    dims, tables = _resample_args("resample", x, size, mode, antialias, wrap_x)
    B, C, _, _, Ho, Wo = dims
    _chk(out, f32, "out")
    if out is None:
        out = torch.empty((B, C, Ho, Wo), dtype=f32, device=x.device)
    elif tuple(out.shape) != (B, C, Ho, Wo):
        raise _lib.MdxError(f"out: shape {tuple(out.shape)}, expected {(B, C, Ho, Wo)}")
    _lib.check(_lib.load().mdx_resample_f32(_ptr(x), _ptr(out), *dims, *tables, _stream()), "mdx_resample_f32")
    return out


def resample_noised(x, size, a, b, *, scale=1.0, noise=None, seeds=None, stream=RNG_ENCODE, draw=0, mode="bicubic",
                    antialias=None, wrap_x=False, z0_out=None, xt_out=None):
    """The resample fused onto the start of an img2img run, one launch: (z0, xt) with z0 = scale * resample(x, size, ...) and
    xt = a * z0 + b * n -- bit for bit q_sample(z0, n, a, b).  n: `noise` [B, C, H_out, W_out], or drawn per sample from `seeds`
    (ints, or ops.seeds_tensor's tensor) at (stream, draw) -- the bits of randn_seeded(seeds, stream, draw, (C, H_out, W_out)), never stored.
    Exactly one of noise and seeds.  z0_out / xt_out: a tensor to write, None for a fresh one, False to leave that output out
    (not both; without xt no noise source is needed)."""
    dims, tables = _resample_args("resample_noised", x, size, mode, antialias, wrap_x)
    B, C, _, _, Ho, Wo = dims
    if z0_out is False and xt_out is False:
        raise _lib.MdxError("resample_noised: no output (z0_out and xt_out are both False)")
    if xt_out is not False and (noise is None) == (seeds is None):
        raise _lib.MdxError("resample_noised: pass exactly one of noise and seeds")
    _chk(noise, f32, "noise")
    for name, t in (("z0_out", z0_out), ("xt_out", xt_out)):
        _chk(None if t is False else t, f32, name)
    if seeds is not None:
        if not isinstance(seeds, torch.Tensor):
            seeds = seeds_tensor(seeds, x.device)
        if tuple(seeds.shape) != (B,):
            raise _lib.MdxError(f"resample_noised: {tuple(seeds.shape)} seeds for a batch of {B} (one per sample)")
        _chk(seeds, torch.int64, "seeds")
        if not (0 <= int(stream) < (1 << 31) and 0 <= int(draw) < (1 << 32)):
            raise _lib.MdxError(f"resample_noised: stream must be in [0, 2^31) and draw in [0, 2^32), got {stream!r}, {draw!r}")
    shape = (B, C, Ho, Wo)
    fresh = lambda t: None if t is False else torch.empty(shape, dtype=f32, device=x.device) if t is None else t
    z0_out, xt_out = fresh(z0_out), fresh(xt_out)
    for name, t in (("noise", noise), ("z0_out", z0_out), ("xt_out", xt_out)):
        if t is not None and tuple(t.shape) != shape:
            raise _lib.MdxError(f"{name}: shape {tuple(t.shape)}, expected {shape}")
    _lib.check(_lib.load().mdx_resample_noised_f32(_ptr(x), *dims, *tables, float(scale), float(a), float(b), _ptr(noise),
                                                   _ptr(seeds), int(stream), int(draw), _ptr(z0_out), _ptr(xt_out), _stream()),
               "mdx_resample_noised_f32")
    return z0_out, xt_out


# ---------------------------------------------------------------------------------------------------------------
# Row-local fused SpatialTransformer tail (include/mdx.h: mdx_st_tail_f16, csrc/stchain.hip)
def pack_frag_weight(w2d):
    """[N, K] nn.Dense weight -> MFMA-fragment-major pieces [N/32 column tiles][K/16 k-steps][64 lanes * 8 halves]:
    piece (ct, s)[lane] = W[32 ct + lane % 32][16 s + 8 (lane // 32) + 0..7] -- the first operand of
    v_mfma_f32_32x32x16_f16 exactly as a lane holds it, so a wave loads one piece with ONE coalesced 1 KiB instruction."""
    N, K = w2d.shape
    assert N % 32 == 0 and K % 16 == 0
    t = w2d.to(f16).reshape(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4)     # [ct, s, hi, l31, 8]
    return t.reshape(N // 32, K // 16, 512).contiguous()


def pack_st_tail(wo1, wq2, wo2, w1, w2, wpo, bo1, g2, be2, bo2, g3, be3, b1, b2, bpo):
    """Weights / vectors of one SpatialTransformer block (depth 1) in the layout mdx_st_tail_f16 streams:
    wave w of the C/32 waves owns output columns [32w, 32w+32) of every GEMM of the chain; its pieces are stored in
    consumption order -- to_out1, to_q2, to_out2, 4 x (ff1 chunk: 'a' and 'gate' pieces interleaved per k-step, then the ff2
    K-chunk), proj_out -- as ONE contiguous stream.  w1: [8C, C] (reference order: a rows then gate rows), w2: [C, 4C].
    Returns (stream fp16 [C/32, 16 C/16, 512], vec fp32 [16 C])."""
    C = wo1.shape[0]
    NW, KS = C // 32, C // 16
    f = pack_frag_weight
    fo1, fq2, fo2, fpo = f(wo1), f(wq2), f(wo2), f(wpo)        # [NW, KS, 512]
    f1 = f(w1)                                                  # [8C/32, KS, 512]: tiles [0, 4C/32) = a, then gate
    f2 = f(w2)                                                  # [NW, 4C/16, 512]
    parts = [fo1, fq2, fo2]
    for c in range(4):
        a = f1[c * NW:(c + 1) * NW]
        g = f1[4 * C // 32 + c * NW:4 * C // 32 + (c + 1) * NW]
        parts.append(torch.stack([a, g], 2).reshape(NW, 2 * KS, 512))
        parts.append(f2[:, c * KS:(c + 1) * KS])
    parts.append(fpo)
    stream = torch.cat(parts, 1).contiguous()
    assert stream.shape == (NW, 16 * KS, 512)
    vec = torch.cat([v.to(f32).reshape(-1) for v in (bo1, g2, be2, bo2, g3, be3, b1, b2, bpo)]).contiguous()
    assert vec.numel() == 16 * C
    return stream, vec


def st_tail_supported(C, heads, dim_head, tokens, tile_rows):
    return bool(_lib.load().mdx_st_tail_supported(int(C), int(heads), int(dim_head), int(tokens), int(tile_rows)))


def make_st_tail_desc(attn_out, tok, x_in, out, ctx_k, ctx_vt, stream, vec, B, tokens, C, heads, dim_head, ctx_len, ctx_cap,
                      tile_rows=64, ln_eps=1e-5, colstats_out=None, debug_out=None, debug_stage=0):
    d = _lib.StTailDesc()
    d.attn_out, d.tok, d.x_in, d.out = attn_out.data_ptr(), tok.data_ptr(), x_in.data_ptr(), out.data_ptr()
    d.ctx_k, d.ctx_vt, d.wstream, d.vec = ctx_k.data_ptr(), ctx_vt.data_ptr(), stream.data_ptr(), vec.data_ptr()
    d.colstats_out = 0 if colstats_out is None else colstats_out.data_ptr()
    d.debug_out = 0 if debug_out is None else debug_out.data_ptr()
    d.debug_stage = int(debug_stage)
    d.B, d.tokens, d.C, d.heads, d.dim_head = int(B), int(tokens), int(C), int(heads), int(dim_head)
    d.ctx_len, d.ctx_cap = int(ctx_len), int(ctx_cap)
    d.scale, d.ln_eps, d.tile_rows = float(dim_head) ** -0.5, float(ln_eps), int(tile_rows)
    d.warm = int(os.environ.get("MDX_ST_TAIL_WARM", "1"))
    return d


def st_tail_run(desc):
    _lib.check(_lib.load().mdx_st_tail_f16(ctypes.byref(desc), _stream()), "mdx_st_tail_f16")


def pack_st_head(wpi, wq, wk, wv, gn_g, gn_b, bpi, g1, be1):
    """Weights / vectors of the fused SpatialTransformer head (mdx_st_head_f16): per wave its proj_in, to_q, to_k, to_v column
    tiles as one contiguous stream of MFMA-fragment pieces.  Returns (stream fp16 [C/32, 4 C/16, 512], vec fp32 [5 C])."""
    f = pack_frag_weight
    stream = torch.cat([f(wpi), f(wq), f(wk), f(wv)], 1).contiguous()
    vec = torch.cat([t.to(f32).reshape(-1) for t in (gn_g, gn_b, bpi, g1, be1)]).contiguous()
    return stream, vec


def st_head_supported(C, tokens, tile_rows):
    return bool(_lib.load().mdx_st_head_supported(int(C), int(tokens), int(tile_rows)))


def make_st_head_desc(x, colstats, nrb, stream, vec, tok, qk, vt, vt_ld, B, tokens, C, tile_rows=32, gn_eps=1e-6, ln_eps=1e-5,
                      debug_out=None, debug_stage=0):
    d = _lib.StHeadDesc()
    d.x, d.colstats, d.nrb = x.data_ptr(), colstats.data_ptr(), int(nrb)
    d.wstream, d.vec = stream.data_ptr(), vec.data_ptr()
    d.tok, d.qk, d.vt, d.vt_ld = tok.data_ptr(), qk.data_ptr(), vt.data_ptr(), int(vt_ld)
    d.debug_out = 0 if debug_out is None else debug_out.data_ptr()
    d.debug_stage = int(debug_stage)
    d.B, d.tokens, d.C = int(B), int(tokens), int(C)
    d.gn_eps, d.ln_eps, d.tile_rows = float(gn_eps), float(ln_eps), int(tile_rows)
    d.warm = int(os.environ.get("MDX_ST_TAIL_WARM", "1"))
    return d


def st_head_run(desc):
    _lib.check(_lib.load().mdx_st_head_f16(ctypes.byref(desc), _stream()), "mdx_st_head_f16")


LORA_ROWMAJOR, LORA_TILED, LORA_FRAG = _lib.LORA_ROWMAJOR, _lib.LORA_TILED, _lib.LORA_FRAG


def lora_merge(base, dst, layout, A=None, B=None, scale=1.0, gamma=None, beta=None, bias=None, S=None, cb=None, ld=0,
               dst_n0=0, dst_N=None, piece_stride=0, piece_offset=0):
    """mdx_lora_merge_f16 (include/mdx.h): W' = fp16(base + scale * B @ A) of one nn.Dense weight [N, K], written IN PLACE into
    rows [dst_n0, dst_n0 + N) of `dst` in the layout a kernel reads -- LORA_ROWMAJOR ([dst_N, ld] fp16), LORA_TILED (the
    pack_gemm_weight storage) or LORA_FRAG (pack_frag_weight pieces; k-steps [piece_offset, piece_offset + K/16) of
    `piece_stride` pieces per column tile).  base fp32 [N, K]; A fp32 [R, K] and B fp32 [N, R] or None (a pure re-pack).
    gamma / beta (/ bias): the LayerNorm fold of fold_layernorm computed from the merged matrix; S and cb ([>= N] fp32 views
    that start at this matrix's first row) receive the row sums and the folded bias."""
    _chk(base, f32, "base"); _chk(dst, f16, "dst")
    N, K = base.shape
    R = 0
    if A is not None or B is not None:
        if A is None or B is None:
            raise _lib.MdxError("lora_merge: A and B go together")
        _chk(A, f32, "A"); _chk(B, f32, "B")
        R = A.shape[0]
        if tuple(A.shape) != (R, K) or tuple(B.shape) != (N, R):
            raise _lib.MdxError(f"lora_merge: A {tuple(A.shape)} / B {tuple(B.shape)} do not match base {(N, K)}")
    dst_N = N + dst_n0 if dst_N is None else int(dst_N)
    if layout == LORA_ROWMAJOR:
        ld = int(ld) or K
        need = (dst_N - 1) * ld + K
    elif layout == LORA_TILED:
        need = ((dst_N + 63) // 64 * 64) * ((K + 63) // 64 * 64)
    elif layout == LORA_FRAG:
        piece_stride = int(piece_stride) or K // 16
        need = dst_N // 32 * piece_stride * 512
    else:
        raise _lib.MdxError(f"lora_merge: unknown layout {layout}")
    if dst.numel() < need:
        raise _lib.MdxError(f"lora_merge: dst holds {dst.numel()} halves, the destination needs {need}")
    for name, v, n in (("gamma", gamma, K), ("beta", beta, K), ("bias", bias, N), ("S", S, N), ("cb", cb, N)):
        _chk(v, f32, name)
        if v is not None and v.numel() < n:
            raise _lib.MdxError(f"lora_merge: {name} holds {v.numel()} values, needs {n}")
    d = _lib.LoraMergeDesc()
    d.base, d.A, d.B = base.data_ptr(), (A.data_ptr() if R else 0), (B.data_ptr() if R else 0)
    d.N, d.K, d.R, d.scale = N, K, R, float(scale)
    d.gamma, d.beta, d.bias, d.S, d.cb = (0 if v is None else v.data_ptr() for v in (gamma, beta, bias, S, cb))
    d.dst, d.layout, d.ld, d.dst_n0, d.dst_N = dst.data_ptr(), int(layout), int(ld), int(dst_n0), dst_N
    d.piece_stride, d.piece_offset = int(piece_stride), int(piece_offset)
    _lib.check(_lib.load().mdx_lora_merge_f16(ctypes.byref(d), _stream()), "mdx_lora_merge_f16")
    return dst


# ---------------------------------------------------------------------------------------------------------------
# ControlNet (include/mdx.h: mdx_control_add_f16, mdx_silu_f16)
CONTROL_MAX_SEGS = _lib.CONTROL_MAX_SEGS


def silu_(x):
    """x <- silu(x) in place (mdx_silu_f16): fp16, contiguous, a multiple of 8 values."""
    _chk(x, f16, "x")
    _lib.check(_lib.load().mdx_silu_f16(_ptr(x), x.numel(), _stream()), "mdx_silu_f16")
    return x


class ControlAdd:
    """One mdx_control_add_f16 launch: dst[s][r] += scale[s][r] * src[s][src_row[r]] for up to 16 fp16 tensors [nb, ...] at
    once, in place.  The descriptor (the destinations and their row sizes) is fixed here; everything else lives in three
    device tables this object owns and the kernel reads when it runs -- `scale` fp32 [n_seg, nb], `src_row` int32 [nb] (-1:
    the row is not touched) and the source pointers -- so a captured graph that holds run() serves any later set_sources /
    set_rows / set_scale.  Until the first set_rows every row is -1: run() changes nothing."""

    def __init__(self, dsts):
        dsts = list(dsts)
        if not 1 <= len(dsts) <= CONTROL_MAX_SEGS:
            raise _lib.MdxError(f"ControlAdd: {len(dsts)} segments outside [1, {CONTROL_MAX_SEGS}]")
        nb, dev = int(dsts[0].shape[0]), dsts[0].device
        d = _lib.ControlAddDesc()
        d.n_seg, d.nb = len(dsts), nb
        for s, t in enumerate(dsts):
            _chk(t, f16, f"dst[{s}]")
            if int(t.shape[0]) != nb or t.device != dev:
                raise _lib.MdxError(f"ControlAdd: dst[{s}] has {int(t.shape[0])} rows on {t.device}, dst[0] {nb} on {dev}")
            d.dst[s], d.elems_per_row[s] = t.data_ptr(), t.numel() // nb
        self.dsts, self.nb, self.n_seg, self.device = dsts, nb, len(dsts), dev
        self.scale = torch.zeros((len(dsts), nb), dtype=f32, device=dev)
        self.src_row = torch.full((nb,), -1, dtype=torch.int32, device=dev)
        self.src_ptrs = torch.zeros((CONTROL_MAX_SEGS,), dtype=torch.int64, device=dev)
        d.src, d.src_row, d.scale = self.src_ptrs.data_ptr(), self.src_row.data_ptr(), self.scale.data_ptr()
        self.desc = d
        self.sources = None         # the tensors the pointer table names (kept alive), and their row count
        self.rows = None            # host copy of src_row
        self.table_writes = 0       # uploads of the pointer table
        self._scale_src = None

    def set_sources(self, srcs, rows=None):
        """The tensor added into dst[s] is srcs[s]: fp16 [rows, ...] with dst[s]'s row size, 16-byte aligned.  `rows`: the row
        map that goes with them (set_rows; None keeps the current one) -- checked against the NEW sources, so a caller that
        changes both (another ControlNet batch) never has one checked against the other's predecessor.  The pointer table is
        uploaded only when a pointer changed."""
        srcs = list(srcs)
        if len(srcs) != self.n_seg:
            raise _lib.MdxError(f"ControlAdd: {len(srcs)} sources for {self.n_seg} segments")
        n_src = int(srcs[0].shape[0])
        for s, (t, dt) in enumerate(zip(srcs, self.dsts)):
            _chk(t, f16, f"src[{s}]")
            if t.device != self.device or int(t.shape[0]) != n_src or n_src < 1 or t.numel() // n_src != dt.numel() // self.nb:
                raise _lib.MdxError(f"ControlAdd: src[{s}] {tuple(t.shape)} on {t.device} does not match dst[{s}] "
                                    f"{tuple(dt.shape)} (rows of {dt.numel() // self.nb} halves, {n_src} source rows)")
            if t.data_ptr() % 16:
                raise _lib.MdxError(f"ControlAdd: src[{s}] is not 16-byte aligned")
        new_rows = self.rows if rows is None else [int(v) for v in rows]
        if new_rows is not None and max(new_rows) >= n_src:
            raise _lib.MdxError(f"ControlAdd: the row map {new_rows} reads past the {n_src} source rows")
        ptrs = [t.data_ptr() for t in srcs]
        if self.sources is None or ptrs != [t.data_ptr() for t in self.sources]:
            self.src_ptrs[:self.n_seg].copy_(torch.tensor(ptrs, dtype=torch.int64))
            self.table_writes += 1
        self.sources = srcs
        if rows is not None:
            self.set_rows(new_rows)

    def set_rows(self, rows):
        """rows[r]: the source row added into destination row r, or -1 to leave that row alone."""
        rows = [int(v) for v in rows]
        n_src = int(self.sources[0].shape[0]) if self.sources is not None else None
        if len(rows) != self.nb or any(v < -1 for v in rows) or (n_src is not None and max(rows) >= n_src):
            raise _lib.MdxError(f"ControlAdd: the row map {rows} must hold {self.nb} entries in [-1, {n_src})")
        if rows != self.rows:
            self.src_row.copy_(torch.tensor(rows, dtype=torch.int32))
            self.rows = rows

    def set_scale(self, scale):
        """scale: fp32 [n_seg, nb] (anything that broadcasts to it), host or device."""
        if isinstance(scale, torch.Tensor):       # the same tensor, unchanged since the last call: the table holds it already
            kept = self._scale_src
            if kept is not None and kept[0]() is scale and kept[1] == scale._version:
                return
        s = torch.as_tensor(scale, dtype=f32)
        self.scale.copy_(s.to(self.device).expand(self.n_seg, self.nb))
        self._scale_src = (weakref.ref(scale), scale._version) if isinstance(scale, torch.Tensor) else None

    def run(self):
        if self.sources is None and self.rows is not None and max(self.rows) >= 0:
            raise _lib.MdxError("ControlAdd: set_sources() must come before a run that reads them")
        _lib.check(_lib.load().mdx_control_add_f16(ctypes.byref(self.desc), _stream()), "mdx_control_add_f16")


def control_add(dsts, srcs, rows, scale):
    """One-shot form of ControlAdd (tests, tools): dst[s][r] += scale[s][r] * src[s][rows[r]] in place."""
    ca = ControlAdd(dsts)
    ca.set_sources(srcs, rows)
    ca.set_scale(scale)
    ca.run()
    return ca
