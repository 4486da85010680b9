"""UNetModel -- MI355X-native mirror of the reference's
vision/stablediffusionv2/ldm/modules/diffusionmodules/openaimodel.py:245-577 (and the Wukong copy).

Same constructor keywords (the ``unet_config.params`` keys of the reference YAMLs) and the same
``construct(x, timesteps, context)`` call; parameters are loaded by the reference's names
 via ``load_state_dict``.  Execution is completely different from the
reference's per-primitive MindSpore graph:

  * activations live in HBM as NHWC fp16 ([B, H*W, C] == token-major), so SpatialTransformer's
    NCHW<->NLC transposes (attention.py:243-253) vanish and every conv is an implicit GEMM;
  * the forward pass is PLANNED once per (B, H, W): a flat list of C-ABI kernel calls on
    pre-allocated, liveness-reused buffers (static addresses => capturable as ONE hipGraph);
  * Concat of skip connections (openaimodel.py:568) is never materialised (two-source kernels),
    nearest-2x Upsample is folded into the following conv's gather, the ResBlock time-embedding
    add / bias / residual adds / GEGLU are GEMM epilogues;
  * cross-attention K / V^T of the text context (constant over the sampling loop) are cached.

There is no CPU path: every op is a HIP kernel from libmdx.so.
"""
import ctypes
import math
import os
import re
import weakref

import torch

from .... import ops
from ...._lib import MdxError
from ....planner import PlanBuilder, round_up, capture_or_eager
from ....loader import WeightLoader, named_layers

f16, f32 = torch.float16, torch.float32

# parameter-name prefixes of the delta-tuning package's LoRADense (lora_a / lora_b); see UNetModel.lora_parameter_shapes
LORA_PREFIXES = ("tk_delta_", "mindpet_delta_")
_LORA_KEY = re.compile(r"^(.*)\.(" + "|".join(LORA_PREFIXES) + r")lora_([ab])$")
_LORA_TARGETS = ("to_q", "to_k", "to_v", "to_out.0")


def is_lora_key(name):
    return _LORA_KEY.match(name) is not None


class Control:
    """What UNetModel.forward_nhwc(control=) carries (ControlledUnetModel.forward of the ControlNet paper's cldm.py): the
    residual tensors of one ControlNet evaluation -- one per input block, then the middle block's, as
    ControlNet.forward_residuals returns them: fp16 [b, H * W, C] NHWC -- and the two tables of ops.ControlAdd: rows[r] = the
    residual row added to UNet batch row r (-1: that row runs without control) and scale, fp32 [n, B] (or what broadcasts to
    it): residual i reaches row r multiplied by scale[i][r]."""

    def __init__(self, sources, rows, scale):
        self.sources, self.rows, self.scale = list(sources), [int(r) for r in rows], scale


class UNetModel:
    def __init__(self, image_size=32, in_channels=4, model_channels=320, out_channels=4, num_res_blocks=2,
                 attention_resolutions=(4, 2, 1), dropout=0.0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2,
                 num_classes=None, use_checkpoint=False, use_fp16=False, num_heads=-1, num_head_channels=-1,
                 num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False, use_spatial_transformer=False, transformer_depth=1, context_dim=None,
                 n_embed=None, legacy=True, use_linear_in_transformer=False, enable_lora=False, lora_rank=4, lora_alpha=4,
                 max_context_len=80, device="cuda:0"):
        """max_context_len: capacity (keys) of the cached text context, rounded up to a multiple of 8; 80 holds one 77-token CLIP
        window, a prompt of n chunks needs n * 77 (set_max_context_len changes it later).  enable_lora / lora_rank / lora_alpha (WK openaimodel.py:302-304): to_q, to_k, to_v and to_out.0 of every
        CrossAttention become LoRA targets (WK attention.py:118-126).  The reference wires these keywords for Wukong only;
        here they work for every configuration (SDv2 included).  The adapter is MERGED into the packed weights in place
        (load_lora_state_dict), so the denoising loop is the code that runs without it."""
        # openaimodel.py:305-321 argument checks
        if use_spatial_transformer:
            assert context_dim is not None, "context_dim is required with use_spatial_transformer"
        if context_dim is not None:
            assert use_spatial_transformer, "context_dim requires use_spatial_transformer"
        if num_heads == -1:
            assert num_head_channels != -1, "Either num_heads or num_head_channels has to be set"
        if num_head_channels == -1:
            assert num_heads != -1, "Either num_heads or num_head_channels has to be set"
        if not use_spatial_transformer:
            raise NotImplementedError("AttentionBlock is an empty stub in the reference (openaimodel.py:208-242)")
        if dims != 2:
            raise NotImplementedError("dims != 2: the image UNet is the only instantiation on the denoising path")
        self.conv_resample = bool(conv_resample)
        self.num_classes = num_classes
        self.use_scale_shift_norm = bool(use_scale_shift_norm)
        self.resblock_updown = bool(resblock_updown)
        self.transformer_depth = int(transformer_depth)
        self.n_embed = n_embed                       # predict_codebook_ids (openaimodel.py:344, 527-531)
        assert self.transformer_depth >= 1
        self.image_size = image_size
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.out_channels = out_channels
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = list(attention_resolutions)
        self.channel_mult = list(channel_mult)
        self.num_heads = num_heads
        self.num_head_channels = num_head_channels
        self.context_dim = int(context_dim)
        self.legacy = legacy
        self.use_linear = use_linear_in_transformer
        self.use_fp16 = use_fp16
        self.device = torch.device(device)
        self.time_embed_dim = model_channels * 4
        self.input_blocks, self.middle_block, self.output_blocks = self._structure()
        self.cin_pad = round_up(in_channels, 8)
        self.final_channels = out_channels if n_embed is None else int(n_embed)
        self.cout_pad = round_up(self.final_channels, 8)
        self.w = None          # packed device weights
        self._plans = {}
        self._ctx_key = None
        self._ctx_ref = None
        self.use_graph = True
        # capacity of the cached context: 77 CLIP tokens rounded up to a multiple of 8 by default (V^T rows are 16-B chunked)
        self.max_context_len = self._check_context_cap(max_context_len)
        self.last_launch_count = 0
        self.enable_lora = bool(enable_lora)
        self.lora_rank = int(lora_rank)
        self.lora_alpha = float(lora_alpha)
        if self.enable_lora and not (1 <= self.lora_rank <= 64 and self.lora_alpha != 0):
            raise ValueError(f"UNetModel: lora_rank must be in [1, 64] and lora_alpha non-zero (got {lora_rank}, {lora_alpha})")
        self._lora_base = {}      # target name -> fp32 device copy of the base matrix (enable_lora only)
        self._lora_sites = {}     # target name -> the places the matrix lives in self.w (kwargs of ops.lora_merge)
        self._lora = None         # target name -> (A [rank, in], B [out, rank]) fp32 on the device
        self._lora_mult = 1.0

    @staticmethod
    def _check_context_cap(n):
        n = int(n)
        if not 1 <= n <= 1024:
            raise MdxError(f"UNetModel: max_context_len must be in [1, 1024] (got {n})")
        return round_up(n, 8)

    def set_max_context_len(self, n):
        """Capacity of the cached text context in keys (rounded up to a multiple of 8, at most 1024).  Plans size their
        context buffers by it, so a CHANGE drops the plans, their captured graphs and the cached context projections; the same
        value again is a no-op.  Call it between evaluations (never from inside a sampling loop: the next evaluation plans and
        captures again).  On several ranks every rank must set the same value before conditioning is broadcast."""
        n = self._check_context_cap(n)
        if n != self.max_context_len:
            self.max_context_len = n
            self._plans = {}
            self._ctx_key = None
            self._ctx_ref = None
        return self

    # ------------------------------------------------------------------ structure (openaimodel.py:351-526)
    def _heads(self, ch, num_heads):
        if self.num_head_channels == -1:
            dim_head = ch // num_heads
        else:
            num_heads = ch // self.num_head_channels
            dim_head = self.num_head_channels
        if self.legacy:
            dim_head = ch // num_heads  # use_spatial_transformer branch of openaimodel.py:375-376
        return num_heads, dim_head

    def _structure(self):
        mc = self.model_channels
        nh = self.num_heads
        inb = [[("conv", self.in_channels, mc)]]
        chans = [mc]
        ch, ds = mc, 1
        for level, mult in enumerate(self.channel_mult):
            for _ in range(self.num_res_blocks):
                layers = [("res", ch, mult * mc)]
                ch = mult * mc
                if ds in self.attention_resolutions:
                    nh, dh = self._heads(ch, nh)
                    layers.append(("st", ch, nh, dh))
                inb.append(layers)
                chans.append(ch)
            if level != len(self.channel_mult) - 1:
                inb.append([("resdown", ch, ch) if self.resblock_updown else ("down", ch)])
                chans.append(ch)
                ds *= 2
        nh, dh = self._heads(ch, nh)
        mid = [("res", ch, ch), ("st", ch, nh, dh), ("res", ch, ch)]
        outb = []
        for level, mult in list(enumerate(self.channel_mult))[::-1]:
            for i in range(self.num_res_blocks + 1):
                ich = chans.pop()
                layers = [("res", ch + ich, mc * mult)]
                ch = mc * mult
                if ds in self.attention_resolutions:
                    nh, dh = self._heads(ch, nh)
                    layers.append(("st", ch, nh, dh))
                if level and i == self.num_res_blocks:
                    layers.append(("resup", ch, ch) if self.resblock_updown else ("up", ch))
                    ds //= 2
                outb.append(layers)
        return inb, mid, outb

    def parameter_shapes(self):
        """name -> shape, in the reference's naming."""
        mc, ted, ctx = self.model_channels, self.time_embed_dim, self.context_dim
        s = {"time_embed.0.weight": (ted, mc), "time_embed.0.bias": (ted,),
             "time_embed.2.weight": (ted, ted), "time_embed.2.bias": (ted,)}
        if self.num_classes is not None:
            s["label_emb.embedding_table"] = (self.num_classes, ted)
        ssn = 2 if self.use_scale_shift_norm else 1
        for pre, layer in named_layers(self):
            kind = layer[0]
            if kind == "conv":
                s[pre + "conv.weight"] = (layer[2], layer[1], 3, 3)
                s[pre + "conv.bias"] = (layer[2],)
            elif kind in ("res", "resdown", "resup"):
                cin, cout = layer[1], layer[2]
                s[pre + "in_layers_norm.gamma"] = (cin,)
                s[pre + "in_layers_norm.beta"] = (cin,)
                s[pre + "in_layers_conv.conv.weight"] = (cout, cin, 3, 3)
                s[pre + "in_layers_conv.conv.bias"] = (cout,)
                s[pre + "emb_layers.1.weight"] = (ssn * cout, ted)
                s[pre + "emb_layers.1.bias"] = (ssn * cout,)
                s[pre + "out_layers_norm.gamma"] = (cout,)
                s[pre + "out_layers_norm.beta"] = (cout,)
                s[pre + "out_layers_conv.conv.weight"] = (cout, cout, 3, 3)
                s[pre + "out_layers_conv.conv.bias"] = (cout,)
                if cin != cout:
                    s[pre + "skip_connection.conv.weight"] = (cout, cin, 1, 1)
                    s[pre + "skip_connection.conv.bias"] = (cout,)
            elif kind == "st":
                ch, inner = layer[1], layer[2] * layer[3]
                s[pre + "norm.gamma"] = (ch,)
                s[pre + "norm.beta"] = (ch,)
                s[pre + "proj_in.weight"] = (inner, ch) if self.use_linear else (inner, ch, 1, 1)
                s[pre + "proj_in.bias"] = (inner,)
                s[pre + "proj_out.weight"] = (ch, inner) if self.use_linear else (ch, inner, 1, 1)
                s[pre + "proj_out.bias"] = (ch,)
                for k in range(self.transformer_depth):
                    t = pre + f"transformer_blocks.{k}."
                    for a, cd in (("attn1.", inner), ("attn2.", ctx)):
                        s[t + a + "to_q.weight"] = (inner, inner)
                        s[t + a + "to_k.weight"] = (inner, cd)
                        s[t + a + "to_v.weight"] = (inner, cd)
                        s[t + a + "to_out.0.weight"] = (inner, inner)
                        s[t + a + "to_out.0.bias"] = (inner,)
                    s[t + "ff.net.0.proj.weight"] = (inner * 8, inner)
                    s[t + "ff.net.0.proj.bias"] = (inner * 8,)
                    s[t + "ff.net.2.weight"] = (inner, inner * 4)
                    s[t + "ff.net.2.bias"] = (inner,)
                    for n in ("norm1", "norm2", "norm3"):
                        s[t + n + ".gamma"] = (inner,)
                        s[t + n + ".beta"] = (inner,)
            elif kind == "down" and self.conv_resample:     # Downsample(use_conv=False) is a parameter-free average pool
                s[pre + "op.conv.weight"] = (layer[1], layer[1], 3, 3)
                s[pre + "op.conv.bias"] = (layer[1],)
            elif kind == "up" and self.conv_resample:
                s[pre + "conv.conv.weight"] = (layer[1], layer[1], 3, 3)
                s[pre + "conv.conv.bias"] = (layer[1],)
        self._head_shapes(s)
        return s

    def _head_shapes(self, s):
        """What the network owns behind its blocks: `out` (and `id_predictor`).  ControlNet has its zero convs here."""
        mc = self.model_channels
        s["out.0.gamma"] = (mc,)
        s["out.0.beta"] = (mc,)
        s["out.2.conv.weight"] = (self.out_channels, mc, 3, 3)
        s["out.2.conv.bias"] = (self.out_channels,)
        if self.n_embed is not None:        # the reference builds `out` as well (openaimodel.py:520-531); only id_predictor runs
            s["id_predictor.0.gamma"] = (mc,)
            s["id_predictor.0.beta"] = (mc,)
            s["id_predictor.1.conv.weight"] = (self.n_embed, mc, 1, 1)
            s["id_predictor.1.conv.bias"] = (self.n_embed,)

    def _lora_targets(self):
        """(reference name of the Dense, out, in) of every LoRA target, in structure order."""
        for pre, layer in named_layers(self):
            if layer[0] != "st":
                continue
            inner = layer[2] * layer[3]
            for k in range(self.transformer_depth):
                t = pre + f"transformer_blocks.{k}."
                for a, cd in (("attn1.", inner), ("attn2.", self.context_dim)):
                    for n in _LORA_TARGETS:
                        yield t + a + n, inner, (inner if n in ("to_q", "to_out.0") else cd)

    def lora_parameter_shapes(self, prefix=LORA_PREFIXES[0]):
        """name -> shape of the adapter parameters: for to_q / to_k / to_v / to_out.0 of attn1 and attn2 of every transformer
        block, `<dense>.<prefix>lora_a` (rank, in) and `<dense>.<prefix>lora_b` (out, rank).  `prefix` is one of LORA_PREFIXES, the
        two names the delta-tuning package has used; the reference tree does not contain that package, so these key names are
        UNPINNED."""
        if prefix not in LORA_PREFIXES:
            raise ValueError(f"lora_parameter_shapes: prefix must be one of {LORA_PREFIXES}")
        s = {}
        for name, nout, nin in self._lora_targets():
            s[f"{name}.{prefix}lora_a"] = (self.lora_rank, nin)
            s[f"{name}.{prefix}lora_b"] = (nout, self.lora_rank)
        return s

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, params, strict=True):
        """params: name -> array/tensor keyed by the reference's parameter names.  Packs everything into
        the kernels' layouts on the device (fp16 weights, fp32 biases / norm affine)."""
        shapes = self.parameter_shapes()
        who = "UNetModel.load_state_dict"
        lora_params = {}
        if self.enable_lora:    # the adapter may ride in the same dict (one merged checkpoint) or come in a second call
            lora_params = {k: v for k, v in params.items() if is_lora_key(k)}
            params = {k: v for k, v in params.items() if k not in lora_params}
        # every owned parameter is needed to run: missing keys always raise; strict additionally rejects unexpected ones
        L = WeightLoader(params, self.device, who)
        L.check(shapes, unexpected=strict)
        if lora_params:
            lora_params = self._check_lora(lora_params, strict, who)
        ln_fold = os.environ.get("MDX_UNET_LN_FOLD", "1") != "0"
        qkv_merge = os.environ.get("MDX_UNET_QKV_MERGE", "1") != "0"
        w = L.w
        w["te0.w"], w["te0.b"] = L.raw("time_embed.0.weight", f16), L.vec("time_embed.0.bias")
        w["te2.w"], w["te2.b"] = L.raw("time_embed.2.weight", f16), L.vec("time_embed.2.bias")
        if self.num_classes is not None:
            w["label_emb"] = L.raw("label_emb.embedding_table", f32)
        emb_w, emb_b, self._emb_off = [], [], {}
        off = 0
        for pre, layer in named_layers(self):
            kind = layer[0]
            if kind == "conv":
                w[pre + "w"], w[pre + "b"] = L.conv(pre + "conv.weight", cin_pad=self.cin_pad), L.vec(pre + "conv.bias")
            elif kind in ("res", "resdown", "resup"):
                cin, cout = layer[1], layer[2]
                for n in ("in_layers_norm", "out_layers_norm"):
                    L.norm(pre + n, pre + n)
                w[pre + "conv1.w"], w[pre + "conv1.b"] = L.conv(pre + "in_layers_conv.conv.weight"), L.vec(pre + "in_layers_conv.conv.bias")
                w[pre + "conv2.w"], w[pre + "conv2.b"] = L.conv(pre + "out_layers_conv.conv.weight"), L.vec(pre + "out_layers_conv.conv.bias")
                if cin != cout:
                    w[pre + "skip.w"], w[pre + "skip.b"] = L.conv(pre + "skip_connection.conv.weight"), L.vec(pre + "skip_connection.conv.bias")
                emb_w.append(L.raw(pre + "emb_layers.1.weight", f16))
                emb_b.append(L.vec(pre + "emb_layers.1.bias"))
                self._emb_off[pre] = off
                off += cout * (2 if self.use_scale_shift_norm else 1)
            elif kind == "st":
                inner = layer[2] * layer[3]
                L.norm(pre + "norm", pre + "norm")
                proj = {}
                for n in ("proj_in", "proj_out"):
                    wt = L.raw(pre + n + ".weight", f16)
                    proj[n] = wt.reshape(wt.shape[0], wt.shape[1])     # 1x1 conv == Dense in NHWC
                    w[pre + n + ".w"], w[pre + n + ".b"] = L.dense(proj[n]), L.vec(pre + n + ".bias")
                for k in range(self.transformer_depth):
                    t = pre + f"transformer_blocks.{k}."
                    # self-attention: ONE [q | k | v] projection launch; the q|k columns are stored row-major and the v columns
                    # transposed (mdx_gemm_desc.n_split), which needs 2 * inner to be a multiple of 128
                    wq, wk, wv = (L.raw(t + f"attn1.to_{n}.weight", f16) for n in "qkv")
                    for n in ("norm1", "norm2", "norm3"):
                        L.norm(t + n, t + n)
                    # LayerNorm fold (mdx_gemm_desc.ln_stats): norm1/2/3 disappear into the GEMMs around them -- the consumer
                    # weights become gamma (.) W, with S = row sums and W beta (+ b) as the bias (ops.fold_layernorm)
                    fold = inner % 64 == 0 and ln_fold

                    def put(name, wt, norm, bias=None):
                        if fold:
                            wt, w[name + ".s"], w[name + ".cb"] = ops.fold_layernorm(wt, w[t + norm + ".g"], w[t + norm + ".b"], bias)
                        w[name + ".w"] = L.dense(wt)
                    if (2 * wq.shape[0]) % 128 == 0 and qkv_merge:
                        put(t + "attn1.qkv", torch.cat([wq, wk, wv], 0), "norm1")
                    else:   # fall back to a [q | k] launch and a transposed-store v launch
                        w[t + "attn1.qk.w"] = L.dense(torch.cat([wq, wk], 0))
                        w[t + "attn1.v.w"] = L.dense(wv)
                    wq2 = L.raw(t + "attn2.to_q.weight", f16)
                    put(t + "attn2.q", wq2, "norm2")
                    w[t + "attn2.k.w"] = L.dense(t + "attn2.to_k.weight")
                    w[t + "attn2.v.w"] = L.dense(t + "attn2.to_v.weight")
                    wo = {a: L.raw(t + a + ".to_out.0.weight", f16) for a in ("attn1", "attn2")}
                    for a in ("attn1", "attn2"):
                        w[t + a + ".o.w"], w[t + a + ".o.b"] = L.dense(wo[a]), L.vec(t + a + ".to_out.0.bias")
                    # GEGLU (attention.py:41-51): interleave 64 'x' rows with their 64 'gate' rows per 128-wide tile
                    gw, gb = L.raw(t + "ff.net.0.proj.weight", f16), L.vec(t + "ff.net.0.proj.bias")
                    half = 4 * inner
                    w[t + "ff1.b"] = ops.geglu_interleave(gb[:half], gb[half:], 64)
                    put(t + "ff1", ops.geglu_interleave(gw[:half], gw[half:], 64), "norm3", w[t + "ff1.b"])
                    w2 = L.raw(t + "ff.net.2.weight", f16)
                    w[t + "ff2.w"], w[t + "ff2.b"] = L.dense(w2), L.vec(t + "ff.net.2.bias")
                    # row-local fused tail (mdx_st_tail_f16): to_out1 .. proj_out as one launch where a level has enough
                    # token rows to fill the chip; its own packing (MFMA-fragment-major per-wave streams, unfolded LayerNorms)
                    if (self.transformer_depth == 1 and inner == layer[1]
                            and ops.st_tail_supported(inner, layer[2], layer[3], 64, 64)):
                        w[t + "tail.stream"], w[t + "tail.vec"] = ops.pack_st_tail(
                            wo["attn1"], wq2, wo["attn2"], gw, w2, proj["proj_out"],
                            w[t + "attn1.o.b"], w[t + "norm2.g"], w[t + "norm2.b"], w[t + "attn2.o.b"], w[t + "norm3.g"],
                            w[t + "norm3.b"], gb, w[t + "ff2.b"], w[pre + "proj_out.b"])
                        if ops.st_head_supported(inner, 64, 64):
                            w[t + "head.stream"], w[t + "head.vec"] = ops.pack_st_head(
                                proj["proj_in"], wq, wk, wv, w[pre + "norm.g"], w[pre + "norm.b"],
                                w[pre + "proj_in.b"], w[t + "norm1.g"], w[t + "norm1.b"])
            elif kind == "down" and self.conv_resample:
                w[pre + "w"], w[pre + "b"] = L.conv(pre + "op.conv.weight"), L.vec(pre + "op.conv.bias")
            elif kind == "up" and self.conv_resample:
                w[pre + "w"], w[pre + "b"] = L.conv(pre + "conv.conv.weight"), L.vec(pre + "conv.conv.bias")
                if layer[1] % 64 == 0 and ops.get_option("unet_subpixel_upsample"):
                    # sub-pixel form of nearest-2x + conv (mdx_gemm_desc.w_sub): 4 Cin instead of 9 Cin products per output; the
                    # library uses it where the eight-wave conv core applies and falls back to `w` + the upsampling gather elsewhere
                    w[pre + "wsub"] = ops.pack_subpixel_conv_weight(L.raw(pre + "conv.conv.weight", f32))
        w["emb.w"] = torch.cat(emb_w, 0).contiguous()
        w["emb.b"] = torch.cat(emb_b, 0).contiguous()
        self._emb_total = off
        unused = self._load_head(L)
        self._frag_w = {}
        self._geglu80 = {}
        self._ff_proj = {}
        self._plans = {}
        self._ctx_key = None
        self._ctx_ref = None
        self._lora = None       # a new base load drops the adapter (it is merged again below when `params` carried one)
        self._lora_base, self._lora_sites = {}, {}
        if self.enable_lora:
            for name, _, _ in self._lora_targets():
                self._lora_base[name] = L.own(name + ".weight", f32)
        self.w = L.finish(shapes, unused=unused)
        if self.enable_lora:
            self._lora_sites = self._find_lora_sites()
            if lora_params:
                self._set_lora(lora_params)
        return self

    def _load_head(self, L):
        """Pack what _head_shapes names; returns the names the class owns but never runs."""
        w = L.w
        # with n_embed the reference builds `out` as well (openaimodel.py:520-531); only id_predictor runs
        norm, conv = ("out.0", "out.2.conv") if self.n_embed is None else ("id_predictor.0", "id_predictor.1.conv")
        w["out.g"], w["out.b"] = L.vec(norm + ".gamma"), L.vec(norm + ".beta")
        w["out.w"] = L.conv(conv + ".weight", cout_pad=self.cout_pad)
        w["out.cb"] = L.vec(conv + ".bias", pad=self.cout_pad)
        return () if self.n_embed is None else ["out.0.gamma", "out.0.beta", "out.2.conv.weight", "out.2.conv.bias"]

    def weight_bytes(self):
        """Bytes of device memory the loaded weights hold; with enable_lora this includes the fp32 copies of the LoRA target
        matrices (the merge source) and a loaded adapter."""
        n = sum(t.numel() * t.element_size() for t in self.w.values())
        n += sum(t.numel() * t.element_size() for t in self._lora_base.values())
        if self._lora:
            n += sum(a.numel() * 4 + b.numel() * 4 for a, b in self._lora.values())
        return n

    # ------------------------------------------------------------------ LoRA
    def _find_lora_sites(self):
        """Every place a LoRA target matrix lives in self.w, as keyword arguments of ops.lora_merge.  The plan-time copies
        self._frag_w (3x3 conv weights in fragment-major form), self._geglu80 (ff.net.0.proj re-packed at unit 80) and self._ff_proj
        (proj_out composed with ff.net.2) hold no LoRA target -- conv and feed-forward weights are not adapted (WK attention.py:118-126) -- so they are left alone."""
        w = self.w
        T, F = ops.LORA_TILED, ops.LORA_FRAG
        sites = {}
        for pre, layer in named_layers(self):
            if layer[0] != "st":
                continue
            inner = layer[2] * layer[3]
            ks = inner // 16
            for k in range(self.transformer_depth):
                t = pre + f"transformer_blocks.{k}."

                def tiled(key, n0=0, dst_n=inner, norm=None):
                    kw = dict(dst=w[key + ".w"], layout=T, dst_n0=n0, dst_N=dst_n)
                    if norm is not None and (key + ".s") in w:      # LayerNorm-folded consumer (ops.fold_layernorm)
                        kw.update(gamma=w[t + norm + ".g"], beta=w[t + norm + ".b"], S=w[key + ".s"][n0:], cb=w[key + ".cb"][n0:])
                    return kw

                def frag(key, slot, per_wave):
                    return dict(dst=w[t + key], layout=F, dst_N=inner, piece_stride=per_wave * ks, piece_offset=slot * ks)
                merged = (t + "attn1.qkv.w") in w
                for i, n in enumerate("qkv"):
                    if merged:
                        here = [tiled(t + "attn1.qkv", i * inner, 3 * inner, "norm1")]
                    elif n == "v":
                        here = [tiled(t + "attn1.v")]
                    else:
                        here = [tiled(t + "attn1.qk", i * inner, 2 * inner)]
                    if (t + "head.stream") in w:        # [proj_in | to_q | to_k | to_v] per wave (ops.pack_st_head)
                        here.append(frag("head.stream", 1 + i, 4))
                    sites[t + f"attn1.to_{n}"] = here
                sites[t + "attn2.to_q"] = [tiled(t + "attn2.q", norm="norm2")]
                sites[t + "attn2.to_k"] = [tiled(t + "attn2.k")]
                sites[t + "attn2.to_v"] = [tiled(t + "attn2.v")]
                sites[t + "attn1.to_out.0"] = [tiled(t + "attn1.o")]
                sites[t + "attn2.to_out.0"] = [tiled(t + "attn2.o")]
                if (t + "tail.stream") in w:            # [to_out1 | to_q2 | to_out2 | ...] per wave (ops.pack_st_tail)
                    for slot, name in enumerate(("attn1.to_out.0", "attn2.to_q", "attn2.to_out.0")):
                        sites[t + name].append(frag("tail.stream", slot, 16))
        assert set(sites) == set(self._lora_base)
        return sites

    def _check_lora(self, params, strict, who):
        """Validate an adapter dict (either key prefix, not both) -> {canonical-prefix name: value}.  Raises before anything
        is written."""
        found = {m.group(2) for m in map(_LORA_KEY.match, params) if m}
        if len(found) > 1:
            raise KeyError(f"{who}: adapter keys mix the prefixes {sorted(found)}")
        prefix = found.pop() if found else LORA_PREFIXES[0]
        shapes = self.lora_parameter_shapes(prefix)
        WeightLoader(params, self.device, who).check(shapes, unexpected=strict)
        return {k.replace("." + prefix, "." + LORA_PREFIXES[0]): params[k] for k in shapes}

    def _set_lora(self, checked):
        p, L = LORA_PREFIXES[0], WeightLoader(checked, self.device, "UNetModel.load_lora_state_dict")
        self._lora = {name: (L.own(f"{name}.{p}lora_a", f32), L.own(f"{name}.{p}lora_b", f32)) for name in self._lora_base}
        self._merge_lora()

    def _merge_lora(self):
        """(Re)write every LoRA target from its fp32 base and the current adapter / scale: one ops.lora_merge launch per place
        the matrix lives.  In place -- the tensors of self.w keep their addresses, so plans and captured graphs stay valid; only
        the cached context projections (attn2.to_k / to_v of the text context) are stale and run again on the next call."""
        scale = self._lora_mult * self.lora_alpha / self.lora_rank
        for name, base in self._lora_base.items():
            a, b = self._lora[name] if self._lora else (None, None)
            for site in self._lora_sites[name]:
                ops.lora_merge(base, A=a, B=b, scale=scale, **site)
        self._ctx_key = None
        self._ctx_ref = None

    def _need_lora(self, who):
        if not self.enable_lora:
            raise MdxError(f"UNetModel.{who}: the model was built without enable_lora=True")
        if self.w is None:
            raise MdxError(f"UNetModel.{who}: load_state_dict() must be called first (the adapter is merged into the base weights)")

    def load_lora_state_dict(self, params, strict=True):
        """Apply a LoRA adapter ({name: array} keyed `<dense>.tk_delta_lora_a|b` or `<dense>.mindpet_delta_lora_a|b`): the
        second call of the reference's flow (WK txt2img.py:222-225).  Missing adapter keys always raise; strict additionally
        rejects unexpected ones.  Replaces a previously loaded adapter; buffers, plans and graphs are kept."""
        self._need_lora("load_lora_state_dict")
        self._set_lora(self._check_lora(dict(params), strict, "UNetModel.load_lora_state_dict"))
        return self

    def set_lora_scale(self, m=1.0):
        """Adapter strength: the merged weights become W + m * (lora_alpha / lora_rank) * B A (m = 1: the reference's layer)."""
        self._need_lora("set_lora_scale")
        m = float(m)
        if not math.isfinite(m):
            raise ValueError("set_lora_scale: the multiplier must be finite")
        self._lora_mult = m
        if self._lora:
            self._merge_lora()
        return self

    def unload_lora(self):
        """Back to the base weights (bit for bit what load_state_dict packed)."""
        self._need_lora("unload_lora")
        if self._lora:
            self._lora = None
            self._merge_lora()
        return self

    @property
    def lora_loaded(self):
        return self._lora is not None

    # ------------------------------------------------------------------ planning
    class _Plan:
        pass

    def _planner(self, B, H, W, fuse_head, selfctx, control):
        return _UNetPlanner(self, B, H, W, fuse_head, selfctx, control)

    def _plan(self, B, H, W, _selfctx=False, control=False):
        # _selfctx: the `context=None` form of construct() (DiffusionWrapper keys None / 'concat' / 'adm', WK ddpm.py:361-374):
        # attn2 attends to its own normalised input (attention.py:133 `context = default(context, x)`), so its to_k / to_v run per
        # step on LayerNorm(tokens) instead of once on the text context; plans of the two forms are kept side by side.
        # control: the plan of forward_nhwc(control=) -- one ops.ControlAdd launch behind the middle block; a plan of its own,
        # so the plain plan and everything it launches are what they are without ControlNet
        key = (B, H, W, "selfctx") if _selfctx else (B, H, W, "control") if control else (B, H, W)
        if key in self._plans:
            return self._plans[key]
        if self.w is None:
            raise MdxError("UNetModel: load_state_dict() must be called before the first forward")
        for lvl in range(len(self.channel_mult) - 1):
            if (H >> lvl) % 2 or (W >> lvl) % 2:
                raise MdxError(f"UNetModel: latent {H}x{W} is not divisible by 2^{len(self.channel_mult) - 1}")
        try:
            P = self._planner(B, H, W, True, _selfctx, control).build()
        except _HeadNotWired:
            # a fused head whose input tensor's producer cannot emit column statistics in its final launch form: plan again
            # with the unfused GroupNorm / proj_in / qkv launches (plans are built once per shape)
            P = self._planner(B, H, W, False, _selfctx, control).build()
        self._plans[key] = P
        return P

    # ------------------------------------------------------------------ execution
    def _ensure_context(self, P, context):
        """Project the text context through every attn2.to_k / to_v once per context tensor: it is constant
        across the sampling loop (the reference recomputes it at 16 sites x 51 calls)."""
        # The cache is tied to the tensor OBJECT (weak reference) and its version counter, not to its address: a later
        # conditioning tensor can be allocated at the same address with the same version, and must not hit the cache.
        key = (context.data_ptr(), context._version, tuple(context.shape), context.dtype, id(P))
        alive = self._ctx_ref() if self._ctx_ref is not None else None
        if key == self._ctx_key and alive is context:
            return
        Bc, T, Dc = context.shape
        if Bc != P.B or Dc != self.context_dim:
            raise MdxError(f"context shape {tuple(context.shape)} does not match batch {P.B} / context_dim {self.context_dim}")
        if T > self.max_context_len:
            raise MdxError(f"context length {T} > max_context_len={self.max_context_len}")
        P.ctx_pad.zero_()
        P.ctx_pad[:, :T].copy_(context)
        P.ctx_len = T
        for d in getattr(P, "xattn_descs", ()):      # the query projections that carry their cross-attention (mdx_gemm_desc.xattn_len)
            d.xattn_len = T
        for op in P.ctxops:
            op()
        self._ctx_key = key
        self._ctx_ref = weakref.ref(context)
        # the attention ops read P.ctx_len at call time; a captured graph bakes it in
        if getattr(P, "graph_ctx_len", None) != T:
            P.graph = None
            P.dup_graph = None

    def time_embedding_table(self, t):
        """Everything the UNet derives from the timestep alone -- sinusoid, time_embed MLP and the 22 ResBlock
        emb_layers (openaimodel.py:550-551, 150-157, 188) -- for ALL the steps of a sampling run in one batched pass:
        t [S] -> [S, emb_total] fp32.  A sampler computes it once per sample() (the 51 MB of emb weights are then read
        once per run instead of once per step) and passes row i to forward_nhwc(..., temb=row)."""
        if self.w is None:
            raise MdxError("UNetModel: load_state_dict() must be called before time_embedding_table()")
        if self.num_classes is not None:
            raise MdxError("UNetModel: a class-conditional UNet adds label_emb(y) before the ResBlock projections; "
                           "there is no timestep-only table")
        t = torch.as_tensor(t, dtype=f32).to(self.device).reshape(-1).contiguous()
        w = self.w
        e0 = ops.timestep_embedding(t, self.model_channels)
        e1 = ops.dense_small(e0, w["te0.w"], w["te0.b"], act_out=True)
        e2 = ops.dense_small(e1, w["te2.w"], w["te2.b"])
        return ops.dense_small(e2, w["emb.w"], w["emb.b"], act_in=True)

    def forward_nhwc(self, x, timesteps, context=None, temb=None, y=None, cfg_dup=False, control=None):
        """Run the UNet; returns the plan's static NHWC fp16 eps buffer [B, H*W, 8] (first 4 channels valid).
        The buffer is overwritten by the next call.  temb: optional row(s) of time_embedding_table() for `timesteps`
        ([emb_total] or [B, emb_total]); the time-embedding launches are then skipped.  y: [B] class labels of a
        class-conditional UNet (num_classes).  cfg_dup: the caller states that the two halves of the batch carry the SAME x and
        timesteps and differ only in `context` (classifier-free guidance, plms.py:192-195 `x_in = cat([x] * 2)`): the launches in
        front of the first cross-attention may then run on one half (_dup_body).  control: a Control -- the residuals of a
        ControlNet evaluation, added to the skip connections and the middle block's output by one launch (the plan keyed
        (B, H, W, "control")); such a call needs a text context, takes no y and makes no use of cfg_dup."""
        if control is not None:
            if context is None or y is not None:
                raise MdxError("UNetModel: control= needs a text context and takes no class labels")
            if not isinstance(control, Control):
                raise MdxError("UNetModel: control= takes an openaimodel.Control")
            cfg_dup = False
        if (y is not None) != (self.num_classes is not None):      # openaimodel.py:545-547
            raise MdxError("UNetModel: must specify y if and only if the model is class-conditional")
        if y is not None and temb is not None:
            raise MdxError("UNetModel: time_embedding_table() rows do not carry the label embedding; pass timesteps with y")
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise MdxError("UNetModel: x must be a CUDA(HIP) tensor (no CPU fallback)")
        B, C, H, W = x.shape
        if C != self.in_channels:
            raise MdxError(f"UNetModel: expected {self.in_channels} input channels, got {C}")
        if context is None:
            # construct(x, t) / construct(x, t, y=) of DiffusionWrapper keys None / 'concat' / 'adm' (WK ddpm.py:361-374): attn2's
            # to_k / to_v (Dense(context_dim, inner)) then see the block's own tokens, which only type-checks -- in the reference
            # as here -- when context_dim equals the transformer width at every attention level
            if getattr(self, "_selfctx_bad", None) is None:      # (structure and context_dim are fixed at construction: checked once,
                self._selfctx_bad = sorted({l[2] * l[3] for _, l in named_layers(self)      # not on every sampler step)
                                            if l[0] == "st" and l[2] * l[3] != self.context_dim})
            bad = self._selfctx_bad
            if bad:
                raise MdxError(f"UNetModel: context=None makes attn2 attend to its own input (attention.py:133), which needs "
                               f"context_dim == transformer width; context_dim={self.context_dim}, widths {bad}")
            P = self._plan(B, H, W, _selfctx=True)
        else:
            P = self._plan(B, H, W, control=control is not None)
            self._ensure_context(P, context)
        if control is not None:         # device tables the captured launch reads: nothing here touches the graph
            P.control.set_sources(control.sources, control.rows)
            P.control.set_scale(control.scale)
        self._evaluate(P, x, timesteps, temb, y, cfg_dup and context is not None and y is None)
        return P.eps_nhwc

    def _evaluate(self, P, x, timesteps, temb=None, y=None, cfg_dup=False):
        """One evaluation of plan P: x and the timestep rows into the plan's static inputs, then the captured graph (or the op
        list).  The caller has made the plan's context current."""
        B = P.B
        P.x_static.copy_(x)
        if temb is not None:
            if temb.shape[-1] != self._emb_total or temb.dtype != f32:
                raise MdxError(f"UNetModel: temb must be fp32 [.., {self._emb_total}] rows of time_embedding_table()")
            P.emb_all.copy_(temb)          # [emb_total] broadcasts over the batch
        else:
            P.t_static.copy_(timesteps.to(device=self.device, dtype=f32) if isinstance(timesteps, torch.Tensor)
                             else torch.as_tensor(timesteps, dtype=f32, device=self.device))
            if y is not None:
                yy = torch.as_tensor(y).to(device=self.device, dtype=torch.long).reshape(-1)
                if yy.shape[0] != B:
                    raise MdxError(f"UNetModel: y has {yy.shape[0]} labels for a batch of {B}")
                if int(yy.min()) < 0 or int(yy.max()) >= self.num_classes:
                    raise MdxError(f"UNetModel: class label outside [0, {self.num_classes})")
                P.y_static.copy_(yy)
            for op in P.main[:P.temb_ops]:
                op()
        dup = self._dup_body(P) if cfg_dup else None
        if dup is not None and ops.get_option("unet_cfg_dup_check"):
            hb = B // 2
            same = torch.equal(P.x_static[:hb], P.x_static[hb:]) and torch.equal(P.emb_all[:hb], P.emb_all[hb:])
            if not same:
                raise MdxError("UNetModel: cfg_dup=True, but the two halves of the batch do not carry the same x / timesteps")
        if self.use_graph and not P.graph_failed:
            if dup is not None:
                if P.dup_graph is None:
                    self._capture(P, dup)
                if P.dup_graph is not None:
                    P.dup_graph.replay()
                    return
            if P.graph is None:
                self._capture(P)
            if P.graph is not None:
                P.graph.replay()
                return
        body = dup if dup is not None else P.main[P.temb_ops:]
        for op in body:
            op()
        self.last_launch_count = P.temb_ops + len(body)

    def _dup_body(self, P):
        """The op list of one evaluation whose batch is [uncond ; cond] of the SAME latents (classifier-free guidance, plms.py:192-195):
        until the first cross-attention both halves compute the same numbers -- conv_in, the first ResBlock, the first
        SpatialTransformer's GroupNorm / proj_in / qkv, its self-attention (at 64^2 .. 96^2 tokens the largest attention of the
        network) and, where it is a launch of its own in both plans, attn1's output projection.  Those launches run from the plan of
        HALF the batch; its live tensors (the ResBlock output, the token stream and the attention output -- or the token stream behind
        to_out and its LayerNorm row statistics) are then written to both halves of this plan's buffers and this plan continues
        with what follows.  conv_in itself runs at the full batch (its output is the outermost skip connection, with column
        statistics for the last GroupNorm: writing it costs what copying it would).  None when the option is off
        (ops option unet_cfg_dup = smallest batch, 0 = never), the batch is odd or the network has no attention at its first level."""
        mn = ops.get_option("unet_cfg_dup")
        if not mn or P.B < mn or P.B % 2 or P.ck is None:
            return None
        if hasattr(P, "dup_body"):
            return P.dup_body
        P.dup_body = None
        h = P.B // 2
        PA = self._plan(h, P.H, P.W)
        if PA.ck is None:
            return None
        # the splice point: behind attn1's output projection when both plans launch it (a plan whose fused tail starts at to_out
        # does not), else behind the self-attention
        late = "op2" in P.ck and "op2" in PA.ck and len(P.ck["live2"]) == len(PA.ck["live2"])
        ko, kl = ("op2", "live2") if late else ("op", "live")
        ib, ic = P.main.index(P.ck[ko]), P.main.index(P.ck["conv_in"])
        ja, jc = PA.main.index(PA.ck[ko]), PA.main.index(PA.ck["conv_in"])
        xin_a, xin_b = PA.ck["xin"], P.ck["xin"]
        copies = [lambda: xin_a.copy_(xin_b[:h]), lambda: PA.emb_all.copy_(P.emb_all[:h])]
        spread = []
        for src, dst in zip(PA.ck[kl], P.ck[kl]):
            if not (dst.shape[0] == 2 * src.shape[0] and dst.shape[1:] == src.shape[1:] and dst.dtype == src.dtype):
                raise MdxError(f"UNetModel: guidance-duplicate prefix: live tensors of the two plans do not pair up "
                               f"({tuple(src.shape)} vs {tuple(dst.shape)})")
            spread.append(lambda src=src, dst=dst, k=src.shape[0]: (dst[:k].copy_(src), dst[k:].copy_(src)))
        P.dup_half = PA
        P.dup_body = P.main[P.temb_ops:ic + 1] + copies + PA.main[jc:ja + 1] + spread + P.main[ib + 1:]
        small = {"kind": "small", "flops": 0, "launches": 1, "info": "guidance-duplicate prefix: copy"}
        P.dup_meta = (P.meta[P.temb_ops:ic + 1] + [dict(small) for _ in copies] + PA.meta[jc:ja + 1]
                      + [dict(small, launches=2) for _ in spread] + P.meta[ib + 1:])     # (parallel to dup_body, for the profilers)
        return P.dup_body

    def _capture(self, P, dup=None):
        """Capture the whole forward as one hipGraph (kills ~450 launch gaps per call)."""
        body = dup if dup is not None else P.main[P.temb_ops:]   # the graph starts from P.emb_all (filled eagerly or from the sampler's table)
        graphs = capture_or_eager([body])
        if graphs is None:
            P.graph, P.graph_failed = None, True
        elif dup is not None:
            P.dup_graph = graphs[0]
        else:
            P.graph = graphs[0]
        if graphs is not None:
            P.graph_ctx_len = P.ctx_len

    def construct(self, x, timesteps=None, context=None, y=None):
        """openaimodel.py:536-576.  x [N,C,H,W], timesteps [N], context [N,T,context_dim] -> eps [N,C,H,W] fp32."""
        eps = self.forward_nhwc(x, timesteps, context, y=y)
        B, _, H, W = x.shape
        return ops.nhwc_to_nchw(eps, self.final_channels, H, W)

    __call__ = construct
    forward = construct


class _HeadNotWired(Exception):
    """A fused SpatialTransformer head / GroupNorm-in-conv launch did not get its column statistics (UNetModel._plan)."""


class _UNetPlanner(PlanBuilder):
    """One (B, H, W) plan of a UNetModel: walks the block structure once and emits the op list (planner.PlanBuilder)."""

    def __init__(self, net, B, H, W, fuse_head, selfctx, control=False):
        super().__init__(net.device, B, track_producers=True)
        self.net, self.w, self.H, self.W = net, net.w, H, W
        self.fuse_head, self.selfctx, self.control = fuse_head, selfctx, control
        self.TC = net.max_context_len
        # keys the roofline metadata counts per query: one CLIP window at the default capacity, else the plan's capacity
        self.ctx_flops = 77 if self.TC == 80 else self.TC
        self.mod_ld = net._emb_total
        self.P = UNetModel._Plan()
        self.ctxops = []
        self.ck = {}            # checkpoint of the guidance-duplicate prefix (UNetModel._dup_body)
        self.hs = []            # (tensor, h, w) held as skip connections
        self.ctx_kv = {}        # transformer block -> cached context K / V^T buffers
        self.xattn_descs, self.ln_stats, self.tails, self.heads_fused, self.ragged_vt = [], {}, [], [], []

    def build(self):
        P, net, B = self.P, self.net, self.B
        dev = self.dev
        P.B, P.H, P.W = B, self.H, self.W
        P.x_static = torch.zeros((B, net.in_channels, self.H, self.W), dtype=f32, device=dev)
        P.t_static = torch.zeros((B,), dtype=f32, device=dev)
        self.time_embedding()
        xin = self.get((B, self.H * self.W, net.cin_pad))
        self.emit(lambda: ops.nchw_to_nhwc(P.x_static, net.cin_pad, out=xin), "small")
        self.ck["xin"] = xin
        # ---- context plan: to_k / to_v of attn2 for every SpatialTransformer (attention.py:119-121)
        P.ctx_pad = torch.zeros((B, self.TC, net.context_dim), dtype=f16, device=dev)
        P.ctx_len = 0
        self.walk(xin)
        for t, (kc, vtc) in self.ctx_kv.items():
            inner = kc.shape[2]
            self.dense(P.ctx_pad, B, self.TC, net.context_dim, inner, self.w[t + "attn2.k.w"], out=kc, out_ld=inner,
                       oplist=self.ctxops)
            self.dense(P.ctx_pad, B, self.TC, net.context_dim, inner, self.w[t + "attn2.v.w"], out=vtc, out_ld=self.TC,
                       out_mode=ops.OUT_TRANSPOSED, oplist=self.ctxops)
        self.finish(P)
        P.ctxops, P.attn_ws, P.colstats = self.ctxops, self.attn_ws, self.colstats
        P.arena_bytes = self.A.total
        P.ln_stats = self.ln_stats
        P.tails = self.tails
        P.ragged_vt = self.ragged_vt    # (owned by the plan: descriptors hold raw pointers)
        P.heads_fused = self.heads_fused
        P.ctx_kv = self.ctx_kv          # the cached context K / V^T buffers: descriptors hold raw pointers only
        P.xattn_descs = self.xattn_descs
        P.ck = self.ck if (self.ck.get("op") is not None and not self.selfctx) else None
        P.graph = None
        P.dup_graph = None
        P.graph_failed = False
        return P

    def time_embedding(self):
        """openaimodel.py:550-551, 150-157: 4 tiny launches."""
        P, net, w, B, dev = self.P, self.net, self.w, self.B, self.dev
        mc, ted = net.model_channels, net.time_embed_dim
        t_emb = torch.empty((B, mc), dtype=f32, device=dev)
        e1 = torch.empty((B, ted), dtype=f32, device=dev)
        emb = torch.empty((B, ted), dtype=f32, device=dev)
        P.emb_all = torch.empty((B, net._emb_total), dtype=f32, device=dev)
        self.emit(lambda: ops.timestep_embedding(P.t_static, mc, out=t_emb), "small")
        self.emit(lambda: ops.dense_small(t_emb, w["te0.w"], w["te0.b"], act_out=True, out=e1), "small", 2 * B * mc * ted)
        self.emit(lambda: ops.dense_small(e1, w["te2.w"], w["te2.b"], out=emb), "small", 2 * B * ted * ted)
        if net.num_classes is not None:    # emb + label_emb(y) (openaimodel.py:552-554): a [B, ted] row gather, outside the graph
            P.y_static = torch.zeros((B,), dtype=torch.long, device=dev)
            self.emit(lambda: emb.add_(w["label_emb"].index_select(0, P.y_static)), "small")
        self.emit(lambda: ops.dense_small(emb, w["emb.w"], w["emb.b"], act_in=True, out=P.emb_all), "small",
                  2 * B * ted * net._emb_total)
        P.temb_ops = len(self.main)   # main[:temb_ops] only fill P.emb_all: skipped when the caller hands the rows in

    # ------------------------------------------------------------------ the walk (openaimodel.py:556-576)
    def held(self, t):        # still needed as a skip connection?
        return any(t is s_[0] for s_ in self.hs)

    def walk(self, xin):
        net, w, B = self.net, self.w, self.B
        h, wd = self.H, self.W
        cur = None
        for i, blk in enumerate(net.input_blocks):
            for j, layer in enumerate(blk):
                pre = f"input_blocks.{i}.{j}."
                if layer[0] == "conv":
                    cur, h, wd = self.conv3(xin, net.cin_pad, layer[2], w[pre + "w"], w[pre + "b"], h, wd)
                    self.ck["conv_in"] = self.main[-1]
                    self.release(xin)
                    continue
                new, h2, w2 = self.layer_op(pre, layer, cur, None, h, wd)
                if not self.held(cur):
                    self.release(cur)
                cur, h, wd = new, h2, w2
            self.hs.append((cur, h, wd))
        self.ck.setdefault("op", None)      # (no self-attention in input block 1: no guidance-duplicate prefix)
        for j, layer in enumerate(net.middle_block):
            new, h, wd = self.layer_op(f"middle_block.{j}.", layer, cur, None, h, wd)
            if not self.held(cur):
                self.release(cur)
            cur = new
        if self.control:
            self.control_add(cur)
        for i, blk in enumerate(net.output_blocks):
            skip, sh, sw = self.hs.pop()
            assert (sh, sw) == (h, wd)
            for j, layer in enumerate(blk):
                new, h, wd = self.layer_op(f"output_blocks.{i}.{j}.", layer, cur, skip if j == 0 else None, h, wd)
                self.release(cur)
                if j == 0:
                    self.release(skip)
                cur = new
        mc = net.model_channels
        a = self.get((B, h * wd, mc))
        # `out` = GroupNorm -> SiLU -> 3x3 conv; predict_codebook_ids: `id_predictor` = GroupNorm -> 1x1 conv (:520-531, 573-576)
        self.gn(cur, None, w["out.g"], w["out.b"], 1e-5, net.n_embed is None, a)
        self.P.eps_nhwc = torch.empty((B, h * wd, net.cout_pad), dtype=f16, device=self.dev)
        self.gemm(a=a, w=w["out.w"], N=net.cout_pad, B=B, H=h, W=wd, c1=mc, out=self.P.eps_nhwc, out_ld=net.cout_pad,
                  bias=w["out.cb"], ksize=3 if net.n_embed is None else 1)

    def control_add(self, mid):
        """The control plan's one extra op, behind the middle block (cldm.py ControlledUnetModel.forward): the ControlNet's
        residuals are added IN PLACE to every skip connection still held and to the middle block's output `mid`, by one
        ops.ControlAdd launch whose sources, row map and scales are device tables (UNetModel.forward_nhwc fills them per call).
        The column statistics a producer's epilogue wrote for these tensors describe them BEFORE the add: the tensors leave
        `producer`, so every GroupNorm that reads them from here on computes its own statistics (gn() looks the producer up
        when it is emitted).  Nothing crosses the add the other way either: a GroupNorm takes over its producer's split-K
        reduce (fuse_splitk_into_groupnorm) only with x2 None and the producer's launch right in front of it, and the
        GroupNorms behind the add read [cur | skip] pairs."""
        dsts = [s_[0] for s_ in self.hs] + [mid]
        ca = self.P.control = ops.ControlAdd(dsts)
        self.emit(ca.run, "small", 0, 1, f"control_add segments={len(dsts)} halves/row={sum(t.numel() for t in dsts) // self.B}")
        for t in dsts:
            self.producer.pop(t.data_ptr(), None)

    def layer_op(self, pre, layer, cur, skip, h, wd):
        net, w, B = self.net, self.w, self.B
        kind = layer[0]
        if kind == "res":
            return self.resblock(pre, cur, skip, layer[1], layer[2], h, wd)
        if kind in ("resdown", "resup"):
            return self.resblock(pre, cur, None, layer[1], layer[2], h, wd, mode=kind[3:])
        if kind == "st":
            return self.transformer(pre, cur, layer[1], layer[2], layer[3], h, wd), h, wd
        if kind == "down":          # Downsample openaimodel.py:63-88
            if net.conv_resample:
                return self.conv3(cur, layer[1], layer[1], w[pre + "w"], w[pre + "b"], h, wd, stride=2)
            new = self.get((B, (h // 2) * (wd // 2), layer[1]))
            self.emit(lambda cur=cur, new=new: ops.avgpool2x2(cur, B, h, wd, layer[1], out=new), "small")
            return new, h // 2, wd // 2
        if kind == "up":            # Upsample openaimodel.py:33-60 (the nearest-2x is folded into the conv's gather)
            if net.conv_resample:
                return self.conv3(cur, layer[1], layer[1], w[pre + "w"], w[pre + "b"], h, wd, upsample=1, wsub=w.get(pre + "wsub"))
            new = self.get((B, 4 * h * wd, layer[1]))
            self.emit(lambda cur=cur, new=new: ops.upsample_nearest2x(cur, B, h, wd, layer[1], out=new), "small")
            return new, 2 * h, 2 * wd
        raise ValueError(kind)

    # ------------------------------------------------------------------ ResBlock
    def gn_conv_ok(self, src, c_in, c_out, hh, ww, wt):
        """Can GroupNorm + SiLU of `src` run inside the 3x3 conv that consumes it (mdx_gemm_desc.gn_colstats)?  At the levels
        with at least `unet_gn_conv_fuse` output rows (below that the GroupNorm launch doubles as the split-K reduce of the
        conv in front of it), for inputs some GEMM launch produced (its epilogue supplies the statistics), convs that
        resolve to the HALO kernel with 64-column tiles."""
        B = self.B
        mrows = ops.get_option("unet_gn_conv_fuse")
        if not self.fuse_head or not mrows or B * hh * ww < mrows or c_in % 64 or c_in > 640 or (hh == 8 and ww == 8):
            return False
        if self.producer.get(src.data_ptr()) is None:
            return False
        probe = ops.make_gemm_desc(a=src, w=wt, N=c_out, B=B, H=hh, W=ww, c1=c_in, out=src, out_ld=c_out, ksize=3)
        q = ops.gemm_query(probe)
        return q[3] == 1 and q[1] == 64

    def conv2(self, pre, src, x, x2, xs, cin, cout, c2, ho, wo, fusable, gn=None):
        """The ResBlock's second conv + the skip path: skip_connection (1x1 over the raw input, openaimodel.py:174) as extra K
        tiles of the conv where that is possible (one launch less per ResBlock whose channel count changes, and the skip tensor
        never exists), else a launch of its own added as the conv's residual."""
        w, B = self.w, self.B
        if cin != cout and fusable and self.skip_fusable(src, cin - c2, c2, cout, ho, wo, w[pre + "conv2.w"]):
            if (pre + "conv2skip.b") not in w:
                w[pre + "conv2skip.b"] = (w[pre + "conv2.b"] + w[pre + "skip.b"]).contiguous()
            out, _, _ = self.conv3(src, cout, cout, w[pre + "conv2.w"], w[pre + "conv2skip.b"], ho, wo, gn=gn,
                                   skip=(x, x2, cin - c2, c2, w[pre + "skip.w"]))
            self.release(src)
            return out
        if cin != cout:
            skip = self.dense(x, B, x.shape[1], cin, cout, w[pre + "skip.w"], bias=w[pre + "skip.b"], src2=x2, c2=c2)
        else:
            assert x2 is None
            skip = xs
        out, _, _ = self.conv3(src, cout, cout, w[pre + "conv2.w"], w[pre + "conv2.b"], ho, wo, residual=skip, gn=gn)
        self.release(src)
        if skip is not x:
            self.release(skip)
        return out

    def resblock(self, pre, x, x2, cin, cout, h, wd, mode=None):
        """ResBlock.construct openaimodel.py:176-205; x2 = skip tensor of the (virtual) concat.  mode 'up' / 'down' is the
        resblock_updown form: nearest-2x / 2x2 average pooling of BOTH the normalised branch and the skip input
        (the nearest-2x of the branch is folded into conv1's gather)."""
        net, w, B, P = self.net, self.w, self.B, self.P
        c2 = 0 if x2 is None else x2.shape[2]
        hw = h * wd
        eoff = net._emb_off[pre]
        film = net.use_scale_shift_norm
        rowbias = None if film else P.emb_all[:, eoff:eoff + cout]  # view: pointer = base + eoff, ld = emb_total
        gn1 = x2 is None and mode is None and self.gn_conv_ok(x, cin, cout, h, wd, w[pre + "conv1.w"])
        a = None
        if not gn1:
            a = self.get((B, hw, cin))
            self.gn(x, x2, w[pre + "in_layers_norm.g"], w[pre + "in_layers_norm.b"], 1e-5, True, a)
        if mode == "up":
            assert x2 is None and cin == cout
            hbuf, ho, wo = self.conv3(a, cin, cout, w[pre + "conv1.w"], w[pre + "conv1.b"], h, wd, upsample=1, rowbias=rowbias)
            xs = self.get((B, ho * wo, cin))
            self.emit(lambda x=x, xs=xs: ops.upsample_nearest2x(x, B, h, wd, cin, out=xs), "small")
        elif mode == "down":
            assert x2 is None and cin == cout
            ap = self.get((B, hw // 4, cin))
            self.emit(lambda a=a, ap=ap: ops.avgpool2x2(a, B, h, wd, cin, out=ap), "small")
            hbuf, ho, wo = self.conv3(ap, cin, cout, w[pre + "conv1.w"], w[pre + "conv1.b"], h // 2, wd // 2, rowbias=rowbias)
            self.release(ap)
            xs = self.get((B, hw // 4, cin))
            self.emit(lambda x=x, xs=xs: ops.avgpool2x2(x, B, h, wd, cin, out=xs), "small")
        elif gn1:     # GroupNorm + SiLU of x inside conv1 (mdx_gemm_desc.gn_colstats): no GroupNorm launch, no normalised copy
            hbuf, ho, wo = self.conv3(x, cin, cout, w[pre + "conv1.w"], w[pre + "conv1.b"], h, wd, rowbias=rowbias,
                                      gn=(w[pre + "in_layers_norm.g"], w[pre + "in_layers_norm.b"], 1e-5))
            xs = x
        else:
            hbuf, ho, wo = self.conv3(a, cin, cout, w[pre + "conv1.w"], w[pre + "conv1.b"], h, wd, rowbias=rowbias)
            xs = x
        if a is not None:
            self.release(a)
        if (not film and mode is None) and self.gn_conv_ok(hbuf, cout, cout, ho, wo, w[pre + "conv2.w"]):
            # out_layers: GroupNorm + SiLU of conv1's output inside conv2 (statistics from conv1's epilogue)
            gnp = (w[pre + "out_layers_norm.g"], w[pre + "out_layers_norm.b"], 1e-5)
            return self.conv2(pre, hbuf, x, x2, xs, cin, cout, c2, ho, wo, True, gn=gnp), ho, wo
        a2 = self.get((B, ho * wo, cout))
        if film:    # use_scale_shift_norm: GN(h) * (1 + scale) + shift (openaimodel.py:193-198)
            self.gn(hbuf, None, w[pre + "out_layers_norm.g"], w[pre + "out_layers_norm.b"], 1e-5, True, a2,
                    scale=P.emb_all[:, eoff:eoff + cout], shift=P.emb_all[:, eoff + cout:eoff + 2 * cout])
        else:
            self.gn(hbuf, None, w[pre + "out_layers_norm.g"], w[pre + "out_layers_norm.b"], 1e-5, True, a2)
        self.release(hbuf)
        return self.conv2(pre, a2, x, x2, xs, cin, cout, c2, ho, wo, mode is None), ho, wo

    # ------------------------------------------------------------------ SpatialTransformer
    def geglu_tile160(self, d, t, inner):
        """The GEGLU projection of block `t` on the 128 x 160 tile where the library would run it there (tile table): that tile pairs
        column j with column j + 80, so the launch needs w / bias / S[n] packed at unit 80 (mdx_gemm_desc.geglu_unit).  The second
        packing is a row permutation of the first, made once per weight on first need and kept for every later plan."""
        w, g80 = self.w, self.net._geglu80
        if (8 * inner) % 160 or inner % 64:
            return
        d.geglu_unit = 80
        ok = ops.gemm_check(d) and ops.gemm_query(d)[1] == 160
        if not ok:
            d.geglu_unit = 0
            return
        for k in ("ff1.w", "ff1.b", "ff1.s", "ff1.cb"):
            if (t + k) in w and (t + k) not in g80:
                src = w[t + k]
                if k == "ff1.w":
                    src = ops.pack_gemm_weight(ops.geglu_repack(ops.unpack_gemm_weight(src, 8 * inner, inner), 64, 80))
                else:
                    src = ops.geglu_repack(src, 64, 80)
                g80[t + k] = src
        d.w = g80[t + "ff1.w"].data_ptr()
        d._w_tensor = g80[t + "ff1.w"]
        if d.ln_stats:
            d.bias, d.ln_s = g80[t + "ff1.cb"].data_ptr(), g80[t + "ff1.s"].data_ptr()
        else:
            d.bias = g80[t + "ff1.b"].data_ptr()

    def ff_proj_weights(self, pre, t, ch, inner, n):
        """[Wc | W_p] packed as one [ch, 5 inner] dense weight and bc = b_p + W_p b_f2 (ops.compose_ff_proj) for the last block `t`
        of the SpatialTransformer `pre`, or None below the gate (ops option unet_ff_proj_fuse = smallest inner, 0 = never; M >= 128).
        Made once per weight on first need and kept for every later plan; the originals stay for the plans below the gate."""
        w, fp = self.w, self.net._ff_proj
        thr = ops.get_option("unet_ff_proj_fuse")
        if not thr or inner < thr or inner % 64 or self.B * n < 128:
            return None
        if t not in fp:
            w_p = ops.unpack_gemm_weight(w[pre + "proj_out.w"], ch, inner)
            w_f2 = ops.unpack_gemm_weight(w[t + "ff2.w"], inner, 4 * inner)
            comp, bc = ops.compose_ff_proj(w_p, w[pre + "proj_out.b"], w_f2, w[t + "ff2.b"])
            fp[t] = (ops.pack_gemm_weight(comp), bc)
        return fp[t]

    def tail_rows(self, t, n, heads, dh):
        """Rows per block of the fused SpatialTransformer tail for this block, or 0 = unfused launches.  The fused launch
        needs enough row blocks to fill the chip: 32-row blocks from 192 blocks up (UNet batch 2 at a 64 x 64 latent = 256),
        64-row blocks (half the weight traffic through L2) once those alone give >= 2 blocks per CU.
        ops.set_option("unet_st_tail", 0 | 32 | 64) forces a choice (0 = never)."""
        TC = self.TC
        if (t + "tail.stream") not in self.w or self.net.transformer_depth != 1 or self.selfctx:
            return 0
        if TC > 1024 or TC % 8:     # mdx_st_tail_f16: capacity a multiple of 8, <= 1024 (96-key chunks with online softmax past 96)
            return 0
        forced = ops.get_option("unet_st_tail")
        cands = [forced] if forced in (32, 64) else ([] if forced == 0 else [64, 32])
        for r in cands:
            if not ops.st_tail_supported(heads * dh, heads, dh, n, r):
                continue
            blocks = self.B * n // r
            if forced in (32, 64) or (r == 64 and blocks >= 512) or (r == 32 and blocks >= 192):
                return r
        return 0

    def head_rows(self, t, x, n, heads, dh):
        """Rows per block of the fused SpatialTransformer head (GroupNorm .. q|k|v^T), or 0.  Only together with the fused
        tail, and only when x's producer is a GEMM / conv launch (its epilogue supplies the GroupNorm column partials)."""
        if not self.fuse_head or (t + "head.stream") not in self.w or ops.get_option("unet_st_head") == 0:
            return 0
        r = self.tail_rows(t, n, heads, dh)
        if not r or not ops.st_head_supported(heads * dh, n, r) or self.producer.get(x.data_ptr()) is None:
            return 0
        return r

    def context_kv(self, t, inner):
        """The cached K / V^T of the text context for block `t` (written by the context plan)."""
        kc = torch.zeros((self.B, self.TC, inner), dtype=f16, device=self.dev)
        vtc = torch.zeros((self.B, inner, self.TC), dtype=f16, device=self.dev)
        self.ctx_kv[t] = (kc, vtc)
        return kc, vtc

    def fused_tail(self, t, rows_t, o, tok, x, ch, inner, heads, dh, n):
        """Everything after the self-attention core of block `t` + proj_out + the residual: ONE row-local launch."""
        w, B, P, TC = self.w, self.B, self.P, self.TC
        kc, vtc = self.context_kv(t, inner)
        out = self.get((B, n, ch))
        td = ops.make_st_tail_desc(o, tok, x, out, kc, vtc, w[t + "tail.stream"], w[t + "tail.vec"], B, n, ch, heads,
                                   dh, 1, TC, tile_rows=rows_t)
        self.tails.append(td)
        td._bufs = (o, tok, x, out, kc, vtc)      # keeps the views alive; tools / tests read them
        self.producer[out.data_ptr()] = td

        def run_tail(td=td):
            td.ctx_len = P.ctx_len      # read at call time like the attention ops; a captured graph bakes it in
            ops.st_tail_run(td)
        self.emit(run_tail, "gemm", 2 * B * n * 16 * inner * inner + 4 * B * heads * n * self.ctx_flops * dh, 1,
                  f"st_tail M={B * n} C={inner} rows={rows_t} (to_out1..proj_out fused)")
        return out

    def stats_buf(self, rows, width):
        """{sum, sumsq} per 64-column slice of a token row: written by the GEMM that produces the rows, read by the
        GEMM that consumes LayerNorm(rows) (mdx_gemm_desc.stats_out / ln_stats).  One buffer per shape: the stream is
        in order and every consumer runs before the next producer."""
        if (rows, width) not in self.ln_stats:
            self.ln_stats[(rows, width)] = torch.zeros((rows, width // 64, 2), dtype=f32, device=self.dev)
        return self.ln_stats[(rows, width)]

    def vt_buffer(self, n, inner):
        """V^T [B, inner, row length] for attention.  Token counts that are not a multiple of 8 (5 x 5 ... 7 x 7 images at the
        deepest level of 320 / 384 / 448-pixel runs; the reference takes any multiple of 64 pixels) get rows padded to 8 in a
        DEDICATED zeroed buffer: the transposed store never writes the pad, the attention kernel's 16-byte V^T loads read it
        (times a zero probability), so it must stay finite -- an arena buffer would hand it another tensor's bytes."""
        if n % 8 == 0:
            return self.get((self.B, inner, n))
        t_ = torch.zeros((self.B, inner, round_up(n, 8)), dtype=f16, device=self.dev)
        self.ragged_vt.append(t_)
        return t_

    def vt_release(self, t_):
        if not any(t_ is r for r in self.ragged_vt):
            self.release(t_)

    def first_self_attention(self):
        """Is the op just emitted the first self-attention of the network, behind input block 1's ResBlock (only the first
        conv's output is held as a skip)?  That is where the guidance-duplicate prefix ends."""
        return "op" not in self.ck and "conv_in" in self.ck and len(self.hs) == 1

    def fused_transformer(self, t0, rows_h, x, ch, heads, dh, n):
        """Fused head + fused tail: GroupNorm .. q|k|v^T in one launch, the attention core, to_out1 .. proj_out in one."""
        w, B = self.w, self.B
        inner = heads * dh
        tok = self.get((B, n, inner))
        qk = self.get((B, n, 2 * inner))
        vt = self.get((B, inner, n))
        hd = ops.make_st_head_desc(x, x, 1, w[t0 + "head.stream"], w[t0 + "head.vec"], tok, qk, vt, n, B, n, ch,
                                   tile_rows=rows_h)
        hd.colstats = 0      # wired by finish() from x's producer (or the plan is rebuilt without it)
        self.heads_fused.append(hd)
        hd._bufs = (x, tok, qk, vt)
        self.gn_calls.append(dict(x1=x, x2=None, head=hd, meta=len(self.meta), film=False,
                                  prod=(self.producer.get(x.data_ptr()), None)))
        self.emit(lambda hd=hd: ops.st_head_run(hd), "gemm", 2 * B * n * 4 * inner * inner, 1,
                  f"st_head M={B * n} C={inner} rows={rows_h} (GroupNorm..q|k|v fused)")
        o = self.get((B, n, inner))
        self.attention(qk, vt, o, heads, dh, f"self B={B} h={heads} N={n} d={dh}", split_kv=True)
        if self.first_self_attention():
            self.ck.update(op=self.main[-1], live=(x, tok, o))
        out = self.fused_tail(t0, self.tail_rows(t0, n, heads, dh), o, tok, x, ch, inner, heads, dh, n)
        self.release(qk, vt, tok, o)
        return out

    def transformer(self, pre, x, ch, heads, dh, h, wd):
        """SpatialTransformer.construct attention.py:237-256 + `transformer_depth` BasicTransformerBlocks :181-185
        (NHWC == tokens)."""
        net, w, B, P, TC = self.net, self.w, self.B, self.P, self.TC
        dense, emit, selfctx = self.dense, self.emit, self.selfctx
        n = h * wd
        inner = heads * dh
        scale = dh ** -0.5
        t0 = pre + "transformer_blocks.0."
        rows_h = self.head_rows(t0, x, n, heads, dh)
        if rows_h:
            return self.fused_transformer(t0, rows_h, x, ch, heads, dh, n)
        a = self.get((B, n, ch))
        self.gn(x, None, w[pre + "norm.g"], w[pre + "norm.b"], 1e-6, False, a)
        # LayerNorm fold: `st` receives the row statistics from each producer of the token stream
        st = self.stats_buf(B * n, inner) if (t0 + "attn2.q.s") in w else None
        fold1 = st is not None and (t0 + "attn1.qkv.s") in w

        def consumer(name):   # kwargs of a GEMM that consumes LN(rows) with folded weights
            return dict(bias=w[name + ".cb"], ln_stats=st, ln_s=w[name + ".s"], ln_eps=1e-5)

        def layernorm(src, t, norm, ln):
            emit(lambda: ops.layernorm(src, w[t + norm + ".g"], w[t + norm + ".b"], 1e-5, out=ln), "layernorm")
        tok = dense(a, B, n, ch, inner, w[pre + "proj_in.w"], bias=w[pre + "proj_in.b"], stats_out=st if fold1 else None)
        # SpatialTransformer.norm has no activation (attention.py:243-247): proj_in can apply it to its A fragments from the
        # producer's column statistics (mdx_gemm_desc.gn_colstats on a dense launch).  Decided when the statistics are wired
        # (planner.wire_groupnorm_colstats): on success the GroupNorm op above is dropped and proj_in reads the raw x
        pf = ops.get_option("unet_gn_proj_fuse")
        if (self.fuse_head and pf and n >= pf and n % 64 == 0 and ch % 64 == 0 and ch <= 2560
                and self.producer.get(x.data_ptr()) is not None):
            self.gn_calls[-1]["proj"] = dict(desc=self.descs[-1], meta=len(self.meta) - 1)
        self.release(a)
        for k in range(net.transformer_depth):
            t = pre + f"transformer_blocks.{k}."
            last = k == net.transformer_depth - 1
            # --- attn1 (self)
            ln = self.get((B, n, inner))
            if not fold1:
                layernorm(tok, t, "norm1", ln)
            vt = self.vt_buffer(n, inner)
            nv = vt.shape[2]        # row length of V^T: n, or n rounded up to 8 (ragged_vt)
            if (t + "attn1.qkv.w") in w:
                qk = self.get((B, n, 2 * inner))
                self.gemm(a=tok if fold1 else ln, w=w[t + "attn1.qkv.w"], N=3 * inner, B=B, H=n, W=1, c1=inner, out=qk,
                          out_ld=2 * inner, out2=vt, out2_ld=nv, n_split=2 * inner,
                          **(consumer(t + "attn1.qkv") if fold1 else {}))
            else:
                qk = dense(ln, B, n, inner, 2 * inner, w[t + "attn1.qk.w"])
                dense(ln, B, n, inner, inner, w[t + "attn1.v.w"], out=vt, out_ld=nv, out_mode=ops.OUT_TRANSPOSED)
            o = ln  # reuse: ln is dead after the projections
            self.attention(qk, vt, o, heads, dh, f"self B={B} h={heads} N={n} d={dh}", split_kv=True)
            first = self.first_self_attention()
            rows_t = self.tail_rows(t, n, heads, dh)
            if first:       # splice point "behind the self-attention": every plan has it
                self.ck.update(op=self.main[-1], live=(x, tok, o))
            if rows_t:
                out = self.fused_tail(t, rows_t, o, tok, x, ch, inner, heads, dh, n)
                self.release(qk); self.vt_release(vt); self.release(tok, ln)
                return out
            tok2 = dense(o, B, n, inner, inner, w[t + "attn1.o.w"], bias=w[t + "attn1.o.b"], residual=tok, stats_out=st)
            if first:       # attn1's output projection (+ the row statistics attn2.q's LayerNorm fold reads) is still context-free:
                # a later splice point, used when BOTH plans of a guidance-duplicate pair have it (the fused tail starts at to_out)
                self.ck.update(op2=self.main[-1], live2=(x, tok2) + (() if st is None else (st,)))
            self.release(qk); self.vt_release(vt); self.release(tok)
            # --- attn2 (cross): K / V^T of the context are produced by the context plan
            # (round 6) head dim 64 (SDv2): the 77-key attention rides on the query projection as its EPILOGUE -- one 64-column
            # tile is one head (mdx_gemm_desc.xattn_k): no attention launch, no fp16 round trip of q; bit-identical to the two launches
            xfuse = (ops.get_option("unet_xattn_fuse") and not selfctx and dh == 64 and TC <= 1024 and TC % 8 == 0
                     and n % 64 == 0)
            xkw = {}
            if xfuse:
                kc, vtc = self.context_kv(t, inner)
                xkw = dict(tile_n=64, splitk=1, tile_m=0 if n % 128 == 0 else 64, xattn_k=kc, xattn_vt=vtc, xattn_len=TC,
                           xattn_cap=TC, xattn_scale=scale, out=o, out_ld=inner)
            if st is None:
                layernorm(tok2, t, "norm2", ln)
                q2 = dense(ln, B, n, inner, inner, w[t + "attn2.q.w"], **xkw)
            else:
                q2 = dense(tok2, B, n, inner, inner, w[t + "attn2.q.w"], **consumer(t + "attn2.q"), **xkw)
                if selfctx:    # k / v below read LayerNorm(tok2) itself: one explicit launch (this form is not a hot path)
                    layernorm(tok2, t, "norm2", ln)
            if xfuse:
                self.xattn_descs.append(self.descs[-1])      # (their xattn_len follows the context: _ensure_context)
                self.meta[-1]["flops"] += 4 * B * heads * n * self.ctx_flops * dh
                self.meta[-1]["info"] += f" +cross-attention h={heads} d={dh}"
                q2 = None
            if selfctx:
                # context = default(context, x) (attention.py:133): keys / values are projections of attn2's own input
                k2 = dense(ln, B, n, inner, inner, w[t + "attn2.k.w"])
                v2t = self.vt_buffer(n, inner)
                nv2 = v2t.shape[2]
                dense(ln, B, n, inner, inner, w[t + "attn2.v.w"], out=v2t, out_ld=nv2, out_mode=ops.OUT_TRANSPOSED)
                self.attn_ws_need = max(self.attn_ws_need, ops.attention_ws_bytes(B, heads, dh, n, n))
                emit(lambda q2=q2, k2=k2, v2t=v2t, o=o, nv2=nv2: ops.attention(
                    q2.data_ptr(), k2.data_ptr(), v2t.data_ptr(), o.data_ptr(), B, heads, dh, n, n, scale,
                    n * inner, inner, n * inner, inner, inner * nv2, nv2, n * inner, inner, ws=self.attn_ws),
                    "attention", 4 * B * heads * n * n * dh, 1, f"attn2-self B={B} h={heads} N={n} d={dh}")
                self.release(k2); self.vt_release(v2t)
            elif not xfuse:
                kc, vtc = self.context_kv(t, inner)
                emit(lambda q2=q2, kc=kc, vtc=vtc, o=o: ops.attention(
                    q2.data_ptr(), kc.data_ptr(), vtc.data_ptr(), o.data_ptr(), B, heads, dh, n, P.ctx_len, scale,
                    n * inner, inner, TC * inner, inner, inner * TC, TC, n * inner, inner),
                    "attention", 4 * B * heads * n * self.ctx_flops * dh, 1, f"cross B={B} h={heads} N={n} d={dh}")
            tok3 = dense(o, B, n, inner, inner, w[t + "attn2.o.w"], bias=w[t + "attn2.o.b"], residual=tok2, stats_out=st)
            if q2 is not None:
                self.release(q2)
            self.release(tok2)
            # --- feed-forward (GEGLU fused in the first GEMM's epilogue)
            if st is None:
                layernorm(tok3, t, "norm3", ln)
                g = dense(ln, B, n, inner, 8 * inner, w[t + "ff1.w"], bias=w[t + "ff1.b"], epilogue=ops.EPI_GEGLU)
            else:
                g = dense(tok3, B, n, inner, 8 * inner, w[t + "ff1.w"], epilogue=ops.EPI_GEGLU, **consumer(t + "ff1"))
            self.geglu_tile160(self.descs[-1], t, inner)
            fpw = self.ff_proj_weights(pre, t, ch, inner, n) if last else None
            if fpw is not None:
                # ff2 + proj_out of the last block as ONE launch over [g | tok3] (ops.compose_ff_proj): the producer of `out`,
                # as proj_out is, so the next GroupNorm still gets its column statistics from this epilogue
                out = dense(g, B, n, 5 * inner, ch, fpw[0], bias=fpw[1], src2=tok3, c2=inner, residual=x)
                self.meta[-1]["info"] += " (ff2 + proj_out fused)"
                self.release(g, tok3, ln)
                return out
            # the next block's norm1 reads its row statistics from this block's last producer
            tok = dense(g, B, n, 4 * inner, inner, w[t + "ff2.w"], bias=w[t + "ff2.b"], residual=tok3,
                        stats_out=st if (fold1 and not last) else None)
            self.release(g, tok3, ln)
        out = dense(tok, B, n, inner, ch, w[pre + "proj_out.w"], bias=w[pre + "proj_out.b"], residual=x)
        self.release(tok)
        return out

    # ------------------------------------------------------------------ passes of finish()
    def before_wiring(self):
        self.stream_small_convs()
        self.fuse_splitk_into_groupnorm()

    def stream_small_convs(self):
        """Weight-streaming form of the small-M 3x3 convs (mdx_gemm_desc.w_frag): at M = 128 (the 8 x 8 level at UNet batch
        2) a conv is a 30 MB weight stream with almost no arithmetic; the launches that resolve to 128 x 64 HALO tiles read a
        fragment-major copy of their weights straight into registers, twelve 1 KiB pieces in flight per wave.  Measured
        (round 3, op profile): M = 128 convs 20.3 -> 18.8 us, M = 512 convs 30.0 -> 31.0 us (each piece is fetched by the two
        waves that share its columns, which halves the unique bytes in flight): default threshold 128."""
        max_m = ops.get_option("unet_conv_stream")
        if not max_m:
            return
        frag_w = self.net._frag_w
        for d in self.descs:
            M = d.B * d.H * d.W      # (stride 1: output rows)
            if not (d.ksize == 3 and d.stride == 1 and not d.upsample and d.c2 == 0 and d.c1 % 64 == 0 and d.N % 64 == 0
                    and M <= max_m and d.out_mode == ops.OUT_ROWMAJOR and not d.skip_w and not d.gn_gamma):
                continue
            q = ops.gemm_query(d)
            w4 = ops.get_option("unet_conv_stream_w4")
            if w4 and q[3] == 1 and d.N % 128 == 0 and d.c1 // 64 >= 5 and not d.colstats_out and not d.defer_reduce:
                # side-by-side waves on 128-column tiles (every weight piece fetched once per block), slab split-K
                keep = (d.tile_m, d.tile_n, d.splitk)
                d.tile_m, d.tile_n, d.splitk = 128, 128, min(d.c1 // 64, w4)
                q = ops.gemm_query(d)
                if not (q[0] == 128 and q[1] == 128 and q[3] == 1 and q[2] > 4 and not q[6]):
                    d.tile_m, d.tile_n, d.splitk = keep
                    q = ops.gemm_query(d)
            if not (q[0] == 128 and q[1] in (64, 128) and q[3] == 1):
                continue
            if q[1] == 128 and not (q[2] > 1 and not q[6]):
                continue
            wkey = d._w_tensor.data_ptr()
            if wkey not in frag_w:    # (one fragment-major copy per weight, shared by the plans of every shape)
                frag_w[wkey] = ops.pack_frag_weight(ops.unpack_gemm_weight(d._w_tensor, d.N, 9 * d.c1)).reshape(-1)
            d.w, d.w_frag = frag_w[wkey].data_ptr(), 1

    def fuse_splitk_into_groupnorm(self):
        """The one-launch GroupNorm of the deep levels can also BE the split-K reduce of the conv right in front of it
        (mdx_gemm_desc.defer_reduce): -22 launches per evaluation at equal time (ops._OPTIONS["unet_gn_splitk_fuse"])."""
        fuse_hw = ops.get_option("unet_gn_splitk_fuse")     # for tensors of at most this many pixels per sample (0 = never)
        if not fuse_hw:
            return
        for c in self.gn_calls:
            if c.get("head") is not None or c.get("conv") is not None or c.get("proj") is not None:
                continue
            _, HW, C1 = c["x1"].shape
            if HW > fuse_hw:
                continue
            cpg = C1 // 32
            L = cpg // math.gcd(cpg, 8)
            d = c["prod"][0]
            if (c["x2"] is None and not c["film"] and L <= 64 and HW * L * 16 <= (64 << 10) and isinstance(d, ops.GemmDesc)
                    and d.N == C1
                    and d.out_ld == C1 and self.op_index.get(ctypes.addressof(d)) == c["meta"] - 1
                    and ops.gemm_query(d)[2] > 1 and ops.groupnorm_from_splitk_ok(d)
                    # (a two-source launch that reduces its split in the kernel keeps doing so: deferring the reduce would move it
                    # from the lean dense kernel to slabs on the generic one, which is what the ff2 + proj_out fusion must not pay)
                    and not (d.c2 and ops.gemm_query(d)[6])):
                d.defer_reduce = 1
                c["fs"] = d
                self.meta[c["meta"] - 1]["launches"] = 1

    def after_wiring(self):
        if any(not hd.colstats for hd in self.heads_fused) or any(not dd.gn_colstats for dd in self.gn_convs):
            raise _HeadNotWired()
        # ---- first-use tuning (off by default): a resolution / batch the tile table was not measured at runs the cost model's
        # tiles, 10-20 % off on some shapes; with the option on, every such launch form is timed once per shape (ops.tune_cache)
        if ops.get_option("unet_tune_first_use"):
            tws = ops.new_gemm_workspace(256 << 20, self.dev)
            self.patch_workspace(tws)
            self.P.tuned_shapes = ops.tune_untuned(self.descs)
            torch.cuda.synchronize()
            del tws
            ops.release_tune_scratch()
            self.patch_workspace(self.gemm_ws)
