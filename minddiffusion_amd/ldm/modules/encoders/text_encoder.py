"""TextEncoder on the MI355X kernels -- mirror of the reference's ldm/modules/encoders/text_encoder.py
(TextEncoder :114-153, Transformer :100-111, ResidualAttentionBlock :81-97, MultiheadAttention :25-66; the Wukong copy
differs only in its real QuickGELU, WK text_encoder.py:67-74).  SURVEY.md 8(f) item 2: the step right before the
denoising loop -- it turns token ids into the [B, 77, width] conditioning that the UNet's cross-attention reads.

Planned executor like UNetModel: token + positional embedding (one gather kernel), then per layer
    LayerNorm -> in_proj as two GEMMs (q|k row-major, v stored transposed) -> causal flash attention -> out_proj (+x)
    LayerNorm -> c_fc with the GELU fused in the epilogue -> c_proj (+x)
and the final LayerNorm; 8 launches per layer, captured as one hipGraph.  The reference's [T, B, C] transposes
(:148-150) are layout only and disappear (token-major [B, T, C] throughout).  The sequence is padded from 77 to 80 tokens
(the transposed V store wants a multiple of 8): under the causal mask the 3 trailing pad positions cannot influence the
77 real ones, and they are dropped from the result.
"""
import numpy as np
import torch

from ...._lib import MdxError
from .... import ops
from ....loader import WeightLoader
from ....planner import PlanBuilder, capture_or_eager

f16, f32 = torch.float16, torch.float32


class TextEncoder:
    def __init__(self, context_length, vocab_size, output_dim, width, layers, heads, dtype=None, act="gelu_tanh",
                 device=None, use_graph=True, ln_eps=1e-5):
        if width % heads or (width // heads) not in (40, 64, 80, 160):
            raise MdxError(f"TextEncoder: head dim {width / heads} is not supported by mdx_attention_f16 (40/64/80/160)")
        if act not in ("gelu_tanh", "quick_gelu"):
            raise ValueError("act must be 'gelu_tanh' (SDv2: nn.GELU) or 'quick_gelu' (Wukong: x * sigmoid(1.702 x))")
        self.context_length, self.vocab_size, self.output_dim = context_length, vocab_size, output_dim
        self.width, self.layers, self.heads, self.act = width, layers, heads, act
        self.t_pad = (context_length + 7) // 8 * 8
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device()
                                                                                   if torch.cuda.is_available() else 0)
        self.use_graph = use_graph
        # ln_1 / ln_2 epsilon: SDv2 passes epsilon=1e-5 (text_encoder.py:84,93); Wukong builds nn.LayerNorm([d_model]) with
        # MindSpore's default 1e-7 (WK text_encoder.py:91,100).  ln_final is the default 1e-7 in both.
        self.ln_eps = float(ln_eps)
        self.w = None
        self._plans = {}

    def parameter_shapes(self, prefix=""):
        w = self.width
        s = {prefix + "embedding_table": (self.vocab_size, w), prefix + "positional_embedding": (self.context_length, w),
             prefix + "ln_final.gamma": (w,), prefix + "ln_final.beta": (w,)}
        for i in range(self.layers):
            b = f"{prefix}transformer_layer.resblocks.{i}."
            s[b + "attn.attn.in_proj.weight"] = (3 * w, w); s[b + "attn.attn.in_proj.bias"] = (3 * w,)
            s[b + "attn.attn.out_proj.weight"] = (w, w); s[b + "attn.attn.out_proj.bias"] = (w,)
            s[b + "ln_1.gamma"] = (w,); s[b + "ln_1.beta"] = (w,)
            s[b + "c_fc.weight"] = (4 * w, w); s[b + "c_fc.bias"] = (4 * w,)
            s[b + "c_proj.weight"] = (w, 4 * w); s[b + "c_proj.bias"] = (w,)
            s[b + "ln_2.gamma"] = (w,); s[b + "ln_2.beta"] = (w,)
        return s

    def load_state_dict(self, params, prefix="", strict=True):
        shapes = self.parameter_shapes(prefix)
        L = WeightLoader(params, self.device, "TextEncoder.load_state_dict", prefix=prefix)
        L.check(shapes, unexpected=strict)
        wd = self.width
        w = L.w
        w["emb"] = L.raw("embedding_table", f16)
        pos = torch.zeros((self.t_pad, wd), dtype=f16, device=self.device)      # pad rows: zeros (never read back)
        pos[: self.context_length] = L.raw("positional_embedding", f16)
        w["pos"] = pos
        L.norm("lnf", "ln_final")
        for i in range(self.layers):
            b, o = f"transformer_layer.resblocks.{i}.", f"l{i}."
            ipw, ipb = L.raw(b + "attn.attn.in_proj.weight", f16), L.vec(b + "attn.attn.in_proj.bias")
            w[o + "qk.w"], w[o + "qk.b"] = L.dense(ipw[: 2 * wd]), ipb[: 2 * wd].contiguous()
            w[o + "v.w"], w[o + "v.b"] = L.dense(ipw[2 * wd:]), ipb[2 * wd:].contiguous()
            w[o + "out.w"], w[o + "out.b"] = L.dense(b + "attn.attn.out_proj.weight"), L.vec(b + "attn.attn.out_proj.bias")
            w[o + "fc.w"], w[o + "fc.b"] = L.dense(b + "c_fc.weight"), L.vec(b + "c_fc.bias")
            w[o + "proj.w"], w[o + "proj.b"] = L.dense(b + "c_proj.weight"), L.vec(b + "c_proj.bias")
            for n in ("ln_1", "ln_2"):
                L.norm(o + n, b + n)
        self.w = L.finish(shapes)
        self._plans.clear()

    class _Plan:
        graph = None
        graph_failed = False

    def _plan(self, B):
        if B in self._plans:
            return self._plans[B]
        if self.w is None:
            raise MdxError("TextEncoder: load_state_dict() must be called before the first forward")
        dev, w, wd, T, H = self.device, self.w, self.width, self.t_pad, self.heads
        dh = wd // H
        P = TextEncoder._Plan()
        pb = PlanBuilder(dev, B)
        P.tokens = torch.zeros((B, T), dtype=torch.int32, device=dev)
        P.ones = torch.ones((B, T), dtype=torch.int32, device=dev)
        epi = ops.EPI_GELU if self.act == "gelu_tanh" else ops.EPI_QUICKGELU

        def layernorm(src, g, b, eps, out):
            pb.emit(lambda: ops.layernorm(src.view(B * T, wd), g, b, eps, out=out.view(B * T, wd)), "layernorm")

        x = pb.get((B, T, wd))
        # gather(embedding_table, ids) + positional_embedding (:144-147); mask all ones, so `pad` is never read
        pb.emit(lambda: ops.glide_text_embed(P.tokens, P.ones, w["emb"], w["pos"], w["pos"], out=x), "small")
        a = pb.get((B, T, wd))
        qk = pb.get((B, T, 2 * wd))
        vt = pb.get((B, wd, T))
        o = pb.get((B, T, wd))
        h = pb.get((B, T, 4 * wd))
        x2 = pb.get((B, T, wd))
        for i in range(self.layers):
            L = f"l{i}."
            layernorm(x, w[L + "ln_1.g"], w[L + "ln_1.b"], self.ln_eps, a)
            pb.dense(a, B, T, wd, 2 * wd, w[L + "qk.w"], bias=w[L + "qk.b"], out=qk, out_ld=2 * wd)
            pb.dense(a, B, T, wd, wd, w[L + "v.w"], bias=w[L + "v.b"], out=vt, out_ld=T, out_mode=ops.OUT_TRANSPOSED)
            pb.attention(qk, vt, o, H, dh, causal=True)                                         # mask :136-139, :57-60
            pb.dense(o, B, T, wd, wd, w[L + "out.w"], bias=w[L + "out.b"], residual=x, out=x2, out_ld=wd)   # x + attn(ln_1(x)) :94
            layernorm(x2, w[L + "ln_2.g"], w[L + "ln_2.b"], self.ln_eps, a)
            pb.dense(a, B, T, wd, 4 * wd, w[L + "fc.w"], bias=w[L + "fc.b"], epilogue=epi, out=h, out_ld=4 * wd)
            pb.dense(h, B, T, 4 * wd, wd, w[L + "proj.w"], bias=w[L + "proj.b"], residual=x2, out=x, out_ld=wd)   # x + mlp(ln_2(x)) :95
        P.out = torch.empty((B, T, wd), dtype=f16, device=dev)
        # ln_final = nn.LayerNorm([width]): MindSpore's default epsilon is 1e-7 (:132)
        layernorm(x, w["lnf.g"], w["lnf.b"], 1e-7, P.out)
        pb.finish(P)
        self._plans[B] = P
        return P

    def construct(self, text):
        """text_encoder.py:141-153.  text: int token ids [B, context_length] (any integer tensor / array) ->
        [B, context_length, width] fp16 on the GPU.  A long prompt cut into n windows (encoders.chunk_token_ids) comes as
        [B, n, context_length]: the B * n windows are encoded in ONE pass, each on its own (causal attention never crosses a
        window), and returned side by side as [B, n * context_length, width]."""
        tok = torch.as_tensor(np.asarray(text) if not isinstance(text, torch.Tensor) else text)
        if tok.dim() == 3 and tok.shape[2] == self.context_length and tok.shape[1] > 0:
            b, n = tok.shape[0], tok.shape[1]
            return self.construct(tok.reshape(b * n, self.context_length)).view(b, n * self.context_length, self.width)
        if tok.dim() != 2 or tok.shape[1] != self.context_length:
            raise MdxError(f"TextEncoder: expected token ids [B, {self.context_length}] or [B, n, {self.context_length}], "
                           f"got {tuple(tok.shape)}")
        if not torch.cuda.is_available() or self.device.type != "cuda":
            raise MdxError("TextEncoder: the HIP device is required (no CPU fallback)")
        B = tok.shape[0]
        P = self._plan(B)
        P.tokens[:, : self.context_length].copy_(tok.to(device=self.device, dtype=torch.int32))
        if self.use_graph and not P.graph_failed:
            if P.graph is None:
                graphs = capture_or_eager([P.main])
                P.graph, P.graph_failed = (None, True) if graphs is None else (graphs[0], False)
            if P.graph is not None:
                P.graph.replay()
                return P.out[:, : self.context_length].clone()   # a fresh tensor: callers keep c and uc side by side
        for op in P.main:
            op()
        return P.out[:, : self.context_length].clone()

    __call__ = construct
