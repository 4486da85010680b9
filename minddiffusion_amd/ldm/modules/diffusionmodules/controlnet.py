"""ControlNet (Zhang, Rao, Agrawala 2023, "Adding Conditional Control to Text-to-Image Diffusion Models") -- not in the
reference trees; the definition is cldm.py of the paper's repository (ControlNet.forward), restated:

    g     = input_hint_block(hint)                       eight 3x3 convs, SiLU between them, 8x down: image -> latent grid
    h     = input_blocks[0](x) + g
    r_i   = zero_convs[i](h)  after input block i        (1x1 convs)
    r_mid = middle_block_out(h)  after the middle block

The body is the UNet's own encoder half -- input_blocks and middle_block with their own weights, time_embed and emb_layers -- so
the class is a UNetModel whose structure has no output_blocks and no `out`, planned by a _UNetPlanner whose walk stops behind
the middle block.  The zero convs are dense launches into static fp16 NHWC buffers the plan owns; UNetModel.forward_nhwc(
control=) adds them into the UNet (ops.ControlAdd).  The hint does not change over a sampling run: `g` is cached per hint
tensor, so the hint block runs once per hint, not once per step.

Parameter names follow the UNet's conv naming: `input_hint_block.{0,2,..,14}.conv.weight|bias`, `zero_convs.{i}.0.conv.*`,
`middle_block_out.0.conv.*`.  They are UNPINNED: no reference tree has a ControlNet to pin them to.
"""
import weakref

import torch

from .... import ops
from ...._lib import MdxError
from ....planner import round_up
from .openaimodel import UNetModel, _UNetPlanner, f16, f32

# (output channels, stride) of the hint block's convs but the last, which maps 256 -> model_channels at stride 1
HINT_LAYERS = ((16, 1), (16, 1), (32, 2), (32, 1), (96, 2), (96, 1), (256, 2))
HINT_SCALE = 8          # image pixels per latent pixel: three stride-2 convs


class ControlNet(UNetModel):
    def __init__(self, hint_channels=3, **unet_config):
        if unet_config.get("enable_lora"):
            raise MdxError("ControlNet: enable_lora is not supported (LoRA adapters go on the UNet)")
        if unet_config.get("num_classes") is not None:
            raise MdxError("ControlNet: a class-conditional (num_classes) ControlNet is not supported")
        hint_channels = int(hint_channels)
        if not 1 <= hint_channels <= 8:
            raise MdxError(f"ControlNet: hint_channels must be in [1, 8], got {hint_channels}")
        super().__init__(**unet_config)
        self.hint_channels = hint_channels
        self.hint_pad = round_up(hint_channels, 8)      # zero weight columns, as conv_in pads 4 -> 8
        self.hint_runs = 0                              # evaluations of the hint block
        self._hint_key = self._hint_ref = None

    def _structure(self):
        inb, mid, _ = super()._structure()
        return inb, mid, []

    def hint_layers(self):
        """(cin, cout, stride) of the eight hint convs."""
        chans = [c for c, _ in HINT_LAYERS] + [self.model_channels]
        strides = [s for _, s in HINT_LAYERS] + [1]
        return list(zip([self.hint_channels] + chans[:-1], chans, strides))

    def block_channels(self):
        """Output channels of every input block: the widths of the zero convs."""
        out = []
        for blk in self.input_blocks:
            last = blk[-1]
            out.append(last[1] if last[0] in ("st", "down") else last[2])
        return out

    def _head_shapes(self, s):
        for k, (cin, cout, _) in enumerate(self.hint_layers()):
            s[f"input_hint_block.{2 * k}.conv.weight"] = (cout, cin, 3, 3)
            s[f"input_hint_block.{2 * k}.conv.bias"] = (cout,)
        chans = self.block_channels()
        for pre, ch in [(f"zero_convs.{i}.0.", ch) for i, ch in enumerate(chans)] + [("middle_block_out.0.", chans[-1])]:
            s[pre + "conv.weight"] = (ch, ch, 1, 1)
            s[pre + "conv.bias"] = (ch,)

    def _load_head(self, L):
        w = L.w
        for k in range(len(HINT_LAYERS) + 1):
            pre = f"input_hint_block.{2 * k}."
            w[pre + "w"] = L.conv(pre + "conv.weight", cin_pad=self.hint_pad if k == 0 else None)
            w[pre + "b"] = L.vec(pre + "conv.bias")
        chans = self.block_channels()
        for pre, ch in [(f"zero_convs.{i}.0.", ch) for i, ch in enumerate(chans)] + [("middle_block_out.0.", chans[-1])]:
            w[pre + "w"] = L.dense(L.raw(pre + "conv.weight", f16).reshape(ch, ch))      # 1x1 conv == Dense in NHWC
            w[pre + "b"] = L.vec(pre + "conv.bias")
        return ()

    def load_state_dict(self, params, strict=True):
        super().load_state_dict(params, strict=strict)
        self._hint_key = self._hint_ref = None
        return self

    def set_max_context_len(self, n):
        before = self._plans
        super().set_max_context_len(n)
        if self._plans is not before:       # the plans were dropped, and the cached hint features with them
            self._hint_key = self._hint_ref = None
        return self

    # ------------------------------------------------------------------ planning / execution
    def _planner(self, B, H, W, fuse_head, selfctx, control):
        if selfctx or control:
            raise MdxError("ControlNet: the network is evaluated with a text context, through forward_residuals()")
        return _ControlNetPlanner(self, B, H, W, fuse_head, False)

    def _ensure_hint(self, P, hint):
        """Run the hint block once per hint tensor: keyed by the tensor OBJECT and its version counter, as
        UNetModel._ensure_context keys the text context."""
        if not (isinstance(hint, torch.Tensor) and hint.is_cuda and hint.dim() == 4):
            raise MdxError("ControlNet: hint must be a CUDA(HIP) tensor [B, hint_channels, 8 H, 8 W] (no CPU fallback)")
        want = (P.B, self.hint_channels, HINT_SCALE * P.H, HINT_SCALE * P.W)
        if tuple(hint.shape) != want:
            raise MdxError(f"ControlNet: hint has shape {tuple(hint.shape)}, a {P.B} x {P.H} x {P.W} latent batch needs {want} "
                           f"(the hint is at image resolution, {HINT_SCALE} x the latent)")
        key = (hint.data_ptr(), hint._version, tuple(hint.shape), hint.dtype, id(P))
        alive = self._hint_ref() if self._hint_ref is not None else None
        if key == self._hint_key and alive is hint:
            return
        P.hint_static.copy_(hint)
        for op in P.hint_ops:
            op()
        self.hint_runs += 1
        self._hint_key, self._hint_ref = key, weakref.ref(hint)

    def hint_features(self, hint):
        """g = input_hint_block(hint): the plan's static NHWC fp16 buffer [B, H * W, model_channels], H x W the latent grid."""
        if not (isinstance(hint, torch.Tensor) and hint.dim() == 4):
            raise MdxError("ControlNet: hint must be a tensor [B, hint_channels, 8 H, 8 W]")
        B, _, Hh, Wh = (int(v) for v in hint.shape)
        if Hh % HINT_SCALE or Wh % HINT_SCALE:
            raise MdxError(f"ControlNet: the hint's size {Hh} x {Wh} is not {HINT_SCALE} x a latent grid")
        P = self._plan(B, Hh // HINT_SCALE, Wh // HINT_SCALE)
        self._ensure_hint(P, hint)
        return P.hint_g

    def forward_residuals(self, x, timesteps, context, hint, temb=None):
        """One ControlNet evaluation -> the plan's static residual buffers, fp16 NHWC [B, h * w, C]: one per input block, then the
        middle block's.  They are overwritten by the next call.  temb: row(s) of this network's time_embedding_table()."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4):
            raise MdxError("ControlNet: x must be a CUDA(HIP) tensor [B, C, H, W] (no CPU fallback)")
        if context is None:
            raise MdxError("ControlNet: a text context is required")
        B, C, H, W = (int(v) for v in x.shape)
        if C != self.in_channels:
            raise MdxError(f"ControlNet: expected {self.in_channels} input channels, got {C}")
        P = self._plan(B, H, W)
        self._ensure_context(P, context)
        self._ensure_hint(P, hint)
        self._evaluate(P, x, timesteps, temb)
        return P.residuals

    def forward_nhwc(self, *a, **kw):
        raise MdxError("ControlNet: the network has no output of its own; call forward_residuals() and hand the result to "
                       "UNetModel.forward_nhwc(control=)")

    def construct(self, *a, **kw):
        return self.forward_nhwc()

    __call__ = construct
    forward = construct


class _ControlNetPlanner(_UNetPlanner):
    """The UNet's plan up to the middle block, with the hint block in front (a side op list, run when the hint changes) and a
    zero conv behind every block."""

    def walk(self, xin):
        net, w, B, P = self.net, self.w, self.B, self.P
        h, wd = self.H, self.W
        P.hint_static = torch.zeros((B, net.hint_channels, HINT_SCALE * h, HINT_SCALE * wd), dtype=f32, device=self.dev)
        P.hint_g = torch.zeros((B, h * wd, net.model_channels), dtype=f16, device=self.dev)
        P.residuals = []
        self.hint_block()
        cur = None
        for i, blk in enumerate(net.input_blocks):
            for j, layer in enumerate(blk):
                pre = f"input_blocks.{i}.{j}."
                if layer[0] == "conv":      # h = conv_in(x) + g: the hint features ride as the launch's residual
                    cur, h, wd = self.conv3(xin, net.cin_pad, layer[2], w[pre + "w"], w[pre + "b"], h, wd, residual=P.hint_g)
                    self.release(xin)
                    continue
                new, h2, w2 = self.layer_op(pre, layer, cur, None, h, wd)
                self.release(cur)
                cur, h, wd = new, h2, w2
            self.zero_conv(f"zero_convs.{i}.0.", cur, h * wd)
        self.ck.setdefault("op", None)      # (the guidance-duplicate prefix is not used for this plan)
        for j, layer in enumerate(net.middle_block):
            new, h, wd = self.layer_op(f"middle_block.{j}.", layer, cur, None, h, wd)
            self.release(cur)
            cur = new
        self.zero_conv("middle_block_out.0.", cur, h * wd)
        self.release(cur)

    def first_self_attention(self):
        return False

    def zero_conv(self, pre, x, n):
        """r = zero_conv(h): a dense launch into a static buffer of the plan.  It stands between h's producer and the next
        GroupNorm, so that GroupNorm does not take over the producer's split-K reduce (fuse_splitk_into_groupnorm needs the
        producer's launch right in front of it) and this launch reads a finished h."""
        ch = int(x.shape[2])
        out = torch.zeros((self.B, n, ch), dtype=f16, device=self.dev)
        self.dense(x, self.B, n, ch, ch, self.w[pre + "w"], bias=self.w[pre + "b"], out=out, out_ld=ch)
        self.P.residuals.append(out)

    def hint_block(self):
        """input_hint_block at image resolution -> P.hint_g, as the side op list P.hint_ops (ControlNet._ensure_hint)."""
        net, w, B, P = self.net, self.w, self.B, self.P
        main, meta = [], []
        self.into = (main, meta)
        first = len(self.descs)
        hh, hw = HINT_SCALE * self.H, HINT_SCALE * self.W
        a = self.get((B, hh * hw, net.hint_pad))
        self.emit(lambda a=a: ops.nchw_to_nhwc(P.hint_static, net.hint_pad, out=a), "small")
        layers = net.hint_layers()
        cin = net.hint_pad
        for k, (_, cout, stride) in enumerate(layers):
            pre = f"input_hint_block.{2 * k}."
            if k == len(layers) - 1:
                self.gemm(a=a, w=w[pre + "w"], N=cout, B=B, H=hh, W=hw, c1=cin, out=P.hint_g, out_ld=cout, bias=w[pre + "b"],
                          ksize=3)
                self.release(a)
                break
            out, hh, hw = self.conv3(a, cin, cout, w[pre + "w"], w[pre + "b"], hh, hw, stride=stride)
            self.emit(lambda out=out: ops.silu_(out), "small")
            self.release(a)
            a, cin = out, cout
        assert (hh, hw) == (self.H, self.W)
        self.into = (self.main, self.meta)
        self.hint_descs = self.descs[first:]
        P.hint_ops = main

    def after_wiring(self):
        super().after_wiring()
        # the hint block's channel counts (16, 32, 96, 256) are multiples of 8 -- the documented contract of mdx_gemm_desc, which no
        # other model exercises at these sizes: every descriptor is validated on the host before the first launch relies on it
        for d in self.hint_descs:
            if not ops.gemm_check(d):
                raise MdxError(f"ControlNet: the hint conv c1={d.c1} N={d.N} stride={d.stride} at {d.H} x {d.W} is refused by "
                               f"mdx_gemm_check")
