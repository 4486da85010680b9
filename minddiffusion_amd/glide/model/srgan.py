"""SRGAN Generator on the MI355X kernels -- the 4x post-upscaler of Taichu-GLIDE's CLI (txt2img.py:107,129-130), after
vision/Taichu-GLIDE/model/glide_text2im/model/srgan.py:41-117:

    c1  = PReLU(Conv9x9(3 -> 64)(x))                                        mdx_srgan_conv_in_f16 (fp32 NCHW in, NHWC fp16 out)
    t   = c1; 16 x  t = BN2(Conv3x3(PReLU(BN1(Conv3x3(t))))) + t            mdx_gemm_f16, BN folded, MDX_EPI_PRELU / residual
    out = c1 + PReLU(Conv3x3(t))                                            mdx_gemm_f16, MDX_EPI_PRELU + residual (after the act.)
    log2(f) x  out = PReLU(DepthToSpace(2)(Conv3x3(64 -> 256)(out)))        mdx_gemm_f16, MDX_OUT_D2S2 + MDX_EPI_PRELU
    y   = tanh(Conv9x9(64 -> 3)(out))                                       mdx_srgan_conv_out_f32 (fp32 NCHW out)

BatchNorm runs in inference mode (moving statistics; the reference never calls set_train()) and is folded into the conv weight
and bias on the host in float64.  Execution model as the VAE (ldm/modules/diffusionmodules/model.py): a plan per (B, H, W) on
an arena, a flat C-ABI call list replayed as one hipGraph.  Activations are NHWC fp16; the 256^2 x 8 plan at f = 4 holds about
1.6 GB of them (the 1024^2 x 64-channel fp16 tensor alone is 1.07 GB, the 512^2 one 0.27 GB, the trunk's 256^2 ones 67 MB
each, the fp32 output 0.1 GB).
"""
import math

import numpy as np
import torch

from ..._lib import MdxError
from ... import ops
from ...ldm.modules.diffusionmodules.model import _run_plan
from ...loader import WeightLoader
from ...planner import PlanBuilder

f16, f32 = torch.float16, torch.float32

BN_EPS = 1e-5          # nn.BatchNorm2d default (srgan.py:45,48)
TRUNK = 16             # residual blocks (srgan.py:88-91)
CH = 64

# Channel order of ops.DepthToSpace(2) (srgan.py:63): MindSpore's TF-compatible DCR -- output [n, c, 2h+i, 2w+j] is conv output
# channel (2i+j) * C + c.  The GEMM's MDX_OUT_D2S2 store takes column n to sub-pixel q = n // C, channel n % C, so the packed
# weight rows are the conv's output channels in the order d2s_weight_rows() returns.  "CRD" (torch pixel_shuffle: c * 4 + q)
# is the one alternative; switch it here.
D2S_ORDER = "DCR"


def d2s_weight_rows(C, order=D2S_ORDER):
    """GEMM column n -> conv output channel whose weights it carries (a permutation of the conv's 4C output rows)."""
    n = np.arange(4 * C)
    q, c = n // C, n % C
    if order == "DCR":
        return q * C + c
    if order == "CRD":
        return c * 4 + q
    raise ValueError(order)


def fold_batchnorm(weight, bias, gamma, beta, mean, var, eps=BN_EPS):
    """BN(conv(x)) in inference mode as one conv: (w * s, (b - mean) * s + beta), s = gamma / sqrt(var + eps); float64."""
    w = np.asarray(weight, np.float64)
    s = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    wf = w * s[:, None, None, None]
    bf = (np.asarray(bias, np.float64) - np.asarray(mean, np.float64)) * s + np.asarray(beta, np.float64)
    return wf, bf


def prelu_keys(base, params):
    """nn.PReLU stores its slope in attribute `w` but names the Parameter `a`: accept either spelling."""
    for k in (base + ".a", base + ".w"):
        if k in params:
            return k
    raise MdxError(f"SRGAN Generator: missing PReLU slope {base}.a (or {base}.w)")


class Generator:
    def __init__(self, upscale_factor, device=None, use_graph=True):
        f = int(upscale_factor)
        if f not in (2, 4, 8):
            raise MdxError(f"SRGAN Generator: upscale_factor must be 2, 4 or 8 (got {upscale_factor})")
        self.upscale_factor = f
        self.n_sub = int(math.log(f, 2))                 # srgan.py:79-80
        self.device = torch.device(device if device is not None else "cuda")
        self.use_graph = bool(use_graph)
        self.w = None
        self._plans = {}

    # ------------------------------------------------------------------ structure
    def _prelu_bases(self):
        return (["conv1.1"] + [f"trunk.{i}.prelu" for i in range(TRUNK)] + ["conv2.1"]
                + [f"subpixel_conv.{j}.prelu" for j in range(self.n_sub)])

    def parameter_shapes(self, prelu="a"):
        """Reference parameter names -> shapes (PReLU slopes spelled `<cell>.a`, or `.w` with prelu='w')."""
        s = {"conv1.0.weight": (CH, 3, 9, 9), "conv1.0.bias": (CH,), f"conv1.1.{prelu}": (CH,)}
        for i in range(TRUNK):
            p = f"trunk.{i}."
            for c in ("conv1", "conv2"):
                s[p + c + ".weight"] = (CH, CH, 3, 3)
                s[p + c + ".bias"] = (CH,)
            for b in ("bn1", "bn2"):
                for n in ("gamma", "beta", "moving_mean", "moving_variance"):
                    s[p + b + "." + n] = (CH,)
            s[p + "prelu." + prelu] = (CH,)
        s["conv2.0.weight"] = (CH, CH, 3, 3); s["conv2.0.bias"] = (CH,); s[f"conv2.1.{prelu}"] = (CH,)
        for j in range(self.n_sub):
            p = f"subpixel_conv.{j}."
            s[p + "conv.weight"] = (4 * CH, CH, 3, 3); s[p + "conv.bias"] = (4 * CH,); s[p + "prelu." + prelu] = (CH,)
        s["conv3.weight"] = (3, CH, 9, 9); s["conv3.bias"] = (3,)
        return s

    def normalize_keys(self, params):
        """Map `<cell>.w` PReLU spellings to `<cell>.a` (the names parameter_shapes() uses)."""
        out = dict(params)
        for base in self._prelu_bases():
            if base + ".a" not in out and base + ".w" in out:
                out[base + ".a"] = out.pop(base + ".w")
        return out

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, params, strict=True):
        """params: reference parameter name -> array (PReLU slopes as `.a` or `.w`).  BN folded, weights packed once."""
        params = self.normalize_keys(params)
        shapes = self.parameter_shapes()
        for base in self._prelu_bases():
            prelu_keys(base, params)                     # a missing slope raises with both spellings named
        L = WeightLoader(params, self.device, "SRGAN Generator", error=MdxError, via_f32=True)
        L.check(shapes, unexpected=strict)
        w, g = L.w, L.src
        w["in.w"], w["in.b"], w["in.a"] = L.raw("conv1.0.weight", f16), L.vec("conv1.0.bias"), L.vec("conv1.1.a")
        for i in range(TRUNK):
            p = f"trunk.{i}."
            for c, b in (("conv1", "bn1"), ("conv2", "bn2")):
                wf, bf = fold_batchnorm(g(p + c + ".weight"), g(p + c + ".bias"), g(p + b + ".gamma"), g(p + b + ".beta"),
                                        g(p + b + ".moving_mean"), g(p + b + ".moving_variance"))
                w[p + c + ".w"], w[p + c + ".b"] = L.conv(wf), L.vec(bf)
            w[p + "a"] = L.vec(p + "prelu.a")
        w["c2.w"], w["c2.b"], w["c2.a"] = L.conv("conv2.0.weight"), L.vec("conv2.0.bias"), L.vec("conv2.1.a")
        rows = d2s_weight_rows(CH)
        for j in range(self.n_sub):
            p = f"subpixel_conv.{j}."
            w[p + "w"] = L.conv(np.asarray(g(p + "conv.weight"))[rows])
            w[p + "b"] = L.vec(np.asarray(g(p + "conv.bias"))[rows])
            w[p + "a"] = L.vec(p + "prelu.a")
        w["out.w"], w["out.b"] = L.raw("conv3.weight", f16), L.vec("conv3.bias")
        self.w = L.finish(shapes)
        self._plans.clear()

    # ------------------------------------------------------------------ plan
    class _Plan:
        graph = None
        graph_failed = False

    def _plan(self, B, H, W):
        key = (B, H, W)
        if key in self._plans:
            return self._plans[key]
        if self.w is None:
            raise MdxError("SRGAN Generator: load_state_dict() must be called first")
        dev, w = self.device, self.w
        P = Generator._Plan()
        pb = PlanBuilder(dev, B)
        P.x_static = torch.zeros((B, 3, H, W), dtype=f32, device=dev)
        c1 = pb.get((B, H, W, CH))
        pb.emit(lambda: ops.srgan_conv_in(P.x_static, w["in.w"], w["in.b"], w["in.a"], out=c1), "srgan_conv_in",
                2 * B * H * W * CH * 243, 1, f"9x9 3->64 {H}x{W}")

        def conv(src, wt, bias, out, n, h, wd, **kw):
            pb.gemm(a=src, w=wt, N=n, B=B, H=h, W=wd, c1=CH, out=out, out_ld=CH, bias=bias, ksize=3, **kw)

        t = c1
        for i in range(TRUNK):                           # ResidualBlock.construct, srgan.py:50-57
            p = f"trunk.{i}."
            u = pb.get((B, H, W, CH))
            conv(t, w[p + "conv1.w"], w[p + "conv1.b"], u, CH, H, W, epilogue=ops.EPI_PRELU, act_slope=w[p + "a"])
            t2 = pb.get((B, H, W, CH))
            conv(u, w[p + "conv2.w"], w[p + "conv2.b"], t2, CH, H, W, residual=t, residual_ld=CH)
            pb.release(u)
            if t is not c1:
                pb.release(t)
            t = t2
        s = pb.get((B, H, W, CH))                         # out = conv1 + PReLU(conv2(trunk)), srgan.py:108-113
        conv(t, w["c2.w"], w["c2.b"], s, CH, H, W, epilogue=ops.EPI_PRELU, act_slope=w["c2.a"], residual=c1, residual_ld=CH)
        pb.release(t)
        pb.release(c1)
        h, wd = H, W
        for j in range(self.n_sub):                      # SubpixelConvolutionLayer.construct, srgan.py:67-72
            p = f"subpixel_conv.{j}."
            o = pb.get((B, 2 * h, 2 * wd, CH))
            conv(s, w[p + "w"], w[p + "b"], o, 4 * CH, h, wd, epilogue=ops.EPI_PRELU, act_slope=w[p + "a"],
                 out_mode=ops.OUT_D2S2)
            pb.release(s)
            s, h, wd = o, 2 * h, 2 * wd
        P.out_nchw = torch.empty((B, 3, h, wd), dtype=f32, device=dev)
        pb.emit(lambda: ops.srgan_conv_out(s, w["out.w"], w["out.b"], B, h, wd, out=P.out_nchw), "srgan_conv_out",
                2 * B * h * wd * 3 * CH * 81, 1, f"9x9 64->3 {h}x{wd}")
        pb.finish(P)
        P.activation_bytes = pb.A.total
        P.out_hw = (h, wd)
        self._plans[key] = P
        return P

    # ------------------------------------------------------------------ run
    def construct(self, x):
        """x fp32 NCHW [B, 3, H, W] on the GPU (tanh range) -> fp32 NCHW [B, 3, f H, f W] (a buffer owned by the plan,
        overwritten by the next call with the same shape)."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise MdxError("SRGAN Generator: x must be a CUDA(HIP) tensor (no CPU fallback)")
        if x.dim() != 4 or x.shape[1] != 3:
            raise MdxError(f"SRGAN Generator: expected [B, 3, H, W], got {tuple(x.shape)}")
        B, _, H, W = x.shape
        P = self._plan(int(B), int(H), int(W))
        P.x_static.copy_(x)
        _run_plan(self, P)
        return P.out_nchw

    __call__ = construct
