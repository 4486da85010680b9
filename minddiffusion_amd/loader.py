"""The weight loader every model's ``load_state_dict`` is written on (the counterpart of planner.PlanBuilder for the other half
of a model class): key / shape checking, host -> device conversion, the plain packings, and a record of which checkpoint names
were read, so that ``parameter_shapes()`` and the load cannot drift apart.  Host-only: plain torch, nothing is launched.

    L = WeightLoader(params, self.device, "Model.load_state_dict")
    L.check(shapes, unexpected=strict)
    w = L.w
    w["conv.w"], w["conv.b"] = L.conv("conv.weight"), L.vec("conv.bias")
    L.norm("n1", "norm1")                       # norm1.gamma / norm1.beta -> w["n1.g"], w["n1.b"]
    custom = ops.pack_something(L.raw("qkv.weight", f16))
    L.finish(shapes)
"""
import numpy as np
import torch

from . import ops
from .weights import check_state_dict

f16, f32 = torch.float16, torch.float32


def named_layers(net):
    """(reference name prefix, layer) of every layer of a UNet's input_blocks / middle_block / output_blocks, in order."""
    for i, blk in enumerate(net.input_blocks):
        for j, layer in enumerate(blk):
            yield f"input_blocks.{i}.{j}.", layer
    for j, layer in enumerate(net.middle_block):
        yield f"middle_block.{j}.", layer
    for i, blk in enumerate(net.output_blocks):
        for j, layer in enumerate(blk):
            yield f"output_blocks.{i}.{j}.", layer


class LoaderMismatch(Exception):
    """parameter_shapes() and load_state_dict() of a class disagree about the names the class owns."""


class WeightLoader:
    def __init__(self, params, device, who, error=None, prefix="", via_f32=False):
        """`error`: the exception class of key / shape errors (None: KeyError / ValueError).  `prefix`: put in front of every key.
        `via_f32`: the SRGAN conversion -- on the host, float64 -> float32 (-> float16), then to the device; otherwise
        ``t.to(device, dtype)`` directly.  The two round a float64 input to float16 differently, and both are kept."""
        self.params, self.device, self.who, self.error = params, torch.device(device), who, error
        self.prefix, self.via_f32 = prefix, via_f32
        self.w = {}             # what the model keeps: kernel-side name -> packed tensor
        self.used = set()       # checkpoint names read so far (with the prefix)

    def check(self, shapes, unexpected=True):
        """Every name of `shapes` is needed to run: a missing key or a wrong shape always raises.  Keys outside `shapes` raise
        when `unexpected` is set (the caller's strict; never where the dict is shared with a sibling object)."""
        seen = self.params if unexpected else {k: v for k, v in self.params.items() if k in shapes}
        check_state_dict(shapes, seen, True, self.who, error=self.error)

    def src(self, key):
        """The caller's own array / tensor under `key`, recorded as read."""
        self.used.add(self.prefix + key)
        return self.params[self.prefix + key]

    def _to(self, a, dtype):
        if self.via_f32:
            t = torch.as_tensor(np.asarray(a, np.float64), dtype=f32)
            return (t if dtype == f32 else t.to(dtype)).to(self.device).contiguous()
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=self.device, dtype=dtype).contiguous()

    def raw(self, x, dtype):
        """Key (or an array / tensor computed from some) -> contiguous tensor of `dtype` on the device."""
        return self._to(self.src(x) if isinstance(x, str) else x, dtype)

    def own(self, key, dtype):
        """raw(), but never the caller's own tensor: what the model keeps must not change when the caller reuses its buffer
        for the next checkpoint."""
        a = self.src(key)
        t = self._to(a, dtype)
        return t.clone() if t is a else t

    def vec(self, x, pad=None):
        """fp32 vector, zero-padded to `pad` entries."""
        v = self.raw(x, f32)
        if pad is None or v.numel() == pad:
            return v
        out = torch.zeros(pad, dtype=f32, device=self.device)
        out[: v.numel()] = v
        return out

    def conv(self, x, cin_pad=None, cout_pad=None):
        """[Cout, Cin, kh, kw] -> the packed GEMM weight storage (ops.pack_conv_weight, include/mdx.h)."""
        return ops.pack_conv_weight(self.raw(x, f32), cin_pad, cout_pad)

    def dense(self, x):
        """nn.Dense weight [out, in] -> the packed GEMM weight storage."""
        return ops.pack_gemm_weight(self.raw(x, f16))

    def norm(self, dst, key):
        """The affine pair `key`.gamma / .beta -> w[dst + ".g"], w[dst + ".b"] (fp32)."""
        self.w[dst + ".g"], self.w[dst + ".b"] = self.vec(key + ".gamma"), self.vec(key + ".beta")

    def finish(self, shapes, unused=()):
        """End of a load: every name of `shapes` (except `unused`, names the class owns but does not run) was read, and every
        name read is in `shapes`.  Returns w."""
        never = [k for k in shapes if k not in self.used and k not in unused]
        unknown = sorted(k for k in self.used if k not in shapes)
        if never or unknown:
            raise LoaderMismatch(f"{self.who}: parameter_shapes() names {never[:3]} ({len(never)}) that the load never reads; "
                                 f"the load reads {unknown[:3]} ({len(unknown)}) that parameter_shapes() does not name")
        return self.w
