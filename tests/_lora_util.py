"""Shared helpers of the LoRA tests: synthetic adapters, the merged fp32 parameters the oracle runs on, fp16 ulp distances."""
import numpy as np
import torch

RANK, ALPHA = 4, 4


def make_adapter(lora_shapes, seed):
    """A ~ N(0, 1/K), B ~ N(0, 0.25): with W ~ N(0, 1/K) this makes |s B A| ~ |W| at rank 4, alpha 4, so the adapter visibly
    changes the output (a zero-initialised B, as a fresh LoRADense has, would test nothing)."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shape in lora_shapes.items():
        if name.endswith("lora_a"):
            out[name] = (rng.standard_normal(shape) / np.sqrt(shape[1])).astype(np.float32)
        else:
            out[name] = (0.5 * rng.standard_normal(shape)).astype(np.float32)
    return out


def merged_params(params, adapter, scale):
    """The reference of the merged model: fp32 parameters W + scale * (B @ A), computed in float64."""
    out = dict(params)
    for name, a in adapter.items():
        if not name.endswith("lora_a"):
            continue
        dense, tail = name.rsplit(".", 1)
        b = adapter[dense + "." + tail[:-1] + "b"]
        w = params[dense + ".weight"].astype(np.float64) + scale * (b.astype(np.float64) @ a.astype(np.float64))
        out[dense + ".weight"] = w.astype(np.float32)
    return out


def ulp_distance(a, b):
    """Element-wise distance of two fp16 tensors in units of the last place (0 for +0 / -0)."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


def one_ulp_condition(got, ref, max_ulp=1, what=""):
    """The merge condition: elements that differ from the float64 reference are at most `max_ulp` fp16 ulp away and are at most
    2e-3 of all.  (The fp32 arithmetic the kernel is defined by differs from float64 in 1.8e-4 .. 3.1e-4 of the elements on
    these distributions, never by more than 1 ulp: the cap is a condition with that head-room, not a measurement.)"""
    d = ulp_distance(got, ref)
    share = float((d != 0).float().mean())
    worst = int(d.max())
    print(f"LORA {what}: differing share {share:.3e}, max ulp {worst}")
    assert worst <= max_ulp, f"{what}: an element is {worst} ulp from the reference"
    assert share <= 2e-3, f"{what}: {share:.3e} of the elements differ"
    return share
