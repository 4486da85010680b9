"""Sentinel-guarded outputs and NaN-poisoned inputs for the footprint tests (tests/test_footprint_gpu.py,
tests/test_norm_regimes_gpu.py).

guarded() puts an output -- contiguous or strided -- in the middle of ONE flat allocation filled with a sentinel that is exact in the
dtype and not NaN; assert_footprint() then asserts, bit for bit, that every element of the allocation OUTSIDE the logical output still
holds the sentinel: the pads in front and behind, and the gaps inside a strided output (columns N .. out_ld - 1, rows outside a token
sub-range, channels C .. out_ld - 1 of a depth-to-space pixel).  The payload starts as sentinel too, so an element the launch leaves
out fails the parity check (and assert_footprint(..., written=True)).

poisoned() is the mirror image for inputs: the logical operand sits inside a NaN-filled allocation, pads and stride gaps NaN, so a
result that depends on anything outside the operand is not finite.  Memory a kernel's header says must be finite (`zero_shape`) is
zero-filled the way the product fills it, NaN only beyond it.

Pad size is derived, not measured: a tail error of a tiled kernel writes inside its own tile, the largest tile of the library is
256 rows x 192 columns, so a pad is 2 x 256 x (row stride in elements), never less than 4096 elements.  The row stride is the stride
of the second-to-last dimension (the leading dimension of a row-major / transposed matrix, the pixel stride of an NHWC image).
LIMIT: a store farther from the output than one pad is not seen; neither is one that lands inside the payload of the same output.
"""
import numpy as np
import torch

SENT = -1234.0          # exact in fp16 and fp32, not NaN
MIN_PAD = 4096          # elements
MAX_TILE_ROWS = 256     # the largest tile of the library: 256 rows x 192 columns
_INT = {torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def _device(device):
    if device is not None:
        return device
    return "cuda:0" if torch.cuda.is_available() else "cpu"


def _contiguous(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= int(s)
    return tuple(reversed(st))


def _layout(shape, strides, pad):
    shape = tuple(int(s) for s in shape)
    strides = _contiguous(shape) if strides is None else tuple(int(s) for s in strides)
    assert len(shape) == len(strides) and all(s > 0 for s in shape) and all(s >= 0 for s in strides)
    span = 1 + sum((s - 1) * st for s, st in zip(shape, strides))
    row = strides[-2] if len(shape) >= 2 else 1
    if pad is None:
        pad = max(MIN_PAD, 2 * MAX_TILE_ROWS * row)
    pad = (int(pad) + 63) // 64 * 64      # keeps the payload 128-byte aligned inside the allocation
    return shape, strides, span, pad


def guarded(shape, dtype=torch.float16, strides=None, pad=None, device=None):
    """(buf, view): `view` (shape, strides in elements) in the middle of the flat sentinel-filled allocation `buf`."""
    shape, strides, span, pad = _layout(shape, strides, pad)
    buf = torch.full((pad + span + pad,), SENT, dtype=dtype, device=_device(device))
    return buf, buf.as_strided(shape, strides, pad)


def payload_mask(buf, view):
    """Boolean mask over `buf`: True where an element belongs to `view` (a view of buf's storage)."""
    assert view.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr(), "the view is not a view of this buffer"
    off = view.storage_offset() - buf.storage_offset()
    idx = torch.arange(buf.numel(), device=buf.device).as_strided(tuple(view.shape), tuple(view.stride()), off)
    mask = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    mask[idx.reshape(-1)] = True
    return mask


def _bits(t):
    return t.view(_INT[t.dtype])


def assert_footprint(buf, written_mask_or_view, name, written=False):
    """Synchronises, then asserts bit equality with the sentinel for every element of `buf` outside the logical output (a view of
    buf, a list of views, or a boolean mask over buf).  written=True also asserts that no payload element still holds the sentinel."""
    if buf.is_cuda:
        torch.cuda.synchronize()
    w = written_mask_or_view
    if isinstance(w, (list, tuple)):
        mask = payload_mask(buf, w[0])
        for v in w[1:]:
            mask |= payload_mask(buf, v)
    elif w.dtype == torch.bool:
        assert w.shape == buf.shape
        mask = w
    else:
        mask = payload_mask(buf, w)
    sent = _bits(torch.full((1,), SENT, dtype=buf.dtype, device=buf.device))
    intact = _bits(buf) == sent
    stray = (~intact & ~mask).nonzero().reshape(-1)
    if stray.numel() and not bool(mask.any()):
        raise AssertionError(f"{name}: {int(stray.numel())} elements of a buffer the launch must not touch were written")
    if stray.numel():
        inside = mask.nonzero().reshape(-1)
        first, last = int(inside[0]), int(inside[-1])
        s0, s1 = int(stray[0]), int(stray[-1])
        where = []
        if s0 < first:
            where.append(f"wrote in front of its output (first at {s0 - first} elements)")
        if s1 > last:
            where.append(f"wrote behind its output (last at +{s1 - last} elements)")
        gaps = int(((stray > first) & (stray < last)).sum())
        if gaps:
            g = int(stray[(stray > first) & (stray < last)][0]) - first
            where.append(f"wrote into a stride gap of its output ({gaps} elements, first at offset {g} of the payload span)")
        raise AssertionError(f"{name}: {'; '.join(where)}; {int(stray.numel())} stray elements")
    if written:
        left = int((intact & mask).sum())
        assert left == 0, f"{name}: {left} elements of the output were not written"


def poisoned(array, shape=None, strides=None, dtype=None, zero_shape=None, pad=None, device=None):
    """(buf, view): the values of `array` (numpy or torch, reshaped to `shape`) at `strides` inside a NaN-filled flat allocation: pads
    and stride gaps are NaN.  zero_shape: an extent >= shape (same strides, same origin) that is zero-filled before the values go in
    -- memory the kernel's header requires to be finite, filled as the product fills it."""
    t = torch.from_numpy(np.ascontiguousarray(array)) if isinstance(array, np.ndarray) else array
    dtype = dtype or t.dtype
    shape = tuple(t.shape) if shape is None else tuple(shape)
    outer = shape if zero_shape is None else tuple(zero_shape)
    assert len(outer) == len(shape) and all(o >= s for o, s in zip(outer, shape))
    _, strides, span, pad = _layout(outer, strides, pad)
    dev = _device(device)
    buf = torch.full((pad + span + pad,), float("nan"), dtype=dtype, device=dev)
    if zero_shape is not None:
        buf.as_strided(outer, strides, pad).zero_()
    view = buf.as_strided(shape, strides, pad)
    view.copy_(t.reshape(shape).to(dev, dtype))
    return buf, view
