"""Host-side helpers for prompts longer than one CLIP window.

A prompt of more than 75 tokens is cut into 75-token chunks; every chunk becomes its own 77-token window (bos, the chunk,
eos, padding), the windows are encoded independently (TextEncoder.construct takes [B, n, 77]) and their encodings are
concatenated to one [B, n * 77, D] cross-attention context.  Classifier-free guidance concatenates the conditional and the
unconditional context into one batch, so both must have the same number of windows: pad_conditioning extends the shorter
one with encodings of the empty window.
"""
import numpy as np
import torch

from ...._lib import MdxError

WINDOW = 77     # CLIP context length: bos + 75 tokens + eos


def chunk_token_ids(ids, bos, eos, pad=None, body=75):
    """ids: a batch of ragged sequences of UN-delimited token ids (no bos / eos) -> int32 array [B, n, body + 2].
    Every window is `bos`, up to `body` ids, `eos`, then padding (`pad`; None pads with `eos`, CLIP's convention).  n is the
    batch maximum of ceil(len / body); shorter prompts get whole empty windows, an empty prompt is one empty window."""
    body = int(body)
    if body < 1:
        raise MdxError(f"chunk_token_ids: body must be positive (got {body})")
    seqs = [[int(t) for t in np.asarray(s).reshape(-1)] for s in ids]
    if not seqs:
        raise MdxError("chunk_token_ids: empty batch")
    n = max(1, max(-(-len(s) // body) for s in seqs))
    fill = int(eos if pad is None else pad)
    out = np.full((len(seqs), n, body + 2), fill, dtype=np.int32)
    for b, s in enumerate(seqs):
        for k in range(n):
            part = s[k * body:(k + 1) * body]
            out[b, k, 0] = bos
            out[b, k, 1:1 + len(part)] = part
            out[b, k, 1 + len(part)] = eos
    return out


def pad_conditioning(c, uc, empty):
    """Bring a conditional and an unconditional context [B, n * 77, D] to the same length: the shorter one is extended with
    copies of `empty`, the [1, 77, D] encoding of the empty window (bos, eos, padding).  Lengths that are no multiple of 77
    are an error: there is no telling which windows such a tensor holds.  Returns (c, uc); equal lengths come back as they are."""
    for name, x in (("c", c), ("uc", uc)):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] == 0 or x.shape[1] % WINDOW:
            raise MdxError(f"pad_conditioning: {name} must be a tensor [B, n * {WINDOW}, D] "
                           f"(got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__})")
    if c.shape[1] == uc.shape[1]:
        return c, uc
    if not isinstance(empty, torch.Tensor) or empty.dim() != 3 or empty.shape[0] != 1 or empty.shape[1] != WINDOW:
        raise MdxError(f"pad_conditioning: empty must be the [1, {WINDOW}, D] encoding of the empty window")
    if not (c.shape[2] == uc.shape[2] == empty.shape[2]):
        raise MdxError(f"pad_conditioning: widths differ ({c.shape[2]}, {uc.shape[2]}, {empty.shape[2]})")
    T = max(c.shape[1], uc.shape[1])

    def extend(x):
        if x.shape[1] == T:
            return x
        e = empty.to(device=x.device, dtype=x.dtype).expand(x.shape[0], WINDOW, x.shape[2])
        return torch.cat([x] + [e] * ((T - x.shape[1]) // WINDOW), dim=1)
    return extend(c), extend(uc)
