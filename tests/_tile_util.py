"""Shared helpers of the tiled-VAE tests: the numpy float32 restatement of mdx_tile_blend_f32's arithmetic (include/mdx.h), its
float64 counterpart, and the tile grid and chunk rule of AutoencoderKL.enable_tiling restated, so that the references share
nothing with the product but the decoder / encoder calls between the slices and the blend."""
import numpy as np
import torch


def offsets(length, tile, stride, wrap=False):
    """0, s, 2s, ... while o + t < L, then a last tile at L - t; wrapped: 0, s, 2s, ... while o < L."""
    if wrap:
        return list(range(0, length, stride))
    return [o for o in range(0, length, stride) if o + tile < length] + [length - tile]


def ramp(n, r):
    """min(i + 1, n - i, r), i < n: integers."""
    i = np.arange(n)
    return np.minimum(np.minimum(i + 1, n - i), r)


def weights(th, tw, ry, rx):
    """[th, tw] float32, integer-valued: the min-ramp weight of every tile-local pixel."""
    return (ramp(th, ry)[:, None] * ramp(tw, rx)[None, :]).astype(np.float32)


def to_unit(v):
    """The float32 steps of torch.clamp((v + 1.0) / 2.0, 0.0, 1.0)."""
    u = ((v + np.float32(1.0)).astype(np.float32) / np.float32(2.0)).astype(np.float32)
    return np.minimum(np.maximum(u, np.float32(0.0)), np.float32(1.0))


def blend_ref(tiles, oy, ox, Hc, Wc, ry, rx, mode="raw"):
    """tiles: np.float32 [NB * N, C, TH, TW], row j * N + k, k = iy * nx + ix; a tile at ox covers columns (ox + i) mod Wc.
    Ascending k; first term acc = q * e, later terms acc = f32(acc + f32(q * e)); qsum likewise; one f32 divide; a pixel with
    one term takes the tile's bits.  Returns ([NB, C, Hc, Wc] float32, the count [Hc, Wc])."""
    assert tiles.dtype == np.float32
    org = [(a, b) for a in oy for b in ox]
    N, (C, TH, TW) = len(org), tiles.shape[1:]
    NB = tiles.shape[0] // N
    e = tiles.reshape(NB, N, C, TH, TW)
    q = weights(TH, TW, ry, rx)
    acc = np.zeros((NB, C, Hc, Wc), np.float32)
    one = np.zeros((NB, C, Hc, Wc), np.float32)
    qsum = np.zeros((Hc, Wc), np.float32)
    cnt = np.zeros((Hc, Wc), np.int64)
    for k, (a, b) in enumerate(org):
        rows, cols = np.arange(a, a + TH), (b + np.arange(TW)) % Wc
        ix = np.ix_(rows, cols)
        first = (cnt[ix] == 0)[None, None]
        term = (q[None, None] * e[:, k]).astype(np.float32)
        sub = (np.arange(NB)[:, None, None, None], np.arange(C)[None, :, None, None], rows[None, None, :, None],
               cols[None, None, None, :])
        acc[sub] = np.where(first, term, (acc[sub] + term).astype(np.float32))
        one[sub] = np.where(first, e[:, k], one[sub])
        qsum[ix] = np.where(cnt[ix] == 0, q, (qsum[ix] + q).astype(np.float32))
        cnt[ix] += 1
    assert cnt.min() >= 1
    out = np.where((cnt == 1)[None, None], one, (acc / qsum[None, None]).astype(np.float32))
    return (to_unit(out) if mode == "unit" else out), cnt


def blend_ref64(tiles, oy, ox, Hc, Wc, ry, rx):
    """The float64 min-ramp weighted mean of tiles [NB * N, C, TH, TW] (any float dtype) on the canvas: [NB, C, Hc, Wc]."""
    org = [(a, b) for a in oy for b in ox]
    N, (C, TH, TW) = len(org), tiles.shape[1:]
    NB = tiles.shape[0] // N
    e = np.asarray(tiles, np.float64).reshape(NB, N, C, TH, TW)
    q = weights(TH, TW, ry, rx).astype(np.float64)
    num, den = np.zeros((NB, C, Hc, Wc)), np.zeros((Hc, Wc))
    for k, (a, b) in enumerate(org):
        rows, cols = np.arange(a, a + TH), (b + np.arange(TW)) % Wc
        for i, r in enumerate(rows):                     # (fancy += does not accumulate repeated columns; none repeat here)
            num[:, :, r, cols] += q[i][None, None] * e[:, k, :, i]
            den[r, cols] += q[i]
    return num / den[None, None]


def gather_ref(canvas, oy, ox, th, tw):
    """torch indexing: ALL tiles of canvas [NB, C, Hc, Wc] as [NB * N, C, th, tw], row j * N + k, columns modulo Wc."""
    Wc = canvas.shape[-1]
    tiles = [canvas[:, :, a:a + th][..., (b + torch.arange(tw, device=canvas.device)) % Wc] for a in oy for b in ox]
    return torch.stack(tiles, 1).reshape(-1, canvas.shape[1], th, tw).contiguous()


def run_chunks(net, tiles, m):
    """The chunk rule: chunk c holds rows c m .. min((c + 1) m, T) - 1, the last chunk repeats its last row up to m rows; `net`
    always sees exactly m rows.  Returns the T outputs stacked (clones: net may reuse its output buffer)."""
    T = tiles.shape[0]
    outs = []
    for c0 in range(0, T, m):
        chunk = tiles[c0:c0 + m]
        n = chunk.shape[0]
        if n < m:
            chunk = torch.cat([chunk] + [chunk[-1:]] * (m - n))
        outs.append(net(chunk.contiguous())[:n].clone())
    return torch.cat(outs)
