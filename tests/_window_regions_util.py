"""Shared helpers of the region / wrap-around tests of the windowed evaluation, restated independently of the product: the wrap
grid rule, the active-pair list, a numpy restatement of the uniform wrapped average (the arithmetic include/mdx.h states for
mdx_window_average_regions_f16 without regions), a float64 reference of the region mean with the pieces of its error bound, a
float32 emulation of the kernel's arithmetic (to confirm the bound on the CPU), the gather as torch.roll plus slicing, and a
HostComposition for regions and wrap."""
import numpy as np
import torch

import _window_util as U


def wrap_offsets(length, stride):
    """The wrapped x offsets: 0, s, 2s, ... while o < L."""
    return list(range(0, length, stride))


def x_offsets(Wc, w, stride, wrap):
    """A canvas no wider than the window has nothing to wrap."""
    return wrap_offsets(Wc, stride) if wrap and Wc > w else U.offsets(Wc, w, min(stride, w))


def columns(o, w, Wc):
    """The canvas columns of a window at x offset o, in the window's order."""
    return (o + np.arange(w)) % Wc


def pair_list(masks, oy, ox, h, w):
    """[(k, r), ...] sorted by k then r: r is active in window k iff its mask is non-zero somewhere inside it (wrap included)."""
    Wc = masks.shape[2]
    out = []
    for k, (a, b) in enumerate(U.origins(oy, ox)):
        for r in range(masks.shape[0]):
            if masks[r, a:a + h][:, columns(b, w, Wc)].any():
                out.append((k, r))
    return out


def coverage(oy, ox, h, w, Hc, Wc):
    cnt = np.zeros((Hc, Wc), np.int64)
    for a, b in U.origins(oy, ox):
        cnt[np.ix_(np.arange(a, a + h), columns(b, w, Wc))] += 1
    return cnt


def average_wrap_ref(win, oy, ox, h, w, Hc, Wc, C):
    """win: np.float16 [NB * N, h * w, ld], row j * N + k, the windows wrapping modulo Wc.  Sequential np.float32 adds in
    ascending k, one np.float32 divide, astype(np.float16); a pixel under one window keeps that window's halves (x / 1 is
    exact); channels [C, ld) are 0.  Returns ([NB, Hc * Wc, ld] float16, the count [Hc, Wc])."""
    org = U.origins(oy, ox)
    N, ld = len(org), win.shape[2]
    NB = win.shape[0] // N
    e = win.reshape(NB, N, h, w, ld)
    acc = np.zeros((NB, Hc, Wc, ld), np.float32)
    cnt = np.zeros((Hc, Wc), np.int64)
    for k, (a, b) in enumerate(org):
        idx = np.ix_(np.arange(a, a + h), columns(b, w, Wc))
        first = (cnt[idx] == 0)[None, :, :, None]
        ek = e[:, k].astype(np.float32)
        sub = acc[:, idx[0], idx[1]]
        acc[:, idx[0], idx[1]] = np.where(first, ek, (sub + ek).astype(np.float32))
        cnt[idx] += 1
    assert cnt.min() >= 1
    with np.errstate(invalid="ignore"):
        out = (acc / cnt.astype(np.float32)[None, :, :, None]).astype(np.float16)
    out[..., C:] = 0
    return out.reshape(NB, Hc * Wc, ld), cnt


def region_terms(pairs, masks, wts, oy, ox, h, w):
    """Per pair p, in pair order: (rows, cols, q [h, w] float32) -- the canvas pixels of its window and
    q = M_r(pixel) * wt(pixel - origin) as the kernel forms it: m alone without weights, else ONE float32 multiply."""
    org = U.origins(oy, ox)
    Wc = masks.shape[2]
    out = []
    for k, r in pairs:
        a, b = org[k]
        rows, cols = np.arange(a, a + h), columns(b, w, Wc)
        m = masks[r][np.ix_(rows, cols)].astype(np.float32)
        out.append((rows, cols, m if wts is None else (m * wts.astype(np.float32)).astype(np.float32)))
    return out


def region_ref64(win, pairs, masks, wts, oy, ox, h, w, C):
    """The float64 region mean out(p) = sum q e / sum q over the pairs that cover p (not rounded), with what the error bound
    needs: returns (ref [NB, Hc, Wc, ld] float64, T [Hc, Wc] the count of terms with q > 0, sum |q e| / sum q [NB, Hc, Wc, ld])."""
    R, Hc, Wc = masks.shape
    P, ld = len(pairs), win.shape[2]
    NB = win.shape[0] // P
    e = win.reshape(NB, P, h, w, ld).astype(np.float64)
    num, mag = np.zeros((NB, Hc, Wc, ld)), np.zeros((NB, Hc, Wc, ld))
    den, T = np.zeros((Hc, Wc)), np.zeros((Hc, Wc), np.int64)
    for p, (rows, cols, q) in enumerate(region_terms(pairs, masks, wts, oy, ox, h, w)):
        idx = np.ix_(rows, cols)
        q64 = q.astype(np.float64)
        on = q64 > 0
        term = np.where(on[None, :, :, None], q64[None, :, :, None] * e[:, p], 0.0)     # a masked-out row may hold anything
        num[:, idx[0], idx[1]] += term
        mag[:, idx[0], idx[1]] += np.abs(term)
        den[idx] += q64
        T[idx] += on
    assert den.min() > 0
    ref, mag = num / den[None, :, :, None], mag / den[None, :, :, None]
    ref[..., C:] = 0
    mag[..., C:] = 0
    return ref, T, mag


def region_emul32(win, pairs, masks, wts, oy, ox, h, w, C):
    """The kernel's arithmetic in numpy float32: pairs in order (ascending k, then r); a term with m == 0 skipped; first term
    acc = q * e, later acc = fma(q, e, acc) (q * e is exact in float64: the sum is rounded to float64, then to float32),
    qsum by float32 adds; float16(acc / qsum); a pixel with one term keeps that term's halves.  [NB, Hc * Wc, ld] float16."""
    R, Hc, Wc = masks.shape
    P, ld = len(pairs), win.shape[2]
    NB = win.shape[0] // P
    e = win.reshape(NB, P, h, w, ld)
    acc = np.zeros((NB, Hc, Wc, ld), np.float32)
    one = np.zeros((NB, Hc, Wc, ld), np.float16)
    qsum, T = np.zeros((Hc, Wc), np.float32), np.zeros((Hc, Wc), np.int64)
    for p, (rows, cols, q) in enumerate(region_terms(pairs, masks, wts, oy, ox, h, w)):
        idx = np.ix_(rows, cols)
        on, first = q > 0, T[idx] == 0
        qb, eb = q[None, :, :, None], np.where(on[None, :, :, None], e[:, p], np.float16(0))
        prod = (qb * eb.astype(np.float32)).astype(np.float32)
        fma = (qb.astype(np.float64) * eb.astype(np.float64) + acc[:, idx[0], idx[1]].astype(np.float64)).astype(np.float32)
        new = np.where(first[None, :, :, None], prod, fma)
        acc[:, idx[0], idx[1]] = np.where(on[None, :, :, None], new, acc[:, idx[0], idx[1]])
        one[:, idx[0], idx[1]] = np.where((on & first)[None, :, :, None], e[:, p], one[:, idx[0], idx[1]])
        qsum[idx] = np.where(on, np.where(first, q, (qsum[idx] + q).astype(np.float32)), qsum[idx])
        T[idx] += on
    out = (acc / qsum[None, :, :, None]).astype(np.float16)
    out = np.where((T == 1)[None, :, :, None], one, out)
    out[..., C:] = 0
    return out.reshape(NB, Hc * Wc, ld)


def region_bound(got, ref64, T, mag):
    """ulp16 / 2 + (2 T + 3) 2^-24 sum |q e| / sum q, per element; ulp16: the fp16 spacing at max(|got|, |ref64|).  The second
    summand is the fp32 accumulation bound: one rounding per multiply, fma, add and divide."""
    big = np.maximum(np.abs(got.astype(np.float64)), np.abs(ref64))
    with np.errstate(divide="ignore"):
        ulp16 = 2.0 ** (np.maximum(np.floor(np.log2(big)), -14.0) - 10.0)      # (subnormals and 0: 2^-24)
    return ulp16 / 2 + (2 * T[None, :, :, None] + 3) * 2.0 ** -24 * mag


def gather_rows_ref(canvas, oy, ox, h, w, rows):
    """torch.roll plus slicing: the windows rows[i] of canvas [NB, C, Hc, Wc] as [NB * n, C, h, w], row j * n + i; a window that
    runs over the right edge continues at column 0."""
    org = U.origins(oy, ox)
    cut = [torch.roll(canvas, -org[k][1], 3)[:, :, org[k][0]:org[k][0] + h, :w] for k in rows]
    return torch.stack(cut, 1).reshape(-1, canvas.shape[1], h, w).contiguous()


class HostComposition:
    """Any LatentDiffusion, with apply_model_nhwc replaced by the host composition of a wrapped and / or region evaluation:
    torch.roll plus slicing for the window batches, the inner model on the same batch sizes (so the same launch plans), the
    contexts of a chunk by indexing, and the average by `average(win, self)` -- default: the numpy restatement without regions,
    and with regions `region_average`, which a GPU test sets (the kernel's arithmetic is tested on its own).

    masks (np [R, Hc, Wc]) / contexts (R tensors [NB, T, D], the model call's own row layout): regions; None: none."""

    def __init__(self, inner, window, stride, max_unet_batch=16, wrap_x=False, masks=None, contexts=None, region_average=None):
        self.inner, self.window, self.stride, self.cap, self.wrap = inner, window, stride, max_unet_batch, wrap_x
        self.masks, self.contexts, self.region_average = masks, contexts, region_average
        self.calls = 0

    def __getattr__(self, name):
        if name == "inner":
            raise AttributeError(name)
        return getattr(self.inner, name)

    def apply_model_nhwc(self, x, t, cond, temb=None, cfg_dup=False):
        NB, _, Hc, Wc = x.shape
        h, w = min(self.window[0], Hc), min(self.window[1], Wc)
        oy = U.offsets(Hc, h, min(self.stride[0], h))
        ox = x_offsets(Wc, w, min(self.stride[1], w), self.wrap)
        N = len(oy) * len(ox)
        self.pairs = [(k, None) for k in range(N)] if self.masks is None else pair_list(self.masks, oy, ox, h, w)
        P = len(self.pairs)
        self.chunks = U.chunks(P, NB, self.cap)
        outs = []
        for p0, n in self.chunks:
            kw = {}
            if temb is not None:
                kw["temb"] = temb.repeat_interleave(n, 0) if temb.dim() == 2 else temb
            part = self.pairs[p0:p0 + n]
            if self.masks is None:
                ctx = None if cond is None else cond.repeat_interleave(n, 0)
            else:
                assert cond.shape == self.contexts[0].shape
                ctx = torch.stack([self.contexts[r] for _, r in part], 1).reshape((NB * n,) + tuple(cond.shape[1:])).contiguous()
            e = self.inner.apply_model_nhwc(gather_rows_ref(x, oy, ox, h, w, [k for k, _ in part]), t.repeat_interleave(n, 0),
                                            ctx, cfg_dup=cfg_dup, **kw)
            outs.append(e.reshape(NB, n, h * w, -1).clone())
        win = torch.cat(outs, 1).reshape(NB * P, h * w, -1).contiguous()
        C = int(self.inner.unet.final_channels)
        self.calls += 1
        if self.masks is not None:
            return self.region_average(win, self, (Hc, Wc), (h, w))
        return torch.from_numpy(average_wrap_ref(win.cpu().numpy(), oy, ox, h, w, Hc, Wc, C)[0]).to(x.device)


# ---- the inputs of the kernel tests, shared by the GPU tests and the CPU confirmation of the error bound
# name: (canvas [NB, C, Hc, Wc], x stride, wrap); 8 x 8 windows, row stride 4.  seam4: the window at 16 straddles the seam, float4
# form; odd3: scalar form, Wc % s != 0; grid2d: two window rows, 9 channels; clamped: no wrap, so its edge columns lie under one
# window and a binary mask leaves them exactly one term
CANVASES = {"seam4": ((4, 4, 8, 20), 4, True), "odd3": ((4, 4, 8, 18), 3, True), "grid2d": ((2, 9, 12, 20), 4, True),
            "clamped": ((2, 4, 8, 20), 4, False)}
WIN = 8


def canvas_grid(name):
    """(shape, oy, ox, wrap) of a canvas of CANVASES."""
    shape, s, wrap = CANVASES[name]
    return shape, U.offsets(shape[2], WIN, 4), x_offsets(shape[3], WIN, s, wrap), wrap


def region_masks(kind, Hc, Wc):
    """R = 3 masks [3, Hc, Wc] float32.  stripes: binary vertical stripes 5 columns wide, which cut through the 8-wide windows;
    ramp: soft -- a ramp along x, its complement, and a half-height ramp along y -- with exact zeros at its ends."""
    y, x = np.meshgrid(np.arange(Hc), np.arange(Wc), indexing="ij")
    if kind == "stripes":
        m = np.stack([((x // 5) % 3 == r) for r in range(3)])
    else:
        a = x / (Wc - 1.0)
        m = np.stack([a, 1.0 - a, 0.5 * y / (Hc - 1.0)])
    return np.ascontiguousarray(m.astype(np.float32))


def pair_outputs(name, kind, ld=8):
    """(win np.float16 [NB * P, 64, ld] random, pairs, masks) of a canvas and a mask kind: every channel filled."""
    shape, oy, ox, _ = canvas_grid(name)
    masks = region_masks(kind, shape[2], shape[3])
    pairs = pair_list(masks, oy, ox, WIN, WIN)
    seed = sorted(CANVASES).index(name) * 2 + (kind == "ramp")
    win = np.random.RandomState(100 + seed).randn(shape[0] * len(pairs), WIN * WIN, ld).astype(np.float16)
    return win, pairs, masks
