"""Shared helpers of the windowed-evaluation tests: the numpy restatement of mdx_window_average_f16's arithmetic (include/mdx.h)
and a test-local model whose apply_model_nhwc is the HOST composition of a windowed evaluation -- torch slicing, the inner
model on the same window batches, the numpy average -- with no product code but the inner model between the slices and the
average: the grid rule and the chunk list are restated here too."""
import numpy as np
import torch


def offsets(length, window, stride):
    """The grid rule, restated here so that the reference shares nothing with the product: 0, s, 2s, ... while o + w < L, then a
    last window at L - w."""
    out = [o for o in range(0, length, stride) if o + window < length]
    return out + [length - window]


def chunks(n_windows, canvas_batch, max_unet_batch):
    """[(k0, n), ...]: the windows in order, at most max_unet_batch // canvas_batch per chunk (restated likewise)."""
    cap = max_unet_batch // canvas_batch
    return [(k0, min(cap, n_windows - k0)) for k0 in range(0, n_windows, cap)]


def origins(oy, ox):
    """(oy, ox) of window k = iy * nx + ix, in ascending k."""
    return [(a, b) for a in oy for b in ox]


def average_ref(win, oy, ox, h, w, Hc, Wc, C):
    """win: np.float16 [NB * N, h * w, ld], row j * N + k.  Uniform weights: sequential np.float32 adds in ascending k, one
    np.float32 divide, astype(np.float16); channels [C, ld) are 0.  Returns ([NB, Hc * Wc, ld] float16, the count [Hc, Wc])."""
    org = origins(oy, ox)
    N, ld = len(org), win.shape[2]
    NB = win.shape[0] // N
    e = win.reshape(NB, N, h, w, ld)
    acc = np.zeros((NB, Hc, Wc, ld), np.float32)
    cnt = np.zeros((Hc, Wc), np.int64)
    for k, (a, b) in enumerate(org):
        first = (cnt[a:a + h, b:b + w] == 0)[None, :, :, None]
        ek = e[:, k].astype(np.float32)
        acc[:, a:a + h, b:b + w] = np.where(first, ek, (acc[:, a:a + h, b:b + w] + ek).astype(np.float32))
        cnt[a:a + h, b:b + w] += 1
    assert cnt.min() >= 1
    with np.errstate(invalid="ignore"):
        out = (acc / cnt.astype(np.float32)[None, :, :, None]).astype(np.float16)
    out[..., C:] = 0
    return out.reshape(NB, Hc * Wc, ld), cnt


def weighted_ref64(win, wts, oy, ox, h, w, Hc, Wc, C):
    """The float64 weighted mean, rounded once to float16 ([NB, Hc * Wc, ld]) -- and the count."""
    org = origins(oy, ox)
    N, ld = len(org), win.shape[2]
    NB = win.shape[0] // N
    e = win.reshape(NB, N, h, w, ld).astype(np.float64)
    num = np.zeros((NB, Hc, Wc, ld), np.float64)
    den = np.zeros((Hc, Wc), np.float64)
    cnt = np.zeros((Hc, Wc), np.int64)
    w64 = wts.astype(np.float64)
    for k, (a, b) in enumerate(org):
        num[:, a:a + h, b:b + w] += w64[None, :, :, None] * e[:, k]
        den[a:a + h, b:b + w] += w64
        cnt[a:a + h, b:b + w] += 1
    out = (num / den[None, :, :, None]).astype(np.float16)
    out[..., C:] = 0
    return out.reshape(NB, Hc * Wc, ld), cnt


def gather_ref(canvas, oy, ox, h, w, k0, n):
    """torch slicing: windows k0 .. k0 + n - 1 of canvas [NB, C, Hc, Wc] as [NB * n, C, h, w], row j * n + kk."""
    org = origins(oy, ox)[k0:k0 + n]
    return torch.stack([canvas[:, :, a:a + h, b:b + w] for a, b in org], 1).reshape(-1, canvas.shape[1], h, w).contiguous()


class HostComposition:
    """Any LatentDiffusion, with apply_model_nhwc replaced by the host composition of the windowed evaluation of `wm` (a
    WindowedDiffusion on the same inner model): slice the window batches of the chunk list with torch, call the inner model on
    them (the same batch sizes, so the same launch plans), combine on the CPU with average_ref."""

    def __init__(self, inner, window, stride, max_unet_batch=16):
        self.inner, self.window, self.stride, self.cap = inner, window, stride, max_unet_batch
        self.calls = 0

    def __getattr__(self, name):
        if name == "inner":
            raise AttributeError(name)
        return getattr(self.inner, name)

    def apply_model_nhwc(self, x, t, cond, temb=None, cfg_dup=False):
        NB, _, Hc, Wc = x.shape
        h, w = min(self.window[0], Hc), min(self.window[1], Wc)
        oy = offsets(Hc, h, min(self.stride[0], h))
        ox = offsets(Wc, w, min(self.stride[1], w))
        outs = []
        self.chunks = chunks(len(oy) * len(ox), NB, self.cap)
        for k0, n in self.chunks:
            kw = {}
            if temb is not None:
                kw["temb"] = temb.repeat_interleave(n, 0) if temb.dim() == 2 else temb
            e = self.inner.apply_model_nhwc(gather_ref(x, oy, ox, h, w, k0, n), t.repeat_interleave(n, 0),
                                            None if cond is None else cond.repeat_interleave(n, 0), cfg_dup=cfg_dup, **kw)
            outs.append(e.cpu().numpy().reshape(NB, n, h * w, -1))
        win = np.concatenate(outs, 1).reshape(NB * len(oy) * len(ox), h * w, -1)
        C = int(self.inner.unet.final_channels)
        self.calls += 1
        return torch.from_numpy(average_ref(win, oy, ox, h, w, Hc, Wc, C)[0]).to(x.device)
