"""WindowedDiffusion -- overlapping-window evaluation of the UNet on a latent canvas larger than the resolution a checkpoint was
trained at (MultiDiffusion, Bar-Tal et al. 2023; not in the reference): a 512 x 2048 panorama, or 1024^2 from a 512 checkpoint.

Per model call the canvas is cut into overlapping windows of the trained size, the UNet runs on the windows as ONE batch (or a
few, `max_unet_batch`), and the outputs are averaged where windows overlap.  The samplers here are linear in the model output
and all windows see the same canvas, so averaging the outputs and stepping once equals averaging per-window steps.  The class
is a model wrapper: samplers, sessions and the pipeline reach the network through ``apply_model_nhwc`` alone, so PLMS / DDIM /
DPM-Solver, v-prediction, guidance rescale, per-request lists and seeds, img2img and the mask blend, hybrid inpainting (its
c_concat channels ride inside ``x`` and are windowed with it), LoRA and sampling sessions run on a large canvas unchanged.
Two HIP launches per call surround the UNet (csrc/window.hip): ops.window_gather and ops.window_average.

wrap_x: the windows wrap around the canvas' right edge into its left one (a 360-degree panorama: both edges lie inside one
window).  ``with wm.regions(masks, contexts):`` gives every region of the canvas its own text context (MultiDiffusion section
4.2 without bootstrapping): the UNet runs once per ACTIVE (window, region) pair and the outputs are averaged with the region
masks as weights.  Both go through ops.window_gather_rows and ops.window_average_regions, one launch each, and change
nothing in the UNet, the step kernels or the samplers.  Known cost: under guidance the unconditional half is evaluated once
per pair, so the R regions of one window repeat the same unconditional evaluation.
"""
import contextlib
import functools
import weakref

import numpy as np
import torch

from .... import distributed as D
from .... import ops
from ...._lib import MdxError
from ....ops import window_offsets  # noqa: F401  (the grid rule, public here too)


def gaussian_weights(h, w, sigma_frac=0.5):
    """[h, w] fp32 weights for feathered seams: the separable Gaussian exp(-d^2 / (2 sigma^2)) of the distance d to the window
    centre, sigma = sigma_frac * the window's extent per axis, computed in float64.  Every weight is > 0."""
    h, w, sigma_frac = int(h), int(w), float(sigma_frac)
    if h < 1 or w < 1 or not 0.0 < sigma_frac < float("inf"):
        raise ValueError(f"gaussian_weights: h, w >= 1 and a positive finite sigma_frac, got {h}, {w}, {sigma_frac!r}")

    def axis(n):
        d = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
        return np.exp(-0.5 * (d / (sigma_frac * n)) ** 2)
    return torch.from_numpy(np.outer(axis(h), axis(w)).astype(np.float32))


def _pair(v, name):
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        return int(v), int(v)
    try:
        a, b = v
        if any(isinstance(q, bool) or int(q) != q for q in (a, b)):
            raise TypeError
        return int(a), int(b)
    except (TypeError, ValueError):
        raise MdxError(f"WindowedDiffusion: {name} must be an int or an (H, W) pair of ints, got {v!r}") from None


def chunk_list(n_windows, canvas_batch, max_unet_batch):
    """[(k0, n), ...]: range(n_windows) in order, in chunks of at most max_unet_batch // canvas_batch windows."""
    cap = int(max_unet_batch) // int(canvas_batch)
    if cap < 1:
        raise MdxError(f"WindowedDiffusion: a canvas batch of {canvas_batch} does not fit max_unet_batch={max_unet_batch} "
                       f"(one window of every canvas row is the smallest UNet batch)")
    return [(k0, min(cap, n_windows - k0)) for k0 in range(0, n_windows, cap)]


class WindowedDiffusion:
    """A LatentDiffusion evaluated in overlapping windows.  window / stride: latent pixels, ints or (h, w) pairs; stride None:
    half the window.  weights: None (the plain mean) or [h, w] positive weights (gaussian_weights) for feathered seams.
    max_unet_batch (even): the largest UNet batch one chunk of windows may make.  wrap_x: windows wrap around the x axis (on a
    canvas wider than the window; a narrower or equal one has nothing to wrap).  Everything else -- the schedule arrays,
    parameterization, unet, model.conditioning_key, time_embedding_table, the first and cond stage models, the LoRA calls --
    is the inner model's."""

    def __init__(self, model, window=(64, 64), stride=None, weights=None, max_unet_batch=16, wrap_x=False):
        if isinstance(model, WindowedDiffusion):
            raise MdxError("WindowedDiffusion: the model is already windowed")
        if getattr(model, "is_controlled", False):
            raise MdxError("WindowedDiffusion: a ControlledDiffusion model is not windowed (the hint has no per-window form)")
        key = getattr(getattr(model, "model", None), "conditioning_key", "crossattn")
        unet = getattr(model, "unet", None)
        if key == "adm" or getattr(unet, "num_classes", None) is not None:
            raise MdxError("WindowedDiffusion: a class-conditional ('adm') model is not windowed (its labels have no "
                           "timestep-only table and no per-window form)")
        if D.world()[1] > 1:
            raise MdxError("WindowedDiffusion: runs on a single rank (the sharded form is not built)")
        h, w = _pair(window, "window")
        sh, sw = (max(h // 2, 1), max(w // 2, 1)) if stride is None else _pair(stride, "stride")
        if h < 1 or w < 1:
            raise MdxError(f"WindowedDiffusion: window must be positive, got {(h, w)}")
        if not (1 <= sh <= h and 1 <= sw <= w):
            raise MdxError(f"WindowedDiffusion: stride {(sh, sw)} must be in [1, window = {(h, w)}] per axis (a larger one "
                           f"leaves canvas pixels uncovered)")
        div = 1 << (len(getattr(unet, "channel_mult", (1,))) - 1)
        if h % div or w % div:
            raise MdxError(f"WindowedDiffusion: window {h}x{w} is not divisible by {div} (the UNet halves it "
                           f"{len(unet.channel_mult) - 1} times)")
        if isinstance(max_unet_batch, bool) or int(max_unet_batch) != max_unet_batch or max_unet_batch < 2 or max_unet_batch % 2:
            raise MdxError(f"WindowedDiffusion: max_unet_batch must be an even int >= 2, got {max_unet_batch!r}")
        if weights is not None:
            weights = torch.as_tensor(weights, dtype=torch.float32)
            if tuple(weights.shape) != (h, w):
                raise MdxError(f"WindowedDiffusion: weights have shape {tuple(weights.shape)}, the window is {(h, w)}")
            if not bool((weights > 0).all()) or not bool(torch.isfinite(weights).all()):
                raise MdxError("WindowedDiffusion: weights must be positive and finite (a pixel's weights are divided by their sum)")
            weights = weights.contiguous()
        self.inner = model
        self.window, self.stride = (h, w), (sh, sw)
        self.weights = weights
        self.max_unet_batch = int(max_unet_batch)
        self.wrap_x = bool(wrap_x)
        self.chunks = []            # [(p0, n), ...] of the last windowed call: ranges of its UNet rows (self.pairs)
        self.pairs = []             # [(k, r), ...] the UNet rows of the last windowed call, plain, wrapped or with regions: window
                                    # k for region r; without regions r is None and the rows are the windows, (k, None), k < N
        self.grid = None            # ops.WindowGrid of the last windowed call
        self.evals = 0              # windowed calls (a single-window call forwards and does not count)
        self.context_refreshes = 0  # in-place refreshes of a per-window context repeat
        self._grids, self._bufs, self._ctx = {}, {}, {}
        self._weights_dev = None
        self._regions = None        # inside `with regions(...)`: {"plan", "contexts", "rows"}
        self._rows, self._rctx = {}, {}

    def __getattr__(self, name):    # (only reached for what the wrapper does not define)
        if name == "inner":
            raise AttributeError(name)
        return getattr(self.inner, name)

    # ---- the grid of one canvas shape
    def grid_for(self, Hc, Wc):
        """The ops.WindowGrid of an Hc x Wc canvas: a window larger than the canvas on an axis becomes the canvas extent."""
        key = (int(Hc), int(Wc))
        if key not in self._grids:
            h, w = min(self.window[0], key[0]), min(self.window[1], key[1])
            self._grids[key] = ops.WindowGrid(key, (h, w), (min(self.stride[0], h), min(self.stride[1], w)),
                                              wrap_x=self.wrap_x and key[1] > w)
        return self._grids[key]

    # ---- regions: a mask over the canvas and a text context each
    @contextlib.contextmanager
    def regions(self, masks, contexts):
        """Inside the block every model call evaluates R regions: masks [R, Hc, Wc] (fp32, finite, >= 0, their sum > 0 at every
        pixel) for the canvas shape that will be called, contexts a list of R tensors in the model call's OWN row layout
        [NB, T, D] -- what the sampler hands over as `cond`; under guidance cat([uc, c_r]) -- so the wrapper never guesses
        which rows are unconditional.  A call whose cond differs from them in rows, T, D, dtype or device, or whose canvas
        has another shape, is an MdxError.  Outside the block the wrapper is what it is without it."""
        if self._regions is not None:
            raise MdxError("WindowedDiffusion.regions: already inside a regions block")
        masks = torch.as_tensor(masks)
        if masks.dim() != 3:
            raise MdxError(f"WindowedDiffusion.regions: masks have shape {tuple(masks.shape)}, expected [R, Hc, Wc]")
        contexts = list(contexts)
        if len(contexts) != int(masks.shape[0]) or not contexts:
            raise MdxError(f"WindowedDiffusion.regions: {len(contexts)} contexts for {int(masks.shape[0])} masks")
        first = contexts[0]
        for r, c in enumerate(contexts):
            if not (isinstance(c, torch.Tensor) and c.is_cuda and c.dim() == 3):
                raise MdxError(f"WindowedDiffusion.regions: context {r} must be a CUDA(HIP) tensor [NB, T, D]")
            if tuple(c.shape) != tuple(first.shape) or c.dtype != first.dtype or c.device != first.device:
                raise MdxError(f"WindowedDiffusion.regions: context {r} is {tuple(c.shape)} {c.dtype} on {c.device}, context 0 "
                               f"{tuple(first.shape)} {first.dtype} on {first.device} (bring them to one length with "
                               f"encoders.pad_conditioning)")
        Hc, Wc = int(masks.shape[1]), int(masks.shape[2])
        g = self.grid_for(Hc, Wc)
        if self.weights is not None and (g.h, g.w) != self.window:
            raise MdxError(f"WindowedDiffusion: the weights are for {self.window} windows, a {Hc}x{Wc} canvas clips them to "
                           f"{(g.h, g.w)}")
        self._regions = {"plan": ops.RegionPlan(g, masks), "contexts": contexts}
        try:
            yield self
        finally:
            self._regions = None

    def _in_bufs(self, x, n):
        """The UNet input batch and timestep rows of a chunk of n windows."""
        key = (tuple(x.shape), n, x.device)
        if key not in self._bufs:
            NB, C = int(x.shape[0]), int(x.shape[1])
            z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=x.device)
            self._bufs[key] = {"x": z(NB * n, C, self.grid.h, self.grid.w), "t": z(NB * n)}
        return self._bufs[key]

    def _out_buf(self, x, ld, rows=None):
        """The canvas result [NB, Hc * Wc, ld]; with rows, the staged outputs [NB * rows, h * w, ld] of all the UNet rows of a
        call (several chunks only)."""
        g, NB = self.grid, int(x.shape[0])
        key = (rows, NB, g.Hc, g.Wc, g.h, g.w, ld, x.device)
        if key not in self._bufs:
            shape = (NB, g.Hc * g.Wc, ld) if rows is None else (NB * rows, g.h * g.w, ld)
            self._bufs[key] = torch.zeros(shape, dtype=torch.float16, device=x.device)
        return self._bufs[key]

    def _context(self, cond, n):
        """The per-window repeat [NB * n, T, D] of the caller's context, row j * n + kk = cond[j]: a persistent buffer, refreshed
        in place only when the caller's tensor object or its version changes (the rule of UNetModel._ensure_context), so the
        UNet re-projects it only when the prompt changes and a session's in-place context writes stay visible."""
        if cond is None:
            return None
        key = (cond.data_ptr(), cond._version, tuple(cond.shape), cond.dtype, cond.device)
        ent = self._ctx.get(n)
        if ent is not None and ent["key"] == key and ent["ref"]() is cond:
            return ent["buf"]
        NB = int(cond.shape[0])
        shape = (NB * n,) + tuple(cond.shape[1:])
        if ent is None or tuple(ent["buf"].shape) != shape or ent["buf"].dtype != cond.dtype or ent["buf"].device != cond.device:
            ent = self._ctx[n] = {"buf": torch.empty(shape, dtype=cond.dtype, device=cond.device)}
        ent["buf"].view((NB, n) + tuple(cond.shape[1:])).copy_(cond[:, None].expand((NB, n) + tuple(cond.shape[1:])))
        ent["key"], ent["ref"] = key, weakref.ref(cond)
        self.context_refreshes += 1
        return ent["buf"]

    def _chunk_rows(self, g, plan, p0, n):
        """The ops.WindowRows of pairs p0 .. p0 + n - 1 (their window numbers), made once per plan and range."""
        owner = g if plan is None else plan
        key = (id(owner), p0, n)
        ent = self._rows.get(key)
        if ent is None or ent[0] is not owner:                              # (the owner is kept: ids are reused)
            windows = range(p0, p0 + n) if plan is None else plan.pair_window.host[p0:p0 + n]
            if len(self._rows) > 64:
                self._rows.clear()
            ent = self._rows[key] = (owner, ops.WindowRows(windows))
        return ent[1]

    def _region_context(self, cond, p0, n):
        """The context buffer [NB * n, T, D] of pairs p0 .. p0 + n - 1, row j * n + i = contexts[pair_region[p0 + i]][j]: one
        persistent buffer per chunk, refreshed in place only when one of the chunk's region tensors (the object or its version
        counter) changes -- the rule of _context, over all the regions of the chunk."""
        reg = self._regions
        ctxs, first = reg["contexts"], reg["contexts"][0]
        if not (isinstance(cond, torch.Tensor) and tuple(cond.shape) == tuple(first.shape) and cond.dtype == first.dtype
                and cond.device == first.device):
            what = (f"{tuple(cond.shape)} {cond.dtype} on {cond.device}" if isinstance(cond, torch.Tensor) else repr(cond))
            raise MdxError(f"WindowedDiffusion.regions: the call's cond is {what}, the region contexts are "
                           f"{tuple(first.shape)} {first.dtype} on {first.device} (rows, T, D, dtype and device must agree)")
        ids = tuple(int(r) for r in reg["plan"].pair_region.host[p0:p0 + n])
        used = sorted(set(ids))
        key = (ids,) + tuple((ctxs[r].data_ptr(), ctxs[r]._version) for r in used)
        ent = self._rctx.get((p0, n))
        if ent is not None and ent["key"] == key and all(ref() is ctxs[r] for ref, r in zip(ent["refs"], used)):
            return ent["buf"]
        NB = int(first.shape[0])
        shape = (NB * n,) + tuple(first.shape[1:])
        if ent is None or tuple(ent["buf"].shape) != shape or ent["buf"].dtype != first.dtype or ent["buf"].device != first.device:
            ent = self._rctx[(p0, n)] = {"buf": torch.empty(shape, dtype=first.dtype, device=first.device)}
        view = ent["buf"].view((NB, n) + tuple(first.shape[1:]))
        for i, r in enumerate(ids):
            view[:, i].copy_(ctxs[r])
        ent["key"], ent["refs"] = key, [weakref.ref(ctxs[r]) for r in used]
        self.context_refreshes += 1
        return ent["buf"]

    def _chunk_kw(self, buf, temb, NB, n, device):
        """The temb keyword of a chunk of n rows per canvas row: per-sample rows repeated, one row handed on as it is."""
        if temb is None:
            return {}
        if temb.dim() != 2:
            return {"temb": temb}             # one row: it broadcasts over any batch
        if "temb" not in buf or buf["temb"].shape[1] != temb.shape[1]:
            buf["temb"] = torch.empty((NB * n, temb.shape[1]), dtype=temb.dtype, device=device)
        buf["temb"].view(NB, n, -1).copy_(temb[:, None, :].expand(NB, n, temb.shape[1]))
        return {"temb": buf["temb"]}

    def _weights_on(self, device):
        if self.weights is None:
            return None
        if self._weights_dev is None or self._weights_dev.device != device:
            self._weights_dev = self.weights.to(device)
        return self._weights_dev

    # ---- the model call
    def apply_model_nhwc(self, x, t, cond, temb=None, cfg_dup=False):
        """LatentDiffusion.apply_model_nhwc on the canvas x [NB, C, Hc, Wc]: NHWC fp16 [NB, Hc * Wc, ld], a buffer of the
        wrapper's that stays valid until the next call.  A single window the size of the canvas forwards to the inner model:
        no launch is added and no bit changes."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4):
            raise MdxError("WindowedDiffusion: x must be a CUDA(HIP) tensor [NB, C, H, W] (no CPU fallback)")
        NB, C, Hc, Wc = (int(v) for v in x.shape)
        g = self.grid_for(Hc, Wc)
        if g.N == 1 and self._regions is None:
            return self.inner.apply_model_nhwc(x, t, cond, temb=temb, cfg_dup=cfg_dup)
        if self.weights is not None and (g.h, g.w) != self.window:
            raise MdxError(f"WindowedDiffusion: the weights are for {self.window} windows, a {Hc}x{Wc} canvas clips them to "
                           f"{(g.h, g.w)}")
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        t = torch.as_tensor(t, device=x.device).to(torch.float32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(NB)
        plan = None if self._regions is None else self._regions["plan"]
        if plan is not None and plan.grid is not g:
            raise MdxError(f"WindowedDiffusion.regions: the masks are for a {plan.grid.Hc}x{plan.grid.Wc} canvas, the call is on "
                           f"{g.Hc}x{g.Wc}")
        # The UNet rows are pairs -- (window, region), or without regions the windows -- cut into chunks of at most
        # max_unet_batch // NB rows (row order j * n + i keeps the [uncond ; cond] halves identical inputs).  The one choice of
        # the launches: a range of windows of a clamped grid, or a table of window numbers, region masks and wrap-around.
        if plan is None and not g.wrap_x:
            gather = lambda p0, n, out: ops.window_gather(x, g, p0, n, out=out)
            average = ops.window_average
        else:
            gather = lambda p0, n, out: ops.window_gather_rows(x, g, self._chunk_rows(g, plan, p0, n), out=out)
            average = functools.partial(ops.window_average_regions, plan=plan)
        P = g.N if plan is None else plan.P
        self.grid = g
        self.pairs = [(k, None) for k in range(g.N)] if plan is None else list(plan.pairs)
        self.chunks = chunk_list(P, NB, self.max_unet_batch)
        stage = None
        for p0, n in self.chunks:
            buf = self._in_bufs(x, n)
            gather(p0, n, buf["x"])
            buf["t"].view(NB, n).copy_(t.reshape(NB, 1).expand(NB, n))
            ctx = self._context(cond, n) if plan is None else self._region_context(cond, p0, n)
            e = self.inner.apply_model_nhwc(buf["x"], buf["t"], ctx, cfg_dup=cfg_dup,
                                            **self._chunk_kw(buf, temb, NB, n, x.device))
            ld = int(e.shape[2])
            if len(self.chunks) == 1:
                stage = e                     # one chunk: its rows are in staging order already, averaged from where they lie
            else:                             # the UNet's static output is overwritten by the next chunk
                stage = self._out_buf(x, ld, rows=P)
                stage.view(NB, P, g.h * g.w, ld)[:, p0:p0 + n].copy_(e.view(NB, n, g.h * g.w, ld))
        out = self._out_buf(x, ld)
        average(stage, g, self._out_channels(), out=out, weights=self._weights_on(x.device))
        self.evals += 1
        return out

    def _out_channels(self):
        return int(getattr(self.inner.unet, "final_channels", self.inner.channels))

    def apply_model(self, x_noisy, t, cond=None, return_ids=False, c_concat=None, c_crossattn=None):
        """The NCHW form (LatentDiffusion.apply_model): the same pass, then ops.nhwc_to_nchw."""
        c_concat, c_crossattn = self.inner._split_cond(cond, c_concat, c_crossattn)
        x = x_noisy.to(torch.float32)
        if c_concat is not None:
            x = torch.cat([x, c_concat.to(device=x.device, dtype=x.dtype)], 1)
        out = self.apply_model_nhwc(x.contiguous(), t, c_crossattn)
        return ops.nhwc_to_nchw(out, self._out_channels(), int(x.shape[2]), int(x.shape[3]))
