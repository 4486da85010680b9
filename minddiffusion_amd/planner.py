"""Host side of the planned executors: every model turns its structure into a flat list of C-ABI calls on pre-allocated,
liveness-reused buffers ONCE per input shape, through the one PlanBuilder below (UNet, GLIDE, VAE, SRGAN, text encoders).

    Arena             plan-time buffer reuse
    PlanBuilder       emit / gemm / gn / dense / conv3 / attention while a model walks its layers, then finish(P): size the shared
                      split-K workspace, wire GroupNorm statistics to their producers, size again, drop dead ops, check, account
    capture_or_eager  warm up, synchronise, capture as hipGraph(s); None (and a warning) when the runtime refuses

Nothing here launches a kernel; the emitted closures do, through ops.py.
"""
import ctypes
import math
import os
import warnings

import numpy as np
import torch

from . import _lib, ops
from .ops import FoldedColStats

f16, f32 = torch.float16, torch.float32


def round_up(x, m):
    return (x + m - 1) // m * m


class Arena:
    """Liveness-based buffer reuse at PLAN time (exact-size buckets).  Execution never allocates."""

    def __init__(self, device):
        self.device = device
        self.free = {}
        self.bases = []   # every allocation, kept alive for the plan's lifetime: GEMM descriptors hold raw pointers
        self.total = 0

    def get(self, shape, dtype=f16):
        n = int(np.prod(shape))
        nbytes = round_up(n * torch.empty((), dtype=dtype).element_size(), 256)
        lst = self.free.get(nbytes)
        if lst:
            base = lst.pop()
        else:
            base = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.bases.append(base)
            self.total += nbytes
        t = base[: n * torch.empty((), dtype=dtype).element_size()].view(dtype).view(*shape)
        t._mdx_base = base
        return t

    def release(self, t):
        base = t._mdx_base
        self.free.setdefault(base.numel(), []).append(base)


def _one_launch_groupnorm(HW, C):
    """Does a GroupNorm of C channels over HW pixels per sample take the one-launch fused kernel (norm.hip groupnorm_impl)?"""
    cpg = C // 32
    L = cpg // math.gcd(cpg, 8)           # chunk columns of the minimal whole-group column block
    return L <= 64 and HW * L * 16 <= (64 << 10)


class PlanBuilder:
    """Collects the op list (`main`), its profiling records (`meta`, parallel to `main`) and the GEMM descriptors of one plan.

    track_producers: remember which GEMM launch wrote each tensor last (planning order == run order), so that finish() can
    hand a GroupNorm its statistics from the producers' epilogues (mdx_gemm_desc.colstats_out).  An untracked builder never
    sets colstats_out: its GroupNorms stay on plain ops.groupnorm."""

    def __init__(self, device, batch, track_producers=False):
        self.dev, self.B = device, batch
        self.A = Arena(device)
        self.main, self.meta, self.descs = [], [], []
        self.into = (self.main, self.meta)      # where emit() appends (GLIDE routes its late text ops elsewhere)
        self.tag = {}                           # extra fields of every meta record emitted from now on
        self.splitk = 0                         # mdx_gemm_desc.splitk of dense() launches (1 = never split K)
        self.mod_ld = 0                         # row stride of the per-sample emb rows (rowbias / FiLM scale, shift)
        self.track = track_producers
        self.producer = {}      # device address of a tensor -> the descriptor of the launch that wrote it last
        self.op_index = {}      # descriptor address -> index of its op in `main`
        self.gn_calls = []      # GroupNorm sites, for the statistics wiring
        self.gn_convs = []      # convs that apply the GroupNorm of their input themselves (mdx_gemm_desc.gn_colstats)
        self.colstats = {}      # descriptor address -> statistics buffer (keeps them alive)
        self.gn_need, self.attn_ws_need = 4, 0
        self.gemm_ws = self.gn_ws = self.attn_ws = None

    # ------------------------------------------------------------------ buffers
    def get(self, shape, dtype=f16):
        t = self.A.get(shape, dtype)
        self.producer.pop(t.data_ptr(), None)   # a buffer handed out again is no longer "the output of that GEMM"
        return t

    def release(self, *tensors):
        for t in tensors:
            self.A.release(t)

    # ------------------------------------------------------------------ ops
    def emit(self, fn, kind, flops=0, launches=1, info=""):
        main, meta = self.into
        main.append(fn)
        meta.append({"kind": kind, "flops": int(flops), "launches": launches, "info": info, **self.tag})
        return meta[-1]

    def gemm(self, oplist=None, **kw):
        """One mdx_gemm_f16 launch (keywords of ops.make_gemm_desc).  oplist: a side list (the UNet's context plan) instead of
        the plan itself -- such launches have no meta record and produce nothing a GroupNorm reads."""
        d = ops.make_gemm_desc(**kw)
        d._w_tensor = kw["w"]       # (python-side attribute: the packed weight tensor this descriptor points at)
        self.descs.append(d)
        fn = (lambda d=d: ops.gemm_run(d))
        if oplist is not None:
            oplist.append(fn)
            return d
        if self.track:
            self.producer[kw["out"].data_ptr()] = d
            if self.into[0] is self.main:
                self.op_index[ctypes.addressof(d)] = len(self.main)
        ks, st, up = kw.get("ksize", 1), kw.get("stride", 1), kw.get("upsample", 0)
        hs, ws = (2 * kw["H"], 2 * kw["W"]) if up else (kw["H"], kw["W"])
        pad = 1 if ks == 3 else 0
        m_rows = kw["B"] * ((hs + 2 * pad - ks) // st + 1) * ((ws + 2 * pad - ks) // st + 1)
        kdim = ks * ks * (kw["c1"] + kw.get("c2", 0))
        rec = self.emit(fn, "gemm", 2 * m_rows * kw["N"] * kdim, 1, f"M={m_rows} N={kw['N']} K={kdim} k{ks}s{st}u{up}")
        rec["desc"] = d             # launches / split are filled in by account_gemm_launches (finish)
        return d

    def gn(self, x1, x2, g, b, eps, silu, out, scale=None, shift=None):
        """GroupNorm(32) (+ SiLU) of the virtual concat [x1 | x2]; scale / shift: FiLM rows `GN(h) * (1 + scale) + shift`
        (views of the [B, mod_ld] emb table).  How it runs is decided in finish(): statistics from the producers' epilogues,
        as the split-K reduce of the conv in front of it (the UNet planner's pass), or the plain launch."""
        Bq, HW, C1 = x1.shape
        C = C1 + (0 if x2 is None else x2.shape[2])
        self.gn_need = max(self.gn_need, ops.groupnorm_ws_floats(Bq, HW, C))
        prod = self.producer.get
        call = dict(x1=x1, x2=x2, g=g, b=b, eps=eps, silu=silu, out=out, cs=None, meta=len(self.meta), film=scale is not None,
                    prod=(prod(x1.data_ptr()), None if x2 is None else prod(x2.data_ptr())))
        self.producer.pop(out.data_ptr(), None)      # the GroupNorm output is not a GEMM output
        if self.track:
            self.gn_calls.append(call)
        mod_ld = self.mod_ld

        def run(c=call):
            if c.get("fs") is not None:     # the producer deferred its split-K reduce to this GroupNorm (one launch for both)
                return ops.groupnorm_from_splitk(c["fs"], g, b, eps, silu, out)
            if c["cs"] is not None:         # statistics from the producers' epilogues: one launch, one read of x
                cs1, n1, cs2, n2 = c["cs"]
                return ops.groupnorm_colstats(x1, cs1, n1, x2, cs2, n2, g, b, eps, silu, out=out, scale=scale, shift=shift,
                                              mod_ld=mod_ld if scale is not None else 0)
            if scale is not None:
                return ops.groupnorm_scaleshift(x1, x2, g, b, scale, shift, mod_ld, eps, silu, ws=self.gn_ws, out=out)
            return ops.groupnorm(x1, x2, g, b, eps, silu, ws=self.gn_ws, out=out)
        # (a tracked plan starts from the two-launch form and finish() corrects it; an untracked one is not accounted)
        self.emit(run, "groupnorm", 0, 2 if self.track else 1, f"B={Bq} HW={HW} C={C}")

    def dense(self, src, rows_b, tokens, cin, nout, wt, bias=None, residual=None, epilogue=ops.EPI_NONE, out=None,
              out_ld=None, out_mode=ops.OUT_ROWMAJOR, src2=None, c2=0, oplist=None, **kw):
        """Dense / 1x1 conv on [rows_b, tokens, cin] token rows; allocates the output unless `out` is given."""
        cols = nout // 2 if epilogue == ops.EPI_GEGLU else nout
        if out is None:
            out, out_ld = self.get((rows_b, tokens, cols)), cols
        kw.setdefault("splitk", self.splitk)
        self.gemm(oplist, a=src, w=wt, N=nout, B=rows_b, H=tokens, W=1, c1=cin - c2, out=out, out_ld=out_ld, a2=src2, c2=c2,
                  bias=bias, residual=residual, residual_ld=cols if residual is not None else 0, epilogue=epilogue,
                  out_mode=out_mode, **kw)
        return out

    def conv3(self, src, cin, cout, wt, bias, h, wd, stride=1, upsample=0, rowbias=None, residual=None, src2=None, c2=0,
              skip=None, gn=None, wsub=None, asym_pad=0):
        """3x3 conv (pad 1; nearest-2x folded into the gather with `upsample`) -> (out, ho, wo).
        skip = (x, x2, c1, c2, packed 1x1 weights): a ResBlock's skip_connection rides on this launch as extra K tiles
        (mdx_gemm_desc.skip_w); `bias` then holds the sum of both convs' biases.  gn = (gamma, beta, eps): GroupNorm + SiLU of
        `src` inside the conv; the statistics pointer is wired in finish()."""
        B = self.B
        hs, ws = (2 * h, 2 * wd) if upsample else (h, wd)
        ho, wo = (hs + 2 - 3) // stride + 1, (ws + 2 - 3) // stride + 1
        out = self.get((B, ho * wo, cout))
        kw = {}
        if skip is not None:
            kw = dict(skip_a=skip[0], skip_a2=skip[1], skip_c1=skip[2], skip_c2=skip[3], skip_w=skip[4])
        if gn is not None:
            kw.update(gn_gamma=gn[0], gn_beta=gn[1], gn_eps=gn[2], gn_silu=1)
        if wsub is not None:
            kw["w_sub"] = wsub
        d = self.gemm(a=src, w=wt, N=cout, B=B, H=h, W=wd, c1=cin - c2, out=out, out_ld=cout, a2=src2, c2=c2, bias=bias,
                      rowbias=rowbias, rowbias_ld=self.mod_ld if rowbias is not None else 0, residual=residual,
                      residual_ld=cout if residual is not None else 0, ksize=3, stride=stride, upsample=upsample,
                      asym_pad=asym_pad, **kw)
        rec = self.meta[-1]
        if skip is not None:
            rec["flops"] += 2 * B * ho * wo * cout * (skip[2] + skip[3])
            rec["info"] += f" +skip1x1 K={skip[2] + skip[3]}"
        if gn is not None:
            self.gn_convs.append(d)
            rec["info"] += " +groupnorm(in)"
            self.gn_calls.append(dict(x1=src, x2=None, conv=d, meta=len(self.meta) - 1, film=False,
                                      prod=(self.producer.get(src.data_ptr()), None)))
        return out, ho, wo

    def skip_fusable(self, a2, c1, c2, cout, ho, wo, wt):
        """Can a ResBlock's 1x1 skip_connection ride on its second conv (mdx_gemm_desc.skip_w)?  Channel counts in whole
        64-channel K tiles, and the conv must resolve to the HALO 3x3 kernel."""
        if not ops.get_option("unet_skip_fuse") or c1 % 64 or c2 % 64 or cout % 64:
            return False
        probe = ops.make_gemm_desc(a=a2, w=wt, N=cout, B=self.B, H=ho, W=wo, c1=cout, out=a2, out_ld=cout, ksize=3)
        return ops.gemm_query(probe)[3] == 1

    def attention(self, qk, vt, o, heads, dh, info="", causal=False, split_kv=False):
        """Self-attention on the fused-projection layout: qk [B, n, 2 * inner] holds q | k side by side, vt [B, inner, nv] is
        V^T (nv >= n: rows padded to 8), o [B, n, inner].  split_kv: the launch may use the plan's split-KV workspace."""
        B, n, inner = o.shape
        nv = vt.shape[2]
        if split_kv:
            self.attn_ws_need = max(self.attn_ws_need, ops.attention_ws_bytes(B, heads, dh, n, n))
        return self.emit(lambda: ops.attention(
            qk.data_ptr(), qk.data_ptr() + inner * 2, vt.data_ptr(), o.data_ptr(), B, heads, dh, n, n, dh ** -0.5,
            n * 2 * inner, 2 * inner, n * 2 * inner, 2 * inner, inner * nv, nv, n * inner, inner, causal=causal,
            ws=self.attn_ws if split_kv else None), "attention", 4 * B * heads * n * n * dh, 1, info)

    # ------------------------------------------------------------------ finish
    def _size_workspace(self):
        """The shared split-K workspace, sized for the hungriest descriptor and patched into all of them (grows only)."""
        need = max([ops.gemm_workspace_bytes(d) for d in self.descs] + [16])
        if self.gemm_ws is None or need > self.gemm_ws.numel() * 4:
            self.gemm_ws = ops.new_gemm_workspace(need, self.dev)
            self.patch_workspace(self.gemm_ws)

    def patch_workspace(self, ws):
        for d in self.descs:
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4

    def before_wiring(self):
        """Planner-specific passes on the descriptors, with the workspace of the first sizing in place."""

    def after_wiring(self):
        """Planner-specific passes behind the statistics wiring (dead ops are still in the lists)."""

    def finish(self, P):
        self._size_workspace()
        self.gn_ws = torch.empty(self.gn_need, dtype=f32, device=self.dev)
        if self.attn_ws_need:
            self.attn_ws = ops.attention_workspace(self.attn_ws_need, self.dev)
        self.before_wiring()
        if self.track and os.environ.get("MDX_UNET_GN_COLSTATS", "1") != "0":
            wire_groupnorm_colstats(self.gn_calls, self.meta, self.B, self.dev, self.colstats)
        else:
            for c in self.gn_calls:     # launch accounting of the one-launch fused kernel
                C = c["x1"].shape[2] + (0 if c["x2"] is None else c["x2"].shape[2])
                if _one_launch_groupnorm(c["x1"].shape[1], C):
                    self.meta[c["meta"]]["launches"] = 1
        self.after_wiring()
        # the statistics epilogue is part of the tile table's launch-variant key: a wired producer may resolve to another row
        # (another split) than the one the shared workspace was sized for -- size it again and grow it if needed
        self._size_workspace()
        if any(m.get("dead") for m in self.meta):      # GroupNorm launches that moved into the GEMM behind them
            keep = [i for i, m in enumerate(self.meta) if not m.get("dead")]
            self.main[:] = [self.main[i] for i in keep]
            self.meta[:] = [self.meta[i] for i in keep]
        check_colstats_wiring(self.descs)
        account_gemm_launches(self.meta)     # last: the column-statistics wiring above can change a launch's table row
        assert len(self.main) == len(self.meta)
        P.main, P.meta, P.descs, P.arena = self.main, self.meta, self.descs, self.A   # the arena owns the activation buffers
        P.gemm_ws, P.gn_ws = self.gemm_ws, self.gn_ws
        return P


def capture_or_eager(bodies, warm=None):
    """Warm up each op list once (`warm`: other lists to run instead, when one pass covers several bodies), synchronise, capture
    each body as one hipGraph -> the graphs in order, or None when the runtime refuses (the caller then runs eagerly)."""
    try:
        for body in (bodies if warm is None else warm):
            for op in body:
                op()
        torch.cuda.synchronize()
        return [ops.capture_graph(body) for body in bodies]
    except Exception as e:  # pragma: no cover - depends on the runtime
        warnings.warn(f"hipGraph capture failed, running eagerly: {e}")
        return None


# ---------------------------------------------------------------------------------------------------------------
# Post-passes of finish()
def account_gemm_launches(meta):
    """After the shared workspace is patched into the descriptors: launches per GEMM op = the kernel plus a split-K reduce
    launch unless the split is reduced in the kernel; the op's info string gets the real split."""
    for m in meta:
        d = m.get("desc")
        if d is None:
            continue
        q = ops.gemm_query(d)
        m["launches"] = 2 if (q[2] > 1 and not q[6] and not d.defer_reduce) else 1
        m["info"] = m["info"].split(" split=")[0] + f" split={q[2] if q[2] > 1 else 0}" + ("i" if q[6] else "")


def check_colstats_wiring(descs):
    """AFTER the shared split-K workspace has its final size: wire_groupnorm_colstats sized every statistics buffer for the row
    blocks the launch reports under an AMPLE workspace (its ideal form); the launch takes that form only if the final workspace
    really holds it.  A plan that kept the first-sized workspace would fail at its first launch with a colstats_cap mismatch --
    fail here instead, with the descriptor named."""
    for d in descs:
        rows = getattr(d, "_cs_rows", None)
        if rows is None or not d.colstats_out:
            continue
        now = ops.gemm_query(d)[5]
        if now != rows:
            raise _lib.MdxError(f"GroupNorm statistics wiring: the launch M={d.B * d.H * d.W} N={d.N} k{d.ksize} writes {now}-row "
                                f"blocks under the final workspace ({d.workspace_bytes} bytes) but its statistics buffer was sized "
                                f"for {rows}-row blocks: size the workspace from gemm_workspace_bytes() AFTER the wiring pass")


def _unwire(fresh, table):
    """Producers wired for a GroupNorm that ends up not using them must not keep paying for the statistics epilogue (nor resolve
    to that launch variant's tile-table row)."""
    for key, d in fresh:
        table.pop(key, None)
        d.colstats_out = 0
        if hasattr(d, "colstats_cap"):
            d.colstats_cap = 0
    fresh.clear()


def wire_groupnorm_colstats(gn_calls, meta, batch, device, table):
    """Run AFTER the split-K workspace is patched into the descriptors (mdx_gemm_query then sees the real split factors): every
    GroupNorm whose inputs are GEMM outputs and that would take the two-launch path (>= ~1k pixels per sample) gets its
    statistics from its producers' epilogues (mdx_gemm_desc.colstats_out) -- gn_stats and its read pass disappear.  gn_calls:
    dicts with x1, x2, prod = (desc of x1's producer, desc of x2's producer), meta = index into `meta`; sets call["cs"] = (cs1,
    nrb1, cs2, nrb2).  `table` keeps the statistics buffers alive (descriptor address -> tensor)."""
    fold_many = ops.get_option("gn_colstats_fold") != 0
    for c in gn_calls:
        _, HW, C1 = c["x1"].shape
        # fused SpatialTransformer head / GroupNorm inside the consuming conv: the statistics feed that launch (any block count)
        is_head = c.get("head") is not None or c.get("conv") is not None or c.get("proj") is not None
        C2 = 0 if c["x2"] is None else c["x2"].shape[2]
        if not is_head and _one_launch_groupnorm(HW, C1 + C2):
            meta[c["meta"]]["launches"] = 1
            continue

        fresh = []      # producers wired by THIS GroupNorm (undone if its other source cannot supply statistics)

        def stats_of(d, cx):
            if isinstance(d, _lib.StTailDesc):      # fused SpatialTransformer tail: per-row-block column sums of its output
                key = ctypes.addressof(d)
                if key not in table:
                    rows = d.tile_rows
                    if d.C != cx or HW % rows or HW // rows > 128:
                        return None
                    buf = torch.zeros((batch * (HW // rows), cx, 2), dtype=f32, device=device)
                    d.colstats_out = buf.data_ptr()
                    table[key] = (buf, HW // rows)
                    fresh.append((key, d))
                return table[key]
            if d is None or d.N != cx or d.out_ld != cx or d.defer_reduce:
                return None
            key = ctypes.addressof(d)
            if key in table:
                return table[key]
            # The statistics epilogue is part of the launch VARIANT the tile table is keyed by: ask with the field already set
            # (any non-null value), or the row blocks the query reports are those of a different tile / split choice than the
            # launch will make (a 64-row split-K reduce writing into a buffer sized for 128-row tiles).
            d.colstats_out = 8
            # ... and with an AMPLE workspace: finish() sizes the shared workspace again after this pass (to the largest ideal
            # need of any descriptor), so the launch will take the variant's ideal form -- with the workspace of the first
            # sizing the query can report a fallback (e.g. an un-split 128-row tile where the tuned row splits five ways and its
            # reduce kernel writes 64-row blocks: found by tools/shape_sweep.py --model glide at a 32-pixel base, round 5 -- the
            # launch then refused the statistics buffer as too small)
            keep_ws = d.workspace_bytes
            d.workspace_bytes = 1 << 40
            rows = ops.gemm_query(d)[5]
            d.workspace_bytes = keep_ws
            if rows <= 0 or HW % rows or HW // rows > 4096:
                d.colstats_out = 0
                return None
            buf = torch.zeros((batch * (HW // rows), cx, 2), dtype=f32, device=device)
            d.colstats_out, d.colstats_cap = buf.data_ptr(), batch * (HW // rows)
            d._cs_rows = rows       # (python-side) what the buffer was sized for: check_colstats_wiring() re-asks after the final sizing
            if HW // rows > 64 and not is_head and fold_many:
                # > 64 row blocks per sample (GLIDE's 128 x 128 / 256 x 256 levels: 512 HALO patches): folding them in EVERY
                # gn_apply block cost more than the statistics pass it saved (profiles/r02_e_ab.txt); they are folded ONCE by
                # a small launch in front of the GroupNorm instead (mdx_colstats_fold_f32)
                table[key] = (FoldedColStats(buf, HW // rows, batch), HW // rows)
            elif HW // rows > 64 and not is_head:
                d.colstats_out = 0
                return None
            else:
                table[key] = (buf, HW // rows)
            fresh.append((key, d))
            return table[key]
        s1 = stats_of(c["prod"][0], C1)
        if c.get("proj") is not None:
            # GroupNorm (no activation) in front of a Dense / 1x1 conv: the consumer applies it to its A fragments when the
            # producer can supply column statistics in <= 64 row blocks per sample and an M tile stays inside one sample;
            # otherwise this call falls back to the GroupNorm launch it was planned with (handled below like any other)
            pj = c.pop("proj")
            dd = pj["desc"]
            ok = False
            if s1 is not None and not isinstance(s1[0], FoldedColStats) and int(s1[1]) <= 64:
                keep = (dd.a, dd.gn_colstats, dd.gn_nrb, dd.gn_gamma, dd.gn_beta, dd.gn_eps, dd.gn_silu)
                dd.a, dd.gn_colstats, dd.gn_nrb = c["x1"].data_ptr(), s1[0].data_ptr(), int(s1[1])
                dd.gn_gamma, dd.gn_beta, dd.gn_eps, dd.gn_silu = c["g"].data_ptr(), c["b"].data_ptr(), float(c["eps"]), 0
                ok = ops.gemm_check(dd) and HW % ops.gemm_query(dd)[0] == 0
                if not ok:
                    dd.a, dd.gn_colstats, dd.gn_nrb, dd.gn_gamma, dd.gn_beta, dd.gn_eps, dd.gn_silu = keep
            if ok:
                dd._gn_src = (c["x1"], s1[0])       # (python-side: keeps the raw input and the statistics buffer alive)
                meta[c["meta"]]["dead"] = True      # finish() drops the GroupNorm op
                meta[pj["meta"]]["info"] += " +groupnorm(in)"
                continue
            _unwire(fresh, table)
            is_head = False
            if _one_launch_groupnorm(HW, C1 + C2):
                meta[c["meta"]]["launches"] = 1
                continue
            s1 = stats_of(c["prod"][0], C1)
        if is_head:
            if s1 is not None and c.get("head") is not None:
                c["head"].colstats, c["head"].nrb = s1[0].data_ptr(), int(s1[1])
            elif s1 is not None:
                c["conv"].gn_colstats, c["conv"].gn_nrb = s1[0].data_ptr(), int(s1[1])
            continue
        s2 = stats_of(c["prod"][1], C2) if C2 else (None, 0)
        if s1 is None or s2 is None:    # one source cannot supply statistics: the GroupNorm takes the two-launch path
            _unwire(fresh, table)
            continue
        c["cs"] = (s1[0], s1[1], s2[0], s2[1])
        meta[c["meta"]]["launches"] = 1 + isinstance(s1[0], FoldedColStats) + isinstance(s2[0], FoldedColStats)
