"""Tap tables of the separable resampling kernel (include/mdx.h: mdx_resample_f32, csrc/resample.hip).

The kernel knows no interpolation mode: per axis it gets, for every output index i, a first input index start[i] and T weights, and
computes sum_k w[i][k] * in[e(start[i] + k)] as one ascending fp32 fma chain (e clamps to the axis, or wraps with wrap_x).  The
tables are computed here in float64 and rounded once to fp32.

Modes (s = n_in / n_out):
  nearest    one tap at (i * n_in) // n_out, integer arithmetic -- the rule mdx_inpaint_concat_f32 documents for its mask.  This is
             torch's "nearest" at integer ratios only: torch rounds a float scale.
  bilinear, bicubic without antialiasing: F.interpolate(align_corners=False).  The source coordinate is (i + 0.5) s - 0.5, clamped
             at 0 for bilinear; 2 taps, or 4 taps of the cubic convolution kernel with A = -0.75.
  bilinear, bicubic with antialiasing: torch's antialias=True.  Centre c = (i + 0.5) s, support {1, 2} * max(s, 1), taps
             lo = max(int(c - sup + 0.5), 0) .. hi = min(int(c + sup + 0.5), n_in), weights f((k - c + 0.5) / max(s, 1)) with the
             triangle or the cubic with A = -0.5, normalised to sum 1.
  lanczos3   the same scheme with f(x) = sinc(x) sinc(x / 3) on |x| < 3 (support 3 max(s, 1)); always antialiased.
n_out == n_in is the identity in every mode: one tap of weight 1.
wrap=True (the x axis of a panorama): no tap is truncated or clamped -- the full support is kept, start may be negative or reach
past n_in, and the kernel reduces the indices mod n_in.
"""
import numpy as np

MAX_TAPS = 32           # MDX_RESAMPLE_MAX_TAPS (include/mdx.h)
TILE_ROWS = 16          # RS_TH (csrc/resample.hip): the kernel's strip covers the rows of this many consecutive outputs
MODES = ("nearest", "bilinear", "bicubic", "lanczos3")


def _cubic(x, A):
    """The cubic convolution kernel (Keys) with parameter A, on |x| < 2."""
    x = np.abs(x)
    near = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * A
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _triangle(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _lanczos3(x):
    return np.where(np.abs(x) < 3.0, np.sinc(x) * np.sinc(x / 3.0), 0.0)


_FILTERS = {"bilinear": (_triangle, 1.0), "bicubic": (lambda x: _cubic(x, -0.5), 2.0), "lanczos3": (_lanczos3, 3.0)}


def _area_tables(n_in, n_out, mode, wrap):
    """The antialiased scheme (and lanczos3): per output index a window of the filter, scaled by max(s, 1), normalised."""
    f, half = _FILTERS[mode]
    s = n_in / n_out
    stretch = max(s, 1.0)
    sup = half * stretch
    rows = []
    for i in range(n_out):
        c = (i + 0.5) * s
        if wrap:
            lo, hi = int(np.floor(c - sup + 0.5)), int(np.floor(c + sup + 0.5))
        else:
            lo, hi = max(int(c - sup + 0.5), 0), min(int(c + sup + 0.5), n_in)
        k = np.arange(lo, hi, dtype=np.float64)
        w = f((k - c + 0.5) / stretch)
        rows.append((lo, w / w.sum()))
    return rows


def _point_tables(n_in, n_out, mode, wrap):
    """bilinear / bicubic as F.interpolate(align_corners=False) samples them, without antialiasing."""
    s = n_in / n_out
    rows = []
    for i in range(n_out):
        src = (i + 0.5) * s - 0.5
        if mode == "bilinear":
            if not wrap:
                src = max(src, 0.0)
            i0 = int(np.floor(src))
            lam = src - i0
            rows.append((i0, np.array([1.0 - lam, lam], np.float64)))
        else:
            i0 = int(np.floor(src))
            t = src - i0
            rows.append((i0 - 1, _cubic(np.array([t + 1.0, t, 1.0 - t, 2.0 - t], np.float64), -0.75)))
    return rows


def tap_table(n_in, n_out, mode, antialias=False, wrap=False, dtype=np.float32):
    """(start int32 [n_out], w dtype [n_out, T]) of one axis: output i is sum_k w[i, k] * in[e(start[i] + k)].  Rows that need
    fewer than T taps are padded with zero weights.  Computed in float64; dtype float32 (what the kernel takes) rounds once,
    float64 returns the unrounded weights.  A table of more than MAX_TAPS taps is refused (ValueError)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"tap_table: extents must be positive, got n_in={n_in}, n_out={n_out}")
    if mode not in MODES:
        raise ValueError(f"tap_table: mode must be one of {MODES}, got {mode!r}")
    if n_in == n_out:
        rows = [(i, np.ones(1, np.float64)) for i in range(n_out)]
    elif mode == "nearest":
        rows = [((i * n_in) // n_out, np.ones(1, np.float64)) for i in range(n_out)]
    elif mode == "lanczos3" or antialias:
        rows = _area_tables(n_in, n_out, mode, wrap)
    else:
        rows = _point_tables(n_in, n_out, mode, wrap)
    T = max(len(w) for _, w in rows)
    if T > MAX_TAPS:
        raise ValueError(f"tap_table: {mode}{' (antialiased)' if antialias or mode == 'lanczos3' else ''} from {n_in} to {n_out} "
                         f"needs {T} taps; the resampling kernel takes at most {MAX_TAPS} (resample in two steps)")
    start = np.array([lo for lo, _ in rows], np.int32)
    w = np.zeros((n_out, T), np.float64)
    for i, (_, wi) in enumerate(rows):
        w[i, :len(wi)] = wi
    return start, w.astype(dtype)


def strip_rows(n_in, n_out, T):
    """The rows of the LDS strip the kernel sizes from the geometry (csrc/resample.hip, resample_plan): enough for the input rows
    TILE_ROWS consecutive outputs of a tap_table reach."""
    return min((((TILE_ROWS - 1) * n_in + n_out - 1) // n_out) + T + 2, n_in)


def tile_span(start, T, n_in):
    """The most input rows any aligned tile of TILE_ROWS outputs reaches under the clamped edge rule (what the kernel stages)."""
    start = np.asarray(start, np.int64)
    lo, hi = np.clip(start, 0, n_in - 1), np.clip(start + T - 1, 0, n_in - 1)
    return max(int(hi[i:i + TILE_ROWS].max() - lo[i:i + TILE_ROWS].min()) + 1 for i in range(0, len(start), TILE_ROWS))
