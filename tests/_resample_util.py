"""The resampling kernel's definition restated in numpy (tests/test_resample_cpu.py, tests/test_resample_kernels_gpu.py)."""
import numpy as np


def apply_tables(x, ys, yw, xs, xw, wrap_x=False):
    """The kernel's definition in numpy, in the dtype of x: columns first (clamped, or wrapped), then rows (clamped)."""
    H, W = x.shape[-2:]
    xi = xs[:, None].astype(np.int64) + np.arange(xw.shape[1])[None]
    xi = xi % W if wrap_x else np.clip(xi, 0, W - 1)
    t = (x[..., :, xi] * xw).sum(-1)
    yi = np.clip(ys[:, None].astype(np.int64) + np.arange(yw.shape[1])[None], 0, H - 1)
    return (t[..., yi, :] * yw[..., None]).sum(-2)


def parity_bound(yw, xw, x_max):
    """max |kernel - float64 restatement on the same fp32 tables|, derived: each fp32 fma chain of T terms carries a relative error
    of at most gamma_T ~ T * 2^-24 on sum |w| |x| (Higham, Accuracy and Stability, the inner-product bound with u = 2^-24); the
    horizontal result is stored and fed to the vertical chain, which is the factor 2.  Lx, Ly: the largest row sums of |w|."""
    Lx, Ly = float(np.abs(xw).sum(1).max()), float(np.abs(yw).sum(1).max())
    return 2.0 * (xw.shape[1] + yw.shape[1]) * 2.0 ** -24 * Lx * Ly * float(x_max)
