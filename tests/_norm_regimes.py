"""Input regimes for the normalisation kernels, their float64 references, and a numpy emulation of one-pass fp32 statistics.

A regime is a kind of input at which a normalisation kernel can be wrong without the usual `randn * 1.5 + 0.3` noticing:

  unit       1.5 z + 0.3                     the suite's ordinary input (baseline)
  eps        2^-8 z                          variance 1.5e-5: eps = 1e-5 against 1e-6 is a 25 % effect on the output
  offset8    0.25 z +- 2                     mean / std = 8:   one-pass variance (sum x^2 / n - mean^2) cancels 2 digits ...
  offset32   0.25 z +- 8                     mean / std = 32:  ... 3 digits: the most fp32 carries at rel-L2 1e-3
  offset128  0.25 z +- 32                    mean / std = 128: beyond it; measured against one_pass_floor
  const      one group == 4.0, one == 0      variance exactly 0: the clamp and eps are all that is left
  spike      unit, one element = 2000        a variance dominated by one value

`z` is standard normal, STANDARDISED per group (per row for LayerNorm) so that every group realises the nominal mean and spread;
the sign of an offset alternates by group and sample.  Everything returned is float32 holding fp16-exact values, so the kernel
(fp16 input) and the float64 references here see the same numbers.  Plain helper module: no fixtures, no test collection.
"""
import numpy as np

REGIMES = ("unit", "eps", "offset8", "offset32", "offset128", "const", "spike")
OFFSETS = {"offset8": 2.0, "offset32": 8.0, "offset128": 32.0}      # mean; the spread is 0.25
OFFSET_STD = 0.25
EPS_STD = 2.0 ** -8
SPIKE = 2000.0


def h16(a):
    return np.asarray(a, dtype=np.float16).astype(np.float32)


def const_groups(b, groups):
    """(index of the group that is 4.0 everywhere, index of the all-zero group) of sample b in the `const` regime."""
    return b % groups, (b + 1) % groups


def regime(name, rng, B, C, HW, groups):
    """fp16-exact float32 [B, C, HW] (channel-major: transpose for the NHWC kernels)."""
    assert name in REGIMES and C % groups == 0
    cpg = C // groups
    z = rng.standard_normal((B, groups, cpg * HW))
    if cpg * HW > 1:
        z = (z - z.mean(-1, keepdims=True)) / z.std(-1, keepdims=True)
    if name == "eps":
        x = EPS_STD * z
    elif name in OFFSETS:
        sign = 1.0 - 2.0 * ((np.arange(B)[:, None] + np.arange(groups)[None, :]) % 2)
        x = OFFSET_STD * z + OFFSETS[name] * sign[:, :, None]
    else:
        x = 1.5 * z + 0.3
    if name == "const":
        assert groups >= 2
        for b in range(B):
            gc, gz = const_groups(b, groups)
            x[b, gc] = 4.0
            x[b, gz] = 0.0
    x = x.reshape(B, C, HW)
    if name == "spike":
        for b in range(B):
            x[b, (7 * b + 3) % C, (5 * b + 1) % HW] = SPIKE
    return h16(x)


def const_rows(rows):
    """(rows that are 4.0 everywhere, all-zero rows) of the row version of the `const` regime."""
    r = np.arange(rows)
    return r[r % 3 == 0], r[r % 3 == 1]


def regime_rows(name, rng, rows, C):
    """Row version for LayerNorm: fp16-exact float32 [rows, C]; a row is what a group is above."""
    if name == "const":
        x = regime("unit", rng, rows, C, 1, 1).reshape(rows, C)
        r4, r0 = const_rows(rows)
        x[r4] = 4.0
        x[r0] = 0.0
        return x
    return regime(name, rng, rows, C, 1, 1).reshape(rows, C)


def affine(rng, C):
    """gamma, beta with |gamma|, |beta| <= 3 (fp32)."""
    return rng.uniform(-3, 3, C).astype(np.float32), rng.uniform(-3, 3, C).astype(np.float32)


def silu(y):
    return y / (1.0 + np.exp(-y))


def group_stats(x, groups):
    """float64 per-(sample, group) mean and biased variance of x [B, C, HW]."""
    B, C, HW = x.shape
    xg = np.asarray(x, np.float64).reshape(B, groups, -1)
    return xg.mean(-1), xg.var(-1)


def gn_apply(x, mean, var, gamma, beta, eps, act=False, scale=None, shift=None):
    """float64 GroupNorm output from given per-(sample, group) statistics; scale / shift: optional FiLM rows [B, C]."""
    B, C, HW = x.shape
    groups = mean.shape[1]
    xg = np.asarray(x, np.float64).reshape(B, groups, -1)
    y = ((xg - mean[..., None]) / np.sqrt(var[..., None] + eps)).reshape(B, C, HW)
    y = y * np.asarray(gamma, np.float64)[None, :, None] + np.asarray(beta, np.float64)[None, :, None]
    if scale is not None:
        y = y * (1.0 + np.asarray(scale, np.float64)[:, :, None]) + np.asarray(shift, np.float64)[:, :, None]
    return silu(y) if act else y


def gn_ref(x, gamma, beta, eps, groups, act=False, scale=None, shift=None):
    """float64 nn.GroupNorm(groups, C, eps) [FiLM] [SiLU] of x [B, C, HW]."""
    mean, var = group_stats(x, groups)
    return gn_apply(x, mean, var, gamma, beta, eps, act, scale, shift)


def ln_ref(x, gamma, beta, eps):
    """float64 nn.LayerNorm([C], eps) of rows [rows, C]."""
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = x.var(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def one_pass_stats(x, groups, chain=16):
    """What a one-pass fp32 kernel makes of the statistics of x [B, C, HW]: every lane adds `chain` values (and their squares)
    serially in float32, the lanes' partials are then folded by np.sum(dtype=float32) (pairwise, like a shuffle / LDS tree);
    mean = s / n, var = max(q / n - mean^2, 0), all float32.  Returns float64 copies of the float32 mean and variance."""
    B, C, HW = x.shape
    xg = np.asarray(x, np.float32).reshape(B, groups, -1)
    n = xg.shape[-1]
    lanes = -(-n // chain)
    pad = np.zeros((B, groups, lanes * chain), np.float32)
    pad[..., :n] = xg
    pad = pad.reshape(B, groups, lanes, chain)
    s = np.zeros((B, groups, lanes), np.float32)
    q = np.zeros((B, groups, lanes), np.float32)
    for k in range(chain):
        v = pad[..., k]
        s = s + v
        q = q + v * v
    s, q = np.sum(s, -1, dtype=np.float32), np.sum(q, -1, dtype=np.float32)
    inv = np.float32(1.0) / np.float32(n)
    mean = s * inv
    var = np.maximum(q * inv - mean * mean, np.float32(0.0))
    assert mean.dtype == np.float32 and var.dtype == np.float32
    return mean.astype(np.float64), var.astype(np.float64)


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(((got - ref) ** 2).sum()) / (np.sqrt((ref ** 2).sum()) + 1e-30))


def one_pass_floor(x, groups, gamma=None, beta=None, eps=1e-5, act=False, scale=None, shift=None, chain=16):
    """rel-L2 error that one-pass fp32 statistics alone (no output rounding) leave in GroupNorm(x) [FiLM] [SiLU]: the emulation of
    one_pass_stats against exact statistics, everything downstream of the statistics in float64.  gamma / beta default to 1 / 0."""
    C = x.shape[1]
    gamma = np.ones(C) if gamma is None else gamma
    beta = np.zeros(C) if beta is None else beta
    mean, var = one_pass_stats(x, groups, chain)
    got = gn_apply(x, mean, var, gamma, beta, eps, act, scale, shift)
    return rel_l2(got, gn_ref(x, gamma, beta, eps, groups, act, scale, shift))
