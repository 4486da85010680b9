"""Keeps the input regimes of tests/_norm_regimes.py honest, and shows that the tolerances of tests/test_norm_regimes_gpu.py
can be met by a correct kernel: a numpy emulation of one-pass fp32 statistics (what every GroupNorm form and every
LayerNorm-fold site computes) plus fp16 output rounding stays inside them.  No GPU."""
import numpy as np
import pytest

import _norm_regimes as R

# (B, C, HW, groups): 640 and 40 960 values per group -- the smallest and the largest group of the GPU cases
SHAPES = [(2, 320, 64, 32), (1, 320, 4096, 32)]
# serial additions per lane before the tree: 4 (fused forms on 2 x 2 pixels) ... 64 (a 256-slab of a 128 x 128 tensor)
CHAINS = [4, 16, 64]


@pytest.fixture(scope="module")
def inputs():
    out = {}
    for shape in SHAPES:
        for name in R.REGIMES:
            out[name, shape] = R.regime(name, np.random.RandomState(len(name) + shape[2]), *shape)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d" % (s[1] // s[3] * s[2]))
@pytest.mark.parametrize("name", R.REGIMES)
def test_regimes_realise_their_nominal_statistics(inputs, name, shape):
    B, C, HW, groups = shape
    x = inputs[name, shape]
    assert x.dtype == np.float32 and x.shape == (B, C, HW)
    assert np.array_equal(x, R.h16(x)), "not fp16-exact"
    mean, var = R.group_stats(x, groups)
    std = np.sqrt(var)
    if name in R.OFFSETS:
        ratio = np.abs(mean) / std
        nominal = R.OFFSETS[name] / R.OFFSET_STD
        assert np.all(np.abs(ratio / nominal - 1) < 0.1), (ratio.min(), ratio.max())
        sign = np.sign(mean)
        assert np.all(sign[:, 1:] == -sign[:, :-1]) and (B == 1 or np.all(sign[1:] == -sign[:-1])), "offsets must alternate"
    elif name == "eps":
        assert np.all(np.abs(std / R.EPS_STD - 1) < 0.1) and np.all(np.abs(mean) < 0.1 * std)
        tiny = np.abs(x[x != 0]) < 2.0 ** -14
        assert tiny.any() and tiny.mean() < 0.05, "a few, not many, fp16 subnormals"
    elif name == "unit":
        assert np.all(np.abs(std / 1.5 - 1) < 0.1) and np.all(np.abs(mean / 0.3 - 1) < 0.1)
    elif name == "const":
        for b in range(B):
            gc, gz = R.const_groups(b, groups)
            xg = x[b].reshape(groups, -1)
            assert np.all(xg[gc] == 4.0) and np.all(xg[gz] == 0.0)
            rest = [g for g in range(groups) if g not in (gc, gz)]
            assert np.all(np.abs(std[b, rest] / 1.5 - 1) < 0.1)
    else:
        assert all((x[b] == R.SPIKE).sum() == 1 for b in range(B))
        assert np.sort(var.reshape(-1))[-B] > 0.5 * R.SPIKE ** 2 / (C // groups * HW), "the spike must dominate its group's variance"


def test_row_regimes():
    for name in R.REGIMES:
        x = R.regime_rows(name, np.random.RandomState(3), 5, 72)
        assert x.shape == (5, 72) and np.array_equal(x, R.h16(x))
    x = R.regime_rows("const", np.random.RandomState(3), 5, 72)
    r4, r0 = R.const_rows(5)
    assert list(r4) == [0, 3] and list(r0) == [1, 4] and np.all(x[r4] == 4.0) and np.all(x[r0] == 0.0) and x[2].std() > 1
    x = R.regime_rows("offset32", np.random.RandomState(3), 5, 72)
    assert np.all(np.abs(np.abs(x.mean(1)) / x.std(1) / 32 - 1) < 0.1)


def test_eps_regime_makes_eps_visible(inputs):
    """eps = 1e-5 against 1e-6 under a variance of 1.5e-5: rstd differs by 25 %, far above any tolerance of the GPU tests --
    a site that drops eps, hard-codes it, or swaps two of them cannot pass both settings."""
    for shape in SHAPES:
        x = inputs["eps", shape]
        g, b = R.affine(np.random.RandomState(1), shape[1])
        assert R.rel_l2(R.gn_ref(x, g, 0 * b, 1e-6, shape[3]), R.gn_ref(x, g, 0 * b, 1e-5, shape[3])) > 0.2
        # with the |beta| <= 3 of the GPU tests in the denominator the effect is still 50 x the 1e-3 tolerance
        assert R.rel_l2(R.gn_ref(x, g, b, 1e-6, shape[3]), R.gn_ref(x, g, b, 1e-5, shape[3])) > 0.05
    rows = R.regime_rows("eps", np.random.RandomState(2), 5, 320)
    g, b = R.affine(np.random.RandomState(1), 320)
    assert R.rel_l2(R.ln_ref(rows, g, 0 * b, 1e-6), R.ln_ref(rows, g, 0 * b, 1e-5)) > 0.2


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d" % (s[1] // s[3] * s[2]))
def test_one_pass_fp32_leaves_a_margin_at_offset32(inputs, shape, chain):
    """sum x^2 / n - mean^2 in fp32 at mean / std = 32: at most 3e-4, a third of the 1e-3 the GPU tests allow."""
    floor = R.one_pass_floor(inputs["offset32", shape], shape[3], chain=chain)
    print(f"one_pass_floor offset32 n={shape[1] // shape[3] * shape[2]} chain={chain}: {floor:.3e}")
    assert floor <= 3e-4, floor
    assert R.one_pass_floor(inputs["offset8", shape], shape[3], chain=chain) <= 3e-5


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d" % (s[1] // s[3] * s[2]))
def test_offset128_bound_covers_the_spread_between_chain_lengths(inputs, shape):
    """The GPU tests bound offset128 by 4 * one_pass_floor(chain = 16) + 5e-4: every emulated accumulation order, with fp16 output
    rounding on top, must fit under it."""
    x = inputs["offset128", shape]
    g, b = R.affine(np.random.RandomState(4), shape[1])
    floor = R.one_pass_floor(x, shape[3], g, b)
    ref = R.gn_ref(x, g, b, 1e-5, shape[3])
    for chain in CHAINS:
        mean, var = R.one_pass_stats(x, shape[3], chain)
        err = R.rel_l2(R.h16(R.gn_apply(x, mean, var, g, b, 1e-5)), ref)
        print(f"offset128 n={shape[1] // shape[3] * shape[2]} chain={chain}: emulated {err:.3e}, floor(16) {floor:.3e}")
        assert err <= 4 * floor + 5e-4, (chain, err, floor)


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d" % (s[1] // s[3] * s[2]))
@pytest.mark.parametrize("name", [n for n in R.REGIMES if n != "offset128"])
def test_a_correct_one_pass_kernel_meets_the_gpu_tolerances(inputs, name, shape, act):
    """Emulated one-pass statistics + fp16 output rounding against the float64 reference, at the tolerances of the GPU file:
    rel-L2 1e-3, max_abs 2e-2 (not for spike), and 4e-3 against act(beta) on the constant and the all-zero groups."""
    B, C, HW, groups = shape
    x = inputs[name, shape]
    g, b = R.affine(np.random.RandomState(5), C)
    ref = R.gn_ref(x, g, b, 1e-5, groups, act)
    for chain in CHAINS:
        mean, var = R.one_pass_stats(x, groups, chain)
        got = R.h16(R.gn_apply(x, mean, var, g, b, 1e-5, act))
        assert R.rel_l2(got, ref) <= 1e-3, (chain, R.rel_l2(got, ref))
        if name != "spike":
            assert np.abs(got - ref).max() <= 2e-2
        if name == "const":
            cpg = C // groups
            tgt = R.silu(b.astype(np.float64)) if act else b.astype(np.float64)
            for s in range(B):
                for gi in R.const_groups(s, groups):
                    sl = slice(gi * cpg, (gi + 1) * cpg)
                    assert np.abs(got[s, sl] - tgt[sl, None]).max() <= 4e-3
