"""tests/_isolation.py catches what it is for: three numpy stand-ins for a batched op -- a clean one, one that reads a neighbour
and multiplies the value away, one that indexes a per-sample quantity off by one -- and the harness's own control."""
import numpy as np
import pytest
import torch

import _isolation as I

pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")      # NaN / Inf go in on purpose
B, T, C = 3, 5, 8


def problem(seed=3):
    rng = np.random.RandomState(seed)
    return dict(x=rng.standard_normal((B, T, C)).astype(np.float32), bias=rng.standard_normal((B, C)).astype(np.float32),
                w=rng.standard_normal((C, C)).astype(np.float32))


PER_SAMPLE = {"x": {"axis": 0}, "bias": {"axis": 0}}


def clean(inp):
    return np.stack([inp["x"][b] @ inp["w"] + inp["bias"][b] for b in range(B)])


def masked_neighbour(inp):
    """Row b also reads sample b + 1 and multiplies it by zero: invisible to any finite-data parity test."""
    x = inp["x"]
    with np.errstate(invalid="ignore"):
        return np.stack([x[b] @ inp["w"] + inp["bias"][b] + 0.0 * x[(b + 1) % B] for b in range(B)])


def off_by_one_bias(inp):
    return np.stack([inp["x"][b] @ inp["w"] + inp["bias"][b - 1] for b in range(B)])


own = lambda out, b: [out[b]]


def failed_variants(op, r):
    with pytest.raises(AssertionError) as e:
        I.assert_isolated("stand_in", op, problem(), PER_SAMPLE, r, own)
    return {v for v in I.VARIANTS if f"{v}: output 0 of sample {r}" in str(e.value)}, str(e.value)


@pytest.mark.parametrize("r", range(B))
def test_clean_op_passes(r):
    I.assert_isolated("stand_in_clean", clean, problem(), PER_SAMPLE, r, own)


@pytest.mark.parametrize("r", range(B))
def test_masked_neighbour_read_fails_on_nan_and_inf_only(r):
    failed, msg = failed_variants(masked_neighbour, r)
    assert failed == {"nan", "inf"}, msg
    assert "is not finite (first at flat index 0" in msg


@pytest.mark.parametrize("r", range(B))
def test_off_by_one_per_sample_bias_fails_on_other(r):
    failed, msg = failed_variants(off_by_one_bias, r)
    assert "other" in failed and "base" not in failed, msg
    assert "differs from the base run (first at flat index 0" in msg


def test_variants_touch_only_the_neighbours():
    inp = problem()
    inp["h"] = torch.arange(B * T * 4, dtype=torch.float16).reshape(B * T, 4)
    inp["slot"] = torch.tensor([0, 1, 2], dtype=torch.int32)
    per = dict(PER_SAMPLE, h={"rows": T}, slot={"other": torch.tensor([5, 6, 7], dtype=torch.int32)})
    seen = dict(I.variants(inp, per, 1, seed=0))
    assert tuple(seen) == I.VARIANTS and seen["base"]["x"] is inp["x"]
    for kind in ("other", "nan", "inf"):
        v = seen[kind]
        assert v["w"] is inp["w"]                                                   # shared: untouched
        assert np.array_equal(v["x"][1], inp["x"][1]) and np.array_equal(v["bias"][1], inp["bias"][1])
        assert torch.equal(v["h"][T:2 * T], inp["h"][T:2 * T]) and v["h"].dtype == torch.float16
        assert v["slot"].tolist() == [5, 1, 7]
        for b in (0, 2):
            assert not np.array_equal(v["x"][b], inp["x"][b])
    assert np.isnan(seen["nan"]["x"][[0, 2]]).all() and np.isnan(seen["nan"]["bias"][[0, 2]]).all()
    assert bool(torch.isnan(seen["nan"]["h"][:T]).all()) and bool(torch.isnan(seen["nan"]["h"][2 * T:]).all())
    assert np.isposinf(seen["inf"]["x"][[0, 2]]).all()
    h = seen["inf"]["h"][:T].reshape(-1)
    assert bool(torch.isposinf(h[0::2]).all()) and bool((h[1::2] == I.F16_MAX).all())      # fp16: +Inf and 65504
    assert np.isfinite(seen["other"]["x"]).all() and abs(float(seen["other"]["x"][0].mean()) - 0.7) < 1.0
    assert np.array_equal(inp["x"], problem()["x"])                                # the caller's inputs are not modified


def test_a_harness_that_perturbs_nothing_fails_the_control():
    inp = problem()
    with pytest.raises(AssertionError, match="perturbed nothing"):
        I.assert_isolated("stand_in_control", lambda i: clean(inp), inp, PER_SAMPLE, 1, own)
