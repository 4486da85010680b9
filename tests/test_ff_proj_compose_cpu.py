"""proj_out folded into the feed-forward's second Dense (ops.compose_ff_proj, option unet_ff_proj_fuse), on the host.

    out = x + b_p + W_p (tok3 + b_f2 + W_f2 g) = x + bc + [g | tok3] [Wc | W_p]^T,   Wc = fp16(W_p W_f2),  bc = b_p + W_p b_f2

The composed launch rounds differently from the two launches it replaces: it never rounds the [M, C] token tensor to fp16, but it
rounds the product matrix Wc to fp16 once at load time -- into the fp16 subnormal range when the weights are small.  Both paths are
emulated in numpy with fp16 rounding where the kernels round (fp32 accumulation, the accumulator staged as fp16, then
fp16(float(staged) + bias + residual): gemm_epilogue of csrc/gemm_internal.h) and set against the float64 result of the stored fp16
operands.  Condition: the composed path's rel-L2 error is at most 1.25 x the two-launch path's, at weight scales 1, 0.2 and 0.05
(C = 640, M = 256; at 0.05 most entries of Wc are fp16 subnormals).
"""
import numpy as np
import pytest
import torch

C, M = 640, 256


def h16(a):
    return np.asarray(a, dtype=np.float16)


def launch(a16, w16, bias32, res16):
    """One dense launch as the kernels compute it: fp16 operands, fp32 accumulate, fp16 staging, fp16(staged + bias + residual)."""
    acc = a16.astype(np.float32) @ w16.astype(np.float32).T
    staged = acc.astype(np.float16).astype(np.float32)
    return (staged + bias32[None, :] + res16.astype(np.float32)).astype(np.float16)


def rel_l2(got, ref):
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(((got - ref) ** 2).sum() / (ref ** 2).sum()))


@pytest.fixture(scope="module", params=[1.0, 0.2, 0.05], ids=lambda s: f"scale{s}")
def case(request):
    from minddiffusion_amd import ops
    s = request.param
    r = np.random.RandomState(int(1000 * s))
    d = dict(scale=s,
             g=h16(r.standard_normal((M, 4 * C))), tok3=h16(r.standard_normal((M, C))), x=h16(r.standard_normal((M, C))),
             w_f2=h16(s * r.standard_normal((C, 4 * C)) / np.sqrt(4 * C)), w_p=h16(s * r.standard_normal((C, C)) / np.sqrt(C)),
             b_f2=(0.1 * r.standard_normal(C)).astype(np.float32), b_p=(0.1 * r.standard_normal(C)).astype(np.float32))
    comp, bc = ops.compose_ff_proj(*(torch.from_numpy(d[k]) for k in ("w_p", "b_p", "w_f2", "b_f2")))
    d["comp"], d["bc"] = comp.numpy(), bc.numpy()
    f = {k: d[k].astype(np.float64) for k in ("g", "tok3", "x", "w_f2", "w_p", "b_f2", "b_p")}
    d["ref"] = f["x"] + f["b_p"] + (f["tok3"] + f["b_f2"] + f["g"] @ f["w_f2"].T) @ f["w_p"].T
    d["f64"] = f
    return d


def test_composed_path_is_as_accurate_as_the_two_launches(case):
    c = case
    tok = launch(c["g"], c["w_f2"], c["b_f2"], c["tok3"])
    two = launch(tok, c["w_p"], c["b_p"], c["x"])
    one = launch(np.concatenate([c["g"], c["tok3"]], 1), c["comp"], c["bc"], c["x"])
    e_two, e_one = rel_l2(two, c["ref"]), rel_l2(one, c["ref"])
    wc = c["comp"][:, :4 * C]
    sub = float(((np.abs(wc) < 2.0 ** -14) & (wc != 0)).mean())
    print(f"PARITY ff_proj_compose scale={c['scale']}: composed {e_one:.3e}, two launches {e_two:.3e}, apart {rel_l2(one, two):.3e}, "
          f"subnormal entries of Wc {sub:.2f}")
    assert e_one <= 1.25 * e_two, (e_one, e_two)
    if c["scale"] == 0.05:
        assert sub > 0.5, sub      # the case means to exercise subnormal composite weights


def test_composite_weight_and_bias(case):
    c, f = case, case["f64"]
    assert c["comp"].dtype == np.float16 and c["comp"].shape == (C, 5 * C) and c["bc"].dtype == np.float32
    assert np.array_equal(c["comp"][:, 4 * C:], c["w_p"])                      # the residual-stream segment is W_p itself
    wc64 = f["w_p"] @ f["w_f2"]
    got = c["comp"][:, :4 * C].astype(np.float64)
    ulp16 = np.maximum(np.spacing(np.abs(wc64).astype(np.float16)).astype(np.float64), 2.0 ** -24)
    assert np.all(np.abs(got - wc64) <= ulp16)                                  # fp16(W_p W_f2), product taken in fp64
    bc64 = f["b_p"] + f["w_p"] @ f["b_f2"]
    assert np.all(np.abs(c["bc"].astype(np.float64) - bc64) <= np.spacing(np.abs(bc64).astype(np.float32)).astype(np.float64))
