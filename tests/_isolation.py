"""Sample isolation: no output of batch row r depends on the per-sample inputs of the other rows.

The footprint tests (tests/_guard.py) poison everything OUTSIDE the logical inputs; this is the complement: poison inside the
logical inputs, in the other samples.  A case is one batched entry point at a fixed batch size, launch form and row position r.
It runs four times on inputs that differ only in the per-sample inputs of the samples b != r:

  base    the inputs as given (seeded, finite)
  other   the neighbours re-drawn from another seed at another scale and offset (statistics, row maxima, branches differ)
  nan     every per-sample input of the neighbours all NaN
  inf     the same with +Inf (fp16: +Inf and 65504 alternating)

and every output that belongs to sample r must be finite and torch.equal across the four.  No tolerance: the reference of a run
is the same launch on other neighbours.  The control -- some neighbour's output differs between base and other -- fails a harness
that perturbs nothing.  Deliberately NOT asserted: equality across row positions or batch sizes (summation order may differ).

`per_sample` maps an input's name to where its samples are: {"axis": k} (sample index on axis k) or {"rows": T} (T consecutive
rows of axis 0 per sample, the [B * T, C] layout).  Integer inputs (slot positions) cannot hold NaN: give {"other": tensor} and the
neighbours take that tensor's values in all three perturbed variants; on a float input "other" replaces the re-draw.
Inputs are torch tensors or numpy arrays; inputs not named in `per_sample` are shared and pass through untouched.
Plain helper module: no fixtures, no test collection.
"""
import json
import os

import numpy as np
import torch

from _util import LOG

VARIANTS = ("base", "other", "nan", "inf")
F16_MAX = 65504.0


def _samples_first(t, spec):
    """View of t with the sample index as axis 0."""
    if "rows" in spec:
        T = int(spec["rows"])
        assert t.shape[0] % T == 0, (tuple(t.shape), T)
        return t.view(t.shape[0] // T, T, *t.shape[1:])
    return t.movedim(int(spec.get("axis", 0)), 0)


def batch_of(inputs, per_sample):
    sizes = {int(_samples_first(torch.as_tensor(inputs[k]), s).shape[0]) for k, s in per_sample.items()}
    assert len(sizes) == 1, f"per-sample inputs disagree on the batch size: {sorted(sizes)}"
    return sizes.pop()


def _fill(kind, like, spec, gen):
    """A tensor shaped like `like` holding what the neighbours get in variant `kind`."""
    alt = spec.get("other")
    if not like.dtype.is_floating_point:
        assert alt is not None, "an integer per-sample input needs {'other': tensor}"
        return torch.as_tensor(alt).to(like.device, like.dtype).reshape(like.shape)
    if kind == "other":
        if alt is not None:
            return torch.as_tensor(alt).to(like.device, like.dtype).reshape(like.shape)
        z = torch.randn(like.shape, generator=gen, dtype=torch.float32)
        return (2.5 * z + 0.7).to(like.device, like.dtype)
    if kind == "nan":
        return torch.full_like(like, float("nan"))
    f = torch.full_like(like, float("inf"))
    if like.dtype == torch.float16:      # the largest finite fp16 next to +Inf: sums overflow, differences are NaN
        f.view(-1)[1::2] = F16_MAX
    return f


def variants(inputs, per_sample, r, seed):
    """Yields (variant, inputs) for the four variants above; row r and every shared input are the same bits in all of them."""
    gen = torch.Generator().manual_seed(int(seed) + 7919)
    for kind in VARIANTS:
        out = dict(inputs)
        if kind != "base":
            for k, spec in per_sample.items():
                src = inputs[k]
                t = torch.from_numpy(np.array(src)) if isinstance(src, np.ndarray) else src.clone()
                assert t.is_contiguous() or "rows" not in spec
                v = _samples_first(t, spec)
                fill = _samples_first(_fill(kind, t, spec, gen), spec)
                for b in range(v.shape[0]):
                    if b != r:
                        v[b] = fill[b]
                out[k] = t.numpy() if isinstance(src, np.ndarray) else t
        yield kind, out


def _tensors(x):
    return [torch.as_tensor(np.array(t)) if isinstance(t, np.ndarray) else t.detach().clone() for t in x]


def _first_diff(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    ne = (a != b) | (a != a) | (b != b)
    i = int(ne.nonzero()[0]) if bool(ne.any()) else -1
    return i, (float(a[i]), float(b[i])) if i >= 0 else None


def _log(rec):
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    print("PARITY", json.dumps(rec))


def assert_isolated(name, run, inputs, per_sample, r, own, seed=0):
    """run(inputs) -> outputs (fresh or reused buffers, any structure); own(outputs, b) -> the list of tensors / arrays that
    belong to sample b (copied here before the next run).  Asserts, for sample r: finite in all four variants, torch.equal to the
    base run in the other three; and the control on the neighbours.  Reports the variant, the output and the first flat index."""
    B = batch_of(inputs, per_sample)
    assert 0 <= r < B and B >= 2, (r, B)
    mine, theirs = {}, {}
    for kind, inp in variants(inputs, per_sample, r, seed):
        out = run(inp)
        if any(isinstance(t, torch.Tensor) and t.is_cuda for t in own(out, r)):
            torch.cuda.synchronize()
        mine[kind] = _tensors(own(out, r))
        if kind in ("base", "other"):
            theirs[kind] = [_tensors(own(out, b)) for b in range(B) if b != r]
    problems = []
    n = len(mine["base"])
    assert n > 0 and all(t.numel() > 0 for t in mine["base"]), f"{name}: sample {r} owns no output"
    for kind in VARIANTS:
        assert len(mine[kind]) == n
        for i, t in enumerate(mine[kind]):
            if t.dtype.is_floating_point and not bool(torch.isfinite(t).all()):
                j = int((~torch.isfinite(t)).reshape(-1).nonzero()[0])
                problems.append(f"{kind}: output {i} of sample {r} is not finite (first at flat index {j}: {float(t.reshape(-1)[j])})")
            elif kind != "base" and not torch.equal(t, mine["base"][i]):
                j, vals = _first_diff(mine["base"][i], t)
                problems.append(f"{kind}: output {i} of sample {r} differs from the base run (first at flat index {j}: "
                                f"base {vals[0]!r}, {kind} {vals[1]!r})")
    control = any(not torch.equal(x, y) for nb, no in zip(theirs["base"], theirs["other"]) for x, y in zip(nb, no))
    _log(dict(name=name, kind="isolation", r=r, B=B, outputs=n, elements=int(sum(t.numel() for t in mine["base"])),
              control=control, failed=sorted({p.split(":")[0] for p in problems})))
    assert not problems, f"{name} (r = {r}): " + "; ".join(problems)
    assert control, f"{name} (r = {r}): no neighbour's output differs between base and other -- the harness perturbed nothing"
