"""Sampling sessions -- the parts that need no GPU: the slot scheduler against a backend that records its calls (admission order,
slot choice, start ticks, which ticks draw noise and which take the rescale form, retirement), the rows a request brings against
the samplers' own StepTable, the validation of submit's arguments, and the C-ABI declarations of the three slot entries."""
import os
import re

import numpy as np
import pytest

from minddiffusion_amd import _lib, ops
from minddiffusion_amd._lib import MdxError
from minddiffusion_amd.ldm.models.diffusion import schedule as SCH
from minddiffusion_amd.ldm.models.diffusion import session as S
from minddiffusion_amd.ldm.models.diffusion.ddim import DDIMSampler
from minddiffusion_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP
from test_per_request_cpu import StubModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder:
    """The backend surface SlotScheduler drives."""

    def __init__(self):
        self.calls = []

    def admit(self, slot, req, tick):
        self.calls.append(("admit", tick, slot, req.index))

    def tick(self, tick, any_noise, any_rescale):
        self.calls.append(("tick", tick, any_noise, any_rescale))

    def retire(self, slot, req):
        self.calls.append(("retire", slot, req.index))
        return ("latent", req.index)


def rows_for(steps, sigma_at=(), phi=0.0):
    rows = np.zeros((steps, ops.STEP_ROW), np.float32)
    rows[:, ops.STEP_ACTIVE] = 1.0
    rows[:, ops.STEP_RESCALE] = phi
    for p in sigma_at:
        rows[p, ops.STEP_SIGMA] = 0.25
    return rows


def test_scheduler_fills_the_lowest_free_slot_in_submission_order():
    """Steps [4, 1, 2, 1, 3] in 2 slots.  Request 0 draws noise at its positions 1 and 3, request 2 at position 0; requests 1
    and 4 rescale."""
    rec = Recorder()
    sch = S.SlotScheduler(2, rec)
    spec = [(4, (1, 3), 0.0), (1, (), 0.5), (2, (0,), 0.0), (1, (), 0.0), (3, (), 0.7)]
    reqs = [sch.submit(n, rows_for(n, sig, phi), np.zeros(n, np.float32)) for n, sig, phi in spec]
    assert [r.index for r in reqs] == list(range(5)) and not rec.calls            # submit touches nothing
    done = []
    while not sch.idle:
        done.append([(r.index, lat) for r, lat in sch.step()])
    #            tick 0          1    2          3                    4    5    6
    assert done == [[(1, ("latent", 1))], [], [(2, ("latent", 2))], [(0, ("latent", 0)), (3, ("latent", 3))], [], [],
                    [(4, ("latent", 4))]]
    assert sch.now == 7 and sch.step() == [] and sch.now == 7                       # an idle tick does not count
    assert [(r.slot, r.start) for r in reqs] == [(0, 0), (1, 0), (1, 1), (1, 3), (0, 4)]
    assert [c for c in rec.calls if c[0] == "admit"] == [("admit", 0, 0, 0), ("admit", 0, 1, 1), ("admit", 1, 1, 2),
                                                         ("admit", 3, 1, 3), ("admit", 4, 0, 4)]
    # tick: (noise, rescale).  0: r0 pos 0, r1 (phi) | 1: r0 pos 1 (sigma), r2 pos 0 (sigma) | 2: r0 pos 2, r2 pos 1 |
    # 3: r0 pos 3 (sigma), r3 | 4-6: r4 (phi)
    assert [c[1:] for c in rec.calls if c[0] == "tick"] == [(0, False, True), (1, True, False), (2, False, False),
                                                            (3, True, False), (4, False, True), (5, False, True),
                                                            (6, False, True)]
    # a request is admitted before the tick it first runs on, and retired after the tick it last runs on
    order = [c[:2] if c[0] != "retire" else (c[0], c[2]) for c in rec.calls]
    assert order[:4] == [("admit", 0), ("admit", 0), ("tick", 0), ("retire", 1)]
    assert rec.calls.index(("retire", 0, 0)) > rec.calls.index(("tick", 3, True, False))
    assert rec.calls.index(("retire", 0, 0)) < rec.calls.index(("admit", 4, 0, 4))


def test_scheduler_packs_as_a_greedy_simulation_says():
    """The tick count is the packing optimum of FIFO-into-lowest-slot, from an independent restatement."""
    for slots, steps in ((2, [4, 1, 2, 1, 3]), (3, [4, 1, 2, 4, 2]), (4, [20, 50] * 8), (1, [3, 2])):
        sch = S.SlotScheduler(slots, Recorder())
        for n in steps:
            sch.submit(n, rows_for(n), np.zeros(n, np.float32))
        sch.run_until_idle()
        free_at = [0] * slots
        for n in steps:                                         # each request takes the slot that frees first (lowest on ties)
            b = free_at.index(min(free_at))
            free_at[b] += n
        assert sch.now == max(free_at), (slots, steps)
    with pytest.raises(ValueError, match="slots"):
        S.SlotScheduler(0, Recorder())


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_ddim_request_rows_are_the_step_tables(eta):
    model = StubModel()
    steps, scales, phis = [2, 5, 1, 4], [1.5, 3.0, 7.5, 2.0], [0.0, 0.7, 0.3, 1.0]
    sampler = DDIMSampler(model)
    grids = []
    for s in steps:
        sampler.make_schedule(s, ddim_eta=eta, verbose=False)
        grids.append(sampler.time_grid(False, None, None))
    plans = [SCH.ddim_steps(sampler, g, False) for g in grids]
    mixed, t_mixed, _ = SCH.step_table(plans, scales, phis, True)
    for b, s in enumerate(steps):
        rows, t_in = S.request_rows(model, "ddim", s, scales[b], phis[b], eta)
        one, t_one, _ = SCH.step_table([plans[b]], [scales[b]], [phis[b]], True)
        assert rows.dtype == np.float32 and rows.shape == (s, ops.STEP_ROW) and t_in.shape == (s,)
        assert np.array_equal(rows.view(np.uint32), one.host()[:, 0].view(np.uint32))
        assert np.array_equal(rows.view(np.uint32), mixed.host()[:s, b].view(np.uint32))      # and row b of a mixed batch
        assert np.array_equal(t_in, t_one[:, 0]) and np.array_equal(t_in, t_mixed[:s, b])
        assert (rows[:, ops.STEP_SIGMA] != 0).all() == (eta != 0)
        req = S.Request(0, s, rows, t_in)
        assert req.draws == [eta != 0] * s and req.rescales == [phis[b] != 0] * s


def test_dpm_request_rows_are_the_step_tables():
    model = StubModel()
    ns = NoiseScheduleVP("discrete", alphas_cumprod=DPMSolverSampler(model).alphas_cumprod)
    steps, scales, phis = [1, 3, 4, 2], [1.5, 3.0, 7.5, 2.0], [0.0, 0.7, 0.3, 1.0]
    mixed, t_mixed, _ = SCH.step_table([SCH.dpm_steps(ns, s) for s in steps], scales, phis, True)
    for b, s in enumerate(steps):
        rows, t_in = S.request_rows(model, "dpm_solver", s, scales[b], phis[b])
        one, t_one, _ = SCH.step_table([SCH.dpm_steps(ns, s)], [scales[b]], [phis[b]], True)
        assert np.array_equal(rows.view(np.uint32), one.host()[:, 0].view(np.uint32))
        assert np.array_equal(rows.view(np.uint32), mixed.host()[:s, b].view(np.uint32))
        assert np.array_equal(t_in, t_one[:, 0]) and np.array_equal(t_in, t_mixed[:s, b])
        assert rows[0, ops.STEP_SIGMA] == 0          # c1 of a newcomer's first row: the previous prediction is not read
    with pytest.raises(ValueError, match="eta"):
        S.request_rows(model, "dpm_solver", 3, 2.0, 0.0, eta=0.5)
    with pytest.raises(ValueError, match="sampler"):
        S.request_rows(model, "plms", 3, 2.0)
    with pytest.raises(IndexError, match="choose S dividing"):          # no 3-step DDIM grid on 1000 training steps
        S.request_rows(model, "ddim", 3, 2.0)


def test_submit_argument_validation():
    ok = dict(steps=4, scale=7.5, guidance_rescale=0.3, eta=0.0, seed=5)
    chk = lambda sampler="ddim", **kw: S.check_request(sampler, 50, **dict(ok, **kw))
    assert chk() == (4, 7.5, 0.3, 0.0, 5)
    assert chk(seed=(1 << 64) - 1)[4] == -1 and chk(seed=-(1 << 63))[4] == -(1 << 63)
    assert chk(mask=None, x0=None, score_corrector=None, quantize_x0=False) == (4, 7.5, 0.3, 0.0, 5)
    for bad in (0, -1, 2.5, True, "4", float("nan")):
        with pytest.raises(ValueError, match="int >= 1"):
            chk(steps=bad)
    with pytest.raises(ValueError, match="max_steps=50"):
        chk(steps=51)
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="guidance_rescale"):
            chk(guidance_rescale=bad)
    with pytest.raises(ValueError, match="finite"):
        chk(scale=float("inf"))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eta"):
            chk(eta=bad)
    with pytest.raises(ValueError, match="DPM-Solver"):
        chk("dpm_solver", eta=0.5)
    for bad in (1.5, True, 1 << 64, -(1 << 63) - 1, "7"):
        with pytest.raises(MdxError, match="seed"):
            chk(seed=bad)
    for k, v in (("mask", object()), ("x0", object()), ("score_corrector", object()), ("quantize_x0", True)):
        with pytest.raises(ValueError, match=f"{k} is not available in a session"):
            chk(**{k: v})
    with pytest.raises(TypeError, match="unexpected keyword"):
        chk(strength=0.5)


def test_session_refuses_plms_and_unknown_samplers_before_touching_a_device():
    with pytest.raises(MdxError, match="PLMS evaluates the model twice"):
        S.SamplingSession(StubModel(), 2, sampler="plms")
    with pytest.raises(ValueError, match="sampler must be one of"):
        S.SamplingSession(StubModel(), 2, sampler="euler")


def test_the_package_exports_the_session():
    import minddiffusion_amd
    from minddiffusion_amd.pipeline import DiffusionPipeline
    assert minddiffusion_amd.SamplingSession is S.SamplingSession
    assert callable(DiffusionPipeline.session) and callable(DiffusionPipeline.serve)
    with pytest.raises(AttributeError):
        minddiffusion_amd.NoSuchThing


def test_more_than_one_rank_is_refused(monkeypatch):
    from minddiffusion_amd import distributed as D
    monkeypatch.setattr(D, "world", lambda: (0, 2))
    with pytest.raises(MdxError, match="single rank"):
        S.SamplingSession(StubModel(), 2, sampler="ddim")


def test_the_slot_entries_are_declared_with_the_headers_argument_counts():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdx.h")).read(), flags=re.S)
    for name in ("mdx_sampler_step_slots_f32", "mdx_randn_slots_f32", "mdx_slot_gather_f32"):
        args = re.search(rf"\bint {name}\s*\(([^)]*)\)", header).group(1)
        res, argtypes = _lib.SIGNATURES[name]
        assert res is _lib.c_int and len(argtypes) == len(args.split(",")), name
        assert argtypes[-1] is _lib.c_void_p                    # the stream
    # the slots entry is the table entry with `table` replaced by (sched, slot_start, slot_len, cap, tick)
    assert len(_lib.SIGNATURES["mdx_sampler_step_slots_f32"][1]) == len(_lib.SIGNATURES["mdx_sampler_step_table_f32"][1]) + 4
    assert len(_lib.SIGNATURES["mdx_randn_slots_f32"][1]) == len(_lib.SIGNATURES["mdx_randn_f32"][1]) + 3
    lib = _lib.load()
    # refused on the host, before any launch: no GPU is needed to see it
    assert lib.mdx_slot_gather_f32(16, 16, 16, 0, 0, 16, 1, 4, 2, None) == -1 and b"cap" in lib.mdx_last_error()
    assert lib.mdx_slot_gather_f32(16, None, 16, 4, 0, 16, 1, 4, 2, None) == -1 and b"null" in lib.mdx_last_error()
    assert lib.mdx_randn_slots_f32(16, 1, 0, 1.0, 0.0, 16, 16, 16, -1, 1, 4, None) == -1 and b"tick" in lib.mdx_last_error()
    assert lib.mdx_randn_slots_f32(16, 1, 0, 1.0, 0.0, 16, None, 16, 0, 1, 4, None) == -1 and b"null" in lib.mdx_last_error()
    step = lambda sched, cap, tick: lib.mdx_sampler_step_slots_f32(16, None, 16, 16, 8, 0, None, None, None, None, None, 16,
                                                                   None, sched, 16, 16, cap, tick, 0, None, 1, 4, 8, 8, None)
    assert step(None, 4, 0) == -1 and b"null slot pointer" in lib.mdx_last_error()
    assert step(16, 0, 0) == -1 and b"cap" in lib.mdx_last_error()
    assert step(16, 4, -1) == -1 and b"tick" in lib.mdx_last_error()
