"""SamplingSession -- continuous batching for the LDM samplers: the B samples of one UNet batch are SLOTS, a request is admitted
into a free slot of a batch that is already running, runs its own complete schedule from there, is handed back on the tick it
finishes, and the slot is refilled.  Neither reference tree has this; sample() / __call__ are untouched.

Three layers:
  * request_rows()      the rows and model-input timesteps of ONE request: its plan (schedule.ddim_steps / dpm_steps, as the
                        samplers build theirs) merged into a one-sample StepTable by schedule.step_table: numpy only.
  * SlotScheduler       which request sits in which slot on which tick: a FIFO into the lowest free slot.  It mirrors every
                        slot's position by counting and never reads the device.
  * SamplingSession     the device state (written only when a request is admitted) and the launches of one tick:
                        ops.slot_blend where some active slot blends (an img2img request with a keep_mask), ops.slot_gather,
                        the two x copies into the guidance batch, the UNet, ops.randn_slots where some active slot draws
                        noise, ops.sampler_step_slots in place.
"""
import collections

import numpy as np
import torch

from .... import distributed as D
from .... import ops
from ...._lib import MdxError
from ...modules.encoders import WINDOW
from .ddim import DDIMSampler
from .dpm_solver import DPMSolverSampler
from .dpm_solver.dpm_solver import NoiseScheduleVP
from .schedule import check_strength, ddim_steps, dpm_partial_start, dpm_steps, per_request, pred_type, step_table

SAMPLERS = ("ddim", "dpm_solver")
_REFUSED_KEYWORDS = ("mask", "x0", "score_corrector", "quantize_x0", "image_guidance_scale", "image_scale")


def request_rows(model, sampler, steps, scale, guidance_rescale=0.0, eta=0.0, t_enc=None):
    """(rows [n, ops.STEP_ROW] float32, t_input [n] float32) of one request: the rows a StepTable holds for it served
    as a batch of one -- its plan from schedule.ddim_steps (on the sampler's own time_grid) or schedule.dpm_steps, merged by
    schedule.step_table and validated by StepTable.host() (finite, phi in [0, 1], sqrt_at != 0) -- and the model-input timestep
    of every evaluation.  `model` needs what a sampler reads before it touches the device (the schedule arrays).
    t_enc None: the full run, n = steps.  Otherwise the partial run of an img2img request, n = t_enc: the last t_enc steps of
    the `steps`-step schedule, as decode(t_start=t_enc) (DDIM) or sample(S=t_enc, t_start=) (DPM-Solver) walk them."""
    n = steps if t_enc is None else int(t_enc)
    if not 1 <= n <= steps:
        raise ValueError(f"t_enc must be an integer in [1, {steps}] (the model evaluations that remain), got {t_enc!r}")
    if sampler == "ddim":
        s = DDIMSampler(model)
        s.make_schedule(ddim_num_steps=steps, ddim_eta=eta, verbose=False)      # IndexError: no grid for this step count
        plan = ddim_steps(s, s.time_grid(False, None, t_enc), False)
    elif sampler == "dpm_solver":
        if eta != 0.0:
            raise ValueError("eta: DPM-Solver draws no step noise, eta must be 0")
        ac = DPMSolverSampler(model).alphas_cumprod
        plan = dpm_steps(NoiseScheduleVP("discrete", alphas_cumprod=ac), n,
                         None if t_enc is None else dpm_partial_start(ac.shape[0], steps, n))
    else:
        raise ValueError(f"sampler must be one of {SAMPLERS} in a session, got {sampler!r}")
    table, t_rows, total = step_table([plan], [scale], [guidance_rescale], True)
    rows = table.host()[:, 0]
    assert rows.shape == (n, ops.STEP_ROW) and total == n
    return np.ascontiguousarray(rows), np.ascontiguousarray(t_rows[:, 0], dtype=np.float32)


def start_coefficients(model, sampler, steps, t_enc, eta=0.0):
    """(a, b) of x = a z0 + b noise at the level an img2img request starts from: the sampler's own q_coefficients at the start
    DiffusionPipeline._partial_start selects (grid index t_enc of the `steps`-step schedule; for DPM-Solver the continuous time)."""
    if sampler == "ddim":
        s = DDIMSampler(model)
        s.make_schedule(ddim_num_steps=steps, ddim_eta=eta, verbose=False)
        return s.q_coefficients(t_enc)
    d = DPMSolverSampler(model)
    return d.q_coefficients(dpm_partial_start(d.alphas_cumprod.shape[0], steps, t_enc))


def blend_coefficients(model, t_input):
    """[n, 2] float32: (sqrt_alphas_cumprod[t], sqrt_one_minus_alphas_cumprod[t]) at the integer model-input timestep of every
    position -- the sampler's make_schedule arrays, so the values decode() hands ops.q_sample at the top of its iterations."""
    ac = np.asarray(model.alphas_cumprod, dtype=np.float32)
    t = np.asarray(t_input).astype(np.int64)
    return np.ascontiguousarray(np.stack([np.sqrt(ac)[t], np.sqrt(1. - ac)[t]], axis=1), dtype=np.float32)


def check_request(sampler, max_steps, steps, scale, guidance_rescale, eta, seed, **refused):
    """The scalar arguments of SamplingSession.submit, checked and normalised: (steps, scale, guidance_rescale, eta, seed), the
    seed as the int64 pattern the kernels read.  `refused`: the sampler keywords a session does not take -- naming one with a
    value is a ValueError that says why, any other keyword a TypeError."""
    for k, v in refused.items():
        if k not in _REFUSED_KEYWORDS:
            raise TypeError(f"submit() got an unexpected keyword argument {k!r}")
        if v is not None and v is not False:
            raise ValueError(f"submit: {k} is not available in a session: "
                             + ("an img2img request takes init_latent= / init_image= (with strength=) and, for the blend, "
                                "keep_mask="
                                if k in ("mask", "x0") else
                                "three-branch image guidance is not served in sessions (a slot has no c_concat and the step rows "
                                "no middle scale yet)"
                                if k in ("image_guidance_scale", "image_scale") else "it leaves the fused step launch"))
    per_request([steps], [scale], [guidance_rescale], 1)                # an int >= 1, a finite scale, phi in [0, 1]
    steps, scale, guidance_rescale, eta = int(steps), float(scale), float(guidance_rescale), float(eta)
    if steps > max_steps:
        raise ValueError(f"submit: steps={steps} exceeds the session's max_steps={max_steps}")
    if not (np.isfinite(eta) and eta >= 0.):
        raise ValueError(f"submit: eta must be finite and >= 0, got {eta!r}")
    if sampler == "dpm_solver" and eta != 0.:
        raise ValueError("submit: eta: DPM-Solver draws no step noise, eta must be 0")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not -(1 << 63) <= int(seed) < (1 << 64):
        raise MdxError(f"submit: seed {seed!r} is not an integer in [-2^63, 2^64)")
    seed = int(seed) - (1 << 64) if int(seed) >= (1 << 63) else int(seed)
    return steps, scale, guidance_rescale, eta, seed


def _one_sample(name, t, dims, what):
    """A tensor [*dims] or [1, *dims] (None in a dims entry: any extent) -> its [*dims] view."""
    if not isinstance(t, torch.Tensor) or t.dim() not in (len(dims), len(dims) + 1) or (t.dim() > len(dims) and t.shape[0] != 1):
        raise MdxError(f"submit: {name} must be a tensor {what}, got "
                       f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    t = t.reshape(tuple(t.shape[-len(dims):]))
    if any(d is not None and int(s) not in (d if isinstance(d, tuple) else (d,)) for s, d in zip(t.shape, dims)):
        raise MdxError(f"submit: {name} has shape {tuple(t.shape)}, expected {what}")
    return t


def check_init(sampler, steps, shape, vae=None, init_latent=None, init_image=None, strength=None, keep_mask=None):
    """The img2img keywords of SamplingSession.submit, checked: (t_enc, init_latent [C, h, w], init_image [3, H, W], keep_mask
    [1 | C, h, w]), all None for a request that starts from noise.  steps: checked by check_request; shape: the session's latent
    shape; vae: model.first_stage_model.  Validates and reshapes only: nothing is copied or moved."""
    if init_latent is not None and init_image is not None:
        raise ValueError("submit: pass at most one of init_latent and init_image")
    if init_latent is None and init_image is None:
        for k, v in (("strength", strength), ("keep_mask", keep_mask)):
            if v is not None:
                raise ValueError(f"submit: {k} needs an init (init_latent= or init_image=)")
        return None, None, None, None
    t_enc = check_strength("submit", 0.75 if strength is None else strength, steps)
    C, h, w = shape
    if keep_mask is not None:
        if sampler == "dpm_solver":
            raise NotImplementedError("submit: keep_mask: mask blending is implemented by PLMSSampler / DDIMSampler (a 'ddim' "
                                      "session)")
        keep_mask = _one_sample("keep_mask", keep_mask, ((1, C), h, w), f"[1 | {C}, {h}, {w}] (the latent resolution)")
    if init_latent is not None:
        init_latent = _one_sample("init_latent", init_latent, (C, h, w), f"[{C}, {h}, {w}] (the session's latent shape)")
    else:
        if vae is None or not hasattr(vae, "encode_noised"):
            raise MdxError("submit: init_image= needs a VAE with an encoder attached (model.first_stage_model); pass init_latent=")
        init_image = _one_sample("init_image", init_image, (3, None, None), "[3, H, W] in [-1, 1]")
        got = tuple(vae.latent_shape((1,) + tuple(init_image.shape)))[1:]
        if got != (C, h, w):
            raise MdxError(f"submit: init_image {tuple(init_image.shape)} encodes to a latent {got}, the session's is {(C, h, w)}")
    return t_enc, init_latent, init_image, keep_mask


class Request:
    """One submitted request and, once it runs, where: `slot` and `start` (the session tick of its first model evaluation).
    `latent` is the finished [C, H, W] latent (a device tensor) from the tick it ended on.  `steps` is the number of ticks it
    runs: its step count, or t_enc of an img2img request."""

    def __init__(self, index, steps, rows, t_input, payload=None):
        self.index, self.steps, self.rows, self.t_input, self.payload = index, int(steps), rows, t_input, payload
        self.draws = [bool(v) for v in rows[:, ops.STEP_SIGMA] != 0]        # per position: does the step read its noise term
        self.rescales = [bool(v) for v in rows[:, ops.STEP_RESCALE] != 0]
        self.slot = self.start = self.latent = None

    @property
    def done(self):
        return self.latent is not None

    def __repr__(self):
        return f"Request({self.index}, steps={self.steps}, slot={self.slot}, start={self.start}, done={self.done})"


class SlotScheduler:
    """The host side of a session: pending requests wait in a FIFO; at the start of a tick they are admitted, in submission
    order, into the lowest free slots; a request admitted at tick T0 runs on ticks T0 .. T0 + steps - 1 and leaves at the end
    of the last one.  Deterministic, and all of it by counting: nothing here looks at the device.

    backend: an object with admit(slot, request, tick), tick(tick, any_noise, any_rescale) and retire(slot, request) -> latent
    (SamplingSession; the tests' recording stub)."""

    def __init__(self, slots, backend):
        if isinstance(slots, bool) or int(slots) != slots or int(slots) < 1:
            raise ValueError(f"slots must be an int >= 1, got {slots!r}")
        self.backend = backend
        self.slots = [None] * int(slots)
        self.pending = collections.deque()
        self.now = 0                    # the session tick: model evaluations so far
        self.submitted = 0

    def submit(self, steps, rows, t_input, payload=None):
        req = Request(self.submitted, steps, rows, t_input, payload)
        self.submitted += 1
        self.pending.append(req)
        return req

    @property
    def idle(self):
        return not self.pending and all(r is None for r in self.slots)

    def step(self):
        """One tick: admit, run, retire.  Returns [(request, latent)] of the requests that ended on it, by slot.  A tick with
        nothing to run (no pending request, every slot free) does nothing and does not count."""
        for b, held in enumerate(self.slots):
            if held is None and self.pending:
                req = self.pending.popleft()
                req.slot, req.start = b, self.now
                self.slots[b] = req
                self.backend.admit(b, req, self.now)
        running = [r for r in self.slots if r is not None]
        if not running:
            return []
        pos = [self.now - r.start for r in running]
        self.backend.tick(self.now, any(r.draws[p] for r, p in zip(running, pos)),
                          any(r.rescales[p] for r, p in zip(running, pos)))
        finished = []
        for b, r in enumerate(self.slots):
            if r is not None and self.now - r.start == r.steps - 1:
                r.latent = self.backend.retire(b, r)
                finished.append((r, r.latent))
                self.slots[b] = None
        self.now += 1
        return finished

    def run_until_idle(self):
        finished = []
        while not self.idle:
            finished += self.step()
        return finished


class SamplingSession:
    """A running guidance batch of `slots` samples of one latent shape, one sampler family and one context length, that
    requests enter and leave (module docstring).  Made by DiffusionPipeline.session().

    The device state of slot b -- its rows of sched / temb / seeds / slot_start / slot_len, rows b and slots + b of the
    [2 slots, T, D] context, and x[b] = its start latent -- is written when a request is admitted into it and by nothing else;
    the tick number is an argument of the three slot launches, so there is no cursor on the device.  x, the embedding rows, the
    context and sched are zero at creation: an empty slot evaluates finite numbers that nothing reads.
    DPM-Solver keeps its data predictions in two buffers that alternate by the parity of the SESSION tick; a newcomer's first
    row has c1 = 0, so it does not read the buffer a previous tenant left behind.
    The guidance batch is always used: a scale of exactly 1.0 goes through the combine eu + 1 * (ec - eu).
    temperature / noise_dropout: of the eta > 0 step noise (DDIM), session-wide.
    empty: the [1, 77, D] encoding of the empty window, for contexts shorter than context_len (default: the attached text
    encoder's).
    img2img requests (submit(init_latent= | init_image=, strength=)) start at position 0 of the PARTIAL run: they hold their slot
    for t_enc = int(strength * steps) ticks, from x[b] = a z0 + b noise.  With keep_mask= ('ddim' only) the slot also owns
    x0[b], keep[b], blend_ab[b] and blend_on[b] -- made on the first such admission, written only on admissions -- and every tick
    on which some active slot blends starts with one ops.slot_blend launch (the blend at the top of decode()'s iterations).
    sample_posterior: whether init_image= requests sample the VAE posterior or take its mode."""

    def __init__(self, model, slots, H=512, W=512, sampler="ddim", context_len=WINDOW, max_steps=50, temperature=1.0,
                 noise_dropout=0.0, device=None, empty=None, sample_posterior=True):
        if sampler == "plms":
            raise MdxError("SamplingSession: PLMS evaluates the model twice on a request's first step (plms.py:231-235), which "
                           "one shared evaluation per tick cannot give a newcomer alone: use 'ddim' or 'dpm_solver'")
        if sampler not in SAMPLERS:
            raise ValueError(f"sampler must be one of {SAMPLERS} in a session, got {sampler!r}")
        if D.world()[1] > 1:
            raise MdxError("SamplingSession: runs on a single rank (the sharded form is not built)")
        if getattr(model, "is_controlled", False):
            raise MdxError("SamplingSession: a ControlledDiffusion model is not served in sessions (a slot has no hint of its own)")
        key = getattr(getattr(model, "model", None), "conditioning_key", "crossattn")
        unet = getattr(model, "unet", None)
        if key != "crossattn" or getattr(unet, "num_classes", None) is not None or not hasattr(model, "time_embedding_table"):
            raise MdxError(f"SamplingSession: needs a text-conditional model with a timestep-only embedding table "
                           f"(conditioning_key 'crossattn', no class labels); got conditioning_key={key!r}: there is no "
                           f"per-slot c_concat and no table with a label embedding")
        for name, v in (("max_steps", max_steps), ("context_len", context_len)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError(f"{name} must be an int >= 1, got {v!r}")
        if not 0. <= float(noise_dropout) < 1.:
            raise ValueError("noise_dropout must be in [0, 1)")
        if H % 8 or W % 8:
            raise ValueError(f"H and W must be multiples of 8, got {H} x {W}")
        self.model, self.sampler = model, sampler
        self.scheduler = SlotScheduler(slots, self)
        B = self.B = len(self.scheduler.slots)
        self.shape = (4, H // 8, W // 8)
        self.context_len, self.cap = int(context_len), int(max_steps)
        self.temperature, self.noise_dropout = float(temperature), float(noise_dropout)
        self.pred_type = pred_type(model)
        dev = self.device = torch.device(device) if device is not None else unet.device
        if hasattr(unet, "set_max_context_len") and self.context_len > int(unet.max_context_len):
            unet.set_max_context_len(80 * -(-self.context_len // 80))
        self.empty = empty
        self._rows_cache = {}
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        self.emb_total = int(model.time_embedding_table(z(1)).shape[1])
        self.x = z(B, *self.shape)
        self.x_in = z(2 * B, *self.shape)                      # the guidance batch [uncond; cond]
        self.emb = z(2 * B, self.emb_total)                    # the time-embedding rows of the tick, same layout
        self.t_in = z(2 * B)                                   # (the UNet reads `emb`, not the timesteps)
        self.context = z(2 * B, self.context_len, int(unet.context_dim), dtype=torch.float16)
        self.sched = z(B, self.cap, ops.STEP_ROW)
        self.temb = z(B, self.cap, self.emb_total)
        self.seeds = z(B, dtype=torch.int64)
        self.slot_meta = z(2, B, dtype=torch.int32)            # slot_start | slot_len
        self.slot_start, self.slot_len = self.slot_meta[0], self.slot_meta[1]
        # the noise term of the step: the seeded draw (DDIM, eta > 0), or the previous data prediction (DPM-Solver)
        self.noise = z(B, *self.shape) if sampler == "ddim" else None
        self.x0_bufs = [z(B, *self.shape), z(B, *self.shape)] if sampler == "dpm_solver" else None
        self.sample_posterior = bool(sample_posterior)
        self.x0 = self.keep = self.blend_ab = self.blend_on = None      # the blend state: made by the first keep_mask admission
        self.unet_evals = 0
        self.admissions = 0
        self.blend_launches = 0

    # ---- host: submit never touches the device
    def _rows(self, steps, scale, guidance_rescale, eta, t_enc=None):
        key = (steps, scale, guidance_rescale, eta, t_enc)
        if key not in self._rows_cache:
            self._rows_cache[key] = request_rows(self.model, self.sampler, steps, scale, guidance_rescale, eta, t_enc)
        return self._rows_cache[key]

    def _check_context(self, name, t):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != 1):
            raise MdxError(f"submit: {name} must be a tensor [T, D] or [1, T, D], got "
                           f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        t = t.reshape((1,) + tuple(t.shape[-2:]))
        if t.shape[2] != self.context.shape[2]:
            raise MdxError(f"submit: {name} has width {t.shape[2]}, the UNet's context_dim is {self.context.shape[2]}")
        if t.shape[1] > self.context_len:
            raise MdxError(f"submit: {name} has {t.shape[1]} context tokens, the session was made for {self.context_len}")
        if t.shape[1] < self.context_len and (t.shape[1] % WINDOW or self.context_len % WINDOW):
            raise MdxError(f"submit: {name} has {t.shape[1]} context tokens and the session {self.context_len}: only whole "
                           f"{WINDOW}-token windows can be padded (encoders.pad_conditioning)")
        if t.shape[1] < self.context_len and self.empty is None and getattr(self.model, "cond_stage_model", None) is None:
            raise MdxError(f"submit: {name} is shorter than the session's context_len={self.context_len} and there is nothing "
                           f"to pad it with: pass empty= to the session or attach a text encoder")
        return t

    def submit(self, prompt=None, c=None, uc=None, steps=30, scale=7.5, guidance_rescale=0.0, eta=0.0, seed=0, init_latent=None,
               init_image=None, strength=None, keep_mask=None, **refused):
        """Queue one request; returns its handle (Request).  prompt (with a text encoder attached; encoded when the request is
        admitted) or c / uc tensors [T, D].  Never blocks and never touches the device.
        img2img: init_latent [C, h, w] (already scaled by scale_factor) or init_image [3, H, W] in [-1, 1] (needs
        model.first_stage_model), exactly one; strength in (0, 1], default 0.75: the request runs the last
        t_enc = int(strength * steps) steps of its `steps`-step schedule and holds its slot for t_enc ticks.  keep_mask
        [1 | C, h, w], 1 = keep the init latent there (img2img(mask=)'s meaning; 'ddim' sessions only).  Its draws -- the forward
        noise (ops.RNG_ENCODE), the posterior noise of init_image (ops.RNG_POSTERIOR), the step and blend draws, both counted
        from 0 at its first tick -- depend on `seed` alone.  An init_image is encoded at batch 1 when the request is ADMITTED:
        the encoder runs between two ticks and stalls that tick for every slot.  (The first init_image of a size builds the
        encoder's plan here, to learn its latent shape.)"""
        steps, scale, guidance_rescale, eta, seed = check_request(self.sampler, self.cap, steps, scale, guidance_rescale, eta,
                                                                  seed, **refused)
        t_enc, init_latent, init_image, keep_mask = check_init(
            self.sampler, steps, self.shape, getattr(self.model, "first_stage_model", None), init_latent, init_image, strength,
            keep_mask)
        if (prompt is None) == (c is None):
            raise MdxError("submit: pass either prompt= or c= (and uc=)")
        if prompt is not None:
            if not isinstance(prompt, str):
                raise MdxError("submit: prompt must be one string")
            if getattr(self.model, "cond_stage_model", None) is None:
                raise MdxError("submit: prompt= needs a text encoder attached to the model; pass c= / uc= tensors")
        else:
            c, uc = self._check_context("c", c), self._check_context("uc", uc)
            if uc is None:
                raise MdxError("submit: the guidance batch is always used in a session: pass uc= with c=")
        rows, t_input = self._rows(steps, scale, guidance_rescale, eta, t_enc)
        payload = {"prompt": prompt, "c": c, "uc": uc, "seed": seed, "t_enc": t_enc, "z0": init_latent, "image": init_image,
                   "keep": keep_mask}
        if t_enc is not None:
            key = ("start", steps, t_enc, eta)
            if key not in self._rows_cache:
                self._rows_cache[key] = tuple(float(v) for v in start_coefficients(self.model, self.sampler, steps, t_enc, eta))
            payload["ab"] = self._rows_cache[key]
        if keep_mask is not None:
            payload["blend_ab"] = blend_coefficients(self.model, t_input)
        return self.scheduler.submit(len(rows), rows, t_input, payload)

    def step(self):
        """One tick.  Returns [(handle, latent [C, H, W])] of the requests that ended on it."""
        return self.scheduler.step()

    def run_until_idle(self):
        return self.scheduler.run_until_idle()

    @property
    def tick_count(self):
        return self.scheduler.now

    # ---- device: the three calls the scheduler makes, all enqueued on the current stream, none synchronises
    def _empty_window(self):
        if self.empty is None:
            if getattr(self.model, "cond_stage_model", None) is None:
                raise MdxError("SamplingSession: a context shorter than context_len is padded with the encoding of the empty "
                               "window: pass empty= or attach a text encoder")
            self.empty = self.model.get_learned_conditioning([""])[:, :WINDOW]
        return self.empty

    def _fit(self, t):
        """A request's context at the session's length: extended with whole empty windows, as pad_conditioning does."""
        if t.shape[1] == self.context_len:
            return t
        e = self._empty_window().to(device=t.device, dtype=t.dtype)
        return torch.cat([t] + [e] * ((self.context_len - t.shape[1]) // WINDOW), dim=1)

    def admit(self, b, req, tick):
        p, B, dev = req.payload, self.B, self.device
        if p["prompt"] is not None:
            uc = self.model.get_learned_conditioning([""])
            c = self.model.get_learned_conditioning([p["prompt"]])
            if max(c.shape[1], uc.shape[1]) > self.context_len:
                raise MdxError(f"prompt {p['prompt'][:40]!r} encodes to {max(c.shape[1], uc.shape[1])} context tokens, the "
                               f"session was made for {self.context_len}")
        else:
            c, uc = p["c"], p["uc"]
        c, uc = self._fit(c), self._fit(uc)
        self.context[b].copy_(uc[0], non_blocking=True)         # in place: the UNet's context cache sees the version change
        self.context[B + b].copy_(c[0], non_blocking=True)
        self.seeds[b:b + 1].copy_(torch.tensor([p["seed"]], dtype=torch.int64), non_blocking=True)
        if p.get("t_enc") is None:
            ops.randn_seeded(self.seeds[b:b + 1], ops.RNG_X_T, 0, self.shape, out=self.x[b:b + 1])
        else:
            self._admit_init(b, req)
        if self.blend_on is not None:
            self.blend_on[b:b + 1].copy_(torch.tensor([int(p.get("keep") is not None)], dtype=torch.int32), non_blocking=True)
        self.sched[b, :req.steps].copy_(torch.from_numpy(req.rows), non_blocking=True)
        self.temb[b, :req.steps].copy_(self.model.time_embedding_table(torch.from_numpy(req.t_input).to(dev)))
        self.slot_meta[:, b].copy_(torch.tensor([tick, req.steps], dtype=torch.int32), non_blocking=True)
        self.admissions += 1

    def _admit_init(self, b, req):
        """The start latent of an img2img request, x[b] = a z0 + b randn(seed, RNG_ENCODE, 0) -- noised_latent's two launches on
        the one-row view, or for an image the encoder at batch 1 and its fused launch -- and, with a keep_mask, the slot's blend
        state."""
        p, dev = req.payload, self.device
        a, bb = p["ab"]
        row = self.x[b:b + 1]
        noise = ops.randn_seeded(self.seeds[b:b + 1], ops.RNG_ENCODE, 0, self.shape)
        if p["image"] is not None:
            post = ops.randn_seeded(self.seeds[b:b + 1], ops.RNG_POSTERIOR, 0, self.shape) if self.sample_posterior else None
            image = p["image"].to(device=dev, dtype=torch.float32)[None].contiguous()
            z0, x_enc = self.model.first_stage_model.encode_noised(image, self.model.scale_factor, a, bb, noise, post_noise=post,
                                                                   sample=self.sample_posterior)
            row.copy_(x_enc)
        else:
            z0 = p["z0"].to(device=dev, dtype=torch.float32)[None].contiguous()
            ops.q_sample(z0, noise, a, bb, out=row)
        if p["keep"] is None:
            return
        if self.blend_on is None:
            z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
            self.x0, self.keep = z(self.B, *self.shape), z(self.B, *self.shape)
            self.blend_ab, self.blend_on = z(self.B, self.cap, 2), z(self.B, dtype=torch.int32)
        self.x0[b].copy_(z0[0])
        self.keep[b].copy_(p["keep"].to(device=dev, dtype=torch.float32).expand(self.shape))
        self.blend_ab[b, :req.steps].copy_(torch.from_numpy(p["blend_ab"]), non_blocking=True)

    def tick(self, tick, any_noise, any_rescale):
        B = self.B
        # whether some active slot blends: from the requests held, by counting, as the scheduler finds any_noise
        if any(r is not None and r.payload.get("keep") is not None and 0 <= tick - r.start < r.steps
               for r in self.scheduler.slots):
            ops.slot_blend(self.x0, self.keep, self.x, self.seeds, ops.RNG_BLEND, 0, self.blend_ab, self.blend_on,
                           self.slot_start, self.slot_len, tick)
            self.blend_launches += 1
        ops.slot_gather(self.temb, self.slot_start, self.slot_len, tick, self.emb, reps=2)
        self.x_in[:B].copy_(self.x)
        self.x_in[B:].copy_(self.x)
        out = self.model.apply_model_nhwc(self.x_in, self.t_in, self.context, temb=self.emb, cfg_dup=True)
        self.unet_evals += 1
        noise = pred_x0 = None
        if self.sampler == "dpm_solver":
            pred_x0, prev = self.x0_bufs[tick & 1], self.x0_bufs[(tick & 1) ^ 1]
            noise = prev if any_noise else None
        elif any_noise:
            noise = ops.randn_slots(self.seeds, ops.RNG_STEP, 0, self.slot_start, self.slot_len, tick, self.noise,
                                    scale=self.temperature, dropout=self.noise_dropout)
        ops.sampler_step_slots(self.x, None, out[:B], out[B:], self.pred_type, [], noise, None, self.x, pred_x0, self.sched,
                               self.slot_start, self.slot_len, tick, any_rescale)

    def retire(self, b, req):
        return self.x[b].clone()
