"""Host-side math of DPM-Solver++ as the reference wires it (ldm/models/diffusion/dpm_solver/dpm_solver.py):
``NoiseScheduleVP('discrete')`` (:79-164), the ``time_uniform`` grid (:414-415) and the multistep order-2 update in
data-prediction form (``multistep_dpm_solver_second_update`` :742-797, first-order start / tail :488-532).

Everything here is float64 numpy on S+1 scalars; the per-element work of a step is ONE launch of the fused
``mdx_sampler_step_f32`` kernel (see sampler.py), so there is no tensor math in this file.

``multistep_2m_plan`` is that wiring.  ``solver_plan`` (below it) is the whole of ``DPM_Solver.sample`` -- orders 1-3, multistep,
singlestep ("DPM-Solver-fast") and singlestep_fixed, the three grids, both solver types, both prediction forms,
denoise_to_zero -- as one record per model evaluation, each followed by one ``mdx_sampler_step_lin_f32`` launch (solver.py).
Two options the reference does not have ride on the same records: the Karras sigma grid (``skip_type="karras"``) and the SDE
form of the first- and second-order multistep update (``sde_eta > 0``: "DPM++ 2M SDE"), whose record carries the noise
coefficient ``cn`` of the ``mdx_sampler_step_lin_noise_f32`` launch.
"""
import numpy as np


class NoiseScheduleVP:
    """dpm_solver.py:14-164, 'discrete' schedule only (the only one sampler.py:72 constructs)."""

    def __init__(self, schedule="discrete", betas=None, alphas_cumprod=None):
        if schedule != "discrete":
            raise NotImplementedError("the reference's sampler only builds NoiseScheduleVP('discrete', alphas_cumprod=...)")
        if betas is not None:
            log_alphas = 0.5 * np.cumsum(np.log(1.0 - np.asarray(betas, np.float64)))
        else:
            assert alphas_cumprod is not None
            log_alphas = 0.5 * np.log(np.asarray(alphas_cumprod, np.float64))
        self.schedule = schedule
        self.total_N = len(log_alphas)
        self.T = 1.0
        self.t_array = np.linspace(0.0, 1.0, self.total_N + 1)[1:]       # t_k = (k + 1) / N
        self.log_alpha_array = log_alphas

    @staticmethod
    def _interp(x, xp, yp):
        """interpolate_fn :1126-1171: piecewise linear through (xp, yp), the outermost segments extended linearly."""
        x = np.asarray(x, np.float64)
        idx = np.clip(np.searchsorted(xp, x, side="left"), 1, len(xp) - 1)
        x0, x1, y0, y1 = xp[idx - 1], xp[idx], yp[idx - 1], yp[idx]
        return y0 + (x - x0) * (y1 - y0) / (x1 - x0)

    def marginal_log_mean_coeff(self, t):
        return self._interp(t, self.t_array, self.log_alpha_array)

    def marginal_alpha(self, t):
        return np.exp(self.marginal_log_mean_coeff(t))

    def marginal_std(self, t):
        return np.sqrt(1.0 - np.exp(2.0 * self.marginal_log_mean_coeff(t)))

    def marginal_lambda(self, t):
        lm = self.marginal_log_mean_coeff(t)
        return lm - 0.5 * np.log(1.0 - np.exp(2.0 * lm))

    def inverse_lambda(self, lamb):
        log_alpha = -0.5 * np.logaddexp(0.0, -2.0 * np.asarray(lamb, np.float64))
        return self._interp(log_alpha, self.log_alpha_array[::-1], self.t_array[::-1])

    def model_input_time(self, t_continuous):
        """model_wrapper.get_model_input_time :256-265: continuous t in [1/N, 1] -> the UNet's (fractional) timestep."""
        return (np.asarray(t_continuous, np.float64) - 1.0 / self.total_N) * 1000.0


def time_uniform_steps(ns, steps, t_start=None, t_end=None):
    """DPM_Solver.get_time_steps(skip_type='time_uniform') :414-415 with sample()'s defaults :1040-1041."""
    t_0 = 1.0 / ns.total_N if t_end is None else t_end
    t_T = ns.T if t_start is None else t_start
    return np.linspace(t_T, t_0, steps + 1)


def multistep_2m_plan(ns, steps, order=2, lower_order_final=True, t_start=None):
    """The S updates of DPM_Solver.sample(method='multistep', order=2, predict_x0=True) :1044-1075 as scalars.
    t_start: DPM_Solver.sample's own option (:958-1041) -- the grid runs from t_start instead of T (img2img).

    Step k (k = 0 .. S-1) evaluates the model at timesteps[k] (x0_k = (x - sigma_k eps) / alpha_k) and moves x from
    timesteps[k] to timesteps[k+1]:
        x_next = A * x + c0 * x0_k + c1 * x0_{k-1}
    first order  (:488-511):  A = sigma_t / sigma_s, c0 = -alpha_t * expm1(-h),                     c1 = 0
    second order (:742-773):  A = sigma_t / sigma_s, c0 = -alpha_t (e^{-h} - 1) (1 + 1 / (2 r0)),   c1 = alpha_t (e^{-h} - 1) / (2 r0)
    with h = lambda_t - lambda_s, r0 = (lambda_s - lambda_{s-1}) / h.  S model evaluations in total (the last
    update's target needs none, :1073-1075)."""
    assert order in (1, 2) and steps >= order
    ts = time_uniform_steps(ns, steps, t_start=t_start)
    lam, alpha, sigma = ns.marginal_lambda(ts), ns.marginal_alpha(ts), ns.marginal_std(ts)
    plan = []
    for k in range(steps):
        step = k + 1                                    # index of the target time in `ts`
        if k == 0:
            step_order = 1                              # init by the lower-order solver (:1050-1056)
        elif lower_order_final and steps < 15:
            step_order = min(order, steps + 1 - step)   # :1060-1063
        else:
            step_order = order
        h = lam[k + 1] - lam[k]
        A = sigma[k + 1] / sigma[k]
        if step_order == 1:
            c0, c1 = -alpha[k + 1] * np.expm1(-h), 0.0
        else:
            r0 = (lam[k] - lam[k - 1]) / h
            phi = alpha[k + 1] * (np.exp(-h) - 1.0)
            c0, c1 = -phi * (1.0 + 0.5 / r0), 0.5 * phi / r0
        plan.append(dict(t=ts[k], t_next=ts[k + 1], t_input=float(ns.model_input_time(ts[k])), alpha=alpha[k],
                         sigma=sigma[k], A=A, c0=c0, c1=c1, order=step_order))
    return plan


# ------------------------------------------------------------------ the whole solver: DPM_Solver.sample(...) as launches
# Every model evaluation of a run is followed by exactly ONE launch of the linear form (mdx_sampler_step_lin_f32)
#     x_out = A * x_base + c0 * m_cur + c1 * h1 + c2 * h2
# m_cur: the model value (data or noise prediction) the launch computes from the UNet output at (x_model, t); h1, h2: model
# values stored by earlier launches; x_base: the latent the update starts from -- in a singlestep update the latent at the
# start of the step, while x_model is the intermediate point x_s1 / x_s2.  The reference's difference terms (D1, D2 and the
# (model_s1 - model_s) brackets) are folded into c0 .. c2 here: each update's formula is evaluated on the unit vectors
# standing for the model values it combines, so what is written below is the reference's formula, not its expansion.
# A coefficient that is exactly 0 means the launch skips the term (and never reads its buffer).
#
# Buffer roles are symbolic.  Latents: "x" (the latent at the start of the step; the run's start and result) and "y" (the
# intermediate point of a singlestep update); a launch may write the buffer it reads (element for element).  Model values:
# three slots "m0", "m1", "m2"; a launch stores m_cur in the slot it does not read.
SKIP_TYPES = ("logSNR", "time_uniform", "time_quadratic", "karras")
VALUE_X0, VALUE_EPS = "x0", "eps"


def check_rho(rho):
    """`rho` of the Karras grid as a finite float > 0."""
    v = float(rho)
    if not (np.isfinite(v) and v > 0.):
        raise ValueError(f"rho must be a finite number > 0, got {rho!r}")
    return v


def get_time_steps(ns, skip_type, t_T, t_0, N, rho=7.):
    """DPM_Solver.get_time_steps :395-422, N + 1 times from t_T down to t_0, float64 (the reference's fp16 casts of the
    logSNR endpoints and of the time_uniform grid are not reproduced, see the module docstring).
    "karras" (not in the reference; Karras et al. 2022, eq. 5, k-diffusion's get_sigmas_karras): with sigma(t) = exp(-lambda(t))
    = sigma_t / alpha_t the points are uniform in sigma^(1 / rho), mapped back to times through inverse_lambda."""
    if skip_type == "karras":
        rho = check_rho(rho)
        s_T, s_0 = np.exp(-ns.marginal_lambda(t_T)) ** (1. / rho), np.exp(-ns.marginal_lambda(t_0)) ** (1. / rho)
        ts = ns.inverse_lambda(-rho * np.log(s_T + (np.arange(N + 1) / N) * (s_0 - s_T)))
        ts[0], ts[-1] = t_T, t_0        # as for logSNR
        return ts
    if skip_type == "logSNR":
        lam = np.linspace(ns.marginal_lambda(t_T), ns.marginal_lambda(t_0), N + 1)
        ts = ns.inverse_lambda(lam)
        ts[0], ts[-1] = t_T, t_0        # the round trip through the interpolation leaves the ends a few ulp off
        return ts
    if skip_type == "time_uniform":
        return np.linspace(t_T, t_0, N + 1)
    if skip_type == "time_quadratic":
        ts = np.linspace(t_T ** 0.5, t_0 ** 0.5, N + 1) ** 2
        ts[0], ts[-1] = t_T, t_0
        return ts
    raise ValueError("Unsupported skip_type {}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic' or 'karras'"
                     .format(skip_type))


def singlestep_orders(steps, order):
    """The order of every outer step of "DPM-Solver-fast" and the number K of outer intervals a logSNR grid gets
    (get_orders_and_timesteps_for_singlestep_solver :454-473)."""
    if order == 3:
        K = steps // 3 + 1
        if steps % 3 == 0:
            orders = [3] * (K - 2) + [2, 1]
        elif steps % 3 == 1:
            orders = [3] * (K - 1) + [1]
        else:
            orders = [3] * (K - 1) + [2]
    elif order == 2:
        if steps % 2 == 0:
            K = steps // 2
            orders = [2] * K
        else:
            K = steps // 2 + 1
            orders = [2] * (K - 1) + [1]
    elif order == 1:
        K = steps       # (:470 sets K = 1, which leaves a logSNR grid of 2 points for `steps` updates: an index error there)
        orders = [1] * steps
    else:
        raise ValueError("'order' must be '1' or '2' or '3'.")
    return orders, K


class _Form:
    """What the two prediction forms differ in: with predict_x0 (DPM-Solver++) x is carried by sigma, the model value by
    alpha and the exponent is -h; in the noise form x is carried by alpha, the model value by sigma, the exponent is +h and
    the constant of the phi functions changes sign."""

    def __init__(self, ns, predict_x0):
        self.ns, self.x0 = ns, predict_x0

    def carry(self, s, t):
        ns = self.ns
        if self.x0:
            return float(ns.marginal_std(t) / ns.marginal_std(s))
        return float(np.exp(ns.marginal_log_mean_coeff(t) - ns.marginal_log_mean_coeff(s)))

    def weight(self, t):
        return float(self.ns.marginal_alpha(t) if self.x0 else self.ns.marginal_std(t))

    def phi_1(self, h):
        return float(np.expm1(-h if self.x0 else h))

    def first(self, s, t, h):
        """dpm_solver_first_update :509-532: (A, coefficient of model_s)."""
        return self.carry(s, t), -self.weight(t) * self.phi_1(h)


_E = np.eye(3)


def _singlestep_second(f, s, s1, t, h, r1, solver_type):
    """singlestep_dpm_solver_second_update :566-612: (A, c) of the launch to s1 and of the launch to t, c over
    (model_s, model_s1)."""
    m_s, m_s1 = _E[0], _E[1]
    to_s1 = (f.carry(s, s1), -f.weight(s1) * f.phi_1(r1 * h) * m_s)
    w, phi_1 = f.weight(t), f.phi_1(h)
    if solver_type == "dpm_solver":
        c = -w * phi_1 * m_s - (0.5 / r1) * w * phi_1 * (m_s1 - m_s)
    elif f.x0:
        c = -w * phi_1 * m_s + (1. / r1) * w * (phi_1 / h + 1.) * (m_s1 - m_s)
    else:
        c = -w * phi_1 * m_s - (1. / r1) * w * (phi_1 / h - 1.) * (m_s1 - m_s)
    return to_s1, (f.carry(s, t), c)


def _singlestep_third(f, s, s1, s2, t, h, r1, r2, solver_type):
    """singlestep_dpm_solver_third_update :658-735: the launches to s1, s2 and t, c over (model_s, model_s1, model_s2)."""
    m_s, m_s1, m_s2 = _E
    sign = 1. if f.x0 else -1.
    phi_11, phi_12, phi_1 = f.phi_1(r1 * h), f.phi_1(r2 * h), f.phi_1(h)
    phi_22 = phi_12 / (r2 * h) + sign
    phi_2 = phi_1 / h + sign
    phi_3 = phi_2 / h - 0.5
    w2, w = f.weight(s2), f.weight(t)
    to_s1 = (f.carry(s, s1), -f.weight(s1) * phi_11 * m_s)
    to_s2 = (f.carry(s, s2), -w2 * phi_12 * m_s + sign * (r2 / r1) * w2 * phi_22 * (m_s1 - m_s))
    if solver_type == "dpm_solver":
        c = -w * phi_1 * m_s + sign * (1. / r2) * w * phi_2 * (m_s2 - m_s)
    else:
        D1_0 = (1. / r1) * (m_s1 - m_s)
        D1_1 = (1. / r2) * (m_s2 - m_s)
        D1 = (r2 * D1_0 - r1 * D1_1) / (r2 - r1)
        D2 = 2. * (D1_1 - D1_0) / (r2 - r1)
        c = -w * phi_1 * m_s + sign * w * phi_2 * D1 - w * phi_3 * D2
    return to_s1, to_s2, (f.carry(s, t), c)


def _multistep(f, lam_prev, s, t, h, step_order, solver_type):
    """multistep_dpm_solver_update :874-895 from s to t: (A, c) with c over (model_prev_0, model_prev_1, model_prev_2), the
    newest first.  lam_prev: lambda at the times of model_prev_0, model_prev_1, model_prev_2 (as many as there are)."""
    p0, p1, p2 = _E
    w, phi_1 = f.weight(t), f.phi_1(h)
    sign = 1. if f.x0 else -1.
    A = f.carry(s, t)
    if step_order == 1:
        return A, -w * phi_1 * p0
    r0 = (lam_prev[0] - lam_prev[1]) / h
    D1_0 = (1. / r0) * (p0 - p1)
    if step_order == 2:         # multistep_dpm_solver_second_update :771-796
        if solver_type == "dpm_solver":
            return A, -w * phi_1 * p0 - 0.5 * w * phi_1 * D1_0
        return A, -w * phi_1 * p0 + sign * w * (phi_1 / h + sign) * D1_0
    r1 = (lam_prev[1] - lam_prev[2]) / h        # multistep_dpm_solver_third_update :822-843 (one form for both solver types)
    D1_1 = (1. / r1) * (p1 - p2)
    D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
    D2 = (1. / (r0 + r1)) * (D1_0 - D1_1)
    return A, -w * phi_1 * p0 + sign * w * (phi_1 / h + sign) * D1 - w * ((phi_1 + sign * h) / h ** 2 - 0.5) * D2


def _multistep_sde(ns, lam_prev, s, t, h, step_order, eta, s_noise):
    """The data-prediction multistep update from s to t as an SDE step (not in the reference; diffusers' "sde-dpmsolver++",
    k-diffusion's sample_dpmpp_2m_sde in its midpoint form): (A, c, cn) with c as _multistep has it and cn the coefficient of
    the step's N(0, 1) draw.  The exact solution of the reverse SDE with the noise injection scaled by eta, the data prediction
    held (order 1) or extrapolated linearly in lambda (order 2):
        A = (sigma_t / sigma_s) e^{-eta h},  phi = expm1(-(1 + eta) h),  cn = s_noise sigma_t sqrt(-expm1(-2 eta h))
    so that A^2 sigma_s^2 + cn^2 = sigma_t^2 (s_noise = 1) and A alpha_s + sum(c) = alpha_t whatever eta is."""
    p0, p1, _ = _E
    alpha_t, sigma_t = float(ns.marginal_alpha(t)), float(ns.marginal_std(t))
    A = sigma_t / float(ns.marginal_std(s)) * float(np.exp(-eta * h))
    phi = float(np.expm1(-(1. + eta) * h))
    cn = s_noise * sigma_t * float(np.sqrt(-np.expm1(-2. * eta * h)))
    if step_order == 1:
        return A, -alpha_t * phi * p0, cn
    r0 = (lam_prev[0] - lam_prev[1]) / h
    return A, -alpha_t * phi * (1. + 0.5 / r0) * p0 + (0.5 * alpha_t * phi / r0) * p1, cn


def check_sde(sde_eta, s_noise, method="multistep", order=2, predict_x0=True, solver_type="dpm_solver"):
    """(sde_eta, s_noise) as finite floats >= 0; sde_eta > 0 only where the SDE update is defined: the data-prediction
    multistep update of order 1 or 2 in its 'dpm_solver' (midpoint) form.  s_noise counts only with sde_eta > 0 (1.0 otherwise)."""
    eta, sn = float(sde_eta), float(s_noise)
    for name, v, given in (("sde_eta", eta, sde_eta), ("s_noise", sn, s_noise)):
        if not (np.isfinite(v) and v >= 0.):
            raise ValueError(f"{name} must be a finite number >= 0, got {given!r}")
    if eta > 0.:
        for bad, why in ((method != "multistep", f"method {method!r} (the SDE update is a multistep update)"),
                         (order == 3, "order 3 (the SDE update is of order 1 or 2)"),
                         (not predict_x0, "predict_x0=False (the SDE update is in data-prediction form)"),
                         (solver_type == "taylor", "solver_type 'taylor' (the SDE update is the midpoint form, 'dpm_solver')")):
            if bad:
                raise ValueError(f"sde_eta > 0 is not defined with {why}")
    return eta, sn if eta > 0. else 1.


def _record(ns, t, value, A, c, base, model, hist, store, out, order, t_next, cn=0.):
    c = [float(v) for v in c] + [0.] * (3 - len(c))
    return dict(t=float(t), t_next=float(t_next), t_input=float(ns.model_input_time(t)), alpha_m=float(ns.marginal_alpha(t)),
                sigma_m=float(ns.marginal_std(t)), value=value, A=float(A), c0=c[0], c1=c[1], c2=c[2], base=base, model=model,
                h1=hist[0] if c[1] != 0. else None, h2=hist[1] if c[2] != 0. else None, store=store, out=out, order=order,
                cn=float(cn))


def solver_plan(ns, steps, order=2, skip_type="time_uniform", method="multistep", solver_type="dpm_solver", predict_x0=True,
                lower_order_final=True, denoise_to_zero=False, t_start=None, t_end=None, rho=7., sde_eta=0., s_noise=1.):
    """DPM_Solver(predict_x0=...).sample(steps, t_start, t_end, order, skip_type, method, lower_order_final, denoise_to_zero,
    solver_type) :958-1123 as one record per MODEL EVALUATION, in order; each evaluation is followed by one launch of
        x_out = A * x_base + c0 * m_cur + c1 * h1 + c2 * h2.
    A record: t, t_input (model_input_time(t)), (alpha_m, sigma_m) at t, value ("x0" | "eps": what m_cur is), A, c0, c1, c2,
    the buffer roles base / model / out ("x" | "y"), h1 / h2 (the slots read, None for a zero coefficient), store (the slot
    m_cur goes to), order (of the update the evaluation belongs to) and t_next (the time of x_out).  The run starts with the
    latent in "x" and ends with the result there.
    multistep: `steps` evaluations, the first order - 1 updates of lower order, the last ones too under 15 steps with
    lower_order_final; the last target gets no evaluation.  singlestep: the DPM-Solver-fast order lists, `steps` evaluations.
    singlestep_fixed: steps // order updates of `order`.  denoise_to_zero: one more evaluation at t_0 whose data prediction
    is the result (A = 0, c0 = 1).
    rho: the exponent of skip_type "karras" (read with that grid only).  sde_eta > 0: every multistep update is the SDE step
    _multistep_sde describes and its record's launch adds cn * z, z ~ N(0, 1) fresh per record; a record also carries cn (0.0
    for a deterministic update, denoise_to_zero's included) and draw, its index in the plan (the counter of its noise).
    sde_eta == 0 takes the deterministic code path: A, c0 .. c2 are then what they have always been."""
    if method == "adaptive":
        raise NotImplementedError("method 'adaptive' is not planned: its step size needs a device-to-host error norm every "
                                  "step, and a plan is made before the first launch")
    if method not in ("multistep", "singlestep", "singlestep_fixed"):
        raise ValueError("Got wrong method {}, need to be 'singlestep' or 'multistep' or 'singlestep_fixed' or 'adaptive'"
                         .format(method))
    if order not in (1, 2, 3) or isinstance(order, bool):
        raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))
    if solver_type not in ("dpm_solver", "taylor"):
        raise ValueError("'solver_type' must be either 'dpm_solver' or 'taylor', got {}".format(solver_type))
    if skip_type not in SKIP_TYPES:
        raise ValueError("Unsupported skip_type {}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic' or 'karras'"
                         .format(skip_type))
    rho = check_rho(rho) if skip_type == "karras" else 7.
    sde_eta, s_noise = check_sde(sde_eta, s_noise, method, order, predict_x0, solver_type)
    need = 1 if method == "singlestep" else order        # (:1065 asserts it for multistep; a fixed-order run needs one update)
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < need:
        raise ValueError("steps must be an int >= {} for method {} of order {}, got {!r}".format(need, method, order, steps))
    steps = int(steps)
    t_0 = 1.0 / ns.total_N if t_end is None else float(t_end)
    t_T = ns.T if t_start is None else float(t_start)
    if not 0. < t_0 < t_T <= ns.T:
        raise ValueError("the run goes from t_start down to t_end: need 0 < t_end < t_start <= {}, got t_start {!r}, t_end {!r}"
                         .format(ns.T, t_T, t_0))
    f = _Form(ns, bool(predict_x0))
    value = VALUE_X0 if predict_x0 else VALUE_EPS
    lam_of = lambda t: float(ns.marginal_lambda(t))
    plan = []
    if method == "multistep":
        ts = get_time_steps(ns, skip_type, t_T, t_0, steps, rho)
        lam = ns.marginal_lambda(ts)
        slots = ["m0", "m1", "m2"]      # slots[0]: where this evaluation's value goes; slots[1], slots[2]: the two before it
        for k in range(steps):
            step = k + 1
            if step < order:
                step_order = step                               # init by the lower-order solvers (:1073-1078)
            elif lower_order_final and steps < 15:
                step_order = min(order, steps + 1 - step)       # :1082-1085
            else:
                step_order = order
            lam_prev, h, cn = [lam[k - j] for j in range(step_order)], lam[k + 1] - lam[k], 0.
            if sde_eta > 0.:
                A, c, cn = _multistep_sde(ns, lam_prev, ts[k], ts[k + 1], h, step_order, sde_eta, s_noise)
            else:
                A, c = _multistep(f, lam_prev, ts[k], ts[k + 1], h, step_order, solver_type)
            plan.append(_record(ns, ts[k], value, A, c, "x", "x", slots[1:], slots[0], "x", step_order, ts[k + 1], cn))
            slots = [slots[2], slots[0], slots[1]]
    else:
        if method == "singlestep":
            orders, K = singlestep_orders(steps, order)
            if skip_type == "logSNR":
                outer = get_time_steps(ns, skip_type, t_T, t_0, K, rho)     # "to reproduce the results in DPM-Solver paper" :474-476
            else:
                outer = get_time_steps(ns, skip_type, t_T, t_0, steps, rho)[np.cumsum([0] + orders)]
        else:
            orders = [order] * (steps // order)
            outer = get_time_steps(ns, skip_type, t_T, t_0, len(orders), rho)
        for i, o in enumerate(orders):
            s, t = float(outer[i]), float(outer[i + 1])
            lam_in = ns.marginal_lambda(get_time_steps(ns, skip_type, s, t, o, rho))    # r1, r2 from the inner grid (:1110-1119)
            lam_s, h = lam_of(s), lam_of(t) - lam_of(s)
            if o == 1:
                A, c0 = f.first(s, t, h)
                plan.append(_record(ns, s, value, A, [c0], "x", "x", [None, None], "m0", "x", 1, t))
                continue
            r1 = float((lam_in[1] - lam_in[0]) / (lam_in[-1] - lam_in[0]))
            s1 = float(ns.inverse_lambda(lam_s + r1 * h))
            if o == 2:
                (A1, c_1), (A, c) = _singlestep_second(f, s, s1, t, h, r1, solver_type)
                plan.append(_record(ns, s, value, A1, [c_1[0]], "x", "x", [None, None], "m0", "y", 2, s1))
                plan.append(_record(ns, s1, value, A, [c[1], c[0]], "x", "y", ["m0", None], "m1", "x", 2, t))
                continue
            r2 = float((lam_in[2] - lam_in[0]) / (lam_in[-1] - lam_in[0]))
            s2 = float(ns.inverse_lambda(lam_s + r2 * h))
            (A1, c_1), (A2, c_2), (A, c) = _singlestep_third(f, s, s1, s2, t, h, r1, r2, solver_type)
            plan.append(_record(ns, s, value, A1, [c_1[0]], "x", "x", [None, None], "m0", "y", 3, s1))
            plan.append(_record(ns, s1, value, A2, [c_2[1], c_2[0]], "x", "y", ["m0", None], "m1", "y", 3, s2))
            plan.append(_record(ns, s2, value, A, [c[2], c[0], c[1]], "x", "y", ["m0", "m1"], "m2", "x", 3, t))
    if denoise_to_zero:             # denoise_to_zero_fn :482-486: the data prediction at t_0, whatever the form of the run
        plan.append(_record(ns, t_0, VALUE_X0, 0., [1.], "x", "x", [None, None], "m0", "x", 1, 0.))
    for i, r in enumerate(plan):
        r["draw"] = i
    return plan
