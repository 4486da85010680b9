"""Host-side math of UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion
Models"), the multistep form with the B(h) variants bh1 / bh2: float64 numpy on a few scalars per step, no tensor math.

``unipc_plan`` is one record per MODEL EVALUATION, as dpm_solver.solver_plan's are, each followed by ONE launch of
``mdx_sampler_step_pc_f32`` (dpm_solver/solver.run_solver_plan).  On the grid t_0 > ... > t_N the model is evaluated on the
PREDICTED latents only, m_i = model(x~_i, t_i); the update k, from s = t_{k-1} to t = t_k with h = lambda_t - lambda_s, has order
p = min(k, order) (with lower_order_final also at most N + 1 - k) and, with carry and weight w as dpm_solver._Form has them,
    hh = -h (data prediction) | +h (noise prediction),  h phi_1 = expm1(hh),  B = hh (bh1) | expm1(hh) (bh2)
    r_j = (lambda_{k-1-j} - lambda_{k-1}) / h  for j = 1 .. p - 1,  r_p = 1,   D_j = (m_{k-1-j} - m_{k-1}) / r_j
    R_i = r^(i-1),  b_i = g_i i! / B  with  g_1 = h phi_1 / hh - 1,  g_{i+1} = g_i / hh - 1 / (i+1)!       (i = 1 .. p)
    x_  = carry x_{k-1} - w h phi_1 m_{k-1}
    predictor   x~_k = x_ - w B sum_{j<p} rho^p_j D_j                        rho^p solves the leading (p-1) x (p-1) system ([0.5] at p = 2)
    corrector   x_k  = x_ - w B (sum_{j<p} rho^c_j D_j + rho^c_p (m_k - m_{k-1}))    rho^c solves the p x p system ([0.5] at p = 1)
The corrector of update k needs m_k, which the predictor of update k + 1 needs anyway: record i holds the corrector of update i
over (m_i, m_{i-1}, m_{i-2}, m_{i-3}) and the predictor of update i + 1 over (m_i, m_{i-1}, m_{i-2}), the differences folded
into the coefficients (each formula is evaluated on unit vectors standing for the model values, as solver_plan does it).
"""
import numpy as np

from ..dpm_solver.dpm_solver import SKIP_TYPES, VALUE_EPS, VALUE_X0, _Form, check_rho, get_time_steps

VARIANTS = ("bh1", "bh2")
_E = np.eye(4)      # m_k, m_{k-1}, m_{k-2}, m_{k-3} of an update to t_k


def update_forms(f, lam, ts, k, p, variant):
    """Update k of order p on the grid (ts, lam): (carry, predictor, corrector) with both forms over (m_k, m_{k-1}, m_{k-2},
    m_{k-3}) -- the predictor's first entry is 0."""
    h = lam[k] - lam[k - 1]
    hh = -h if f.x0 else h
    h_phi_1 = float(np.expm1(hh))
    B = hh if variant == "bh1" else h_phi_1
    r = np.array([(lam[k - 1 - j] - lam[k - 1]) / h for j in range(1, p)] + [1.])
    D = [(_E[1 + j] - _E[1]) / r[j - 1] for j in range(1, p)]
    R = np.stack([r ** i for i in range(p)])
    b, g, fact = [], h_phi_1 / hh - 1., 1.
    for i in range(1, p + 1):
        b.append(g * fact / B)
        fact *= i + 1
        g = g / hh - 1. / fact
    b = np.array(b)
    rho_p = [] if p == 1 else [0.5] if p == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])
    rho_c = [0.5] if p == 1 else np.linalg.solve(R, b)
    w = f.weight(ts[k])
    x_ = -w * h_phi_1 * _E[1]
    pred = x_ - w * B * sum((rho_p[j] * D[j] for j in range(p - 1)), np.zeros(4))
    corr = x_ - w * B * (sum((rho_c[j] * D[j] for j in range(p - 1)), np.zeros(4)) + rho_c[-1] * (_E[0] - _E[1]))
    return f.carry(ts[k - 1], ts[k]), pred, corr


def unipc_plan(ns, steps, order=3, variant="bh2", predict_x0=True, lower_order_final=True, corrector=True,
               skip_type="time_uniform", rho=7., t_start=None, t_end=None, denoise_to_zero=False, method="multistep"):
    """The multistep UniPC run of `steps` model evaluations from t_start (None: T) down to t_end (None: 1 / N) as records, in
    order.  Record i: t, t_input, (alpha_m, sigma_m) at t_i, value ("x0" | "eps": what the model value is); Ac, d0, d1, d2, d3:
    the corrector of update i over the launch's (val, h1, h2, h3) -- the keys are ABSENT in record 0, in every record with
    corrector=False and in denoise_to_zero's; Ap, e0, e1, e2: the predictor of update i + 1 over (val, h1, h2), based on the
    corrected latent; order / corr_order: the orders of the two (corr_order 0: none); t_next: t_{i+1}.  Buffer roles, symbolic as solver_plan's: the
    latents "x" (model: the model input, the run's start and result; out: the predicted latent goes back there) and "c" (base /
    corr_out: the corrected latent); the model-value slots "m0" .. "m3" rotate by reference -- store: where this value goes;
    h1, h2, h3: the three values before it, None where neither form has a coefficient.
    The last update has no evaluation at its target, so it is predictor only and its output is the result.  denoise_to_zero:
    one more record at t_N with no corrector, Ap = 0, e0 = 1 and value "x0"."""
    if method != "multistep":
        raise ValueError(f"UniPC: only method 'multistep' is implemented, got {method!r}")
    if order not in (1, 2, 3) or isinstance(order, bool):
        raise ValueError(f"UniPC: order must be 1, 2 or 3, got {order!r}")
    if variant not in VARIANTS:
        raise ValueError(f"UniPC: variant must be 'bh1' or 'bh2', got {variant!r}")
    if skip_type not in SKIP_TYPES:
        raise ValueError("Unsupported skip_type {}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic' or 'karras'"
                         .format(skip_type))
    rho = check_rho(rho) if skip_type == "karras" else 7.
    if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or steps < order:
        raise ValueError(f"UniPC: steps must be an int >= order ({order}), got {steps!r}")
    steps = int(steps)
    t_0 = 1.0 / ns.total_N if t_end is None else float(t_end)
    t_T = ns.T if t_start is None else float(t_start)
    if not 0. < t_0 < t_T <= ns.T:
        raise ValueError("the run goes from t_start down to t_end: need 0 < t_end < t_start <= {}, got t_start {!r}, t_end {!r}"
                         .format(ns.T, t_T, t_0))
    f = _Form(ns, bool(predict_x0))
    value = VALUE_X0 if predict_x0 else VALUE_EPS
    ts = get_time_steps(ns, skip_type, t_T, t_0, steps, rho)
    lam = ns.marginal_lambda(ts)

    def order_of(k):
        p = min(k, order)
        return min(p, steps + 1 - k) if lower_order_final else p

    def record(t, value, corr, corr_order, pred, pred_order, slots, t_next):
        d = (0.,) * 5 if corr is None else corr
        hist = [slots[1 + j] if d[2 + j] != 0. or (j < 2 and pred[2 + j] != 0.) else None for j in range(3)]
        r = dict(t=float(t), t_next=float(t_next), t_input=float(ns.model_input_time(t)), alpha_m=float(ns.marginal_alpha(t)),
                 sigma_m=float(ns.marginal_std(t)), value=value, order=pred_order, corr_order=corr_order, base="c", model="x",
                 corr_out="c", out="x", h1=hist[0], h2=hist[1], h3=hist[2], store=slots[0])
        r.update(zip(("Ap", "e0", "e1", "e2"), pred))
        if corr is not None:
            r.update(zip(("Ac", "d0", "d1", "d2", "d3"), corr))
        return r

    plan, slots = [], ["m0", "m1", "m2", "m3"]
    for i in range(steps):
        corr, corr_order = None, 0
        if corrector and i > 0:
            corr_order = order_of(i)
            A, _, c = update_forms(f, lam, ts, i, corr_order, variant)
            corr = (float(A),) + tuple(float(v) for v in c)
        A, p, _ = update_forms(f, lam, ts, i + 1, order_of(i + 1), variant)
        pred = (float(A),) + tuple(float(v) for v in p[1:])
        plan.append(record(ts[i], value, corr, corr_order, pred, order_of(i + 1), slots, ts[i + 1]))
        slots = [slots[3], slots[0], slots[1], slots[2]]
    if denoise_to_zero:
        plan.append(record(t_0, VALUE_X0, None, 0, (0., 1., 0., 0.), 1, slots, 0.))
    return plan
