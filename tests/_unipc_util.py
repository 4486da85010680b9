"""UniPC in float64 numpy, restated from the paper's loop (Zhao et al. 2023, Algorithms 5-7 / the multistep B(h) update):
the model values are kept as arrays and the differences D_j are formed on them, so nothing here shares the folding of
uni_pc.unipc_plan.  Also: the analytic Gaussian-data model whose probability-flow ODE has a closed solution, and numpy runners
for unipc_plan's and solver_plan's records."""
import math

import numpy as np

from minddiffusion_amd.ldm.models.diffusion.dpm_solver.dpm_solver import NoiseScheduleVP, get_time_steps


def sd_schedule():
    return NoiseScheduleVP("discrete", betas=np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000) ** 2)


class GaussianData:
    """Data ~ N(mu, sd^2) per element: eps*(x, t) = sigma (x - alpha mu) / (alpha^2 sd^2 + sigma^2), and the ODE's solution is
    x(t) = alpha mu + sqrt(alpha^2 sd^2 + sigma^2) z with z fixed by the start."""

    def __init__(self, ns, n=64):
        rng = np.random.RandomState(0)
        self.ns = ns
        self.mu = rng.randn(n) * 0.8
        self.sd = 0.3 + rng.rand(n)
        self.x_T = rng.randn(n)

    def eps(self, x, t):
        a, s = float(self.ns.marginal_alpha(t)), float(self.ns.marginal_std(t))
        return s * (x - a * self.mu) / (a * a * self.sd ** 2 + s * s)

    def value(self, x, t, x0):
        """The model value at (x, t): the data prediction, or the noise prediction."""
        e = self.eps(x, t)
        if not x0:
            return e
        return (x - float(self.ns.marginal_std(t)) * e) / float(self.ns.marginal_alpha(t))

    def exact(self, t_T, t_0):
        ns = self.ns
        spread = lambda t: np.sqrt(float(ns.marginal_alpha(t)) ** 2 * self.sd ** 2 + float(ns.marginal_std(t)) ** 2)
        z = (self.x_T - float(ns.marginal_alpha(t_T)) * self.mu) / spread(t_T)
        return float(ns.marginal_alpha(t_0)) * self.mu + spread(t_0) * z


def unipc_loop(ns, value, x, ts, order, variant, predict_x0, lower_order_final=True, corrector=True):
    """Multistep UniPC on the grid ts from x at ts[0]; value(x, t, predict_x0) is the model.  Returns the latent at ts[-1]: the
    last update is predictor only (there is no model value at its target)."""
    N = len(ts) - 1
    lam = [float(ns.marginal_lambda(t)) for t in ts]
    x = np.array(x, np.float64)
    ms = [value(x, ts[0], predict_x0)]
    for k in range(1, N + 1):
        p = min(k, order)
        if lower_order_final:
            p = min(p, N + 1 - k)
        s, t = ts[k - 1], ts[k]
        h = lam[k] - lam[k - 1]
        m_prev = ms[k - 1]
        rks, D1s = [], []
        for j in range(1, p):
            rk = (lam[k - 1 - j] - lam[k - 1]) / h
            rks.append(rk)
            D1s.append((ms[k - 1 - j] - m_prev) / rk)
        rks = np.array(rks + [1.])
        hh = -h if predict_x0 else h
        h_phi_1 = math.expm1(hh)
        B_h = hh if variant == "bh1" else math.expm1(hh)
        R, b = [], []
        h_phi_k, factorial = h_phi_1 / hh - 1., 1
        for i in range(1, p + 1):
            R.append(rks ** (i - 1))
            b.append(h_phi_k * factorial / B_h)
            factorial *= i + 1
            h_phi_k = h_phi_k / hh - 1. / factorial
        R, b = np.stack(R), np.array(b)
        if predict_x0:
            w = float(ns.marginal_alpha(t))
            x_ = float(ns.marginal_std(t)) / float(ns.marginal_std(s)) * x - w * h_phi_1 * m_prev
        else:
            w = float(ns.marginal_std(t))
            x_ = math.exp(float(ns.marginal_log_mean_coeff(t)) - float(ns.marginal_log_mean_coeff(s))) * x - w * h_phi_1 * m_prev
        rhos_p = [] if p == 1 else [0.5] if p == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])
        x_pred = x_ - w * B_h * sum((rho * D for rho, D in zip(rhos_p, D1s)), np.zeros_like(x))
        if k == N:
            return x_pred
        m_t = value(x_pred, t, predict_x0)
        ms.append(m_t)
        if corrector:
            rhos_c = [0.5] if p == 1 else np.linalg.solve(R, b)
            x = x_ - w * B_h * (sum((rho * D for rho, D in zip(rhos_c[:-1], D1s)), np.zeros_like(x)) + rhos_c[-1] * (m_t - m_prev))
        else:
            x = x_pred
    raise AssertionError("unreachable")


def run_unipc_plan(plan, value, x):
    """unipc_plan's records on numpy arrays, as the step launch runs them."""
    bufs = {"x": np.array(x, np.float64)}
    for r in plan:
        val = value(bufs[r["model"]], r["t"], r["value"] == "x0")
        hist = [None if r[k] is None else bufs[r[k]] for k in ("h1", "h2", "h3")]
        if "Ac" in r:
            xc = r["Ac"] * bufs[r["base"]] + r["d0"] * val
            for d, h in zip((r["d1"], r["d2"], r["d3"]), hist):
                if d != 0.:
                    xc = xc + d * h
        else:
            xc = bufs[r["model"]].copy()
        xp = r["Ap"] * xc + r["e0"] * val
        for e, h in zip((r["e1"], r["e2"]), hist):
            if e != 0.:
                xp = xp + e * h
        bufs[r["store"]], bufs[r["corr_out"]], bufs[r["out"]] = val, xc, xp
    return bufs["x"]


def run_solver_plan(plan, value, x):
    """solver_plan's records on numpy arrays."""
    bufs = {"x": np.array(x, np.float64)}
    for r in plan:
        val = value(bufs[r["model"]], r["t"], r["value"] == "x0")
        out = r["A"] * bufs[r["base"]] + r["c0"] * val
        for c, k in ((r["c1"], r["h1"]), (r["c2"], r["h2"])):
            if c != 0.:
                out = out + c * bufs[k]
        bufs[r["store"]], bufs[r["out"]] = val, out
    return bufs["x"]


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def grid(ns, skip_type, steps, t_T=1., t_0=1e-3, rho=7.):
    return get_time_steps(ns, skip_type, t_T, t_0, steps, rho)
