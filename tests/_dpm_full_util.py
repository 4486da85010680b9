"""The whole DPM-Solver as tensor updates, for tests/test_dpm_solver_gpu.py: a torch-CPU restatement (fp32 images, float64
schedule) written from the solver's formulas on top of oracle.dpm_solver's NoiseScheduleVP / model_wrapper and the oracle UNet,
the way oracle/dpm_solver.py restates the wired multistep order-2 path -- oracle/ itself is untouched.

It keeps the model values as tensors and forms the differences D1, D2 and (m_u - m_s) on them at every update, so it is an
independent check of the product's plan, which folds those differences into three scalar coefficients on the host.

Notation, for an update from s to t with h = lambda_t - lambda_s.  Data-prediction form (DPM-Solver++): x is carried by
sigma_t / sigma_s, the model value m weighs alpha_t, E = expm1(-h).  Noise form: x is carried by alpha_t / alpha_s, m weighs
sigma_t, E = expm1(h), and the constants of the higher phi functions change sign (sgn = -1):
    order 1:        x_t = carry x - w E m_s
    singlestep 2:   u = s + r1 h;  x_u by order 1;  x_t = order 1 - (w E / (2 r1)) (m_u - m_s)
                    'taylor':      x_t = order 1 + sgn (w (E / h + sgn) / r1) (m_u - m_s)
    singlestep 3:   u = s + r1 h, v = s + r2 h;  x_u by order 1;
                    x_v = order 1 to v + sgn (r2 / r1) w_v (expm1(-+r2 h) / (r2 h) + sgn) (m_u - m_s);
                    x_t = order 1 + sgn (w phi_2 / r2) (m_v - m_s),  phi_2 = E / h + sgn
                    'taylor':  D1_0 = (m_u - m_s) / r1, D1_1 = (m_v - m_s) / r2, D1 = (r2 D1_0 - r1 D1_1) / (r2 - r1),
                               D2 = 2 (D1_1 - D1_0) / (r2 - r1);  x_t = order 1 + sgn w phi_2 D1 - w (phi_2 / h - 1/2) D2
    multistep 2:    r0 = h_0 / h, D1_0 = (m_0 - m_1) / r0;  x_t = order 1 - (w E / 2) D1_0;  'taylor': + sgn w (E / h + sgn) D1_0
    multistep 3:    r1 = h_1 / h, D1_1 = (m_1 - m_2) / r1, D1 = D1_0 + r0 / (r0 + r1) (D1_0 - D1_1), D2 = (D1_0 - D1_1) / (r0 + r1);
                    x_t = order 1 + sgn w (E / h + sgn) D1 - w ((E + sgn h) / h^2 - 1/2) D2
Dynamic thresholding of a data prediction: s = a + (b - a) 0.995 between the order statistics k = int((N - 1) 0.995) and k + 1
of |x0| per sample, s = max(s, max_val), x0 = clamp(x0, -s, s) / s.
"""
import torch

from oracle import dpm_solver as OD


class FullSolver:
    def __init__(self, model_fn, ns, predict_x0=True, thresholding=False, max_val=1.0):
        self.model, self.ns = model_fn, ns
        self.predict_x0, self.thresholding, self.max_val = predict_x0, thresholding, max_val
        self.nfe = 0
        self.raw_s = []          # per data-prediction evaluation: [B] thresholds before max(., max_val)

    # ---- schedule scalars at a scalar time (float64 python floats)
    def _at(self, fn, t):
        return float(fn(torch.tensor([t], dtype=torch.float64))[0])

    def lam(self, t):
        return self._at(self.ns.marginal_lambda, t)

    def alpha(self, t):
        return self._at(self.ns.marginal_alpha, t)

    def sigma(self, t):
        return self._at(self.ns.marginal_std, t)

    def t_of_lambda(self, lam):
        return self._at(self.ns.inverse_lambda, lam)

    # ---- model values
    def data_prediction(self, x, t):
        self.nfe += 1
        noise = self.model(x, torch.full((x.shape[0],), t, dtype=torch.float64))
        x0 = (x - self.sigma(t) * noise) / self.alpha(t)
        return self._threshold(x0)

    def _threshold(self, x0):
        if not self.thresholding:
            return x0
        srt = torch.sort(x0.abs().reshape(x0.shape[0], -1), dim=1).values
        k = int((srt.shape[1] - 1) * 0.995)
        s = srt[:, k] + (srt[:, k + 1] - srt[:, k]) * 0.995
        self.raw_s.append(s.clone())
        s = torch.clamp(s, min=self.max_val).reshape(-1, 1, 1, 1)
        return torch.maximum(torch.minimum(x0, s), -s) / s

    def value(self, x, t):
        if self.predict_x0:
            return self.data_prediction(x, t)
        self.nfe += 1
        return self.model(x, torch.full((x.shape[0],), t, dtype=torch.float64))

    # ---- the pieces of an update from s to t
    def _carry_w(self, s, t):
        if self.predict_x0:
            return self.sigma(t) / self.sigma(s), self.alpha(t)
        return self.alpha(t) / self.alpha(s), self.sigma(t)

    def _E(self, h):
        return float(torch.expm1(torch.tensor(-h if self.predict_x0 else h, dtype=torch.float64)))

    @property
    def sgn(self):
        return 1.0 if self.predict_x0 else -1.0

    def first(self, x, s, t, m_s):
        carry, w = self._carry_w(s, t)
        return carry * x - (w * self._E(self.lam(t) - self.lam(s))) * m_s

    def singlestep(self, x, s, t, order, r1, r2, taylor):
        m_s = self.value(x, s)
        if order == 1:
            return self.first(x, s, t, m_s)
        h, sgn = self.lam(t) - self.lam(s), self.sgn
        _, w = self._carry_w(s, t)
        E = self._E(h)
        u = self.t_of_lambda(self.lam(s) + r1 * h)
        m_u = self.value(self.first(x, s, u, m_s), u)
        base = self.first(x, s, t, m_s)
        if order == 2:
            if taylor:
                return base + (sgn * w * (E / h + sgn) / r1) * (m_u - m_s)
            return base - (w * E / (2.0 * r1)) * (m_u - m_s)
        v = self.t_of_lambda(self.lam(s) + r2 * h)
        _, w_v = self._carry_w(s, v)
        x_v = self.first(x, s, v, m_s) + (sgn * (r2 / r1) * w_v * (self._E(r2 * h) / (r2 * h) + sgn)) * (m_u - m_s)
        m_v = self.value(x_v, v)
        phi_2 = E / h + sgn
        if not taylor:
            return base + (sgn * w * phi_2 / r2) * (m_v - m_s)
        D1_0, D1_1 = (m_u - m_s) / r1, (m_v - m_s) / r2
        D1 = (r2 * D1_0 - r1 * D1_1) / (r2 - r1)
        D2 = 2.0 * (D1_1 - D1_0) / (r2 - r1)
        return base + (sgn * w * phi_2) * D1 - (w * (phi_2 / h - 0.5)) * D2

    def multistep(self, x, ms, ts, t, order, taylor):
        """ms / ts: the model values and their times, oldest first; the update starts at ts[-1]."""
        s = ts[-1]
        base = self.first(x, s, t, ms[-1])
        if order == 1:
            return base
        h, sgn = self.lam(t) - self.lam(s), self.sgn
        _, w = self._carry_w(s, t)
        E = self._E(h)
        r0 = (self.lam(ts[-1]) - self.lam(ts[-2])) / h
        D1_0 = (ms[-1] - ms[-2]) / r0
        if order == 2:
            if taylor:
                return base + (sgn * w * (E / h + sgn)) * D1_0
            return base - (0.5 * w * E) * D1_0
        r1 = (self.lam(ts[-2]) - self.lam(ts[-3])) / h
        D1_1 = (ms[-2] - ms[-3]) / r1
        D1 = D1_0 + (r0 / (r0 + r1)) * (D1_0 - D1_1)
        D2 = (D1_0 - D1_1) / (r0 + r1)
        return base + (sgn * w * (E / h + sgn)) * D1 - (w * ((E + sgn * h) / h ** 2 - 0.5)) * D2

    # ---- grids and the run
    def grid(self, skip_type, t_T, t_0, n):
        if skip_type == "logSNR":
            lam = torch.linspace(self.lam(t_T), self.lam(t_0), n + 1, dtype=torch.float64)
            return [float(v) for v in self.ns.inverse_lambda(lam)]
        if skip_type == "time_uniform":
            return [float(v) for v in torch.linspace(t_T, t_0, n + 1, dtype=torch.float64)]
        assert skip_type == "time_quadratic"
        return [float(v) for v in torch.linspace(t_T ** 0.5, t_0 ** 0.5, n + 1, dtype=torch.float64) ** 2]

    @staticmethod
    def fast_orders(steps, order):
        if order == 3:
            K = steps // 3 + 1
            return {0: [3] * (K - 2) + [2, 1], 1: [3] * (K - 1) + [1], 2: [3] * (K - 1) + [2]}[steps % 3]
        if order == 2:
            return [2] * (steps // 2) + [1] * (steps % 2)
        return [1] * steps

    def sample(self, x, steps, order, skip_type, method, solver_type="dpm_solver", lower_order_final=True,
               denoise_to_zero=False, t_start=None, t_end=None):
        t_0 = 1.0 / self.ns.total_N if t_end is None else t_end
        t_T = self.ns.T if t_start is None else t_start
        taylor = solver_type == "taylor"
        if method == "multistep":
            ts = self.grid(skip_type, t_T, t_0, steps)
            ms, tp = [self.value(x, ts[0])], [ts[0]]
            for step in range(1, steps + 1):
                if step < order:
                    o = step
                elif lower_order_final and steps < 15:
                    o = min(order, steps + 1 - step)
                else:
                    o = order
                x = self.multistep(x, ms, tp, ts[step], o, taylor)
                if step < steps:
                    ms, tp = (ms + [self.value(x, ts[step])])[-3:], (tp + [ts[step]])[-3:]
        else:
            if method == "singlestep":
                orders = self.fast_orders(steps, order)
                if skip_type == "logSNR":
                    outer = self.grid(skip_type, t_T, t_0, len(orders))
                else:
                    fine, outer, at = self.grid(skip_type, t_T, t_0, steps), [], 0
                    for o in [0] + orders:
                        at += o
                        outer.append(fine[at])
            else:
                orders = [order] * (steps // order)
                outer = self.grid(skip_type, t_T, t_0, len(orders))
            for i, o in enumerate(orders):
                s, t = outer[i], outer[i + 1]
                lam_in = [self.lam(v) for v in self.grid(skip_type, s, t, o)]
                span = lam_in[-1] - lam_in[0]
                r1 = (lam_in[1] - lam_in[0]) / span if o >= 2 else None
                r2 = (lam_in[2] - lam_in[0]) / span if o >= 3 else None
                x = self.singlestep(x, s, t, o, r1, r2, taylor)
        if denoise_to_zero:
            x = self.data_prediction(x, t_0)
        return x


def sample(model, S, batch_size, shape, conditioning, x_T, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
           order=2, skip_type="time_uniform", method="multistep", solver_type="dpm_solver", predict_x0=True, thresholding=False,
           max_val=1.0, denoise_to_zero=False, lower_order_final=True, t_start=None, t_end=None):
    """oracle.dpm_solver.sample with the whole solver's options; returns (samples, solver)."""
    img = torch.as_tensor(x_T, dtype=torch.float32)
    assert tuple(img.shape) == (batch_size,) + tuple(shape)
    cond = torch.as_tensor(conditioning, dtype=torch.float32)
    uc = None if unconditional_conditioning is None else torch.as_tensor(unconditional_conditioning, dtype=torch.float32)
    ns = OD.NoiseScheduleVP("discrete", alphas_cumprod=model.alphas_cumprod)
    model_fn = OD.model_wrapper(lambda x, t, c: model.apply_model(x, t, c), ns, cond, uc, float(unconditional_guidance_scale))
    solver = FullSolver(model_fn, ns, predict_x0, thresholding, max_val)
    x = solver.sample(img, S, order, skip_type, method, solver_type, lower_order_final, denoise_to_zero, t_start, t_end)
    return x, solver
