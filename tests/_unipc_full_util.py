"""Multistep UniPC as tensor updates on the oracle UNet, for tests/test_unipc_sampling_gpu.py: a torch-CPU restatement (fp32
images, float64 schedule) of the paper's update on top of tests/_dpm_full_util.FullSolver's schedule scalars, model values and
thresholding -- oracle/ itself is untouched.  The model values are kept as tensors and the differences D_j are formed on them at
every update, so it is an independent check of uni_pc.unipc_plan, which folds them into scalars on the host.

Update from s = t_{k-1} to t = t_k, h = lambda_t - lambda_s, order p, hh = -h (data prediction) | h (noise prediction):
    r_j = (lambda_{k-1-j} - lambda_{k-1}) / h, D_j = (m_{k-1-j} - m_{k-1}) / r_j  (j < p),  r_p = 1
    R_i = r^(i-1), b_i = g_i i! / B, g_1 = expm1(hh) / hh - 1, g_{i+1} = g_i / hh - 1 / (i+1)!,  B = hh (bh1) | expm1(hh) (bh2)
    x_ = order-1 update;  predictor x_ - w B sum rho^p_j D_j;  corrector x_ - w B (sum rho^c_j D_j + rho^c_p (m_k - m_{k-1}))
The model is evaluated on the predicted latents only; the last update is predictor only."""
import math

import numpy as np
import torch

import _dpm_full_util as F
from oracle import dpm_solver as OD


class UniPCFull(F.FullSolver):
    def grid(self, skip_type, t_T, t_0, n, rho=7.):
        if skip_type != "karras":
            return super().grid(skip_type, t_T, t_0, n)
        s_T, s_0 = math.exp(-self.lam(t_T)) ** (1. / rho), math.exp(-self.lam(t_0)) ** (1. / rho)
        sig = s_T + torch.arange(n + 1, dtype=torch.float64) / n * (s_0 - s_T)
        ts = [float(v) for v in self.ns.inverse_lambda(-rho * torch.log(sig))]
        ts[0], ts[-1] = t_T, t_0
        return ts

    def sample_unipc(self, x, steps, order=3, variant="bh2", skip_type="time_uniform", lower_order_final=True, corrector=True,
                     denoise_to_zero=False, t_start=None, t_end=None, rho=7.):
        t_0 = 1.0 / self.ns.total_N if t_end is None else t_end
        t_T = self.ns.T if t_start is None else t_start
        ts = self.grid(skip_type, t_T, t_0, steps, rho) if skip_type == "karras" else self.grid(skip_type, t_T, t_0, steps)
        lam = [self.lam(t) for t in ts]
        ms = [self.value(x, ts[0])]
        for k in range(1, steps + 1):
            p = min(k, order)
            if lower_order_final:
                p = min(p, steps + 1 - k)
            s, t, h, m_prev = ts[k - 1], ts[k], lam[k] - lam[k - 1], ms[k - 1]
            rks = [(lam[k - 1 - j] - lam[k - 1]) / h for j in range(1, p)]
            D1s = [(ms[k - 1 - j] - m_prev) / rks[j - 1] for j in range(1, p)]
            rks = np.array(rks + [1.])
            hh = -h if self.predict_x0 else h
            B_h = hh if variant == "bh1" else math.expm1(hh)
            R, b, g, fact = [], [], math.expm1(hh) / hh - 1., 1
            for i in range(1, p + 1):
                R.append(rks ** (i - 1))
                b.append(g * fact / B_h)
                fact *= i + 1
                g = g / hh - 1. / fact
            R, b = np.stack(R), np.array(b)
            _, w = self._carry_w(s, t)
            x_ = self.first(x, s, t, m_prev)
            rhos_p = [] if p == 1 else [0.5] if p == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])
            x_pred = x_
            for rho_j, D in zip(rhos_p, D1s):
                x_pred = x_pred - (w * B_h * float(rho_j)) * D
            if k == steps:
                x = x_pred
                break
            m_t = self.value(x_pred, t)
            ms.append(m_t)
            if corrector:
                rhos_c = [0.5] if p == 1 else np.linalg.solve(R, b)
                x = x_ - (w * B_h * float(rhos_c[-1])) * (m_t - m_prev)
                for rho_j, D in zip(rhos_c[:-1], D1s):
                    x = x - (w * B_h * float(rho_j)) * D
            else:
                x = x_pred
        if denoise_to_zero:
            x = self.data_prediction(x, t_0)
        return x


def sample(model, S, batch_size, shape, conditioning, x_T, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
           predict_x0=True, thresholding=False, max_val=1.0, apply=None, **opts):
    """The restatement on the oracle model with classifier-free guidance; returns (samples, solver).  apply: apply_model(x, t, c)
    in the oracle model's place (hybrid conditioning)."""
    img = torch.as_tensor(x_T, dtype=torch.float32)
    assert tuple(img.shape) == (batch_size,) + tuple(shape)
    cond = torch.as_tensor(conditioning, dtype=torch.float32)
    uc = None if unconditional_conditioning is None else torch.as_tensor(unconditional_conditioning, dtype=torch.float32)
    ns = OD.NoiseScheduleVP("discrete", alphas_cumprod=model.alphas_cumprod)
    model_fn = OD.model_wrapper(apply or (lambda x, t, c: model.apply_model(x, t, c)), ns, cond, uc,
                                float(unconditional_guidance_scale))
    solver = UniPCFull(model_fn, ns, predict_x0, thresholding, max_val)
    return solver.sample_unipc(img, S, **opts), solver
