"""The Karras grid and the SDE form of the multistep DPM-Solver++ update as tensor updates, for tests/test_dpm_sde_gpu.py: a
torch-CPU restatement on top of tests/_dpm_full_util.py (whose FullSolver it extends; that file and oracle/ are untouched).

Neither option is in the reference.  The SDE update is written here the way k-diffusion's sample_dpmpp_2m_sde (midpoint) states
it -- in the variance-exploding variables xh = x / alpha, sh = sigma / alpha = exp(-lambda), with the model values kept as
tensors -- and mapped back by alpha_t, so it is an independent check of the product's plan, which folds everything into the
scalars (A, c0, c1, cn) on the host.  From s to t, h = lambda_t - lambda_s, eta_h = eta h, r = h_last / h:
    xh_t = (sh_t / sh_s) exp(-eta_h) xh_s + (-expm1(-h - eta_h)) m_s                        order 1
           + 0.5 (-expm1(-h - eta_h)) (1 / r) (m_s - m_prev)                                 order 2
           + z sh_t sqrt(-expm1(-2 eta_h)) s_noise,        z ~ N(0, 1), one tensor per update (step_noises[k])
    x_t = alpha_t xh_t
The grid: sh_i = (sh_T^(1/rho) + (i / N) (sh_0^(1/rho) - sh_T^(1/rho)))^rho, t_i = inverse_lambda(-log sh_i)
(k-diffusion's get_sigmas_karras on this schedule's sigma_max / sigma_min)."""
import math

import torch

import _dpm_full_util as F
from oracle import dpm_solver as OD


class SdeSolver(F.FullSolver):
    def __init__(self, model_fn, ns, thresholding=False, max_val=1.0, rho=7.0, sde_eta=0.0, s_noise=1.0, step_noises=None):
        super().__init__(model_fn, ns, True, thresholding, max_val)
        self.rho, self.eta, self.s_noise = rho, sde_eta, s_noise
        self.step_noises = step_noises
        self.updates = 0

    def grid(self, skip_type, t_T, t_0, n):
        if skip_type != "karras":
            return super().grid(skip_type, t_T, t_0, n)
        a, b = math.exp(-self.lam(t_T)) ** (1.0 / self.rho), math.exp(-self.lam(t_0)) ** (1.0 / self.rho)
        ts = [self.t_of_lambda(-math.log((a + (i / n) * (b - a)) ** self.rho)) for i in range(n + 1)]
        ts[0], ts[-1] = t_T, t_0
        return ts

    def multistep(self, x, ms, ts, t, order, taylor):
        k = self.updates
        self.updates += 1
        if self.eta == 0.0:
            return super().multistep(x, ms, ts, t, order, taylor)
        assert order in (1, 2) and not taylor
        s = ts[-1]
        h = self.lam(t) - self.lam(s)
        eta_h = self.eta * h
        sh_s, sh_t = math.exp(-self.lam(s)), math.exp(-self.lam(t))
        xh = x / self.alpha(s)
        xh = (sh_t / sh_s * math.exp(-eta_h)) * xh + (-math.expm1(-h - eta_h)) * ms[-1]
        if order == 2:
            r = (self.lam(ts[-1]) - self.lam(ts[-2])) / h
            xh = xh + (0.5 * (-math.expm1(-h - eta_h)) / r) * (ms[-1] - ms[-2])
        z = torch.as_tensor(self.step_noises[k], dtype=torch.float32)
        xh = xh + (sh_t * math.sqrt(-math.expm1(-2.0 * eta_h)) * self.s_noise) * z
        return self.alpha(t) * xh


def sample(model, S, batch_size, shape, conditioning, x_T, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
           order=2, skip_type="time_uniform", thresholding=False, max_val=1.0, denoise_to_zero=False, lower_order_final=True,
           t_start=None, t_end=None, rho=7.0, sde_eta=0.0, s_noise=1.0, step_noises=None):
    """_dpm_full_util.sample for the multistep data-prediction solver with the Karras grid and the SDE update; returns
    (samples, solver)."""
    img = torch.as_tensor(x_T, dtype=torch.float32)
    assert tuple(img.shape) == (batch_size,) + tuple(shape)
    cond = torch.as_tensor(conditioning, dtype=torch.float32)
    uc = None if unconditional_conditioning is None else torch.as_tensor(unconditional_conditioning, dtype=torch.float32)
    ns = OD.NoiseScheduleVP("discrete", alphas_cumprod=model.alphas_cumprod)
    model_fn = OD.model_wrapper(lambda x, t, c: model.apply_model(x, t, c), ns, cond, uc, float(unconditional_guidance_scale))
    solver = SdeSolver(model_fn, ns, thresholding, max_val, rho, sde_eta, s_noise, step_noises)
    x = solver.sample(img, S, order, skip_type, "multistep", "dpm_solver", lower_order_final, denoise_to_zero, t_start, t_end)
    return x, solver
