"""TEST INFRASTRUCTURE — stateful, line-for-line restatements of [ext] diffusers 0.18.0 EulerDiscreteScheduler (s_churn 0) and
LMSDiscreteScheduler (`__init__`, `init_noise_sigma`, `scale_model_input`, `set_timesteps`, `step`, `get_lms_coefficient` with
its scipy.integrate.quad call), kept apart from the table forms of lgd_amd.scheduler so that the two can be checked against
each other.  Restated from the published classes: no diffusers class has met these restatements.

The classes keep `sigmas` as a torch tensor, float32 after `.astype(np.float32)`.  `dtype` selects the arithmetic that starts
from those values: float32 is what the pipeline computes (the golden of tools/make_golden_sigma.py), float64 widens the same
fp32 sigmas and pins the table forms to ~1e-12.  In `get_lms_coefficient` the integrand is evaluated on elements of that
tensor, so under float32 quad integrates an fp32-rounded polynomial: ~1e-7 relative in the coefficients, which is why the
closed form of lgd_amd.scheduler.LMSDiscreteScheduler is compared under float64."""
import numpy as np
import torch
from scipy import integrate


class _Out:
    def __init__(self, prev_sample, pred_original_sample=None):
        self.prev_sample = prev_sample
        self.pred_original_sample = pred_original_sample


class _Cfg(dict):
    __getattr__ = dict.__getitem__


class _KDiffusionRestate:
    """What the two 0.18.0 classes write identically: betas, sigmas, timestep spacing, input scaling."""
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0, dtype=torch.float32):
        self.config = _Cfg(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule=beta_schedule, prediction_type=prediction_type, timestep_spacing=timestep_spacing,
                           steps_offset=steps_offset, use_karras_sigmas=False, interpolation_type="linear")
        if beta_schedule == "linear":
            self.betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(beta_schedule)
        self.dtype = dtype
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        sigmas = np.array(((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5)
        sigmas = np.concatenate([sigmas[::-1], [0.0]]).astype(np.float32)
        self.sigmas = torch.from_numpy(sigmas).to(dtype)
        self.num_inference_steps = None
        timesteps = np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=float)[::-1].copy()
        self.timesteps = torch.from_numpy(timesteps)
        self.is_scale_input_called = False

    @property
    def init_noise_sigma(self):
        if self.config.timestep_spacing in ["linspace", "trailing"]:
            return self.sigmas.max()
        return (self.sigmas.max() ** 2 + 1) ** 0.5

    def _index(self, timestep):
        if isinstance(timestep, torch.Tensor):
            timestep = timestep.to(self.timesteps.device)
        return (self.timesteps == timestep).nonzero().item()

    def scale_model_input(self, sample, timestep):
        step_index = self._index(timestep)
        sigma = self.sigmas[step_index]
        sample = sample / ((sigma ** 2 + 1) ** 0.5)
        self.is_scale_input_called = True
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        if self.config.timestep_spacing == "linspace":
            timesteps = np.linspace(0, self.config.num_train_timesteps - 1, num_inference_steps, dtype=float)[::-1].copy()
        elif self.config.timestep_spacing == "leading":
            step_ratio = self.config.num_train_timesteps // self.num_inference_steps
            timesteps = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(float)
            timesteps += self.config.steps_offset
        elif self.config.timestep_spacing == "trailing":
            step_ratio = self.config.num_train_timesteps / self.num_inference_steps
            timesteps = (np.arange(self.config.num_train_timesteps, 0, -step_ratio)).round().copy().astype(float)
            timesteps -= 1
        else:
            raise ValueError(self.config.timestep_spacing)
        sigmas = np.array(((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5)
        sigmas = np.interp(timesteps, np.arange(0, len(sigmas)), sigmas)
        sigmas = np.concatenate([sigmas, [0.0]]).astype(np.float32)
        self.sigmas = torch.from_numpy(sigmas).to(self.dtype)
        self.timesteps = torch.from_numpy(timesteps)
        self.derivatives = []

    def _pred_original(self, model_output, sample, sigma):
        if self.config.prediction_type == "epsilon":
            return sample - sigma * model_output
        if self.config.prediction_type == "v_prediction":
            return model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + (sample / (sigma ** 2 + 1))
        raise ValueError(self.config.prediction_type)


class EulerRestate(_KDiffusionRestate):
    def step(self, model_output, timestep, sample, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0):
        step_index = self._index(timestep)
        sigma = self.sigmas[step_index]
        gamma = min(s_churn / (len(self.sigmas) - 1), 2 ** 0.5 - 1) if s_tmin <= sigma <= s_tmax else 0.0
        assert gamma == 0                                   # no churn: the class draws noise and scales it by 0
        sigma_hat = sigma * (gamma + 1)
        pred_original_sample = self._pred_original(model_output, sample, sigma_hat if
                                                   self.config.prediction_type == "epsilon" else sigma)
        derivative = (sample - pred_original_sample) / sigma_hat
        dt = self.sigmas[step_index + 1] - sigma_hat
        prev_sample = sample + derivative * dt
        return _Out(prev_sample, pred_original_sample)


class LMSRestate(_KDiffusionRestate):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.derivatives = []

    def get_lms_coefficient(self, order, t, current_order):
        def lms_derivative(tau):
            prod = 1.0
            for k in range(order):
                if current_order == k:
                    continue
                prod *= (tau - self.sigmas[t - k]) / (self.sigmas[t - current_order] - self.sigmas[t - k])
            return prod

        integrated_coeff = integrate.quad(lms_derivative, self.sigmas[t], self.sigmas[t + 1], epsrel=1e-4)[0]
        return integrated_coeff

    def step(self, model_output, timestep, sample, order=4):
        step_index = self._index(timestep)
        sigma = self.sigmas[step_index]
        pred_original_sample = self._pred_original(model_output, sample, sigma)
        derivative = (sample - pred_original_sample) / sigma
        self.derivatives.append(derivative)
        if len(self.derivatives) > order:
            self.derivatives.pop(0)
        order = min(step_index + 1, order)
        lms_coeffs = [self.get_lms_coefficient(order, step_index, curr_order) for curr_order in range(order)]
        prev_sample = sample + sum(coeff * derivative for coeff, derivative in zip(lms_coeffs, reversed(self.derivatives)))
        return _Out(prev_sample, pred_original_sample)


def sd_config(prediction_type="epsilon", **over):
    """The scheduler_config.json fields of an SD 1.x / 2.x checkpoint that these classes read (no timestep_spacing key: the
    class default "linspace" applies; steps_offset 1 is there and unused by that spacing)."""
    return dict(dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                     prediction_type=prediction_type, steps_offset=1), **over)
