"""TEST INFRASTRUCTURE — a stateful, line-for-line restatement of [ext] diffusers 0.18.0 PNDMScheduler (skip_prk_steps=True,
set_alpha_to_one=False; `set_timesteps`, `step` -> `step_plms`, `_get_prev_sample`), kept apart from the table form of
lgd_amd.scheduler.PNDMScheduler so that the two can be checked against each other.  It keeps `ets`, `counter` and
`cur_sample` as the diffusers class does.  `dtype` selects the arithmetic: float32 is what the pipeline computes (the
golden of tools/make_golden_sd.py), float64 pins the table form to ~1e-15."""
import numpy as np
import torch


class _Out:
    def __init__(self, prev_sample):
        self.prev_sample = prev_sample


class _Cfg(dict):
    __getattr__ = dict.__getitem__


class PNDMRestate:
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 prediction_type="epsilon", dtype=torch.float32):
        self.config = _Cfg(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule="scaled_linear", steps_offset=steps_offset, prediction_type=prediction_type,
                           skip_prk_steps=True, set_alpha_to_one=False)
        # scaled_linear betas in fp32 as diffusers builds them; the cumulative product stays fp32 (the pipeline's
        # alphas); `dtype` only widens the values the step arithmetic starts from
        self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0).to(dtype)
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.pndm_order = 4
        self.cur_model_output = 0
        self.counter = 0
        self.cur_sample = None
        self.ets = []
        self.num_inference_steps = None
        self.timesteps = None

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        step_ratio = self.config.num_train_timesteps // self.num_inference_steps
        self._timesteps = (np.arange(0, num_inference_steps) * step_ratio).round()
        self._timesteps += self.config.steps_offset
        self.prk_timesteps = np.array([])
        self.plms_timesteps = np.concatenate([self._timesteps[:-1], self._timesteps[-2:-1],
                                              self._timesteps[-1:]])[::-1].copy()
        timesteps = np.concatenate([self.prk_timesteps, self.plms_timesteps]).astype(np.int64)
        self.timesteps = torch.from_numpy(timesteps).to(device)
        self.ets = []
        self.counter = 0
        self.cur_model_output = 0

    def scale_model_input(self, sample, *args, **kwargs):
        return sample

    def step(self, model_output, timestep, sample, return_dict=True):
        return self.step_plms(model_output=model_output, timestep=timestep, sample=sample)

    def step_plms(self, model_output, timestep, sample):
        timestep = int(timestep)
        prev_timestep = timestep - self.config.num_train_timesteps // self.num_inference_steps

        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(model_output)
        else:
            prev_timestep = timestep
            timestep = timestep + self.config.num_train_timesteps // self.num_inference_steps

        if len(self.ets) == 1 and self.counter == 0:
            model_output = model_output
            self.cur_sample = sample
        elif len(self.ets) == 1 and self.counter == 1:
            model_output = (model_output + self.ets[-1]) / 2
            sample = self.cur_sample
            self.cur_sample = None
        elif len(self.ets) == 2:
            model_output = (3 * self.ets[-1] - self.ets[-2]) / 2
        elif len(self.ets) == 3:
            model_output = (23 * self.ets[-1] - 16 * self.ets[-2] + 5 * self.ets[-3]) / 12
        else:
            model_output = (1 / 24) * (55 * self.ets[-1] - 59 * self.ets[-2] + 37 * self.ets[-3] - 9 * self.ets[-4])

        prev_sample = self._get_prev_sample(sample, timestep, prev_timestep, model_output)
        self.counter += 1
        return _Out(prev_sample)

    def _get_prev_sample(self, sample, timestep, prev_timestep, model_output):
        alpha_prod_t = self.alphas_cumprod[timestep]
        alpha_prod_t_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev

        if self.config.prediction_type == "v_prediction":
            model_output = (alpha_prod_t ** 0.5) * model_output + (beta_prod_t ** 0.5) * sample
        elif self.config.prediction_type != "epsilon":
            raise ValueError(self.config.prediction_type)

        sample_coeff = (alpha_prod_t_prev / alpha_prod_t) ** (0.5)
        model_output_denom_coeff = alpha_prod_t * beta_prod_t_prev ** (0.5) + (
            alpha_prod_t * beta_prod_t * alpha_prod_t_prev) ** (0.5)
        prev_sample = (sample_coeff * sample - (alpha_prod_t_prev - alpha_prod_t) * model_output
                       / model_output_denom_coeff)
        return prev_sample
