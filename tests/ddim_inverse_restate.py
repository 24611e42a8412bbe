"""TEST INFRASTRUCTURE — a stateful, line-for-line restatement of [ext] diffusers 0.18.0 DDIMInverseScheduler
(`set_timesteps`, `step`) as `DDIMInverseScheduler.from_config(scheduler.config)` builds it next to the DDIM scheduler of
an SD checkpoint (models/models.py:57-59 of the reference), kept apart from the table form of
lgd_amd.scheduler.DDIMInverseScheduler so that the two can be checked against each other.

Final alpha: the DDIM config carries set_alpha_to_one=False; the 0.18.0 class takes that deprecated keyword as
`set_alpha_to_zero`, so final_alpha_cumprod = alphas_cumprod[-1] (with set_alpha_to_zero=True it would be 0).  It applies
when the next timestep is >= num_train_timesteps, which models/pipelines.py:504 (`timesteps[:-1]`) never reaches.

`dtype` selects the arithmetic: float32 is what the pipeline computes (the golden of tools/make_golden_invert.py), float64
pins the table form to ~1e-15."""
import numpy as np
import torch


class _Out:
    def __init__(self, prev_sample, pred_original_sample):
        self.prev_sample = prev_sample
        self.pred_original_sample = pred_original_sample


class _Cfg(dict):
    __getattr__ = dict.__getitem__


class DDIMInverseRestate:
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 prediction_type="epsilon", clip_sample=False, set_alpha_to_zero=False, dtype=torch.float32):
        self.config = _Cfg(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule="scaled_linear", steps_offset=steps_offset, prediction_type=prediction_type,
                           clip_sample=clip_sample, set_alpha_to_zero=set_alpha_to_zero, clip_sample_range=1.0)
        # scaled_linear betas in fp32 as diffusers builds them; `dtype` only widens the values the step starts from
        self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0).to(dtype)
        # "At every step in inverted ddim, we are looking into the next alphas_cumprod.  For the final step, there is no
        # next alphas_cumprod": zero, or the last alpha of the training schedule
        self.final_alpha_cumprod = torch.tensor(0.0, dtype=dtype) if set_alpha_to_zero else self.alphas_cumprod[-1]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps).copy().astype(np.int64))

    @classmethod
    def from_config(cls, config, dtype=torch.float32):
        """What ConfigMixin.from_config does with a DDIMScheduler config: shared fields pass through, and
        `set_alpha_to_one` arrives as the deprecated alias of `set_alpha_to_zero`."""
        return cls(num_train_timesteps=config["num_train_timesteps"], beta_start=config["beta_start"],
                   beta_end=config["beta_end"], steps_offset=config["steps_offset"],
                   prediction_type=config["prediction_type"], clip_sample=config["clip_sample"],
                   set_alpha_to_zero=config["set_alpha_to_one"], dtype=dtype)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        if num_inference_steps > self.config.num_train_timesteps:
            raise ValueError(num_inference_steps)
        self.num_inference_steps = num_inference_steps
        step_ratio = self.config.num_train_timesteps // self.num_inference_steps
        timesteps = (np.arange(0, num_inference_steps) * step_ratio).round().copy().astype(np.int64)
        self.timesteps = torch.from_numpy(timesteps).to(device)
        self.timesteps += self.config.steps_offset

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, variance_noise=None,
             return_dict=True):
        # 1. get previous step value (=t+1)
        prev_timestep = timestep + self.config.num_train_timesteps // self.num_inference_steps

        # 2. compute alphas, betas
        alpha_prod_t = self.alphas_cumprod[timestep]
        alpha_prod_t_prev = (self.alphas_cumprod[prev_timestep] if prev_timestep < self.config.num_train_timesteps
                             else self.final_alpha_cumprod)
        beta_prod_t = 1 - alpha_prod_t

        # 3. compute predicted original sample from predicted noise
        if self.config.prediction_type == "epsilon":
            pred_original_sample = (sample - beta_prod_t ** (0.5) * model_output) / alpha_prod_t ** (0.5)
            pred_epsilon = model_output
        elif self.config.prediction_type == "sample":
            pred_original_sample = model_output
            pred_epsilon = (sample - alpha_prod_t ** (0.5) * pred_original_sample) / beta_prod_t ** (0.5)
        elif self.config.prediction_type == "v_prediction":
            pred_original_sample = (alpha_prod_t ** 0.5) * sample - (beta_prod_t ** 0.5) * model_output
            pred_epsilon = (alpha_prod_t ** 0.5) * model_output + (beta_prod_t ** 0.5) * sample
        else:
            raise ValueError(self.config.prediction_type)

        # 4. clip the predicted x_0
        if self.config.clip_sample:
            pred_original_sample = pred_original_sample.clamp(-self.config.clip_sample_range, self.config.clip_sample_range)

        # 5. "direction pointing to x_t"
        pred_sample_direction = (1 - alpha_prod_t_prev) ** (0.5) * pred_epsilon

        # 6. x_t without "random noise"
        prev_sample = alpha_prod_t_prev ** (0.5) * pred_original_sample + pred_sample_direction
        return _Out(prev_sample, pred_original_sample)
