"""DDIM scheduler (eta = 0) as the reference configures it ([ext] diffusers 0.18.0 DDIMScheduler with
the SD scheduler_config: scaled_linear betas 0.00085..0.012, 1000 train steps, steps_offset=1,
set_alpha_to_one=False, clip_sample=False; used at models/pipelines.py:150,196,221,357,443,545,583).

Keeps the attribute surface the reference touches (`timesteps`, `alphas_cumprod`, `init_noise_sigma`,
`num_inference_steps`, `config.num_train_timesteps`, `scale_model_input`, `set_timesteps`, `step`) so
utils/schedule.py works unchanged, and exports the per-step coefficient table the fused HIP step
kernel reads (`coef_table`).
"""
import numpy as np
import torch


class _Cfg(dict):
    __getattr__ = dict.__getitem__


class _StepOutput:
    """What `step` returns, as far as the reference reads it."""

    def __init__(self, prev_sample):
        self.prev_sample = prev_sample


# `step_kind` of a scheduler class: the fused CFG + step kernel that its coefficient table drives (loop.StepKernel)
DDIM, MULTISTEP, PLMS, LMS = "ddim", "multistep", "plms", "lms"
# column of `guidance_step_table` that holds c_in = 1/sqrt(sigma^2 + 1) under a scheduler with `scales_model_input`
C_IN_GCOL = 1


class DDIMScheduler:
    step_kind = DDIM                  # coef_table -> lgd_cfg_ddim_step_f32

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
                 steps_offset=1, prediction_type="epsilon"):
        self.config = _Cfg(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule="scaled_linear", steps_offset=steps_offset,
                           prediction_type=prediction_type, clip_sample=False, set_alpha_to_one=False)
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.final_alpha_cumprod = self.alphas_cumprod[0]
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = None

    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts) + self.config.steps_offset

    def prev_timestep(self, t, index=None):
        return int(t) - self.config.num_train_timesteps // self.num_inference_steps

    def alpha_pair(self, t):
        prev_t = self.prev_timestep(t)
        a_t = float(self.alphas_cumprod[int(t)])
        a_p = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else float(self.final_alpha_cumprod)
        return a_t, a_p

    def step(self, model_output, timestep, sample):
        """Host/torch form (used by the hook-compatible slow path and by tests)."""
        a_t, a_p = self.alpha_pair(timestep)
        if self.config.prediction_type == "epsilon":
            x0 = (sample - (1 - a_t) ** 0.5 * model_output) / a_t ** 0.5
            e = model_output
        else:
            x0 = a_t ** 0.5 * sample - (1 - a_t) ** 0.5 * model_output
            e = a_t ** 0.5 * model_output + (1 - a_t) ** 0.5 * sample
        return _StepOutput(a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * e)

    def coef_table(self, guidance_scale: float, device, timesteps=None, step_ratios=None) -> torch.Tensor:
        """fp32 [T][4] = {alpha_bar_t, alpha_bar_prev, guidance_scale | sqrt(1-alpha_bar_t), v_pred}.

        Column 2 holds the CFG scale for the step kernel; the guidance update (pipelines.py:62-69)
        uses sqrt(1 - alpha_bar_t), exported separately by `guidance_step_table`."""
        ts = self.timesteps if timesteps is None else timesteps
        rows = []
        for i, t in enumerate(ts):
            t = int(t)
            if step_ratios is not None:
                prev_t = t - step_ratios[i]
            else:
                prev_t = self.prev_timestep(t)
            a_t = float(self.alphas_cumprod[t])
            a_p = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else float(self.final_alpha_cumprod)
            rows.append([a_t, a_p, guidance_scale, 1.0 if self.config.prediction_type == "v_prediction" else 0.0])
        return torch.tensor(rows, dtype=torch.float32, device=device)

    def add_noise(self, original, noise, timestep):
        """[ext] diffusers 0.18.0 DDIMScheduler.add_noise: sqrt(alpha_bar_t) * original + sqrt(1 - alpha_bar_t) * noise,
        alpha_bar_t in the samples' dtype (the background bootstrapping of generation/multidiffusion.py:245-247; the
        device form is lgd_multidiffusion_step_f32).  timestep: int, or a tensor of one per sample."""
        ac = self.alphas_cumprod.to(device=original.device, dtype=original.dtype)
        t = torch.as_tensor(timestep, device=original.device).long()
        sqrt_alpha_prod = (ac[t] ** 0.5).flatten()
        while sqrt_alpha_prod.dim() < original.dim():
            sqrt_alpha_prod = sqrt_alpha_prod.unsqueeze(-1)
        sqrt_one_minus_alpha_prod = ((1 - ac[t]) ** 0.5).flatten()
        while sqrt_one_minus_alpha_prod.dim() < original.dim():
            sqrt_one_minus_alpha_prod = sqrt_one_minus_alpha_prod.unsqueeze(-1)
        return sqrt_alpha_prod * original + sqrt_one_minus_alpha_prod * noise

    def guidance_step_table(self, device, timesteps=None) -> torch.Tensor:
        """fp32 [T][4] with column 0 = sqrt(1 - alpha_bar_t): DDIM has no `sigmas`, so the latent
        update of backward guidance is scaled this way (pipelines.py:62-69)."""
        ts = self.timesteps if timesteps is None else timesteps
        rows = [[float((1 - self.alphas_cumprod[int(t)]) ** 0.5), 0.0, 0.0, 0.0] for t in ts]
        return torch.tensor(rows, dtype=torch.float32, device=device)

    # ---- utils/schedule.py (the optional fast tail of the per-box generations)
    @staticmethod
    def fast_schedule(timesteps, fast_after_steps, fast_rate=2):
        """schedule.py:4-8: keep the first `fast_after_steps` timesteps, then every `fast_rate`-th."""
        if fast_after_steps >= len(timesteps) - 1:
            return timesteps
        return torch.cat((timesteps[:fast_after_steps], timesteps[fast_after_steps + 1::fast_rate]), dim=0)

    def dynamic_step_sizes(self, timesteps):
        """schedule.py:10-12 followed by the scheduler's own prev_timestep rule: before each step the
        reference sets num_inference_steps = N_train // (t - next_t) (next_t = -1 after the last one) and
        DDIM then steps by N_train // num_inference_steps.  Returns that step size per index."""
        n_train = self.config.num_train_timesteps
        out = []
        for i, t in enumerate(timesteps):
            nxt = int(timesteps[i + 1]) if i + 1 < len(timesteps) else -1
            out.append(n_train // (n_train // (int(t) - nxt)))
        return out



class DDIMInverseScheduler(DDIMScheduler):
    """[ext] diffusers 0.18.0 DDIMInverseScheduler as `DDIMInverseScheduler.from_config(scheduler.config)` makes it next to
    the DDIM scheduler of an SD checkpoint (models/models.py:57-59): clip_sample=False, eta 0, epsilon and v_prediction —
    the scheduler of models/pipelines.py:489-539 (`invert`).  diffusers is absent from the sandbox: restated from the
    published class, parity unpinned at this boundary; pinned against a line-for-line stateful restatement
    (tests/ddim_inverse_restate.py) and, step by step, against DDIMScheduler.step, which undoes it for a fixed model output.

    One inversion step is the DDIM step with the noise levels taken in the other direction,
        x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t) ;  x' = sqrt(a_next) x0 + sqrt(1 - a_next) e,   t_next = t + N_train // n,
    so `coef_table` rows are {alpha_bar_t, alpha_bar_next, guidance_scale, v flag} and `lgd_cfg_ddim_step_f32` runs them
    unchanged.  Final alpha: the DDIM config's set_alpha_to_one=False reaches the 0.18.0 class through its deprecated
    keyword as set_alpha_to_zero=False, i.e. final_alpha_cumprod = alphas_cumprod[-1] (not 0) when t_next >= N_train.
    `invert` never takes the last timestep of the schedule, so that value is unreachable from it."""
    inverse = True                    # sampler.LMDSampler._refuse_undefined: the plain CFG loop only

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 prediction_type="epsilon"):
        if prediction_type not in ("epsilon", "v_prediction"):
            raise NotImplementedError(f"DDIMInverseScheduler: prediction_type {prediction_type!r}")
        super().__init__(num_train_timesteps, beta_start, beta_end, steps_offset, prediction_type)
        self.config.update(set_alpha_to_zero=False)
        self.final_alpha_cumprod = self.alphas_cumprod[-1]

    @classmethod
    def from_config(cls, scheduler):
        """The inverse scheduler next to `scheduler` (model_dict.scheduler, or its `config`): the same betas, train step
        count, steps_offset and prediction type."""
        c = scheduler if isinstance(scheduler, dict) else scheduler.config
        return cls(c.num_train_timesteps, c.beta_start, c.beta_end, steps_offset=c.steps_offset,
                   prediction_type=c.prediction_type)

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round().copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts) + self.config.steps_offset

    def next_timestep(self, t):
        return int(t) + self.config.num_train_timesteps // self.num_inference_steps

    def prev_timestep(self, t, index=None):
        """The timestep `step` moves to (the class keeps DDIM's name for it): the NEXT, noisier one."""
        return self.next_timestep(t)

    def alpha_pair(self, t):
        nxt = self.next_timestep(t)
        a_n = float(self.alphas_cumprod[nxt]) if nxt < self.config.num_train_timesteps else float(self.final_alpha_cumprod)
        return float(self.alphas_cumprod[int(t)]), a_n

    def coef_table(self, guidance_scale: float, device, timesteps=None, step_ratios=None) -> torch.Tensor:
        """fp32 [T][4] = {alpha_bar_t, alpha_bar_next, guidance_scale, v_pred}: lgd_cfg_ddim_step_f32's rows."""
        if step_ratios is not None:
            raise RuntimeError("DDIMInverseScheduler: per-step sizes belong to the fast schedule of descending DDIM runs")
        ts = self.timesteps if timesteps is None else timesteps
        v = 1.0 if self.config.prediction_type == "v_prediction" else 0.0
        return torch.tensor([[*self.alpha_pair(t), guidance_scale, v] for t in ts], dtype=torch.float32, device=device)

    def dynamic_step_sizes(self, timesteps):
        """None: the step size is N_train // n at every index (utils/schedule.py only re-derives descending schedules)."""
        return None

    @staticmethod
    def fast_schedule(timesteps, fast_after_steps, fast_rate=2):
        raise RuntimeError("the fast schedule (utils/schedule.py) is not defined for DDIM inversion")

    def add_noise(self, original, noise, timestep):
        raise RuntimeError("DDIMInverseScheduler has no add_noise (the 0.18.0 class has none)")

    def guidance_step_table(self, device, timesteps=None) -> torch.Tensor:
        raise RuntimeError("DDIMInverseScheduler inverts with the plain CFG loop (pipelines.py:489-539): backward guidance "
                           "is not defined under it")


class DPMSolverMultistepScheduler(DDIMScheduler):
    """[ext] diffusers 0.18.0 DPMSolverMultistepScheduler with its defaults (algorithm_type "dpmsolver++",
    solver_order 2, solver_type "midpoint", lower_order_final, no thresholding) — what `load_sd(...,
    use_dpm_multistep_scheduler=True)` selects (models/models.py:46-47).  Restated from the published algorithm
    (DPM-Solver++, Lu et al. 2022, eq. 2M) — diffusers is absent from the sandbox: parity unpinned at this boundary;
    the first-order case is pinned against DDIM, which it equals identically (tests/test_schedule.py).

    The update is linear in (x, x0, x0_prev), so the device side is the fused `lgd_cfg_multistep_step_f32` kernel
    reading one coefficient row per step (`multistep_table`); nothing about the captured hipGraphs changes.
    Backward guidance scales its latent update by sqrt(1 - alpha_bar_t) as with DDIM: the 0.18.0 class has no
    `sigmas` attribute unless Karras sigmas are switched on (pipelines.py:60-69)."""
    step_kind = MULTISTEP             # multistep_table -> lgd_cfg_multistep_step_f32

    def __init__(self, *a, solver_order=2, lower_order_final=True, **k):
        super().__init__(*a, **k)
        self.config.update(solver_order=solver_order, lower_order_final=lower_order_final,
                           algorithm_type="dpmsolver++", solver_type="midpoint")

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        n = self.config.num_train_timesteps
        ts = np.linspace(0, n - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(ts)

    def _als(self, t):
        a = float(self.alphas_cumprod[int(t)])
        alpha, sigma = a ** 0.5, (1.0 - a) ** 0.5
        return alpha, sigma, float(np.log(alpha) - np.log(sigma))

    def multistep_rows(self, timesteps=None):
        """Per step: (c0, c1, A, B, C) of  x0 = c0 x + c1 m ;  x' = A x + B x0 + C x0_prev."""
        ts = [int(t) for t in (self.timesteps if timesteps is None else timesteps)]
        n = len(ts)
        rows = []
        for i, t in enumerate(ts):
            t_next = ts[i + 1] if i + 1 < n else 0                          # the last step lands on timestep 0
            a_t, s_t, l_t = self._als(t)
            a_n, s_n, l_n = self._als(t_next)
            h = l_n - l_t
            if self.config.prediction_type == "v_prediction":
                c0, c1 = a_t, -s_t
            else:
                c0, c1 = 1.0 / a_t, -s_t / a_t
            first = (i == 0 or self.config.solver_order == 1 or
                     (i == n - 1 and self.config.lower_order_final and n < 15))
            A = s_n / s_t
            e = float(np.expm1(-h))                                          # exp(-h) - 1
            if first:
                B, C = -a_n * e, 0.0
            else:
                _, _, l_p = self._als(ts[i - 1])
                r = (l_t - l_p) / h
                B, C = -a_n * e * (1.0 + 0.5 / r), 0.5 * a_n * e / r
            rows.append((c0, c1, A, B, C))
        return rows

    def multistep_table(self, guidance_scale: float, device, timesteps=None) -> torch.Tensor:
        rows = [[c0, c1, A, B, C, guidance_scale, 0.0, 0.0] for c0, c1, A, B, C in self.multistep_rows(timesteps)]
        return torch.tensor(rows, dtype=torch.float32, device=device)

    def coef_table(self, guidance_scale, device, timesteps=None, step_ratios=None):
        raise RuntimeError("DPMSolverMultistepScheduler drives lgd_cfg_multistep_step_f32 (multistep_table)")

    def prev_timestep(self, t, index=None):
        raise RuntimeError("multistep scheduler: the next timestep is the next entry of `timesteps`")

    def step_host(self, model_output, index, sample, x0_prev=None):
        """Torch form of one step (tests): returns (prev_sample, x0)."""
        c0, c1, A, B, C = self.multistep_rows()[index]
        x0 = c0 * sample + c1 * model_output
        out = A * sample + B * x0 + (C * x0_prev if C != 0.0 else 0.0)
        return out, x0


class PNDMScheduler(DDIMScheduler):
    """[ext] diffusers 0.18.0 PNDMScheduler with skip_prk_steps=True, set_alpha_to_one=False (epsilon and v_prediction):
    the PLMS sampler that StableDiffusionPipeline.from_pretrained takes from the runwayml/stable-diffusion-v1-5 and
    stabilityai/stable-diffusion-2-1-base checkpoints, i.e. what generation/stable_diffusion_generate.py:13 runs.
    diffusers is absent from the sandbox: restated from the published algorithm (PLMS, Liu et al. 2022) and the 0.18.0
    class, parity unpinned at this boundary; pinned against a line-for-line stateful restatement (tests/pndm_restate.py)
    and, for a constant noise prediction, against DDIM (tests/test_sd_generate_cpu.py).

    n steps make n+1 UNet evaluations: timesteps = (_t[:-1], _t[-2], _t[-1]) reversed with _t = arange(n) * (1000 // n)
    + steps_offset; the second evaluation re-runs the first step from the saved sample with the average of both outputs.
    Every evaluation is one affine update of (source sample, PLMS combination of the current output and a ring of the
    last three pushed ones), so the device side is the fused `lgd_cfg_plms_step_f32` kernel reading one coefficient
    row per evaluation (`plms_table`); one captured hipGraph replays every evaluation."""
    step_kind = PLMS                  # plms_table -> lgd_cfg_plms_step_f32
    # PLMS weights over (newest, ..., oldest) outputs by history length (PNDMScheduler.step_plms)
    ORDER_WEIGHTS = {1: (1.0,), 2: (1.5, -0.5), 3: (23 / 12, -16 / 12, 5 / 12),
                     4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}
    TABLE_COLS = 16

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 prediction_type="epsilon", skip_prk_steps=True, set_alpha_to_one=False):
        if not skip_prk_steps:
            raise NotImplementedError("PNDMScheduler: only skip_prk_steps=True (PLMS) is implemented")
        if set_alpha_to_one:
            raise NotImplementedError("PNDMScheduler: only set_alpha_to_one=False (the SD 1.5 / 2.1-base value) is implemented")
        if prediction_type not in ("epsilon", "v_prediction"):
            raise NotImplementedError(f"PNDMScheduler: prediction_type {prediction_type!r}")
        super().__init__(num_train_timesteps, beta_start, beta_end, steps_offset, prediction_type)
        self.config.update(skip_prk_steps=True)
        self.counter = 0
        self._host = None

    @classmethod
    def from_config(cls, scheduler):
        """The PNDM scheduler of an SD 1.5 / SD 2.1-base checkpoint next to `scheduler` (model_dict.scheduler): its betas,
        train step count and prediction type, with steps_offset=1, set_alpha_to_one=False, skip_prk_steps=True."""
        c = scheduler.config
        return cls(c.num_train_timesteps, c.beta_start, c.beta_end, steps_offset=1, prediction_type=c.prediction_type)

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        t = (np.arange(0, num_inference_steps) * ratio).round().astype(np.int64) + self.config.steps_offset
        plms = np.concatenate([t[:-1], t[-2:-1], t[-1:]])[::-1].copy()
        self.timesteps = torch.from_numpy(plms)
        self.counter = 0
        self._host = None

    def plms_rows(self, timesteps=None):
        """Per evaluation k: (w_m, w_ring0, w_ring1, w_ring2, a, b, push slot, from_cur, save_cur) of
            comb = w_m m + sum_s w_rings ets[s];  ets[push] = m;  x' = a (cur_sample if from_cur else x) + b comb.
        The j-th push goes to ring slot j % 3, so the oldest output of a fourth-order step sits in the slot the
        current one is pushed to (the kernel reads it first)."""
        ts = [int(t) for t in (self.timesteps if timesteps is None else timesteps)]
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        rows, pushes = [], 0
        for k, t in enumerate(ts):
            prev = t - ratio
            ring = [0.0, 0.0, 0.0]
            push = -1
            if k != 1:
                push, pushes = pushes % 3, pushes + 1
                w = self.ORDER_WEIGHTS[min(pushes, 4)]
                wm = w[0]
                for j, wj in enumerate(w[1:]):            # ets[-2], ets[-3], ets[-4] = pushes - 2, - 3, - 4
                    ring[(pushes - 2 - j) % 3] = wj
            else:                                        # the averaged re-evaluation of the first step
                prev, t = t, t + ratio
                wm, ring[0] = 0.5, 0.5
            a_t = float(self.alphas_cumprod[t])
            a_p = float(self.alphas_cumprod[prev]) if prev >= 0 else float(self.final_alpha_cumprod)
            sc = (a_p / a_t) ** 0.5                          # PNDMScheduler._get_prev_sample
            c = (a_p - a_t) / (a_t * (1 - a_p) ** 0.5 + (a_t * (1 - a_t) * a_p) ** 0.5)
            if self.config.prediction_type == "v_prediction":
                a, b = sc - c * (1 - a_t) ** 0.5, -c * a_t ** 0.5
            else:
                a, b = sc, -c
            rows.append((wm, ring[0], ring[1], ring[2], a, b, push, 1.0 if k == 1 else 0.0, 1.0 if k == 0 else 0.0))
        return rows

    def plms_table(self, guidance_scale: float, device, timesteps=None) -> torch.Tensor:
        """fp32 [E][16] = {w_m, w_ring0..2, a, b, guidance_scale, push slot, from_cur, save_cur, 0...} (lgd_hip.h)."""
        rows = [[wm, w0, w1, w2, a, b, guidance_scale, float(p), fc, sv] + [0.0] * (self.TABLE_COLS - 10)
                for wm, w0, w1, w2, a, b, p, fc, sv in self.plms_rows(timesteps)]
        return torch.tensor(rows, dtype=torch.float32, device=device)

    def host_state(self, like):
        """Ring + saved sample of `step_host`, shaped like one sample."""
        return dict(ets=[torch.zeros_like(like) for _ in range(3)], cur=torch.zeros_like(like))

    def step_host(self, model_output, index, sample, state):
        """Torch form of evaluation `index` in the table form the kernel runs (tests): updates `state` (host_state)
        and returns the new sample."""
        wm, w0, w1, w2, a, b, push, from_cur, save_cur = self.plms_rows()[index]
        comb = wm * model_output
        for s, w in enumerate((w0, w1, w2)):
            if w != 0.0:
                comb = comb + w * state["ets"][s]
        if push >= 0:
            state["ets"][push] = model_output.clone()
        src = state["cur"] if from_cur else sample
        if save_cur:
            state["cur"] = sample.clone()
        return a * src + b * comb

    def step(self, model_output, timestep, sample):
        """Stateful host form with PNDMScheduler.step's surface (evaluations in schedule order)."""
        if self._host is None:
            self._host = self.host_state(sample)
        out = _StepOutput(self.step_host(model_output, self.counter, sample, self._host))
        self.counter += 1
        return out

    def coef_table(self, guidance_scale, device, timesteps=None, step_ratios=None):
        raise RuntimeError("PNDMScheduler drives lgd_cfg_plms_step_f32 (plms_table)")

    def prev_timestep(self, t, index=None):
        raise RuntimeError("PNDMScheduler: the step of evaluation k is a row of plms_rows")


class _SigmaSpaceScheduler:
    """What the k-diffusion family of [ext] diffusers 0.18.0 shares (EulerDiscreteScheduler, LMSDiscreteScheduler): the
    samplers `generate.py --scheduler NAME` reaches through models.load_sd(scheduler_cls=...) and for which
    models/pipelines.py keeps the `sigmas` branch of latent_backward_guidance (:60-61) and calls scale_model_input before
    every UNet evaluation.  They work in sigma space, x = x0 + sigma * eps with sigma = sqrt((1 - abar) / abar), and feed
    the model x / sqrt(sigma^2 + 1).  diffusers is absent from the machines that run the suite: restated from the
    published classes, parity unpinned at this boundary; pinned against line-for-line stateful restatements
    (tests/sigma_sched_restate.py).

    `sigmas` holds the reversed training sigmas with 0 appended from construction on, and the schedule's own after
    `set_timesteps`; `init_noise_sigma` reads whichever is current.  timestep_spacing: "linspace" (the class default,
    hence what an SD 1.x / 2.x scheduler_config.json yields through from_config: it has no such key) has FRACTIONAL
    timesteps, np.linspace(0, N_train - 1, n)[::-1]; "leading" is arange(n) * (N_train // n) + steps_offset; "trailing"
    is round(arange(N_train, 0, -N_train / n)) - 1.  Sigmas of fractional timesteps are interpolated linearly.

    Backward guidance under these samplers (pipelines.py:60-61) is latents - grad * sigma_i^2, the gradient taken with
    respect to the latents; the grad plan returns it with respect to the UNet input x * c_in, c_in = 1/sqrt(sigma^2 + 1),
    so `guidance_step_table` column 0 is sigma_i^2 * c_in_i (the chain rule) and column 1 is c_in_i itself, which
    `lgd_scale_rows_f32` reads by dyn[0] in front of both UNet passes."""
    scales_model_input = True         # the sampler scales the UNet input by guidance_step_table column C_IN_GCOL
    stateless_rows = False            # True: a row reads nothing an earlier step left behind, partial schedules are defined
    DEFAULTS = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                    prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0, use_karras_sigmas=False)

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=0,
                 prediction_type="epsilon", timestep_spacing="linspace", beta_schedule="scaled_linear",
                 use_karras_sigmas=False, interpolation_type="linear"):
        name = type(self).__name__
        if prediction_type not in ("epsilon", "v_prediction"):
            raise NotImplementedError(f"{name}: prediction_type {prediction_type!r}")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise NotImplementedError(f"{name}: timestep_spacing {timestep_spacing!r}")
        if use_karras_sigmas:
            raise NotImplementedError(f"{name}: use_karras_sigmas=True re-spaces the sigmas (Karras et al. 2022, eq. 5); "
                                      "only the checkpoint's own sigmas are implemented")
        if interpolation_type != "linear":
            raise NotImplementedError(f"{name}: interpolation_type {interpolation_type!r}; only \"linear\" is implemented")
        if beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        else:
            raise NotImplementedError(f"{name}: beta_schedule {beta_schedule!r}")
        self.config = _Cfg(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                           beta_schedule=beta_schedule, steps_offset=steps_offset, prediction_type=prediction_type,
                           timestep_spacing=timestep_spacing, interpolation_type="linear", use_karras_sigmas=False)
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.num_inference_steps = None
        sig = self._train_sigmas()
        self.sigmas = torch.from_numpy(np.concatenate([sig[::-1], [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=float)[::-1].copy())

    @classmethod
    def from_config(cls, cfg):
        """The scheduler a checkpoint's scheduler_config (a dict, or an object with `.config`) makes of this class: keys
        the config lacks take the diffusers class defaults (DEFAULTS: linspace spacing, steps_offset 0), keys this class
        does not read (clip_sample, set_alpha_to_one, skip_prk_steps, ...) are ignored as `from_config` ignores them."""
        c = dict(cfg if isinstance(cfg, dict) else cfg.config)
        kw = {k: c.get(k, d) for k, d in cls.DEFAULTS.items()}
        if "interpolation_type" in c:
            kw["interpolation_type"] = c["interpolation_type"]
        return cls(**kw)

    def _train_sigmas(self):
        return (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps
        n, spacing = self.config.num_train_timesteps, self.config.timestep_spacing
        if spacing == "linspace":
            ts = np.linspace(0, n - 1, num_inference_steps, dtype=float)[::-1].copy()
        elif spacing == "leading":
            # fp32 timesteps: the SDXL refiner's schedule (sdxl.SDXLRefiner), kept to the bit
            ts = (np.arange(0, num_inference_steps) * (n // num_inference_steps)).round()[::-1].copy().astype(np.float32)
            ts += self.config.steps_offset
        else:
            ts = np.arange(n, 0, -n / num_inference_steps).round().copy().astype(float) - 1
        sig = self._train_sigmas()
        sig = np.interp(ts, np.arange(0, len(sig)), sig)
        self.sigmas = torch.from_numpy(np.concatenate([sig, [0.0]]).astype(np.float32))
        self.timesteps = torch.from_numpy(ts)

    @property
    def init_noise_sigma(self):
        """Of the current `sigmas`: the training ones before set_timesteps, the schedule's after."""
        if self.config.timestep_spacing in ("linspace", "trailing"):
            return float(self.sigmas.max())
        return float((self.sigmas.max() ** 2 + 1) ** 0.5)

    def index_of(self, t):
        return int((self.timesteps == float(t)).nonzero()[0])

    def scale_model_input(self, sample, timestep):
        s = float(self.sigmas[self.index_of(timestep)])
        return sample / ((s * s + 1) ** 0.5)

    def add_noise(self, original, noise, timestep):
        return original + noise * float(self.sigmas[self.index_of(timestep)])

    def x0_coefficients(self, sigma):
        """(c0, c1) of the data prediction x0 = c0 x + c1 m from the CFG-combined model output m."""
        if self.config.prediction_type == "v_prediction":
            return 1.0 / (sigma * sigma + 1.0), -sigma / (sigma * sigma + 1.0) ** 0.5
        return 1.0, -sigma

    def guidance_step_table(self, device, timesteps=None) -> torch.Tensor:
        """fp32 [T][4] = {sigma_i^2 * c_in_i, c_in_i, 0, 0} (class docstring)."""
        idx = range(len(self.timesteps)) if timesteps is None else map(self.index_of, timesteps)
        rows = []
        for i in idx:
            s = float(self.sigmas[i])
            c_in = 1.0 / (s * s + 1.0) ** 0.5
            rows.append([s * s * c_in, c_in, 0.0, 0.0])
        return torch.tensor(rows, dtype=torch.float32, device=device)

    @staticmethod
    def fast_schedule(timesteps, fast_after_steps, fast_rate=2):
        raise RuntimeError("the fast schedule (utils/schedule.py) shortens `timesteps` and leaves `sigmas` as they are: under "
                           "a sigma-space scheduler the reference then pairs the wrong sigma with each step; not defined")

    def dynamic_step_sizes(self, timesteps):
        return None

    def coef_table(self, guidance_scale, device, timesteps=None, step_ratios=None):
        raise RuntimeError(f"{type(self).__name__} drives the {self.step_kind} step kernel, not lgd_cfg_ddim_step_f32")

    def prev_timestep(self, t, index=None):
        raise RuntimeError("sigma-space scheduler: the next noise level is the next entry of `sigmas`")


class EulerDiscreteScheduler(_SigmaSpaceScheduler):
    """[ext] diffusers 0.18.0 EulerDiscreteScheduler without churn (s_churn 0: deterministic; Karras et al. 2022,
    Algorithm 2), epsilon and v_prediction, three timestep spacings (_SigmaSpaceScheduler).  The bare constructor is the
    SDXL refiner's configuration (scheduler_config of stabilityai/stable-diffusion-xl-refiner-1.0: scaled_linear betas
    0.00085..0.012, 1000 train steps, timestep_spacing "leading", steps_offset 1, epsilon) — the sampler behind
    generation/sdxl_refinement.py:29; `from_config` of an SD 1.x / 2.x scheduler_config gives "linspace" spacing, what
    `generate.py --scheduler EulerDiscreteScheduler` runs.  diffusers is absent from the machines that run the suite:
    restated from the published class, parity unpinned at this boundary; pinned against tests/sigma_sched_restate.py.

    In sigma space (x = x0 + sigma * eps) one Euler step is linear in (x, x0):
        x0 = c0 x + c1 m ;  x' = x + (sigma' - sigma) (x - x0) / sigma = (sigma'/sigma) x + (1 - sigma'/sigma) x0
    with (c0, c1) = (1, -sigma) for epsilon and (1/(sigma^2 + 1), -sigma/sqrt(sigma^2 + 1)) for v_prediction, so the device
    side is the fused `lgd_cfg_multistep_step_f32` kernel with rows {c0, c1, sigma'/sigma, 1 - sigma'/sigma, 0,
    guidance_scale, c_in, 0}; c_in = 1/sqrt(sigma^2 + 1) (scale_model_input) is applied by `lgd_scale_rows_f32` from the
    same row (the refiner) or from guidance_step_table (sampler.LMDSampler).  The last step (sigma' = 0) returns x0."""
    step_kind = MULTISTEP
    stateless_rows = True             # C = 0 in every row: x0_prev is never read
    C_IN_COL = 6

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1,
                 prediction_type="epsilon", timestep_spacing="leading", beta_schedule="scaled_linear",
                 use_karras_sigmas=False, interpolation_type="linear"):
        super().__init__(num_train_timesteps, beta_start, beta_end, steps_offset, prediction_type, timestep_spacing,
                         beta_schedule, use_karras_sigmas, interpolation_type)

    def img2img_start(self, num_inference_steps, strength):
        """StableDiffusionXLImg2ImgPipeline.get_timesteps (no denoising_start): index of the first step that runs."""
        init = min(int(num_inference_steps * strength), num_inference_steps)
        return max(num_inference_steps - init, 0)

    def multistep_rows(self, timesteps=None):
        rows = []
        for i in (range(len(self.timesteps)) if timesteps is None else map(self.index_of, timesteps)):
            s, sn = float(self.sigmas[i]), float(self.sigmas[i + 1])
            c0, c1 = self.x0_coefficients(s)
            rows.append((c0, c1, sn / s, 1.0 - sn / s, 0.0, 1.0 / (s * s + 1.0) ** 0.5))
        return rows

    def multistep_table(self, guidance_scale: float, device, timesteps=None) -> torch.Tensor:
        rows = [[c0, c1, A, B, C, guidance_scale, c_in, 0.0] for c0, c1, A, B, C, c_in in self.multistep_rows(timesteps)]
        return torch.tensor(rows, dtype=torch.float32, device=device)

    def step_host(self, model_output, index, sample):
        """Torch form of one step as the scheduler class writes it (tests); the fp32 sigmas enter as Python floats, so
        that the arithmetic is the sample's own (fp64 samples: fp64 throughout)."""
        s, sn = float(self.sigmas[index]), float(self.sigmas[index + 1])
        if self.config.prediction_type == "v_prediction":
            pred_original = model_output * (-s / (s ** 2 + 1) ** 0.5) + (sample / (s ** 2 + 1))
        else:
            pred_original = sample - s * model_output
        return sample + (sample - pred_original) / s * (sn - s)


class LMSDiscreteScheduler(_SigmaSpaceScheduler):
    """[ext] diffusers 0.18.0 LMSDiscreteScheduler (the linear multistep sampler of k-diffusion, order 4), epsilon and
    v_prediction, on the sigmas, spacings, init_noise_sigma and scale_model_input of _SigmaSpaceScheduler; the bare
    constructor is what `from_config` makes of an SD 1.x scheduler_config (scaled_linear betas, "linspace" spacing).
    diffusers is absent from the machines that run the suite: restated from the published class, parity unpinned at this
    boundary; pinned against tests/sigma_sched_restate.py.

    One step with d_j = (x_j - x0_j) / sigma_j, the derivative of step j:
        order = min(i + 1, 4) ;  x' = x + sum_{k < order} coeff_k d_{i-k}
        coeff_k = integral over [sigma_i, sigma_{i+1}] of the Lagrange basis polynomial of node sigma_{i-k} among
                  sigma_i ... sigma_{i-order+1}.
    The class integrates with scipy.integrate.quad(epsrel=1e-4); the integrand is a polynomial of degree < 4, so
    `lms_coefficients` integrates it exactly in fp64 (in u = tau - sigma_i, whose antiderivative vanishes at the lower
    limit: no cancellation between the two ends).  The two agree to ~2e-12 relative (tests/test_sigma_schedulers_cpu.py):
    the same sampler.

    The device side is `lgd_cfg_lms_step_f32`: the derivatives live in a ring of 4 latents, d_j in slot j % 4, and
    `lms_table` permutes the coefficients onto slots, rows {c0, c1, 1/sigma, w[0..3] by slot, guidance_scale, slot, 0...}
    (16 columns), so the kernel does no modular arithmetic.  A slot's weight is 0 where the order does not reach it."""
    step_kind = LMS                   # lms_table -> lgd_cfg_lms_step_f32
    ORDER = 4
    TABLE_COLS = 16

    def lms_coefficients(self, index, order=None):
        """coeff_k, k < min(index + 1, order): exact fp64 integrals of the Lagrange basis polynomials."""
        order = min(index + 1, self.ORDER if order is None else order)
        s = [float(self.sigmas[index - k]) for k in range(order)]
        h = float(self.sigmas[index + 1]) - s[0]
        out = []
        for k in range(order):
            num, den = np.poly1d([1.0]), 1.0
            for j in range(order):
                if j != k:
                    num = num * np.poly1d([1.0, -(s[j] - s[0])])          # (u - (sigma_{i-j} - sigma_i))
                    den *= s[k] - s[j]
            out.append(float(np.polyint(num)(h)) / den)
        return out

    def lms_rows(self, timesteps=None, order=None):
        """Per step: (c0, c1, 1/sigma, (w_0..w_3) by ring slot, slot of this step's derivative).  `timesteps`: the whole
        schedule only — row i mixes in the derivatives of steps i-1 .. i-3 (sampler: first_step > 0 is refused)."""
        if timesteps is not None and [float(t) for t in timesteps] != [float(t) for t in self.timesteps]:
            raise RuntimeError("LMSDiscreteScheduler: rows exist for the whole schedule only (the ring carries the last "
                               "three derivatives)")
        rows = []
        for i in range(len(self.timesteps)):
            s = float(self.sigmas[i])
            c0, c1 = self.x0_coefficients(s)
            w = [0.0] * self.ORDER
            for k, c in enumerate(self.lms_coefficients(i, order)):
                w[(i - k) % self.ORDER] = c
            rows.append((c0, c1, 1.0 / s, tuple(w), i % self.ORDER))
        return rows

    def lms_table(self, guidance_scale: float, device, timesteps=None) -> torch.Tensor:
        """fp32 [T][16] = {c0, c1, 1/sigma, w_0, w_1, w_2, w_3, guidance_scale, slot, 0...} (lgd_hip.h)."""
        rows = [[c0, c1, inv, *w, guidance_scale, float(slot)] + [0.0] * (self.TABLE_COLS - 9)
                for c0, c1, inv, w, slot in self.lms_rows(timesteps)]
        return torch.tensor(rows, dtype=torch.float32, device=device)

    def host_state(self, like):
        """Ring of `step_host`, shaped like one sample."""
        return dict(ring=[torch.zeros_like(like) for _ in range(self.ORDER)])

    def step_host(self, model_output, index, sample, state, order=None):
        """Torch form of step `index` in the table form the kernel runs (tests): updates `state` (host_state) and
        returns the new sample."""
        c0, c1, inv, w, slot = self.lms_rows(order=order)[index]
        d = (sample - (c0 * sample + c1 * model_output)) * inv
        out = sample + w[slot] * d
        for s in range(self.ORDER):
            if s != slot and w[s] != 0.0:
                out = out + w[s] * state["ring"][s]
        state["ring"][slot] = d.clone()
        return out
