"""TEST INFRASTRUCTURE — the cases of tests/golden/run_sigma_tiny.npz (tools/make_golden_sigma.py) and how their inputs are
drawn, shared by the golden script and the tests.  Text embeddings and unit start noise are regenerated from their seeds
(the file keeps float64 checksums of both); the start latents are that noise times the scheduler's init_noise_sigma.  The
layout, its token positions and the guidance arguments are those of the G5 block of oracle/make_golden.py, with the
iteration plan of the issue: max_iter = [2, 1], max_index_step = 2, loss_threshold = 0.

What the file keeps per case: a fixed, seeded sample of SAMPLE elements of the latents before every step and the final
latents whole; the teacher-forced case (guided Euler) keeps every step's latents whole, since each one is a start."""
import numpy as np
import torch

# name, UNet config, sampler, prediction type, steps, latent seed, guided, whole history kept
CASES = [("tiny_euler_guided", "tiny", "euler", "epsilon", 6, 41, True, True),
         ("tiny_lms_guided", "tiny", "lms", "epsilon", 6, 41, True, False),
         ("tiny_sd21_euler_v", "tiny_sd21", "euler", "v_prediction", 6, 43, False, False)]
TEXT_SEED = 1
SAMPLE = 256
GUIDANCE = 7.5
KEYS = [("mid", 0, 0, 0), ("up", 1, 0, 0), ("up", 1, 1, 0), ("up", 1, 2, 0)]          # pipelines.py:14
# the canonical 2-box layout of oracle/make_golden.py (boxes xyxy in [0, 1])
BBOXES = [[x / 512, y / 512, (x + w) / 512, (y + h) / 512] for x, y, w, h in ([74, 177, 183, 235], [314, 193, 189, 216])]
OBJ_POS = [[1, 2, 3], [5, 6, 7]]
MAX_ITER, MAX_INDEX_STEP = [2, 1], 2
SG_KWARGS = dict(loss_scale=5, loss_threshold=0.0, max_iter=MAX_ITER, max_index_step=MAX_INDEX_STEP, use_ratio_based_loss=False,
                 guidance_attn_keys=KEYS, fg_top_p=0.2, bg_top_p=0.2, fg_weight=1.0, bg_weight=4.0)


def scheduler_config(prediction_type):
    """The scheduler_config.json fields of an SD checkpoint that the sigma-space classes read: no timestep_spacing key, so the
    class default "linspace" applies."""
    return dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                prediction_type=prediction_type, steps_offset=1)


def case_inputs(cfg, seed):
    """(unit start noise (1,C,L,L), text (2,77,Cx) = [uncond; cond]) of a case, fp32 on the CPU."""
    from lgd_amd import weights
    L = cfg.sample_size
    noise = torch.randn((1, cfg.in_channels, L, L), generator=torch.Generator().manual_seed(seed))
    unc, cond = weights.synth_embeddings(cfg, 1, seed=TEXT_SEED)
    return noise, torch.cat([unc, cond])


def sample_index(numel):
    """Sorted element indices of the per-step sample (seeded, the same for every run)."""
    return np.sort(np.random.default_rng(0).choice(numel, SAMPLE, replace=False)).astype(np.int32)


def checksum(t):
    t = torch.as_tensor(t).double()
    return np.array([float(t.sum()), float((t * t).sum())])
