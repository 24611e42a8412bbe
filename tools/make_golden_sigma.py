"""ORACLE TEST INFRASTRUCTURE (needs the reference tree; CPU) — golden of the reference's loops under the sigma-space
samplers (`generate.py --scheduler EulerDiscreteScheduler | LMSDiscreteScheduler`).

Drives the reference's OWN, unmodified `models.pipelines.generate_semantic_guidance` (pipelines.py:129-247, with
latent_backward_guidance :16-82 taking its `sigmas` branch, :60-61) and `models.pipelines.generate` (:250-279) through
oracle/ref_harness.build_model_dict (imported read-only): the reference UNet with the seeded synthetic weights of
lgd_amd.weights, fp32, on CPU.  `model_dict.scheduler` is replaced by tests/sigma_sched_restate.{EulerRestate, LMSRestate} —
stateful line-for-line restatements of the diffusers 0.18.0 classes in fp32, as `scheduler_cls.from_pretrained` configures
them from an SD scheduler_config.json ("linspace" spacing), written apart from the table forms of lgd_amd.scheduler.

Pinning: diffusers is not installed where this runs, so the scheduler side is pinned to the restatements, not to the
diffusers classes themselves; the UNet, the guidance, the energy and the loops are the reference's code.

Recording changes no behaviour: a forward pre-hook on the UNet notes every evaluation's batch size (1: a guidance
iteration, 2: the CFG pass, whose first input row is the step's scaled latents) and a wrapper around
pipelines.latent_backward_guidance notes the loss each call returns.

Cases and what is stored: tests/sigma_golden_cases.py.

    python tools/make_golden_sigma.py [--out PATH]     # default tests/golden/run_sigma_tiny.npz
"""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lgd_amd  # noqa: E402,F401
from lgd_amd import weights  # noqa: E402
import ref_harness as rh  # noqa: E402
from sigma_golden_cases import (BBOXES, CASES, GUIDANCE, OBJ_POS, SG_KWARGS, case_inputs, checksum, sample_index,  # noqa: E402
                                scheduler_config)
from sigma_sched_restate import EulerRestate, LMSRestate  # noqa: E402


def run_case(cfg_name, sampler, prediction, steps, seed, guided, whole):
    cfg = weights.CONFIGS[cfg_name]              # seeded weights: the prediction type is the scheduler's alone
    md = rh.build_model_dict(cfg)
    from models import pipelines
    md.scheduler = (EulerRestate if sampler == "euler" else LMSRestate)(**scheduler_config(prediction))
    noise, text = case_inputs(cfg, seed)
    sigma0 = float(md.scheduler.init_noise_sigma)
    lat = noise * sigma0                                                    # utils/latents.py:20-22
    unc, cond = text[0:1], text[1:2]
    batches, losses, inputs = [], [], []

    def note(mod, args):
        batches.append(int(args[0].shape[0]))
        if args[0].shape[0] == 2:
            inputs.append(args[0][0:1].detach().clone())
    hook = md.unet.register_forward_pre_hook(note)
    inner = pipelines.latent_backward_guidance

    def noting(*a, **k):
        out = inner(*a, **k)
        losses.append(float(out[1]))
        return out
    pipelines.latent_backward_guidance = noting
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if guided:
                out, _, hist = pipelines.generate_semantic_guidance(
                    md, lat.clone(), (text, unc, cond), steps, BBOXES, ["a", "b"], OBJ_POS, guidance_scale=GUIDANCE,
                    semantic_guidance_kwargs=dict(SG_KWARGS, verbose=False), save_all_latents=True, show_progress=False)
            else:
                with torch.no_grad():
                    out, _ = pipelines.generate(md, lat.clone(), (text, unc, cond), steps, guidance_scale=GUIDANCE)
                hist = None
    finally:
        pipelines.latent_backward_guidance = inner
        hook.remove()
    iters, n = [], 0                                                        # guidance iterations in front of each CFG pass
    for b in batches:
        if b == 1:
            n += 1
        else:
            iters.append(n)
            n = 0
    assert len(iters) == steps
    inputs = torch.cat(inputs)
    idx = sample_index(inputs[0].numel())
    r = dict(inputs_sample=inputs.reshape(steps, -1)[:, idx].numpy(), noise_checksum=checksum(noise),
             text_checksum=checksum(text), init_noise_sigma=np.float64(sigma0),
             timesteps=md.scheduler.timesteps.numpy().astype(np.float64), sigmas=md.scheduler.sigmas.numpy(),
             final=out.detach().numpy(), steps=np.int64(steps), guidance_iters=np.array(iters, dtype=np.int64),
             guidance_losses=np.array(losses, dtype=np.float64))
    if hist is not None:
        hist = hist.detach().float()
        assert hist.shape[0] == steps + 1 and torch.equal(hist[-1], out.detach())
        r["latents_sample"] = hist.reshape(steps + 1, -1)[:, idx].numpy()
        if whole:
            r["latents_all"] = hist.numpy()
    return r


def build_arrays():
    torch.set_num_threads(8)
    arrs = dict(sample_index=sample_index(4 * 32 * 32))
    for name, *case in CASES:
        r = run_case(*case)
        for k, v in r.items():
            arrs[f"{name}/{k}"] = v
        print(f"{name}: guidance iterations {r['guidance_iters'].tolist()}, losses {np.round(r['guidance_losses'], 4).tolist()}, "
              f"final |x| max {np.abs(r['final']).max():.4f}")
    return arrs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "run_sigma_tiny.npz"))
    a = ap.parse_args()
    np.savez_compressed(a.out, **build_arrays())
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
