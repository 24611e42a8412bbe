"""ORACLE TEST INFRASTRUCTURE (needs the reference tree; CPU) — golden of the plain Stable Diffusion loop (`sd` plugin).

Drives the reference's OWN, unmodified `models.pipelines.generate` (pipelines.py:250-279) through
oracle/ref_harness.build_model_dict (imported read-only): the reference UNet with the seeded synthetic weights of
lgd_amd.weights, fp32, on CPU.  The scheduler under `model_dict[scheduler_key]` is
  * tests/pndm_restate.PNDMRestate — a stateful line-for-line restatement of diffusers 0.18.0 PNDMScheduler
    (skip_prk_steps=True, set_alpha_to_one=False, fp32 arithmetic as in the pipeline), written apart from the table form
    of lgd_amd.scheduler.PNDMScheduler, or
  * the oracle stub's DDIMScheduler (model_dict.scheduler) for the second case.
A forward pre-hook on the UNet records every evaluation's input sample (no behaviour change).

Pinning: diffusers is not installed where this runs, so the PNDM side is pinned to the restatement, not to the diffusers
class itself; the UNet, the CFG loop and the DDIM stub are the reference's code.

What is stored (tests/sd_golden_cases.py): the start latents (torch.Generator seed per case) and text embeddings
(weights.synth_embeddings) are regenerated from their seeds, and the file keeps float64 checksums of both; every
evaluation's input sample is kept as a fixed, seeded sample of SAMPLE elements (the same indices for every evaluation);
the final latents are kept whole.  That keeps the file small while every evaluation stays checked.

Cases: tiny / epsilon / PNDM / 50 steps;  tiny / DDIM / 50 steps;  tiny_sd21 / v_prediction / PNDM / 20 steps.

    python tools/make_golden_sd.py [--out PATH]     # default tests/golden/run_sd_generate_tiny.npz
"""
import argparse
import os
import sys

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
from pndm_restate import PNDMRestate  # noqa: E402
from sd_golden_cases import CASES, GUIDANCE, case_inputs, checksum, sample_index  # noqa: E402


def run_case(cfg_name, kind, steps, seed):
    cfg = weights.CONFIGS[cfg_name]
    md = rh.build_model_dict(cfg)
    from models import pipelines
    md.pndm = PNDMRestate(prediction_type=cfg.prediction_type)
    lat, text = case_inputs(cfg, seed)
    unc, cond = text[0:1], text[1:2]
    inputs, ts = [], []
    hook = md.unet.register_forward_pre_hook(lambda mod, args: inputs.append(args[0][0:1].clone()) or
                                             ts.append(int(args[1])))
    try:
        out, _ = pipelines.generate(md, lat.clone(), (text, unc, cond), steps, guidance_scale=GUIDANCE,
                                    scheduler_key="pndm" if kind == "pndm" else "scheduler")
    finally:
        hook.remove()
    inputs = torch.cat(inputs)
    idx = sample_index(inputs[0].numel())
    return dict(latents0_checksum=checksum(lat), text_checksum=checksum(text),
                inputs_sample=inputs.reshape(inputs.shape[0], -1)[:, idx].numpy(), timesteps=np.array(ts),
                final=out.numpy(), steps=np.int64(steps), prediction_v=np.int64(cfg.prediction_type == "v_prediction"))


def build_arrays():
    torch.set_num_threads(8)
    arrs = dict(sample_index=sample_index(4 * 32 * 32))
    for name, cfg_name, kind, steps, seed in CASES:
        with torch.no_grad():
            r = run_case(cfg_name, kind, steps, seed)
        for k, v in r.items():
            arrs[f"{name}/{k}"] = v
        print(f"{name}: {r['inputs_sample'].shape[0]} UNet evaluations, final |x| max {np.abs(r['final']).max():.4f}")
    return arrs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "run_sd_generate_tiny.npz"))
    a = ap.parse_args()
    np.savez_compressed(a.out, **build_arrays())
    print("wrote", a.out)
