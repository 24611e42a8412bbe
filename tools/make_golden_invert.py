"""ORACLE TEST INFRASTRUCTURE (needs the reference tree; CPU) — golden of DDIM inversion and of the inversion ->
generate_partial_frozen chain.

Drives the reference's OWN, unmodified `models.pipelines.invert` (pipelines.py:489-539) and
`models.pipelines.generate_partial_frozen` (:541-599) through oracle/ref_harness.build_model_dict (imported read-only): the
reference UNet with the seeded synthetic weights of lgd_amd.weights, fp32, on CPU.  The inverse scheduler is attached here,
    md.inverse_scheduler = DDIMInverseRestate.from_config(md.scheduler.config)
(tests/ddim_inverse_restate.py: a stateful line-for-line restatement of diffusers 0.18.0 DDIMInverseScheduler, fp32
arithmetic as in the pipeline, written apart from the table form of lgd_amd.scheduler.DDIMInverseScheduler).  A forward
pre-hook on the UNet records every evaluation's timestep and batch (no behaviour change).

Pinning: diffusers is not installed where this runs, so the inverse scheduler is pinned to the restatement, not to the
diffusers class itself; the UNet, both loops and the DDIM stub of the chain are the reference's code.

Sensitivity record: inversion under classifier-free guidance is expansive (at scale 7.5 a deviation of this network's
trajectory doubles per step), so every case is run a second time with the reference UNet's parameters rounded to fp16 and
the output of every Conv2d / Linear rounded to fp16 by forward hooks (fp32 arithmetic otherwise; no reference code is
changed) — the number format of the HIP engine's storage.  The rel-L2 per row between the two runs of the reference itself
(`fp16_sensitivity`, and `chain_fp16_sensitivity` for the chain's final latents) is what a free-running comparison of any
fp16 engine with this golden can be held to.

What is stored (tests/invert_golden_cases.py): inputs are regenerated from their seeds and the file keeps float64 checksums;
every row of the returned stack as a fixed, seeded sample of SAMPLE elements; the noisiest row and the chain's final latents
whole.

Cases: tiny / epsilon / 10 steps / scale 7.5;  tiny / scale 0 (the unconditional branch alone; + the chain:
generate_partial_frozen on that stack, box mask, frozen_steps 4, 10 steps, scale 7.5);  tiny_sd21 / v_prediction / scale 1.0.

    python tools/make_golden_invert.py [--out PATH]     # default tests/golden/run_invert_tiny.npz
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
from ddim_inverse_restate import DDIMInverseRestate  # noqa: E402
from invert_golden_cases import (CASES, CHAIN_CASE, CHAIN_FROZEN_STEPS, CHAIN_GUIDANCE, case_inputs, chain_mask,  # noqa: E402
                                 checksum, sample_index)


def fp16_storage(unet):
    """Rounds the parameters to fp16 and, by forward hooks, the output of every Conv2d / Linear (what an engine that keeps
    weights and activations in fp16 and accumulates in fp32 stores)."""
    with torch.no_grad():
        for p in unet.parameters():
            p.copy_(p.half().float())
    for m in unet.modules():
        if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
            m.register_forward_hook(lambda mod, args, out: out.half().float())


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def run_case(name, cfg_name, steps, scale, seed, emulate_fp16=False):
    cfg = weights.CONFIGS[cfg_name]
    md = rh.build_model_dict(cfg)
    if emulate_fp16:
        fp16_storage(md.unet)
    from models import pipelines
    md.inverse_scheduler = DDIMInverseRestate.from_config(md.scheduler.config)
    lat, text = case_inputs(cfg, seed)
    unc, cond = text[0:1], text[1:2]
    ts, batches = [], []
    hook = md.unet.register_forward_pre_hook(lambda mod, args: ts.append(int(args[1])) or batches.append(args[0].shape[0]))
    try:
        stack = pipelines.invert(md, lat.clone(), (text, unc, cond), steps, guidance_scale=scale)
        n_inv = len(ts)
        chain = None
        if name == CHAIN_CASE:
            chain, _ = pipelines.generate_partial_frozen(md, stack, chain_mask(cfg.sample_size), (text, unc, cond), steps,
                                                         CHAIN_FROZEN_STEPS, guidance_scale=CHAIN_GUIDANCE)
    finally:
        hook.remove()
    if emulate_fp16:
        return stack, chain
    idx = sample_index(stack[0].numel())
    stack16, chain16 = run_case(name, cfg_name, steps, scale, seed, emulate_fp16=True)
    out = dict(fp16_sensitivity=np.array([rel_l2(stack16[k], stack[k]) for k in range(stack.shape[0])]),
               latents0_checksum=checksum(lat), text_checksum=checksum(text),
               stack_sample=stack.reshape(stack.shape[0], -1)[:, idx].numpy(), stack_shape=np.array(stack.shape),
               noisiest=stack[0].numpy(), timesteps=np.array(ts[:n_inv]), unet_batch=np.array(batches[:n_inv]),
               steps=np.int64(steps), guidance=np.float64(scale),
               prediction_v=np.int64(cfg.prediction_type == "v_prediction"))
    if chain is not None:
        out.update(chain_final=chain.numpy(), chain_timesteps=np.array(ts[n_inv:]),
                   chain_fp16_sensitivity=np.float64(rel_l2(chain16, chain)))
    return out


def build_arrays():
    torch.set_num_threads(8)
    arrs = dict(sample_index=sample_index(4 * 32 * 32))
    for case in CASES:
        with torch.no_grad():
            r = run_case(*case)
        for k, v in r.items():
            arrs[f"{case[0]}/{k}"] = v
        print(f"{case[0]}: {len(r['timesteps'])} UNet evaluations (batch {set(r['unet_batch'].tolist())}), "
              f"noisiest |x| max {np.abs(r['noisiest']).max():.4f}; fp16 sensitivity per row, noisiest first: "
              + " ".join(f"{v:.2e}" for v in r["fp16_sensitivity"])
              + (f"; chain {float(r['chain_fp16_sensitivity']):.2e}" if "chain_fp16_sensitivity" in r else ""))
    return arrs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "run_invert_tiny.npz"))
    a = ap.parse_args()
    np.savez_compressed(a.out, **build_arrays())
    print("wrote", a.out)
