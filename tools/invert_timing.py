"""Seconds per call of lgd_amd.pipeline.invert_batch (DDIM inversion: T - 1 CFG + inverse-DDIM steps of a T-step schedule)
next to a DDIM lgd_amd.pipeline.sd_generate_batch(decode=False) with the same number of UNet calls, in one process at full
width — the SD1.5 topology with seeded synthetic weights, 64x64 latents — timed with device events after one untimed
call of each that captures the graphs.  Both run the same loop (sampler.LMDSampler.denoise_batch) and the same fused step
kernel, so the two should agree within run-to-run spread.

    python tools/invert_timing.py [--batches 1 8] [--steps 50] [--reps 3]

Prints one JSON line per batch size (profiles/invert_timing.jsonl)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgd_amd  # noqa: E402,F401
from lgd_amd import weights  # noqa: E402
from lgd_amd.pipeline import invert_batch, sd_generate_batch  # noqa: E402
from lgd_amd.sampler import LMDSampler  # noqa: E402
from lgd_amd.scheduler import DDIMScheduler  # noqa: E402
from lgd_amd.unet import UNetEngine  # noqa: E402


def timed(run, reps):
    run()                                                              # graphs, plans, first launches
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        run()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) / 1000.0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU")
    dev = torch.device("cuda:0")
    cfg = weights.CONFIGS["sd15"]
    sm = LMDSampler(UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0)))
    unc, cond = weights.synth_embeddings(cfg, 1, seed=1)
    text = torch.cat([unc, cond])
    for nb in a.batches:
        lats = torch.randn((nb, 4, 64, 64), generator=torch.Generator().manual_seed(nb))
        inv = timed(lambda: invert_batch(sm, [text] * nb, lats, a.steps), a.reps)
        ddim = timed(lambda: sd_generate_batch(sm, [text] * nb, lats, a.steps - 1, scheduler=DDIMScheduler(), decode=False),
                     a.reps)
        print(json.dumps(dict(batch=nb, steps=a.steps, unet_calls=a.steps - 1, invert_seconds_per_call=inv,
                              ddim_generate_seconds_per_call=ddim, invert_seconds=min(inv), ddim_generate_seconds=min(ddim),
                              ratio=min(inv) / min(ddim))), flush=True)


if __name__ == "__main__":
    main()
