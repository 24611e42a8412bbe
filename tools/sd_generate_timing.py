"""Seconds per image of lgd_amd.pipeline.sd_generate_batch (plain SD: CFG + PNDM/PLMS, n steps = n + 1 UNet evaluations,
VAE decode included) at full width — the SD1.5 topology with seeded synthetic weights, 64x64 latents, 512x512 images —
timed with device events after one untimed call that captures the graphs.

    python tools/sd_generate_timing.py [--batches 1 8] [--steps 50] [--reps 2]

Under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/sd_generate_timing.py --reps 1` the same run gives the
fused step's time per launch (kernel cfg_plms_kernel) next to the UNet's kernels."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgd_amd  # noqa: E402,F401
from lgd_amd import weights  # noqa: E402
from lgd_amd.pipeline import sd_generate_batch  # noqa: E402
from lgd_amd.sampler import LMDSampler  # noqa: E402
from lgd_amd.scheduler import PNDMScheduler  # noqa: E402
from lgd_amd.unet import UNetEngine  # noqa: E402
from lgd_amd.vae import make_hip_vae  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU")
    dev = torch.device("cuda:0")
    cfg = weights.CONFIGS["sd15"]
    sm = LMDSampler(UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0)), vae=make_hip_vae(dev))
    unc, cond = weights.synth_embeddings(cfg, 1, seed=1)
    text = torch.cat([unc, cond])
    for nb in a.batches:
        lats = torch.randn((nb, 4, 64, 64), generator=torch.Generator().manual_seed(nb))
        run = lambda: sd_generate_batch(sm, [text] * nb, lats, a.steps, scheduler=PNDMScheduler())  # noqa: E731
        run()                                                          # graphs, plans, first launches
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            _, images = run()
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1) / 1000.0)
        print(json.dumps(dict(batch=nb, steps=a.steps, unet_evaluations=a.steps + 1, seconds_per_call=times,
                              seconds_per_image=min(times) / nb, images=list(images.shape))), flush=True)


if __name__ == "__main__":
    main()
