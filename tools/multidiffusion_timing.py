"""Seconds per image of the MultiDiffusion baseline (lgd_amd.multidiffusion) at full width — the SD1.5 topology and the
SD VAE with seeded synthetic weights, 64x64 latents, 512x512 images, 50 steps, bootstrapping 20 — for layouts of 0, 2
and 5 boxes.  A timed run covers the reference's whole generate(): the background colours and their VAE encodes, the
draws, the denoising loop and the decode (text encoding is outside: seeded embeddings stand in for it).  Device events
time each run after one untimed call that captures the graph.

    python tools/multidiffusion_timing.py [--boxes 0 2 5] [--steps 50] [--bootstrapping 20] [--reps 2]

Under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/multidiffusion_timing.py --reps 1` the same run gives the
step kernel's time per launch (multidiffusion_step_kernel) next to the UNet's kernels."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgd_amd  # noqa: E402,F401
from lgd_amd import multidiffusion as mdc, vae, weights  # noqa: E402
from lgd_amd.sampler import LMDSampler  # noqa: E402
from lgd_amd.unet import UNetEngine  # noqa: E402

BOXES = [("a", [20, 30, 150, 160]), ("b", [300, 40, 180, 150]), ("c", [60, 300, 170, 180]),
         ("d", [320, 300, 150, 170]), ("e", [180, 180, 150, 150])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, nargs="+", default=[0, 2, 5])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--bootstrapping", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU")
    dev = torch.device("cuda:0")
    cfg = weights.CONFIGS["sd15"]
    state = vae.synth_aekl_state_dict(seed=0)
    sm = LMDSampler(UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0)), vae=vae.HipVAEDecoder(state, dev))
    enc = vae.HipVAEEncoder(state, dev)
    for nbox in a.boxes:
        prep = mdc.prepare(BOXES[:nbox], "bg", "n", "n")
        P = len(prep["prompts"])
        unc, cond = weights.synth_embeddings(cfg, P, seed=1)
        texts = torch.cat([unc.expand(P, -1, -1), cond])

        def run(seed=7):
            d = mdc.draw_randomness(enc, dev, seed, a.bootstrapping, P, a.steps)
            return mdc.multidiffusion_generate(sm, texts, prep["masks"], d["start_latent"], d["bg_latents"],
                                               d["picks"], steps=a.steps, n_boot=a.bootstrapping)
        run()                                                          # graph, plan, first launches
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = run()
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1) / 1000.0)
        print(json.dumps(dict(boxes=nbox, prompts=P, steps=a.steps, bootstrapping=a.bootstrapping,
                              unet_batch=2 * mdc.padded_rows(sm, P), seconds_per_image=min(times),
                              seconds_per_run=times, image=list(out["image"].shape))), flush=True)


if __name__ == "__main__":
    main()
