"""Time per step of a MultiDiffusion panorama against the same number of single-view steps — the SD1.5 topology with
seeded synthetic weights, P = 3 prompts, 512 x 2048 pixels (64 x 256 latent, 25 views), 50 steps, bootstrapping 20,
graphs on, no decode.  The single-view loop (one 64 x 64 view, lgd_multidiffusion_step_f32) is the path the panorama
loop was added beside; V of its steps are what V views cost when they are denoised one after the other.

Both loops run in one process, alternating, after an untimed call each that builds the plans and captures the graphs;
every timed block is a whole run between device synchronisations, divided by its steps.  Afterwards one eager panorama
step under ops.LaunchProfiler gives the share of the step spent in the two view kernels.

    python tools/ab_multidiffusion_panorama.py [--width 2048] [--steps 50] [--bootstrapping 20] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgd_amd  # noqa: E402,F401
from lgd_amd import multidiffusion as mdc, ops, weights  # noqa: E402
from lgd_amd.sampler import LMDSampler  # noqa: E402
from lgd_amd.unet import UNetEngine  # noqa: E402


def region_masks(P, hp, wp):
    """Background + P-1 vertical bands at a third of the width each, disjoint."""
    fg = torch.zeros((P - 1, 1, hp, wp))
    band = wp // (P + 1)
    for k in range(P - 1):
        fg[k, 0, hp // 8:hp - hp // 8, (k + 1) * band:(k + 1) * band + band // 2] = 1.0
    return torch.cat([1 - fg.sum(0, keepdim=True), fg])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--bootstrapping", type=int, default=20)
    ap.add_argument("--prompts", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU")
    dev = torch.device("cuda:0")
    cfg = weights.CONFIGS["sd15"]
    eng = UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0))
    sm = LMDSampler(eng)
    P, T, n_boot = a.prompts, a.steps, a.bootstrapping
    hp, wp = 64, a.width // 8
    V = len(mdc.get_views(512, a.width))
    unc, cond = weights.synth_embeddings(cfg, P, seed=1)
    texts = torch.cat([unc.expand(P, -1, -1), cond])
    g = torch.Generator().manual_seed(3)
    bg = torch.randn((n_boot, 4, 64, 64), generator=g) * 0.5
    pano = dict(masks=region_masks(P, hp, wp), start=torch.randn((1, 4, hp, wp), generator=g),
                picks=torch.randint(0, n_boot, (min(n_boot, T), V, P - 1), generator=g))
    one = dict(masks=region_masks(P, 64, 64), start=torch.randn((1, 4, 64, 64), generator=g),
               picks=torch.randint(0, n_boot, (min(n_boot, T), P - 1), generator=g))

    def run(d, sampler=sm, **kw):
        return mdc.multidiffusion_generate(sampler, texts, d["masks"], d["start"], bg, d["picks"], steps=T, n_boot=n_boot,
                                           guidance_scale=7.5, decode=False, **kw)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / T * 1e3

    panorama = lambda: run(pano, indep_uncond=False, normalization=True)
    single = lambda: run(one)
    for fn in (panorama, single, panorama, single):                  # plans, graphs, clocks
        fn()
    t_pano, t_one = [], []
    for _ in range(a.reps):
        t_pano.append(timed(panorama))
        t_one.append(timed(single))
    med = lambda v: sorted(v)[len(v) // 2]
    rows = mdc.padded_rows(sm, P)
    per_call = min(V, eng.max_text_batch // (2 * rows))
    res = dict(prompts=P, rows_per_view=2 * rows, views=V, views_per_call=per_call, calls_per_step=-(-V // per_call),
               steps=T, bootstrapping=n_boot, panorama_ms_per_step=med(t_pano), single_view_ms_per_step=med(t_one),
               sequential_views_ms=V * med(t_one), ratio=med(t_pano) / (V * med(t_one)),
               panorama_ms_all=t_pano, single_view_ms_all=t_one)

    # one eager step under the launch profiler: the share of the view kernels
    ops.PROFILER = ops.LaunchProfiler(max_records=100000)
    try:
        run(pano, sampler=LMDSampler(eng, use_graphs=False), indep_uncond=False, normalization=True, n_steps=1)
        agg = ops.PROFILER.summary()
    finally:
        ops.PROFILER = None
    total = sum(v["ms"] for v in agg.values())
    mine = {k: v for k, v in agg.items() if k.startswith("multidiffusion_views_")}
    res.update(profiled_step_kernel_ms=total,
               view_kernels={k: dict(ms=v["ms"], launches=v["n"], us_per_launch=1e3 * v["ms"] / v["n"]) for k, v in mine.items()},
               view_kernels_share=sum(v["ms"] for v in mine.values()) / total)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
