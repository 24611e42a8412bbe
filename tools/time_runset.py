#!/usr/bin/env python
"""What the prompt-set runner costs against the benchmark it was lifted from, in one session on one GPU:

  1. `python bench.py --workload lmd_v0.1 --prompts 100 --lanes 4` (its own process; finished before anything else starts);
  2. lgd_amd.runset.generate_set on the same 100 prompts, seeded weights and synthetic text side, 50 steps, 4 lanes:
       share / group=None   the calls the benchmark launches (gate: at most 5 % below line 1)
       share / group=8
       layout               one call per layout: the price of images that do not depend on the split

Every arm first runs an untimed 2-step pass over its own calls (launch plans and captured graphs, as bench.py pre-builds
them), then one timed pass between device synchronisations.  Images are decoded to the host as the benchmark does and
kept nowhere.

    python tools/time_runset.py [--out profiles/runset_timing.txt] [--prompts 100] [--steps 50] [--lanes 4]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_line(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--workload",
           "lmd_v0.1", "--prompts", str(args.prompts), "--lanes", str(args.lanes), "--num-inference-steps", str(args.steps)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1100)
    if r.returncode != 0:
        raise SystemExit(f"bench.py failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "runset_timing.txt"))
    ap.add_argument("--prompts", type=int, default=100)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--no-bench", action="store_true", help="skip line 1")
    args = ap.parse_args()

    bench = None if args.no_bench else bench_line(args)

    import torch
    import lgd_amd  # noqa: F401
    from lgd_amd import runset, weights
    from lgd_amd.lanes import LanePool
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.set_num_threads(1)
    cfg = weights.CONFIGS["sd14_gligen"]
    rows = runset.load_cache()
    items = runset.cache_items(rows, runset.select(len(rows), args.prompts, spread=True))
    costs = [runset.layout_cost(it.n_boxes, args.steps) for it in items]
    n_lanes = runset.lanes_for(len(items), args.lanes)
    lanes = runset.synthetic_lanes(cfg, dev, n_lanes)
    make_layout = runset.synthetic_layouts(cfg)
    arms = [("share group=None", dict(batching="share", group=None)), ("share group=8", dict(batching="share", group=8)),
            ("layout", dict(batching="layout"))]
    lines = []
    with LanePool(lanes, device=dev) as pool:
        for name, kw in arms:
            common = dict(costs=costs, decode=True, **kw)
            t0 = time.perf_counter()
            runset.generate_set(pool, items, make_layout, num_inference_steps=2, overall_max_index_step=2,
                                frozen_step_ratio=0.5, **common)
            torch.cuda.synchronize()
            pre = time.perf_counter() - t0
            t0 = time.perf_counter()
            outs = runset.generate_set(pool, items, make_layout, num_inference_steps=args.steps, **common)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            iters = sum(o["guidance_iters"] for o in outs) / len(outs)
            lines.append((name, len(outs) / dt, dt, pre, iters))
            print(f"{name}: {len(outs) / dt:.3f} images/s ({dt:.1f} s, untimed pass {pre:.1f} s)", flush=True)
            del outs

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(f"tools/time_runset.py: {args.prompts} prompts of the lmd_v0.1 cache (spread), {args.steps} steps, {n_lanes} lanes, "
                 f"sd14_gligen, seeded weights, one {torch.cuda.get_device_name(0)}\n")
        if bench is not None:
            fh.write(f"bench.py --workload lmd_v0.1 --prompts {args.prompts} --lanes {args.lanes} --steps 1 --warmup 0: "
                     f"{bench['value']:.3f} images/s ({bench['ms_per_step'] / 1e3:.1f} s)\n")
        for name, ips, dt, pre, iters in lines:
            rel = f", {ips / bench['value']:.3f} of the bench line" if bench is not None else ""
            fh.write(f"runset {name}: {ips:.3f} images/s ({dt:.1f} s; untimed 2-step pass {pre:.1f} s; "
                     f"{iters:.1f} guidance iterations per image){rel}\n")
        fh.write(f"layout / share group=None: {lines[2][1] / lines[0][1]:.3f}\n")
    if bench is not None and lines[0][1] < 0.95 * bench["value"]:
        print(f"GATE MISSED: share group=None {lines[0][1]:.3f} images/s is more than 5 % below the bench line {bench['value']:.3f}")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
