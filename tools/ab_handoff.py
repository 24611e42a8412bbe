"""Host against device hand-off between the two stages of LMD / LMD+ on the same stage-A results: what pipeline._stage_b
runs per layout on the host path (the masks to the host, hostprep.align_with_bboxes + hostprep.compose,
pipeline._align_stage_a's map shifts, pipeline._ref_maps) against lgd_amd.handoff.run for the whole batch (table packing,
one upload, three launches of csrc/handoff.hip).  Seeded synthetic stage-A results of the benchmark's geometry: 64 x 64
latents, 50 steps, the 4 default guidance keys (8 x 8 and 16 x 16 maps, 8 heads), histories as views of one batch tensor,
masks as ONE bool tensor on the device (where the batched refiner leaves them), alignment on.  Both sides ALTERNATE
window by window in one process after untimed warm-up calls; a window is `--iters` calls between device
synchronisations, timed by device events (host work in a window is part of what a call costs).  Medians over `--windows`
windows and their spread are printed per shape (layouts x boxes per layout), one JSON line at the end.

    python tools/ab_handoff.py [--shapes 1x1 4x2 4x5] [--iters 20] [--windows 5] > profiles/handoff_timing.txt
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgd_amd  # noqa: E402,F401
from lgd_amd import handoff, hostprep, pipeline  # noqa: E402
from lgd_amd.sampler import DEFAULT_GUIDANCE_ATTN_KEYS  # noqa: E402

L, C, T, HEADS = 64, 4, 50, 8
KEYS = [tuple(k) for k in DEFAULT_GUIDANCE_ATTN_KEYS]
BOXES = [(0.10, 0.20, 0.55, 0.70), (0.50, 0.35, 0.95, 0.90), (0.25, 0.10, 0.80, 0.60), (0.05, 0.55, 0.45, 0.98),
         (0.30, 0.30, 0.62, 0.58)]


class Lay:
    def __init__(self, boxes):
        self.boxes, self.overall_groups = boxes, [[i] for i in range(len(boxes))]


class MapShapes:
    """What pipeline._ref_maps reads of a sampler (SD v1.x at 64 x 64 latents)."""

    def __init__(self, dev):
        self.dev = dev

    def map_hw(self, L):
        return {k: (64 if k[0] == "mid" else 256) for k in KEYS}

    def heads_of(self, key):
        return HEADS


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def ab(a, b, iters, windows):
    for _ in range(2):
        a()
        b()
    ta, tb = [], []
    for _ in range(windows):
        ta.append(window(a, iters))
        tb.append(window(b, iters))
    return ta, tb


def stage_a(n_lay, n_box, dev):
    g = torch.Generator().manual_seed(100 * n_lay + n_box)
    hist = torch.randn((T + 1, n_lay * n_box, C, L, L), generator=g).to(dev)
    lays = [Lay([BOXES[(li + i) % len(BOXES)] for i in range(n_box)]) for li in range(n_lay)]
    # per-box generations ran on the centred boxes (so_center_box): the masks sit in the middle, the targets do not
    masks = torch.stack([hostprep.proportion_to_mask(hostprep.get_centered_box(list(b)), L, L).bool()
                         for lay in lays for b in lay.boxes]).to(dev)
    saved = [{k: torch.randn((T, 1, HEADS, 64 if k[0] == "mid" else 256, 1), generator=g).to(dev) for k in KEYS}
             for _ in range(n_lay * n_box)]
    bgs = [torch.randn((1, C, L, L), generator=g) for _ in range(n_lay)]
    return lays, hist, masks, saved, bgs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1x1", "4x2", "4x5"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU")
    dev = torch.device("cuda:0")
    shapes = MapShapes(dev)
    result = dict(latents=L, steps=T, keys=len(KEYS), heads=HEADS, iters=a.iters, windows=a.windows, shapes={})
    for shape in a.shapes:
        n_lay, n_box = (int(v) for v in shape.split("x"))
        lays, hist, masks, saved, bgs = stage_a(n_lay, n_box, dev)
        box_of = [(li, i) for li in range(n_lay) for i in range(n_box)]
        kept = {}

        def on_host():
            m = masks.cpu()                                       # pipeline._stage_a: the composition is host code
            out = []
            for li, lay in enumerate(lays):
                rows = [n for n, (l, _) in enumerate(box_of) if l == li]
                d = dict(latents_all=[hist[:, n:n + 1] for n in rows], masks=[m[n] for n in rows],
                         saved=[dict(saved[n]) for n in rows])
                pipeline._align_stage_a(d, lay, KEYS, True, False)
                composed, fg_idx = hostprep.compose(d["latents_all"], d["masks"], T, bgs[li].to(dev))
                out.append(dict(composed=composed, fg_idx=fg_idx, ref_maps=pipeline._ref_maps(shapes, d["saved"], KEYS, L, T),
                                frozen=(fg_idx != 0)))
            kept["host"] = out

        def on_device():
            out = handoff.run(dev, masks=[[masks[n] for n, (l, _) in enumerate(box_of) if l == li] for li in range(n_lay)],
                              targets=[lay.boxes for lay in lays],
                              histories=[[hist[:, n:n + 1] for n, (l, _) in enumerate(box_of) if l == li] for li in range(n_lay)],
                              saved=[[saved[n] for n, (l, _) in enumerate(box_of) if l == li] for li in range(n_lay)],
                              bgs=bgs, keys=KEYS, L=L, T=T, steps=T, align=True, horizontal_shift_only=False, heads=HEADS,
                              max_hw=256)
            for r in out:
                r["frozen"] = r["fg_idx"] != 0
            kept["device"] = out
        t_host, t_dev = ab(on_host, on_device, a.iters, a.windows)
        same = all(torch.equal(h[name].to(dev), d[name]) for h, d in zip(kept["host"], kept["device"])
                   for name in ("composed", "fg_idx", "ref_maps"))
        med = statistics.median
        r = dict(host_ms=med(t_host), host_ms_min_max=[min(t_host), max(t_host)], device_ms=med(t_dev),
                 device_ms_min_max=[min(t_dev), max(t_dev)], ratio_host_over_device=med(t_host) / med(t_dev),
                 device_wholly_below_host=max(t_dev) < min(t_host), results_equal=bool(same))
        result["shapes"][shape] = r
        print(f"# {n_lay} layouts x {n_box} boxes: host {r['host_ms']:.3f} ms [{min(t_host):.3f}, {max(t_host):.3f}], device "
              f"{r['device_ms']:.3f} ms [{min(t_dev):.3f}, {max(t_dev):.3f}], ratio {r['ratio_host_over_device']:.2f}, "
              f"results equal: {same}", flush=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
