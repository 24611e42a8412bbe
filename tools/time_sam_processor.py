"""Time per call of SAM's preprocessing on the device, `DeviceSamProcessor.pixels`, for the two resizes it offers, on
N = 1 and N = 8 images that are already on the device as uint8 (N, 512, 512, 3) (what stage A hands the refiner):

  * torch:  resize="torch", the default — F.interpolate, round / clamp, divide, subtract / divide, pad: separate torch
    launches, each a full pass over the fp32 tensor;
  * pillow: resize="pillow" — one `ops.resample_u8` call (csrc/resample.hip): two launches, the second writes the
    normalised, zero-padded (N, 3, 1024, 1024) tensor once.

Both go through the same public entry, allocations included.  In one process the two ALTERNATE window by window after
untimed warm-up calls; a window is `--iters` calls ended by one device synchronise, timed by the host clock; the median and
the spread over `--windows` windows are printed, one JSON line at the end.  Before anything is timed the outputs are
compared: "pillow" bit for bit with the affine expression on PIL.Image.resize's own bytes, and "torch" against it (they
differ by design: the share of pixels off by half an 8-bit level or more is printed).

    python tools/time_sam_processor.py [--batches 1 8] [--windows 5] [--iters 2000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgd_amd  # noqa: E402,F401
from lgd_amd.sam_refine import DeviceSamProcessor  # noqa: E402


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU")
    dev = torch.device("cuda:0")
    procs = {"torch": DeviceSamProcessor(dev, resize="torch"), "pillow": DeviceSamProcessor(dev, resize="pillow")}
    mean = torch.tensor(DeviceSamProcessor.MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(DeviceSamProcessor.STD, device=dev).view(1, 3, 1, 1)
    level = 1.0 / 255.0 / max(DeviceSamProcessor.STD)
    result = dict(source_side=512, target=1024, windows=a.windows, iters=a.iters, cases={})
    for N in a.batches:
        rng = np.random.RandomState(N)
        host = rng.randint(0, 256, (N, 512, 512, 3)).astype(np.uint8)
        x = torch.from_numpy(host).to(dev)
        pil = np.stack([np.asarray(Image.fromarray(i).resize((1024, 1024), Image.BILINEAR)) for i in host])
        exact = (torch.from_numpy(pil).to(dev).permute(0, 3, 1, 2).float() * (1 / 255) - mean) / std
        fns = {k: (lambda p=p: p.pixels(x)[0]) for k, p in procs.items()}
        same = bool(torch.equal(fns["pillow"](), exact))
        diff = (fns["torch"]() - exact).abs()
        off = float((diff >= 0.5 * level).float().mean())
        for _ in range(3):                                         # every shape of the timed windows, untimed
            for fn in fns.values():
                fn()
        t = {k: [] for k in fns}
        for _ in range(a.windows):
            for k, fn in fns.items():
                t[k].append(window(fn, a.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        out_bytes = N * 3 * 1024 * 1024 * 4
        result["cases"][f"N={N}"] = dict(
            pillow_bit_identical_to_pil=same, torch_share_off_half_level=off, torch_max_abs_diff=float(diff.max()),
            torch_ms=med["torch"] * 1e3, torch_ms_min_max=[min(t["torch"]) * 1e3, max(t["torch"]) * 1e3],
            pillow_ms=med["pillow"] * 1e3, pillow_ms_min_max=[min(t["pillow"]) * 1e3, max(t["pillow"]) * 1e3],
            ratio_torch_over_pillow=med["torch"] / med["pillow"], pillow_output_GBps=out_bytes / med["pillow"] / 1e9)
        print(f"# N={N}: torch {med['torch'] * 1e3:.4f} ms/call [{min(t['torch']) * 1e3:.4f}, {max(t['torch']) * 1e3:.4f}]; "
              f"pillow {med['pillow'] * 1e3:.4f} ms/call [{min(t['pillow']) * 1e3:.4f}, {max(t['pillow']) * 1e3:.4f}] "
              f"({out_bytes / med['pillow'] / 1e9:.0f} GB/s of fp32 output); torch / pillow = {med['torch'] / med['pillow']:.2f}; "
              f"pillow bit-identical to the expression on PIL's bytes: {same}; torch pixels off by >= half a level: "
              f"{100 * off:.1f} %", flush=True)
    print(json.dumps(result), flush=True)
    if not all(c["pillow_bit_identical_to_pil"] for c in result["cases"].values()):
        raise SystemExit("resize='pillow' is not Pillow's arithmetic")


if __name__ == "__main__":
    main()
