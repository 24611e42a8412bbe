"""Time per call of the two image hops that `ops.resample_u8` (csrc/resample.hip) moves onto the GPU, at the geometries
their consumers use and for N = 1 and N = 8 images that are already on the device as uint8 (N, 512, 512, 3):

  * refiner:   512 -> 1024 LANCZOS, then v / 255 * 2 - 1 in fp32 (generation/sdxl_refinement.py + SDXLRefiner.refine);
  * evaluator: 512 -> 768 BICUBIC, then (v / 255 - mean) / std in fp32 (OwlViTImageProcessor).

In one process two paths ALTERNATE window by window after untimed warm-up calls of every shape:

  * host: what runs without the kernel — `.cpu()`, `PIL.Image.resize` image by image, numpy stack, upload, the float
    expression in torch on the device;
  * device: one `ops.resample_u8` call (two launches, the float form folded into the second).

A window is `iters` calls ended by a device synchronise, timed by the host clock (the host path IS host work).  The two
paths' outputs are compared bit for bit before anything is timed.  Medians and the spread over `--windows` windows are
printed, one JSON line at the end.

    python tools/time_resample.py [--batches 1 8] [--windows 5] [--host-iters 3] [--device-iters 2000]
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
from lgd_amd import ops  # noqa: E402

MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
GEOMETRIES = {"refiner_512_1024_lanczos_unit": (1024, "lanczos", Image.LANCZOS, "unit"),
              "evaluator_512_768_bicubic_affine": (768, "bicubic", Image.BICUBIC, "affine")}


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
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--device-iters", type=int, default=2000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU")
    dev = torch.device("cuda:0")
    mean = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    d255 = torch.tensor(255.0, device=dev)        # a tensor divisor: a true division, as the host computes v / 255 today
    result = dict(source_side=512, windows=a.windows, host_iters=a.host_iters, device_iters=a.device_iters, cases={})
    for name, (side, filt, pil_filt, form) in GEOMETRIES.items():
        for N in a.batches:
            rng = np.random.RandomState(N)
            x = torch.from_numpy(rng.randint(0, 256, (N, 512, 512, 3)).astype(np.uint8)).to(dev)
            out = torch.empty((N, 3, side, side), device=dev)
            scratch = torch.empty((N * 512 * side * 3,), device=dev, dtype=torch.uint8)

            def host():
                imgs = x.cpu().numpy()
                r = np.stack([np.asarray(Image.fromarray(i).resize((side, side), pil_filt)) for i in imgs])
                v = torch.from_numpy(r).to(dev).permute(0, 3, 1, 2).float()
                return v / d255 * 2.0 - 1.0 if form == "unit" else (v * (1 / 255) - mean) / std

            def device():
                return ops.resample_u8(x, (side, side), filt, form, mean=MEAN, std=STD, out=out, scratch=scratch)
            same = bool(torch.equal(host(), device()))
            for _ in range(2):                                     # every shape of the timed windows, untimed
                host()
                device()
            t_host, t_dev = [], []
            for _ in range(a.windows):
                t_host.append(window(host, a.host_iters))
                t_dev.append(window(device, a.device_iters))
            mh, md = statistics.median(t_host), statistics.median(t_dev)
            out_bytes = N * 3 * side * side * 4
            result["cases"][f"{name}/N={N}"] = dict(
                bit_identical=same, host_ms=mh * 1e3, host_ms_min_max=[min(t_host) * 1e3, max(t_host) * 1e3],
                device_ms=md * 1e3, device_ms_min_max=[min(t_dev) * 1e3, max(t_dev) * 1e3], ratio_host_over_device=mh / md,
                device_output_GBps=out_bytes / md / 1e9)
            print(f"# {name} N={N}: host path {mh * 1e3:.3f} ms/call [{min(t_host) * 1e3:.3f}, {max(t_host) * 1e3:.3f}]; "
                  f"resample_u8 {md * 1e3:.4f} ms/call [{min(t_dev) * 1e3:.4f}, {max(t_dev) * 1e3:.4f}] "
                  f"({out_bytes / md / 1e9:.0f} GB/s of fp32 output); host / device = {mh / md:.0f}; "
                  f"outputs bit-identical: {same}", flush=True)
    print(json.dumps(result), flush=True)
    if not all(c["bit_identical"] for c in result["cases"].values()):
        raise SystemExit("the two paths disagree")


if __name__ == "__main__":
    main()
