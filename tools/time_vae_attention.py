"""Time of the VAE's mid-block attention under attention = "materialised" (three batched GEMMs + a row softmax over an fp16
score matrix) and attention = "streamed" (two GEMMs for q | k and v, one lgd_attn_wide_f16 launch), on the SD decoder's
architecture with seeded synthetic weights (vae.synth_aekl_state_dict: mid-block width 512):

  * `_Blocks._attn` alone — GroupNorm, projections, attention, to_out — at S = 4096 (64 x 64 latent) with B = 1 and B = 8,
    and at S = 16384 (128 x 128 latent, the refiner's 1024^2 pass) with B = 1;
  * a whole decode of a 1 x 4 x 64 x 64 latent.

Both arms run in one process, ALTERNATING window by window after untimed warm-up calls of every shape; a window is `--iters`
calls between device synchronisations, timed by device events.  Medians and the spread over `--windows` windows are
printed, one JSON line at the end.

    python tools/time_vae_attention.py [--iters 10] [--windows 5]
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
from lgd_amd import vae  # noqa: E402

MODES = vae.ATTENTION_MODES
SHAPES = [(1, 64), (8, 64), (1, 128)]          # (B, latent side): S = side^2


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1000.0 / iters


def alternate(fns, iters, windows):
    """{mode: [seconds per call of each window]}, the modes taking turns."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    times = {m: [] for m in fns}
    for _ in range(windows):
        for m, fn in fns.items():
            times[m].append(window(fn, iters))
    return times


def report(label, times, result):
    med = {m: statistics.median(t) for m, t in times.items()}
    result[label] = {m: dict(ms=med[m] * 1e3, ms_min_max=[min(times[m]) * 1e3, max(times[m]) * 1e3]) for m in times}
    result[label]["streamed_over_materialised"] = med["streamed"] / med["materialised"]
    print(f"# {label}: " + "; ".join(f"{m} {med[m] * 1e3:.3f} ms [{min(times[m]) * 1e3:.3f}, {max(times[m]) * 1e3:.3f}]" for m in times)
          + f"; streamed / materialised = {med['streamed'] / med['materialised']:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU")
    dev = torch.device("cuda:0")
    sd = vae.synth_aekl_state_dict(seed=0)
    hips = {m: vae.HipVAEDecoder(sd, dev, attention=m) for m in MODES}
    C = hips[MODES[0]].c_mid
    result = dict(width=C, iters=a.iters, windows=a.windows)
    for B, L in SHAPES:
        x = (torch.randn((B * L * L, C), generator=torch.Generator().manual_seed(B + L)) * 0.5).to(dev, torch.float16)
        fns = {m: (lambda h=h: h._attn(h.attn, x, B, L, L)) for m, h in hips.items()}
        report(f"mid-block attention S={L * L} B={B}", alternate(fns, a.iters, a.windows), result)
        del x, fns
        torch.cuda.empty_cache()
    z = torch.randn((1, 4, 64, 64), generator=torch.Generator().manual_seed(3)) * 0.9
    report("decode 1x4x64x64", alternate({m: (lambda h=h: h.decode(z)) for m, h in hips.items()}, max(1, a.iters // 2), a.windows), result)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
