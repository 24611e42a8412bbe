"""Images per second of `HipOwlViTDetector.detect()` — the stage-2 evaluator's forward + post_process + score filter +
NMS — at google/owlvit-base-patch32 geometry (768 x 768 images, 576 tokens, `OwlViTConfig()` defaults) with seeded
synthetic weights (tests/owl_detect_cases.redraw_weights; no checkpoint is loaded), Q = 4 queries per image, B = 1 and
B = 8, graphs off.  In the same process transformers' own `OwlViTForObjectDetection` runs in fp16 on the same GPU (its
forward only: no post_process, no NMS), the two ALTERNATING window by window after untimed warm-up calls of every
shape; a window is `--iters` calls between device synchronisations, timed by device events.  Medians and the spread
over `--windows` windows are printed, one JSON line at the end.

    python tools/time_owlvit.py [--batches 1 8] [--iters 20] [--windows 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lgd_amd  # noqa: E402,F401
import owl_detect_cases as cases  # noqa: E402
from lgd_amd import owlvit  # noqa: E402

Q = 4


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU")
    import transformers
    dev = torch.device("cuda:0")
    cfg = transformers.OwlViTConfig()
    hf = cases.redraw_weights(transformers.OwlViTForObjectDetection(cfg), seed=3)
    det = owlvit.from_hf(hf, dev)
    hf = hf.to(dev).half()
    result = dict(geometry="base-patch32", tokens=det.P, queries=Q, iters=a.iters, windows=a.windows, batches={})
    for B in a.batches:
        pv, ids = cases.model_inputs(cfg, B, Q, seed=4)
        pv, ids = pv.to(dev), ids.to(dev)
        pv16, mask = pv.half(), (ids > 0).long()
        kept = []

        def ours():
            kept.append(sum(det.detect(pv, ids, score_threshold=0.1, nms_threshold=0.5).counts))

        def theirs():
            with torch.no_grad():
                return hf(input_ids=ids, pixel_values=pv16, attention_mask=mask).logits
        for _ in range(3):                                         # every shape of the timed windows, untimed
            ours()
            theirs()
        t_ours, t_theirs = [], []
        for _ in range(a.windows):
            t_ours.append(window(ours, a.iters))
            t_theirs.append(window(theirs, a.iters))
        mo, mt = statistics.median(t_ours), statistics.median(t_theirs)
        r = dict(detect_ms=mo * 1e3, detect_ms_min_max=[min(t_ours) * 1e3, max(t_ours) * 1e3],
                 detect_images_per_s=B / mo, transformers_fp16_forward_ms=mt * 1e3,
                 transformers_ms_min_max=[min(t_theirs) * 1e3, max(t_theirs) * 1e3],
                 transformers_images_per_s=B / mt, ratio_transformers_over_detect=mt / mo, boxes_kept_per_call=kept[-1])
        result["batches"][str(B)] = r
        print(f"# B={B}: detect() {mo * 1e3:.3f} ms/call [{min(t_ours) * 1e3:.3f}, {max(t_ours) * 1e3:.3f}] = "
              f"{B / mo:.1f} images/s; transformers fp16 forward {mt * 1e3:.3f} ms/call "
              f"[{min(t_theirs) * 1e3:.3f}, {max(t_theirs) * 1e3:.3f}] = {B / mt:.1f} images/s", flush=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
