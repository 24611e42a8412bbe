"""ORACLE TEST INFRASTRUCTURE (needs the reference tree; CPU) — golden of the detection tail of the stage-2 evaluator.

Imports the reference's OWN, unmodified utils/eval/eval.py (by file path: it needs numpy, PIL and torch only) and, for
every case of tests/owl_detect_cases.py, builds model-shaped inputs (logits [B, P, Q], cxcywh boxes [B, P, 4], fp32),
states `post_process` in fp64 (owl_detect_cases.post_process64), applies the score filter of eval.py:144-148 and calls
the reference's `nms` / `class_aware_nms` on the fp64 candidates.  Recorded per case: the inputs, and per flavour
(plain / class-aware x thresholds 0.05 / 0.5 and 0.3 / 0.3) the counts, kept token indices, labels, scores and boxes in
the reference's output order.

Inputs are built so that fp64 and fp32 arithmetic cannot legitimately disagree, and that is ASSERTED
(owl_detect_cases.check_margins): per-token best logits are a permutation of an evenly spaced grid in [-3, 3] (score
gaps >= 1e-4), no score lies within 1e-4 of a score threshold (the grid is shifted until that holds), boxes are redrawn
until no pairwise IoU lies within 1e-4 of an NMS threshold, and no box is degenerate.

    python tools/make_golden_owl_detect.py [--out PATH]
"""
import argparse
import importlib.util
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import owl_detect_cases as cases  # noqa: E402
import ref_harness as rh  # noqa: E402


def load_reference_eval():
    path = os.path.join(rh.REF_ROOT, "utils", "eval", "eval.py")
    spec = importlib.util.spec_from_file_location("ref_utils_eval_eval", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def best_logits(rng, P, kind):
    lo, hi = (-6.0, -4.0) if kind == "below" else (-3.0, 3.0)
    grid = np.linspace(lo, hi, P) if P > 1 else np.zeros(1)
    for shift in np.arange(0.0, 0.05, 0.00017):                 # move the grid off the score thresholds
        s = 1.0 / (1.0 + np.exp(-(grid + shift).astype(np.float32).astype(np.float64)))
        if min(np.abs(s - t).min() for t in cases.SCORE_THRESHOLDS) >= 1.2 * cases.MARGIN:
            return rng.permutation(grid + shift)
    raise AssertionError("no grid shift clears the score thresholds")


def draw_boxes(rng, n, kind, P):
    if kind == "disjoint":                                      # one box inside each cell of a grid
        g = int(np.ceil(np.sqrt(P)))
        cell = 1.0 / g
        ix, iy = np.arange(P) % g, np.arange(P) // g
        return np.stack([(ix + 0.5) * cell, (iy + 0.5) * cell, np.full(P, 0.5 * cell) + 0.2 * cell * rng.random(P),
                         np.full(P, 0.5 * cell) + 0.2 * cell * rng.random(P)], axis=-1)[:n]
    if kind == "identical":
        return np.array([0.5, 0.5, 0.4, 0.3]) + 2e-3 * rng.random((n, 4))
    cxy = 0.15 + 0.7 * rng.random((n, 2))
    wh = 0.08 + 0.3 * rng.random((n, 2))
    return np.concatenate([cxy, wh], axis=-1)


def image_inputs(rng, c, masked_q):
    P, Q, kind = c["P"], c["Q"], c["kind"]
    best = best_logits(rng, P, kind)
    live = [q for q in range(Q) if q != masked_q]
    labels = rng.choice(live, size=P)
    logits = best[:, None] - 0.1 - 2.0 * rng.random((P, Q))     # the others stay at least 0.1 below the best
    logits[np.arange(P), labels] = best
    logits = logits.astype(np.float32)
    if masked_q is not None:
        logits[:, masked_q] = cases.FMIN
    boxes = draw_boxes(rng, P, kind, P).astype(np.float32)
    for _ in range(200):                                        # redraw the boxes of every IoU too close to a threshold
        iou = cases.iou_matrix(cases.post_process64(logits, boxes)[2])
        np.fill_diagonal(iou, -1.0)
        bad = np.zeros(P, bool)
        for t in cases.NMS_THRESHOLDS:
            bad |= (np.abs(iou - t) < 2 * cases.MARGIN).any(axis=1)
        if not bad.any():
            break
        boxes[bad] = draw_boxes(rng, int(bad.sum()), kind, P).astype(np.float32)
    cases.check_margins(logits, boxes)
    return logits, boxes


def run_flavour(ref, logits, boxes, class_aware, score_thr, nms_thr):
    """One image through the reference: returns (kept token indices, labels, scores, boxes) in its output order."""
    scores, labels, xyxy = cases.post_process64(logits, boxes)
    keep = scores >= score_thr                                   # eval.py:144-148
    cand = np.nonzero(keep)[0]
    fn = ref.class_aware_nms if class_aware else ref.nms
    with redirect_stdout(io.StringIO()):
        pb, ps, pl = fn(xyxy[keep], scores[keep], labels[keep], nms_thr)
    pb, ps, pl = np.asarray(pb, np.float64).reshape(-1, 4), np.asarray(ps, np.float64), np.asarray(pl, np.int64)
    by_score = {float(scores[i]): int(i) for i in cand}          # scores are distinct (asserted margins)
    assert len(by_score) == len(cand)
    index = np.array([by_score[float(s)] for s in ps], np.int64)
    assert np.array_equal(xyxy[index], pb) and np.array_equal(labels[index], pl)
    return index, pl, ps, pb


def build_arrays():
    ref = load_reference_eval()
    arrs = {}
    for ci, c in enumerate(cases.CASES):
        rng = np.random.default_rng(1000 + ci)
        B, P, Q = c["B"], c["P"], c["Q"]
        per = [image_inputs(rng, c, c["masked"][1] if c["masked"] and c["masked"][0] == b else None) for b in range(B)]
        logits, boxes = np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
        arrs[f"{c['name']}/logits"], arrs[f"{c['name']}/pred_boxes"] = logits, boxes
        for name, aware, st, nt in cases.FLAVOURS:
            count = np.zeros(B, np.int64)
            index = np.full((B, P), -1, np.int64)
            labels = np.full((B, P), -1, np.int64)
            scores, out = np.zeros((B, P)), np.zeros((B, P, 4))
            for b in range(B):
                i, l, s, bx = run_flavour(ref, logits[b], boxes[b], aware, st, nt)
                n = count[b] = len(i)
                index[b, :n], labels[b, :n], scores[b, :n], out[b, :n] = i, l, s, bx
            for k, v in (("count", count), ("index", index), ("labels", labels), ("scores", scores), ("boxes", out)):
                arrs[f"{c['name']}/{name}/{k}"] = v
            print(f"{c['name']:>18} {name}: kept {count.tolist()} of {P}")
    return arrs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "owl_detect_cases.npz"))
    a = ap.parse_args()
    np.savez_compressed(a.out, **build_arrays())
    print("wrote", a.out)
