"""Golden of the box-prompt branch of the reference's `models/sam.py` (sam_refine_attn with use_box_input=True, :125-172):
what its own `preprocess_mask` and `utils.binary_mask_to_box` compute from an attention map, and what its own
`get_iou_with_resize` + `select_mask` then select among fixed candidates.

Runs where the reference checkout is available (oracle/ref_harness.py), on the CPU.  The reference's unmodified
`sam_refine_attn` is called; the only stand-in is `sam_box_input`, which records the box it is handed and answers with
candidates cut from a seeded field around the map's mass — the reference hands the processor a two-level box list there, which
transformers refuses, so the network cannot be part of this golden (and need not be: it is neither smoothing, opening, box
nor selection).  `preprocess_mask` is wrapped to record the opened mask it returns.  `cv2` is oracle/stubs/cv2.py (same-size
resize = identity, the case these inputs produce).

Writes tests/golden/sam_refine_attn_box.npz — data only: the settings, the attention maps, and per case the opened coarse
mask, the box, the candidates with their predicted IoUs, the selected mask and its confidence.

    python tools/make_golden_sam_box_prompt.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as H  # noqa: E402
import sam_cases  # noqa: E402

KW = dict(height=512, width=512, H=64, W=64, discourage_mask_below_confidence=0.85, discourage_mask_below_coarse_iou=0.2)
# (gaussian_sigma, mask_th_for_box, n_erode_dilate_mask_for_box, maps): generation/lmd.py's settings for the box prompt on
# the two maps that keep every normalised value 1e-4 away from 0.05, and a setting all four maps keep clear of
SETTINGS = [(0.1, 0.05, 1, (2, 3)), (0.1, 0.2, 1, (0, 1, 2, 3)), (1.5, 0.3, 3, (0, 1, 2, 3))]
CONF = np.array([[0.91, 0.88, 0.95], [0.80, 0.90, 0.86], [0.97, 0.70, 0.89], [0.86, 0.87, 0.60]], dtype=np.float32)


def candidates(a, n):
    """Three nested 64 x 64 candidates around the map's own mass (so that their IoUs with the coarse mask lie on both sides
    of the threshold): the heavily smoothed, normalised map plus a seeded smooth perturbation, cut at three levels."""
    from scipy import ndimage
    g = torch.Generator().manual_seed(100 + n)
    low = torch.randn(1, 1, 8, 8, generator=g)
    noise = torch.nn.functional.interpolate(low, size=(64, 64), mode="bicubic", align_corners=False)[0, 0].numpy()
    field = ndimage.gaussian_filter(a.astype(float), sigma=3.0)
    field = (field - field.min()) / (field.max() - field.min()) + 0.04 * noise
    return np.stack([field > t for t in (0.03, 0.2, 0.55)])


def main():
    H.setup()
    from models import sam as ref_sam
    attn = [np.asarray(a, dtype=np.float32) for a in sam_cases.refine_inputs()[2]]
    image = np.zeros((512, 512, 3), dtype=np.uint8)                # never looked at: the stand-in answers
    seen = {}
    real_pre = ref_sam.preprocess_mask

    def pre(*a, **k):
        seen["coarse"] = real_pre(*a, **k)
        return seen["coarse"]

    def box_input(model_dict, image, input_boxes, target_mask_shape, **_k):
        seen["box"] = [int(v) for v in input_boxes[0]]
        assert tuple(target_mask_shape) == (64, 64)
        return [seen["cand"][None]], seen["conf"]
    ref_sam.preprocess_mask, ref_sam.sam_box_input = pre, box_input
    out = dict(maps=np.stack(attn), settings=np.array([s[:3] for s in SETTINGS], dtype=np.float64), conf=CONF,
               cand=np.stack([candidates(attn[n], n) for n in range(4)]),
               below=np.array([KW["discourage_mask_below_confidence"], KW["discourage_mask_below_coarse_iou"]]))
    cases = []
    for si, (sigma, th, n_open, which) in enumerate(SETTINGS):
        for n in which:
            seen.update(cand=out["cand"][n], conf=CONF[n])
            m, c = ref_sam.sam_refine_attn(sam_input_image=image, token_attn_np=attn[n], model_dict=None, use_box_input=True,
                                           gaussian_sigma=sigma, mask_th_for_box=th, n_erode_dilate_mask_for_box=n_open,
                                           mask_th_for_point=0.25, verbose=False, **KW)
            k = len(cases)
            cases.append((si, n))
            out[f"coarse{k}"], out[f"box{k}"] = np.asarray(seen["coarse"]).astype(np.uint8), np.array(seen["box"], dtype=np.int64)
            out[f"mask{k}"], out[f"picked_conf{k}"] = np.asarray(m).astype(np.uint8), np.float32(c)
            print(f"case {k}: setting {si} map {n}: {int(out[f'coarse{k}'].sum())} coarse pixels, box {seen['box']}, "
                  f"selected area {int(out[f'mask{k}'].sum())}, conf {float(c):.2f}")
    out["cases"] = np.array(cases, dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", "sam_refine_attn_box.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
