"""Cases of tests/golden/owl_detect_cases.npz (tools/make_golden_owl_detect.py), shared by the generator and the tests:
the shapes, the flavours, the fp64 statement of `post_process` and the margin conditions under which the reference's
fp64 arithmetic and an fp32 kernel cannot legitimately disagree."""
import numpy as np

MARGIN = 1e-4
# name, B, P, Q, masked (image, query) or None, kind
CASES = [
    dict(name="p1", B=1, P=1, Q=1, masked=None, kind="random"),
    dict(name="p36_q3_b2_masked", B=2, P=36, Q=3, masked=(1, 2), kind="random"),
    dict(name="p65", B=1, P=65, Q=2, masked=None, kind="random"),
    dict(name="p576_q5", B=1, P=576, Q=5, masked=None, kind="random"),
    dict(name="p1000_q1", B=1, P=1000, Q=1, masked=None, kind="random"),
    dict(name="all_below", B=1, P=36, Q=3, masked=None, kind="below"),
    dict(name="disjoint", B=1, P=36, Q=3, masked=None, kind="disjoint"),
    dict(name="near_identical", B=1, P=36, Q=3, masked=None, kind="identical"),
]
# name, class_aware, score threshold, NMS threshold
FLAVOURS = [("plain_005_05", False, 0.05, 0.5), ("plain_03_03", False, 0.3, 0.3),
            ("aware_005_05", True, 0.05, 0.5), ("aware_03_03", True, 0.3, 0.3)]
SCORE_THRESHOLDS = (0.05, 0.3)
NMS_THRESHOLDS = (0.5, 0.3)
FMIN = float(np.finfo(np.float32).min)


def post_process64(logits, pred_boxes):
    """fp64 statement of OwlViTImageProcessor.post_process on ONE image with target size 1 x 1: logits [P, Q] and cxcywh
    boxes [P, 4] (fp32 inputs, widened) -> (scores, labels, xyxy boxes)."""
    lg = logits.astype(np.float64)
    labels = lg.argmax(axis=-1)
    scores = 1.0 / (1.0 + np.exp(-lg.max(axis=-1)))
    cx, cy, w, h = (pred_boxes.astype(np.float64)[:, i] for i in range(4))
    return scores, labels, np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], axis=-1)


def iou_matrix(xyxy):
    """Pairwise inter / (area_i + area_j - inter) in fp64, as utils/eval/eval.py:58-73 computes one row of it."""
    x0, y0, x1, y1 = (xyxy[:, i] for i in range(4))
    area = (x1 - x0) * (y1 - y0)
    w = np.maximum(0.0, np.minimum(x1[:, None], x1[None]) - np.maximum(x0[:, None], x0[None]))
    h = np.maximum(0.0, np.minimum(y1[:, None], y1[None]) - np.maximum(y0[:, None], y0[None]))
    inter = w * h
    return inter / (area[:, None] + area[None] - inter)


def margins(logits, pred_boxes):
    """The conditions of one image: (smallest gap between two scores, smallest distance of a score to a score threshold,
    smallest distance of a pairwise IoU to an NMS threshold, smallest box side)."""
    scores, _, xyxy = post_process64(logits, pred_boxes)
    s = np.sort(scores)
    gap = float(np.diff(s).min()) if len(s) > 1 else np.inf
    thr = float(min(np.abs(scores - t).min() for t in SCORE_THRESHOLDS))
    iou = iou_matrix(xyxy)[np.triu_indices(len(scores), 1)]
    nms = float(min(np.abs(iou - t).min() for t in NMS_THRESHOLDS)) if iou.size else np.inf
    side = float(min((xyxy[:, 2] - xyxy[:, 0]).min(), (xyxy[:, 3] - xyxy[:, 1]).min()))
    return gap, thr, nms, side


def check_margins(logits, pred_boxes):
    gap, thr, nms, side = margins(logits, pred_boxes)
    assert gap >= MARGIN, f"score gap {gap:.3e}"
    assert thr >= MARGIN, f"score within {thr:.3e} of a score threshold"
    assert nms >= MARGIN, f"IoU within {nms:.3e} of an NMS threshold"
    assert side >= 1e-3, f"degenerate box, side {side:.3e}"
    return gap, thr, nms, side


# ---- model cases (transformers' OwlViTForObjectDetection with seeded synthetic weights)
def tiny_hf_config():
    """Image 96, patch 16 (36 tokens); vision 96 wide, 3 heads; text 64 wide, 2 heads, 16 positions; vocab 1000 with the
    EOS id the highest; projection 64."""
    from transformers import OwlViTConfig
    return OwlViTConfig(
        text_config=dict(vocab_size=1000, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                         num_attention_heads=2, max_position_embeddings=16, pad_token_id=0, bos_token_id=998,
                         eos_token_id=999),
        vision_config=dict(hidden_size=96, intermediate_size=192, num_hidden_layers=2, num_attention_heads=3,
                           image_size=96, patch_size=16),
        projection_dim=64)


def redraw_weights(model, seed):
    """Default init saturates every score to 0 or 1.  Matrices uniform +-fan_in^-0.5, biases 0.05 * randn, LayerNorm
    weights 1 + 0.05 * randn, class-head logit_shift bias 0 and logit_scale bias 1."""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("class_head.logit_shift.bias"):
                p.zero_()
            elif name.endswith("class_head.logit_scale.bias"):
                p.fill_(1.0)
            elif p.dim() >= 2:
                fan_in = p[0].numel()
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * fan_in ** -0.5)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.05 * torch.randn(p.shape, generator=g))
            elif name.endswith("class_embedding"):
                p.copy_(torch.randn(p.shape, generator=g) * p.numel() ** -0.5)
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return model.eval()


def model_inputs(cfg, B, Q, seed, zero_rows=()):
    """pixel_values (B, 3, S, S) and input_ids (B*Q, 16): BOS, a few word ids, EOS (the highest id), zero padding; the
    rows in `zero_rows` are all zero (padded queries)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    t = cfg.text_config
    S = cfg.vision_config.image_size
    pixel_values = torch.randn(B, 3, S, S, generator=g)
    ids = torch.zeros(B * Q, t.max_position_embeddings, dtype=torch.int64)
    for r in range(B * Q):
        if r in zero_rows:
            continue
        n = 2 + int(torch.randint(0, 6, (1,), generator=g))
        ids[r, 0] = t.bos_token_id
        ids[r, 1:1 + n] = torch.randint(1, t.bos_token_id, (n,), generator=g)
        ids[r, 1 + n] = t.eos_token_id
    return pixel_values, ids
