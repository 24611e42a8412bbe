"""Shared by the tests of csrc/sam_tail.hip: seeded inputs and the HOST statement of what the kernels compute — the
repository's own functions (lgd_amd.sam_refine) run with torch on the CPU, which is what the per-box path runs today."""
import numpy as np
import torch
import torch.nn.functional as F

import lgd_amd  # noqa: F401
from lgd_amd import sam_refine

OFFSETS = (0.5, 1.0, 2.0)
BELOW_CONF, BELOW_IOU = 0.85, 0.2
AMBIGUOUS_CAP = 1e-3           # at most 0.1 % of a case's latent-grid pixels may sit within 1e-4 of a threshold


def make_logits(N, S, seed, K=3):
    """Smooth blobs with both signs: randn at S/8, bicubic to S, x4, minus a different constant per candidate (so that
    the candidates nest and differ in area, as SAM's three masks do)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(N, K, S // 8, S // 8, generator=g)
    up = F.interpolate(low, size=(S, S), mode="bicubic", align_corners=False) * 4
    return (up - torch.tensor(OFFSETS[:K]).view(1, K, 1, 1)).contiguous()


def geom_of(h, w, target):
    nh, nw = sam_refine.DeviceSamProcessor("cpu", longest_edge=target)._shape(h, w)
    return [h, w, nh, nw]


def host_candidates(logits_item, geom, target, grid):
    """post_process_masks + the resize to the latent grid of sam_refine.sam(), fp32 on the CPU -> bool (K, H, W)."""
    h, w, nh, nw = geom
    proc = sam_refine.DeviceSamProcessor("cpu", longest_edge=target)
    full = proc.post_process_masks(logits_item[None, None], [[h, w]], [[nh, nw]])
    return F.interpolate(full[0].float(), grid, mode="bilinear").bool()[0].numpy()


def ambiguous(logits_item, geom, target, grid):
    """Latent-grid pixels (K, H, W) whose value changes when the h x w image is thresholded at +1e-4 instead of -1e-4,
    with the whole chain in fp64: there the rounding of an fp32 chain may decide."""
    h, w, nh, nw = geom
    m = F.interpolate(logits_item.double()[None], (target, target), mode="bilinear", align_corners=False)
    m = F.interpolate(m[..., :nh, :nw], (h, w), mode="bilinear", align_corners=False)
    lo = F.interpolate((m > -1e-4).double(), grid, mode="bilinear").bool()
    hi = F.interpolate((m > 1e-4).double(), grid, mode="bilinear").bool()
    return (lo != hi)[0].numpy()


def host_select(cand, iou_row, coarse, below_conf=BELOW_CONF, below_iou=BELOW_IOU):
    """get_iou_with_resize + select_mask on bool candidates (K, H, W) -> dict(mask, conf, pick, area, inter, union,
    ious).  The counts restate hostprep.iou's two sums (its quotient is what get_iou_with_resize returns)."""
    coarse = np.asarray(coarse).astype(bool)
    ious = sam_refine.get_iou_with_resize(coarse, cand, masks_shape=coarse.shape)
    mask, conf = sam_refine.select_mask(cand, iou_row, coarse_ious=ious, rule="largest_over_conf",
                                        discourage_mask_below_confidence=below_conf,
                                        discourage_mask_below_coarse_iou=below_iou)
    c = cand
    if cand.shape[1:] != coarse.shape:
        t = torch.from_numpy(cand.astype(np.float32))[:, None]
        c = (F.interpolate(t, coarse.shape, mode="bilinear", align_corners=False)[:, 0] > 0).numpy()
    inter = np.logical_and(coarse[None], c).reshape(len(c), -1).sum(1)
    union = np.logical_or(coarse[None], c).reshape(len(c), -1).sum(1)
    assert np.array_equal(ious, inter / (union + 1e-6))
    area = cand.reshape(len(cand), -1).sum(1)
    score = area - area.max() * (iou_row < below_conf) - area.max() * (ious < below_iou)
    pick = int(np.argmax(score))
    assert np.array_equal(mask, cand[pick]) and conf == iou_row[pick]
    return dict(mask=mask, conf=conf, pick=pick, area=area, inter=inter, union=union, ious=ious)


def box_coarse(hc, wc, frac=(0.2, 0.25, 0.8, 0.75)):
    m = np.zeros((hc, wc), dtype=np.uint8)
    x0, y0, x1, y1 = frac
    m[int(y0 * hc):max(int(y1 * hc), int(y0 * hc) + 1), int(x0 * wc):max(int(x1 * wc), int(x0 * wc) + 1)] = 1
    return m


def block_mean(a, hm, wm):
    h, w = a.shape
    return a.reshape(hm, h // hm, wm, w // wm).mean(axis=(1, 3)).astype(np.float32)
