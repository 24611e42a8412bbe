"""The hand-off between the two stages of LMD / LMD+ on the device (csrc/handoff.hip): centre-of-mass alignment
(utils/latents.py:85-118), composition of the box histories (utils/latents.py:38-83), the shift of the saved maps
(utils/attn.py:40-70) and their gather into the energy kernel's reference tensor (utils/guidance.py:201), for ALL layouts
of a batch in three launches.  The host code that does the same box by box is hostprep.align_with_bboxes / compose and
pipeline._align_stage_a / _ref_maps; results are element for element the same.

What happens on the host here is table packing only: addresses and strides of the histories and maps stage A left on the
device, the target boxes, the layout segments.  The tables go up in one non-blocking copy from pinned memory in front of
the launches; nothing is read back.

One defined difference: a box whose (shifted) mask is empty makes the host code raise ValueError('The mask is empty').  A
launch cannot raise without a read, so here such a box is skipped — it owns no pixel — and row 7 of its plan row says so.
"""
import numpy as np
import torch

from . import ops

F32 = torch.float32
MODES = ("host", "device")
# What handoff=None resolves to when stage A's masks are already device tensors (the batched refiner).  The measured
# default: tools/ab_handoff.py, DESIGN.md (d) "The hand-off on the device".
DEFAULT_WITH_DEVICE_MASKS = "device"


def resolve(handoff, masks_on_device):
    """The `handoff` keyword of the pipelines -> "host" or "device".  None: the device path exactly when stage A's masks
    are device tensors already, so that no path pays a copy the other would not."""
    if handoff is None:
        return DEFAULT_WITH_DEVICE_MASKS if masks_on_device else "host"
    if handoff not in MODES:
        raise ValueError(f"handoff must be one of {MODES} or None (got {handoff!r})")
    return handoff


def _upload(host, dev):
    return host.to(dev, non_blocking=True)


def _staging(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, pin_memory=dev.type == "cuda")


def pack_tables(arrays, dev):
    """numpy arrays (int32 / int64 / float64) -> device tensors of the same shapes: one pinned staging buffer with 8-byte
    aligned sections, one non-blocking copy."""
    spans, total = [], 0
    for a in arrays:
        spans.append((total, a.nbytes))
        total += (a.nbytes + 7) // 8 * 8
    host = _staging((max(total, 8),), torch.uint8, dev)
    for a, (off, n) in zip(arrays, spans):
        if n:
            host[off:off + n].copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)))
    buf = _upload(host, dev)
    kinds = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.float64): torch.float64}
    return [buf[off:off + n].view(kinds[a.dtype]).reshape(a.shape) for a, (off, n) in zip(arrays, spans)]


def masks_as_one(masks, L, dev):
    """The boxes' (L, L) masks -> one uint8 [NB, L, L] device tensor.  Device masks that are consecutive rows of one
    tensor (the batched refiner's output) are taken as they lie; host masks are stacked and uploaded once."""
    if not masks:
        return torch.zeros((0, L, L), dtype=torch.uint8, device=dev)
    masks = [torch.as_tensor(m) for m in masks]
    if any(tuple(m.shape) != (L, L) for m in masks):
        raise ValueError(f"every mask must be {(L, L)}")
    if any(m.device != masks[0].device for m in masks):
        raise ValueError("the masks of one batch must live on one device")
    first = masks[0]
    if first.device.type == "cpu" and dev.type != "cpu":
        host = _staging((len(masks), L, L), torch.uint8, dev)
        for row, m in zip(host, masks):
            row.copy_(m != 0)
        return _upload(host, dev)
    if first.dtype in (torch.bool, torch.uint8) and all(
            m.dtype == first.dtype and m.is_contiguous() and m._base is not None and m._base is first._base
            and m.storage_offset() == first.storage_offset() + n * L * L for n, m in enumerate(masks)):
        one = first.as_strided((len(masks), L, L), (L * L, L, 1))
    else:
        one = torch.stack([m != 0 for m in masks])
    return one.view(torch.uint8) if one.dtype == torch.bool else one


def _history_row(h, L, need):
    if h.dtype != F32 or h.dim() != 5 or h.shape[1] != 1 or tuple(h.shape[3:]) != (L, L) \
            or tuple(h.stride()[2:]) != (L * L, L, 1):
        raise ValueError("a history is an fp32 [rows, 1, C, L, L] tensor or view whose images are contiguous")
    if h.shape[0] < need:
        raise ValueError(f"a history of {h.shape[0]} rows cannot feed a composition of {need}")
    return h.data_ptr(), h.stride(0)


def _map_row(m, heads, align):
    if m.dtype != F32 or m.dim() != 5 or m.shape[1] != 1 or m.shape[2] != heads or m.shape[4] != 1 or not m.is_contiguous():
        raise ValueError("a saved map is a contiguous fp32 [rows, 1, heads, side * side, 1] tensor")
    side = int(round(m.shape[3] ** 0.5))
    if side * side != m.shape[3]:
        raise ValueError(f"a saved map of {m.shape[3]} pixels is not square")
    if align and side % 8:
        raise AssertionError(f"{side, side} is not a multiple of (8, 8)")            # as shift_tensor asserts
    return m.data_ptr(), m.shape[0], side


def run(dev, *, masks, targets, histories, saved, bgs, keys, L, T, steps, align, horizontal_shift_only,
        heads=None, max_hw=None):
    """All layouts of a batch.  Per layout (lists of equal length NL): masks[l] = its boxes' (L, L) masks, targets[l] = the
    xyxy box each will occupy (the flattened overall boxes), histories[l] = fp32 [rows, 1, C, L, L] tensors or views,
    saved[l] = per box {key: fp32 [rows, 1, heads, side^2, 1]}, bgs[l] = the background latent (1, C, L, L).  steps: the
    composition's (rows >= steps + 1).  heads / max_hw: of the reference maps (None: none are made).

    -> per layout dict(composed [steps + 1, 1, C, L, L], fg_idx int64 [L, L], ref_maps [T, n, len(keys), heads, max_hw] or
    None, latents_all = the aligned histories [rows, 1, C, L, L] per box (the given ones with align off), plan int32 [n, 8]),
    all views of per-batch device tensors."""
    dev = torch.device(dev)
    NL = len(bgs)
    counts = [len(m) for m in masks]
    if not (len(masks) == len(targets) == len(histories) == len(saved) == NL) or NL == 0:
        raise ValueError("one entry per layout, at least one layout")
    if any(len(t) != n or len(h) != n for t, h, n in zip(targets, histories, counts)):
        raise ValueError("every box of a layout brings a mask, a target box and a history")
    seg = np.zeros(NL + 1, dtype=np.int32)
    seg[1:] = np.cumsum(counts)
    NB = int(seg[-1])
    lay_of = np.repeat(np.arange(NL, dtype=np.int32), counts)
    flat_hist = [h for per in histories for h in per]
    hist = np.array([_history_row(h, L, steps + 1) for h in flat_hist], dtype=np.int64).reshape(NB, 2)
    tgt = np.array([list(map(float, t)) for per in targets for t in per], dtype=np.float64).reshape(NB, 4)
    want_maps = heads is not None and NB > 0
    tables = [seg, lay_of, tgt, hist]
    if want_maps:
        if any(len(s) != n for s, n in zip(saved, counts)):
            raise ValueError("every box of a layout brings its saved maps")
        tables.append(np.array([_map_row(s[tuple(k)], heads, align) for per in saved for s in per for k in keys],
                               dtype=np.int64).reshape(NB, len(keys), 3))
        if int(tables[-1][:, :, 2].max()) ** 2 > max_hw:
            raise ValueError("a saved map is larger than max_hw")
    rows = None
    if align and NB:
        rows = flat_hist[0].shape[0]
        if any(h.shape[0] != rows for h in flat_hist):
            raise ValueError("aligned histories are returned as one tensor: every history must have the same rows")
    if any(h.device != dev for h in flat_hist):
        raise ValueError("the histories live on the device of the hand-off")

    seg_d, lay_of_d, tgt_d, hist_d, *maps_d = pack_tables(tables, dev)
    bg_h = [torch.as_tensor(b) for b in bgs]
    C = bg_h[0].shape[-3]
    if all(b.device.type == "cpu" for b in bg_h):
        stage = _staging((NL, C, L, L), F32, dev)
        for row, b in zip(stage, bg_h):
            row.copy_(b.reshape(C, L, L))
        bg = _upload(stage, dev)
    else:
        bg = torch.cat([b.reshape(1, C, L, L).to(dev, F32) for b in bg_h])
    masks_d = masks_as_one([m for per in masks for m in per], L, dev)

    plan, win = ops.handoff_place(masks_d, tgt_d, seg_d, max(counts), align=align,
                                  horizontal_shift_only=horizontal_shift_only)
    composed, fg_idx, aligned = ops.handoff_compose(plan, win, seg_d, hist_d, bg, steps, rows=rows)
    ref = ops.handoff_ref_maps(plan, seg_d, lay_of_d, maps_d[0], T, heads, max_hw, L) if want_maps else None

    out = []
    per_box = T * len(keys) * heads * max_hw if want_maps else 0
    for l in range(NL):
        b0, b1 = int(seg[l]), int(seg[l + 1])
        lat = [aligned[b].unsqueeze(1) for b in range(b0, b1)] if aligned is not None else list(histories[l])
        out.append(dict(composed=composed[l].unsqueeze(1), fg_idx=fg_idx[l], plan=plan[b0:b1], latents_all=lat,
                        ref_maps=(ref[b0 * per_box:b1 * per_box].view(T, b1 - b0, len(keys), heads, max_hw)
                                  if want_maps else None)))
    return out
