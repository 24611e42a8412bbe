"""Per-box against batched SAM mask refinement (lgd_amd.sam_refine.SamRefiner.box N times against ONE .boxes call), and the
part after the model on its own: `post_process_masks` + the resize to the latent grid + `_pick` as the per-box path runs
them (device interpolations, then masks and scores to the host, IoU and selection in numpy) against ops.sam_mask_tail on
the same logits.  sam-vit-base geometry with the seeded synthetic weights of `bench.py --sam` (no checkpoint is loaded),
512 x 512 uint8 images already on the device for the batched path and on the host for the per-box path (where each path
finds them in the pipeline), N = 1, 2 and 8.  Both sides of a pair ALTERNATE window by window in one process after untimed
warm-up calls of every shape; a window is `--iters` calls (four times as many for the tail alone) between device synchronisations, timed by device events (the
per-box side synchronises inside every call as well: that is part of what it costs).  Medians over `--windows` windows
and their spread are printed, one JSON line at the end.

    python tools/ab_sam_refine.py [--batches 1 2 8] [--iters 5] [--windows 5] > profiles/sam_refine_batched_timing.txt

`--box-prompt` times the box prompt of an attention map instead (`use_box_input=True`; 16 x 16 maps, N = 8 and 32 unless
`--batches` says otherwise): ONE `attns()` call of a refiner built with `attn_box="device"` (lgd_sam_attn_box_prompt_f32,
the model in chunks, the mask tail) against the per-image `attn()` loop over the same N items (scipy smoothing and opening,
binary_mask_to_box, processor, model, post-processing and selection per image, images and maps on the host where that
path finds them).  `attn()` hands `sam_box_input` a two-level box list, which the processors refuse (lgd_amd.sam_refine's
module docstring); the loop runs it with the box one list level deeper, the one change that lets it return a mask.
`--arms host` times that loop alone and uses nothing this arm's device path added, so the same file also runs against an
older checkout of the package (`--package-root`).

    python tools/ab_sam_refine.py --box-prompt [--arms host device] > profiles/sam_box_prompt_timing.txt
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--package-root" in sys.argv:                                  # another checkout's package (its own built library)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1])
sys.path.insert(0, ROOT)
import lgd_amd  # noqa: E402,F401
from lgd_amd import ops, sam_refine  # noqa: E402
from lgd_amd.hostprep import proportion_to_mask  # noqa: E402

SIDE, GRID = 512, 64
BOXES = [(0.10, 0.20, 0.55, 0.70), (0.50, 0.35, 0.95, 0.90), (0.25, 0.10, 0.80, 0.60), (0.05, 0.55, 0.45, 0.98)]


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
    for _ in range(2):                                             # every shape of the timed windows, untimed
        a()
        b()
    ta, tb = [], []
    for _ in range(windows):
        ta.append(window(a, iters))
        tb.append(window(b, iters))
    return ta, tb


def make_sam(dev):
    import transformers
    torch.manual_seed(0)
    hf = transformers.SamModel(transformers.SamConfig())              # architecture + parameter names; random weights
    with torch.no_grad():
        for name, prm in hf.named_parameters():                       # HF zero-initialises the position tables
            if "pos" in name:
                prm.normal_(0.0, 0.02)
    return sam_refine.wrap_sam(hf, "device", device=dev)


def box_prompt(a, md, dev):
    """The box prompt of an attention map: N x attn() against one attns(attn_box="device")."""
    kw = dict(height=SIDE, width=SIDE, use_box_input=True)         # sigma 0.1, th 0.05, one erosion / dilation: lmd.py's
    per_image = sam_refine.SamRefiner(md, batched=False, **kw)
    device = sam_refine.SamRefiner(md, batched=True, attn_box="device", **kw) if "device" in a.arms else None
    real = sam_refine.sam_box_input
    sam_refine.sam_box_input = lambda m, image, input_boxes, **k: real(m, image, [[list(input_boxes[0])]], **k)
    g = torch.Generator().manual_seed(11)
    result = dict(geometry="sam-vit-base", image=SIDE, grid=GRID, map=16, arms=a.arms, iters=a.iters, windows=a.windows,
                  package_root=os.path.relpath(ROOT, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), batches={})
    med = statistics.median
    for N in a.batches or [8, 32]:
        low = torch.rand(N, 3, 16, 16, generator=g)
        imgs = (F.interpolate(low, size=(SIDE, SIDE), mode="bicubic", align_corners=False).clamp(0, 1) * 255).round().byte()
        host = np.ascontiguousarray(imgs.permute(0, 2, 3, 1).numpy())
        on_dev = torch.from_numpy(host).to(dev)
        # one blob per map, away from the border: bicubic of a 4 x 4 seed whose largest entry is inside
        seed = torch.rand(N, 1, 4, 4, generator=g) * 0.2
        for n in range(N):
            seed[n, 0, 1 + n % 2, 1 + (n // 2) % 2] = 1.0
        maps = F.interpolate(seed, size=(16, 16), mode="bicubic", align_corners=False)[:, 0].clamp_min(0).contiguous()
        maps_np, maps_dev = maps.numpy(), maps.to(dev)
        kept = []

        def one_by_one():
            kept.append([per_image.attn(host[n], maps_np[n])[1] for n in range(N)])

        def in_one():
            kept.append(device.attns(on_dev, maps_dev)[1])
        with contextlib.redirect_stdout(io.StringIO()):           # _pick prints every choice it makes
            if device is None:
                t_one, _ = ab(one_by_one, lambda: None, a.iters, a.windows)
                t_dev = None
            elif "host" not in a.arms:
                t_dev, _ = ab(in_one, lambda: None, a.iters, a.windows)
                t_one = None
            else:
                t_one, t_dev = ab(one_by_one, in_one, a.iters, a.windows)
        r = {}
        line = f"# box prompt, N={N}:"
        if t_one:
            r.update(per_image_ms=med(t_one), per_image_ms_min_max=[min(t_one), max(t_one)])
            line += f" {N} x attn() {r['per_image_ms']:.3f} ms [{min(t_one):.3f}, {max(t_one):.3f}]"
        if t_dev:
            r.update(device_ms=med(t_dev), device_ms_min_max=[min(t_dev), max(t_dev)])
            line += f" one attns(attn_box='device') {r['device_ms']:.3f} ms [{min(t_dev):.3f}, {max(t_dev):.3f}]"
        if t_one and t_dev:
            r.update(ratio_per_image_over_device=med(t_one) / med(t_dev))
            line += f" ratio {r['ratio_per_image_over_device']:.2f}"
        result["batches"][str(N)] = r
        print(line, flush=True)
        del kept[:]
    sam_refine.sam_box_input = real
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=None)
    ap.add_argument("--box-prompt", action="store_true")
    ap.add_argument("--arms", nargs="+", choices=["host", "device"], default=["host", "device"])
    ap.add_argument("--package-root", default=None)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU")
    dev = torch.device("cuda:0")
    md = make_sam(dev)
    if a.box_prompt:
        return box_prompt(a, md, dev)
    a.batches = a.batches or [1, 2, 8]
    per_box = sam_refine.SamRefiner(md, height=SIDE, width=SIDE, batched=False)
    batched = sam_refine.SamRefiner(md, height=SIDE, width=SIDE, batched=True)
    proc = md["sam_processor"]
    g = torch.Generator().manual_seed(7)
    result = dict(geometry="sam-vit-base", image=SIDE, grid=GRID, iters=a.iters, windows=a.windows, batches={})
    for N in a.batches:
        low = torch.rand(N, 3, 16, 16, generator=g)
        imgs = (F.interpolate(low, size=(SIDE, SIDE), mode="bicubic", align_corners=False).clamp(0, 1) * 255).round().byte()
        host = np.ascontiguousarray(imgs.permute(0, 2, 3, 1).numpy())
        on_dev = torch.from_numpy(host).to(dev)
        boxes = [BOXES[n % len(BOXES)] for n in range(N)]
        kept = []

        def one_by_one():
            kept.append([per_box.box(host[n], boxes[n])[1] for n in range(N)])

        def in_one():
            kept.append(batched.boxes(on_dev, boxes)[1])
        quiet = contextlib.redirect_stdout(io.StringIO())         # _pick prints every choice it makes
        with quiet:
            t_one, t_bat = ab(one_by_one, in_one, a.iters, a.windows)

        # the part after the model, on the logits of one forward pass
        enc = proc(on_dev, input_boxes=[[[b[0] * SIDE, b[1] * SIDE, b[2] * SIDE, b[3] * SIDE]] for b in boxes])
        out = md["sam_model"](**enc)
        logits, iou = out.pred_masks[:, 0].float().contiguous(), out.iou_scores[:, 0].float().contiguous()
        coarse_np = [proportion_to_mask(b, GRID, GRID, return_np=True) for b in boxes]
        coarse = torch.from_numpy(np.stack(coarse_np).astype(np.uint8)).to(dev)
        geom = torch.tensor([[SIDE, SIDE, 1024, 1024]] * N, dtype=torch.int32, device=dev)
        sizes, resh = torch.tensor([[SIDE, SIDE]]), torch.tensor([[1024, 1024]])

        def host_tail():
            for n in range(N):                                     # what sam() and _pick do after the model, per box
                full = proc.post_process_masks(logits[n:n + 1, None], sizes, resh)
                conf = iou[n].cpu().numpy()
                small = F.interpolate(full[0].float(), (GRID, GRID), mode="bilinear").bool().cpu().numpy()
                kept.append(sam_refine._pick(small[0], conf, coarse_np[n], 0.85, 0.25)[1])

        def kernel_tail():
            kept.append(ops.sam_mask_tail(logits, iou, geom, 1024, (GRID, GRID), coarse, 0.85, 0.25)[1])
        with quiet:                                               # short calls: four times as many per window
            t_host, t_kern = ab(host_tail, kernel_tail, 4 * a.iters, a.windows)
        med = statistics.median
        r = dict(per_box_ms=med(t_one), per_box_ms_min_max=[min(t_one), max(t_one)], batched_ms=med(t_bat),
                 batched_ms_min_max=[min(t_bat), max(t_bat)], ratio_per_box_over_batched=med(t_one) / med(t_bat),
                 host_tail_ms=med(t_host), host_tail_ms_min_max=[min(t_host), max(t_host)], kernel_tail_ms=med(t_kern),
                 kernel_tail_ms_min_max=[min(t_kern), max(t_kern)], ratio_host_tail_over_kernel=med(t_host) / med(t_kern))
        result["batches"][str(N)] = r
        print(f"# N={N}: whole call: {N} x box() {r['per_box_ms']:.3f} ms [{min(t_one):.3f}, {max(t_one):.3f}], one boxes() "
              f"{r['batched_ms']:.3f} ms [{min(t_bat):.3f}, {max(t_bat):.3f}], ratio {r['ratio_per_box_over_batched']:.2f}; "
              f"after the model: host tail {r['host_tail_ms']:.3f} ms [{min(t_host):.3f}, {max(t_host):.3f}], kernel tail "
              f"{r['kernel_tail_ms']:.4f} ms [{min(t_kern):.4f}, {max(t_kern):.4f}], ratio {r['ratio_host_tail_over_kernel']:.1f}",
              flush=True)
        del kept[:]
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
