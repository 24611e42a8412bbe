"""Shared by tests/test_handoff_cpu.py and tests/test_handoff_gpu.py: seeded stage-A results, the host path as the
reference (hostprep.align_with_bboxes + compose, pipeline._align_stage_a + _ref_maps, all on the CPU), and a torch / numpy
restatement of the three ops of csrc/handoff.hip written from the rules of include/lgd_hip.h — it stands in for the
kernels where there is no GPU."""
import numpy as np
import torch

from lgd_amd import hostprep, pipeline

KEYS = [("mid", 0, 0, 0), ("up", 1, 0, 0)]           # map sides 8 and 16 at L = 16 .. 64
L, C, STEPS, T, HEADS = 16, 4, 3, 4, 2
SIDES = {KEYS[0]: 8, KEYS[1]: 16}


class Lay:
    """What the hand-off reads of a CachedLayout."""

    def __init__(self, boxes):
        self.boxes = [tuple(b) for b in boxes]
        self.overall_groups = [[i] for i in range(len(boxes))]


class HostSampler:
    """What pipeline._ref_maps reads of a sampler."""

    def __init__(self, sides=SIDES, heads=HEADS, dev="cpu"):
        self.sides, self.heads, self.dev = sides, heads, torch.device(dev)

    def map_hw(self, L):
        return {k: s * s for k, s in self.sides.items()}

    def heads_of(self, key):
        return self.heads


def rect(x0, y0, x1, y1, L=L):
    m = torch.zeros(L, L, dtype=torch.bool)
    m[y0:y1, x0:x1] = True
    return m


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def stage_a(masks_per_layout, targets_per_layout, seed=0, *, L=L, C=C, hist_rows=STEPS + 1, map_rows=T, chunks=1,
            keys=KEYS, sides=SIDES, heads=HEADS):
    """Stage-A results on the CPU for layouts with the given masks: histories are views `hist[:, b:b+1]` of `chunks`
    batch tensors (as LMDSampler.denoise_batch returns them), saved maps [map_rows, 1, heads, side^2, 1]."""
    n = sum(len(m) for m in masks_per_layout)
    per_chunk = -(-n // chunks) if n else 0
    batches = [seeded((hist_rows, min(per_chunk, n - c * per_chunk), C, L, L), seed + 10 + c)
               for c in range(chunks) if n - c * per_chunk > 0]
    lays, per_lay, b = [], [], 0
    for li, (masks, targets) in enumerate(zip(masks_per_layout, targets_per_layout)):
        d = dict(latents_all=[], masks=[], saved=[])
        for m in masks:
            batch, col = batches[b // per_chunk], b % per_chunk
            d["latents_all"].append(batch[:, col:col + 1])
            d["masks"].append(m.clone())
            d["saved"].append({k: seeded((map_rows, 1, heads, sides[k] ** 2, 1), seed + 1000 + 10 * b + ki)
                               for ki, k in enumerate(keys)})
            b += 1
        lays.append(Lay(targets))
        per_lay.append(d)
    bgs = [seeded((1, C, L, L), seed + 500 + li) for li in range(len(lays))]
    return lays, per_lay, bgs, batches


def to_device(per_lay, bgs, batches, dev):
    """The same stage-A results on `dev`, histories again views of the (moved) batch tensors."""
    moved = [b.to(dev) for b in batches]
    index = {}
    for bi, b in enumerate(batches):
        for col in range(b.shape[1]):
            index[b[:, col:col + 1].data_ptr()] = (bi, col)
    out = []
    for d in per_lay:
        hist = []
        for h in d["latents_all"]:
            bi, col = index[h.data_ptr()]
            hist.append(moved[bi][:, col:col + 1])
        out.append(dict(latents_all=hist, masks=[m.to(dev) for m in d["masks"]],
                        saved=[{k: v.to(dev) for k, v in s.items()} for s in d["saved"]]))
    return out, [b.to(dev) for b in bgs], moved


def host_path(lays, per_lay, bgs, *, keys=KEYS, L=L, T=T, steps=STEPS, align, horizontal_shift_only, sampler=None):
    """The host hand-off as pipeline._stage_b runs it, on copies: per layout dict(composed, fg_idx, ref_maps, latents_all,
    offsets in pixels)."""
    sampler = sampler or HostSampler()
    out = []
    for lay, d, bg in zip(lays, per_lay, bgs):
        d = dict(latents_all=list(d["latents_all"]), masks=[m.clone() for m in d["masks"]],
                 saved=[dict(s) for s in d["saved"]])
        offsets = []
        if align:
            for m, t in zip(d["masks"], lay.boxes):
                cx, cy = hostprep.binary_mask_to_center(m, normalize=True)
                x_off = (t[0] + t[2]) / 2 - cx
                y_off = 0. if horizontal_shift_only else (t[1] + t[3]) / 2 - cy
                offsets.append((round(x_off * 8) * (L // 8), round(y_off * 8) * (L // 8)))
        else:
            offsets = [(0, 0)] * len(d["masks"])
        pipeline._align_stage_a(d, lay, keys, align, horizontal_shift_only)
        composed, fg_idx = hostprep.compose(d["latents_all"], d["masks"], steps, bg)
        ref = pipeline._ref_maps(sampler, d["saved"], keys, L, T) if d["saved"] else None
        out.append(dict(composed=composed, fg_idx=fg_idx, ref_maps=ref, latents_all=d["latents_all"], offsets=offsets,
                        areas=[int(m.sum()) for m in d["masks"]]))
    return out


def distinct_areas(host):
    """np.argsort leaves the order of equal (shifted) areas open, so the host path is a reference only without them; the
    tie rule of the device path has its own test."""
    return all(len(set(h["areas"])) == len(h["areas"]) for h in host)


def compose_in_order(histories, masks, order, steps, bg):
    """The composition rule with the painter's order given: step 0 takes the grown bounding box of each (already
    shifted) mask in turn, then every step takes the masks in turn."""
    composed = torch.zeros((steps + 1, *bg.shape))
    composed[0] = bg
    fg_idx = torch.zeros(bg.shape[-2:], dtype=torch.long)
    for i in order:
        box = hostprep.binary_mask_to_box_mask(masks[i]).bool()
        composed[0][..., box] = histories[i][0][..., box]
    for i in order:
        composed[..., masks[i]] = histories[i][:steps + 1][..., masks[i]]
        fg_idx[masks[i]] = i + 1
    return composed, fg_idx


# -------------------------------------------------------------------------------------------------
# the three ops, restated from the header's rules (CPU tensors; addresses are resolved through `roots`)
# -------------------------------------------------------------------------------------------------
class Restated:
    """Drop-in for lgd_amd.ops.handoff_place / handoff_compose / handoff_ref_maps.  roots: the CPU tensors the address
    tables may point into (batch tensors of histories, saved maps)."""

    def __init__(self, roots):
        self.roots = [(r.data_ptr(), r.data_ptr() + r.numel() * 4, r) for r in roots if r.numel()]
        self.calls = []

    def _at(self, address, size, stride):
        for lo, hi, r in self.roots:
            if lo <= address < hi:
                assert r.dtype == torch.float32 and r.is_contiguous() and (address - lo) % 4 == 0
                return torch.as_strided(r, size, stride, (address - lo) // 4)
        raise AssertionError(f"address {address:#x} is in no known tensor")

    def handoff_place(self, masks, targets, seg, max_boxes, *, align, horizontal_shift_only):
        self.calls.append("place")
        masks = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        assert masks.dtype == torch.uint8 and targets.dtype == torch.float64 and seg.dtype == torch.int32
        NB, L = masks.shape[0], masks.shape[1]
        if L % 8:
            raise RuntimeError("lgd_handoff_place failed: invalid argument")
        seg = seg.numpy()
        assert int(seg[-1]) == NB == targets.shape[0] and max(np.diff(seg), default=0) == max_boxes
        plan = np.zeros((NB, 8), dtype=np.int32)
        win = np.full((len(seg) - 1, 2, L, L), -1, dtype=np.int32)
        ys, xs = np.mgrid[0:L, 0:L]
        shifted = np.zeros((NB, L, L), dtype=bool)
        for b in range(NB):
            m = masks[b].numpy() != 0
            n, sx, sy = int(m.sum()), int(xs[m].sum()), int(ys[m].sum())
            ox = oy = 0
            if align and n:
                t = targets[b].numpy()
                cx = float(np.float32(sx) / np.float32(n)) / L
                cy = float(np.float32(sy) / np.float32(n)) / L
                ox = round(((t[0] + t[2]) / 2 - cx) * 8) * (L // 8)
                oy = 0 if horizontal_shift_only else round(((t[1] + t[3]) / 2 - cy) * 8) * (L // 8)
            src_y, src_x = ys - oy, xs - ox
            ok = (src_y >= 0) & (src_y < L) & (src_x >= 0) & (src_x < L)
            shifted[b][ok] = m[src_y[ok], src_x[ok]]
            area = int(shifted[b].sum())
            if area:
                yy, xx = np.nonzero(shifted[b])
                plan[b] = [ox, oy, area, max(xx.min() - 1, 0), max(yy.min() - 1, 0), min(xx.max() + 1, L),
                           min(yy.max() + 1, L), 0]
            else:
                plan[b] = [ox, oy, 0, 0, 0, -1, -1, 1]
        for l in range(len(seg) - 1):
            boxes = list(range(seg[l], seg[l + 1]))
            for b in sorted(boxes, key=lambda b: -plan[b, 2]):                        # sorted() is stable
                if plan[b, 7]:
                    continue
                win[l, 0][shifted[b]] = b - seg[l]
                win[l, 1][(xs >= plan[b, 3]) & (xs <= plan[b, 5]) & (ys >= plan[b, 4]) & (ys <= plan[b, 6])] = b - seg[l]
        return torch.from_numpy(plan), torch.from_numpy(win)

    def _shift(self, img, ox, oy):
        """img [..., L, L] read at (y - oy, x - ox), zero outside."""
        L = img.shape[-1]
        out = torch.zeros_like(img)
        ys = [y for y in range(L) if 0 <= y - oy < L]
        xs = [x for x in range(L) if 0 <= x - ox < L]
        if ys and xs:
            out[..., ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = img[..., ys[0] - oy:ys[-1] - oy + 1, xs[0] - ox:xs[-1] - ox + 1]
        return out

    def handoff_compose(self, plan, win, seg, hist, bg, steps, *, rows=None):
        self.calls.append("compose")
        NL, C, L = bg.shape[0], bg.shape[1], bg.shape[2]
        NB = plan.shape[0]
        need = rows if rows is not None else steps + 1
        shifted = [self._shift(self._at(int(hist[b, 0]), (max(need, steps + 1), C, L, L), (int(hist[b, 1]), L * L, L, 1)),
                               int(plan[b, 0]), int(plan[b, 1])) for b in range(NB)]
        composed = torch.zeros((NL, steps + 1, C, L, L))
        fg_idx = torch.zeros((NL, L, L), dtype=torch.int64)
        for l in range(NL):
            wm, wb = win[l, 0], win[l, 1]
            composed[l, 0] = bg[l]
            for b in range(int(seg[l]), int(seg[l + 1])):
                local = b - int(seg[l])
                by_box = ((wm < 0) & (wb == local)).expand(C, L, L)
                composed[l, 0][by_box] = shifted[b][0][by_box]
            for b in range(int(seg[l]), int(seg[l + 1])):
                local = b - int(seg[l])
                own = (wm == local).expand(steps + 1, C, L, L)
                composed[l][own] = shifted[b][:steps + 1][own]
            fg_idx[l] = (wm + 1).long()
        aligned = torch.stack([s[:rows] for s in shifted]) if rows is not None and NB else None
        return composed, fg_idx, aligned

    def handoff_ref_maps(self, plan, seg, lay_of, maps, T, heads, max_hw, L):
        self.calls.append("ref_maps")
        NB, NK = maps.shape[0], maps.shape[1]
        out = torch.zeros(NB * T * NK * heads * max_hw)
        per_box = T * NK * heads * max_hw
        for b in range(NB):
            l = int(lay_of[b])
            b0, nb = int(seg[l]), int(seg[l + 1]) - int(seg[l])
            view = out[b0 * per_box:(b0 + nb) * per_box].view(T, nb, NK, heads, max_hw)
            for k in range(NK):
                rows, side = int(maps[b, k, 1]), int(maps[b, k, 2])
                m = self._at(int(maps[b, k, 0]), (rows, heads, side, side), (heads * side * side, side * side, side, 1))
                eighth = L // 8
                sh = self._shift(m, int(plan[b, 0]) // eighth * (side // 8), int(plan[b, 1]) // eighth * (side // 8))
                n = min(T, rows)
                view[:n, b - b0, k, :, :side * side] = sh[:n].reshape(n, heads, side * side)
        return out


# -------------------------------------------------------------------------------------------------
# seeded random layouts (0, 1 and 5 boxes; overlapping masks)
# -------------------------------------------------------------------------------------------------
def random_layouts(seed, counts=(0, 1, 5), L=L):
    """Per layout: masks = a solid rectangle plus a few stray pixels (so centres are non-trivial fractions), targets with
    their centres in the middle half of the frame (no mask leaves the frame entirely)."""
    rng = np.random.RandomState(seed)
    masks, targets = [], []
    for n in counts:
        ms, ts = [], []
        for _ in range(n):
            w, h = rng.randint(3, L // 2 + 1, size=2)
            x0, y0 = rng.randint(0, L - w + 1), rng.randint(0, L - h + 1)
            m = rect(x0, y0, x0 + w, y0 + h, L)
            for _ in range(3):
                m[min(max(y0 + rng.randint(-1, h + 1), 0), L - 1), min(max(x0 + rng.randint(-1, w + 1), 0), L - 1)] = True
            cx, cy = rng.uniform(0.3, 0.7, size=2)
            bw, bh = rng.uniform(0.1, 0.5, size=2)
            ms.append(m)
            ts.append((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2))
        masks.append(ms)
        targets.append(ts)
    return masks, targets


def same(a, b):
    """torch.equal across devices (the sign of a zero is open: torch.equal compares -0 == +0 as equal)."""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())
