"""Shared by the tests of lgd_sam_attn_box_prompt_f32 (csrc/sam_tail.hip): the cases and a numpy restatement of what the
kernel computes that does not use scipy — the Gaussian smoothing with `reflect` borders, the min-max threshold, the
opening as explicit loops over the 4 neighbours with a zero border, and the grown bounding box.
tests/test_sam_box_prompt_cpu.py checks the restatement against scipy.ndimage and hostprep.binary_mask_to_box; the GPU
test checks the kernel against the restatement AND against scipy.

Threshold margin.  An opening spreads one flipped pixel to its neighbours, so no pixel may be left out of a comparison
here (the point-prompt test leaves a band out).  A (map, sigma, mask_th) item is used only if no normalised fp64 value
lies within MARGIN = 1e-4 of the threshold — the kernel's fp32 smoothing is within 1e-6 of fp64 — and `natural_cases`
asserts it.  Of the 64 x 64, 16 x 16, 8 x 8 and 8 x 12 maps of tests/test_sam_tail_gpu.py at sigma in {0.1, 1.5} and
mask_th in {0.05, 0.25} that leaves out the items listed in LEFT_OUT (1, 2 or 4 pixels at the threshold each); among the
rest the opening changes masks (16 x 16, sigma 0.1, th 0.25: 29 -> 28 -> 24 -> 0 pixels for n_open = 0..3) and empties
them (8 x 8 from n_open = 2 on)."""
import numpy as np

import lgd_amd  # noqa: F401
import sam_cases
import sam_tail_cases as tc

SIDE = 512                      # image side the prompts are scaled to: up_w = SIDE // wm, up_h = SIDE // hm
MARGIN = 1e-4
SIGMAS, THRESHOLDS, OPENS = (0.1, 1.5), (0.05, 0.25), (0, 1, 2, 3)
MIN_NATURAL = 30
# (maps, sigma, mask_th) -> the map indices with a normalised value within MARGIN of the threshold
LEFT_OUT = {("64x64", 0.1, 0.05): (0, 1), ("64x64", 0.1, 0.25): (3,), ("64x64", 1.5, 0.05): (0, 1, 2),
            ("64x64", 1.5, 0.25): (3,), ("16x16", 0.1, 0.05): (1, 3)}


# ---- the restatement (fp64, no scipy)
def smooth(a, sigma):
    """scipy.ndimage.gaussian_filter with its defaults: radius int(4 sigma + 0.5), weights exp(-x^2 / 2 sigma^2) / sum,
    axis 0 then axis 1, mode `reflect` (d c b a | a b c d | d c b a) at any distance."""
    a = np.asarray(a, dtype=np.float64)
    r = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x * x)
    w /= w.sum()
    for axis in (0, 1):
        n = a.shape[axis]
        out = np.zeros_like(a)
        for j in range(-r, r + 1):
            idx = (np.arange(n) + j) % (2 * n)
            idx = np.where(idx < n, idx, 2 * n - 1 - idx)
            out += w[j + r] * np.take(a, idx, axis=axis)
        a = out
    return a


def normalised(s):
    """(s - min) / max(s - min), or None for a constant map (the reference divides 0 by 0 there: NaN > th is False)."""
    d = s - s.min()
    return None if d.max() == 0 else d / d.max()


def step(mask, erode):
    """One erosion or dilation with the pixel and its 4 neighbours; everything outside the map is 0."""
    h, w = mask.shape
    pad = np.zeros((h + 2, w + 2), dtype=bool)                    # the zero border
    pad[1:-1, 1:-1] = mask
    out = pad[1:-1, 1:-1].copy()
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):             # the 4 neighbours, one at a time
        near = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        out = (out & near) if erode else (out | near)
    return out


def opened(mask, n_open):
    mask = np.asarray(mask).astype(bool)
    for erode in [True] * n_open + [False] * n_open:
        mask = step(mask, erode)
    return mask


def grown_box(mask, up_w, up_h):
    """utils.binary_mask_to_box(enlarge_box_by_one=True, w_scale=up_w, h_scale=up_h) with loops -> ([x0, y0, x1, y1],
    empty): the zero box and True where the mask has no pixel (the reference raises there)."""
    h, w = mask.shape
    ys = [y for y in range(h) for x in range(w) if mask[y, x]]
    xs = [x for y in range(h) for x in range(w) if mask[y, x]]
    if not ys:
        return [0, 0, 0, 0], True
    ymin, ymax = max(min(ys) - 1, 0), min(max(ys) + 1, h)
    xmin, xmax = max(min(xs) - 1, 0), min(max(xs) + 1, w)
    return [xmin * up_w, ymin * up_h, xmax * up_w, ymax * up_h], False


def scales(hm, wm):
    """sam_refine_attn's (w, h) naming: up_w = height // wm, up_h = width // hm."""
    return SIDE // wm, SIDE // hm


def restate(a, sigma, mask_th, n_open):
    """One map -> dict(smooth fp64, coarse bool, box [4], empty bool, near = pixels within MARGIN of the threshold)."""
    s = smooth(a, sigma)
    nrm = normalised(s)
    if nrm is None:
        first, near = np.zeros(s.shape, dtype=bool), 0
    else:
        first, near = nrm > mask_th, int((np.abs(nrm - mask_th) < MARGIN).sum())
    coarse = opened(first, n_open)
    box, empty = grown_box(coarse, *scales(*s.shape))
    return dict(smooth=s, coarse=coarse, box=box, empty=empty, near=near, before=int(first.sum()))


# ---- natural maps: those of tests/test_sam_tail_gpu.py::_prompt_maps
def natural_maps():
    big = sam_cases.refine_inputs()[2]
    return {"64x64": np.stack(big).astype(np.float32), "16x16": np.stack([tc.block_mean(a, 16, 16) for a in big]),
            "8x8": np.stack([tc.block_mean(a, 8, 8) for a in big]), "8x12": tc.block_mean(big[0][:, :48], 8, 12)[None]}


_NATURAL = None


def natural_cases():
    """[(name, sigma, mask_th, n_open, maps fp32 [N, hm, wm], [restate(...)] * N)]: every combination of the four map
    sets, SIGMAS, THRESHOLDS and OPENS, with the items of LEFT_OUT taken out.  Built once; nobody changes it."""
    global _NATURAL
    if _NATURAL is not None:
        return _NATURAL
    cases, pixels = [], []
    for name, maps in natural_maps().items():
        for sigma in SIGMAS:
            for th in THRESHOLDS:
                near = [restate(m, sigma, th, 0)["near"] for m in maps]
                # the filter is the rule, LEFT_OUT is what it gives for these maps: both are pinned
                assert tuple(i for i, k in enumerate(near) if k) == LEFT_OUT.get((name, sigma, th), ()), (name, sigma, th, near)
                keep = [i for i, k in enumerate(near) if not k]
                assert keep, (name, sigma, th)
                for n_open in OPENS:
                    want = [restate(maps[i], sigma, th, n_open) for i in keep]
                    assert all(w["near"] == 0 for w in want)
                    cases.append((name, sigma, th, n_open, np.ascontiguousarray(maps[keep]), want))
                    pixels.append((name, sigma, th, n_open, [int(w["coarse"].sum()) for w in want]))
    assert len(cases) >= MIN_NATURAL, len(cases)
    # every outcome is reached: masks the opening leaves alone, masks it changes, masks it empties
    flat = [(w["before"], int(w["coarse"].sum())) for c in cases if c[3] > 0 for w in c[5]]
    assert any(b == a for b, a in flat) and any(0 < a < b for b, a in flat) and any(a == 0 < b for b, a in flat)
    trace = {p[3]: p[4][0] for p in pixels if p[:3] == ("16x16", 0.1, 0.25)}
    assert [trace[n] for n in OPENS] == [29, 28, 24, 0], trace
    _NATURAL = cases
    return cases


def natural_ids():
    return [f"{name}-s{sigma}-th{th}-open{n_open}" for name in ("64x64", "16x16", "8x8", "8x12") for sigma in SIGMAS
            for th in THRESHOLDS for n_open in OPENS]


# ---- synthetic maps: 0 / 1 valued, sigma 0.1 (radius 0: the filter is the identity), mask_th 0.5
SYN_SIGMA, SYN_TH = 0.1, 0.5


def _blank(h, w):
    return np.zeros((h, w), dtype=np.float32)


def synthetic_maps():
    """name -> (map fp32 [h, w], {n_open: pixels of the opened mask} for the outcomes the case is there for)."""
    out = {}
    out["1x1"] = (np.ones((1, 1), np.float32), {0: 0, 1: 0})                  # constant: empty whatever the threshold
    a = _blank(1, 5)
    a[0, 1:4] = 1
    out["1x5"] = (a, {0: 3, 1: 0})                                            # no row above or below: all of it erodes
    out["5x1"] = (np.ascontiguousarray(a.T), {0: 3, 1: 0})
    a = np.ones((3, 3), np.float32)
    a[0, 0] = 0
    out["3x3"] = (a, {0: 8, 1: 5, 2: 0})                                      # one erosion leaves the centre: PLUS_3X3
    a = _blank(12, 12)
    a[4:8, :] = 1
    a[:, 4:8] = 1
    out["cross_on_all_borders"] = (a, {0: 80, 1: 72, 2: 40})                  # 4 wide arms; the rows ON the border erode, and a
    #                                                                           4-neighbour dilation does not return the 8 tip corners
    a = _blank(12, 12)
    a[5, 7] = 1
    out["lone_pixel"] = (a, {0: 1, 1: 0})
    a = _blank(12, 12)
    a[2:7, 1:4] = 1
    a[2:7, 8:11] = 1
    a[4, 4:8] = 1
    out["bridge"] = (a, {0: 34, 1: BRIDGE_AFTER})                            # the 1-pixel bridge is cut in BRIDGE_GAP; its ends grow back
    out["constant"] = (np.full((12, 12), 0.37, np.float32), {0: 0, 1: 0, 3: 0})
    a = np.ones((12, 12), np.float32)
    a[6, 3] = 0
    out["all_but_one"] = (a, {0: 143})
    return out


BRIDGE_GAP, BRIDGE_AFTER = ((4, 5), (4, 6)), 24
PLUS_3X3 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)   # the 3 x 3 case at n_open = 1, by hand: the centre
#                                                                       survives (its 4 neighbours are set) and dilates


def batches():
    """Launches of N = 1, 4 and 67 items: [(label, maps [N, h, w], sigma, th, n_open)].  N = 4: the four 12 x 12 shapes
    in one launch, each with its own outcome.  N = 67 (more items than a wave has lanes, more than a few CUs' worth of
    workgroups): the four 16 x 16 natural maps at sigma 0.1 / th 0.25 — none within 2e-3 of the threshold — rolled to
    67 different positions; a roll moves the values, not the normalisation."""
    syn = synthetic_maps()
    four = np.stack([syn[k][0] for k in ("cross_on_all_borders", "lone_pixel", "bridge", "all_but_one")])
    nat = natural_maps()["16x16"]
    many = np.stack([np.roll(nat[n % 4], (3 * n % 16, 5 * n % 16), axis=(0, 1)) for n in range(67)])
    out = [(f"{k}-open{n}", v[0][None], SYN_SIGMA, SYN_TH, n) for k, v in syn.items() for n in OPENS]
    out += [(f"four-open{n}", four, SYN_SIGMA, SYN_TH, n) for n in (0, 1, 2)]
    out += [(f"sixty-seven-open{n}", many, 0.1, 0.25, n) for n in (1, 2)]
    return out
