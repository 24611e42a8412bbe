"""Pillow's Image.resize for 8-bit RGB images, restated in numpy, and the cases the resampling tests share.

The restatement is the contract include/lgd_hip.h states for lgd_resample_plan / lgd_resample_u8 ([ext] Pillow
src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc and the two 8-bit passes), written from that text
and independent of the library: tests/test_resample_cpu.py holds it against PIL.Image.resize bit for bit, and the library
against it.  Scalars are Python floats (fp64) and the sine is libm's (math.sin), as in Pillow."""
import math

import numpy as np
from PIL import Image

PRECISION_BITS = 32 - 8 - 2
FILTERS = {"bilinear": 2, "bicubic": 3, "lanczos": 1}          # Pillow's Image.Resampling codes
PIL_FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_KERNELS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def plan(n_in, n_out, filter):
    """(coef int32 [n_out, width], bounds int32 [n_out, 2] = (xmin, count), width) of one axis."""
    f, support0 = _KERNELS[filter]
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = support0 * filterscale
    ss = 1.0 / filterscale
    width = int(math.ceil(support)) * 2 + 1
    coef = np.zeros((n_out, width), np.int32)
    bounds = np.zeros((n_out, 2), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), n_in) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(count)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            coef[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, count)
    return coef, bounds, width


def _pass(img, coef, bounds, axis):
    """One pass over `axis` of a uint8 (.., h, w, 3) array: int32 sums, arithmetic shift, clip to 0 .. 255."""
    src = np.moveaxis(img.astype(np.int32), axis, 0)
    out = np.empty((coef.shape[0],) + src.shape[1:], np.int32)
    for o in range(coef.shape[0]):
        xmin, count = bounds[o]
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)
        for x in range(count):
            acc = acc + coef[o, x] * src[xmin + x]
        out[o] = acc >> PRECISION_BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize(img, size, filter):
    """uint8 (h, w, 3) or (N, h, w, 3) -> uint8 (.., H, W, 3): horizontal pass, then vertical on its uint8 result; a
    pass whose size does not change is left out."""
    H, W = size
    h, w = img.shape[-3], img.shape[-2]
    if w != W:
        c, b, _ = plan(w, W, filter)
        img = _pass(img, c, b, img.ndim - 2)
    if h != H:
        c, b, _ = plan(h, H, filter)
        img = _pass(img, c, b, img.ndim - 3)
    return img


def pil_resize(img, size, filter):
    """PIL.Image.resize itself on a uint8 (h, w, 3) array (PIL's size is (width, height))."""
    return np.asarray(Image.fromarray(img).resize((size[1], size[0]), PIL_FILTERS[filter]))


# (h, w) -> (H, W): the smallest shapes at which each thing can go wrong
SMALL = [
    ((16, 16), (32, 32)),     # plain upscale; 0/255 input puts about a quarter of the LANCZOS outputs on the clip, both sides
    ((16, 24), (48, 40)),     # non-square, a different scale per axis
    ((24, 16), (12, 8)),      # downscale: widened windows
    ((24, 24), (8, 8)),       # downscale by 3: 7 - 19 taps
    ((13, 9), (9, 13)),       # one axis down, one up, odd sizes
    ((8, 8), (8, 20)),        # the vertical pass left out
    ((20, 8), (8, 8)),        # the horizontal pass left out
    ((3, 3), (11, 11)),       # the window clipped at both borders at once
]
FILTER_NAMES = ("bilinear", "bicubic", "lanczos")
PATTERNS = ("random", "binary")
CASES = [(src, dst, f, p) for src, dst in SMALL for f in FILTER_NAMES for p in PATTERNS]
# the geometries the consumers use, one image each
CONSUMER = [((512, 512), (768, 768), "bicubic", "random"), ((512, 512), (1024, 1024), "lanczos", "random")]


def case_id(c):
    (h, w), (H, W), f, p = c
    return f"{h}x{w}-{H}x{W}-{f}-{p}"


def image(shape, pattern, seed=0, n=None):
    """Seeded uint8 (h, w, 3) image, or (n, h, w, 3) different ones: uniform bytes, or only 0 and 255."""
    rng = np.random.RandomState(1000 * seed + 7 * shape[0] + shape[1])
    full = ((n,) if n else ()) + tuple(shape) + (3,)
    if pattern == "random":
        return rng.randint(0, 256, full).astype(np.uint8)
    return (rng.randint(0, 2, full) * 255).astype(np.uint8)


_WANT = {}


def expected(c, n=None):
    """Pillow's result for a case (computed once per process and shared; treat as read-only): (input, output), with a
    leading batch axis of n different images when n is given."""
    key = (c, n)
    if key not in _WANT:
        src, dst, f, p = c
        img = image(src, p, n=n)
        out = pil_resize(img, dst, f) if n is None else np.stack([pil_resize(i, dst, f) for i in img])
        img.setflags(write=False), out.setflags(write=False)
        _WANT[key] = (img, out)
    return _WANT[key]
