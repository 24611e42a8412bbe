"""The canvas form of the device resampler (lgd_resample_canvas_u8 through ops.resample_u8(..., canvas=, pad=)): the
resized image at the top left of a larger canvas, everything else the pad value, all written by the last resize pass.
The reference is the torch expression of the form applied to Pillow's own bytes (PIL.Image.resize, bit for bit) and
placed in a canvas filled with the pad.  Shapes are the smallest at which each path can go wrong; the output sits between
guard elements in a buffer prefilled with NaN (255 for uint8), so an element the kernel leaves out, writes twice with
different values or writes outside the canvas shows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lgd_amd  # noqa: E402,F401
import resample_cases as rc  # noqa: E402
from lgd_amd import _lib, ops  # noqa: E402

ERR_ARG = -1
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILTER = "bilinear"
GUARD = 37                                                       # elements on each side of the output
PAD = {"u8": 7, "affine": -1.5, "unit": -1.5}                    # non-zero: the fill is visibly the kernel's
# (source, resized, canvas, what it exercises)
SHAPES = [((5, 7), (8, 11), (8, 11), "no pad"),
          ((6, 4), (16, 11), (16, 16), "pad on the right only"),
          ((8, 16), (4, 16), (16, 16), "vertical pass only, pad at the bottom"),
          ((16, 12), (16, 12), (16, 16), "no pass"),
          ((9, 5), (3, 2), (7, 5), "down-scale, pad on both sides, odd row lengths")]
FORMS = [("u8", torch.uint8), ("affine", torch.float32), ("affine", torch.float16), ("unit", torch.float32),
         ("unit", torch.float16)]
FORM_IDS = ["u8", "affine-fp32", "affine-fp16", "unit-fp32", "unit-fp16"]
SHAPE_IDS = [f"{h}x{w}-{H}x{W}-in-{CH}x{CW}" for (h, w), (H, W), (CH, CW), _ in SHAPES]


def _form(pil, form, dtype):
    """The torch expression of `form` on Pillow's bytes, uint8 (N, H, W, 3) on the device, in the contract's operation
    order; every divisor is a device tensor (torch's kernel for a Python-scalar divisor multiplies by the reciprocal)."""
    if form == "u8":
        return pil
    v = pil.permute(0, 3, 1, 2).float()
    if form == "affine":
        m = torch.tensor(MEAN, device=pil.device, dtype=torch.float32).view(1, 3, 1, 1)
        s = torch.tensor(STD, device=pil.device, dtype=torch.float32).view(1, 3, 1, 1)
        return ((v * (1 / 255) - m) / s).to(dtype).contiguous()
    d = torch.tensor(255.0, device=pil.device, dtype=torch.float32)
    return (v / d * 2.0 - 1.0).to(dtype).contiguous()


_WANT = {}


def _case(dev, shape, form, dtype, n):
    """(source uint8 (n, h, w, 3) on the device, the expected canvas), computed once per case and shared (read-only)."""
    key = (shape[:3], form, dtype, n)
    if key not in _WANT:
        (h, w), (H, W), (CH, CW), _ = shape
        img = rc.image((h, w), "random", seed=4, n=n)
        pil = torch.from_numpy(np.stack([rc.pil_resize(i, (H, W), FILTER) for i in img])).to(dev)
        inner = _form(pil, form, dtype)
        if form == "u8":
            want = torch.full((n, CH, CW, 3), PAD[form], device=dev, dtype=dtype)
            want[:, :H, :W] = inner
        else:
            want = torch.full((n, 3, CH, CW), PAD[form], device=dev, dtype=dtype)
            want[:, :, :H, :W] = inner
        _WANT[key] = (torch.from_numpy(img.copy()).to(dev), want)
    return _WANT[key]


def _guarded(dev, shape, dtype):
    """(buffer, view of `shape` inside it): NaN (255) everywhere, GUARD elements on each side of the view."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), 255 if dtype == torch.uint8 else float("nan"), device=dev, dtype=dtype)
    return buf, buf[GUARD:GUARD + numel].view(shape)


def _untouched(buf):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool((g == 255).all()) if buf.dtype == torch.uint8 else bool(torch.isnan(g).all())


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = got != want                                           # a NaN left from the prefill differs from everything
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, the first at {tuple(bad.nonzero()[0].tolist())}"


@pytest.mark.parametrize("n", [1, 3], ids=["N1", "N3"])
@pytest.mark.parametrize("form,dtype", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_canvas_equals_the_torch_expression_on_pillows_bytes(dev, shape, form, dtype, n):
    (h, w), (H, W), (CH, CW), what = shape
    x, want = _case(dev, shape, form, dtype, n)
    buf, out = _guarded(dev, tuple(want.shape), dtype)
    got = ops.resample_u8(x, (H, W), FILTER, form, dtype=dtype, mean=MEAN, std=STD, canvas=(CH, CW), pad=PAD[form], out=out)
    assert got.data_ptr() == out.data_ptr()
    _same(got, want)
    assert _untouched(buf), what
    # without out=: the wrapper allocates the canvas
    _same(ops.resample_u8(x, (H, W), FILTER, form, dtype=dtype, mean=MEAN, std=STD, canvas=(CH, CW), pad=PAD[form]), want)
    if (CH, CW) == (H, W):                                      # no pad: the dense call's bits
        _same(got, ops.resample_u8(x, (H, W), FILTER, form, dtype=dtype, mean=MEAN, std=STD))


@pytest.mark.parametrize("form,dtype", FORMS[:2], ids=FORM_IDS[:2])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_source_at_an_odd_byte_address(dev, shape, form, dtype):
    """src and scratch (and a uint8 out) need no alignment: each sits at an odd byte offset of a larger buffer."""
    (h, w), (H, W), (CH, CW), _ = shape
    x, want = _case(dev, shape, form, dtype, 3)
    src = torch.full((x.numel() + 16,), 0x5A, device=dev, dtype=torch.uint8)
    src[1:1 + x.numel()] = x.reshape(-1)
    mid = torch.full((3 * h * W * 3 + 16,), 0x5A, device=dev, dtype=torch.uint8)
    odd = src[1:1 + x.numel()].view(3, h, w, 3)
    buf, out = _guarded(dev, tuple(want.shape), dtype)
    assert odd.data_ptr() % 2 == 1 and mid[5:].data_ptr() % 2 == 1 and (form != "u8" or out.data_ptr() % 2 == 1)
    got = ops.resample_u8(odd, (H, W), FILTER, form, dtype=dtype, mean=MEAN, std=STD, canvas=(CH, CW), pad=PAD[form], out=out,
                          scratch=mid[5:5 + 3 * h * W * 3])
    _same(got, want)
    assert _untouched(buf)
    assert bool((mid[:5] == 0x5A).all()) and bool((mid[5 + 3 * h * W * 3:] == 0x5A).all())


def test_one_captured_graph_replayed_twice(dev):
    """Every shape in every form inside ONE captured graph (tables resident after the warm-up: kernels only).  The
    outputs are poisoned again between the replays, so each replay has to write every element: identical bits both times,
    and the eager call's."""
    keys = [(s, f, d) for s in SHAPES for f, d in FORMS]
    ins = {k: _case(dev, k[0], k[1], k[2], 3) for k in keys}

    def buffers():
        return {k: _guarded(dev, tuple(ins[k][1].shape), k[2]) for k in keys}
    scratch = {s[:3]: torch.empty((3 * s[0][0] * s[1][1] * 3,), device=dev, dtype=torch.uint8) for s in SHAPES}

    def launch(bufs):
        for (s, f, d), (_, out) in bufs.items():
            ops.resample_u8(ins[(s, f, d)][0], s[1], FILTER, f, dtype=d, mean=MEAN, std=STD, canvas=s[2], pad=PAD[f], out=out,
                            scratch=scratch[s[:3]])
    eager, graphed = buffers(), buffers()
    launch(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(buffers())                                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        launch(graphed)
    for _ in range(2):
        for buf, _out in graphed.values():
            buf.fill_(255 if buf.dtype == torch.uint8 else float("nan"))
        cg.replay()
        torch.cuda.synchronize()
        for k in keys:
            _same(graphed[k][1], ins[k][1])
            assert torch.equal(graphed[k][1], eager[k][1]), k
            assert _untouched(graphed[k][0]), k


def _refusals():
    nan, inf = float("nan"), float("inf")
    return [("CH < H", {"CH": 15}), ("CW < W", {"CW": 10}), ("CH 0", {"CH": 0}), ("pad nan", {"pad": nan}),
            ("pad inf", {"pad": inf}), ("pad -inf", {"pad": -inf}), ("u8 pad 0.5", {"form": 0, "pad": 0.5}),
            ("u8 pad 256", {"form": 0, "pad": 256.0}), ("u8 pad -1", {"form": 0, "pad": -1.0}), ("u8 pad nan", {"form": 0, "pad": nan}),
            ("src NULL", {"src": None}), ("out NULL", {"out": None}), ("scratch NULL", {"scratch": None}),
            ("coef_x NULL", {"coef_x": None}), ("bounds_y NULL", {"bounds_y": None}), ("fp32 out off 2 bytes", {"out": 2}),
            ("coef_y off 2 bytes", {"coef_y": 2}), ("out is src", {"out": "src"}), ("N 0", {"N": 0}), ("form 3", {"form": 3}),
            ("filter 0", {"filter": 0}), ("width_x + 1", {"width_x": 1}), ("rows_y - 1", {"rows_y": -1})]


_REFUSALS = _refusals()


@pytest.mark.parametrize("what,change", _REFUSALS, ids=[w for w, _ in _REFUSALS])
def test_refusal_answers_err_arg_without_a_launch(dev, what, change):
    """6 x 4 -> 16 x 11 in a 16 x 16 canvas on real operands, one argument made wrong: LGD_ERR_ARG, and the output buffer
    (four times the canvas, so that no reading of the wrong argument could leave it) keeps its prefill."""
    n, (h, w), (H, W), (CH, CW) = 2, (6, 4), (16, 11), (16, 16)
    x = torch.from_numpy(rc.image((h, w), "random", seed=4, n=n).copy()).to(dev)
    cx, bx, wx = ops.resample_tables(w, W, FILTER, dev)
    cy, by, wy = ops.resample_tables(h, H, FILTER, dev)
    scratch = torch.empty((4 * n * h * W * 3,), device=dev, dtype=torch.uint8)
    out = torch.full((4 * n * 3 * CH * CW,), float("nan"), device=dev, dtype=torch.float32)
    a = dict(src=x.data_ptr(), N=n, h=h, w=w, H=H, W=W, filter=rc.FILTERS[FILTER], coef_x=cx.data_ptr(), bounds_x=bx.data_ptr(),
             width_x=wx, rows_x=W, coef_y=cy.data_ptr(), bounds_y=by.data_ptr(), width_y=wy, rows_y=H, scratch=scratch.data_ptr(),
             form=1, out_f16=0, r=1 / 255, m0=MEAN[0], m1=MEAN[1], m2=MEAN[2], s0=STD[0], s1=STD[1], s2=STD[2],
             out=out.data_ptr(), CH=CH, CW=CW, pad=0.0, stream=None)
    for k, v in change.items():
        if k in ("CH", "CW", "pad", "form", "filter", "N") or v is None:
            a[k] = v
        elif v == "src":
            a[k] = a["src"]
        else:
            a[k] = a[k] + v                                      # an offset: bytes for an address, a count otherwise
    torch.cuda.synchronize()
    names = ("src N h w H W filter coef_x bounds_x width_x rows_x coef_y bounds_y width_y rows_y scratch form out_f16 "
             "r m0 m1 m2 s0 s1 s2 out CH CW pad stream").split()
    assert len(names) == len(_lib.SIGNATURES["lgd_resample_canvas_u8"])
    assert _lib.load().lgd_resample_canvas_u8(*(a[k] for k in names)) == ERR_ARG, what
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), what
    # and through the wrapper the refusal is an error, not a result
    if what == "pad nan":
        with pytest.raises(RuntimeError):
            ops.resample_u8(x, (H, W), FILTER, "affine", canvas=(CH, CW), pad=float("nan"))
