"""Pillow-exact resizing (csrc/resample.hip, ops.resample_u8, lgd_amd/owl_processor.py), checked where there is no GPU:

  * the numpy restatement of tests/resample_cases.py equals PIL.Image.resize bit for bit on every case (this is about the
    oracle: it holds without the library);
  * the library's host plan function, through ctypes, returns exactly the restatement's coefficients, bounds and row width
    for every (in, out, filter) of the case table;
  * every refusal the header lists answers LGD_ERR_ARG on placeholder pointers — a launch attempt on a host without a GPU
    would answer LGD_ERR_LAUNCH, so the refusal happens before the device;
  * the ops wrapper raises on host tensors before the library is called, and DeviceOwlProcessor refuses the configurations
    it does not serve."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import _lib, ops
from lgd_amd.owl_processor import DeviceOwlProcessor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_cases as rc  # noqa: E402

ERR_ARG, ERR_LAUNCH, ERR_UNSUPPORTED = -1, -2, -3
ALL = rc.CASES + rc.CONSUMER


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("c", ALL, ids=[rc.case_id(c) for c in ALL])
def test_restatement_equals_pillow(c):
    img, want = rc.expected(c)
    got = rc.resize(img, c[1], c[2])
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"


def test_binary_lanczos_upscale_reaches_the_clip_on_both_sides():
    """What makes the 0 / 255 pattern a case of its own: a good share of the unclipped sums leave 0 .. 255, both ways."""
    c = ((16, 16), (32, 32), "lanczos", "binary")
    img, want = rc.expected(c)
    cx, bx, _ = rc.plan(16, 32, "lanczos")
    mid = rc._pass(img, cx, bx, 1).astype(np.int64)
    acc = np.stack([sum(int(cx[o, x]) * mid[bx[o, 0] + x] for x in range(bx[o, 1])) for o in range(32)])
    raw = (acc + (1 << 21)) >> 22
    assert (raw < 0).mean() > 0.02 and (raw > 255).mean() > 0.02
    assert np.array_equal(np.clip(raw, 0, 255), want)


AXES = sorted({(s[i], d[i], f) for s, d, f, _ in ALL for i in (0, 1) if s[i] != d[i]})


@pytest.mark.parametrize("n_in,n_out,f", AXES, ids=[f"{a}-{b}-{f}" for a, b, f in AXES])
def test_plan_function_equals_restatement(n_in, n_out, f):
    coef, bounds, width = ops.resample_plan(n_in, n_out, f)
    want_c, want_b, want_w = rc.plan(n_in, n_out, f)
    assert width == want_w and tuple(coef.shape) == (n_out, want_w)
    assert np.array_equal(bounds.numpy(), want_b)
    assert np.array_equal(coef.numpy(), want_c)


def test_plan_width_query_and_refusals():
    lib = _lib.load()
    w = C.c_int(-1)
    assert lib.lgd_resample_plan(24, 8, rc.FILTERS["lanczos"], None, None, C.byref(w)) == 0 and w.value == 19
    assert lib.lgd_resample_plan(512, 1024, rc.FILTERS["lanczos"], None, None, C.byref(w)) == 0 and w.value == 7
    coef = (C.c_int32 * (8 * 19))()
    bounds = (C.c_int32 * 16)()
    pc, pb = C.addressof(coef), C.addressof(bounds)
    assert lib.lgd_resample_plan(24, 8, 1, pc, pb, None) == 0            # the width is optional with the tables
    for what, args in [("in 0", (0, 8, 1, pc, pb, None)), ("out -1", (24, -1, 1, pc, pb, None)),
                       ("filter 0", (24, 8, 0, pc, pb, None)), ("filter 4", (24, 8, 4, pc, pb, None)),
                       ("coef without bounds", (24, 8, 1, pc, None, None)), ("bounds without coef", (24, 8, 1, None, pb, None)),
                       ("nothing to write", (24, 8, 1, None, None, None)), ("coef off 2 bytes", (24, 8, 1, pc + 2, pb, None)),
                       ("bounds off 2 bytes", (24, 8, 1, pc, pb + 2, None)),
                       ("width off 1 byte", (24, 8, 1, None, None, pc + 1)), ("tables overlap", (24, 8, 1, pc, pc + 16, None))]:
        assert lib.lgd_resample_plan(*args) == ERR_ARG, what
    assert lib.lgd_resample_plan(16385, 8, 1, None, None, C.byref(w)) == ERR_UNSUPPORTED
    assert lib.lgd_resample_plan(8, 16385, 1, None, None, C.byref(w)) == ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------
# the launch's refusals, on placeholder addresses
# ---------------------------------------------------------------------------------------------
ARGS = ("src N h w H W filter coef_x bounds_x width_x rows_x coef_y bounds_y width_y rows_y scratch form out_f16 "
        "r m0 m1 m2 s0 s1 s2 out stream").split()
SRC, OUT, SCRATCH, CX, BX, CY, BY = (0x10000000 * i for i in range(1, 8))


def _base():
    fl = rc.FILTERS["lanczos"]
    wx, wy = rc.plan(24, 40, "lanczos")[2], rc.plan(16, 48, "lanczos")[2]
    return dict(src=SRC, N=2, h=16, w=24, H=48, W=40, filter=fl, coef_x=CX, bounds_x=BX, width_x=wx, rows_x=40, coef_y=CY,
                bounds_y=BY, width_y=wy, rows_y=48, scratch=SCRATCH, form=0, out_f16=0, r=1 / 255, m0=0.5, m1=0.5, m2=0.5,
                s0=0.25, s1=0.25, s2=0.25, out=OUT, stream=None)


def _answer(change):
    a = dict(_base(), **change)
    assert len(ARGS) == len(_lib.SIGNATURES["lgd_resample_u8"])
    return _lib.load().lgd_resample_u8(*(a[k] for k in ARGS))


SRC_BYTES, MID_BYTES = 2 * 16 * 24 * 3, 2 * 16 * 40 * 3
REFUSALS = [(f"{p} NULL", {p: None}) for p in ("src", "out", "coef_x", "bounds_x", "coef_y", "bounds_y", "scratch")]
REFUSALS += [(f"{n} = {v}", {n: v}) for n in ("N", "h", "w", "H", "W") for v in (0, -1)]
REFUSALS += [(f"filter {v}", {"filter": v}) for v in (0, 4, -1)] + [(f"form {v}", {"form": v}) for v in (3, -1)]
REFUSALS += [(f"out_f16 {v}", {"out_f16": v}) for v in (2, -1)]
REFUSALS += [(f"{p} off 2 bytes", {p: _base()[p] + 2}) for p in ("coef_x", "bounds_x", "coef_y", "bounds_y")]
REFUSALS += [("width_x + 1", {"width_x": _base()["width_x"] + 1}), ("width_y - 2", {"width_y": _base()["width_y"] - 2}),
             ("width_x 0", {"width_x": 0}), ("rows_x + 1", {"rows_x": 41}), ("rows_y - 1", {"rows_y": 47}),
             ("rows_x of the input", {"rows_x": 24}),
             ("fp32 out off 2 bytes", {"form": 1, "out": OUT + 2}), ("fp16 out off 1 byte", {"form": 2, "out_f16": 1, "out": OUT + 1}),
             ("out is src", {"out": SRC}), ("out inside src", {"out": SRC + SRC_BYTES - 1}),
             ("out ends inside src", {"out": SRC - 1}), ("out inside scratch", {"out": SCRATCH + MID_BYTES - 1}),
             ("scratch inside src", {"scratch": SRC + SRC_BYTES - 1}), ("scratch is src", {"scratch": SRC}),
             ("out inside coef_x", {"out": CX + 4}), ("out inside bounds_y", {"out": BY})]


@pytest.mark.parametrize("what,change", REFUSALS, ids=[w for w, _ in REFUSALS])
def test_host_refusal(what, change):
    assert _answer(change) == ERR_ARG, what


def test_unsupported_sizes():
    assert _answer({"N": 65536}) == ERR_UNSUPPORTED
    assert _answer({"H": 16385, "rows_y": 16385}) == ERR_UNSUPPORTED


ACCEPTED = [("base", {}), ("operands at odd addresses", {"src": SRC + 1, "out": OUT + 3, "scratch": SCRATCH + 5}),
            ("fp32 out 4-byte aligned", {"form": 1, "out": OUT + 4}), ("fp16 out 2-byte aligned", {"form": 2, "out_f16": 1, "out": OUT + 2}),
            ("only x changes: no y tables, no scratch", {"H": 16, "coef_y": None, "bounds_y": None, "width_y": 0, "rows_y": 0, "scratch": None}),
            ("only y changes: no x tables, no scratch", {"W": 24, "coef_x": None, "bounds_x": None, "width_x": 0, "rows_x": 0, "scratch": None}),
            ("nothing changes", {"H": 16, "W": 24, "coef_x": None, "bounds_x": None, "coef_y": None, "bounds_y": None, "scratch": None}),
            ("out touches src's end", {"out": SRC + SRC_BYTES})]


def test_accepted_calls_reach_the_launch():
    """The base call and the forms the header allows pass every check: on a host without a GPU the launch is reached and
    answers LGD_ERR_LAUNCH.  Where a GPU is present these calls would run on the placeholder addresses, so they are only
    made where there is none (tests/test_resample_gpu.py runs the accepted forms on real operands)."""
    if torch.cuda.is_available():
        return
    for what, change in ACCEPTED:
        assert _answer(change) == ERR_LAUNCH, what


# ---------------------------------------------------------------------------------------------
# the wrapper and the processor
# ---------------------------------------------------------------------------------------------
def _wrapper_faults():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    return [("dtype", lambda: ops.resample_u8(torch.zeros(1, 8, 8, 3), (16, 16), "lanczos")),
            ("not a batch", lambda: ops.resample_u8(u8(8, 8, 3), (16, 16), "lanczos")),
            ("channels", lambda: ops.resample_u8(u8(1, 8, 8, 4), (16, 16), "lanczos")),
            ("strided", lambda: ops.resample_u8(u8(1, 8, 16, 3)[:, :, ::2], (16, 16), "lanczos")),
            ("filter name", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "nearest")),
            ("filter code", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), 0)),
            ("form", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "lanczos", "float")),
            ("u8 form with a float dtype", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "lanczos", "u8", dtype=torch.float32)),
            ("unit form in fp64", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "lanczos", "unit", dtype=torch.float64)),
            ("out shape", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "lanczos", out=u8(1, 16, 16, 4))),
            ("out layout of the other form", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "lanczos", "unit", out=torch.zeros(1, 16, 16, 3))),
            ("out dtype", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "lanczos", "unit", out=torch.zeros(1, 3, 16, 16, dtype=torch.float16))),
            ("scratch size", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "lanczos", scratch=u8(8 * 16 * 3 - 1))),
            ("empty size", lambda: ops.resample_u8(u8(1, 8, 8, 3), (0, 16), "lanczos")),
            ("mean per channel", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "lanczos", "affine", mean=(0.5,)))]


_FAULTS = _wrapper_faults()


@pytest.mark.parametrize("what,call", _FAULTS, ids=[w for w, _ in _FAULTS])
def test_wrapper_check_raises_before_the_library(what, call, monkeypatch):
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail(f"{what}: the library was called"))
    with pytest.raises(RuntimeError):
        call()


def test_tables_are_read_from_the_library_and_cached(monkeypatch):
    """ops.resample_tables asks lgd_resample_plan (never recomputes) and uploads once per (in, out, filter)."""
    calls = []
    real = ops.resample_plan
    monkeypatch.setattr(ops, "resample_plan", lambda *a: calls.append(a) or real(*a))
    monkeypatch.setattr(ops, "_RESAMPLE_TABLES", {})
    a = ops.resample_tables(24, 8, "lanczos", "cpu")
    b = ops.resample_tables(24, 8, 1, torch.device("cpu"))
    assert a[0] is b[0] and a[1] is b[1] and len(calls) == 1
    ops.resample_tables(24, 8, "bicubic", "cpu")
    assert len(calls) == 2
    assert np.array_equal(a[0].numpy(), rc.plan(24, 8, "lanczos")[0])


OWL = dict(do_resize=True, size={"height": 768, "width": 768}, resample=3, do_rescale=True, rescale_factor=1 / 255,
           do_normalize=True, image_mean=[0.48145466, 0.4578275, 0.40821073], image_std=[0.26862954, 0.26130258, 0.27577711],
           do_center_crop=False)


def test_device_owl_processor_reads_the_configuration():
    p = DeviceOwlProcessor(dict(OWL))
    assert p.size == (768, 768) and p.filter == "bicubic" and p.rescale == 1 / 255 and p.mean[0] == 0.48145466
    assert DeviceOwlProcessor(dict(OWL, resample=1, size=(32, 48))).filter == "lanczos"
    assert DeviceOwlProcessor(dict(OWL, do_normalize=False)).std == (1.0, 1.0, 1.0)
    assert DeviceOwlProcessor(dict(OWL, do_rescale=False)).rescale == 1.0
    try:
        from transformers import OwlViTImageProcessor
    except ImportError:
        return
    hf = OwlViTImageProcessor()
    p = DeviceOwlProcessor(hf)
    assert p.size == (768, 768) and p.filter == "bicubic" and p.mean == tuple(float(v) for v in hf.image_mean)
    with pytest.raises(ValueError):
        DeviceOwlProcessor(OwlViTImageProcessor(resample=0))
    with pytest.raises(RuntimeError):
        p.input_ids(["a cat"])                                   # an image processor has no tokenizer


@pytest.mark.parametrize("what,change", [("centre crop", dict(do_center_crop=True)), ("nearest", dict(resample=0)),
                                         ("box", dict(resample=4)), ("hamming", dict(resample=5)), ("no filter", dict(resample=None)),
                                         ("no resize", dict(do_resize=False)), ("shortest edge", dict(size={"shortest_edge": 768})),
                                         ("no size", dict(size=None)), ("padding", dict(do_pad=True)),
                                         ("grey mean", dict(image_mean=[0.5]))], ids=lambda v: v if isinstance(v, str) else "")
def test_device_owl_processor_refuses_what_it_does_not_serve(what, change):
    with pytest.raises(ValueError):
        DeviceOwlProcessor(dict(OWL, **change))
