"""CPU suite for the Pillow-exact SAM preprocessing (DeviceSamProcessor(resize="pillow"), lgd_resample_canvas_u8): the
arithmetic the device path is specified by — tests/resample_cases.py's restatement of Pillow's BILINEAR, then
(v * fp32(1/255) - mean) / std in fp32, then a zero canvas — against the installed Hugging Face SamImageProcessor; the
distance of the resize="torch" processor from it (why the change exists); the export's declarations; its host refusals on
placeholder addresses; the constructor and the wrapper's checks.  tests/test_resample_canvas_gpu.py and
tests/test_sam_processor_pillow_gpu.py run the kernel."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import _lib, ops, sam_refine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resample_cases as rc  # noqa: E402
import sam_cases  # noqa: E402

ERR_ARG, ERR_LAUNCH, ERR_UNSUPPORTED = -1, -2, -3
TARGET = 1024
SIZES = [(512, 512), (96, 64), (1200, 900), (512, 2048)]           # (h, w)
LEVEL = 1.0 / 255.0 / max(sam_refine.DeviceSamProcessor.STD)        # the smallest step of one 8-bit level in output units


def restatement(img, target=TARGET):
    """uint8 (h, w, 3) -> (fp32 (3, target, target), (nh, nw)): the contract of resize="pillow", in numpy."""
    proc = sam_refine.DeviceSamProcessor("cpu", longest_edge=target)
    nh, nw = proc._shape(*img.shape[:2])
    v = rc.resize(img, (nh, nw), "bilinear").astype(np.float32)
    mean, std = np.float32(proc.MEAN), np.float32(proc.STD)
    px = (v * np.float32(1.0 / 255.0) - mean) / std
    assert px.dtype == np.float32
    canvas = np.zeros((3, target, target), np.float32)
    canvas[:, :nh, :nw] = px.transpose(2, 0, 1)
    return canvas, (nh, nw)


def _image(h, w):
    if (h, w) == (512, 512):
        return np.ascontiguousarray(sam_cases.refine_inputs()[0][0])
    return rc.image((h, w), "random", seed=2)


@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_restatement_against_hugging_face_and_the_torch_processors_distance(h, w):
    """<= 1e-6 absolute (the bound of the DeviceOwlProcessor comparison; measured 7.2e-7 at most), pad exactly 0, the same
    reshaped_input_sizes.  The resize="torch" processor is NOT within that bound: on the 512 x 512 case more than 1 % of
    the pixels are off by half an 8-bit level or more (measured: about 27 % off by one full level)."""
    transformers = pytest.importorskip("transformers")
    from PIL import Image
    img = _image(h, w)
    assert img.shape == (h, w, 3) and img.dtype == np.uint8
    want = transformers.SamImageProcessor()(images=Image.fromarray(img), return_tensors="pt")
    ref = want["pixel_values"][0].numpy()
    got, (nh, nw) = restatement(img)
    assert got.shape == ref.shape == (3, TARGET, TARGET)
    assert [nh, nw] == want["reshaped_input_sizes"][0].tolist()
    err = float(np.abs(got - ref).max())
    print(f"[sam pillow] {h}x{w}: restatement against SamImageProcessor max abs {err:.3e}")
    assert err <= 1e-6
    assert not got[:, nh:, :].any() and not got[:, :, nw:].any()
    assert not ref[:, nh:, :].any() and not ref[:, :, nw:].any()
    tpx, _, tresh = sam_refine.DeviceSamProcessor("cpu").pixels(img)
    assert tresh == [[nh, nw]]
    off = np.abs(tpx[0].numpy() - ref)[:, :nh, :nw] >= 0.5 * LEVEL
    print(f"[sam pillow] {h}x{w}: resize='torch' pixels off by >= half a level: {100 * off.mean():.1f} %")
    if (h, w) == (512, 512):
        assert float(np.abs(tpx[0].numpy() - ref).max()) > 1e-6
        assert off.mean() > 0.01


# ---------------------------------------------------------------------------------------------
# declarations
# ---------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported_alike():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgd_hip.h")).read(), flags=re.S)
    counts = {}
    for name in ("lgd_resample_u8", "lgd_resample_canvas_u8"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        counts[name] = len([a for a in m.group(1).split(",") if a.strip()])
        assert counts[name] == len(_lib.SIGNATURES[name]), name
        assert hasattr(_lib.load(), name), name
    assert counts["lgd_resample_canvas_u8"] == counts["lgd_resample_u8"] + 3 == 30
    assert _lib.SIGNATURES["lgd_resample_canvas_u8"][-4:-1] == [C.c_int, C.c_int, C.c_float]
    assert _lib.load().lgd_abi_version() == _lib.ABI_VERSION == 12


# ---------------------------------------------------------------------------------------------
# the launch's refusals, on placeholder addresses (none is dereferenced: a refusal precedes every runtime call)
# ---------------------------------------------------------------------------------------------
ARGS = ("src N h w H W filter coef_x bounds_x width_x rows_x coef_y bounds_y width_y rows_y scratch form out_f16 "
        "r m0 m1 m2 s0 s1 s2 out CH CW pad stream").split()
SRC, OUT, SCRATCH, CX, BX, CY, BY = (0x10000000 * i for i in range(1, 8))


def _base():
    bl = rc.FILTERS["bilinear"]
    wx, wy = rc.plan(24, 40, "bilinear")[2], rc.plan(16, 48, "bilinear")[2]
    return dict(src=SRC, N=2, h=16, w=24, H=48, W=40, filter=bl, coef_x=CX, bounds_x=BX, width_x=wx, rows_x=40, coef_y=CY,
                bounds_y=BY, width_y=wy, rows_y=48, scratch=SCRATCH, form=1, out_f16=0, r=1 / 255, m0=0.5, m1=0.5, m2=0.5,
                s0=0.25, s1=0.25, s2=0.25, out=OUT, CH=64, CW=56, pad=0.0, stream=None)


def _answer(change):
    a = dict(_base(), **change)
    assert len(ARGS) == len(_lib.SIGNATURES["lgd_resample_canvas_u8"])
    return _lib.load().lgd_resample_canvas_u8(*(a[k] for k in ARGS))


SRC_BYTES, MID_BYTES, OUT_BYTES = 2 * 16 * 24 * 3, 2 * 16 * 40 * 3, 2 * 3 * 64 * 56 * 4
REFUSALS = [("CH < H", {"CH": 47}), ("CW < W", {"CW": 39}), ("CH 0", {"CH": 0}), ("CW -1", {"CW": -1}),
            ("pad nan", {"pad": float("nan")}), ("pad inf", {"pad": float("inf")}), ("pad -inf", {"pad": float("-inf")}),
            ("u8 pad 0.5", {"form": 0, "pad": 0.5}), ("u8 pad -1", {"form": 0, "pad": -1.0}),
            ("u8 pad 256", {"form": 0, "pad": 256.0}), ("u8 pad nan", {"form": 0, "pad": float("nan")})]
# everything lgd_resample_u8 refuses
REFUSALS += [(f"{p} NULL", {p: None}) for p in ("src", "out", "coef_x", "bounds_x", "coef_y", "bounds_y", "scratch")]
REFUSALS += [(f"{n} = {v}", {n: v}) for n in ("N", "h", "w", "H", "W") for v in (0, -1)]
REFUSALS += [(f"filter {v}", {"filter": v}) for v in (0, 4)] + [(f"form {v}", {"form": v}) for v in (3, -1)]
REFUSALS += [("out_f16 2", {"out_f16": 2}), ("coef_x off 2 bytes", {"coef_x": CX + 2}), ("bounds_y off 2 bytes", {"bounds_y": BY + 2}),
             ("width_x + 1", {"width_x": _base()["width_x"] + 1}), ("rows_y - 1", {"rows_y": 47}),
             ("fp32 out off 2 bytes", {"out": OUT + 2}), ("fp16 out off 1 byte", {"out_f16": 1, "out": OUT + 1}),
             ("out is src", {"out": SRC}), ("scratch inside src", {"scratch": SRC + SRC_BYTES - 1}),
             # only the CANVAS reaches these: the dense H x W output would end before them
             ("the canvas' last element inside src", {"out": SRC - OUT_BYTES + 4}),
             ("the canvas' last element inside scratch", {"out": SCRATCH - OUT_BYTES + 4}),
             ("the canvas' last element inside coef_x", {"out": CX - OUT_BYTES + 4})]


@pytest.mark.parametrize("what,change", REFUSALS, ids=[w for w, _ in REFUSALS])
def test_host_refusal(what, change):
    assert _answer(change) == ERR_ARG, what


def test_unsupported_sizes():
    assert _answer({"CH": 16385}) == ERR_UNSUPPORTED
    assert _answer({"CW": 16385}) == ERR_UNSUPPORTED
    assert _answer({"N": 65536}) == ERR_UNSUPPORTED


ACCEPTED = [("base", {}), ("canvas = image", {"CH": 48, "CW": 40}), ("pad -1.5", {"pad": -1.5}),
            ("u8 pad 7 at odd addresses", {"form": 0, "pad": 7.0, "src": SRC + 1, "out": OUT + 3, "scratch": SCRATCH + 5}),
            ("u8 pad 255", {"form": 0, "pad": 255.0}), ("fp16", {"form": 2, "out_f16": 1, "out": OUT + 2}),
            ("only x changes", {"H": 16, "coef_y": None, "bounds_y": None, "width_y": 0, "rows_y": 0, "scratch": None}),
            ("nothing changes", {"H": 16, "W": 24, "coef_x": None, "bounds_x": None, "coef_y": None, "bounds_y": None, "scratch": None}),
            ("the canvas touches src's start", {"out": SRC - OUT_BYTES})]


def test_accepted_calls_reach_the_launch():
    """On a host without a GPU an accepted call reaches the launch and answers LGD_ERR_LAUNCH; where a GPU is present it
    would run on the placeholder addresses, so it is only made where there is none."""
    if torch.cuda.is_available():
        return
    for what, change in ACCEPTED:
        assert _answer(change) == ERR_LAUNCH, what


# ---------------------------------------------------------------------------------------------
# the wrapper and the processor
# ---------------------------------------------------------------------------------------------
def _wrapper_faults():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    return [("canvas smaller than the image", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "bilinear", canvas=(16, 15))),
            ("dense out for a canvas call", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "bilinear", canvas=(20, 20), out=u8(1, 16, 16, 3))),
            ("canvas out for a dense call", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "bilinear", out=u8(1, 20, 20, 3))),
            ("float canvas out in the u8 layout", lambda: ops.resample_u8(u8(1, 8, 8, 3), (16, 16), "bilinear", "affine", canvas=(20, 20),
                                                                          out=torch.zeros(1, 20, 20, 3)))]


_FAULTS = _wrapper_faults()


@pytest.mark.parametrize("what,call", _FAULTS, ids=[w for w, _ in _FAULTS])
def test_wrapper_check_raises_before_the_library(what, call, monkeypatch):
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail(f"{what}: the library was called"))
    with pytest.raises(RuntimeError):
        call()


def test_wrapper_picks_the_entry_by_canvas(monkeypatch):
    """canvas=None makes exactly the dense call (27 arguments, no CH / CW / pad); a canvas makes the canvas call with the
    same leading arguments, the same cached tables, and out shaped as the canvas."""
    calls = []
    monkeypatch.setattr(ops, "_call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: C.c_void_p(0))
    x = torch.zeros(2, 8, 6, 3, dtype=torch.uint8)
    dense = ops.resample_u8(x, (16, 11), "bilinear", "affine")
    padded = ops.resample_u8(x, (16, 11), "bilinear", "affine", canvas=(20, 16), pad=-1.5)
    assert tuple(dense.shape) == (2, 3, 16, 11) and tuple(padded.shape) == (2, 3, 20, 16)
    assert tuple(ops.resample_u8(x, (16, 11), "bilinear", canvas=(20, 16), pad=7).shape) == (2, 20, 16, 3)
    (n0, a0), (n1, a1), _ = calls
    assert n0 == "lgd_resample_u8" and len(a0) == len(_lib.SIGNATURES[n0])
    assert n1 == "lgd_resample_canvas_u8" and len(a1) == len(_lib.SIGNATURES[n1])
    assert a1[-4:-1] == (20, 16, -1.5)
    value = lambda v: v.value if hasattr(v, "value") else v
    same = [i for i in range(25) if i != 15]                      # all but scratch (allocated per call) and out
    assert [value(a0[i]) for i in same] == [value(a1[i]) for i in same]


def test_constructor():
    img = _image(96, 64)
    a = sam_refine.DeviceSamProcessor("cpu").pixels(img)
    b = sam_refine.DeviceSamProcessor("cpu", resize="torch").pixels(img)
    assert torch.equal(a[0], b[0]) and a[1:] == b[1:]
    assert sam_refine.DeviceSamProcessor("cpu").resize == "torch"
    with pytest.raises(ValueError):
        sam_refine.DeviceSamProcessor("cpu", resize="pil")
    with pytest.raises(ValueError):
        sam_refine.DeviceSamProcessor("cpu", resize=None)
    with pytest.raises(RuntimeError, match="no torch fallback"):   # no GPU, no HIP resampler: refused, not approximated
        sam_refine.DeviceSamProcessor("cpu", resize="pillow")


def test_sam_refiner_of_the_plugins_passes_the_choice_through(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    from generation import _common
    torch_proc = sam_refine.DeviceSamProcessor("cpu")
    md = dict(sam_model=None, sam_processor=torch_proc)
    assert _common.sam_refiner(md, 512, 512).md["sam_processor"] is torch_proc                    # the default: as carried
    assert _common.sam_refiner(md, 512, 512, sam_resize="torch").md["sam_processor"] is torch_proc
    with pytest.raises(RuntimeError, match="no torch fallback"):                       # rebuilt as "pillow": needs the GPU
        _common.sam_refiner(md, 512, 512, sam_resize="pillow")
    with pytest.raises(ValueError):
        _common.sam_refiner(md, 512, 512, sam_resize="pil")
    with pytest.raises(ValueError):
        _common.sam_refiner(dict(sam_model=None, sam_processor=object()), 512, 512, sam_resize="pillow")
