"""CPU suite for the device box prompt of an attention map (lgd_sam_attn_box_prompt_f32, SamRefiner(attn_box="device")):
the export is declared alike in the header, the binding and the library; the numpy restatement the GPU test compares the
kernel with (tests/sam_box_prompt_cases.py) equals scipy.ndimage and hostprep.binary_mask_to_box on every case; `attn_box`
resolves as documented and `pipeline._batched` answers for all four kinds of refiner."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import lgd_amd  # noqa: F401
import sam_box_prompt_cases as bc
from lgd_amd import _lib, hostprep, pipeline, sam_refine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, NARGS = "lgd_sam_attn_box_prompt_f32", 14


def test_symbol_is_declared_bound_and_exported_with_14_arguments():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgd_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, NAME
    declared = [a.strip() for a in m.group(1).split(",") if a.strip()]
    assert len(declared) == NARGS == len(_lib.SIGNATURES[NAME])
    # pointer / int / float, position by position
    kinds = ["P" if "*" in d else "F" if d.startswith("float") else "I" for d in declared]
    bound = ["P" if t is ctypes.c_void_p else "F" if t is ctypes.c_float else "I" if t is ctypes.c_int else "?"
             for t in _lib.SIGNATURES[NAME]]
    assert kinds == bound, (kinds, bound)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, NAME)
    body = open(os.path.join(ROOT, "llm-groundeddiffusion_amd", "csrc", "sam_tail.hip")).read()
    # one device function smooths for both kernels: the filter's tap loop is written once
    assert body.count("prompt_smooth(") == 3 and body.count("reflect_index(y + j") == 1


def _scipy(a, sigma, th, n_open):
    s = ndimage.gaussian_filter(np.asarray(a).astype(float), sigma=sigma)
    with np.errstate(invalid="ignore"):
        coarse = sam_refine.preprocess_mask(s, th, n_erode_dilate_mask=n_open)
    return s, coarse


def _same_as_scipy(a, sigma, th, n_open, want):
    s, coarse = _scipy(a, sigma, th, n_open)
    assert np.abs(want["smooth"] - s).max() <= 1e-12 * max(np.abs(s).max(), 1e-30)
    assert np.array_equal(want["coarse"], coarse)
    if coarse.any():
        up_w, up_h = bc.scales(*coarse.shape)
        assert not want["empty"] and want["box"] == hostprep.binary_mask_to_box(coarse, w_scale=up_w, h_scale=up_h)
    else:
        assert want["empty"] and want["box"] == [0, 0, 0, 0]
        with pytest.raises(ValueError):                           # where the reference fails: min() of an empty sequence
            hostprep.binary_mask_to_box(coarse, w_scale=1, h_scale=1)


def test_restatement_equals_scipy_on_the_natural_cases():
    cases = bc.natural_cases()
    assert len(cases) >= bc.MIN_NATURAL and len(cases) == len(bc.natural_ids())
    for name, sigma, th, n_open, maps, want in cases:
        for a, w in zip(maps, want):
            assert w["near"] == 0
            _same_as_scipy(a, sigma, th, n_open, w)
    # the sets the margin rule leaves whole, and the two items it is known to take out of the 16 x 16 set
    sizes = {(c[0], c[1], c[2]): len(c[5]) for c in cases}
    assert sizes[("16x16", 0.1, 0.05)] == 2 and sizes[("16x16", 0.1, 0.25)] == 4 and sizes[("8x8", 1.5, 0.05)] == 4
    assert sizes[("8x12", 0.1, 0.05)] == 1
    empties = [(c[0], c[3]) for c in cases for w in c[5] if w["empty"]]
    assert ("8x8", 2) in empties and not any(n == 0 for _, n in empties)


def test_restatement_equals_scipy_on_the_synthetic_cases():
    for name, (a, outcomes) in bc.synthetic_maps().items():
        for n_open in bc.OPENS:
            w = bc.restate(a, bc.SYN_SIGMA, bc.SYN_TH, n_open)
            assert w["near"] == 0
            _same_as_scipy(a, bc.SYN_SIGMA, bc.SYN_TH, n_open, w)
            if n_open in outcomes:
                assert int(w["coarse"].sum()) == outcomes[n_open], (name, n_open)
    syn = bc.synthetic_maps()
    assert np.array_equal(bc.restate(syn["3x3"][0], bc.SYN_SIGMA, bc.SYN_TH, 1)["coarse"], bc.PLUS_3X3)
    before = bc.restate(syn["bridge"][0], bc.SYN_SIGMA, bc.SYN_TH, 0)["coarse"]
    after = bc.restate(syn["bridge"][0], bc.SYN_SIGMA, bc.SYN_TH, 1)["coarse"]
    assert all(before[p] for p in bc.BRIDGE_GAP) and not any(after[p] for p in bc.BRIDGE_GAP)
    assert ndimage.label(before)[1] == 1 and ndimage.label(after)[1] == 2
    for label, maps, sigma, th, n_open in bc.batches():
        assert maps.ndim == 3 and maps.dtype == np.float32
        for a in maps:
            w = bc.restate(a, sigma, th, n_open)
            assert w["near"] == 0, label
            _same_as_scipy(a, sigma, th, n_open, w)
    assert sorted({b[1].shape[0] for b in bc.batches()}) == [1, 4, 67]


class _HostProcessor:
    """Stands for the Hugging Face processor: no `on_device`."""


def test_attn_box_resolution_and_the_pipelines_answer():
    device = dict(sam_model=None, sam_processor=sam_refine.DeviceSamProcessor("cpu"))
    host = dict(sam_model=None, sam_processor=_HostProcessor())
    R = sam_refine.SamRefiner
    # the default is today's behaviour
    assert R(device).attn_box == R(device, use_box_input=True).attn_box == R(host).attn_box == "host"
    with pytest.raises(NotImplementedError):
        R(device, use_box_input=True).attns(np.zeros((1, 64, 64, 3), np.uint8), [np.zeros((8, 8), np.float32)])
    assert R(device, use_box_input=True, attn_box="device").attn_box == "device"
    with pytest.raises(ValueError, match="device processor"):
        R(host, use_box_input=True, attn_box="device")
    with pytest.raises(ValueError, match="attn_box"):
        R(device, attn_box="gpu")
    # the four kinds of refiner x the two prompt kinds
    point, box_host = R(device), R(device, use_box_input=True)
    box_device, on_host = R(device, use_box_input=True, attn_box="device"), R(host, use_box_input=True)
    assert [pipeline._batched(r, "attn") for r in (point, box_host, box_device, on_host)] == [True, False, True, False]
    assert [pipeline._batched(r, "box") for r in (point, box_host, box_device, on_host)] == [True, True, True, False]
    # opting in does not override batched=False, and changes nothing for a point-prompt refiner
    assert not pipeline._batched(R(device, use_box_input=True, attn_box="device", batched=False), "attn")
    assert pipeline._batched(R(device, attn_box="device"), "attn")
    assert box_device.attn_kw == box_host.attn_kw and box_device.attn_kw["gaussian_sigma"] == 0.1


def test_the_plugins_keyword_reaches_the_refiner_and_is_refused_without_the_device_processor(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    from generation import _common
    device = dict(sam_model=None, sam_processor=sam_refine.DeviceSamProcessor("cpu"))
    host = dict(sam_model=None, sam_processor=_HostProcessor())
    assert _common.sam_refiner(device, 512, 512, use_box_input=True).attn_box == "host"
    assert _common.sam_refiner(host, 512, 512, use_box_input=True).attn_box == "host"
    assert _common.sam_refiner(device, 512, 512, use_box_input=True, sam_attn_box="device").attn_box == "device"
    with pytest.raises(ValueError, match="sam_attn_box='device'"):
        _common.sam_refiner(host, 512, 512, use_box_input=True, sam_attn_box="device")
    assert _common.sam_refiner(dict(), 512, 512, sam_attn_box="device") is None


GOLD = os.path.join(ROOT, "tests", "golden", "sam_refine_attn_box.npz")


def test_restatement_and_selection_equal_the_references_own_box_branch():
    """tests/golden/sam_refine_attn_box.npz: what the reference's own sam_refine_attn(use_box_input=True) computed
    (tools/make_golden_sam_box_prompt.py) — opened mask, box, and its selection among fixed candidates."""
    g = np.load(GOLD)
    assert len(g["cases"]) == 10
    picks = set()
    for k, (si, n) in enumerate(g["cases"]):
        sigma, th, n_open = g["settings"][si]
        w = bc.restate(g["maps"][n], sigma, th, int(n_open))
        assert w["near"] == 0 and not w["empty"]
        assert np.array_equal(w["coarse"], g[f"coarse{k}"].astype(bool)) and w["box"] == g[f"box{k}"].tolist()
        mask, conf = sam_refine._pick(g["cand"][n], g["conf"][n], w["coarse"], *g["below"])
        assert np.array_equal(mask, g[f"mask{k}"].astype(bool)) and conf == g[f"picked_conf{k}"]
        picks.add(int(np.argmax([np.array_equal(c, mask) for c in g["cand"][n]])))
    assert picks == {0, 1}                                         # the coarse mask decides: not always the largest
