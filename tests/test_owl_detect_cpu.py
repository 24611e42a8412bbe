"""The stage-2 evaluator, host side: the golden of the detection tail (tests/golden/owl_detect_cases.npz, written by
tools/make_golden_owl_detect.py from the reference's own utils/eval/eval.py) and its margin conditions, the two library
exports, the host box-bias table, the state-dict contract of `owlvit.from_hf`, and the drop-in's `utils.eval` package."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lgd_amd  # noqa: E402,F401
import owl_detect_cases as cases  # noqa: E402
from lgd_amd import _lib, ops, owlvit  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "owl_detect_cases.npz")
DROPIN = os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def test_golden_regenerates_bit_for_bit(tmp_path):
    import ref_harness
    if not ref_harness.available():
        pytest.skip("needs the reference checkout")
    out = tmp_path / "owl.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_owl_detect.py"), "--out", str(out)],
                   check=True, capture_output=True, timeout=600)
    new, old = np.load(out), np.load(GOLDEN)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)


@pytest.mark.parametrize("c", cases.CASES, ids=[c["name"] for c in cases.CASES])
def test_golden_margins_hold(gold, c):
    """fp64 and fp32 cannot legitimately disagree on the committed inputs: score gaps, distance of every score to the
    score thresholds and of every pairwise IoU to the NMS thresholds >= 1e-4, no degenerate box."""
    name = c["name"]
    logits, boxes = gold[f"{name}/logits"], gold[f"{name}/pred_boxes"]
    assert logits.shape == (c["B"], c["P"], c["Q"]) and boxes.shape == (c["B"], c["P"], 4)
    assert logits.dtype == np.float32 and boxes.dtype == np.float32
    for b in range(c["B"]):
        gap, thr, nms, side = cases.check_margins(logits[b], boxes[b])
        print(f"{name}[{b}]: score gap {gap:.2e}, to score threshold {thr:.2e}, IoU to NMS threshold {nms:.2e}, side {side:.2e}")
        best = np.sort(logits[b].max(axis=-1).astype(np.float64))
        if c["P"] > 2:                                         # a permutation of an evenly spaced grid
            np.testing.assert_allclose(np.diff(best), np.diff(best).mean(), rtol=1e-3)
            lo, hi = (-6.0, -4.0) if c["kind"] == "below" else (-3.0, 3.0)
            assert lo <= best[0] < lo + 0.06 and hi <= best[-1] < hi + 0.06
    if c["masked"]:
        b, q = c["masked"]
        assert (logits[b, :, q] == cases.FMIN).all() and (gold[f"{name}/plain_005_05/labels"][b] != q).all()
    for fname, aware, st, nt in cases.FLAVOURS:
        count, index = gold[f"{name}/{fname}/count"], gold[f"{name}/{fname}/index"]
        for b in range(c["B"]):
            n = int(count[b])
            assert len(set(index[b, :n])) == n and (index[b, n:] == -1).all()
            s, l = gold[f"{name}/{fname}/scores"][b, :n], gold[f"{name}/{fname}/labels"][b, :n]
            assert (s >= st).all()
            if aware:                                          # labels ascending, each label's picks by descending score
                assert (np.diff(l) >= 0).all() and all((np.diff(s[l == k]) < 0).all() for k in set(l))
            else:
                assert (np.diff(s) < 0).all()
    special = {"all_below": lambda n: n == 0, "near_identical": lambda n: n == 1}
    if name in special:
        assert all(special[name](int(gold[f"{name}/{f}/count"][0])) for f in ("plain_005_05", "plain_03_03"))
    if name == "disjoint":                                     # everything that passes the score filter is kept
        scores = cases.post_process64(logits[0], boxes[0])[0]
        for fname, _, st, _ in cases.FLAVOURS:
            assert int(gold[f"{name}/{fname}/count"][0]) == int((scores >= st).sum())


def test_library_exports_and_abi():
    header = open(os.path.join(ROOT, "include", "lgd_hip.h")).read()
    assert "#define LGD_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12
    for name in ("lgd_owl_heads_f32", "lgd_detect_nms_f32"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]) == 17
    assert callable(ops.owl_heads) and callable(ops.detect_nms)
    assert os.path.exists(_lib.LIB_PATH), "build() leaves the library in the tree"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "lgd_owl_heads_f32") and hasattr(lib, "lgd_detect_nms_f32") and lib.lgd_abi_version() == 12
    # argument checks answer before anything touches a device
    lib.lgd_detect_nms_f32.argtypes = _lib.SIGNATURES["lgd_detect_nms_f32"]
    lib.lgd_owl_heads_f32.argtypes = _lib.SIGNATURES["lgd_owl_heads_f32"]
    p = ctypes.c_void_p(64)
    assert lib.lgd_detect_nms_f32(0, p, p, None, None, 1, 4097, 1, 0.1, 0.5, 0, p, p, p, p, p, None) == -3
    assert lib.lgd_detect_nms_f32(2, p, p, None, None, 1, 16, 1, 0.1, 0.5, 0, p, p, p, p, p, None) == -1
    assert lib.lgd_detect_nms_f32(0, p, ctypes.c_void_p(68), None, None, 1, 16, 1, 0.1, 0.5, 0, p, p, p, p, p, None) == -1
    assert lib.lgd_owl_heads_f32(p, 1032, p, None, p, p, 1, p, 1, p, p, p, 1, 1, 1, 1032, None) == -3
    assert lib.lgd_owl_heads_f32(p, 64, p, None, p, p, 1, p, 1, p, p, p, 1, 1, 65, 64, None) == -3
    assert lib.lgd_owl_heads_f32(p, 32, p, None, p, p, 1, p, 1, p, p, p, 1, 1, 1, 64, None) == -1


@pytest.mark.parametrize("g", [6, 24])
def test_box_bias_table_matches_transformers(g):
    transformers = pytest.importorskip("transformers")
    cfg = cases.tiny_hf_config()
    cfg.vision_config.image_size = g * cfg.vision_config.patch_size
    hf = transformers.OwlViTForObjectDetection(cfg)
    want = hf.compute_box_bias(g, g)
    got = owlvit.compute_box_bias(g, g)
    assert got.shape == (g * g, 4) and got.dtype == torch.float32
    assert float((got - want).abs().max()) <= 1e-7


def test_from_hf_consumes_the_state_dict():
    transformers = pytest.importorskip("transformers")
    hf = cases.redraw_weights(transformers.OwlViTForObjectDetection(cases.tiny_hf_config()), seed=0)
    det = owlvit.from_hf(hf, device="cpu")
    sd = hf.state_dict()
    assert det.consumed | set(det.unused) == set(sd) and not det.consumed & set(det.unused)
    assert set(det.unused) <= set(owlvit.UNUSED_KEYS)
    assert {"owlvit.visual_projection.weight", "owlvit.logit_scale"} <= set(det.unused)
    assert all(k.endswith("position_ids") or "visual_projection" in k or k == "owlvit.logit_scale" for k in owlvit.UNUSED_KEYS)
    assert det.P == 36 and det.grid == 6 and det.cfg == owlvit.OwlViTConfig.from_hf(hf.config)
    with pytest.raises(RuntimeError, match="does not know"):
        owlvit.HipOwlViTDetector(det.cfg, dict(sd, stray=torch.zeros(1)), "cpu")


def test_dropin_eval_package_resolves_lmd_to_the_reference():
    import ref_harness
    if not ref_harness.available():
        pytest.skip("needs the reference checkout")
    code = ("import utils.eval as e, utils.eval.eval as ee, importlib.util as u, os\n"
            "assert ee.__file__.startswith(os.environ['DROPIN']), ee.__file__\n"
            "assert e.eval_prompt is ee.eval_prompt and callable(e.nms) and callable(e.eval_images)\n"
            "s = u.find_spec('utils.eval.lmd')\n"
            "assert s is not None and s.origin.startswith(os.environ['LGD_REFERENCE_ROOT']), s\n"
            "print('ok')\n")
    env = dict(os.environ, LGD_REFERENCE_ROOT=ref_harness.REF_ROOT, DROPIN=DROPIN,
               PYTHONPATH=os.pathsep.join([ROOT, DROPIN]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


def test_dropin_eval_keeps_the_reference_signatures():
    """Names, parameters and defaults of utils/eval/eval.py (recorded here from the reference's file)."""
    import inspect
    import importlib.util
    spec = importlib.util.spec_from_file_location("lgd_dropin_eval_sig", os.path.join(DROPIN, "utils", "eval", "eval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = {
        "get_eval_info_from_prompt": "(prompt, prompt_type)",
        "nms": "(bounding_boxes, confidence_score, labels, threshold, input_in_pixels=False, return_array=True)",
        "class_aware_nms": "(bounding_boxes, confidence_score, labels, threshold, input_in_pixels=False)",
        "evaluate_with_boxes": "(boxes, eval_info, verbose=False)",
        "to_gen_box_format": "(box, width, height)",
        "eval_prompt": "(p, prompt_type, path, processor, model, score_threshold=0.1, nms_threshold=0.5, "
                       "use_class_aware_nms=False, verbose=False, use_cuda=True)",
    }
    for name, sig in want.items():
        assert str(inspect.signature(getattr(mod, name))) == sig, name
    assert mod.to_gen_box_format((0.25, 0.5, 0.75, 1.0), 200, 100) == [50.0, 50.0, 100.0, 50.0]
    with pytest.raises(ValueError):
        mod.get_eval_info_from_prompt("x", "other")
