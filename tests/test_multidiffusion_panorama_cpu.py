"""MultiDiffusion over several views, host side: get_views, the RNG protocol with one pick per view, the plugin's
sd.generate surface and the new library export, against tests/golden/run_multidiffusion_panorama_tiny.npz and
multidiffusion_panorama_surface.json (tools/make_golden_multidiffusion_panorama.py: the reference's own
MultiDiffusion.generate on CPU)."""
import ctypes
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lgd_amd  # noqa: E402,F401
from lgd_amd import multidiffusion as mdc  # noqa: E402
import md_golden_cases as md_cases  # noqa: E402
import md_pano_golden_cases as cases  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "run_multidiffusion_panorama_tiny.npz")
OLD_GOLDEN = os.path.join(ROOT, "tests", "golden", "run_multidiffusion_tiny.npz")
SURFACE = os.path.join(ROOT, "tests", "golden", "multidiffusion_panorama_surface.json")
DROPIN = os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin")
IDS = [c["name"] for c in cases.CASES]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.mark.parametrize("c", cases.CASES, ids=IDS)
def test_get_views_matches_reference(gold, c):
    views = mdc.get_views(c["height"], c["width"])
    assert len(views) == c["views"]
    assert all(isinstance(v, tuple) and all(type(i) is int for i in v) for v in views)
    assert views == [tuple(int(i) for i in row) for row in gold[f"{c['name']}/views"]]


def test_get_views_counts():
    assert len(mdc.get_views(512, 2048)) == 25 and mdc.get_views(512, 2048)[-1] == (0, 64, 192, 256)
    assert mdc.get_views(512, 512) == [(0, 64, 0, 64)]
    assert mdc.get_views(516, 512) == [(0, 64, 0, 64)]              # 64.5 latent rows are still one window
    assert mdc.get_views(576, 640)[4] == (8, 72, 8, 72)             # row-major: view 4 is row 1, column 1


@pytest.mark.parametrize("c", cases.CASES, ids=IDS)
def test_rng_protocol_matches_reference(gold, c):
    name, P, n_boot = c["name"], len(c["prompts"]), c["n_boot"]
    d = mdc.draw_randomness(md_cases.StandInVAE(), "cpu", c["seed"], n_boot, P, c["steps"],
                            size=(c["height"], c["width"]), n_views=c["views"], bg_size=cases.BG_SIZE)
    hp, wp = c["height"] // 8, c["width"] // 8
    assert tuple(d["start_latent"].shape) == (1, 4, hp, wp)
    sidx = md_cases.sample_index(4 * hp * wp)
    np.testing.assert_array_equal(d["start_latent"].reshape(-1)[sidx].numpy(), gold[f"{name}/start_sample"])
    np.testing.assert_array_equal(md_cases.checksum(d["start_latent"]), gold[f"{name}/start_checksum"])
    np.testing.assert_array_equal(d["picks"].reshape(min(n_boot, c["steps"]), c["views"], P - 1).numpy(), gold[f"{name}/picks"])
    if n_boot:
        np.testing.assert_array_equal(d["colours"].numpy(), gold[f"{name}/colours"])
        assert tuple(d["bg_latents"].shape) == (n_boot, 4, 64, 64)
        idx = gold["sample_index"]
        np.testing.assert_array_equal(d["bg_latents"].reshape(n_boot, -1)[:, idx].numpy(), gold[f"{name}/bg_sample"])
        np.testing.assert_array_equal(md_cases.checksum(d["bg_latents"]), gold[f"{name}/bg_checksum"])
    else:
        assert d["colours"] is None and d["bg_latents"] is None


def test_one_view_draws_what_it_always_drew():
    """n_views=1 (the default) is the single-view protocol: the same numbers and the same shapes as the golden of the
    baseline, whether the keyword is passed or not."""
    old = np.load(OLD_GOLDEN)
    name, _, _, steps, n_boot, _, _, seed = next(c for c in md_cases.CASES if c[0] == "three_back")
    P = len(old[f"{name}/prompts"])
    for kw in ({}, dict(n_views=1, bg_size=(512, 512))):
        d = mdc.draw_randomness(md_cases.StandInVAE(), "cpu", seed, n_boot, P, steps, **kw)
        assert tuple(d["picks"].shape) == (min(n_boot, steps), P - 1)
        np.testing.assert_array_equal(d["picks"].numpy(), old[f"{name}/picks"])
        np.testing.assert_array_equal(d["colours"].numpy(), old[f"{name}/colours"])
        np.testing.assert_array_equal(md_cases.checksum(d["start_latent"]), old[f"{name}/start_checksum"])
        np.testing.assert_array_equal(md_cases.checksum(d["bg_latents"]), old[f"{name}/bg_checksum"])


def test_uncovered_columns_are_zero_in_the_golden(gold):
    assert np.all(gold["uncovered/final"][..., 64:] == 0) and np.any(gold["uncovered/final"][..., :64] != 0)


def test_case_masks():
    m = cases.build_masks(cases.case("grid"))
    assert tuple(m.shape) == (3, 1, 72, 80) and m.dtype == torch.float32
    assert sorted(set(m[1].reshape(-1).tolist())) == pytest.approx([0.0, 0.3, 0.7])   # the soft mask
    assert float(m.sum(0).min()) == pytest.approx(1.0) and float(m.sum(0).max()) == pytest.approx(1.0)


def _dropin():
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import generation.multidiffusion as m
    return m


def _check_signature(fn, want, skip_self=False):
    params = list(inspect.signature(fn).parameters.values())[1 if skip_self else 0:]
    assert [p.name for p in params] == want["params"]
    assert {p.name: p.default for p in params if p.default is not inspect.Parameter.empty} == want["defaults"]


def test_plugin_exports_get_views_and_generate():
    s = json.load(open(SURFACE))
    m = _dropin()
    _check_signature(m.get_views, s["get_views"])
    assert m.get_views(512, 768) == mdc.get_views(512, 768) and len(m.get_views(512, 768)) == 5
    _check_signature(m.MultiDiffusion.generate, s["generate"], skip_self=True)
    sd = m.MultiDiffusion(sampler=None, encoder=None, tokenizer=object(), text_encoder=object(), device="cpu")
    assert sd.sampler is None and sd["device"] == "cpu"                # still the attribute dict run() reads
    _check_signature(sd.generate, s["generate"])
    with pytest.raises(TypeError):                                     # the seed is required, as in the reference
        sd.generate(torch.ones(1, 1, 64, 64), ["a lake"])


def test_library_exports_the_view_step_and_keeps_abi_12():
    from lgd_amd import _lib, ops
    assert len(_lib.SIGNATURES["lgd_multidiffusion_views_f32"]) == 27
    assert _lib.ABI_VERSION == 12
    header = open(os.path.join(ROOT, "include", "lgd_hip.h")).read()
    assert "#define LGD_ABI_VERSION 12" in header and "int lgd_multidiffusion_views_f32(" in header
    assert callable(ops.multidiffusion_views)
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert hasattr(lib, "lgd_multidiffusion_views_f32")
        assert lib.lgd_abi_version() == 12


def test_golden_regenerates_bit_for_bit(tmp_path):
    import ref_harness
    if not ref_harness.available():
        pytest.skip("needs the reference checkout")
    import subprocess
    out, surf = tmp_path / "md.npz", tmp_path / "s.json"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_multidiffusion_panorama.py"), "--out",
                    str(out), "--surface-out", str(surf)], check=True, capture_output=True, timeout=1800)
    new, old = np.load(out), np.load(GOLDEN)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    assert json.load(open(surf)) == json.load(open(SURFACE))
