"""MultiDiffusion baseline, host side: prep, the RNG protocol, add_noise, the truncating image conversion and the plugin
surface against tests/golden/run_multidiffusion_tiny.npz and multidiffusion_surface.json (tools/make_golden_multidiffusion.py,
the reference's own generation/multidiffusion.py on CPU)."""
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
from lgd_amd.scheduler import DDIMScheduler  # noqa: E402
import md_golden_cases as cases  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "run_multidiffusion_tiny.npz")
SURFACE = os.path.join(ROOT, "tests", "golden", "multidiffusion_surface.json")
DROPIN = os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _surface():
    return json.load(open(SURFACE))


def _prep(case):
    name, boxes, bg_prompt, steps, n_boot, first_top, neg, seed = case
    c = _surface()["constants"]
    return mdc.prepare(boxes, bg_prompt, c["bg_negative"], c["fg_negative_prompt"], extra_neg_prompt=neg,
                       first_top=first_top)


@pytest.mark.parametrize("case", cases.CASES, ids=[c[0] for c in cases.CASES])
def test_host_prep_matches_reference(gold, case):
    p = _prep(case)
    name = case[0]
    assert p["prompts"] == list(gold[f"{name}/prompts"])
    assert p["negative_prompts"] == list(gold[f"{name}/negative_prompts"])
    assert p["masks"].dtype == torch.float32
    np.testing.assert_array_equal(p["masks"].numpy(), gold[f"{name}/masks"])


def test_host_prep_first_top_and_rescale(gold):
    # the overlap goes to the last box without first_top and to the first with it; the out-of-bounds box is moved in
    back, top = gold["three_back/masks"], gold["three_top/masks"]
    assert not np.array_equal(back, top)
    assert (back[1:].sum(0) <= 1).all() and (top[1:].sum(0) <= 1).all()
    assert back[3].sum() > top[3].sum() and back[1].sum() < top[1].sum()
    oob = mdc.filter_boxes([{"name": "a boat.", "bounding_box": [-40, 300, 300, 260]}])
    assert oob[0]["name"] == "a boat" and oob[0]["bounding_box"][0] == 0
    assert mdc.prepare([], "x", "a", "b")["masks"].shape == (1, 1, 64, 64)


@pytest.mark.parametrize("case", cases.CASES, ids=[c[0] for c in cases.CASES])
def test_rng_protocol_matches_reference(gold, case):
    name, boxes, bg_prompt, steps, n_boot, first_top, neg, seed = case
    P = len(gold[f"{name}/prompts"])
    d = mdc.draw_randomness(cases.StandInVAE(), "cpu", seed, n_boot, P, steps)
    np.testing.assert_array_equal(d["colours"].numpy(), gold[f"{name}/colours"])
    np.testing.assert_array_equal(d["picks"].numpy(), gold[f"{name}/picks"])
    idx = gold["sample_index"]
    np.testing.assert_array_equal(d["start_latent"].reshape(-1)[idx].numpy(), gold[f"{name}/start_sample"])
    np.testing.assert_array_equal(cases.checksum(d["start_latent"]), gold[f"{name}/start_checksum"])
    bg = d["bg_latents"]
    np.testing.assert_array_equal(bg.reshape(n_boot, -1)[:, idx].numpy(), gold[f"{name}/bg_sample"])
    np.testing.assert_array_equal(cases.checksum(bg), gold[f"{name}/bg_checksum"])
    # the input of step 0 is the start latent for prompt 0 (never bootstrapped)
    np.testing.assert_array_equal(gold[f"{name}/inputs_sample"][0, 0], gold[f"{name}/start_sample"])


def test_add_noise_against_fp64():
    s = DDIMScheduler()
    g = torch.Generator().manual_seed(3)
    x, n = torch.randn(3, 4, 8, 8, generator=g), torch.randn(3, 4, 8, 8, generator=g)
    for t in (1, 481, 981):
        a = s.alphas_cumprod[t].double()
        want = a.sqrt() * x.double() + (1 - a).sqrt() * n.double()
        got = s.add_noise(x, n, torch.tensor(t))
        assert got.dtype == torch.float32
        assert (got.double() - want).abs().max() < 1e-6
    got = s.add_noise(x, n, torch.tensor([1, 481, 981]))
    for i, t in enumerate((1, 481, 981)):
        torch.testing.assert_close(got[i], s.add_noise(x[i], n[i], t), rtol=0, atol=0)


def test_truncating_image_conversion(gold):
    v = torch.tensor([0.0, 0.999, 0.5, 1.0, 0.00392, 0.996]).reshape(1, 3, 1, 2)
    out = mdc.to_uint8_truncating(v)
    assert out.dtype == np.uint8 and out.shape == (1, 1, 2, 3)
    assert out[0, 0, :, :].T.reshape(-1).tolist() == [0, 254, 127, 255, 0, 253]
    # the golden image is the stand-in decoder's output of the final latent, converted this way
    name = "two"
    img = mdc.decode_truncating(_Decode(cases.StandInVAE()), torch.from_numpy(gold[f"{name}/final"]))[0]
    # (the CPU convolutions round differently with the thread count: a value on a level boundary may truncate to the
    # level below, so single levels may differ)
    d = np.abs(img[::8, ::8].astype(int) - gold[f"{name}/image_sub"].astype(int))
    assert d.max() <= 1 and (d > 0).mean() < 1e-3
    a = img.astype(np.float64)
    np.testing.assert_allclose(np.array([a.sum(), (a * a).sum()]), gold[f"{name}/image_checksum"], rtol=1e-5)


class _Decode:
    def __init__(self, vae):
        self.vae = vae

    def decode(self, z):
        return self.vae.decode(z).sample


def _dropin():
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import generation.multidiffusion as m
    return m


def test_plugin_surface_matches_reference():
    s = _surface()
    m = _dropin()
    assert m.version == s["constants"]["version"] == "multidiffusion"
    assert m.bg_negative == s["constants"]["bg_negative"]
    assert m.fg_negative_prompt == s["constants"]["fg_negative_prompt"]
    sig = inspect.signature(m.run)
    assert list(sig.parameters) == s["params"]
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == s["defaults"]
    with pytest.raises(TypeError):
        m.run([], "a lake", original_ind_base=1, generate_kw={"height": 512})


def test_library_exports_the_step_and_keeps_abi_12():
    from lgd_amd import _lib
    assert len(_lib.SIGNATURES["lgd_multidiffusion_step_f32"]) == 18
    assert _lib.ABI_VERSION == 12
    header = open(os.path.join(ROOT, "include", "lgd_hip.h")).read()
    assert "#define LGD_ABI_VERSION 12" in header and "int lgd_multidiffusion_step_f32(" in header
    if os.path.exists(_lib.LIB_PATH):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert hasattr(lib, "lgd_multidiffusion_step_f32")
        assert lib.lgd_abi_version() == 12


def test_golden_regenerates_bit_for_bit(tmp_path):
    import ref_harness
    if not ref_harness.available():
        pytest.skip("needs the reference checkout")
    import subprocess
    out, surf = tmp_path / "md.npz", tmp_path / "s.json"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_multidiffusion.py"), "--out", str(out),
                    "--surface-out", str(surf)], check=True, capture_output=True, timeout=1800)
    new, old = np.load(out), np.load(GOLDEN)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    assert json.load(open(surf)) == _surface()
