"""CPU suite of the plain Stable Diffusion baseline (`sd`): the PNDM (PLMS) scheduler's table form against a stateful
line-for-line restatement of diffusers 0.18.0 PNDMScheduler (tests/pndm_restate.py) and against DDIM, the ABI of the fused
PLMS step, the golden's reproducibility, and the drop-in plugin surface with the engine mocked."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import lgd_amd  # noqa: E402,F401
from lgd_amd import _lib  # noqa: E402
from lgd_amd.scheduler import DDIMScheduler, PNDMScheduler  # noqa: E402
from pndm_restate import PNDMRestate  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "run_sd_generate_tiny.npz")
D = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("n", [5, 10, 30, 50])
def test_pndm_table_form_matches_the_stateful_restatement(n, pred):
    ours, ref = PNDMScheduler(prediction_type=pred), PNDMRestate(prediction_type=pred, dtype=D)
    ours.set_timesteps(n)
    ref.set_timesteps(n)
    assert ours.timesteps.tolist() == ref.timesteps.tolist()
    assert len(ours.timesteps) == n + 1
    g = torch.Generator().manual_seed(n + (7 if pred == "v_prediction" else 0))
    x_ours = x_ref = torch.randn((2, 4, 8, 8), generator=g, dtype=D)
    state = ours.host_state(x_ours)
    worst = 0.0
    for k, t in enumerate(ours.timesteps):
        m = torch.randn((2, 4, 8, 8), generator=g, dtype=D)
        x_ours = ours.step_host(m, k, x_ours, state)
        x_ref = ref.step(m, t, x_ref).prev_sample
        worst = max(worst, _rel(x_ours, x_ref))
    print(f"n={n} {pred}: max rel {worst:.3e}")
    assert worst <= 1e-12


def test_five_steps_reach_every_order_branch():
    s = PNDMScheduler()
    s.set_timesteps(5)
    rows = s.plms_rows()
    assert len(rows) == 6
    t = s.timesteps.tolist()
    assert t == [801, 601, 601, 401, 201, 1]
    # (w_m, ring weights, push slot, from_cur, save_cur) per evaluation
    want = [(1.0, (0, 0, 0), 0, 0, 1),                         # first order, saves the sample
            (0.5, (0.5, 0, 0), -1, 1, 0),                      # averaged re-evaluation from the saved sample, no push
            (1.5, (-0.5, 0, 0), 1, 0, 0),
            (23 / 12, (5 / 12, -16 / 12, 0), 2, 0, 0),
            (55 / 24, (-9 / 24, 37 / 24, -59 / 24), 0, 0, 0),  # the oldest output sits in the slot being pushed to
            (55 / 24, (-59 / 24, -9 / 24, 37 / 24), 1, 0, 0)]
    for k, (row, w) in enumerate(zip(rows, want)):
        wm, w0, w1, w2, a, b, push, fc, sv = row
        assert (wm, push, fc, sv) == (w[0], w[2], w[3], w[4]), k
        assert np.allclose((w0, w1, w2), w[1], rtol=0, atol=1e-15), k
        assert abs(wm + w0 + w1 + w2 - 1.0) < 1e-14                # the PLMS weights sum to one
    # the restatement takes the same branches: its history lengths / counter over the run
    ref = PNDMRestate(dtype=D)
    ref.set_timesteps(5)
    seen = []
    x = torch.zeros(1, dtype=D)
    for t in ref.timesteps:
        x = ref.step(torch.ones(1, dtype=D), t, x).prev_sample
        seen.append((len(ref.ets), ref.counter))
    assert seen == [(1, 1), (1, 2), (2, 3), (3, 4), (4, 5), (4, 6)]


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("n", [5, 50])
def test_constant_prediction_plms_equals_ddim(n, pred):
    """PLMS weights sum to 1 and _get_prev_sample is algebraically the DDIM (eta = 0) update: with a constant model
    output the whole run equals DDIM on the same timesteps (evaluation k >= 1 lands where DDIM step k - 1 does)."""
    p, d = PNDMScheduler(prediction_type=pred), DDIMScheduler(prediction_type=pred)
    p.set_timesteps(n)
    d.set_timesteps(n)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn((1, 4, 8, 8), generator=g, dtype=D)
    m = torch.randn((1, 4, 8, 8), generator=g, dtype=D)
    xd, traj_d = x0, []
    for t in d.timesteps:
        xd = d.step(m, t, xd).prev_sample
        traj_d.append(xd)
    xp, state, traj_p = x0, p.host_state(x0), []
    for k in range(len(p.timesteps)):
        xp = p.step_host(m, k, xp, state)
        traj_p.append(xp)
    assert _rel(traj_p[0], traj_d[0]) < 1e-12
    for k in range(1, len(traj_p)):
        assert _rel(traj_p[k], traj_d[k - 1]) < 1e-12, k


def test_pndm_refuses_what_it_does_not_implement():
    with pytest.raises(NotImplementedError):
        PNDMScheduler(skip_prk_steps=False)
    with pytest.raises(NotImplementedError):
        PNDMScheduler(set_alpha_to_one=True)
    with pytest.raises(RuntimeError):
        PNDMScheduler().coef_table(7.5, "cpu")
    s = PNDMScheduler.from_config(DDIMScheduler(prediction_type="v_prediction"))
    assert s.config.prediction_type == "v_prediction" and s.config.steps_offset == 1
    assert s.config.skip_prk_steps and not s.config.set_alpha_to_one and s.init_noise_sigma == 1.0


def test_plms_table_layout():
    s = PNDMScheduler()
    s.set_timesteps(50)
    tab = s.plms_table(7.5, "cpu")
    assert tab.shape == (51, 16) and tab.dtype == torch.float32
    assert torch.all(tab[:, 6] == 7.5) and torch.all(tab[:, 10:] == 0)
    assert tab[1, 7] == -1 and set(tab[:, 7].tolist()) == {-1.0, 0.0, 1.0, 2.0}


def test_library_exports_the_plms_step():
    import __graft_entry__ as ge
    import re
    ge.build()
    lib = _lib.load()
    assert hasattr(lib, "lgd_cfg_plms_step_f32")
    assert len(_lib.SIGNATURES["lgd_cfg_plms_step_f32"]) == 12
    hdr = open(os.path.join(ROOT, "include", "lgd_hip.h")).read()
    ver = int(re.search(r"#define LGD_ABI_VERSION (\d+)", hdr).group(1))
    assert ver == _lib.ABI_VERSION == lib.lgd_abi_version() == 12


def test_golden_regenerates_bit_identically(tmp_path):
    import ref_harness
    if not ref_harness.available():
        pytest.skip("the reference tree is not present")
    out = tmp_path / "sd.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_sd.py"), "--out", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    new, old = np.load(out), np.load(GOLD)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(new[k], old[k]), k


def test_golden_is_consistent_with_the_restatement():
    """The golden's own evaluation records: n + 1 UNet calls under PNDM on the PLMS schedule, n under DDIM; the start
    latents and text embeddings regenerated from their seeds are the ones the golden was made from."""
    from lgd_amd import weights
    from sd_golden_cases import CASES, case_inputs, checksum, sample_index
    z = np.load(GOLD)
    idx = z["sample_index"]
    assert np.array_equal(idx, sample_index(4 * 32 * 32))
    for case, cfg_name, _, n, seed in CASES:
        evals = n + 1 if case.endswith("pndm") else n
        assert int(z[f"{case}/steps"]) == n
        assert z[f"{case}/inputs_sample"].shape == (evals, idx.size)
        lat, text = case_inputs(weights.CONFIGS[cfg_name], seed)
        assert np.array_equal(checksum(lat), z[f"{case}/latents0_checksum"]), case
        assert np.array_equal(checksum(text), z[f"{case}/text_checksum"]), case
        assert np.array_equal(z[f"{case}/inputs_sample"][0], lat.reshape(-1).numpy()[idx])
    s = PNDMScheduler()
    s.set_timesteps(50)
    assert z["tiny_pndm/timesteps"].tolist() == s.timesteps.tolist()


# ---- drop-in plugin surface (engine mocked: no GPU here)
@pytest.fixture
def dropin(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    import models
    from fake_text import FakeTextEncoder, FakeTokenizer

    class _Unet:
        config = type("C", (), dict(sample_size=64, in_channels=4))()
    md = models.models._EasyDict(tokenizer=FakeTokenizer(), text_encoder=FakeTextEncoder(128, "cpu"), unet=_Unet(),
                                 scheduler=DDIMScheduler(), sampler=object(), vae=None, dtype=torch.float32)
    monkeypatch.setattr(models, "model_dict", md)
    monkeypatch.setattr(models.models, "torch_device", "cpu")        # encode_prompts moves the token ids there
    return models


def test_sd_plugin_surface(dropin, monkeypatch):
    import generation.stable_diffusion_generate as g
    from generation._common import DEFAULT_OVERALL_NEGATIVE_PROMPT
    assert g.version == "sd" and g.num_total_steps == 50 and g.generate_guidance_scale == 7.5
    assert g.negative_prompt("") == DEFAULT_OVERALL_NEGATIVE_PROMPT
    assert g.negative_prompt("x") == "x, " + DEFAULT_OVERALL_NEGATIVE_PROMPT
    seen = {}
    orig_encode = dropin.encode_prompts

    def encode(**kw):
        seen["negative_prompt"], seen["prompts"] = kw["negative_prompt"], kw["prompts"]
        return orig_encode(**kw)

    def fake_batch(sampler, texts, latents, steps, guidance_scale, scheduler):
        seen.update(texts=texts, latents=latents, steps=steps, gs=guidance_scale, scheduler=scheduler)
        return latents, np.zeros((1, 512, 512, 3), np.uint8)
    monkeypatch.setattr(dropin, "encode_prompts", encode)
    monkeypatch.setattr(g, "sd_generate_batch", fake_batch)
    monkeypatch.setattr(g, "start_latents", lambda seed, c, h, w: torch.randn((1, c, h // 8, w // 8),
                                                                            generator=torch.Generator().manual_seed(seed)))
    out = g.run("a cat", seed=7, extra_neg_prompt="blurry dog")
    assert seen["negative_prompt"] == "blurry dog, " + DEFAULT_OVERALL_NEGATIVE_PROMPT and seen["prompts"] == ["a cat"]
    assert seen["texts"][0].shape == (2, 77, 128)
    assert seen["latents"].shape == (1, 4, 64, 64) and seen["steps"] == 50 and seen["gs"] == 7.5
    assert isinstance(seen["scheduler"], PNDMScheduler)
    assert out.image.size == (512, 512) and out.image.mode == "RGB"


def test_refine_accepts_a_pil_image(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    from PIL import Image
    import generation.sdxl_refinement as r
    got = []

    class _Pipe:
        def refine(self, resized, seed, strength, **text):
            got.append(resized)
            return np.zeros((1024, 1024, 3), np.uint8)
    monkeypatch.setattr(r, "pipe", _Pipe())
    arr = np.random.default_rng(0).integers(0, 256, (512, 512, 3), dtype=np.uint8)
    spec = dict(prompt="a cat", extra_neg_prompt="")
    a = r.refine(arr, spec, 1)
    b = r.refine(Image.fromarray(arr), spec, 1)
    assert isinstance(a, Image.Image) and isinstance(b, Image.Image)
    assert got[0].shape == (1024, 1024, 3) and np.array_equal(got[0], got[1])
