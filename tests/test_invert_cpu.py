"""CPU suite of DDIM inversion: lgd_amd.scheduler.DDIMInverseScheduler's schedule and table form against a stateful
line-for-line restatement of diffusers 0.18.0 DDIMInverseScheduler (tests/ddim_inverse_restate.py) and against the forward
DDIM step that undoes it, its refusals, the ABI of the two encode kernels, and the golden's reproducibility."""
import os
import re
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
from lgd_amd.scheduler import DDIM, DDIMInverseScheduler, DDIMScheduler  # noqa: E402
from ddim_inverse_restate import DDIMInverseRestate  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "run_invert_tiny.npz")
D = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _row_step(row, m, x):
    """One table row {alpha_bar_t, alpha_bar_next, guidance_scale, v flag} applied as lgd_cfg_ddim_step_f32 does, in fp64."""
    a_t, a_n, _, v = (float(c) for c in row)
    sa, sb, pa, pb = a_t ** 0.5, (1 - a_t) ** 0.5, a_n ** 0.5, (1 - a_n) ** 0.5
    if v:
        x0, e = sa * x - sb * m, sa * m + sb * x
    else:
        x0, e = (x - sb * m) / sa, m
    return pa * x0 + pb * e


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [3, 10, 50])
def test_schedule_and_table_match_the_stateful_restatement(n, offset, pred):
    base = DDIMScheduler(steps_offset=offset, prediction_type=pred)
    ours = DDIMInverseScheduler.from_config(base.config)
    ref = DDIMInverseRestate.from_config(base.config, dtype=D)
    assert ours.step_kind == DDIM and ours.init_noise_sigma == 1.0
    assert float(ours.final_alpha_cumprod) == float(ref.final_alpha_cumprod) == float(base.alphas_cumprod[-1])
    ours.set_timesteps(n)
    ref.set_timesteps(n)
    assert ours.timesteps.tolist() == ref.timesteps.tolist() == [i * (1000 // n) + offset for i in range(n)]
    tab = ours.coef_table(7.5, "cpu")
    assert tab.shape == (n, 4) and tab.dtype == torch.float32
    assert torch.all(tab[:, 2] == 7.5) and torch.all(tab[:, 3] == (1.0 if pred == "v_prediction" else 0.0))
    assert ours.dynamic_step_sizes(ours.timesteps) is None      # what loop.StepKernel.load hands to coef_table
    assert torch.equal(tab, ours.coef_table(7.5, "cpu", timesteps=ours.timesteps, step_ratios=None))
    g = torch.Generator().manual_seed(17 * n + offset)
    x = torch.randn((2, 4, 8, 8), generator=g, dtype=D)
    assert ours.scale_model_input(x, 1) is x
    worst = 0.0
    for i, t in enumerate(ours.timesteps):                       # the last index takes the final-alpha rule
        m = torch.randn((2, 4, 8, 8), generator=g, dtype=D)
        want = ref.step(m, t, x).prev_sample
        worst = max(worst, _rel(_row_step(tab[i].double(), m, x), want), _rel(ours.step(m, t, x).prev_sample, want))
        x = want
    print(f"n={n} offset={offset} {pred}: max rel {worst:.3e}")
    assert worst <= 1e-12
    last_next = int(ours.timesteps[-1]) + 1000 // n
    want_last = float(base.alphas_cumprod[last_next]) if last_next < 1000 else float(base.alphas_cumprod[-1])
    assert float(tab[-1, 1]) == np.float32(want_last)


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("n", [3, 10, 50])
def test_forward_ddim_step_undoes_the_inverse_step(n, pred):
    """x --inverse step from t--> x' --DDIMScheduler.step from t_next--> x, at every index whose t_next lies on the training
    schedule (the last index of a steps_offset=1 schedule steps past it: the one entry `invert` never takes).  epsilon: the
    same model output both ways.  v_prediction: v depends on the noise level it is read at, so the forward step gets the v
    of the same (x0, epsilon) pair at t_next."""
    fwd = DDIMScheduler(prediction_type=pred)
    inv = DDIMInverseScheduler.from_config(fwd.config)
    fwd.set_timesteps(n)
    inv.set_timesteps(n)
    g = torch.Generator().manual_seed(n)
    checked = 0
    for t in inv.timesteps:
        t_next = int(t) + 1000 // n
        if t_next >= 1000:
            continue
        assert t_next in fwd.timesteps.tolist() and fwd.prev_timestep(t_next) == int(t)
        x = torch.randn((1, 4, 8, 8), generator=g, dtype=D)
        m = torch.randn((1, 4, 8, 8), generator=g, dtype=D)
        x_up = inv.step(m, t, x).prev_sample
        m_back = m
        if pred == "v_prediction":
            a_t, a_n = inv.alpha_pair(t)
            x0, e = a_t ** 0.5 * x - (1 - a_t) ** 0.5 * m, a_t ** 0.5 * m + (1 - a_t) ** 0.5 * x
            m_back = a_n ** 0.5 * e - (1 - a_n) ** 0.5 * x0
        back = fwd.step(m_back, t_next, x_up).prev_sample
        assert _rel(back, x) <= 1e-12, int(t)
        checked += 1
    assert checked == n - 1


def test_inverse_scheduler_refuses_guided_and_fast_use():
    from lgd_amd.sampler import LMDSampler
    s = DDIMInverseScheduler()
    s.set_timesteps(10)
    with pytest.raises(RuntimeError):
        s.guidance_step_table("cpu")                             # the latent update of backward guidance
    with pytest.raises(RuntimeError):
        s.coef_table(7.5, "cpu", step_ratios=[100] * 10)         # per-step sizes of the fast schedule
    with pytest.raises(RuntimeError):
        s.fast_schedule(s.timesteps, 4)
    with pytest.raises(RuntimeError):
        s.add_noise(torch.zeros(1), torch.zeros(1), 1)
    with pytest.raises(NotImplementedError):
        DDIMInverseScheduler(prediction_type="sample")
    off = dict(fast=False, partial=False, conditioned=False)
    LMDSampler._refuse_undefined(DDIM, inverse=True, **off)       # the plain CFG loop passes
    for what in off:
        with pytest.raises(RuntimeError):
            LMDSampler._refuse_undefined(DDIM, inverse=True, **dict(off, **{what: True}))
        LMDSampler._refuse_undefined(DDIM, **dict(off, **{what: True}))      # descending DDIM defines all three


def test_library_exports_the_encode_kernels():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    for name, nargs in (("lgd_image_u8_to_nhwc8_f16", 6), ("lgd_vae_sample_f32", 8)):
        assert hasattr(lib, name)
        assert len(_lib.SIGNATURES[name]) == nargs
    hdr = open(os.path.join(ROOT, "include", "lgd_hip.h")).read()
    ver = int(re.search(r"#define LGD_ABI_VERSION (\d+)", hdr).group(1))
    assert ver == _lib.ABI_VERSION == lib.lgd_abi_version() == 12


def test_get_inverse_timesteps():
    sys.path.insert(0, os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    from models import pipelines
    s = DDIMInverseScheduler()
    s.set_timesteps(10)
    ts, n = pipelines.get_inverse_timesteps(s, 10, strength=1.0)
    assert n == 10 and ts.tolist() == s.timesteps.tolist()
    ts, n = pipelines.get_inverse_timesteps(s, 10, strength=0.35)
    assert n == 3 and ts.tolist() == [1, 101, 201]


def test_golden_regenerates_bit_identically(tmp_path):
    import ref_harness
    if not ref_harness.available():
        pytest.skip("the reference tree is not present")
    out = tmp_path / "invert.npz"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_invert.py"), "--out", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    new, old = np.load(out), np.load(GOLD)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(new[k], old[k]), k


def test_golden_is_consistent_with_its_cases():
    """T - 1 UNet evaluations on the first T - 1 entries of the ascending schedule, the CFG pair unless the scale is 0; the
    stack is (T, 1, C, L, L) with the clean input last; the inputs regenerated from their seeds are the golden's."""
    from lgd_amd import weights
    from invert_golden_cases import CASES, CHAIN_CASE, case_inputs, checksum, sample_index
    z = np.load(GOLD)
    idx = z["sample_index"]
    assert np.array_equal(idx, sample_index(4 * 32 * 32))
    assert os.path.getsize(GOLD) < 256 * 1024
    for case, cfg_name, n, scale, seed in CASES:
        cfg = weights.CONFIGS[cfg_name]
        s = DDIMInverseScheduler(prediction_type=cfg.prediction_type)
        s.set_timesteps(n)
        assert z[f"{case}/timesteps"].tolist() == s.timesteps.tolist()[:-1]
        assert set(z[f"{case}/unet_batch"].tolist()) == ({2} if scale > 0 else {1})
        assert z[f"{case}/stack_shape"].tolist() == [n, 1, cfg.in_channels, cfg.sample_size, cfg.sample_size]
        assert z[f"{case}/stack_sample"].shape == (n, idx.size)
        lat, text = case_inputs(cfg, seed)
        assert np.array_equal(checksum(lat), z[f"{case}/latents0_checksum"]), case
        assert np.array_equal(checksum(text), z[f"{case}/text_checksum"]), case
        assert np.array_equal(z[f"{case}/stack_sample"][-1], lat.reshape(-1).numpy()[idx])      # the clean row
        assert np.array_equal(z[f"{case}/stack_sample"][0], z[f"{case}/noisiest"].reshape(-1)[idx])
        sens = z[f"{case}/fp16_sensitivity"]                      # the reference against itself under fp16 storage
        assert sens.shape == (n,) and sens[-1] == 0.0 and np.all(sens[:-1] > 0) and np.all(np.diff(sens) < 0)
    d = DDIMScheduler()
    d.set_timesteps(10)
    assert z[f"{CHAIN_CASE}/chain_timesteps"].tolist() == d.timesteps.tolist()
    assert 0 < float(z[f"{CHAIN_CASE}/chain_fp16_sensitivity"]) < 1
