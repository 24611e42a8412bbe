"""DDIM inversion on the MI355X: the fused DDIM step kernel on inverse rows against the fp64 host step, the two encode
kernels (lgd_image_u8_to_nhwc8_f16, lgd_vae_sample_f32), pipelines.encode against oracle/restate_sdxl.py's encoder,
invert against the golden of the reference's own loop (tools/make_golden_invert.py), its invariants, the
invert -> generate_partial_frozen chain and the drop-in surface."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "run_invert_tiny.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import lgd_amd  # noqa: E402,F401
from lgd_amd import ops, vae, weights  # noqa: E402
from lgd_amd.pipeline import invert_batch  # noqa: E402
from lgd_amd.sampler import HipGraph, Job, LMDSampler  # noqa: E402
from lgd_amd.scheduler import DDIMInverseScheduler, DDIMScheduler  # noqa: E402
from lgd_amd.unet import UNetEngine  # noqa: E402
from conftest import gate  # noqa: E402
from ddim_inverse_restate import DDIMInverseRestate  # noqa: E402
from invert_golden_cases import (CASES, CHAIN_CASE, CHAIN_FROZEN_STEPS, CHAIN_GUIDANCE, case_inputs,  # noqa: E402
                                 chain_mask)

F32, D = torch.float32, torch.float64
_ENG = {}


def engine(name, dev):
    if name not in _ENG:
        cfg = weights.CONFIGS[name]
        _ENG[name] = UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0))
    return _ENG[name]


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def dropin_models():
    sys.path.insert(0, os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    import models
    return models


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("B", [1, 3])
def test_ddim_kernel_runs_inverse_rows(dev, B, pred):
    """The 9 steps of a 10-step inverse schedule on random CFG pairs: one captured hipGraph with x_out == x, and the same
    run eagerly into a separate output buffer, against the restated scheduler's step in fp64 on the same fp32 inputs."""
    C, L, n = 4, 8, 10
    sch = DDIMInverseScheduler(prediction_type=pred)
    sch.set_timesteps(n)
    ref_s = DDIMInverseRestate(prediction_type=pred, dtype=D)
    ref_s.set_timesteps(n)
    S = n - 1
    tab = sch.coef_table(7.5, dev)
    g = torch.Generator().manual_seed(200 * B + (1 if pred == "v_prediction" else 0))
    x0 = torch.randn((B, C, L, L), generator=g)
    eps_seq = [torch.randn((2 * B, C, L, L), generator=g) for _ in range(S)]
    ref = [x0.double()]
    for k in range(S):
        e = eps_seq[k].double()
        ref.append(ref_s.step(e[:B] + 7.5 * (e[B:] - e[:B]), ref_s.timesteps[k], ref[-1]).prev_sample)
    dyn = torch.zeros(4, device=dev, dtype=torch.int32)
    eps = torch.zeros((2 * B, C, L, L), device=dev, dtype=F32)
    x = torch.zeros((B, C, L, L), device=dev, dtype=F32)
    hist = torch.full((n + 1, B, C, L, L), float("nan"), device=dev, dtype=F32)
    graph = HipGraph(lambda: ops.cfg_ddim_step(eps, x, x, tab, dyn, hist=hist))
    hist.fill_(float("nan"))                      # the capture's warm-up launch wrote row 1
    x.copy_(x0)
    worst = 0.0
    for k in range(S):
        dyn[0] = k
        eps.copy_(eps_seq[k])
        graph()
        worst = max(worst, relerr(x, ref[k + 1]))
        assert torch.equal(hist[k + 1], x)
    torch.cuda.synchronize()
    assert torch.isnan(hist[0]).all() and torch.isnan(hist[n]).all()          # rows the run does not own stay untouched
    # measured on the MI355X: 2.19e-7 .. 3.05e-7 over B in {1, 3} and both predictions (fp32 rounding of the fp64 step)
    gate(f"[ddim kernel, inverse rows B={B} {pred}] graph, x_out == x: max rel err over {S} steps", worst, LIMIT_STEP)
    xa, xb = x0.to(dev).clone(), torch.empty((B, C, L, L), device=dev, dtype=F32)
    worst_e = 0.0
    for k in range(S):
        dyn[0] = k
        eps.copy_(eps_seq[k])
        ops.cfg_ddim_step(eps, xa, xb, tab, dyn)
        xa, xb = xb, xa
        worst_e = max(worst_e, relerr(xa, ref[k + 1]))
    gate(f"[ddim kernel, inverse rows B={B} {pred}] eager, x_out != x: max rel err", worst_e, LIMIT_STEP)
    assert torch.equal(xa, x)                     # aliasing and graph replay change nothing


LIMIT_STEP = 9.2e-7


# ---------------------------------------------------------------------------------------------------------------------
def _split_reference(u8):
    """uint8 (B,H,W,3) on the CPU -> the [B*H*W, 8] fp16 operand: torch fp32 2 * (u / 255) - 1 (true division: CPU), split
    into the fp16 value and the fp16 of its rounding remainder."""
    x = 2.0 * (u8.to(F32) / 255.0) - 1.0
    hi = x.half()
    lo = (x - hi.float()).half()
    out = torch.zeros(u8.shape[:3] + (8,), dtype=torch.float16)
    out[..., 0:3], out[..., 3:6] = hi, lo
    return out.reshape(-1, 8)


def test_image_u8_kernel_is_bit_exact(dev):
    perm = torch.randperm(768, generator=torch.Generator().manual_seed(3))
    every = (torch.arange(768) % 256).to(torch.uint8)[perm].reshape(1, 16, 16, 3)       # all 256 byte values, 3 times
    assert len(set(every.flatten().tolist())) == 256
    pair = torch.randint(0, 256, (2, 8, 8, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    for img in (every, pair):
        got = ops.image_u8_to_nhwc8(img.to(dev))
        want = _split_reference(img)
        assert got.shape == want.shape and got.dtype == torch.float16
        assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    # the same bits as the float path the other callers use (lgd_nchw_to_nhwc8_f16 on the fp32 image)
    x = (2.0 * (every.to(F32) / 255.0) - 1.0).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(ops.nchw_to_nhwc8(x.to(dev)), ops.image_u8_to_nhwc8(every.to(dev)))
    with pytest.raises(RuntimeError):
        ops.image_u8_to_nhwc8(torch.zeros((1, 3, 3, 3), dtype=torch.uint8, device=dev))   # 9 pixels: not whole words


@pytest.mark.parametrize("B,z,H", [(1, 4, 6), (2, 4, 8)])
def test_vae_sample_kernel_vs_fp64(dev, B, z, H):
    g = torch.Generator().manual_seed(10 * B + H)
    mom = torch.randn((B * H * H, 2 * z), generator=g)
    mom[:, z:] *= 3.0
    mom[1, z] = -40.0                              # both clamps act
    mom[2, z + 1] = 25.0
    mom[B * H * H - 1, 2 * z - 1] = 25.0
    mom = mom.half()
    noise = torch.randn((B, z, H, H), generator=g)
    got = ops.vae_sample(mom.to(dev), noise.to(dev), 0.18215)
    m = mom.double().view(B, H, H, 2 * z).permute(0, 3, 1, 2)
    mean, std = m[:, :z], torch.exp(0.5 * m[:, z:].clamp(-30.0, 20.0))
    want = 0.18215 * (mean + std * noise.double())
    assert got.shape == noise.shape and got.dtype == F32
    assert float(std.max()) == pytest.approx(np.exp(10.0)) and float(std.min()) == pytest.approx(np.exp(-15.0))
    # per element, relative to the magnitude of its two terms (a sum of two roundings, an exp and two products in fp32)
    err = ((got.double().cpu() - want).abs() / (0.18215 * (mean.abs() + std * noise.double().abs()))).max()
    # measured on the MI355X: 1.22e-7 (B=1, H=6), 1.37e-7 (B=2, H=8): an fp32 exp, two products, a sum and the scale
    gate(f"[vae sample B={B} z={z} H={H}] max element error relative to its terms", float(err), LIMIT_SAMPLE)
    with pytest.raises(RuntimeError):
        ops.vae_sample(torch.zeros((9, 8), device=dev, dtype=torch.float16), torch.zeros((1, 4, 3, 3), device=dev), 1.0)


LIMIT_SAMPLE = 4.1e-7


# ---------------------------------------------------------------------------------------------------------------------
def test_encode_vs_oracle_and_input_forms(dev):
    """pipelines.encode on a seeded AutoencoderKL state dict at small width, 64 x 64 image: against the fp32 restatement's
    moments with the same noise (drawn from the caller's CPU generator); uint8 array, PIL image and float tensor agree."""
    import restate_sdxl as X
    from PIL import Image
    models = dropin_models()
    from models import pipelines
    sd = vae.synth_aekl_state_dict(ch=(32, 32, 64, 64), layers=1)
    md = models.models._EasyDict(vae=vae.HipVAE(sd, dev), dtype=F32)
    assert md.vae.config.scaling_factor == 0.18215 and md.vae._encoder is None         # built on first use
    arr = np.random.default_rng(5).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    x = (2.0 * (torch.from_numpy(arr).to(F32) / 255.0) - 1.0).permute(2, 0, 1)[None].contiguous()
    gen = lambda: torch.Generator().manual_seed(11)                                    # noqa: E731
    lat = pipelines.encode(md, arr, gen())
    assert lat.shape == (1, 4, 8, 8) and lat.dtype == F32 and lat.device.type == "cuda"
    with torch.no_grad():
        mean, logvar = X.vae_encode_moments(sd, x)
    noise = torch.randn(mean.shape, generator=gen())
    want = 0.18215 * (mean + torch.exp(0.5 * logvar) * noise)
    # measured on the MI355X: 3.25e-4
    gate("[encode] scaled latents vs the fp32 restatement, rel-L2", rel_l2(lat, want), LIMIT_ENCODE)
    assert torch.equal(lat, pipelines.encode(md, Image.fromarray(arr), gen()))
    assert torch.equal(lat, pipelines.encode(md, x, gen()))
    assert not torch.equal(lat, pipelines.encode(md, arr, torch.Generator().manual_seed(12)))
    with pytest.raises(AssertionError):
        pipelines.encode(md, arr.astype(np.float32), gen())
    with pytest.raises(RuntimeError):
        pipelines.encode(md, arr[:, :32], gen())                                       # square images only


LIMIT_ENCODE = 9.7e-4


# ---------------------------------------------------------------------------------------------------------------------
# Limits of the free-running comparisons come from the reference itself: inversion under classifier-free guidance is
# expansive (at scale 7.5 a deviation of this network's trajectory doubles per step), so the golden also holds, per row, how
# far the reference's own loop moves when its UNet stores weights and layer outputs in fp16 (`fp16_sensitivity`,
# tools/make_golden_invert.py).  Every row must stay within SENSITIVITY_FACTOR of that.  Measured on the MI355X, rel-L2 per
# row, noisiest first, next to the golden's fp16 sensitivity of the same row:
#   tiny_g7.5     4.95e-1 2.35e-1 1.15e-1 5.33e-2 2.91e-2 1.44e-2 7.61e-3 4.40e-3 2.67e-3
#     reference   4.56e-1 2.25e-1 1.05e-1 4.86e-2 2.45e-2 1.33e-2 7.53e-3 4.37e-3 2.35e-3     (worst ratio 1.19)
#   tiny_g0       5.43e-3 3.32e-3 2.09e-3 1.43e-3 1.03e-3 7.60e-4 5.77e-4 4.42e-4 3.19e-4
#     reference   5.91e-3 3.34e-3 2.14e-3 1.47e-3 1.07e-3 8.11e-4 5.99e-4 4.33e-4 2.88e-4     (worst ratio 1.11)
#   tiny_sd21_g1  6.16e-3 3.54e-3 2.38e-3 1.61e-3 1.12e-3 8.58e-4 6.10e-4 4.44e-4 3.15e-4
#     reference   6.81e-3 3.88e-3 2.33e-3 1.59e-3 1.12e-3 8.38e-4 6.24e-4 4.56e-4 3.08e-4     (worst ratio 1.02)
# noisiest row, whole: 4.98e-1 (tiny_g7.5), 5.59e-3, 6.67e-3.
SENSITIVITY_FACTOR = 3.0


@pytest.mark.parametrize("case,cfg_name,steps,scale,seed", CASES)
def test_invert_vs_golden_of_the_reference_loop(dev, case, cfg_name, steps, scale, seed):
    """Free-running: every row of the stack pipelines.invert returns (the reference's loop, CPU fp32, under the restated
    inverse scheduler) vs invert_batch on the HIP sampler (fp16 UNet, fused step)."""
    z = np.load(GOLD)
    cfg = weights.CONFIGS[cfg_name]
    sm = LMDSampler(engine(cfg_name, dev))
    lat0, text = case_inputs(cfg, seed)
    out = invert_batch(sm, [text], lat0, steps, guidance_scale=scale)
    assert list(out.shape) == z[f"{case}/stack_shape"].tolist() == [steps, 1, cfg.in_channels, 32, 32]
    assert out.dtype == F32
    assert torch.equal(out[steps - 1].cpu(), lat0)                   # the clean input, last
    idx = torch.from_numpy(z["sample_index"]).long()
    want = torch.from_numpy(z[f"{case}/stack_sample"])
    per = [rel_l2(out[k, 0].reshape(-1).cpu()[idx], want[k]) for k in range(steps)]
    print(f"[{case}] rel-L2 per row, noisiest first: " + " ".join(f"{v:.2e}" for v in per))
    assert per[steps - 1] == 0.0
    assert per.index(max(per)) < steps - 1
    sens = z[f"{case}/fp16_sensitivity"]
    print(f"[{case}] the reference's own fp16 sensitivity:  " + " ".join(f"{v:.2e}" for v in sens))
    gate(f"[{case}] worst row, rel-L2 over the reference's own fp16 sensitivity of that row (free-running)",
         max(per[k] / sens[k] for k in range(steps - 1)), SENSITIVITY_FACTOR)
    gate(f"[{case}] noisiest row (whole) rel-L2", rel_l2(out[0], torch.from_numpy(z[f"{case}/noisiest"])),
         SENSITIVITY_FACTOR * float(sens[0]))
    # noise grows up the stack: the order is noisiest first
    assert rel_l2(out[0], lat0) > rel_l2(out[steps - 2], lat0) > 0


def _g0_case():
    case, cfg_name, steps, scale, seed = CASES[1]
    assert scale == 0.0
    cfg = weights.CONFIGS[cfg_name]
    return cfg, steps, case_inputs(cfg, seed)


def test_scale_zero_ignores_the_cond_embeddings(dev):
    cfg, steps, (lat0, text) = _g0_case()
    sm = LMDSampler(engine("tiny", dev))
    a = invert_batch(sm, [text], lat0, steps, guidance_scale=0.0)
    other = text.clone()
    other[1] = torch.randn(text[1].shape, generator=torch.Generator().manual_seed(77))
    b = invert_batch(sm, [other], lat0, steps, guidance_scale=0.0)
    assert torch.equal(a, b)
    assert not torch.equal(a, invert_batch(sm, [other], lat0, steps, guidance_scale=1.0))


def test_batch_of_two_equals_two_single_runs(dev):
    cfg, steps, (lat0, text) = _g0_case()
    sm = LMDSampler(engine("tiny", dev))
    lat1 = 0.8 * torch.randn(lat0.shape, generator=torch.Generator().manual_seed(78))
    unc, cond = weights.synth_embeddings(cfg, 1, seed=5)
    text1 = torch.cat([unc, cond])
    both = invert_batch(sm, [text, text1], torch.cat([lat0, lat1]), steps, guidance_scale=0.0)
    assert both.shape == (steps, 2, cfg.in_channels, 32, 32)
    one0 = invert_batch(sm, [text], lat0, steps, guidance_scale=0.0)
    one1 = invert_batch(sm, [text1], [lat1], steps, guidance_scale=0.0)
    print(f"[batch of two vs single] rel err image 0 {relerr(both[:, 0:1], one0):.3e}, image 1 {relerr(both[:, 1:2], one1):.3e}")
    assert torch.equal(both[:, 0:1], one0) and torch.equal(both[:, 1:2], one1)


def test_graph_replay_equals_eager(dev):
    cfg, steps, (lat0, text) = _g0_case()
    eng = engine("tiny", dev)
    outs = [invert_batch(LMDSampler(eng, use_graphs=graphs), [text], lat0, steps, guidance_scale=0.0)
            for graphs in (True, False)]
    assert torch.equal(outs[0], outs[1])


def test_history_rows_are_this_calls_own(dev):
    """A longer run on the same state leaves rows behind; a shorter inversion must not return them."""
    cfg, steps, (lat0, text) = _g0_case()
    sm = LMDSampler(engine("tiny", dev))
    invert_batch(sm, [text], 3.0 * lat0, 20, guidance_scale=0.0)
    fresh = invert_batch(LMDSampler(engine("tiny", dev)), [text], lat0, steps, guidance_scale=0.0)
    again = invert_batch(sm, [text], lat0, steps, guidance_scale=0.0)
    assert again.shape[0] == steps and torch.equal(again, fresh)


def test_inverse_scheduler_is_refused_outside_the_plain_loop(dev):
    cfg, steps, (lat0, text) = _g0_case()
    sm = LMDSampler(engine("tiny", dev))
    job = Job(lat0, text)
    inv = DDIMInverseScheduler()
    for kw in (dict(first_step=1), dict(fast_after_steps=2), dict(frozen_steps=2)):
        with pytest.raises(RuntimeError):
            sm.denoise_batch([job], 5, scheduler=inv, **kw)
    guided = Job(lat0, text, guidance=dict(bboxes=[[0.1, 0.1, 0.5, 0.5]], object_positions=[[1]]))
    with pytest.raises(RuntimeError):
        sm.denoise_batch([guided], 5, scheduler=inv)
    with pytest.raises(TypeError):
        invert_batch(sm, [text], lat0, 5, inverse_scheduler=DDIMScheduler())


def test_invert_inside_lanes(dev):
    """invert_batch on the lanes of a lanes.LanePool equals the same jobs on one lane bit for bit."""
    from lgd_amd.lanes import LanePool, make_lanes
    cfg, steps, (lat0, text) = _g0_case()
    lanes = make_lanes(engine("tiny", dev), 2, lambda e: LMDSampler(e))
    jobs = [(lat0 * s, sc) for s, sc in ((1.0, 7.5), (0.5, 0.0), (1.5, 1.0), (0.7, 7.5))]
    run = lambda lane, j: invert_batch(lane.sampler, [text], j[0], 6, guidance_scale=j[1])        # noqa: E731
    with LanePool(lanes, device=dev) as pool:
        two = pool.map(run, jobs)
    with LanePool(lanes[:1], device=dev) as pool:
        one = pool.map(run, jobs)
    for a, b in zip(two, one):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
def _tiny_dropin(dev):
    models = dropin_models()
    cfg = weights.CONFIGS["tiny"]
    md = models.build_model_dict(cfg, weights.synth_state_dict(cfg, 0), device=dev, load_inverse_scheduler=True)
    return models, cfg, md


def test_chain_invert_then_partial_frozen_vs_golden(dev):
    """The drop-in chain invert -> generate_partial_frozen (box mask, frozen_steps 4, 10 steps) against the reference's
    own two calls; inside the mask the blend takes the inverted rows."""
    z = np.load(GOLD)
    models, cfg, md = _tiny_dropin(dev)
    from models import pipelines
    case, cfg_name, steps, scale, seed = CASES[1]
    assert case == CHAIN_CASE
    lat0, text = case_inputs(cfg, seed)
    emb = (text.to(dev), text[0:1].to(dev), text[1:2].to(dev))
    stack = pipelines.invert(md, lat0.to(dev), emb, steps, guidance_scale=scale)
    assert stack.device.type == "cpu" and stack.shape == (steps, 1, cfg.in_channels, 32, 32)
    mask = chain_mask(32)
    lat, images = pipelines.generate_partial_frozen(md, stack, mask, emb, steps, CHAIN_FROZEN_STEPS,
                                                    guidance_scale=CHAIN_GUIDANCE)
    assert images is None
    # two free-running loops back to back: the limit is SENSITIVITY_FACTOR x what the reference's own chain moves under fp16
    # storage (6.35e-2: the guided generation amplifies the 5e-3 of the inverted stack); measured on the MI355X: 6.52e-2
    gate("[chain] final latents of invert -> generate_partial_frozen, rel-L2",
         rel_l2(lat, torch.from_numpy(z[f"{case}/chain_final"])),
         SENSITIVITY_FACTOR * float(z[f"{case}/chain_fp16_sensitivity"]))
    r = md.sampler.denoise(stack, text, steps, guidance_scale=CHAIN_GUIDANCE, frozen_steps=CHAIN_FROZEN_STEPS,
                           frozen_mask=mask, save_all_latents=True)
    assert torch.equal(r["latents"], lat)
    hist, inside = r["latents_all"].cpu(), mask.bool().expand(1, cfg.in_channels, 32, 32)
    for k in range(steps):
        same = torch.equal(hist[k + 1][inside], stack[k + 1][inside]) if k + 1 < steps else False
        assert same == (k < CHAIN_FROZEN_STEPS), k
        assert not torch.equal(hist[k + 1][~inside], stack[min(k + 1, steps - 1)][~inside])


def test_dropin_surface_and_the_reference_call_sequence(dev):
    """load_synthetic(..., load_inverse_scheduler=True) -> encode -> invert -> generate_partial_frozen, as a caller written
    for the reference strings them together; without the flag the dict has the keys it always had."""
    models = dropin_models()
    from models import pipelines
    plain = models.load_synthetic("tiny", device=dev, with_vae=False)
    assert sorted(plain.keys()) == ["dtype", "sampler", "scheduler", "text_encoder", "tokenizer", "unet", "vae"]
    md = models.load_synthetic("tiny", device=dev, load_inverse_scheduler=True)
    assert sorted(md.keys()) == sorted([*plain.keys(), "inverse_scheduler"])
    assert isinstance(md.inverse_scheduler, DDIMInverseScheduler) and isinstance(md.vae, vae.HipVAEDecoder)
    assert md.inverse_scheduler.config.prediction_type == md.scheduler.config.prediction_type
    cfg = weights.CONFIGS["tiny"]
    image = np.random.default_rng(1).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    latents = pipelines.encode(md, image, torch.Generator(device="cuda").manual_seed(3))
    assert latents.shape == (1, 4, 32, 32) and torch.isfinite(latents).all()
    unc, cond = weights.synth_embeddings(cfg, 1, seed=1)
    emb = (torch.cat([unc, cond]).to(dev), unc.to(dev), cond.to(dev))
    T = 4
    stack = pipelines.invert(md, latents, emb, T, guidance_scale=1.0)
    assert stack.shape == (T, 1, 4, 32, 32) and torch.equal(stack[T - 1], latents.cpu())
    ts, n = pipelines.get_inverse_timesteps(md.inverse_scheduler, T, strength=1.0)
    assert n == T and ts.tolist() == [1, 251, 501, 751]
    lat, images = pipelines.generate_partial_frozen(md, stack, chain_mask(32), emb, T, 2, guidance_scale=7.5)
    assert lat.shape == (1, 4, 32, 32) and torch.isfinite(lat).all()
    assert images.shape == (1, 256, 256, 3) and images.dtype == np.uint8
