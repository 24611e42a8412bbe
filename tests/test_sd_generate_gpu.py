"""Plain Stable Diffusion (`sd`) on the MI355X: the fused PLMS step (lgd_cfg_plms_step_f32) against the fp64 host step, the
sampler under PNDM / DDIM against the golden of the reference's own loop (tools/make_golden_sd.py), graph vs eager,
batch vs single, five full-width SD1.5 PNDM steps against oracle/restate.py, and the drop-in plugin end to end."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "run_sd_generate_tiny.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import lgd_amd  # noqa: E402,F401
from lgd_amd import ops, weights  # noqa: E402
from lgd_amd.pipeline import sd_generate_batch  # noqa: E402
from lgd_amd.sampler import HipGraph, LMDSampler  # noqa: E402
from lgd_amd.scheduler import DDIMScheduler, PNDMScheduler  # noqa: E402
from lgd_amd.unet import UNetEngine  # noqa: E402
from conftest import gate  # noqa: E402
from pndm_restate import PNDMRestate  # noqa: E402
from sd_golden_cases import CASES, case_inputs  # noqa: E402

F32 = torch.float32
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


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_plms_kernel_matches_the_fp64_host_step(dev, B, pred):
    """51 evaluations (50 steps) of random CFG pairs through one captured hipGraph with x_out == x, plus the same run
    eagerly into a separate output buffer, against PNDMScheduler.step_host in fp64 on the same fp32 inputs."""
    C, L, n = 4, 64, 50
    sch = PNDMScheduler(prediction_type=pred)
    sch.set_timesteps(n)
    E = len(sch.timesteps)
    tab = sch.plms_table(7.5, dev)
    g = torch.Generator().manual_seed(100 * B + (1 if pred == "v_prediction" else 0))
    x0 = torch.randn((B, C, L, L), generator=g)
    eps_seq = [torch.randn((2 * B, C, L, L), generator=g) for _ in range(E)]
    # fp64 reference
    ref = [x0.double()]
    state = sch.host_state(ref[0])
    for k in range(E):
        e = eps_seq[k].double()
        m = e[:B] + 7.5 * (e[B:] - e[:B])
        ref.append(sch.step_host(m, k, ref[-1], state))
    dyn = torch.zeros(4, device=dev, dtype=torch.int32)
    eps = torch.zeros((2 * B, C, L, L), device=dev, dtype=F32)
    x = torch.zeros((B, C, L, L), device=dev, dtype=F32)
    ets = torch.zeros((3, B, C, L, L), device=dev, dtype=F32)
    cur = torch.zeros_like(x)
    hist = torch.zeros((E + 1, B, C, L, L), device=dev, dtype=F32)
    graph = HipGraph(lambda: ops.cfg_plms_step(eps, x, x, ets, cur, tab, dyn, hist=hist))
    x.copy_(x0)
    ets.fill_(float("nan"))                       # nothing the run has not written itself may be read
    cur.fill_(float("nan"))
    worst = 0.0
    for k in range(E):
        dyn[0] = k
        eps.copy_(eps_seq[k])
        graph()
        worst = max(worst, relerr(x, ref[k + 1]))
    torch.cuda.synchronize()
    # measured 3.6e-7 .. 8.0e-7 (fp32 rounding of the fp64 step) over B in {1, 3, 8} and both predictions
    gate(f"[plms kernel B={B} {pred}] graph, x_out == x: max rel err over {E} evaluations", worst, 2.4e-6)
    assert torch.equal(hist[E], x)
    # eager, separate output buffer (ping-pong)
    xa, xb = x0.to(dev).clone(), torch.empty((B, C, L, L), device=dev, dtype=F32)
    ets.fill_(float("nan"))
    cur.fill_(float("nan"))
    worst_e = 0.0
    for k in range(E):
        dyn[0] = k
        eps.copy_(eps_seq[k])
        ops.cfg_plms_step(eps, xa, xb, ets, cur, tab, dyn)
        xa, xb = xb, xa
        worst_e = max(worst_e, relerr(xa, ref[k + 1]))
    gate(f"[plms kernel B={B} {pred}] eager, x_out != x: max rel err", worst_e, 2.4e-6)
    assert torch.equal(xa, x)                     # aliasing and graph replay change nothing


def test_plms_kernel_rejects_unaligned_sizes(dev):
    sch = PNDMScheduler()
    sch.set_timesteps(5)
    tab = sch.plms_table(7.5, dev)
    dyn = torch.zeros(4, device=dev, dtype=torch.int32)
    x = torch.zeros((1, 1, 3, 3), device=dev)                    # 9 elements: not a whole number of 16-byte vectors
    with pytest.raises(RuntimeError):
        ops.cfg_plms_step(torch.zeros((2, 1, 3, 3), device=dev), x, x, torch.zeros((3, 1, 1, 3, 3), device=dev),
                          torch.zeros_like(x), tab, dyn)


# ---------------------------------------------------------------------------------------------------------------------
# limits: 3x the rel-L2 measured on the MI355X; per-evaluation trajectory max (on the golden's fixed
# sample of elements) and final latents (whole); measured: tiny_pndm 2.08e-3 / 2.20e-3, tiny_ddim 2.31e-3 / 2.31e-3,
# tiny_sd21_pndm 3.04e-3 / 2.99e-3
LIMITS = {"tiny_pndm": (6.2e-3, 6.6e-3), "tiny_ddim": (6.9e-3, 6.9e-3), "tiny_sd21_pndm": (9.0e-3, 9.0e-3)}


@pytest.mark.parametrize("case,cfg_name,kind,steps,seed", CASES)
def test_sampler_vs_golden_of_the_reference_loop(dev, case, cfg_name, kind, steps, seed):
    """Free-running: every evaluation's input sample and the final latents of pipelines.generate (the reference's
    loop, CPU fp32) under the restated PNDM / the stub DDIM, vs the HIP sampler (fp16 UNet, fused step)."""
    z = np.load(GOLD)
    cfg = weights.CONFIGS[cfg_name]
    sm = LMDSampler(engine(cfg_name, dev))
    sch = PNDMScheduler.from_config(sm.scheduler) if kind == "pndm" else DDIMScheduler(prediction_type=cfg.prediction_type)
    assert int(z[f"{case}/steps"]) == steps
    lat0, text = case_inputs(cfg, seed)
    lat, _, hist = sd_generate_batch(sm, [text], lat0, steps, guidance_scale=7.5, scheduler=sch, decode=False,
                                     save_all_latents=True)
    idx = torch.from_numpy(z["sample_index"]).long()
    inputs = torch.from_numpy(z[f"{case}/inputs_sample"])
    E = inputs.shape[0]
    assert hist[0].shape[0] == E + 1
    per = [rel_l2(hist[0][k, 0].reshape(-1).cpu()[idx], inputs[k]) for k in range(E)]
    print(f"[{case}] rel-L2 per evaluation: " + " ".join(f"{v:.2e}" for v in per))
    lim_traj, lim_final = LIMITS[case]
    gate(f"[{case}] max rel-L2 of the evaluation inputs (free-running)", max(per), lim_traj)
    gate(f"[{case}] final latents rel-L2", rel_l2(lat, torch.from_numpy(z[f"{case}/final"])), lim_final)


def test_graph_replay_equals_eager(dev):
    eng = engine("tiny", dev)
    lat0, text = case_inputs(weights.CONFIGS["tiny"], CASES[0][4])
    outs = []
    for graphs in (True, False):
        sm = LMDSampler(eng, use_graphs=graphs)
        outs.append(sd_generate_batch(sm, [text], lat0, 10, scheduler=PNDMScheduler(), decode=False, save_all_latents=True))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2][0], outs[1][2][0])


def test_batch_matches_single(dev):
    """Five prompts in one call padded to a bucket of 8: no image sees another (the same five in reverse order give the
    same latents bit for bit: same bucket, same tiles), and against one-at-a-time runs (bucket 1: other GEMM tiles, so
    fp16 rounding differs) PLMS stays within 3x of what the same comparison measures for the existing DDIM path."""
    eng = engine("tiny", dev)
    cfg = weights.CONFIGS["tiny"]
    sm = LMDSampler(eng)
    sm.max_pad = 0.5                                    # 5 -> one call padded to 8 (not 4 + 1)
    g = torch.Generator().manual_seed(9)
    lats = [torch.randn((1, 4, 32, 32), generator=g) for _ in range(5)]
    texts = []
    for i in range(5):
        unc, cond = weights.synth_embeddings(cfg, 1, seed=10 + i)
        texts.append(torch.cat([unc, cond]))
    worst = {}
    for name, sch in (("pndm", PNDMScheduler()), ("ddim", DDIMScheduler())):
        padded0 = sm.stats["padded_images"]
        batch, _ = sd_generate_batch(sm, texts, lats, 8, scheduler=sch, decode=False)
        assert sm.stats["padded_images"] - padded0 == 3
        rev, _ = sd_generate_batch(sm, texts[::-1], lats[::-1], 8, scheduler=sch, decode=False)
        e_rev = relerr(rev.flip(0), batch)
        print(f"[{name}] batch of 5 vs the same batch reversed: {e_rev:.3e}")
        assert e_rev < 1e-6
        errs = []
        for i in range(5):
            one, _ = sd_generate_batch(sm, [texts[i]], [lats[i]], 8, scheduler=sch, decode=False)
            errs.append(relerr(batch[i:i + 1], one))
        print(f"[{name}] batched (bucket 8) vs single (bucket 1): " + " ".join(f"{e:.3e}" for e in errs))
        worst[name] = max(errs)
    gate("[batch vs single] PLMS, worst image vs 3x the DDIM path's", worst["pndm"], 3 * max(worst["ddim"], 1e-7))


def test_pndm_refuses_guidance_and_partial_schedules(dev):
    from lgd_amd.sampler import Job
    eng = engine("tiny", dev)
    sm = LMDSampler(eng)
    cfg = weights.CONFIGS["tiny"]
    unc, cond = weights.synth_embeddings(cfg, 1, seed=1)
    job = Job(torch.zeros((1, 4, 32, 32)), torch.cat([unc, cond]))
    for kw in (dict(first_step=1), dict(fast_after_steps=2), dict(frozen_steps=2)):
        with pytest.raises(RuntimeError):
            sm.denoise_batch([job], 5, scheduler=PNDMScheduler(), **kw)
    guided = Job(job.latents, job.text, guidance=dict(bboxes=[[0.1, 0.1, 0.5, 0.5]], object_positions=[[1]]))
    with pytest.raises(RuntimeError):
        sm.denoise_batch([guided], 5, scheduler=PNDMScheduler())


# ---------------------------------------------------------------------------------------------------------------------
def test_sd15_full_width_five_pndm_steps_vs_oracle(dev):
    """SD1.5 topology with synthetic weights at 64x64 latents: 5 PNDM steps (6 UNet evaluations) of the HIP sampler vs
    oracle/restate.unet_forward (fp32, CPU) driven by tests/pndm_restate.py."""
    import restate as R
    cfg = weights.CONFIGS["sd15"]
    sd = weights.synth_state_dict(cfg, 0)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    g = torch.Generator().manual_seed(0)
    x = torch.randn((1, 4, 64, 64), generator=g)
    unc, cond = weights.synth_embeddings(cfg, 1, seed=1)
    ehs = torch.cat([unc, cond])
    cd = dict(block_out_channels=cfg.block_out_channels, layers_per_block=cfg.layers_per_block,
              attention_head_dim=cfg.attention_head_dim, norm_num_groups=cfg.norm_num_groups, norm_eps=cfg.norm_eps,
              gligen_positive_len=cfg.gligen_positive_len)
    ref = PNDMRestate(prediction_type=cfg.prediction_type)
    ref.set_timesteps(5)
    lat, hist_ref, eps_ref = x.clone(), [x.clone()], []
    with torch.no_grad():
        for t in ref.timesteps:
            e = R.unet_forward(sd, cd, torch.cat([lat] * 2), int(t), ehs)
            eps_ref.append(e)
            lat = ref.step(e[:1] + 7.5 * (e[1:] - e[:1]), t, lat).prev_sample
            hist_ref.append(lat.clone())
    eng = UNetEngine(cfg, dev, sd)
    sm = LMDSampler(eng)
    out, _, hist = sd_generate_batch(sm, [ehs], x, 5, decode=False, save_all_latents=True)
    # the first evaluation's noise prediction, on the same input (the engine's UNet vs the oracle's)
    eng.prepare_timesteps([int(ref.timesteps[0])])
    eng.prepare_text(ehs)
    eng.set_step(0)
    plan = eng.plan(2, 64)
    plan.latents_in.copy_(torch.cat([x] * 2).to(dev))
    plan.forward()
    torch.cuda.synchronize()
    # measured: noise prediction 1.93e-3; latents 1.89e-3 .. 2.41e-3 over the six evaluations
    gate("[sd15 PNDM] evaluation 0 noise prediction rel-L2", rel_l2(plan.eps_out, eps_ref[0]), 6e-3)
    for k in range(1, len(hist_ref)):
        gate(f"[sd15 PNDM] latents after evaluation {k - 1} (free-running) rel-L2", rel_l2(hist[0][k, 0], hist_ref[k]),
             7.2e-3)
    print(f"[sd15 PNDM] final latents rel-L2 {rel_l2(out, hist_ref[-1]):.3e}, relerr {relerr(out, hist_ref[-1]):.3e}")


# ---------------------------------------------------------------------------------------------------------------------
def test_sd_plugin_end_to_end_and_sdxl_refine(dev):
    """generation.stable_diffusion_generate.run on synthetic SD1.5 with the fake text side: a 512x512 RGB PIL image from
    start latents that are the torch.Generator("cuda") draw bit for bit; then the --sdxl post-pass on that PIL image."""
    sys.path.insert(0, os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    import models
    from fake_text import FakeTextEncoder, FakeTokenizer
    import generation.stable_diffusion_generate as g
    md = models.load_synthetic("sd15", device=dev)
    md.tokenizer, md.text_encoder = FakeTokenizer(), FakeTextEncoder(768)
    models.model_dict, models.sd_key, models.sd_version = md, "sd15", "sdv1.5"
    seen = {}
    orig = g.sd_generate_batch

    def spy(sampler, texts, latents, *a, **k):
        seen["latents"], seen["scheduler"] = latents.clone(), k.get("scheduler")
        return orig(sampler, texts, latents, *a, **k)
    g.sd_generate_batch = spy
    try:
        out = g.run("a cat", seed=7, extra_neg_prompt="x")
    finally:
        g.sd_generate_batch = orig
    want = torch.randn((1, 4, 64, 64), generator=torch.Generator("cuda").manual_seed(7), device="cuda", dtype=F32)
    assert torch.equal(seen["latents"], want)
    assert isinstance(seen["scheduler"], PNDMScheduler)
    assert out.image.size == (512, 512) and out.image.mode == "RGB"
    arr = np.asarray(out.image)
    assert arr.std() > 0
    import generation.sdxl_refinement as r
    r.init_synthetic(device=dev)
    rc = weights.CONFIGS["sdxl_refiner"]
    gen = torch.Generator().manual_seed(1)
    spec = dict(prompt="a cat", extra_neg_prompt="x",
                sdxl_prompt_embeds=torch.randn((2, 77, rc.cross_attention_dim), generator=gen),
                sdxl_pooled=torch.randn((2, rc.pooled_dim), generator=gen))
    ref_img = r.refine(out.image, spec, refine_seed=5, refinement_step_ratio=0.1)
    assert ref_img.size == (1024, 1024)
    assert np.array_equal(np.asarray(ref_img), np.asarray(r.refine(arr, spec, refine_seed=5, refinement_step_ratio=0.1)))


def test_dropin_generate_with_every_scheduler(dev):
    """models.pipelines.generate (pipelines.py:250-279): DDIM and DPM-Solver++ (existing kernels) and PNDM (the PLMS
    kernel) read from model_dict[scheduler_key]; no_set_timesteps runs the schedule as set."""
    sys.path.insert(0, os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    import models
    from models import pipelines
    from lgd_amd.scheduler import DPMSolverMultistepScheduler
    cfg = weights.CONFIGS["tiny"]
    md = models.build_model_dict(cfg, weights.synth_state_dict(cfg, 0))
    md["pndm"] = PNDMScheduler.from_config(md.scheduler)
    md["dpm"] = DPMSolverMultistepScheduler()
    unc, cond = weights.synth_embeddings(cfg, 2, seed=1)
    unc = unc.expand(2, -1, -1)
    emb = (torch.cat([unc, cond]).to(dev), unc.to(dev), cond.to(dev))
    lat = torch.randn((2, 4, 32, 32), generator=torch.Generator().manual_seed(4)).to(dev)
    for key in ("scheduler", "dpm", "pndm"):
        out, images = pipelines.generate(md, lat, emb, 6, scheduler_key=key)
        assert out.shape == lat.shape and images is None and torch.isfinite(out).all()
        one, _ = pipelines.generate(md, lat[1:], (torch.stack([emb[0][1], emb[0][3]]), None, None), 6, scheduler_key=key)
        assert relerr(out[1:], one) < 1e-3, key          # bucket 2 vs bucket 1: GEMM tiles may differ
    md.pndm.set_timesteps(6)
    again, _ = pipelines.generate(md, lat, emb, 999, scheduler_key="pndm", no_set_timesteps=True)
    assert torch.equal(again, pipelines.generate(md, lat, emb, 6, scheduler_key="pndm")[0])
