"""The sigma-space samplers (EulerDiscreteScheduler, LMSDiscreteScheduler) on the MI355X: the fused LMS step
(lgd_cfg_lms_step_f32) against the fp64 host step, its refusals, the sampler under both against the golden of the
reference's own loops (tools/make_golden_sigma.py), graph vs eager, batch vs single, the drop-in under
load_synthetic(scheduler_cls=...), and two guided Euler steps at full width against oracle/restate.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "run_sigma_tiny.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import lgd_amd  # noqa: E402,F401
from lgd_amd import ops, weights  # noqa: E402
from lgd_amd.pipeline import sd_generate_batch  # noqa: E402
from lgd_amd.sampler import HipGraph, LMDSampler  # noqa: E402
from lgd_amd.scheduler import DDIMScheduler, EulerDiscreteScheduler, LMSDiscreteScheduler  # noqa: E402
from lgd_amd.unet import UNetEngine  # noqa: E402
from conftest import gate  # noqa: E402
from sigma_golden_cases import BBOXES, CASES, GUIDANCE, MAX_INDEX_STEP, MAX_ITER, OBJ_POS, SG_KWARGS, case_inputs, scheduler_config  # noqa: E402
from sigma_sched_restate import EulerRestate  # noqa: E402

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


def make_scheduler(kind, prediction="epsilon"):
    cls = EulerDiscreteScheduler if kind == "euler" else LMSDiscreteScheduler
    return cls.from_config(scheduler_config(prediction))


def guidance_dict():
    return dict(SG_KWARGS, bboxes=BBOXES, object_positions=OBJ_POS)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
N_STEPS = 10                                      # the order ramp 1 -> 4, the ring wrapping twice, the final sigma' = 0 step
# (B, C, L): 4 vectors, under one wave; a partial block; many blocks
SHAPES = [(1, 4, 2), (3, 4, 6), (2, 4, 64)]
# measured on the MI355X: 1.9e-7 .. 4.15e-7 (fp32 rounding of the fp64 step and of the table) over the three shapes, both
# prediction types and both cases, next to the PLMS kernel's 3.6e-7 .. 8.0e-7; the limit is 3x the largest
LIMIT_KERNEL = 1.25e-6


def _kernel_case(dev, shape, pred, blend):
    B, C, L = shape
    sch = make_scheduler("lms", pred)
    sch.set_timesteps(N_STEPS)
    tab = sch.lms_table(GUIDANCE, dev)
    g = torch.Generator().manual_seed(1000 * B + 10 * L + (1 if pred == "v_prediction" else 0) + (2 if blend else 0))
    x0 = torch.randn((B, C, L, L), generator=g) * sch.init_noise_sigma
    eps_seq = [torch.randn((2 * B, C, L, L), generator=g) for _ in range(N_STEPS)]
    frozen = torch.randn((N_STEPS + 1, B, C, L, L), generator=g) if blend else None
    mask = torch.rand((B, L * L), generator=g) if blend else None
    frozen_steps = 3 if blend else 0
    ref = [x0.double()]
    state = sch.host_state(ref[0])
    for r in state["ring"]:
        r.fill_(float("nan"))
    for k in range(N_STEPS):
        e = eps_seq[k].double()
        xn = sch.step_host(e[:B] + GUIDANCE * (e[B:] - e[:B]), k, ref[-1], state)
        if k < frozen_steps:
            mk = mask.double().reshape(B, 1, L, L)
            xn = frozen[k + 1].double() * mk + xn * (1 - mk)
        ref.append(xn)
    dyn = torch.zeros(4, device=dev, dtype=torch.int32)
    dyn[1] = frozen_steps
    eps = torch.zeros((2 * B, C, L, L), device=dev, dtype=F32)
    x = torch.zeros((B, C, L, L), device=dev, dtype=F32)
    ring = torch.zeros((4, B, C, L, L), device=dev, dtype=F32)
    hist = torch.zeros((N_STEPS + 1, B, C, L, L), device=dev, dtype=F32) if blend else None
    kw = dict(frozen_ref=frozen.to(dev), mask=mask.to(dev), hist=hist) if blend else {}
    graph = HipGraph(lambda: ops.cfg_lms_step(eps, x, x, ring, tab, dyn, **kw))
    x.copy_(x0)
    ring.fill_(float("nan"))                      # nothing the run has not written itself may be read
    worst = 0.0
    for k in range(N_STEPS):
        dyn[0] = k
        eps.copy_(eps_seq[k])
        graph()
        worst = max(worst, relerr(x, ref[k + 1]))
        if blend:
            assert torch.equal(hist[k + 1], x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all())
    # eager, separate output buffer (ping-pong)
    xa, xb = x0.to(dev).clone(), torch.empty((B, C, L, L), device=dev, dtype=F32)
    ring.fill_(float("nan"))
    for k in range(N_STEPS):
        dyn[0] = k
        eps.copy_(eps_seq[k])
        ops.cfg_lms_step(eps, xa, xb, ring, tab, dyn, **kw)
        xa, xb = xb, xa
    assert torch.equal(xa, x)                     # aliasing and graph replay change nothing
    return worst


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("shape", SHAPES)
def test_lms_kernel_matches_the_fp64_host_step(dev, shape, pred):
    """10 steps of random CFG pairs through one captured hipGraph with x_out == x, and the same run eagerly into a second
    buffer (bit-identical), against LMSDiscreteScheduler.step_host in fp64 on the same fp32 inputs; the ring starts as NaN."""
    gate(f"[lms kernel {shape} {pred}] max rel err over {N_STEPS} steps", _kernel_case(dev, shape, pred, False), LIMIT_KERNEL)


@pytest.mark.parametrize("shape", SHAPES)
def test_lms_kernel_blend_and_history(dev, shape):
    """frozen_ref / mask / hist on, dyn[1] = 3: the first three steps blend, every step writes its history row."""
    gate(f"[lms kernel {shape} blend] max rel err over {N_STEPS} steps", _kernel_case(dev, shape, "epsilon", True), LIMIT_KERNEL)


def test_lms_kernel_refusals(dev):
    """Each refused on the host, before any launch: the outputs keep their sentinel."""
    sch = make_scheduler("lms")
    sch.set_timesteps(5)
    tab = sch.lms_table(GUIDANCE, dev)
    dyn = torch.zeros(4, device=dev, dtype=torch.int32)

    def bufs(B, C, L):
        return (torch.zeros((2 * B, C, L, L), device=dev), torch.full((B, C, L, L), 7.0, device=dev),
                torch.full((4, B, C, L, L), 7.0, device=dev))
    eps, x, ring = bufs(1, 1, 3)                                 # 9 elements: no whole number of 16-byte vectors
    with pytest.raises(RuntimeError):
        ops.cfg_lms_step(eps, x, x, ring, tab, dyn)
    eps, x, ring = bufs(1, 4, 4)
    with pytest.raises(RuntimeError):                            # frozen_ref without mask
        ops.cfg_lms_step(eps, x, x, ring, tab, dyn, frozen_ref=torch.zeros((6, 1, 4, 4, 4), device=dev))
    big = torch.full((5, 1, 4, 4, 4), 7.0, device=dev)
    with pytest.raises(RuntimeError):                            # the ring's last slot is x
        ops.cfg_lms_step(eps, big[3], big[4], big[:4], tab, dyn)
    with pytest.raises(RuntimeError):                            # x_out inside the ring
        ops.cfg_lms_step(eps, x, big[1], big[:4], tab, dyn)
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()) and bool((ring == 7.0).all()) and bool((big == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# the sampler against the golden of the reference's loops.  Limits: 3x the rel-L2 measured on the MI355X, next
# to the DDIM figure of the same tiny loops (tests/test_sd_generate_gpu.py: tiny_ddim 2.31e-3 free-running over 50 steps).
#   plain Euler (tiny_sd21, v), free-running, 6 steps:  UNet inputs 3.1e-8 9.99e-4 2.32e-3 3.97e-3 6.32e-3 1.138e-2, final
#     1.185e-2 (six steps from sigma 14.6 to 0: under v_prediction x0 is nearly -m at large sigma, so the fp16 UNet's error goes
#     straight into the latents, and the final step returns x0)
#   guided Euler, teacher-forced, per step:             5.82e-3 3.43e-4 1.09e-4 5.49e-5 4.90e-5 2.62e-6 (2, 1, 0 ... iterations)
#   guided LMS, free-running:                           after each step 6.05e-3 5.94e-3 5.96e-3 5.97e-3 5.97e-3 5.97e-3, final
#     5.78e-3 — behind two guided steps, which amplify perturbations on the tiny net
#     (tests/test_oracle.py::test_guided_step_amplifies_input_perturbations)
#   guidance losses, worst relative difference:         Euler 1.44e-4, LMS 1.44e-4 (iteration counts equal)
LIMIT_PLAIN = (3.4e-2, 3.55e-2)
LIMIT_EULER_TF = [1.75e-2, 1.03e-3, 3.3e-4, 1.65e-4, 1.47e-4, 7.9e-6]
LIMIT_LMS = (1.8e-2, 1.73e-2)
LIMIT_LOSS = dict(euler=4.3e-4, lms=4.3e-4)


def _case(name):
    z = np.load(GOLD)
    row = next(c for c in CASES if c[0] == name)
    _, cfg_name, kind, pred, steps, seed, guided, whole = row
    cfg = weights.CONFIGS[cfg_name]
    noise, text = case_inputs(cfg, seed)
    sch = make_scheduler(kind, pred)
    # the fp32 cumulative product of the alphas may differ in its last bit from host to host: a few fp32 ulps
    assert abs(sch.init_noise_sigma / float(z[f"{name}/init_noise_sigma"]) - 1) < 1e-6
    sch.set_timesteps(steps)
    assert sch.timesteps.tolist() == z[f"{name}/timesteps"].tolist()
    assert torch.allclose(sch.sigmas, torch.from_numpy(z[f"{name}/sigmas"]), rtol=1e-6, atol=0)
    g = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}
    return cfg_name, sch, noise * sch.init_noise_sigma, text, steps, g, torch.from_numpy(z["sample_index"]).long()


def _last_losses(trace):
    """The loss of each step's last guidance iteration, as latent_backward_guidance returns it."""
    out = {}
    for t in trace:
        out[t["index"]] = t["loss"]
    return [out[i] for i in sorted(out)]


def test_plain_euler_v_prediction_vs_golden(dev):
    """pipelines.generate under Euler / v_prediction / linspace, free-running: every step's scaled UNet input and the final
    latents."""
    cfg_name, sch, lat0, text, steps, g, idx = _case("tiny_sd21_euler_v")
    sm = LMDSampler(engine(cfg_name, dev))
    lat, _, hist = sd_generate_batch(sm, [text], lat0, steps, guidance_scale=GUIDANCE, scheduler=sch, decode=False,
                                     save_all_latents=True)
    c_in = 1 / (sch.sigmas[:-1].double() ** 2 + 1).sqrt()
    per = [rel_l2(hist[0][k, 0].reshape(-1).cpu().double()[idx] * c_in[k], g["inputs_sample"][k]) for k in range(steps)]
    print("[tiny_sd21_euler_v] rel-L2 per step input: " + " ".join(f"{v:.2e}" for v in per))
    gate("[tiny_sd21_euler_v] max rel-L2 of the UNet inputs (free-running)", max(per), LIMIT_PLAIN[0])
    gate("[tiny_sd21_euler_v] final latents rel-L2", rel_l2(lat, g["final"]), LIMIT_PLAIN[1])


def test_guided_euler_teacher_forced_vs_golden(dev):
    """generate_semantic_guidance under Euler: every step replayed from the golden's own latents of that step — scaled
    guidance passes with the sigma^2 update, scaled CFG pass, Euler step — must land on the golden's next latents, with
    the golden's iteration counts and losses."""
    cfg_name, sch, lat0, text, steps, g, idx = _case("tiny_euler_guided")
    sm = LMDSampler(engine(cfg_name, dev))
    hist_ref = torch.from_numpy(g["latents_all"])
    assert torch.allclose(hist_ref[0], lat0, rtol=1e-6, atol=0)       # init_noise_sigma: an fp32 ulp from host to host
    worst_loss = 0.0
    for i in range(steps):
        tr = []
        out = sm.denoise(hist_ref[i], text, steps, guidance_scale=GUIDANCE, guidance=guidance_dict(), first_step=i, n_steps=1,
                         scheduler=sch, trace=tr)
        torch.cuda.synchronize()
        assert out["guidance_iters"] == int(g["guidance_iters"][i]) == (MAX_ITER[i] if i < MAX_INDEX_STEP else 0)
        if tr:
            worst_loss = max(worst_loss, abs(_last_losses(tr)[0] - g["guidance_losses"][i]) / g["guidance_losses"][i])
        gate(f"[tiny_euler_guided] teacher-forced step {i} ({out['guidance_iters']} guidance iterations): latents rel-L2",
             rel_l2(out["latents_all"][i + 1], hist_ref[i + 1]), LIMIT_EULER_TF[i])
    gate("[tiny_euler_guided] guidance loss, worst relative difference", worst_loss, LIMIT_LOSS["euler"])


def test_guided_lms_free_running_vs_golden(dev):
    cfg_name, sch, lat0, text, steps, g, idx = _case("tiny_lms_guided")
    sm = LMDSampler(engine(cfg_name, dev))
    tr = []
    out = sm.denoise(lat0, text, steps, guidance_scale=GUIDANCE, guidance=guidance_dict(), scheduler=sch, trace=tr)
    torch.cuda.synchronize()
    assert out["guidance_iters"] == int(g["guidance_iters"].sum()) == sum(MAX_ITER)
    assert [sum(1 for t in tr if t["index"] == i) for i in range(steps)] == g["guidance_iters"].tolist()
    per = [rel_l2(out["latents_all"][k, 0].reshape(-1).cpu()[idx], g["latents_sample"][k]) for k in range(1, steps + 1)]
    print("[tiny_lms_guided] rel-L2 after each step: " + " ".join(f"{v:.2e}" for v in per))
    losses = _last_losses(tr)
    worst_loss = max(abs(a - b) / b for a, b in zip(losses, g["guidance_losses"][:MAX_INDEX_STEP]))
    gate("[tiny_lms_guided] max rel-L2 of the latents after each step (free-running)", max(per), LIMIT_LMS[0])
    gate("[tiny_lms_guided] final latents rel-L2", rel_l2(out["latents"], g["final"]), LIMIT_LMS[1])
    gate("[tiny_lms_guided] guidance loss, worst relative difference", worst_loss, LIMIT_LOSS["lms"])
    with pytest.raises(RuntimeError, match="LMSDiscreteScheduler"):
        sm.denoise(lat0, text, steps, first_step=1, n_steps=1, scheduler=sch)
    for s in (sch, make_scheduler("euler")):
        with pytest.raises(RuntimeError, match="fast schedule"):
            sm.denoise(lat0, text, steps, fast_after_steps=2, scheduler=s)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["euler", "lms"])
def test_graph_replay_equals_eager(dev, kind):
    """Plain and guided: the captured graphs replay the eager launch sequence bit for bit; and a DDIM run on the same state
    in between is not disturbed by the scaled graphs, nor they by it."""
    cfg_name, _, lat0, text, steps, _, _ = _case("tiny_euler_guided")
    eng = engine(cfg_name, dev)
    outs = []
    for graphs in (True, False):
        sm = LMDSampler(eng, use_graphs=graphs)
        plain = sm.denoise(lat0, text, steps, scheduler=make_scheduler(kind))
        ddim = sm.denoise(lat0 / lat0.std(), text, steps)
        guided = sm.denoise(lat0, text, steps, guidance=guidance_dict(), scheduler=make_scheduler(kind))
        outs.append((plain["latents_all"], ddim["latents_all"], guided["latents_all"]))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0][0], outs[0][2])            # guidance moved the latents


def test_batch_matches_single(dev):
    """Two jobs in one call against the two run singly (bucket 2 vs bucket 1: where the GEMM tiles differ, fp16 rounding does):
    the sigma-space samplers stay within 3x of what the same comparison measures for the DDIM path — measured: all three
    bit-identical on the tiny net —; and the two jobs swapped give the same latents (no image sees the other)."""
    cfg = weights.CONFIGS["tiny"]
    sm = LMDSampler(engine("tiny", dev))
    g = torch.Generator().manual_seed(9)
    noise = [torch.randn((1, 4, 32, 32), generator=g) for _ in range(2)]
    texts = []
    for i in range(2):
        unc, cond = weights.synth_embeddings(cfg, 1, seed=10 + i)
        texts.append(torch.cat([unc, cond]))
    worst = {}
    for name, sch in (("euler", make_scheduler("euler")), ("lms", make_scheduler("lms")), ("ddim", DDIMScheduler())):
        lats = [n * sch.init_noise_sigma for n in noise]
        batch, _ = sd_generate_batch(sm, texts, lats, 6, scheduler=sch, decode=False)
        rev, _ = sd_generate_batch(sm, texts[::-1], lats[::-1], 6, scheduler=sch, decode=False)
        assert relerr(rev.flip(0), batch) < 1e-6, name
        errs = [relerr(batch[i:i + 1], sd_generate_batch(sm, [texts[i]], [lats[i]], 6, scheduler=sch, decode=False)[0])
                for i in range(2)]
        print(f"[{name}] batched (bucket 2) vs single (bucket 1): " + " ".join(f"{e:.3e}" for e in errs))
        worst[name] = max(errs)
    for name in ("euler", "lms"):
        gate(f"[batch vs single] {name}, worst image vs 3x the DDIM path's", worst[name], 3 * max(worst["ddim"], 1e-7))


def test_dropin_under_load_synthetic_scheduler_cls(dev):
    """models.load_synthetic(..., scheduler_cls="EulerDiscreteScheduler") -> pipelines.generate_semantic_guidance: the
    sampler's own free-running latents of the guided Euler case, and the golden's within the free-running limit."""
    sys.path.insert(0, os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    import models
    from models import pipelines
    cfg_name, sch, lat0, text, steps, g, idx = _case("tiny_euler_guided")
    md = models.load_synthetic(cfg_name, device=dev, with_vae=False, scheduler_cls="EulerDiscreteScheduler")
    assert type(md.scheduler) is EulerDiscreteScheduler and md.scheduler.config.timestep_spacing == "linspace"
    assert md.sampler.scheduler is md.scheduler
    emb = (text.to(dev), text[0:1].to(dev), text[1:2].to(dev))
    lat, images, hist = pipelines.generate_semantic_guidance(
        md, lat0.to(dev), emb, steps, BBOXES, ["a", "b"], OBJ_POS, guidance_scale=GUIDANCE,
        semantic_guidance_kwargs=dict(SG_KWARGS, verbose=False), save_all_latents=True, show_progress=False)
    assert images is None and hist.shape[0] == steps + 1
    own = LMDSampler(engine(cfg_name, dev)).denoise(lat0, text, steps, guidance_scale=GUIDANCE, guidance=guidance_dict(), scheduler=sch)
    print(f"[dropin euler] against the sampler's own run: {relerr(hist, own['latents_all']):.3e}; against the golden, "
          f"final rel-L2 {rel_l2(lat, g['final']):.3e}")
    assert torch.equal(hist.cpu(), own["latents_all"].cpu())
    # latent_backward_guidance under the scheduler it is handed: one call at step 1 equals the sampler's
    md2 = models.load_synthetic(cfg_name, device=dev, with_vae=False)
    models.model_dict = md2
    one, loss = pipelines.latent_backward_guidance(sch, md2.unet, text[1:2].to(dev), 1, BBOXES, OBJ_POS, sch.timesteps[1],
                                                   torch.from_numpy(g["latents_all"][1]).to(dev), torch.tensor(10000.),
                                                   model_dict=md2, **{k: v for k, v in SG_KWARGS.items()})
    md2.scheduler.set_timesteps(steps)
    ddim, _ = pipelines.latent_backward_guidance(md2.scheduler, md2.unet, text[1:2].to(dev), 1, BBOXES, OBJ_POS,
                                                 md2.scheduler.timesteps[1],
                                                 torch.from_numpy(g["latents_all"][1]).to(dev), torch.tensor(10000.),
                                                 model_dict=md2, **{k: v for k, v in SG_KWARGS.items()})
    assert not torch.equal(one, ddim) and abs(float(loss) - g["guidance_losses"][1]) / g["guidance_losses"][1] < LIMIT_LOSS["euler"]


# ---------------------------------------------------------------------------------------------------------------------
# measured on the MI355X: latents after step 0 / step 1 2.69e-3 / 2.71e-3 (rel-L2; guidance losses 45.5198 43.5569 45.3055
# against the oracle's 45.5225 43.5582 45.3035); limits 3x.  The test's ~16 s are the 860 M seeded weights and their engine, as
# in the other full-width tests: at 32x32 latents it measured 15.7 s (3.62e-3 / 3.67e-3), so the latents stay at 64x64
LIMIT_FULL = [8.1e-3, 8.1e-3]


def test_sd14_gligen_two_guided_euler_steps_vs_oracle(dev):
    """Full width (sd14_gligen topology, synthetic weights, 64x64 latents, fuser off): two guided Euler steps of a 6-step
    linspace schedule, free-running, against the loop of pipelines.py:129-247 written over oracle/restate.py's UNet and
    energy (fp32, CPU) and driven by tests/sigma_sched_restate.EulerRestate: scale_model_input in front of both passes
    (:42, :196), the update latents - grad * sigmas[index] ** 2 (:61)."""
    import restate as R
    cfg = weights.CONFIGS["sd14_gligen"]
    sd = weights.synth_state_dict(cfg, 0)
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    cd = dict(block_out_channels=cfg.block_out_channels, layers_per_block=cfg.layers_per_block,
              attention_head_dim=cfg.attention_head_dim, norm_num_groups=cfg.norm_num_groups, norm_eps=cfg.norm_eps,
              gligen_positive_len=cfg.gligen_positive_len)
    T, run = 6, 2
    keys = SG_KWARGS["guidance_attn_keys"]
    ekw = {k: SG_KWARGS[k] for k in ("use_ratio_based_loss", "fg_top_p", "bg_top_p", "fg_weight", "bg_weight")}
    unc, cond = weights.synth_embeddings(cfg, 1, seed=1)
    ehs = torch.cat([unc, cond])
    ref = EulerRestate(**scheduler_config("epsilon"))
    x = torch.randn((1, 4, 64, 64), generator=torch.Generator().manual_seed(0)) * float(ref.init_noise_sigma)
    ref.set_timesteps(T)
    lat, hist_ref, losses_ref = x.clone(), [], []
    for index, t in enumerate(ref.timesteps[:run]):
        for _ in range(MAX_ITER[index]):
            lat = lat.detach().requires_grad_(True)
            saved = {}
            with torch.enable_grad():
                R.unet_forward(sd, cd, ref.scale_model_input(lat, t), t, cond, saved=saved, save_keys=keys, stop_after=keys[-1])
                loss = R.compute_ca_lossv3(saved, BBOXES, OBJ_POS, keys, index=index, **ekw) * SG_KWARGS["loss_scale"]
                grad = torch.autograd.grad(loss, [lat])[0]
            lat = lat.detach() - grad * ref.sigmas[index] ** 2
            losses_ref.append(float(loss))
        with torch.no_grad():
            e = R.unet_forward(sd, cd, torch.cat([ref.scale_model_input(lat, t)] * 2), t, ehs)
            lat = ref.step(e[:1] + GUIDANCE * (e[1:] - e[:1]), t, lat).prev_sample
        hist_ref.append(lat.clone())
    sm = LMDSampler(UNetEngine(cfg, dev, sd))
    tr = []
    out = sm.denoise(x, ehs, T, guidance_scale=GUIDANCE, guidance=guidance_dict(), n_steps=run,
                     scheduler=make_scheduler("euler"), trace=tr)
    torch.cuda.synchronize()
    assert out["guidance_iters"] == sum(MAX_ITER) == len(tr)
    print("[sd14_gligen euler] guidance losses hip " + " ".join(f"{t['loss']:.4f}" for t in tr) + " oracle " +
          " ".join(f"{v:.4f}" for v in losses_ref))
    for i in range(run):
        gate(f"[sd14_gligen euler] latents after guided step {i} (free-running) rel-L2",
             rel_l2(out["latents_all"][i + 1], hist_ref[i]), LIMIT_FULL[i])
