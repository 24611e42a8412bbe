"""TEST INFRASTRUCTURE — the state-reuse suite (tests/test_state_reuse_gpu.py, tests/test_state_reuse_cpu.py): what a second
call on a long-lived sampler may find in the fixed-address device state of the first, and the calls whose results must
not depend on it.

Three parts, importable without a GPU:
  * the poison walker: every tensor reachable from a sampler, found by walking the object graph (not from a list of
    attribute names), and `poison`, which overwrites the floating ones on the device with NaN bit patterns and sets the
    engine-wide frozen-step count to 1000;
  * the call descriptions of the sequences A - F: plain dicts (an `api`, a `label`, the arguments), inputs drawn from
    weights.synth_embeddings, seeded generators and the committed goldens;
  * `fresh(engine)`: a new sampler on a new engine that shares only the packed weights, the arm every call is compared
    against bit for bit.
"""
import gc
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = [("mid", 0, 0, 0), ("up", 1, 0, 0), ("up", 1, 1, 0), ("up", 1, 2, 0)]
OBJ_KEY = ("down", 2, 1, 0)
BBOXES = [[74 / 512, 177 / 512, (74 + 183) / 512, (177 + 235) / 512],
          [314 / 512, 193 / 512, (314 + 189) / 512, (193 + 216) / 512]]
OBJ_POS = [[1, 2, 3], [5, 6, 7]]
STALE_FROZEN_STEPS = 1000          # what `poison` leaves in eng.dyn[1]: past every schedule, so a count that is not reset blends


# ---- the poison walker --------------------------------------------------------------------------------------------------
def _is_graph(obj):
    return type(obj).__name__ in ("HipGraph", "CUDAGraph")


def walk_tensors(root, exclude=()):
    """[(path, tensor)] of every torch.Tensor reachable from `root` through `__dict__`, dicts, lists, tuples and sets — so
    through StateCache.states, LoopState.steps and whatever a later change adds — each tensor object once.  Not entered:
    the objects in `exclude` (by identity), captured graphs, modules, functions, classes and torch's own objects.  A tensor
    whose storage is also reachable from an excluded object (a view of a packed weight) is left out as well."""
    barred = set()
    for ex in exclude:
        for _, t in walk_tensors(ex):
            barred.add(_storage_key(t))
    skip = {id(ex) for ex in exclude}
    seen, out = set(), []

    def visit(obj, path):
        if id(obj) in seen or id(obj) in skip:
            return
        seen.add(id(obj))
        if isinstance(obj, torch.Tensor):
            if _storage_key(obj) not in barred:
                out.append((path, obj))
            return
        if obj is None or isinstance(obj, (str, bytes, int, float, bool, complex, np.ndarray, np.generic, type,
                                           types.ModuleType, types.FunctionType, types.MethodType,
                                           types.BuiltinFunctionType, torch.nn.Module, torch.Generator)):
            return
        if _is_graph(obj) or type(obj).__module__.split(".")[0] == "torch":
            return
        if isinstance(obj, dict):
            for k, v in obj.items():
                visit(v, f"{path}[{k!r}]")
        elif isinstance(obj, (list, tuple, set, frozenset)):
            for i, v in enumerate(obj):
                visit(v, f"{path}[{i}]")
        elif hasattr(obj, "__dict__"):
            for k, v in vars(obj).items():
                visit(v, f"{path}.{k}")

    visit(root, type(root).__name__)
    return out


def _storage_key(t):
    return (str(t.device), t.untyped_storage().data_ptr()) if t.numel() else (str(t.device), id(t))


def excluded_of(sampler):
    """What the walker must not enter: the packed weights (shared with every other engine), and a VAE next to the sampler."""
    ex = [sampler.eng.w]
    for name in ("vae", "enc", "dec", "text_encoder"):
        if getattr(sampler, name, None) is not None:
            ex.append(getattr(sampler, name))
    return ex


def poison(sampler, any_device=False):
    """Between two calls: every floating tensor of the sampler's state (on the GPU; anywhere with any_device) gets the
    all-ones byte pattern (NaN in fp16 and fp32, as UNetEngine.poison_arena writes), eng.dyn[1] becomes
    STALE_FROZEN_STEPS, other integer tensors stay.  Values only: nothing poisoned is an address or an index.
    Returns the paths it poisoned."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    done = []
    for path, t in walk_tensors(sampler, exclude=excluded_of(sampler)):
        if not (t.is_cuda or any_device) or not t.is_floating_point() or t.numel() == 0:
            continue
        if t.is_contiguous():
            t.view(torch.uint8).fill_(0xFF)
        else:
            t.fill_(float("nan"))
        done.append(path)
    dyn = getattr(getattr(sampler, "eng", None), "dyn", None)
    if dyn is not None:
        dyn[1:2].fill_(STALE_FROZEN_STEPS)
        done.append("eng.dyn[1]")
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return done


# ---- the other arm --------------------------------------------------------------------------------------------------------
def fresh_engine(engine):
    """A new engine on `engine`'s packed weights (as lanes.make_lanes builds lane 1): nothing a run writes is shared."""
    from lgd_amd.unet import UNetEngine
    return UNetEngine(engine.cfg, engine.device, text_len=engine.text_len, max_text_batch=engine.max_text_batch,
                      weights=engine.w)


def fresh(engine):
    """A new LMDSampler (captured graphs on) on a new engine that shares `engine`'s weights and nothing else."""
    from lgd_amd.sampler import LMDSampler
    return LMDSampler(fresh_engine(engine), use_graphs=True)


def fresh_refiner(engine):
    from lgd_amd.sdxl import SDXLRefiner
    return SDXLRefiner(fresh_engine(engine), None, None, use_graphs=True)


def release():
    """Drops the engines of finished arms (a Plan and its engine refer to each other) and their arenas."""
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def text_of(cfg_name, seed):
    from lgd_amd import weights
    unc, cond = weights.synth_embeddings(weights.CONFIGS[cfg_name], 1, seed=seed)
    return torch.cat([unc, cond])


def scheduler_of(name):
    """A new scheduler object per call, as a caller that passes `scheduler=` makes one."""
    from lgd_amd import scheduler as S
    from sigma_golden_cases import scheduler_config
    if name in ("euler", "lms"):
        cls = S.EulerDiscreteScheduler if name == "euler" else S.LMSDiscreteScheduler
        return cls.from_config(scheduler_config("epsilon"))
    return dict(ddim=S.DDIMScheduler, pndm=S.PNDMScheduler, dpm=S.DPMSolverMultistepScheduler)[name]()


def lmd_guidance(max_iter=(2, 1), max_index_step=3):
    return dict(bboxes=BBOXES, object_positions=OBJ_POS, loss_scale=5, loss_threshold=0.0, max_iter=list(max_iter),
                max_index_step=max_index_step, guidance_attn_keys=KEYS, use_ratio_based_loss=False, fg_top_p=0.2,
                bg_top_p=0.2, fg_weight=1.0, bg_weight=4.0)


def box_mask(L, seed):
    """A frozen mask (L, L) in [0, 1] with a zero region, a one region and fractional values in between."""
    m = torch.rand((L, L), generator=torch.Generator().manual_seed(seed))
    m[: L // 3] = 0.0
    m[-(L // 4):] = 1.0
    return m


def denoise_call(label, cfg, steps, *, sched="ddim", L=32, seed=0, jobs=1, history=(), mask=(), guided=(), **kw):
    """A `denoise_batch` call on `jobs` images of side L.  history: {job: rows} jobs whose latents are a (rows, 1, C, L, L)
    history; mask: jobs that carry a frozen mask; guided: jobs under LMD guidance (kw may carry `guidance=` for another)."""
    return dict(api="denoise", label=label, cfg=cfg, steps=steps, sched=sched, L=L, seed=seed, jobs=jobs,
                history=dict(history), mask=tuple(mask), guided=tuple(guided), kw=kw)


def build_jobs(call):
    from lgd_amd.sampler import Job
    from lgd_amd.weights import CONFIGS
    C, L = CONFIGS[call["cfg"]].in_channels, call["L"]
    sigma = float(scheduler_of(call["sched"]).init_noise_sigma) if call["sched"] in ("euler", "lms") else 1.0
    guidance = call["kw"].get("guidance", lmd_guidance())
    out = []
    for b in range(call["jobs"]):
        s = 100 * call["seed"] + b
        rows = call["history"].get(b)
        lat = rnd(1, C, L, L, seed=s) * sigma if rows is None else rnd(rows, 1, C, L, L, seed=s)
        out.append(Job(lat, text_of(call["cfg"], s + 1), guidance=guidance if b in call["guided"] else None,
                       frozen_mask=box_mask(L, s + 2) if b in call["mask"] else None))
    return out


def golden_gligen_call():
    """The guided + GLIGEN + frozen-mask DDIM call of test_engine_gpu.py's arena test (and of its test_gligen_loop, which
    holds it to the reference's own loop): inputs from tests/golden/loops_tiny_gligen.npz."""
    return dict(api="golden_gligen", label="guided + GLIGEN + frozen mask, DDIM, 4 steps (golden)", cfg="tiny_gligen",
                steps=4, sched="ddim", jobs=1,
                kw=dict(gligen_scheduled_sampling_beta=0.5, frozen_steps=2, saved_cross_attn_keys=[OBJ_KEY, *KEYS],
                        return_cond_ca_only=True))


def refusal_arguments(call):
    """What `_denoise_chunk` hands LMDSampler._refuse_undefined for this call (api "denoise", "golden_gligen", "invert")."""
    kw = call["kw"]
    sch = scheduler_of(call["sched"])
    if call["api"] == "invert":
        from lgd_amd.scheduler import DDIMInverseScheduler
        sch = DDIMInverseScheduler.from_config(sch)
    guided = call["api"] == "golden_gligen" or bool(call.get("guided"))
    gligen = call["api"] == "golden_gligen"
    return sch.step_kind, dict(fast=kw.get("fast_after_steps") is not None, partial=int(kw.get("first_step", 0)) > 0,
                               conditioned=kw.get("frozen_steps", 0) > 0 or gligen or guided,
                               inverse=getattr(sch, "inverse", False),
                               sigma_space=bool(getattr(sch, "scales_model_input", False)),
                               stateless=getattr(sch, "stateless_rows", False))


# ---- the sequences ----------------------------------------------------------------------------------------------------------
G = "tiny_gligen"
SEQ_A = [
    denoise_call("PNDM plain, 6 steps (7 evaluations)", G, 6, sched="pndm", seed=1),
    golden_gligen_call(),
    denoise_call("DDIM plain, 3 steps, guidance scale 1", G, 3, seed=2, guidance_scale=1.0),
    denoise_call("DPM-Solver multistep, frozen mask, 5 steps", G, 5, sched="dpm", seed=3, history={0: 6}, mask=(0,),
                 frozen_steps=2),
    denoise_call("LMS guided, 5 steps", G, 5, sched="lms", seed=4, guided=(0,),
                 guidance=lmd_guidance(max_index_step=2)),
    denoise_call("Euler, first_step=2, n_steps=1", G, 5, sched="euler", seed=5, first_step=2, n_steps=1),
    denoise_call("BoxDiff-guided DDIM, 4 steps", G, 4, seed=6, guided=(0,),
                 guidance=dict(bboxes=BBOXES, object_positions=OBJ_POS, use_boxdiff=True, max_index_step=3)),
    denoise_call("LMD-guided DDIM, 4 steps", G, 4, seed=7, guided=(0,), saved_cross_attn_keys=[OBJ_KEY, *KEYS]),
    dict(api="invert", label="invert_batch, 4 steps", cfg=G, steps=4, sched="ddim", jobs=1, seed=8,
         kw=dict(guidance_scale=3.0)),
    denoise_call("DDIM with fast_after_steps", G, 7, seed=9, fast_after_steps=3),
]
PARTIAL_A = 5                     # index of the partial-schedule call in SEQ_A

SEQ_B = [
    # a state is made of zeros: the two calls after this one must find a USED (2, C, 32) state
    denoise_call("two plain jobs: the (2, C, 32) state exists from here on", G, 4, seed=10, jobs=2),
    denoise_call("two jobs, frozen_steps=2: one with mask and history, one without", G, 4, seed=11, jobs=2,
                 history={0: 5}, mask=(0,), frozen_steps=2),
    denoise_call("two jobs, frozen_steps=3, histories of 2 rows (shorter than frozen_steps + 1)", G, 4, seed=12, jobs=2,
                 history={0: 2, 1: 2}, mask=(0, 1), frozen_steps=3),
]

SEQ_C = [
    denoise_call("60 steps plain (past STATE_MIN_STEPS: a new state)", "tiny", 60, seed=21),
    denoise_call("4 steps plain on the 60-step state", "tiny", 4, seed=22),
    denoise_call("60 steps again", "tiny", 60, seed=23),
]

_D = dict(
    a=denoise_call("guided, 1 image, side 32", "tiny", 3, seed=31, guided=(0,)),
    b=denoise_call("plain with saved maps, 1 image, side 32", "tiny", 3, seed=32, saved_cross_attn_keys=[OBJ_KEY, *KEYS]),
    c=denoise_call("plain, 2 images, side 16", "tiny", 3, L=16, seed=33, jobs=2),
    d=denoise_call("guided, 2 images, side 32", "tiny", 3, seed=34, jobs=2, guided=(0, 1)),
)
# a, b, a: one state, the plans of `a` dropped by `b` and rebuilt under the state's live graphs;  c, d: other states (the
# cache holds one), dropped while their plans live;  a, b again on a rebuilt state
SEQ_D = [_D[k] for k in "abacdab"]

SEQ_E = [
    dict(api="refine", label="8 steps from first_index=4", cfg="tiny_xl", seed=41,
         kw=dict(first_index=4, num_inference_steps=8, guidance_scale=5.0, height=256, width=256)),
    dict(api="refine", label="4 steps from 0", cfg="tiny_xl", seed=42,
         kw=dict(first_index=0, num_inference_steps=4, guidance_scale=7.0, height=512, width=256, aesthetic_score=5.0)),
]


def md_call(label, seed, *, width=64, picks_rows=2, noise=False, **kw):
    """A multidiffusion_generate call: P = 3 prompts on a 64 x `width` latent (64: the region path, wider: the views
    path), 4 steps, 2 bootstrapping backgrounds.  Everything but the shapes follows the seed."""
    return dict(api="md", label=label, cfg="tiny", seed=seed, width=width, picks_rows=picks_rows, noise=noise, kw=kw)


SEQ_F = {
    "region": [md_call("region path, whole schedule", 51, picks_rows=4, guidance_scale=10.0),
               md_call("region path, other masks / scale / noise, first_step=1", 52, noise=True, guidance_scale=6.0,
                       first_step=1, n_steps=2)],
    "views": [md_call("views path, whole schedule", 53, width=72, picks_rows=4, guidance_scale=10.0, normalization=True),
              md_call("views path, other masks / scale / noise, first_step=2", 54, width=72, noise=True, guidance_scale=6.0,
                      normalization=True, first_step=2)],
}
MD_STEPS, MD_BOOT, MD_P = 4, 2, 3


def md_inputs(call):
    from lgd_amd import weights
    from lgd_amd.multidiffusion import get_views
    cfg = weights.CONFIGS[call["cfg"]]
    s, W, P = call["seed"], call["width"], MD_P
    g = torch.Generator().manual_seed(s)
    owner = torch.randint(0, P, (64, W), generator=g)                      # disjoint masks: every pixel has one prompt
    masks = torch.stack([(owner == k).float() for k in range(P)]).reshape(P, 1, 64, W)
    unc, cond = weights.synth_embeddings(cfg, P, seed=s)
    V = len(get_views(8 * 64, 8 * W))
    picks = torch.randint(0, MD_BOOT, (call["picks_rows"], V, P - 1), generator=g)
    return dict(texts=torch.cat([unc.expand(P, -1, -1), cond]), masks=masks, start_latent=rnd(1, cfg.in_channels, 64, W, seed=s + 1),
                bg_latents=rnd(MD_BOOT, cfg.in_channels, 64, 64, seed=s + 2, scale=0.5),
                picks=picks if W != 64 else picks[:, 0],
                noise=rnd(1, cfg.in_channels, 64, W, seed=s + 3) if call["noise"] else None)


# ---- running a call -------------------------------------------------------------------------------------------------------
def run_call(sampler, call):
    """-> dict of results, tensors and ints, that both arms must agree on bit for bit (per job: a list of such dicts)."""
    api = call["api"]
    if api == "denoise":
        kw = {k: v for k, v in call["kw"].items() if k != "guidance"}
        res = sampler.denoise_batch(build_jobs(call), call["steps"], scheduler=scheduler_of(call["sched"]), **kw)
        return [dict(latents=r["latents"], latents_all=r["latents_all"], guidance_iters=r["guidance_iters"],
                     **{f"saved{k}": v for k, v in r["saved"].items()}) for r in res]
    if api == "golden_gligen":
        from lgd_amd.sampler import prepare_gligen_condition
        g = np.load(os.path.join(GOLD, "loops_tiny_gligen.npz"))
        gl = prepare_gligen_condition(BBOXES, torch.from_numpy(g["phrase_emb"]), sampler.dev)
        r = sampler.denoise(torch.from_numpy(g["lat_all_in"]), torch.from_numpy(g["ehs"]), call["steps"], gligen=gl,
                            guidance=lmd_guidance(), frozen_mask=torch.from_numpy(g["frozen_mask"]),
                            return_token_ca_only=7, scheduler=scheduler_of(call["sched"]), **call["kw"])
        return [dict(latents=r["latents"], latents_all=r["latents_all"], guidance_iters=r["guidance_iters"],
                     **{f"saved{k}": v for k, v in r["saved"].items()})]
    if api == "invert":
        from lgd_amd.pipeline import invert_batch
        from lgd_amd.weights import CONFIGS
        lat = rnd(1, CONFIGS[call["cfg"]].in_channels, 32, 32, seed=call["seed"], scale=0.8)
        return [dict(inverted=invert_batch(sampler, [text_of(call["cfg"], call["seed"])], lat, call["steps"], **call["kw"]))]
    if api == "refine":
        from lgd_amd.weights import CONFIGS
        cfg, s = CONFIGS[call["cfg"]], call["seed"]
        lat = rnd(1, cfg.in_channels, 32, 32, seed=s, scale=2.0)
        return [dict(latents=sampler.refine_latents(lat, rnd(2, 77, cfg.cross_attention_dim, seed=s + 1),
                                                    rnd(2, cfg.pooled_dim, seed=s + 2), **call["kw"]))]
    if api == "md":
        from lgd_amd.multidiffusion import multidiffusion_generate
        d = md_inputs(call)
        r = multidiffusion_generate(sampler, d["texts"], d["masks"], d["start_latent"], d["bg_latents"], d["picks"],
                                    steps=MD_STEPS, n_boot=MD_BOOT, decode=False, save_all_latents=True, noise=d["noise"],
                                    **call["kw"])
        return [dict(latent=r["latent"], latents_all=r["latents_all"])]
    raise ValueError(api)


def differences(a, b):
    """Names of the results of one call that differ between two arms, or hold a non-finite value in the first."""
    bad = []
    for j, (ra, rb) in enumerate(zip(a, b)):
        if sorted(ra) != sorted(rb):
            bad.append(f"job {j}: keys")
            continue
        for k, va in ra.items():
            vb = rb[k]
            if torch.is_tensor(va):
                if not bool(torch.isfinite(va).all()):
                    bad.append(f"job {j}: {k} not finite")
                elif va.shape != vb.shape or not torch.equal(va, vb):
                    bad.append(f"job {j}: {k}")
            elif va != vb:
                bad.append(f"job {j}: {k} {va} != {vb}")
    if len(a) != len(b):
        bad.append("job count")
    return bad
