"""No loop state and no captured graph leaks into the next call ("What a call owes the state it reuses").

The rule of every test here: each call of a sequence runs on ONE long-lived sampler with captured graphs, after
state_reuse_cases.poison has overwritten every floating device tensor reachable from it with NaN patterns and set the
engine-wide frozen-step count to 1000; the same call runs on `fresh(engine)`, a new sampler on a new engine that shares the
packed weights only.  Final latents, the whole history, every saved map and the guidance iteration count must be equal bit
for bit — the project already holds samplers and lanes to bit-reproducibility, so there is no tolerance to set.

What the suite found when it was written (both fixed since, the tests stay as the guard):
  * the frozen-mask blend of cfg_ddim / cfg_multistep / cfg_lms multiplies frozen_ref rows by the mask, and the host loaded
    those rows only for jobs with a mask and a history, and only as many as the history had: on a used state the job
    without a mask, and both jobs with histories of 2 rows under frozen_steps = 3, came back NaN (sequence B);
  * latents_all returned the state's whole history: after first_step=2, n_steps=1 (sequence A, call 6) and in both
    MultiDiffusion paths (sequence F) the rows the call had not written were the earlier call's (here: the poison).
One mutation the issue names is NOT caught, because it changes nothing a kernel reads: `st.picks.zero_()` in
multidiffusion_generate.  The state key holds the step count and the bootstrapping count, so the picks rows a step reads
(step < min(n_boot, steps)) are exactly the rows every call overwrites.

Wall time on the MI355X (pytest's `call` phase, both arms of every call): A 3.2 s, B 0.9 s, C 1.5 s, D 1.8 s, E 0.8 s,
F 1.0 s (region) and 0.7 s (views)."""
import os
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lgd_amd  # noqa: E402,F401
from lgd_amd import weights  # noqa: E402
from lgd_amd.unet import UNetEngine  # noqa: E402
from conftest import gate  # noqa: E402
import state_reuse_cases as sr  # noqa: E402

_BASE = {}


def base(name, dev):
    """The engine that owns the packed weights of a configuration: packed once per module, never run."""
    if name not in _BASE:
        cfg = weights.CONFIGS[name]
        kw = dict(max_text_batch=2) if cfg.addition_embed_type == "text_time" else {}
        _BASE[name] = UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0), **kw)
    return _BASE[name]


def run_sequence(sm, make_fresh, calls, after=None):
    """Runs `calls` on the long-lived `sm` (poisoned before each) and each on a fresh arm -> the first arm's results.
    Every difference of the whole sequence is reported, not only the first."""
    t0, bad, outs = time.perf_counter(), [], []
    for i, call in enumerate(calls):
        sr.poison(sm)
        a = sr.run_call(sm, call)
        other = make_fresh()
        b = sr.run_call(other, call)
        torch.cuda.synchronize()
        bad += [f"call {i + 1} ({call['label']}): {d}" for d in sr.differences(a, b)]
        outs.append(a)
        if after is not None:
            after(i, call, other)
        del other, b
        sr.release()
    print(f"[state reuse] {len(calls)} calls, both arms: {time.perf_counter() - t0:.2f} s")
    assert not bad, "results on the reused state differ from a fresh sampler's:\n  " + "\n  ".join(bad)
    return outs


def assert_only_rows(hist, first, last, what):
    """The contract of loop.history_of: rows first .. last are the call's, every other row is zero."""
    rows = hist.shape[0]
    other = [r for r in range(rows) if not first <= r <= last]
    assert other, what
    assert float(hist[other].abs().max()) == 0.0, f"{what}: rows the call did not write are not zero"
    for r in range(first, last + 1):
        assert float(hist[r].abs().max()) > 0.0, f"{what}: row {r} is empty"


# ---- A ----------------------------------------------------------------------------------------------------------------------
def test_scheduler_and_conditioning_changes_on_one_state(dev):
    """Ten calls on the one (1, C, 32) state of a tiny_gligen sampler: PLMS, guided + GLIGEN + frozen DDIM, plain DDIM at
    scale 1, DPM-Solver with a frozen mask, guided LMS, one Euler step in mid-schedule, BoxDiff, LMD guidance, inversion,
    the fast schedule.  Call 2 is also held to the reference's own loop at test_gligen_loop's limits."""
    eng = base("tiny_gligen", dev)
    sm = sr.fresh(eng)
    outs = run_sequence(sm, lambda: sr.fresh(eng), sr.SEQ_A)
    assert len(sm._states.states) == 1 and next(iter(sm._states.states))[0] == 1       # one state served all ten
    kinds = sorted(next(iter(sm._states.states.values())).steps)
    assert len(kinds) == 4, kinds                                                        # DDIM, multistep, PLMS, LMS
    # call 2 against tests/golden/loops_tiny_gligen.npz (the reference's generate_gligen), at the limits of
    # test_engine_gpu.py::test_gligen_loop
    g = np.load(os.path.join(sr.GOLD, "loops_tiny_gligen.npz"))
    out = outs[1][0]
    ref = torch.from_numpy(g["gligen_latents_all"])
    e = float((out["latents_all"].cpu() - ref).abs().max() / ref.abs().max())
    got, want = out[f"saved{('up', 1, 1, 0)}"][1].double().cpu(), torch.from_numpy(g["gligen_saved_up11_step1"]).double()
    assert out["guidance_iters"] == 4
    gate("[state reuse] call 2, gligen latents_all (free-running)", e, 5e-2)
    gate("[state reuse] call 2, gligen saved map rel-L2", float((got - want).norm() / want.norm()), 1.5e-1)
    # the partial schedule: 5 steps, first_step=2, n_steps=1 -> rows 2 (its start) and 3 (its step)
    assert_only_rows(outs[sr.PARTIAL_A][0]["latents_all"], 2, 3, "Euler first_step=2, n_steps=1")
    # the inversion returns T rows, all its own
    assert outs[8][0]["inverted"].shape[0] == 4


# ---- B ----------------------------------------------------------------------------------------------------------------------
def test_frozen_blend_reads_only_what_this_call_loaded(dev):
    """frozen_steps > 0 in a batch of two where one job has no mask and no history, then histories shorter than
    frozen_steps + 1 rows: the blend of the step kernels reads frozen_ref rows that this call did not load."""
    eng = base("tiny_gligen", dev)
    run_sequence(sr.fresh(eng), lambda: sr.fresh(eng), sr.SEQ_B)


# ---- C ----------------------------------------------------------------------------------------------------------------------
def test_capacity_grows_and_a_short_run_follows(dev):
    """60 steps exceed the capacity of a new state (STATE_MIN_STEPS), so the state and its graphs are made again; a 4-step
    run then replays the 60-step state's graphs over its longer tables, and 60 steps run again."""
    eng = base("tiny", dev)
    sm = sr.fresh(eng)
    sr.run_call(sm, sr.denoise_call("4 steps first: a state of the minimum capacity", "tiny", 4, seed=20))
    small = next(iter(sm._states.states.values()))
    assert small.capacity == sm.STATE_MIN_STEPS < 60
    run_sequence(sm, lambda: sr.fresh(eng), sr.SEQ_C)
    big = next(iter(sm._states.states.values()))
    assert big is not small and big.capacity == 60 and len(sm._states.states) == 1


# ---- D ----------------------------------------------------------------------------------------------------------------------
def test_eviction_of_plans_and_states_under_live_graphs(dev):
    """MAX_PLANS = 2 and one resident state: plans are dropped and built again while graphs captured over them live, and
    states are dropped while their plans live.  The arena is only ever carved again from offset 0, never freed or moved:
    a plan built again has the addresses it had, which is what the comment at the eviction promises the graphs."""
    eng = base("tiny", dev)
    sm = sr.fresh(eng)
    sm.eng.MAX_PLANS = 2
    sm._states.capacity = 1
    seen, keep, rebuilt, need = {}, [], [], [0]

    def addresses(plan):
        return (plan.latents_in.data_ptr(), plan.eps_out.data_ptr() if plan.eps_out is not None else None,
                tuple(sorted((k, v.data_ptr()) for k, v in plan.maps.items())))

    def after(i, call, other):
        assert len(sm.eng._plans) <= 2 and len(sm._states.states) == 1
        for key, plan in sm.eng._plans.items():
            keep.append(plan)                                   # alive for the whole test: no id is used twice
            need[0] = max(need[0], plan.arena_bytes)
            if key in seen and seen[key][0] != id(plan):
                rebuilt.append(key)
                assert addresses(plan) == seen[key][1], f"call {i + 1}: a plan built again moved in the arena"
            seen[key] = (id(plan), addresses(plan))

    run_sequence(sm, lambda: sr.fresh(eng), sr.SEQ_D, after=after)
    assert len(set(rebuilt)) >= 2, rebuilt
    seg = sm.eng.ARENA_SEGMENT
    assert sm.eng.arena_bytes() <= ((need[0] + seg - 1) // seg + 1) * seg


# ---- E ----------------------------------------------------------------------------------------------------------------------
def test_sdxl_refiner_two_schedules_on_one_state(dev):
    """SDXLRefiner keys its state by (L, steps run) and its graph by "step" alone: 8 steps from index 4, then 4 steps from
    0, with other embeddings, sizes, scores and guidance scale."""
    eng = base("tiny_xl", dev)
    ref = sr.fresh_refiner(eng)
    run_sequence(ref, lambda: sr.fresh_refiner(eng), sr.SEQ_E)
    assert len(ref._states.states) == 1 and len(next(iter(ref._states.states.values())).graphs) == 1


# ---- F ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["region", "views"])
def test_multidiffusion_two_calls_on_one_state(dev, path):
    """multidiffusion_generate twice under one state key: other masks, guidance scale, frozen noise and picks, the second
    call from a later step."""
    eng = base("tiny", dev)
    sm = sr.fresh(eng)
    calls = sr.SEQ_F[path]
    outs = run_sequence(sm, lambda: sr.fresh(eng), calls)
    assert len(sm.md_states.states) == 1
    kw = calls[1]["kw"]
    first = kw["first_step"]
    last = min(sr.MD_STEPS, first + kw["n_steps"]) if kw.get("n_steps") else sr.MD_STEPS
    assert_only_rows(outs[1][0]["latents_all"], first, last, calls[1]["label"])
