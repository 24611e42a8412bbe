"""The UNet reverse plan without a GPU (tests/unet_plan_cases.py): for every case

  * the graph read from the plan's metas IS the UNet: its fp64 forward equals oracle/restate.unet_forward in fp64 on the same
    inputs, at every saved map and every named activation;
  * graph + VJP statements ARE the gradient: the fp64 VJP chain, fed random map cotangents, equals torch.autograd through the
    restatement at the latents and at every named activation.  Both compare reference with reference, at rel-L2 <= 1e-9
    (fp64 roundoff over ~200 ops; measured 2e-15 .. 2e-14, printed).  This settles the graph, the statements and the
    intentional constant cuts against an independent oracle;
  * completeness holds;
  * the fp32 emulation of the plan passes the walker: every ratio <= 1 (the bounds are not too tight), integrity holds;
  * the sensitivity condition holds: with the case's power-of-two cotangent scale (unet_plan_cases.COT_SCALE = 2^9 for all
    cases) every gradient tensor of the fp64 chain has a median |value| >= 2^-11 — so the 2^-25 term of the bounds is at most
    2^-14 of it — and no |value| above 2^14.  Measured: the smallest median is 1.05 (case D, the GEGLU of down_blocks.1), the
    largest value 6478 (case C); no tensor needs the 2^-14 floor.  The rows of the fuser's grounding tokens are structurally 0.

Wrong plans (the emulated ops are altered, not the kernels), each caught where stated:
  accumulate flag inverted on a fan-in            per-op check        .wd taps not flipped                 per-op check
  Wd row slices of the two sources swapped        per-op check        alpha dropped in a dgrad             per-op check
  fuser tail rows not cleared                     per-op check (NaN)  a pending gradient buffer overwritten  integrity
  an Act removed from a gouts                     completeness, and the chain against autograd

Case F: UNetEngine.plan refuses a grad plan behind up block 1 before any op is built."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_plan_cases as U  # noqa: E402
from conftest import gate  # noqa: E402

F64 = torch.float64
CASE_NAMES = sorted(U.CASES)
_SETUP, _ORACLE = {}, {}


def setup(case):
    if case not in _SETUP:
        _SETUP[case] = U.Setup(case)
    return _SETUP[case]


def oracle(case):
    """(chain, chain maps, restatement maps, taps, autograd latent gradient, autograd tap gradients): computed once"""
    if case not in _ORACLE:
        s = setup(case)
        ch = U.Chain(s, pure=True)
        maps = ch.forward(s.lat)
        _ORACLE[case] = (ch, maps) + U.restate_run(s, s.cot)
    return _ORACLE[case]


@pytest.mark.parametrize("case", CASE_NAMES)
def test_graph_is_the_unet(case):
    s = setup(case)
    ch, maps, saved, taps, _, _ = oracle(case)
    worst = max(U.rel_l2(maps[k], saved[k].detach()) for k in s.keys)
    named = [n for n in s.plan.dbg if n in taps]
    assert named, "no named activation in common with the restatement"
    worst = max([worst] + [U.rel_l2(ch.vals[id(s.plan.dbg[n])], U.tap_to_rows(taps[n].detach())) for n in named])
    print(f"[unet plan {case}] {len(s.plan.ops)} ops, {len(named)} named activations")
    gate(f"case {case}: fp64 graph forward vs the restatement, worst rel-L2 over maps and named activations", worst, 1e-9)


@pytest.mark.parametrize("case", CASE_NAMES)
def test_vjp_chain_is_the_gradient(case):
    s = setup(case)
    ch, _, _, taps, g_auto, tap_grads = oracle(case)
    g, grads = ch.backward(s.cot, 1.0)
    worst = U.rel_l2(g, g_auto)
    named = [n for n in s.plan.dbg if n in tap_grads and id(s.plan.dbg[n]) in grads]
    assert named
    worst = max([worst] + [U.rel_l2(grads[id(s.plan.dbg[n])], U.tap_to_rows(tap_grads[n])) for n in named])
    gate(f"case {case}: fp64 VJP chain vs torch.autograd, worst rel-L2 over the latents and {len(named)} named activations", worst, 1e-9)
    # ---- sensitivity condition, with the fp64 chain alone (at the scale the walkers divide the latent gradient by, too)
    lo, hi, lo_name = math.inf, 0.0, None
    # the fuser's concat buffer and its q | k | v projection: the gradient rows of the 30 grounding tokens are structurally 0
    padded = {id(m["out"]): m["S"] for m in s.graph.metas if m["kind"] == "layernorm" and m["S"]}
    padded.update({id(m["ins"][0]): m["S"] for m in s.graph.metas if m["kind"] == "self_attn" and m["Sk"] > m["S"]})
    for i, m in enumerate(s.graph.metas):
        for a in U.Graph.inputs(m):
            if id(a) in grads:
                t = grads[id(a)].abs()
                if id(a) in padded:
                    t = t.view(s.B, padded[id(a)] + U.N_OBJ_TOKENS, -1)[:, :padded[id(a)]]
                med = float(t.median())
                if med < lo:
                    lo, lo_name = med, s.graph.label(i)
                hi = max(hi, float(t.max()))
    gl = (g / U.GRAD_SCALE).abs()
    lo, hi = min(lo, float(gl.median())), max(hi, float(gl.max()))
    print(f"[unet plan {case}] smallest median |gradient| {lo:.4g} ({lo_name}), largest |gradient| {hi:.4g}")
    assert lo >= 2.0 ** -11 and hi <= 2.0 ** 14


@pytest.mark.parametrize("case", CASE_NAMES)
def test_completeness(case):
    assert setup(case).graph.completeness() == []


@pytest.mark.parametrize("case", CASE_NAMES)
def test_emulated_plan_passes_the_walker(case):
    s = setup(case)
    w = U.Walker(s)
    w.run()
    assert w.integrity == [], w.integrity[:5]
    assert w.x0_grad_stable
    f, fname = w.worst("fwd")
    b, bname = w.worst("bwd")
    print(f"[unet plan {case}] emulation: forward {f:.4f} ({fname}), backward {b:.4f} ({bname})")
    assert f <= 1.0, (f, fname)
    assert b <= 1.0, (b, bname)


# ---- wrong plans ---------------------------------------------------------------------------------------
def _walk(case, mutant, i, **kw):
    s = setup(case)
    w = U.Walker(s, U.Emulator(s, mutant))
    w.run(check_fwd=set(), check_bwd={i}, until=i, **kw)
    return w


def test_mutant_accumulate_flag_inverted():
    s = setup("E")
    i = U.find_op(s, lambda m, op: op.bwd is not None and any(op.acc))
    pos = s.plan.ops[i].acc.index(True)
    assert _walk("E", None, i, integrity=False).bwd_ratio[i][0] <= 1.0
    w = _walk("E", dict(kind="acc_inverted", op=i, pos=pos), i, integrity=False)
    assert w.bwd_ratio[i][0] > 1.0 and w.bwd_ratio[i][1] == f"gradient {pos}", w.bwd_ratio[i]
    # the other direction: a first writer that accumulates adds to the poison
    j = U.find_op(s, lambda m, op: op.bwd is not None and m["kind"] == "linear" and not op.acc[0])
    assert _walk("E", dict(kind="acc_inverted", op=j, pos=0), j, integrity=False).bwd_ratio[j][0] == math.inf


def test_mutant_wd_taps_not_flipped():
    s = setup("E")
    i = U.find_op(s, lambda m, op: m["kind"] == "conv" and op.bwd is not None)
    w = _walk("E", dict(kind="wd_not_flipped", op=i), i, integrity=False)
    assert w.bwd_ratio[i][0] > 1.0 and w.bwd_ratio[i][1] == "gradient 0", w.bwd_ratio[i]


def test_mutant_wd_row_slices_swapped():
    s = setup("A")
    # the two-source dgrads of the UNet are the conv_shortcuts behind a skip concat (Wt row slices); Plan.conv's are unused
    i = max(j for j, m in enumerate(s.graph.metas) if m["kind"] == "shortcut" and len(m["ins"]) == 2)
    assert _walk("A", None, i, integrity=False).bwd_ratio[i][0] <= 1.0
    w = _walk("A", dict(kind="wd_slices_swapped", op=i), i, integrity=False)
    assert w.bwd_ratio[i][0] > 1.0, w.bwd_ratio[i]


def test_mutant_alpha_dropped_and_tail_rows_not_cleared():
    s = setup("B")
    i = max(j for j, m in enumerate(s.graph.metas) if m["kind"] == "linear" and m["params"]["alpha"])
    assert s.graph.metas[i]["alpha"] not in (0.0, 1.0)
    w = _walk("B", dict(kind="alpha_dropped", op=i), i, integrity=False)
    assert w.bwd_ratio[i][0] > 1.0 and w.bwd_ratio[i][1] == "gradient 0", w.bwd_ratio[i]
    j = max(k for k, m in enumerate(s.graph.metas) if m["kind"] == "self_attn" and m["Sk"] > m["S"])
    w = _walk("B", dict(kind="tail_not_cleared", op=j), j, integrity=False)
    assert w.bwd_ratio[j][0] == math.inf, w.bwd_ratio[j]            # the poison is still in the rows of the grounding tokens


def test_mutant_pending_gradient_overwritten():
    """conv_in's output feeds norm1 and, as the residual, conv2 of the first resnet: its gradient is written by conv2's backward
    and waits for norm1's.  norm2's backward, in between, overwrites it."""
    s = setup("E")
    x0 = s.plan._x0
    writer = U.find_op(s, lambda m, op: m["kind"] == "conv" and m["res"] is x0)
    i = writer - 1
    assert x0 not in s.plan.ops[i].gouts
    s2 = setup("E")
    w = U.Walker(s2, U.Emulator(s2, dict(kind="clobber", op=i, victim=x0)))
    w.run(check_fwd=set(), check_bwd=set())
    assert len(w.integrity) == 1 and w.integrity[0].startswith(f"backward of {s.graph.label(i)} changed gradient"), w.integrity


def test_mutant_act_removed_from_gouts():
    s = setup("E")
    ch, _, _, _, g_auto, _ = oracle("E")
    i = U.find_op(s, lambda m, op: m["kind"] == "conv" and m["res"] is not None)
    pos = s.plan.ops[i].gouts.index(s.graph.metas[i]["res"])
    bad = s.graph.completeness(gouts_of={i: [a for a in s.plan.ops[i].gouts if a is not s.graph.metas[i]["res"]]})
    assert len(bad) == 1 and bad[0][0] == s.graph.label(i), bad
    g, _ = ch.backward(s.cot, 1.0, drop={(i, pos)})
    assert U.rel_l2(g, g_auto) > 1e-9


# ---- case F ---------------------------------------------------------------------------------------------
def test_grad_plan_behind_up_block_1_is_refused():
    s = U.Setup("E", build_plan=False)
    before = len(s.eng._arena)
    with pytest.raises(ValueError) as e:
        s.eng.plan(2, U.L, grad=True, stop_key=("up", 2, 0, 0), save_keys=[("up", 2, 0, 0)])
    assert str(e.value) == ("grad plan refused: attention key ('up', 2, 0, 0) lies in up block 2, and a grad plan ends at up block 1 "
                            "at the latest (no dgrad weights are packed behind it)")
    with pytest.raises(ValueError, match="grad plan refused: without a stop_key the plan runs to the end of the network"):
        s.eng.plan(2, U.L, grad=True, save_keys=[("mid", 0, 0, 0)])
    assert len(s.eng._arena) == before and not s.eng._plans, "something was built before the refusal"
    s.eng.plan(2, U.L, grad=False, save_keys=[("up", 3, 0, 0)])          # serving such keys without a gradient is untouched


def test_restatement_runs_in_fp64_and_fp32_is_unchanged():
    import restate as R
    t = torch.tensor([1, 601, 999])
    half = 32
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    e = t[:, None].float() * freqs[None]
    assert torch.equal(R.timestep_embedding(t, 64), torch.cat([torch.cos(e), torch.sin(e)], dim=-1))
    assert R.timestep_embedding(t, 64, F64).dtype == F64
