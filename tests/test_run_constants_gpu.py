"""The constants of a run on the device against fp64 (tests/unet_fwd_plan_cases.py, last section; the bound is derived there
and shown neither too tight nor blind by tests/test_run_constants_cpu.py):

  * prepare_timesteps([981, 601, 1]): every resnet's slice of the table (w.temb_offsets) against sinusoid -> linear_1 -> SiLU ->
    linear_2 -> SiLU -> time_emb_proj with by-name weights; set_step(1) leaves row 601 in temb_cur bit for bit and changes
    neither the text K/V nor the concat buffers;
  * the text_time branch (tiny_xl, R = 2 images with different text_embeds and time_ids): the layout [T][temb_rows x sum Cout],
    per-image rows in their places, rows >= R zero;
  * prepare_text with Bt = 3: every layer's [K | V], the "@1" layers included; rows >= Bt x T keep what they held;
  * prepare_gligen with Bt = 4: PositionNet's tokens (UNetEngine._objs), and the grounding tails of every fuser layer against
    fuser.linear + fuser.norm1 of those tokens as given, for concat buffers of B = 4 and B = 2 (the Bt // 2 arm) at
    obj_batch_offset 0 and, for B = 2, 2; the buffer of B = 4 at offset 2 (toff + B > Bt) and one of B = 3 stay untouched, as do
    the visual rows of every buffer.  The first half of the grounding batch is masked out (the null features), 27 of the 30
    tokens are unused and one box between two live ones is masked.

Measured on an MI355X (worst error / bound): time-embedding table 2.3e-3 (22 resnet slices), text_time table 4.1e-4 (22 slices
x 2 images), [K | V] 0.48 (tiny_xl, 22 layers) and 0.33 (tiny_gligen, 16 layers), PositionNet's tokens 3.2e-3, grounding tails
0.078 (16 fuser layers x 3 served buffers); set_step exact; nothing outside the declared rows was written.  The host emulation
of the same rounding points gives 2.3e-3, 4.1e-4, 0.56, 0.34, 3.6e-3 and 0.14.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_fwd_plan_cases as Fw  # noqa: E402
import unet_plan_cases as U  # noqa: E402
from conftest import gate  # noqa: E402
from lgd_amd import weights  # noqa: E402
from lgd_amd.unet import N_OBJ_TOKENS, UNetEngine  # noqa: E402

F64, H16 = torch.float64, torch.float16
SENT = 2.0


def engine(name, dev):
    cfg = weights.CONFIGS[name]
    sd = weights.synth_state_dict(cfg, 0)
    return cfg, {k: v.to(F64) for k, v in sd.items()}, UNetEngine(cfg, dev, sd), Fw.constant_inputs(cfg)


def resnet_widths(cfg, sd64):
    return {r.prefix: sd64[f"{r.prefix}.time_emb_proj.weight"].shape[0] for b in weights.unet_blocks(cfg) for r in b.resnets}


def test_temb_table_and_set_step(dev):
    cfg, sd64, eng, d = engine("tiny_gligen", dev)
    plan = eng.plan(2, U.L, fuser=True)                                  # its concat buffers and K/V are part of the snapshot
    eng.prepare_text(d["ehs"])
    eng.prepare_gligen(**d["gligen"])
    tab = eng.prepare_timesteps(Fw.TIMESTEPS)
    torch.cuda.synchronize()
    ref = Fw.temb_tables(Fw.RefB(), cfg, sd64, Fw.TIMESTEPS)
    widths = resnet_widths(cfg, sd64)
    assert tuple(tab.shape) == (3, sum(widths.values())) and set(eng.w.temb_offsets) == set(ref)
    worst = max(Fw.const_ratio(tab[:, eng.w.temb_offsets[p]:eng.w.temb_offsets[p] + n], ref[p]) for p, n in widths.items())
    gate(f"tiny_gligen: {len(ref)} resnet slices of the time-embedding table, worst error / bound", worst, 1.0)
    others = list(eng.text_kv.values()) + list(eng._fuser_cat.values()) + [tab]
    before = [t.clone() for t in others]
    eng.set_step(1)
    torch.cuda.synchronize()
    assert torch.equal(U._bits(eng.temb_cur[0]), U._bits(tab[1]))
    assert all(torch.equal(U._bits(a), U._bits(b)) for a, b in zip(others, before)), "set_step changed a text K/V or concat buffer"
    assert plan is not None


def test_text_time_table_layout(dev):
    cfg, sd64, eng, d = engine("tiny_xl", dev)
    tab = eng.prepare_timesteps(Fw.TIMESTEPS, d["added"])
    torch.cuda.synchronize()
    ref = Fw.temb_tables(Fw.RefB(), cfg, sd64, Fw.TIMESTEPS, d["added"])
    widths = resnet_widths(cfg, sd64)
    total, Rn = sum(widths.values()), d["added"]["time_ids"].shape[0]
    assert tuple(tab.shape) == (3, eng.temb_rows * total)
    t3 = tab.view(3, eng.temb_rows, total)
    assert not bool(t3[:, Rn:].any()), "rows of images the call did not name are not zero"
    worst = 0.0
    for p, n in widths.items():
        off = eng.w.temb_offsets[p]
        worst = max(worst, Fw.const_ratio(t3[:, :Rn, off:off + n], ref[p].reshape(3, Rn, n)))
    gate(f"tiny_xl: {len(ref)} resnet slices x {Rn} images of the text_time table, worst error / bound", worst, 1.0)
    eng.set_step(1)
    torch.cuda.synchronize()
    assert torch.equal(U._bits(eng.temb_cur), U._bits(t3[1]))


@pytest.mark.parametrize("name", ["tiny_xl", "tiny_gligen"])
def test_prepare_text(dev, name):
    cfg, sd64, eng, d = engine(name, dev)
    for kv in eng.text_kv.values():
        kv.fill_(SENT)
    eng.prepare_text(d["ehs"])
    torch.cuda.synchronize()
    ref = Fw.text_kv(Fw.RefB(), cfg, sd64, d["ehs"])
    assert set(ref) == set(eng.text_kv)
    assert (name == "tiny_xl") == any("@1" in k for k in ref)
    Bt = d["ehs"].shape[0]
    worst = max(Fw.const_ratio(eng.text_kv[k][:Bt], ref[k]) for k in ref)
    gate(f"{name}: [K | V] of {len(ref)} layers for a text batch of {Bt}, worst error / bound", worst, 1.0)
    assert all(bool((kv[Bt:] == SENT).all()) for kv in eng.text_kv.values()), "rows behind the text batch were written"


def test_prepare_gligen(dev):
    cfg, sd64, eng, d = engine("tiny_gligen", dev)
    plan = eng.plan(2, U.L, fuser=True)
    S_of = {m["name"][:-len(".transformer_blocks.0.fuser.norm1")]: m["S"] for m in (op.meta for op in plan.ops)
            if m["kind"] == "layernorm" and m["S"]}
    forms = [(4, 0), (2, 0), (2, 2), (4, 2), (3, 0)]                    # (B, obj_batch_offset); the last two are not served
    for B, off in forms:
        for k, S in S_of.items():
            eng.fuser_cat(k, B, S, off)
    for cat in eng._fuser_cat.values():
        cat.fill_(SENT)
    gl = d["gligen"]
    Bt = gl["boxes"].shape[0]
    eng.prepare_gligen(**gl)
    torch.cuda.synchronize()
    ref_objs = Fw.position_net_objs(Fw.RefB(), cfg, sd64, gl["boxes"], gl["masks"], gl["positive_embeddings"])
    gate("tiny_gligen: PositionNet's grounding tokens, error / bound", Fw.const_ratio(eng._objs, ref_objs), 1.0)
    ref = Fw.grounding_tails(Fw.RefB(), cfg, sd64, Fw.E(eng._objs.cpu()), Bt)
    assert set(ref) == set(S_of)
    worst, served = 0.0, 0
    for (k, B, off), cat in eng._fuser_cat.items():
        c3 = cat.view(B, S_of[k] + N_OBJ_TOKENS, -1)
        assert bool((c3[:, :S_of[k]] == SENT).all()), f"visual rows of the concat buffer {k, B, off} were written"
        if (B, off) in forms[:3]:
            served += 1
            r = ref[k]
            worst = max(worst, Fw.const_ratio(c3[:, S_of[k]:], Fw.E(r.v[off:off + B], r.e[off:off + B])))
        else:
            assert bool((cat == SENT).all()), f"the concat buffer {k, B, off} is not served by this call and was written"
    assert served == 3 * len(S_of)
    gate(f"tiny_gligen: grounding tails of {len(S_of)} fuser layers x 3 served buffers, worst error / bound", worst, 1.0)
