"""The constants of a run against fp64, without a GPU (tests/unet_fwd_plan_cases.py, last section): with the reference alone

  * an fp32 / fp16 emulation of exactly the engine's rounding points stays inside the derived bound of every constant: the
    time-embedding table of tiny and of tiny_xl (text_time, R = 2 images), the text K/V of every layer ("@1" included),
    PositionNet's grounding tokens and the grounding tails of every fuser layer;
  * four wrong constants fall outside it: sin and cos exchanged in the timestep sinusoid, PositionNet's freq base 100 -> 10000,
    the null feature applied where mask = 1, the K and V halves exchanged;
  * the value the bound is centred on (fp64 with the storage roundings applied) is tied to the exact-weight fp64 constants
    (Setup.pure_constants' formulas: oracle/restate.py) at rel-L2 <= 8 x 2^-11: at most eight storage roundings of relative
    size 2^-11 lie between the two (measured 1e-4 .. 4e-4, printed).

PositionNet's first contraction has K = 832 (768 phrase-embedding columns, 64 Fourier columns); a worst-case bound sees the
Fourier columns only if they carry a comparable share of it, so the phrase embeddings of these tests are drawn at 2^-4
(unet_fwd_plan_cases.EMB_SCALE).  Measured error / bound of the wrong constants: sincos 12.9 (tiny) / 2.3 (tiny_xl), freq base
1.36, null feature 1.55, K | V swapped > 1e3."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_fwd_plan_cases as Fw  # noqa: E402
import unet_plan_cases as U  # noqa: E402
from conftest import gate  # noqa: E402
from lgd_amd import weights  # noqa: E402

F64 = torch.float64
R = Fw.R
_C = {}


def case(name):
    if name not in _C:
        cfg = weights.CONFIGS[name]
        sd = weights.synth_state_dict(cfg, 0)
        _C[name] = (cfg, sd, {k: v.to(F64) for k, v in sd.items()}, Fw.constant_inputs(cfg))
    return _C[name]


def constants(be, name, what, wrong=None):
    cfg, sd, sd64, d = case(name)
    sd = sd64 if be.ref else sd
    if what == "temb":
        return Fw.temb_tables(be, cfg, sd, Fw.TIMESTEPS, d.get("added"), wrong=wrong)
    if what == "kv":
        return Fw.text_kv(be, cfg, sd, d["ehs"], wrong=wrong)
    gl = d["gligen"]
    objs = Fw.position_net_objs(be, cfg, sd, gl["boxes"], gl["masks"], gl["positive_embeddings"], wrong=wrong)
    if what == "objs":
        return {"objs": objs}
    given = Fw.position_net_objs(Fw.EmuB(), cfg, case(name)[1], gl["boxes"], gl["masks"], gl["positive_embeddings"]).to(torch.float16)
    return Fw.grounding_tails(be, cfg, sd, Fw.E(given) if be.ref else given.float(), gl["boxes"].shape[0])


CONSTANTS = [("tiny", "temb"), ("tiny_xl", "temb"), ("tiny_xl", "kv"), ("tiny_gligen", "kv"), ("tiny_gligen", "objs"), ("tiny_gligen", "tails")]


@pytest.mark.parametrize("name,what", CONSTANTS)
def test_emulation_stays_inside_the_bound(name, what):
    ref, emu = constants(Fw.RefB(), name, what), constants(Fw.EmuB(), name, what)
    assert set(ref) == set(emu) and ref
    worst = max(Fw.const_ratio(emu[k], ref[k]) for k in ref)
    loose = max(float((ref[k].e / ref[k].v.abs().clamp_min(2.0 ** -14)).median()) for k in ref)
    print(f"[run constants] {name} {what}: {len(ref)} tensors, emulation error / bound {worst:.4f}, median bound / |value| {loose:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("name,what,wrong", [("tiny", "temb", "sincos"), ("tiny_xl", "temb", "sincos"), ("tiny_gligen", "objs", "freq"),
                                             ("tiny_gligen", "objs", "null"), ("tiny_xl", "kv", "kv")])
def test_wrong_constant_falls_outside(name, what, wrong):
    ref, bad = constants(Fw.RefB(), name, what), constants(Fw.EmuB(), name, what, wrong=wrong)
    ratios = [Fw.const_ratio(bad[k], ref[k]) for k in ref]
    print(f"[run constants] {name} {what} with {wrong} wrong: error / bound {min(ratios):.3g} .. {max(ratios):.3g}")
    assert min(ratios) > 1.0                               # every tensor of the constant shows it


def test_values_are_the_pure_constants():
    Fn = torch.nn.functional
    for name in ("tiny_xl", "tiny_gligen"):
        cfg, sd, sd64, d = case(name)
        ref = constants(Fw.RefB(), name, "kv")
        ehs = d["ehs"].to(F64).reshape(-1, d["ehs"].shape[-1])
        worst = 0.0
        for k, r in ref.items():
            p, _, dpt = k.partition("@")
            t = f"{p}.transformer_blocks.{dpt or 0}.attn2"
            pure = torch.cat([Fn.linear(ehs, sd64[f"{t}.to_k.weight"]), Fn.linear(ehs, sd64[f"{t}.to_v.weight"])], -1)
            worst = max(worst, U.rel_l2(r.v, pure))
        gate(f"{name}: text K/V value vs the exact-weight fp64 constant, worst rel-L2", worst, 8 * 2.0 ** -11)
    cfg, sd, sd64, d = case("tiny_gligen")
    gl = {k: v.to(F64) for k, v in d["gligen"].items()}
    pure = R.position_net(sd64, gl["boxes"], gl["masks"], gl["positive_embeddings"])
    objs = constants(Fw.RefB(), "tiny_gligen", "objs")["objs"]
    gate("tiny_gligen: PositionNet value vs oracle/restate.position_net in fp64, rel-L2", U.rel_l2(objs.v, pure), 8 * 2.0 ** -11)
    # the time embedding of tiny against Setup.pure_constants' own chain (case F's setup: timestep 601 is row 1 of the table)
    s = Fw.FSetup("F")
    pc = s.pure_constants()
    ref = constants(Fw.RefB(), "tiny", "temb")
    worst = 0.0
    for m in s.graph.metas:
        if m["kind"] == "conv" and m["temb_off"] is not None:
            worst = max(worst, U.rel_l2(ref[m["name"][:-len(".conv1")]].v[1], s.temb_rows_of(m, pc)[0]))
    gate("tiny: time-embedding rows of timestep 601 vs Setup.pure_constants, worst rel-L2", worst, 8 * 2.0 ** -11)
