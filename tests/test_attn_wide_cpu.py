"""lgd_attn_wide_f16 where there is no GPU (tests/attn_wide_cases.py):

  * the derived bound of attn_conformance_cases.fwd_reference is not too tight for this kernel — an fp32 emulation with
    the kernel's rounding points and its tiling (32 keys, running max, P rounded to fp16) stays inside on every case and
    data pass the GPU suite runs — and not too loose: a dropped last key, a counted pad key and an omitted scale fall
    outside;
  * the host refusals are what the REFUSALS table says, answered by the entry point before the device is touched;
  * the "hot" operands of the GPU suite meet their own preconditions;
  * the VAE classes accept "materialised" and "streamed" and nothing else, and the builders hand the keyword down.

(The 4096 x 4096 x 512 case of the GPU suite is left out here: its fp64 reference is GPU work.)"""
import inspect
import os
import sys

import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import _lib, vae

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_conformance_cases as acc  # noqa: E402
import attn_wide_cases as awc  # noqa: E402

F32, F64, H16 = torch.float32, torch.float64, torch.float16


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__ as ge
    ge.build()


def _ops64(case, ps):
    d = case.data(ps)
    return d.q[:, 0].to(F64), d.k[:, 0].to(F64), d.v[:, 0].to(F64)


@pytest.mark.parametrize("name", list(awc.BY_NAME))
def test_emulation_with_the_kernels_roundings_stays_inside_the_bound(name):
    case = awc.BY_NAME[name]
    worst = {}
    for ps in awc.PASSES:
        q, k, v = _ops64(case, ps)
        ref = awc.reference(case, q, k, v)
        assert bool(torch.isfinite(ref["o"]).all()) and bool((ref["bound_o"] > 0).all()), ps
        worst[ps] = awc.ratio(awc.emulation(q.to(F32), k.to(F32), v.to(F32), case.scale), ref)
    print(f"[attn_wide bound] {name}: emulation error / bound " + ", ".join(f"{p} {v:.3f}" for p, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("name", [n for n, c in awc.BY_NAME.items() if c.Sk >= 8])
def test_a_dropped_last_key_is_outside_the_bound(name):
    """Spiked data: one query puts nearly all its weight on the last key."""
    case = awc.BY_NAME[name]
    q, k, v = _ops64(case, "spiked")
    ref = awc.reference(case, q, k, v)
    assert awc.ratio(awc.emulation(q.to(F32), k.to(F32), v.to(F32), case.scale, drop_last=True), ref) > 2.0


@pytest.mark.parametrize("name", [n for n, c in awc.BY_NAME.items() if c.Sk <= 77])
def test_a_counted_pad_key_is_outside_the_bound(name):
    """At most 77 keys, offset V and small logits: a zero pad key takes 1 / (Sk + 1) of the weight (at 330 keys that
    fraction is of the size of the bound itself: test_attn_conformance_cpu.py)."""
    case = awc.BY_NAME[name]
    q, k, v = _ops64(case, "voffset")
    ref = awc.reference(case, q, k, v)
    assert awc.ratio(awc.emulation(q.to(F32), k.to(F32), v.to(F32), case.scale, pad_key=True), ref) > 2.0


@pytest.mark.parametrize("name", [n for n, c in awc.BY_NAME.items() if c.Sk > 1])
@pytest.mark.parametrize("ps", awc.PASSES)
def test_an_omitted_scale_is_outside_the_bound(name, ps):
    case = awc.BY_NAME[name]
    q, k, v = _ops64(case, ps)
    ref = awc.reference(case, q, k, v)
    assert awc.ratio(awc.emulation(q.to(F32), k.to(F32), v.to(F32), case.scale, no_scale=True), ref) > 2.0


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_the_refusal_table_is_well_formed():
    names = [n[2:] if n.startswith("p:") else n for n in awc.ARGS.split()]
    for what, change, _ in awc.REFUSALS:
        assert set(change) <= set(names), what
        assert len(awc.refusal_args(change, acc.P)) == len(_lib.SIGNATURES["lgd_attn_wide_f16"]), what
    assert {what for what, _, _ in awc.REFUSALS} >= {"NULL q", "B < 1", "Sq < 1", "Sk < 1", "d < 8", "d % 8", "ldq < d", "o is q", "d > 512"}


@pytest.mark.parametrize("what,change,code", awc.REFUSALS, ids=[w for w, _, _ in awc.REFUSALS])
def test_host_refusal(what, change, code):
    rc = _lib.load().lgd_attn_wide_f16(*awc.refusal_args(change, acc.P))
    assert rc == code, (what, rc)
    with pytest.raises(RuntimeError):
        _lib.check(rc, "lgd_attn_wide_f16")


def test_the_abi_version_did_not_move():
    assert _lib.load().lgd_abi_version() == 12 and "lgd_attn_wide_f16" in _lib.SIGNATURES


# ---------------------------------------------------------------------------------------------
# the "hot" operands
# ---------------------------------------------------------------------------------------------
def test_hot_operands_meet_their_preconditions():
    q, k, v = (t.to(F64) for t in awc.hot_operands())
    t = q @ k.T                                                        # scale = 1
    idx = torch.tensor([awc.hot_target(i) for i in range(awc.HOT_S)])
    assert len(set(idx.tolist())) == awc.HOT_S
    target = t[torch.arange(awc.HOT_S), idx]
    assert float(target.min()) > 65504.0                               # every row's target logit is beyond fp16
    assert bool(torch.isinf(t.to(H16)).any(dim=1).all())               # and its fp16 store has +inf in every row
    assert bool((t.to(H16)[torch.arange(awc.HOT_S), idx] == float("inf")).all())
    rest = t.clone()
    rest[torch.arange(awc.HOT_S), idx] = float("-inf")
    second = rest.amax(dim=1)
    assert float((target - second).min()) >= 100.0                     # fp32 softmax: exp2(-144) and below, exactly one-hot
    assert float((second / target).max()) < 0.75                       # "about half": 70 q_i . q_i' against 70 |q_i|^2
    assert float((q.norm(dim=1) - awc.HOT_NORM).abs().max()) < 0.05
    # the emulation of the kernel returns v[j(i)] to the last bit: the only rounding left is O's, of an fp16 value
    o = awc.emulation(q.to(F32)[None], k.to(F32)[None], v.to(F32)[None], 1.0)[0]
    assert torch.equal(o, v.to(F32)[idx])


# ---------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------
def test_the_vae_classes_take_the_two_modes_and_nothing_else():
    sd = vae.synth_aekl_state_dict((32, 32, 64, 64), 1, seed=1)
    assert vae.ATTENTION_MODES == ("materialised", "streamed")
    for cls in (vae.HipVAEDecoder, vae.HipVAEEncoder, vae.HipVAE):
        assert inspect.signature(cls.__init__).parameters["attention"].default == "materialised"
        assert cls(sd, "cpu").attention == "materialised"
        assert cls(sd, "cpu", attention="streamed").attention == "streamed"
        for bad in ("flash", "", None, "Streamed"):
            with pytest.raises(ValueError, match="attention is one of"):
                cls(sd, "cpu", attention=bad)
    both = vae.HipVAE(sd, "cpu", attention="streamed")
    assert both.encoder.attention == "streamed"                        # the lazy encoder inherits it
    assert vae.HipVAE(sd, "cpu").encoder.attention == "materialised"


def test_the_builders_hand_the_keyword_down():
    from lgd_amd import sdxl
    assert inspect.signature(sdxl.build_synthetic).parameters["vae_attention"].default is None
    for fn in (vae.probe_ranges, vae.calibrate_ranges):
        assert inspect.signature(fn).parameters["attention"].default == "materialised"
    assert vae.attention_kw(None) == {} and vae.attention_kw("streamed") == {"attention": "streamed"}
    dropin = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llm-groundeddiffusion_amd", "dropin")
    for rel, fns in (("generation/sdxl_refinement.py", ("init", "init_synthetic", "from_diffusers")), ("models/models.py", ("load_sd",))):
        src = open(os.path.join(dropin, rel)).read()
        for fn in fns:
            head = src[src.index(f"def {fn}("):]
            assert "vae_attention=None" in head[:head.index('"""')], (rel, fn)
