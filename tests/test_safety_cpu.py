"""The safety checker (csrc/safety.hip, lgd_amd/safety.py, lgd_amd/clip_processor.py), checked where there is no GPU:

  * every REFUSALS row of tests/safety_cases.py answers exactly LGD_ERR_ARG through the library with placeholder pointers, the
    limits answer LGD_ERR_UNSUPPORTED, and the accepted calls reach the launch (asked only on a host without a GPU, where the
    launch answers LGD_ERR_LAUNCH; with one it would run on those addresses);
  * the decision rule's restatement gives the known answers, equals the reference's `round(score, 3) > 0` on a sweep around the
    boundary, and every mutation of it changes an answer of the table;
  * DeviceClipProcessor parses transformers' default CLIPImageProcessor, refuses what it does not serve, and its geometry
    with a numpy restatement of the arithmetic reproduces transformers' processor;
  * the loader consumes a state dict under diffusers' key names completely and refuses an unknown key."""
import os
import sys

import numpy as np
import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import _lib, ops
from lgd_amd.clip_processor import DeviceClipProcessor
from lgd_amd.safety import HipSafetyChecker, SafetyConfig, default_processor_config, synth_state_dict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import safety_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_LAUNCH, ERR_UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__ as ge
    ge.build()


def _answer(fn, change):
    return getattr(_lib.load(), fn)(*sc.call_args(fn, change))


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def test_exports_and_header():
    header = open(os.path.join(ROOT, "include", "lgd_hip.h")).read()
    assert "#define LGD_ABI_VERSION 12" in header and _lib.ABI_VERSION == 12
    for fn in sc.ARGS:
        assert f"int {fn}(" in header and hasattr(_lib.load(), fn)
        assert len(sc.ARGS[fn].split()) == len(_lib.SIGNATURES[fn]), fn
    assert callable(ops.safety_head) and callable(ops.blank_flagged)


def test_the_refusal_table_is_well_formed():
    labels = {}
    for fn, what, change in sc.REFUSALS + sc.UNSUPPORTED:
        assert set(change) <= {n[2:] if n.startswith("p:") else n for n in sc.ARGS[fn].split()}, (fn, what)
        assert what not in labels.setdefault(fn, set()), (fn, what)
        labels[fn].add(what)
    for fn in sc.ARGS:
        assert {f"{p} NULL" for p in sc.pointers(fn)} <= labels[fn]
        assert {f"{p} off {a // 2} bytes" for p, a in sc.ALIGN[fn].items()} <= labels[fn]
    assert {"D = 6", "B = 0", "B = -1", "n_concepts = 0", "D = 1028", "n_concepts = 65", "n_special = 33",
            "B = 65536"} <= labels["lgd_safety_head_f32"]
    assert {"N = 0", "image_bytes = -1", "flag_stride = 0"} <= labels["lgd_blank_flagged_u8"]
    # an overlap row moves an operand by a multiple of its alignment: it is refused for the overlap
    for fn, what, change in sc.REFUSALS:
        for k, v in change.items():
            if isinstance(v, tuple):
                assert v[1] % sc.ALIGN[fn].get(k, 1) == 0, (fn, what)


@pytest.mark.parametrize("fn,what,change", sc.REFUSALS, ids=[f"{f}:{w}" for f, w, _ in sc.REFUSALS])
def test_host_refusal(fn, what, change):
    assert _answer(fn, change) == ERR_ARG, (fn, what)


@pytest.mark.parametrize("fn,what,change", sc.UNSUPPORTED, ids=[f"{f}:{w}" for f, w, _ in sc.UNSUPPORTED])
def test_limits_are_unsupported(fn, what, change):
    assert _answer(fn, change) == ERR_UNSUPPORTED, (fn, what)


def test_accepted_calls_reach_the_launch():
    if torch.cuda.is_available():
        pytest.skip("the placeholder pointers would be launched on")
    for fn, change in sc.ACCEPTED:
        assert _answer(fn, change) == ERR_LAUNCH, (fn, change)


def _wrapper_faults():
    f = lambda *s: torch.zeros(*s)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    i = lambda *s: torch.zeros(*s, dtype=torch.int32)
    return [("safety_head: embeds dtype", lambda: ops.safety_head(f(2, 8).half(), f(3, 8), f(3), f(17, 8), f(17))),
            ("safety_head: embeds narrower than D", lambda: ops.safety_head(f(2, 4), f(3, 8), f(3), f(17, 8), f(17))),
            ("safety_head: embeds column stride", lambda: ops.safety_head(f(2, 16)[:, ::2], f(3, 8), f(3), f(17, 8), f(17))),
            ("safety_head: special without its weights", lambda: ops.safety_head(f(2, 8), f(3, 8), None, f(17, 8), f(17))),
            ("safety_head: special width", lambda: ops.safety_head(f(2, 8), f(3, 4), f(3), f(17, 8), f(17))),
            ("safety_head: concept_w count", lambda: ops.safety_head(f(2, 8), f(3, 8), f(3), f(17, 8), f(16))),
            ("safety_head: scores count", lambda: ops.safety_head(f(2, 8), f(3, 8), f(3), f(17, 8), f(17), scores=f(2, 17))),
            ("safety_head: flags dtype", lambda: ops.safety_head(f(2, 8), f(3, 8), f(3), f(17, 8), f(17), flags=f(2, 2))),
            ("blank_flagged: images dtype", lambda: ops.blank_flagged(f(2, 4, 4, 3), i(2))),
            ("blank_flagged: images strided", lambda: ops.blank_flagged(u8(2, 4, 8, 3)[:, :, :4], i(2))),
            ("blank_flagged: flags count", lambda: ops.blank_flagged(u8(2, 4, 4, 3), i(3))),
            ("blank_flagged: flags dtype", lambda: ops.blank_flagged(u8(2, 4, 4, 3), torch.zeros(2, dtype=torch.int64))),
            ("blank_flagged: flags is a matrix", lambda: ops.blank_flagged(u8(2, 4, 4, 3), i(2, 2)))]


_FAULTS = _wrapper_faults()


@pytest.mark.parametrize("what,call", _FAULTS, ids=[w for w, _ in _FAULTS])
def test_wrapper_check_raises_before_the_library(what, call, monkeypatch):
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail(f"{what}: the library was called"))
    with pytest.raises(RuntimeError):
        call()


def test_wrappers_pass_strides_and_counts(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "_call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    e = torch.zeros(2, 12)[:, :8]
    _, flags = ops.safety_head(e, None, None, torch.zeros(5, 8), torch.zeros(5))
    ops.blank_flagged(torch.zeros(2, 4, 4, 3, dtype=torch.uint8), flags[:, 0])
    (n0, a0), (n1, a1) = calls
    assert n0 == "lgd_safety_head_f32" and len(a0) == len(_lib.SIGNATURES[n0]) and a0[1] == 12 and a0[4] == 0 and a0[7] == 5
    assert a0[2].value is None and a0[3].value is None and a0[10:12] == (2, 8)
    assert n1 == "lgd_blank_flagged_u8" and len(a1) == len(_lib.SIGNATURES[n1]) and a1[1] == 48 and a1[3] == 2 and a1[4] == 2


# ---------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.RULE_CASES, ids=[c[0] for c in sc.RULE_CASES])
def test_rule_known_answers(case):
    _, special, concepts, hits, nsfw, special_hit = case
    cos = special + concepts
    got = sc.decide(cos, [0.0] * len(cos), len(special))
    assert (got["hits"], got["has_nsfw"], got["special"]) == (hits, nsfw, special_hit)
    assert all(sc.hit_reference(s) == h for s, h in zip(got["scores"], got["hits"]))    # the reference's own test agrees


@pytest.mark.parametrize("mutation", sc.MUTATIONS)
def test_rule_mutation_changes_an_answer(mutation):
    changed = []
    for name, special, concepts, hits, nsfw, special_hit in sc.RULE_CASES:
        cos = special + concepts
        got = sc.decide(cos, [0.0] * len(cos), len(special), mutation)
        if (got["hits"], got["has_nsfw"], got["special"]) != (hits, nsfw, special_hit):
            changed.append(name)
    print(f"[mutation] {mutation}: changes {changed}")
    assert changed


def test_hit_test_is_the_reference_rounding():
    """fl32(s * 1000) > 0.5 against round(numpy.float32(s), 3) > 0: 20 000 values within 2e-6 of 0.0005, 20 000 in +-0.05 and
    the hand-picked ones.  (A sweep of 400 005 values gave no mismatch when the rule was written; this one keeps the test
    quick.)"""
    g = np.random.default_rng(0)
    vals = np.concatenate([0.0005 + g.uniform(-2e-6, 2e-6, 20000), g.uniform(-0.05, 0.05, 20000),
                           [0.0005, 0.0004, 0.0006, 0.0, -0.0005]]).astype(np.float32)
    bad = [float(v) for v in vals if sc.hit(v) != sc.hit_reference(v)]
    assert not bad, bad[:5]


def test_head_cases_keep_their_margin():
    """The GPU comparison asks for exact flags: every fp64 score of every case is farther from 0.0005 than twice the cosine
    bound, and the four outcomes occur."""
    seen = set()
    for shape in sc.HEAD_SHAPES:
        B, D, ns, nc, ld = shape
        c = sc.head_case(*shape)
        scores, flags, through = sc.head_reference(c["cos"], c["w"], ns)
        assert c["margin"] == 2 * sc.cosine_bound(D) and float(np.abs(scores - 0.0005).min()) > c["margin"], shape
        seen |= {sc.outcome(flags[b], through[b]) for b in range(B)}
        # the fp32 restatement decides as the fp64 one
        for b in range(min(B, 3)):
            got = sc.decide(c["cos"][b].astype(np.float32), c["w"], ns)
            assert (int(got["has_nsfw"]), int(got["special"])) == tuple(flags[b]), (shape, b)
    assert seen == {"nothing", "special only", "concept", "concept through the adjustment"}, seen


# ---------------------------------------------------------------------------------------------
# the processor
# ---------------------------------------------------------------------------------------------
def _hf_processor(**kw):
    from transformers import CLIPImageProcessor
    return CLIPImageProcessor(**kw)


def test_processor_parses_transformers_default():
    hf = _hf_processor()
    for src in (hf, hf.to_dict(), default_processor_config()):
        p = DeviceClipProcessor(src)
        assert (p.edge, p.filter) == (224, "bicubic") and abs(p.rescale - 1 / 255) < 1e-12
        assert np.allclose(p.mean, hf.image_mean, atol=0, rtol=1e-7) and np.allclose(p.std, hf.image_std, atol=0, rtol=1e-7)


@pytest.mark.parametrize("what,change", [
    ("a non-square crop", dict(crop_size={"height": 224, "width": 200})),
    ("a fixed (height, width) size", dict(size={"height": 224, "width": 224})),
    ("an unknown filter", dict(resample=0)),
    ("no resize", dict(do_resize=False)),
    ("no centre crop", dict(do_center_crop=False)),
    ("a crop of another size", dict(crop_size={"height": 200, "width": 200})),
    ("two mean values", dict(image_mean=(0.5, 0.5))),
])
def test_processor_refuses(what, change):
    with pytest.raises(ValueError):
        DeviceClipProcessor(dict(default_processor_config(), **change))


@pytest.mark.parametrize("hw", [(512, 512), (512, 2048), (72, 80), (80, 72)])
def test_processor_geometry_against_transformers(hw):
    s = 224 if hw[0] >= 512 else 28
    p = DeviceClipProcessor(default_processor_config(s))
    (H, W), (top, left) = sc.clip_geometry(hw[0], hw[1], s)
    assert p.resized_size(*hw) == (H, W) and p.crop_box(H, W) == (top, left) and min(H, W) == s
    g = np.random.default_rng(hw[0] * 4096 + hw[1])
    images = g.integers(0, 256, (1,) + hw + (3,), dtype=np.uint8)
    hf = _hf_processor(size={"shortest_edge": s}, crop_size={"height": s, "width": s})
    want = hf(images=[im for im in images], return_tensors="np")["pixel_values"]
    got = sc.clip_pixel_values(images, s, p.mean, p.std, p.rescale)
    err = float(np.abs(got - want).max())
    print(f"[processor] {hw} -> {(H, W)} crop at {(top, left)}: max |restatement - transformers| {err:.3e} (gate 1e-6)")
    assert got.shape == want.shape == (1, 3, s, s) and err < 1e-6


# ---------------------------------------------------------------------------------------------
# the loader
# ---------------------------------------------------------------------------------------------
TINY = SafetyConfig(image_size=56, patch_size=14, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                    num_attention_heads=2, projection_dim=32)


def _diffusers_state_dict(cfg, seed=0):
    """A CLIPVisionModelWithProjection's weights under diffusers' StableDiffusionSafetyChecker key names."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    hf = CLIPVisionModelWithProjection(CLIPVisionConfig(
        image_size=cfg.image_size, patch_size=cfg.patch_size, hidden_size=cfg.hidden_size,
        intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, projection_dim=cfg.projection_dim)).eval()
    sd = {("vision_model." + k if k.startswith("vision_model.") else k): v for k, v in hf.state_dict().items()}
    sd["concept_embeds"], sd["special_care_embeds"] = torch.randn(17, cfg.projection_dim), torch.randn(3, cfg.projection_dim)
    sd["concept_embeds_weights"], sd["special_care_embeds_weights"] = torch.rand(17), torch.rand(3)
    return hf, sd


def test_loader_consumes_diffusers_keys():
    _, sd = _diffusers_state_dict(TINY)
    assert "vision_model.vision_model.pre_layrnorm.weight" in sd and "visual_projection.weight" in sd
    m = HipSafetyChecker(TINY, sd, "cpu")
    assert m.consumed == set(sd) and not m.unused
    assert tuple(m.patch.shape) == (64, 592) and not bool(m.patch[:, 588:].any())        # K: 588 -> 592, zeros
    assert m.processor.edge == 56 and len(m.layers) == 2
    m = HipSafetyChecker(TINY, dict(sd, **{"vision_model.vision_model.embeddings.position_ids": torch.arange(17)[None]}), "cpu")
    assert m.unused == ["vision_model.vision_model.embeddings.position_ids"]
    with pytest.raises(RuntimeError, match="does not know"):
        HipSafetyChecker(TINY, dict(sd, extra_key=torch.zeros(1)), "cpu")
    with pytest.raises(KeyError):
        HipSafetyChecker(TINY, {k: v for k, v in sd.items() if k != "concept_embeds_weights"}, "cpu")


def test_synthetic_state_dict_has_the_same_keys():
    _, sd = _diffusers_state_dict(TINY)
    syn = synth_state_dict(TINY, seed=3, concept_threshold=-1.0)
    assert {k: tuple(v.shape) for k, v in syn.items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert bool((syn["concept_embeds_weights"] == -1.0).all()) and syn["special_care_embeds_weights"].shape == (3,)
    m = HipSafetyChecker.synthetic(TINY, seed=3, device="cpu", concept_threshold=1.0)
    assert bool((m.concept_w == 1.0).all())


def test_default_stays_off():
    """Opting in is the only way a result moves: the public entry points take the checker as a keyword that defaults to none."""
    import inspect
    from lgd_amd.pipeline import sd_generate_batch
    assert inspect.signature(sd_generate_batch).parameters["safety_checker"].default is None
