"""The safety checker on the GPU (csrc/safety.hip, lgd_amd/safety.py, lgd_amd/clip_processor.py, the `sd` plug-in): the
head kernel against the fp64 restatement of tests/safety_cases.py, the blanking kernel byte by byte, the device processor
against transformers' CLIPImageProcessor, the tower against transformers' `CLIPVisionModelWithProjection` with seeded
weights (no checkpoint and no diffusers exist on the test machines), `check_device` end to end and from a captured graph,
and the public surface."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lgd_amd  # noqa: E402,F401
import safety_cases as sc  # noqa: E402
from conftest import gate  # noqa: E402
from lgd_amd import ops  # noqa: E402
from lgd_amd.clip_processor import DeviceClipProcessor  # noqa: E402
from lgd_amd.safety import HipSafetyChecker, SafetyConfig, default_processor_config  # noqa: E402

F32 = torch.float32
GUARD = 64


# ---------------------------------------------------------------------------------------------
# the head
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.HEAD_SHAPES, ids=["B{}-D{}-s{}-c{}-ld{}".format(*s) for s in sc.HEAD_SHAPES])
def test_head_against_fp64(dev, shape):
    """Scores within (D + 8) * 2^-24 of the fp64 restatement, flags exactly equal (every fp64 score is farther from 0.0005
    than twice that bound), nothing written outside scores and flags."""
    B, D, ns, nc, ld = shape
    c = sc.head_case(*shape)
    want_s, want_f, _ = sc.head_reference(c["cos"], c["w"], ns)
    bound = sc.cosine_bound(D)
    assert float(np.abs(want_s - 0.0005).min()) > 2 * bound
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows = ns + nc
    sbuf = torch.full((2 * GUARD + B * rows,), -7.0, device=dev)
    fbuf = torch.full((2 * GUARD + B * 2,), -7, device=dev, dtype=torch.int32)
    e = t(c["e"])
    scores, flags = ops.safety_head(e[:, :D], t(c["special"]) if ns else None, t(c["special_w"]) if ns else None,
                                    t(c["concepts"]), t(c["concept_w"]), scores=sbuf[GUARD:GUARD + B * rows].view(B, rows),
                                    flags=fbuf[GUARD:GUARD + 2 * B].view(B, 2))
    torch.cuda.synchronize()
    err = float(np.abs(scores.cpu().numpy().astype(np.float64) - want_s).max())
    gate(f"safety_head scores B={B} D={D} rows={ns}+{nc} ld={ld}", err, bound)
    np.testing.assert_array_equal(flags.cpu().numpy(), want_f)
    assert bool((sbuf[:GUARD] == -7).all()) and bool((sbuf[GUARD + B * rows:] == -7).all())
    assert bool((fbuf[:GUARD] == -7).all()) and bool((fbuf[GUARD + 2 * B:] == -7).all())


def test_head_without_special_rows_takes_null(dev):
    c = sc.head_case(3, 36, 0, 1, 36)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    _, flags = ops.safety_head(t(c["e"]), None, None, t(c["concepts"]), t(c["concept_w"]))
    np.testing.assert_array_equal(flags.cpu().numpy(), sc.head_reference(c["cos"], c["w"], 0)[1])
    assert not bool(flags[:, 1].any())


# ---------------------------------------------------------------------------------------------
# blanking
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image_bytes", [1, 35, 4099, 64 * 64 * 3])
def test_blank_flagged(dev, image_bytes):
    """N = 4 images at a base offset of 0, 1 and 15 bytes, flags none / all / alternating at stride 1 and 2: flagged images
    all zero, the others and the guard bytes on both sides bit-identical."""
    N = 4
    g = torch.Generator().manual_seed(image_bytes)
    src = torch.randint(1, 256, (2 * GUARD + 15 + N * image_bytes,), generator=g, dtype=torch.uint8).to(dev)
    for off in (0, 1, 15):
        for pattern in ((0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 7, 0), (0, -1, 0, 1)):
            for stride in (1, 2):
                buf = src.clone()
                assert buf.data_ptr() % 16 == 0
                lo = GUARD + off
                images = buf[lo:lo + N * image_bytes].view(N, image_bytes)
                store = torch.full((N, stride), 5, dtype=torch.int32)
                store[:, 0] = torch.tensor(pattern, dtype=torch.int32)
                flags = store.to(dev)[:, 0]
                assert ops.blank_flagged(images, flags) is images
                torch.cuda.synchronize()
                want = src.clone()
                for n, f in enumerate(pattern):
                    if f:
                        want[lo + n * image_bytes:lo + (n + 1) * image_bytes] = 0
                assert torch.equal(buf, want), (image_bytes, off, pattern, stride)


# ---------------------------------------------------------------------------------------------
# the processor
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [28, 224])
@pytest.mark.parametrize("hw", [(64, 64), (72, 80), (80, 72)])
def test_processor_against_transformers(dev, hw, s):
    from transformers import CLIPImageProcessor
    hf = CLIPImageProcessor(size={"shortest_edge": s}, crop_size={"height": s, "width": s})
    images = np.random.default_rng(hw[0] * 100 + s).integers(0, 256, (2,) + hw + (3,), dtype=np.uint8)
    want = hf(images=[im for im in images], return_tensors="pt")["pixel_values"]
    for src in (hf, default_processor_config(s)):
        got = DeviceClipProcessor(src).pixel_values(torch.from_numpy(images).to(dev))
        assert got.dtype == F32 and tuple(got.shape) == (2, 3, s, s)
        gate(f"DeviceClipProcessor {hw} -> {s}", float((got.cpu() - want).abs().max()), 1e-6)


# ---------------------------------------------------------------------------------------------
# the tower
# ---------------------------------------------------------------------------------------------
TINY = SafetyConfig(image_size=56, patch_size=14, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                    num_attention_heads=2, projection_dim=32)
LARGE2 = SafetyConfig(num_hidden_layers=2)              # ViT-L/14 geometry: 224^2, 257 tokens, 1024 wide, 16 heads, 768 out


def _hf_tower(cfg, seed):
    """transformers' module with seeded weights (its own initialisation with the matrices scaled by 3 and perturbed norms
    and biases, so that the embedding depends on the image: at the initialisation's own scale the class token hardly sees
    the patches), and the same weights under diffusers' key names."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    hf = CLIPVisionModelWithProjection(CLIPVisionConfig(
        image_size=cfg.image_size, patch_size=cfg.patch_size, hidden_size=cfg.hidden_size,
        intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, projection_dim=cfg.projection_dim)).eval()
    with torch.no_grad():
        for k, p in hf.named_parameters():
            if p.dim() >= 2 and "position" not in k:
                p.mul_(3.0)
            if "norm" in k:
                p.add_(0.1 * torch.randn_like(p))
            elif k.endswith("bias"):
                p.add_(0.02 * torch.randn_like(p))
    sd = {("vision_model." + k if k.startswith("vision_model.") else k): v for k, v in hf.state_dict().items()}
    sd["concept_embeds"], sd["special_care_embeds"] = torch.randn(17, cfg.projection_dim), torch.randn(3, cfg.projection_dim)
    sd["concept_embeds_weights"], sd["special_care_embeds_weights"] = torch.full((17,), 2.0), torch.full((3,), 2.0)
    return hf, sd


def _cosines(e, rows):
    n = lambda x: x / x.norm(dim=1, keepdim=True)
    return n(e.double()) @ n(rows.double()).T


# 3x the first measurement against transformers: rel-L2 of image_embeds 1.045e-3 (tiny) and 1.318e-3
# (large2), cosine error 5.47e-4 and 8.02e-5; DESIGN.md "Safety checker" records them
TOWER_GATES = {"tiny": (3.14e-3, 1.64e-3), "large2": (3.96e-3, 2.41e-4)}


@pytest.mark.parametrize("name,cfg,B", [("tiny", TINY, 3), ("large2", LARGE2, 2)])
def test_tower_against_transformers(dev, name, cfg, B):
    hf, sd = _hf_tower(cfg, seed=11)
    x = torch.randn(B, 3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(5)) * 1.2
    with torch.no_grad():
        want = hf(pixel_values=x).image_embeds
    m = HipSafetyChecker(cfg, sd, dev)
    got = m.embed(x.to(dev)).cpu()
    assert got.dtype == F32 and got.shape == want.shape
    rows = torch.randn(20, cfg.projection_dim, generator=torch.Generator().manual_seed(6))
    rel = float((got - want).norm() / want.norm())
    cos = float((_cosines(got, rows) - _cosines(want, rows)).abs().max())
    spread = float((_cosines(want, want) - torch.eye(B)).abs().max())
    print(f"[tower] {name}: rel-L2 {rel:.4e}, max |cos error| {cos:.4e}; largest |cos| between two images' embeddings "
          f"{spread:.3f}")
    assert spread < 0.95                                     # the embedding depends on the image
    gate(f"safety tower {name} image_embeds rel-L2", rel, TOWER_GATES[name][0])
    gate(f"safety tower {name} cosine against 20 rows", cos, TOWER_GATES[name][1])


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
def test_check_device_end_to_end_and_from_a_graph(dev):
    """N = 4 seeded uint8 images through processor, tower, head and blanking.  Concept 0 is image 0's own fp32 embedding and
    concept 1 image 2's, with the threshold 0.05 under that image's transformers cosine; every other threshold is 0.05 above
    the largest cosine of its row: images 0 and 2 are flagged, 1 and 3 are not, with 0.05 to spare."""
    from transformers import CLIPImageProcessor
    cfg, s = TINY, TINY.image_size
    hf, sd = _hf_tower(cfg, seed=21)
    images = np.random.default_rng(3).integers(0, 256, (4, 64, 64, 3), dtype=np.uint8)
    hfp = CLIPImageProcessor(size={"shortest_edge": s}, crop_size={"height": s, "width": s})
    with torch.no_grad():
        e = hf(pixel_values=hfp(images=[im for im in images], return_tensors="pt")["pixel_values"]).image_embeds
    sd["concept_embeds"][0], sd["concept_embeds"][1] = e[0], e[2]
    rows = torch.cat([sd["special_care_embeds"], sd["concept_embeds"]])
    cos = _cosines(e, rows).numpy()                                          # transformers' fp32 forward, cosines in fp64
    w = cos.max(axis=0) + 0.05
    w[3], w[4] = cos[0, 3] - 0.05, cos[2, 4] - 0.05
    sd["special_care_embeds_weights"], sd["concept_embeds_weights"] = torch.from_numpy(w[:3]).float(), torch.from_numpy(w[3:]).float()
    w32 = torch.cat([sd["special_care_embeds_weights"], sd["concept_embeds_weights"]]).numpy()
    _, want_flags, _ = sc.head_reference(cos, w32, 3)
    np.testing.assert_array_equal(want_flags, [[1, 0], [0, 0], [1, 0], [0, 0]])
    assert float(np.abs(cos - w32.astype(np.float64) - 0.0005).min()) > 0.04  # every decision has its 0.05 (less rounding)

    m = HipSafetyChecker(cfg, sd, dev, hfp)
    src = torch.from_numpy(images).to(dev)
    scores, flags = m.scores(m.processor.pixel_values(src))
    err = float(np.abs(scores.cpu().numpy().astype(np.float64) + w32.astype(np.float64) - cos).max())
    gate("check_device cosines against transformers fp32", err, 0.005)       # keeps the decisions from flipping
    work = src.clone()
    out, flags = m.check_device(work)
    assert out is work and flags.is_cuda and flags.dtype == torch.int32
    np.testing.assert_array_equal(flags.cpu().numpy(), want_flags)
    for n in range(4):
        assert torch.equal(out[n], torch.zeros_like(src[n]) if want_flags[n, 0] else src[n]), n
    assert bool(src[0].any()) and bool(src[2].any())

    static = src.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.check_device(src.clone())                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        g_out, g_flags = m.check_device(static)
    static.copy_(src)
    g_flags.fill_(-7)
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_out, out) and torch.equal(g_flags, flags)

    # the diffusers call surface: host arrays are blanked like the reference blanks them
    host = images.astype(np.float32) / 255
    got, has = m(host, m.processor.pixel_values(src))
    assert has == [True, False, True, False] and not got[0].any() and not got[2].any()
    assert np.array_equal(got[1], images[1].astype(np.float32) / 255)


# ---------------------------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------------------------
def test_sd_plugin_and_batch_entry(dev, monkeypatch):
    """generation.stable_diffusion_generate.run on synthetic SD1.5 (2 steps) with a synthetic checker of ViT-L/14 geometry:
    thresholds of -1 flag every image (cosines lie in [-1, 1]) -> a black image and nsfw_content_detected; thresholds of +1
    flag none -> the bytes of a run without a checker.  sd_generate_batch(decode="device") returns device flags."""
    sys.path.insert(0, os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    import models
    from fake_text import FakeTextEncoder, FakeTokenizer
    import generation.stable_diffusion_generate as g
    md = models.load_synthetic("sd15", device=dev, safety_checker=True)
    checker = md["safety_checker"]
    assert isinstance(checker, HipSafetyChecker) and md["safety_processor"] is checker.processor
    assert (checker.cfg.image_size, checker.cfg.patch_size, checker.cfg.hidden_size, len(checker.layers)) == (224, 14, 1024, 2)
    md.tokenizer, md.text_encoder = FakeTokenizer(), FakeTextEncoder(768)
    monkeypatch.setattr(models, "model_dict", md)
    monkeypatch.setattr(g, "num_total_steps", 2)
    seen = {}
    orig = g.sd_generate_batch

    def spy(sampler, texts, latents, *a, **k):
        seen["call"] = (sampler, texts, latents.clone(), a, dict(k))
        return orig(sampler, texts, latents, *a, **k)
    monkeypatch.setattr(g, "sd_generate_batch", spy)

    checker.special_w.fill_(1.0)
    checker.concept_w.fill_(1.0)
    kept = g.run("a cat", seed=7)
    assert kept.nsfw_content_detected is False and "safety_checker" in seen["call"][4]
    checker.concept_w.fill_(-1.0)
    black = g.run("a cat", seed=7)
    assert black.nsfw_content_detected is True and black.image.size == (512, 512) and not np.asarray(black.image).any()

    del md["safety_checker"], md["safety_processor"]
    plain = g.run("a cat", seed=7)
    assert "nsfw_content_detected" not in plain and "safety_checker" not in seen["call"][4]
    arr = np.asarray(plain.image)
    assert arr.std() > 0 and np.array_equal(arr, np.asarray(kept.image))

    sampler, texts, latents, a, k = seen["call"]
    k.pop("scheduler")                                       # every call makes its own PNDMScheduler, as run() does
    checker.concept_w.fill_(1.0)
    lat, images, flags = orig(sampler, texts, latents, *a, decode="device", safety_checker=checker, **k)
    assert images.is_cuda and flags.is_cuda and flags.dtype == torch.int32 and tuple(flags.shape) == (1, 2)
    assert not bool(flags.any()) and np.array_equal(images[0].cpu().numpy(), arr)
    lat2, images2 = orig(sampler, texts, latents, *a, decode="device", **k)
    assert torch.equal(images2, images) and torch.equal(lat2, lat)
    checker.concept_w.fill_(-1.0)
    _, images3, flags3 = orig(sampler, texts, latents, *a, safety_checker=checker, **k)
    assert isinstance(images3, np.ndarray) and not images3.any() and flags3.tolist() == [[1, 0]]
    with pytest.raises(ValueError):
        orig(sampler, texts, latents, *a, decode=False, safety_checker=checker, **k)
    with pytest.raises(TypeError):
        models.load_synthetic("sd15", device=dev, with_vae=False, safety_checker="yes")
