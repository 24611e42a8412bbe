"""Pillow-exact resizing on the GPU (csrc/resample.hip through ops.resample_u8) and its consumers: every case of
tests/resample_cases.py against PIL.Image.resize itself, bit for bit; the float forms against the torch expression on
Pillow's bytes, bit for bit; DeviceOwlProcessor against transformers' OwlViTImageProcessor; detect(), the refiner and the
generators' decode="device" against the host paths they replace."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lgd_amd  # noqa: E402,F401
import owl_detect_cases as owl_cases  # noqa: E402
import resample_cases as rc  # noqa: E402
from lgd_amd import ops, owlvit, weights  # noqa: E402
from lgd_amd.owl_processor import DeviceOwlProcessor  # noqa: E402

ALL = rc.CASES + rc.CONSUMER
IDS = [rc.case_id(c) for c in ALL]
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
POISON = 0x5A


def _mismatch(got, want):
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    bad = got != want
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} elements differ, the first at {tuple(np.argwhere(bad)[0])}"


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_u8_form_equals_pillow(dev, c):
    img, want = rc.expected(c)
    got = ops.resample_u8(torch.from_numpy(img.copy())[None].to(dev), c[1], c[2])
    _mismatch(got[0], want)


@pytest.mark.parametrize("c", rc.CASES, ids=IDS[:len(rc.CASES)])
def test_batch_of_three_different_images(dev, c):
    """One call for three images: a wrong batch stride of the input, the scratch or the output shows."""
    img, want = rc.expected(c, n=3)
    assert not np.array_equal(want[0], want[1])
    _mismatch(ops.resample_u8(torch.from_numpy(img.copy()).to(dev), c[1], c[2]), want)


@pytest.mark.parametrize("c", rc.CASES[::5], ids=IDS[:len(rc.CASES):5])
def test_operands_carved_out_at_the_minimum_alignment(dev, c):
    """The header asks no alignment of src, scratch and a uint8 out: each sits at an odd byte offset of a larger poisoned
    buffer, and the bytes around the output stay as they were."""
    (h, w), (H, W), f, _ = c
    img, want = rc.expected(c, n=3)
    n_in, n_mid, n_out = 3 * h * w * 3, 3 * h * W * 3, 3 * H * W * 3
    src = torch.full((n_in + 16,), POISON, device=dev, dtype=torch.uint8)
    mid = torch.full((n_mid + 16,), POISON, device=dev, dtype=torch.uint8)
    dst = torch.full((n_out + 16,), POISON, device=dev, dtype=torch.uint8)
    src[1:1 + n_in] = torch.from_numpy(img.copy()).to(dev).reshape(-1)
    out = dst[3:3 + n_out].view(3, H, W, 3)
    assert src[1:].data_ptr() % 2 == 1 and out.data_ptr() % 2 == 1 and mid[5:].data_ptr() % 2 == 1
    got = ops.resample_u8(src[1:1 + n_in].view(3, h, w, 3), (H, W), f, out=out, scratch=mid[5:5 + n_mid])
    assert got.data_ptr() == out.data_ptr()
    _mismatch(got, want)
    assert bool((dst[:3] == POISON).all()) and bool((dst[3 + n_out:] == POISON).all())
    assert bool((mid[:5] == POISON).all()) and bool((mid[5 + n_mid:] == POISON).all())
    # a float output at the minimum alignment of its element: 2 bytes for fp16, 4 for fp32
    for dtype, size in ((torch.float16, 2), (torch.float32, 4)):
        buf = torch.zeros((n_out + 8,), device=dev, dtype=dtype)
        o = buf[1:1 + n_out].view(3, 3, H, W)
        assert o.data_ptr() % (2 * size) == size
        got = ops.resample_u8(src[1:1 + n_in].view(3, h, w, 3), (H, W), f, "unit", dtype=dtype, out=o)
        assert torch.equal(got, _unit(torch.from_numpy(want.copy()).to(dev), dtype))
        assert float(buf[0]) == 0 and bool((buf[1 + n_out:] == 0).all())


def _affine(u8, dtype):
    """The torch expression of form "affine" on a uint8 (N, H, W, 3) device batch, in the contract's operation order."""
    v = u8.permute(0, 3, 1, 2).float()
    m = torch.tensor(MEAN, device=u8.device, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(STD, device=u8.device, dtype=torch.float32).view(1, 3, 1, 1)
    return ((v * (1 / 255) - m) / s).to(dtype).contiguous()


def _unit(u8, dtype):
    """The torch expression of form "unit", v / 255 * 2 - 1 with a true division, as the host computes it for the refiner
    today.  The divisor is a device tensor: torch's GPU kernel for a Python-scalar divisor multiplies by the fp32
    reciprocal instead (one rounding more), which is another expression."""
    d = torch.tensor(255.0, device=u8.device, dtype=torch.float32)
    return (u8.permute(0, 3, 1, 2).float() / d * 2.0 - 1.0).to(dtype).contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("c", rc.CASES[::5] + rc.CONSUMER, ids=IDS[:len(rc.CASES):5] + IDS[-2:])
def test_float_forms_equal_the_torch_expression_on_pillows_bytes(dev, c, dtype):
    img, want = rc.expected(c, n=None)
    x = torch.from_numpy(img.copy())[None].to(dev)
    pil = torch.from_numpy(want.copy())[None].to(dev)
    got = ops.resample_u8(x, c[1], c[2], "affine", dtype=dtype, rescale=1 / 255, mean=MEAN, std=STD)
    assert got.dtype == dtype and tuple(got.shape) == (1, 3) + tuple(c[1])
    assert torch.equal(got, _affine(pil, dtype)), "affine"
    got = ops.resample_u8(x, c[1], c[2], "unit", dtype=dtype)
    assert torch.equal(got, _unit(pil, dtype)), "unit"


def test_forms_on_an_image_that_keeps_its_size(dev):
    """Neither pass runs: the form is applied to the bytes themselves (what the refiner does with resize=None)."""
    x = torch.from_numpy(rc.image((12, 20), "random", n=2).copy()).to(dev)
    assert torch.equal(ops.resample_u8(x, (12, 20), "lanczos"), x)
    assert torch.equal(ops.resample_u8(x, (12, 20), "bicubic", "unit"), _unit(x, torch.float32))
    assert torch.equal(ops.resample_u8(x, (12, 20), "bilinear", "affine", dtype=torch.float16, mean=MEAN, std=STD),
                       _affine(x, torch.float16))


def test_eager_and_captured_graph_bit_identical(dev):
    """Every small case in all three forms, launched eagerly and inside ONE captured graph (the tables are resident after
    the warm-up, so the capture holds kernels only): identical bits."""
    ins = {c: torch.from_numpy(rc.expected(c)[0].copy())[None].to(dev) for c in rc.CASES}

    def buffers():
        return {(c, form): torch.empty((1,) + tuple(c[1]) + (3,) if form == "u8" else (1, 3) + tuple(c[1]), device=dev,
                                       dtype=torch.uint8 if form == "u8" else torch.float16 if form == "unit" else torch.float32)
                for c in rc.CASES for form in ops.RESAMPLE_FORMS}
    scratch = {c: torch.empty((c[0][0] * c[1][1] * 3,), device=dev, dtype=torch.uint8) for c in rc.CASES}

    def launch(bufs):
        for (c, form), out in bufs.items():
            ops.resample_u8(ins[c], c[1], c[2], form, dtype=out.dtype, mean=MEAN, std=STD, out=out, scratch=scratch[c])
    eager, graphed = buffers(), buffers()
    launch(eager)
    cg = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch(buffers())                                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(cg):
        launch(graphed)
    cg.replay()
    torch.cuda.synchronize()
    for key in eager:
        assert torch.equal(eager[key], graphed[key]), key
    for c in rc.CASES:
        _mismatch(graphed[(c, "u8")][0], rc.expected(c)[1])


def test_stream_argument(dev):
    c = rc.CASES[0]
    img, want = rc.expected(c)
    x = torch.from_numpy(img.copy())[None].to(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    got = ops.resample_u8(x, c[1], c[2], stream=s)
    s.synchronize()
    _mismatch(got[0], want)


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator
# ---------------------------------------------------------------------------------------------------------------------
def test_device_owl_processor_against_transformers(dev):
    """The installed OwlViTImageProcessor (768 x 768, BICUBIC, CLIP normalisation) on the same image: the uint8 stage is
    Pillow's exactly; pixel_values within 1e-6 absolute — four fp32 ulps at |v| <= 2.3, the fp32 formula against the
    processor measured 4.8e-7 on the host."""
    transformers = pytest.importorskip("transformers")
    hf = transformers.OwlViTImageProcessor()
    c = rc.CONSUMER[0]
    img, want = rc.expected(c)
    from PIL import Image
    ref = hf(images=Image.fromarray(img), return_tensors="pt")["pixel_values"]
    proc = DeviceOwlProcessor(hf)
    x = torch.from_numpy(img.copy())[None].to(dev)
    _mismatch(proc.resized(x)[0], want)
    pv = proc.pixel_values(x)
    assert pv.dtype == torch.float32 and tuple(pv.shape) == tuple(ref.shape) == (1, 3, 768, 768)
    err = float((pv.cpu() - ref).abs().max())
    print(f"[DeviceOwlProcessor] pixel_values against OwlViTImageProcessor: max abs {err:.3e}, |v| <= {float(ref.abs().max()):.3f}")
    assert err <= 1e-6


class _StubProcessor:
    """Stands in for OwlViTProcessor: a real image-processor configuration at the tiny detector's input size, fixed id rows
    for whatever text it is given."""

    def __init__(self, image_processor, ids):
        self.image_processor, self.ids = image_processor, ids

    def __call__(self, text=None, images=None, return_tensors="pt"):
        assert images is None, "the pixels must not come through the processor"
        n = len(text[0])
        return {"input_ids": self.ids[:n], "attention_mask": (self.ids[:n] > 0).long()}


def _dropin_eval():
    path = os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin", "utils", "eval", "eval.py")
    spec = importlib.util.spec_from_file_location("lgd_dropin_utils_eval_eval_resample", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_detect_fed_by_the_device_processor(dev):
    """The tiny synthetic detector of tests/test_owl_detect_gpu.py (96 x 96 input): detect() on DeviceOwlProcessor's
    pixel_values against detect() on the torch expression applied to Pillow's bytes — identical outputs; and
    eval_device_images builds the det_boxes of that path."""
    transformers = pytest.importorskip("transformers")
    cfg = owl_cases.tiny_hf_config()
    torch.manual_seed(0)
    hf = owl_cases.redraw_weights(transformers.OwlViTForObjectDetection(cfg), seed=3).to(dev)
    det = owlvit.from_hf(hf, dev)
    Q = 3
    _, ids = owl_cases.model_inputs(cfg, 2, Q, seed=4)
    ip = transformers.OwlViTImageProcessor(size={"height": 96, "width": 96})
    proc = DeviceOwlProcessor(_StubProcessor(ip, ids[:Q]))
    imgs = rc.image((40, 56), "random", seed=3, n=2)
    x = torch.from_numpy(imgs.copy()).to(dev)
    pil = torch.from_numpy(np.stack([rc.pil_resize(i, (96, 96), "bicubic") for i in imgs])).to(dev)
    pv = proc.pixel_values(x)
    assert torch.equal(pv, _affine(pil, torch.float32))
    kw = dict(score_threshold=0.2, nms_threshold=0.4)
    ids2 = torch.cat([ids[:Q], ids[:Q]])
    got, want = det.detect(pv, ids2, **kw), det.detect(_affine(pil, torch.float32), ids2, **kw)
    assert got.counts == want.counts and sum(got.counts) > 0
    for a, b in zip((got.boxes, got.scores, got.labels, got.index), (want.boxes, want.scores, want.labels, want.index)):
        assert torch.equal(a, b)
    ev = _dropin_eval()
    names = [f"a photo of thing {i}" for i in range(Q)]
    for p in (proc, proc.processor):                          # the device processor, or the processor it is built from
        two = ev.eval_device_images(det, p, x, [names, names[:Q - 1]], **kw)
        d = det.detect(_affine(pil, torch.float32), torch.cat([ids[:Q], ids[:Q - 1], torch.zeros_like(ids[:1])]), **kw)
        for b in range(2):
            boxes, scores, labels = (t.cpu().numpy() for t in d.image(b))
            want_boxes = [{"name": names[l], "bounding_box": ev.to_gen_box_format(bx, 56, 40), "score": sc}
                          for bx, sc, l in zip(boxes, scores, labels)]
            assert len(two[b]) == len(want_boxes)
            for u, v in zip(two[b], want_boxes):
                assert u["name"] == v["name"] and u["score"] == v["score"] and u["bounding_box"] == v["bounding_box"]
        assert sum(len(t) for t in two) > 0
    with pytest.raises(TypeError):
        ev.eval_device_images(det, proc, imgs, [names, names])             # host pixels: that is eval_images' job
    with pytest.raises(ValueError):
        ev.eval_device_images(det, proc, x, [names])


# ---------------------------------------------------------------------------------------------------------------------
# the refiner and the generators
# ---------------------------------------------------------------------------------------------------------------------
def _rnd(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def test_refine_from_a_device_image(dev, monkeypatch):
    """The tiny synthetic refiner of tests/test_sdxl_gpu.py: refine(device uint8, resize=S) equals refine(the Pillow-LANCZOS
    resized numpy image) with the same seed, bit for bit; output="device" is the uint8 return left on the GPU; the drop-in
    module takes the same path for a device tensor."""
    from PIL import Image
    from lgd_amd import sdxl
    cfg = weights.CONFIGS["tiny_xl"]
    ref, _ = sdxl.build_synthetic("tiny_xl", dev, seed=0, vae_ch=(32, 32, 32, 32), vae_layers=1)
    pe, pooled = _rnd(2, 77, cfg.cross_attention_dim, seed=8), _rnd(2, cfg.pooled_dim, seed=9)
    img = rc.image((96, 96), "random", seed=5)
    S = 256
    resized = np.asarray(Image.fromarray(img).resize((S, S), Image.LANCZOS))
    kw = dict(seed=11, strength=0.5, num_inference_steps=4)
    x = torch.from_numpy(img.copy()).to(dev)
    lat_host = ref.refine(resized, pe, pooled, output="latent", **kw)
    lat_dev = ref.refine(x, pe, pooled, output="latent", resize=S, **kw)
    assert torch.equal(lat_dev, lat_host)
    want = ref.refine(resized, pe, pooled, **kw)
    got = ref.refine(x, pe, pooled, resize=S, **kw)
    assert isinstance(got, np.ndarray) and got.shape == (S, S, 3) and np.array_equal(got, want)
    on_dev = ref.refine(x, pe, pooled, resize=S, output="device", **kw)
    assert torch.is_tensor(on_dev) and on_dev.is_cuda and on_dev.dtype == torch.uint8 and on_dev.is_contiguous()
    _mismatch(on_dev, want)
    # a device image of the final size: no pass runs, the bytes go through the same form
    assert np.array_equal(ref.refine(torch.from_numpy(resized.copy()).to(dev), pe, pooled, **kw), want)
    with pytest.raises(ValueError):
        ref.refine(resized, pe, pooled, resize=S, **kw)
    with pytest.raises(ValueError):
        ref.refine(x[None], pe, pooled, resize=S, **kw)
    # the drop-in module
    sys.path.insert(0, os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    import generation.sdxl_refinement as mod
    monkeypatch.setattr(mod, "pipe", ref)
    monkeypatch.setattr(mod, "REFINE_SIZE", S)               # the module's own constant is 1024: the same path, 16 x cheaper
    spec = dict(prompt="a photo", extra_neg_prompt="bad", sdxl_prompt_embeds=pe, sdxl_pooled=pooled)
    host = mod.refine(img, spec, refine_seed=5, refinement_step_ratio=0.1)
    from_dev = mod.refine(x, spec, refine_seed=5, refinement_step_ratio=0.1)
    assert isinstance(from_dev, Image.Image) and from_dev.size == (mod.REFINE_SIZE,) * 2
    assert np.array_equal(np.asarray(from_dev), np.asarray(host))
    left = mod.refine_device(x, spec, refine_seed=5, refinement_step_ratio=0.1)
    assert torch.is_tensor(left) and left.is_cuda
    _mismatch(left, np.asarray(host))


def test_decode_device_returns_the_bytes_of_decode_true(dev):
    from lgd_amd.pipeline import CachedLayout, lmd_generate_batch, lmd_plus_generate_batch, sd_generate_batch
    from lgd_amd.sampler import LMDSampler
    from lgd_amd.scheduler import DDIMScheduler
    from lgd_amd.unet import UNetEngine
    from lgd_amd.vae import make_hip_vae
    L = 32
    vae = make_hip_vae(dev)
    boxes = [("a white deer", [74, 177, 183, 235]), ("a gray bear", [314, 193, 189, 216])]

    def both(run):
        host, left = run(True), run("device")
        for a, b in zip(host, left):
            assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape[-3:] == (8 * L, 8 * L, 3)
            assert torch.is_tensor(b) and b.is_cuda and b.dtype == torch.uint8
            _mismatch(b, a)
    cfg = weights.CONFIGS["tiny_gligen"]
    sm = LMDSampler(UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0)), DDIMScheduler(), vae=vae)
    lays = [CachedLayout.synthetic(cfg, boxes, 3), CachedLayout.synthetic(cfg, boxes[:1], 5)]
    kw = dict(num_inference_steps=4, height=8 * L, width=8 * L, overall_loss_threshold=0.0, overall_max_index_step=2,
              overall_max_iter=[1])
    both(lambda d: [r["image"] for r in lmd_plus_generate_batch(sm, lays, decode=d, **kw)])
    cfg = weights.CONFIGS["tiny"]
    sm = LMDSampler(UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0)), DDIMScheduler(), vae=vae)
    lays = [CachedLayout.synthetic(cfg, boxes, 3)]
    both(lambda d: [r["image"] for r in lmd_generate_batch(sm, lays, decode=d, loss_threshold=0.0, max_index_step=1,
                                                           max_iter=[1], **kw)])
    unc, cond = weights.synth_embeddings(cfg, 1, seed=10)
    lat = _rnd(2, 4, L, L, seed=9)
    both(lambda d: sd_generate_batch(sm, [torch.cat([unc, cond])] * 2, lat, 2, decode=d)[1])
    with pytest.raises(ValueError):
        sd_generate_batch(sm, [torch.cat([unc, cond])] * 2, lat, 2, decode="host")
