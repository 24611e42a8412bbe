"""DeviceSamProcessor(resize="pillow") on the GPU: SAM's input as the Hugging Face SamImageProcessor computes it (Pillow
BILINEAR, 1/255, mean / std, zero padding) from ONE ops.resample_u8 call, and the refiner on top of it.

Measured on an MI355X (the synthetic refine model of tests/sam_cases.py; tests/golden/sam_refine.npz = the reference's own
models/sam.py with the Hugging Face processor): pixel_values against SamImageProcessor 7.2e-7 at most and bit for bit the
torch expression on Pillow's bytes; worst mask agreement of the golden replay (per-image calls through the drop-in
module) 0.9729 with resize="pillow" — the HIP model under the Hugging Face processor itself measures 0.973
(tests/test_sam_gpu.py) — and 0.9443 with resize="torch" (box 1; printed for the record, not gated: that processor is not
this file's subject).  Batched against per-image: every item alone through boxes() / attns() equals box() / attn() pixel
for pixel; inside one call of four, item 1 of boxes() agrees 0.9890 and the other seven items 1.0000 (the encoder's GEMM
tiles follow the batch size, tests/test_sam_batched_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lgd_amd  # noqa: E402,F401
import resample_cases as rc  # noqa: E402
import sam_cases  # noqa: E402
import sam_refine_checks  # noqa: E402
from lgd_amd import sam_refine  # noqa: E402

MIN_AGREE, CONF_TOL = 0.95, 3e-2                                  # the limits of the golden replay on the HIP model
TARGET = 1024


def _torch_expression(img, target=TARGET):
    """uint8 (h, w, 3) on the host -> what resize="pillow" must give for it, fp32 (3, target, target) on the host: the
    affine form (tests/test_resample_gpu.py's expression, the divisor a tensor) on Pillow's own bytes in a zero canvas."""
    nh, nw = sam_refine.DeviceSamProcessor("cpu", longest_edge=target)._shape(*img.shape[:2])
    v = torch.from_numpy(rc.pil_resize(img, (nh, nw), "bilinear").copy()).permute(2, 0, 1).float()
    m = torch.tensor(sam_refine.DeviceSamProcessor.MEAN, dtype=torch.float32).view(3, 1, 1)
    s = torch.tensor(sam_refine.DeviceSamProcessor.STD, dtype=torch.float32).view(3, 1, 1)
    out = torch.zeros(3, target, target)
    out[:, :nh, :nw] = (v * (1 / 255) - m) / s
    return out, [nh, nw]


def _hf(transformers, imgs):
    from PIL import Image
    return transformers.SamImageProcessor()(images=[Image.fromarray(i) for i in imgs], return_tensors="pt")


def test_pixel_values_against_hugging_face_and_pillows_bytes(dev):
    transformers = pytest.importorskip("transformers")
    proc = sam_refine.DeviceSamProcessor(dev, resize="pillow")
    square = rc.image((512, 512), "random", seed=1, n=3)
    small = rc.image((96, 64), "random", seed=1)
    for name, imgs, fed in (("512x512 x 3, a device tensor", list(square), torch.from_numpy(square.copy()).to(dev)),
                            ("96x64, a host array", [small], small)):
        px, orig, resh = proc.pixels(fed)
        assert px.is_cuda and px.dtype == torch.float32 and tuple(px.shape) == (len(imgs), 3, TARGET, TARGET)
        want = _hf(transformers, imgs)
        assert resh == want["reshaped_input_sizes"].tolist() and orig == want["original_sizes"].tolist()
        err = float((px.cpu() - want["pixel_values"]).abs().max())
        print(f"[sam pillow] {name}: pixel_values against SamImageProcessor max abs {err:.3e}")
        assert err <= 1e-6
        for n, img in enumerate(imgs):
            exact, shape = _torch_expression(img)
            assert shape == resh[n]
            assert torch.equal(px[n].cpu(), exact), (name, n)
            nh, nw = shape
            assert not bool(px[n, :, nh:, :].any()) and not bool(px[n, :, :, nw:].any())
    assert resh == [[1024, 683]]
    # a list of mixed sizes: one call per image, each its own canvas
    mixed = [square[0], small, rc.image((40, 100), "random", seed=3), torch.from_numpy(square[1].copy()).to(dev)]
    px, orig, resh = proc.pixels(mixed)
    assert tuple(px.shape) == (4, 3, TARGET, TARGET) and orig == [[512, 512], [96, 64], [40, 100], [512, 512]]
    for n, img in enumerate([square[0], small, mixed[2], square[1]]):
        exact, shape = _torch_expression(img)
        assert shape == resh[n] and torch.equal(px[n].cpu(), exact), n
    # the whole processor call: the same tensors and the prompt scaling of the Hugging Face processor
    hfp = transformers.SamProcessor(transformers.SamImageProcessor())
    bx = [[[10.0, 20.0, 60.0, 90.0]]]
    got, want = proc([small], input_boxes=bx), hfp([small], input_boxes=bx, return_tensors="pt")
    assert float((got["pixel_values"].cpu() - want["pixel_values"]).abs().max()) <= 1e-6
    assert torch.equal(got["reshaped_input_sizes"], want["reshaped_input_sizes"].long())
    assert torch.allclose(got["input_boxes"], want["input_boxes"].double())


@pytest.fixture(scope="module")
def dicts(dev):
    """ONE HIP model under the three processors: "device" (today's), a default-constructed one, "device-pillow"."""
    transformers = pytest.importorskip("transformers")
    hf = sam_cases.build_refine_hf(transformers)
    md = sam_refine.wrap_sam(hf, "device", device=dev)
    pil = sam_refine.wrap_sam(hf, "device-pillow", device=dev)
    assert md["sam_processor"].resize == "torch" and pil["sam_processor"].resize == "pillow" and pil["sam_processor"].on_device
    return dict(torch=md, default=dict(sam_model=md["sam_model"], sam_processor=sam_refine.DeviceSamProcessor(dev)),
                pillow=dict(sam_model=md["sam_model"], sam_processor=pil["sam_processor"]))


def _refiner(sam_dict, **kw):
    k = sam_refine_checks.KW
    return sam_refine.SamRefiner(sam_dict, height=k["height"], width=k["width"],
                                 discourage_mask_below_confidence=k["discourage_mask_below_confidence"],
                                 discourage_mask_below_coarse_iou=k["discourage_mask_below_coarse_iou"],
                                 use_box_input=False, gaussian_sigma=1.5, mask_th_for_point=0.25, **kw)


def _pairs():
    images, boxes, attn = sam_cases.refine_inputs()
    owner = [ii for ii, per_image in enumerate(boxes) for _ in per_image]
    return np.stack([images[ii] for ii in owner]), [b for per_image in boxes for b in per_image], attn


@pytest.mark.parametrize("kind", ["box", "attn"])
def test_batched_equals_per_image_item_by_item(dicts, dev, kind):
    """Over the "pillow" processor both paths feed the model the same pixels (one resample call per item or per batch,
    the result per image independent of what it shares the call with), and the tail is the host chain pixel for pixel
    (tests/test_sam_tail_gpu.py): item n of boxes() / attns() is box() / attn() of item n, masks pixel for pixel.  Each
    item goes through the batched entry on its own so that the network runs the same GEMM tiles as the per-image call.
    Across batch sizes the encoder's tile choice differs and bit equality is not expected: the call with all four items
    is held to the gate of tests/test_sam_batched_gpu.py (0.95 / 3e-2) and its agreement is printed (measured 0.9890 on
    item 1 of boxes(), 1.0000 on every other item)."""
    stack, flat_boxes, attn = _pairs()
    batched, single = _refiner(dicts["pillow"]), _refiner(dicts["pillow"], batched=False)
    assert batched.batched and not single.batched
    x = torch.from_numpy(stack).to(dev)
    if kind == "box":
        all_m, all_c = batched.boxes(x, flat_boxes)
    else:
        all_m, all_c = batched.attns(x, attn)
    assert all_m.is_cuda and all_m.dtype == torch.bool and tuple(all_m.shape) == (4, 64, 64) and tuple(all_c.shape) == (4,)
    for n in range(4):
        if kind == "box":
            m, c = batched.boxes(x[n:n + 1], flat_boxes[n:n + 1])
            wm, wc = single.box(stack[n], flat_boxes[n])
        else:
            m, c = batched.attns(x[n:n + 1], attn[n:n + 1])
            wm, wc = single.attn(stack[n], attn[n])
        agree = float((m[0].cpu().numpy() == np.asarray(wm).astype(bool)).mean())
        agree4 = float((all_m[n].cpu().numpy() == np.asarray(wm).astype(bool)).mean())
        print(f"[sam pillow] {kind} item {n}: agreement with the per-image call {agree:.4f} (in the batch of four {agree4:.4f}), "
              f"confidence {float(c[0]):.6f} / {float(all_c[n]):.6f} against {float(wc):.6f}")
        assert np.array_equal(m[0].cpu().numpy(), np.asarray(wm).astype(bool)), (kind, n, agree)
        assert abs(float(c[0]) - float(wc)) <= 1e-6, (kind, n)
        assert agree4 >= MIN_AGREE and abs(float(all_c[n]) - float(wc)) <= CONF_TOL, (kind, n, agree4)


def test_golden_replay_with_both_processors(dicts, monkeypatch):
    """tests/golden/sam_refine.npz through tests/sam_refine_checks.py at the limits tests/test_sam_gpu.py holds the HIP
    model to (0.95 / 3e-2) for resize="pillow".  The same replay with resize="torch" is measured and printed only (the
    replay's own assertions switched off: 0.9443 on box 1, below that limit)."""
    monkeypatch.syspath_prepend(os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    from models import sam as dsam
    worst = sam_refine_checks.replay(dsam, dicts["pillow"], min_agree=MIN_AGREE, conf_tol=CONF_TOL)
    print(f"[sam pillow] golden replay, resize='pillow': worst mask agreement {worst:.4f}")
    assert worst >= MIN_AGREE
    record = sam_refine_checks.replay(dsam, dicts["torch"], min_agree=0.0, conf_tol=float("inf"))
    print(f"[sam pillow] golden replay, resize='torch' (not gated): worst mask agreement {record:.4f}")


def test_batched_call_against_the_golden(dicts, dev):
    """One boxes() and one attns() call over the "pillow" processor against what the reference selected, with the gate of
    tests/test_sam_batched_gpu.py."""
    g = np.load(sam_refine_checks.GOLD)
    stack, flat_boxes, attn = _pairs()
    r = _refiner(dicts["pillow"])
    x = torch.from_numpy(stack).to(dev)
    for kind, (m, c) in (("box", r.boxes(x, flat_boxes)), ("attn", r.attns(x, attn))):
        for n in range(4):
            agree = float((m[n].cpu().numpy() == g[f"{kind}{n}_mask"].astype(bool)).mean())
            print(f"[sam pillow] {kind}s() item {n} against the golden: agreement {agree:.4f}, confidence {float(c[n]):.4f} "
                  f"against {float(g[f'{kind}{n}_conf']):.4f}")
            assert agree >= MIN_AGREE and abs(float(c[n]) - float(g[f"{kind}{n}_conf"])) <= CONF_TOL, (kind, n)


def test_defaults_unchanged(dicts, dev):
    """resize="torch", the default constructor and wrap_sam(..., "device") are one processor: the same pixels and the same
    boxes() bits; the "pillow" processor's pixels are others (it is an opt-in, not a silent change)."""
    stack, flat_boxes, _ = _pairs()
    x = torch.from_numpy(stack).to(dev)
    explicit = sam_refine.DeviceSamProcessor(dev, resize="torch")
    a, b, c = (p.pixels(x)[0] for p in (dicts["torch"]["sam_processor"], dicts["default"]["sam_processor"], explicit))
    assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(a, dicts["pillow"]["sam_processor"].pixels(x)[0])
    m0, c0 = _refiner(dicts["torch"]).boxes(x, flat_boxes)
    m1, c1 = _refiner(dicts["default"]).boxes(x, flat_boxes)
    assert torch.equal(m0, m1) and torch.equal(c0, c1)
