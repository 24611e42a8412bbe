"""CPU suite for the batched mask refinement: the two exports of csrc/sam_tail.hip are declared alike in the header and the
binding, `SamRefiner.batched` resolves from the processor, and the device processor treats a stacked batch exactly as it
treats its images one by one."""
import os
import re

import numpy as np
import pytest
import torch

import lgd_amd  # noqa: F401
import sam_cases
from lgd_amd import _lib, sam_refine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_both_symbols_are_declared_and_bound_with_matching_argument_counts():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgd_hip.h")).read(), flags=re.S)
    for name, nargs in (("lgd_sam_mask_tail_f32", 20), ("lgd_sam_attn_prompt_f32", 12)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs == len(_lib.SIGNATURES[name]), name
    assert os.path.exists(os.path.join(ROOT, "llm-groundeddiffusion_amd", "csrc", "sam_tail.hip"))


class _HostProcessor:
    """Stands for the Hugging Face processor: no `on_device`."""


def test_batched_resolves_from_the_processor():
    device = dict(sam_model=None, sam_processor=sam_refine.DeviceSamProcessor("cpu"))
    host = dict(sam_model=None, sam_processor=_HostProcessor())
    assert sam_refine.SamRefiner(device).batched is True
    assert sam_refine.SamRefiner(device, batched=False).batched is False
    assert sam_refine.SamRefiner(device, batched=True).batched is True
    assert sam_refine.SamRefiner(host).batched is False
    assert sam_refine.SamRefiner(host, batched=False).batched is False
    with pytest.raises(ValueError):
        sam_refine.SamRefiner(host, batched=True)
    # the attention map's box prompt needs an erosion, which is host code: `attns` refuses it and the pipeline calls
    # `attn` per box, while the same refiner's `boxes` stays batched
    from lgd_amd import pipeline
    r = sam_refine.SamRefiner(device, use_box_input=True)
    assert r.batched is True and pipeline._batched(r, "box") and not pipeline._batched(r, "attn")
    with pytest.raises(NotImplementedError):
        r.attns(np.zeros((1, 64, 64, 3), np.uint8), [np.zeros((8, 8), np.float32)])
    plain = sam_refine.SamRefiner(device)
    assert pipeline._batched(plain, "box") and pipeline._batched(plain, "attn")
    assert not pipeline._batched(None, "box") and not pipeline._batched(sam_refine.SamRefiner(host), "attn")
    with pytest.raises(RuntimeError):
        sam_refine.SamRefiner(host, batched=False).boxes(np.zeros((1, 64, 64, 3), np.uint8), [(0.1, 0.1, 0.9, 0.9)])


@pytest.mark.parametrize("size", [(512, 512), (96, 64), (1200, 900)])
def test_processor_on_a_stacked_batch_equals_its_per_image_results(size):
    """Up-scaling (512 -> 1024), a padded side (96 x 64 -> 1024 x 683) and anti-aliased down-scaling (1200 -> 1024)."""
    proc = sam_refine.DeviceSamProcessor("cpu")
    g = torch.Generator().manual_seed(3)
    batch = torch.randint(0, 256, (3, *size, 3), generator=g, dtype=torch.uint8)
    if size == (512, 512):
        batch[:2] = torch.from_numpy(np.stack(sam_cases.refine_inputs()[0]))
    boxes = [[[10.0, 20.0, 50.0, 60.0]]] * 3
    one = [proc(batch[i].numpy(), input_boxes=[boxes[i]]) for i in range(3)]
    for images in (batch, batch.numpy(), [b.numpy() for b in batch], list(batch)):
        enc = proc(images, input_boxes=boxes)
        assert enc["pixel_values"].shape == (3, 3, 1024, 1024)
        for i in range(3):
            assert torch.equal(enc["pixel_values"][i], one[i]["pixel_values"][0])
            assert torch.equal(enc["input_boxes"][i], one[i]["input_boxes"][0])
        assert torch.equal(enc["original_sizes"], torch.cat([o["original_sizes"] for o in one]))
        assert torch.equal(enc["reshaped_input_sizes"], torch.cat([o["reshaped_input_sizes"] for o in one]))
    px, orig, resh = proc.pixels(batch)
    assert torch.equal(px, enc["pixel_values"]) and orig == [list(size)] * 3 and resh == enc["reshaped_input_sizes"].tolist()
    mixed = proc([batch[0].numpy(), batch[1, :40].numpy()])
    assert mixed["original_sizes"].tolist() == [list(size), [40, size[1]]]
    assert torch.equal(mixed["pixel_values"][0], one[0]["pixel_values"][0])


def test_batched_calls_equal_the_per_image_calls_with_host_stand_ins_for_the_two_kernels(monkeypatch):
    """Everything of boxes() / attns() except the kernels themselves, without a GPU: the network runs through the torch
    restatement of its kernels in fp32 (tests/ops_emul.py, as tests/test_sam_refine_host.py does), and the two ops of
    csrc/sam_tail.hip are replaced by the host code they restate (tests/sam_tail_cases.py, scipy).  Then one call for
    the four pairs of refine_inputs(), in model chunks of 3 + 1, gives the masks of box() / attn() pixel for pixel: the
    prompt scaling, the coarse masks, the geometry rows and the chunking are right, and each item meets its own IoU row.
    (The kernels against that host code: tests/test_sam_tail_gpu.py.)"""
    transformers = pytest.importorskip("transformers")
    from scipy import ndimage
    import ops_emul
    import sam_tail_cases as tc
    from lgd_amd import ops, sam as lsam, vit

    def host_tail(logits, iou, geom, target, grid, coarse, below_conf, below_iou, want_cand=True):
        picked = [tc.host_select(tc.host_candidates(logits[n], geom[n].tolist(), target, grid), iou[n].numpy(),
                                 coarse[n].numpy(), below_conf, below_iou) for n in range(logits.shape[0])]
        return (torch.from_numpy(np.stack([p["mask"] for p in picked]).astype(np.uint8)),
                torch.tensor([float(p["conf"]) for p in picked]), None, None)

    def host_prompt(attn, sigma, mask_th, up_w, up_h, want_smooth=False):
        smooth = [ndimage.gaussian_filter(a.astype(float), sigma=sigma) for a in attn.numpy()]
        peaks = [np.unravel_index(s.argmax(), s.shape) for s in smooth]
        return (torch.from_numpy(np.stack([sam_refine.preprocess_mask(s, mask_th) for s in smooth]).astype(np.uint8)),
                torch.tensor([[float(x * up_h), float(y * up_w)] for y, x in peaks]), None)
    ops_emul.install(monkeypatch, lsam, vit)
    monkeypatch.setattr(ops, "sam_mask_tail", host_tail)
    monkeypatch.setattr(ops, "sam_attn_prompt", host_prompt)
    md = sam_refine.wrap_sam(sam_cases.build_refine_hf(transformers), "device", device="cpu")
    images, boxes, attn = sam_cases.refine_inputs()
    owner = [ii for ii, per_image in enumerate(boxes) for _ in per_image]
    stack, flat = np.stack([images[ii] for ii in owner]), [b for per_image in boxes for b in per_image]
    many = sam_refine.SamRefiner(md, discourage_mask_below_coarse_iou=0.2)
    many.MODEL_CHUNK = 3
    one = sam_refine.SamRefiner(md, discourage_mask_below_coarse_iou=0.2, batched=False)
    bm, bc = many.boxes(torch.from_numpy(stack), flat)
    am, ac = many.attns(stack, attn)
    assert bm.dtype == am.dtype == torch.bool and tuple(bm.shape) == tuple(am.shape) == (4, 64, 64)
    for n in range(4):
        m, c = one.box(stack[n], flat[n])
        assert np.array_equal(bm[n].numpy(), m) and abs(float(bc[n]) - float(c)) < 1e-5, n
        m, c = one.attn(stack[n], attn[n])
        assert np.array_equal(am[n].numpy(), m) and abs(float(ac[n]) - float(c)) < 1e-5, n
