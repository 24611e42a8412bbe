"""The box prompt of an attention map on the device: lgd_sam_attn_box_prompt_f32 (csrc/sam_tail.hip), ops.sam_attn_box_prompt,
SamRefiner(use_box_input=True, attn_box="device").attns and the LMD pipeline's one call for all boxes.

Kernel.  The references are the numpy restatement of tests/sam_box_prompt_cases.py (no scipy) AND scipy.ndimage with
hostprep.binary_mask_to_box, on fp64.  The opened mask is byte-exact, the box and the empty flag are exact, the smoothed map
is within 1e-6 of its maximum (the bound of the point-prompt test, fp32 sums against fp64).  No pixel is left out: every
case keeps every normalised value 1e-4 away from the threshold (asserted by the case builder on the CPU).  Every output
lies between two guard bands that must come back untouched.

Refiner.  `attns()` against the same refiner's per-image `attn()`.  As the module docstring of lgd_amd.sam_refine records,
`sam_refine_attn(use_box_input=True)` hands the processor a two-level box list, as the reference does, and both processors
refuse it ("Input boxes must be a list of list of list of floating points"), so `attn()` cannot return a mask for such a
refiner.  The comparison therefore runs `attn()` itself with ONE thing changed: `sam_box_input` receives the box one list
level deeper (`_nested_boxes`), which is what the processor takes and what `sam_refine_boxes` hands it.  Everything else —
scipy's smoothing and opening, binary_mask_to_box, the processor, the model, post_process_masks, `_pick` — is `attn()`'s.
Masks must be equal; confidences agree within the 3e-2 that tests/test_sam_batched_gpu.py applies to the point branch.
Equality is asserted where the network computes the same thing on both sides: with MODEL_CHUNK = 1 the model sees every
item alone, as under `attn()`, and then all that differs between the two paths is this change's code — all four masks are
equal pixel for pixel.  With the four items in ONE model call the encoder's GEMM tiles follow the batch size (the module
docstring of tests/test_sam_batched_gpu.py), and logits at the threshold may flip: first measured on an MI355X, 1 and 10
of 4096 pixels differ on items 0 and 1 (agreement 0.9998 and 0.9976), none on items 2 and 3, confidences within 4e-4.
That comparison, and the one between chunkings, meets the gate that file applies (agreement >= 0.95, confidence 3e-2)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu

import lgd_amd  # noqa: E402,F401
import sam_box_prompt_cases as bc  # noqa: E402
import sam_cases  # noqa: E402
import sam_refine_checks  # noqa: E402
from lgd_amd import _lib, hostprep, ops, sam_refine, weights  # noqa: E402
from lgd_amd.hostprep import proportion_to_mask  # noqa: E402

GUARD = 64                      # elements on each side of every output
MIN_AGREE, CONF_TOL = 0.95, 3e-2


class _Guarded:
    """An output buffer of `n` elements between two bands of GUARD elements holding `fill`."""

    def __init__(self, n, dtype, fill, dev):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD * self.buf.element_size())

    def take(self, *shape):
        head, tail = self.buf[:GUARD].cpu(), self.buf[GUARD + self.n:].cpu()
        assert bool((head == self.fill).all()) and bool((tail == self.fill).all()), "a guard band was written"
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().reshape(shape)


def _launch(dev, maps, sigma, th, n_open, with_smooth=True):
    """One launch through the C entry with guarded outputs -> (coarse, boxes, empty, smooth or None) on the host."""
    lib = _lib.load()
    N, hm, wm = maps.shape
    up_w, up_h = bc.scales(hm, wm)
    attn = torch.from_numpy(np.ascontiguousarray(maps)).to(dev)
    co, bx = _Guarded(N * hm * wm, torch.uint8, 0xA5, dev), _Guarded(N * 4, torch.float32, 7.0, dev)
    em, sm = _Guarded(N, torch.int32, 7, dev), _Guarded(N * hm * wm, torch.float32, 7.0, dev)
    rc = lib.lgd_sam_attn_box_prompt_f32(C.c_void_p(attn.data_ptr()), N, hm, wm, sigma, th, n_open, up_w, up_h, co.ptr, bx.ptr,
                                         em.ptr, sm.ptr if with_smooth else C.c_void_p(0), C.c_void_p(0))
    assert rc == 0, rc
    torch.cuda.synchronize()
    smooth = sm.take(N, hm, wm)
    if not with_smooth:
        assert (smooth == 7.0).all()
    return co.take(N, hm, wm), bx.take(N, 4), em.take(N), smooth if with_smooth else None


def _check(label, maps, sigma, th, n_open, got, want=None):
    coarse, boxes, empty, smooth = got
    assert set(np.unique(coarse)) <= {0, 1} and set(np.unique(empty)) <= {0, 1}
    for n, a in enumerate(maps):
        w = want[n] if want is not None else bc.restate(a, sigma, th, n_open)
        assert w["near"] == 0
        s = ndimage.gaussian_filter(a.astype(float), sigma=sigma)
        with np.errstate(invalid="ignore"):
            sc = sam_refine.preprocess_mask(s, th, n_erode_dilate_mask=n_open)
        assert np.array_equal(w["coarse"], sc)                    # restatement and scipy agree (also in the CPU suite)
        if smooth is not None:
            err = float(np.abs(smooth[n] - s).max() / max(np.abs(s).max(), 1e-30))
            print(f"[sam box prompt] {label} item {n}: smooth err {err:.2e}, {int(sc.sum())} pixels, box {boxes[n].tolist()}, "
                  f"empty {int(empty[n])}")
            assert err <= 1e-6
        assert np.array_equal(coarse[n].astype(bool), w["coarse"]), (label, n, int((coarse[n].astype(bool) != w["coarse"]).sum()))
        assert int(empty[n]) == int(w["empty"]), (label, n)
        assert boxes[n].tolist() == [float(v) for v in w["box"]], (label, n, boxes[n].tolist(), w["box"])
        if sc.any():
            up_w, up_h = bc.scales(*sc.shape)
            assert boxes[n].tolist() == [float(v) for v in hostprep.binary_mask_to_box(sc, w_scale=up_w, h_scale=up_h)]
        else:
            assert int(empty[n]) == 1 and boxes[n].tolist() == [0.0] * 4


@pytest.mark.parametrize("case", range(len(bc.natural_ids())), ids=bc.natural_ids())
def test_kernel_vs_restatement_and_scipy_natural(dev, case):
    name, sigma, th, n_open, maps, want = bc.natural_cases()[case]
    _check(name, maps, sigma, th, n_open, _launch(dev, maps, sigma, th, n_open), want)


@pytest.mark.parametrize("case", range(len(bc.batches())), ids=[b[0] for b in bc.batches()])
def test_kernel_vs_restatement_and_scipy_synthetic(dev, case):
    label, maps, sigma, th, n_open = bc.batches()[case]
    got = _launch(dev, maps, sigma, th, n_open)
    _check(label, maps, sigma, th, n_open, got)
    name = label.rsplit("-open", 1)[0]
    outcomes = bc.synthetic_maps().get(name, (None, {}))[1]
    if n_open in outcomes:
        assert int(got[0].sum()) == outcomes[n_open]


def test_smooth_may_be_null_and_the_wrapper_returns_the_same(dev):
    name, sigma, th, n_open, maps, want = next(c for c in bc.natural_cases() if c[0] == "8x12" and c[3] == 1 and c[1] == 1.5)
    full = _launch(dev, maps, sigma, th, n_open)
    bare = _launch(dev, maps, sigma, th, n_open, with_smooth=False)
    _check("smooth=NULL", maps, sigma, th, n_open, bare, want)
    assert all(np.array_equal(a, b) for a, b in zip(full[:3], bare[:3]))
    t = torch.from_numpy(maps).to(dev)
    up_w, up_h = bc.scales(*maps.shape[1:])
    three = ops.sam_attn_box_prompt(t, sigma, th, n_open, up_w, up_h)
    four = ops.sam_attn_box_prompt(t, sigma, th, n_open, up_w, up_h, want_smooth=True)
    assert len(three) == 3 and len(four) == 4
    for out in (three, four):
        assert all(x.is_cuda for x in out)
        assert out[0].dtype == torch.uint8 and out[1].dtype == torch.float32 and out[2].dtype == torch.int32
        assert tuple(out[1].shape) == (len(maps), 4) and tuple(out[2].shape) == (len(maps),)
        for a, b in zip(full, out):
            assert np.array_equal(a, b.cpu().numpy())
    with pytest.raises(RuntimeError):
        ops.sam_attn_box_prompt(t.double(), sigma, th, n_open, up_w, up_h)


def test_eager_and_a_captured_graph_give_identical_bytes(dev):
    maps = torch.from_numpy(bc.natural_maps()["16x16"]).to(dev)

    def run():
        return ops.sam_attn_box_prompt(maps, 1.5, 0.25, 2, 32, 32, want_smooth=True)
    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                     # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    for t in captured:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert int(eager[0].sum()) > 0
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


def test_argument_checks(dev):
    lib = _lib.load()
    a = torch.zeros(1, 8, 8, device=dev)
    t = dict(coarse=torch.full((1, 8, 8), 7, dtype=torch.uint8, device=dev), boxes=torch.full((1, 4), 7.0, device=dev),
             empty=torch.full((2,), 7, dtype=torch.int32, device=dev), smooth=torch.full((1, 8, 8), 7.0, device=dev))
    p = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}
    p["attn"] = C.c_void_p(a.data_ptr())
    null = C.c_void_p(0)

    def call(N=1, hm=8, wm=8, sigma=1.5, th=0.25, n_open=1, up_w=64, up_h=64, **over):
        q = dict(p, **over)
        return lib.lgd_sam_attn_box_prompt_f32(q["attn"], N, hm, wm, sigma, th, n_open, up_w, up_h, q["coarse"], q["boxes"],
                                               q["empty"], q["smooth"], null)
    for name in ("attn", "coarse", "boxes", "empty"):
        assert call(**{name: null}) == -1, name
    assert call(N=0) == -1 and call(hm=0) == -1 and call(wm=-1) == -1
    assert call(up_w=0) == -1 and call(up_h=0) == -1
    assert call(sigma=0.0) == -1 and call(sigma=-1.0) == -1 and call(n_open=-1) == -1
    assert call(boxes=C.c_void_p(t["boxes"].data_ptr() + 2)) == -1
    assert call(hm=128, wm=128) == -3 and call(hm=64, wm=65) == -3
    assert call(sigma=16.2) == -3                                 # radius 65
    assert call(N=65536) == -3 and call(n_open=65) == -3
    torch.cuda.synchronize()
    for k, v in t.items():                                        # nothing was launched: no operand changed
        assert bool((v == 7).all()), k
    assert call() == 0 and call(smooth=null) == 0                 # and the same operands are accepted
    torch.cuda.synchronize()
    assert int(t["empty"][0]) == 1 and int(t["empty"][1]) == 7    # a constant map: flagged, and only its own flag written


def test_kernel_and_tail_vs_the_references_own_box_branch(dev):
    """tests/golden/sam_refine_attn_box.npz (tools/make_golden_sam_box_prompt.py): the opened mask and the box the
    reference's sam_refine_attn(use_box_input=True) computed, and its selection among fixed candidates.  The kernel's
    mask and box equal the reference's, and ops.sam_mask_tail, scoring those candidates against the KERNEL's opened mask,
    selects what the reference selected.  The candidates reach the tail as logits of +-1 at 64 x 64 with a 64 x 64 image
    and grid: every resampling of the tail is then the identity."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_refine_attn_box.npz"))
    for si, (sigma, th, n_open) in enumerate(g["settings"]):
        ks = [k for k, (s, _) in enumerate(g["cases"]) if s == si]
        ns = [int(g["cases"][k][1]) for k in ks]
        maps = torch.from_numpy(np.ascontiguousarray(g["maps"][ns])).to(dev)
        coarse, boxes, empty = ops.sam_attn_box_prompt(maps, sigma, th, int(n_open), 512 // 64, 512 // 64)
        logits = torch.from_numpy(np.where(g["cand"][ns], 1.0, -1.0).astype(np.float32)).to(dev)
        geom = torch.tensor([[64, 64, 64, 64]] * len(ks), dtype=torch.int32, device=dev)
        mask, conf, stats, cand = ops.sam_mask_tail(logits, torch.from_numpy(g["conf"][ns]).to(dev), geom, 64, (64, 64), coarse,
                                                    float(g["below"][0]), float(g["below"][1]))
        assert int(empty.sum()) == 0
        assert np.array_equal(cand.cpu().numpy().astype(bool), g["cand"][ns])
        for i, k in enumerate(ks):
            assert np.array_equal(coarse[i].cpu().numpy(), g[f"coarse{k}"]), k
            assert boxes[i].cpu().tolist() == [float(v) for v in g[f"box{k}"]], k
            assert np.array_equal(mask[i].cpu().numpy(), g[f"mask{k}"]), k
            assert float(conf[i]) == float(g[f"picked_conf{k}"]), k


# ---- the refiner on the tiny SAM configuration of tests/test_sam_batched_gpu.py
BOX_KW = dict(use_box_input=True, gaussian_sigma=0.1, mask_th_for_box=0.2, n_erode_dilate_mask_for_box=1)


@pytest.fixture(scope="module")
def sam_dict(dev):
    transformers = pytest.importorskip("transformers")
    return sam_refine.wrap_sam(sam_cases.build_refine_hf(transformers), "device", device=dev)


def _refiner(sam_dict, **kw):
    k = sam_refine_checks.KW
    return sam_refine.SamRefiner(sam_dict, height=k["height"], width=k["width"],
                                 discourage_mask_below_confidence=k["discourage_mask_below_confidence"],
                                 discourage_mask_below_coarse_iou=k["discourage_mask_below_coarse_iou"], **BOX_KW, **kw)


def _pairs():
    images, boxes, attn = sam_cases.refine_inputs()
    owner = [ii for ii, per_image in enumerate(boxes) for _ in per_image]
    attn = [np.asarray(a, dtype=np.float32) for a in attn]
    for a in attn:                                                # no normalised value near the threshold: the fp32 and
        w = bc.restate(a, BOX_KW["gaussian_sigma"], BOX_KW["mask_th_for_box"], 1)   # fp64 masks are the same mask
        assert w["near"] == 0 and not w["empty"]
    return np.stack([images[ii] for ii in owner]), attn


def _nested_boxes(monkeypatch):
    """`attn()` with the box one list level deeper at `sam_box_input`, the form the processor takes (module docstring)."""
    real = sam_refine.sam_box_input

    def nested(md, image, input_boxes, **kw):
        assert len(input_boxes) == 1 and len(input_boxes[0]) == 4 and not isinstance(input_boxes[0][0], (list, tuple))
        return real(md, image, [[list(input_boxes[0])]], **kw)
    monkeypatch.setattr(sam_refine, "sam_box_input", nested)


@pytest.fixture(scope="module")
def batched_result(sam_dict, dev):
    stack, attn = _pairs()
    r = _refiner(sam_dict, attn_box="device")
    m, c = r.attns(torch.from_numpy(stack).to(dev), torch.from_numpy(np.stack(attn)).to(dev))
    assert m.is_cuda and m.dtype == torch.bool and tuple(m.shape) == (4, 64, 64)
    assert c.is_cuda and c.dtype == torch.float32 and tuple(c.shape) == (4,)
    return m.cpu().numpy(), c.cpu().numpy()


def test_one_attns_call_vs_attn_per_image(sam_dict, dev, batched_result, monkeypatch):
    stack, attn = _pairs()
    r = _refiner(sam_dict, attn_box="device")
    with pytest.raises(ValueError, match="list of list of list"):  # why the comparison nests the box: attn() as it stands
        r.attn(stack[0], attn[0])
    _nested_boxes(monkeypatch)
    one = [r.attn(stack[n], attn[n]) for n in range(4)]
    alone = _refiner(sam_dict, attn_box="device")
    alone.MODEL_CHUNK = 1                                         # the model sees each item alone, as under attn()
    m1, c1 = alone.attns(torch.from_numpy(stack).to(dev), torch.from_numpy(np.stack(attn)).to(dev))
    for name, (masks, conf) in (("one item per model call", (m1.cpu().numpy(), c1.cpu().numpy())),
                                ("four items in one model call", batched_result)):
        for n, (m, c) in enumerate(one):
            agree = float((masks[n] == np.asarray(m).astype(bool)).mean())
            print(f"[sam box prompt] attns() vs attn(), {name}: item {n} agreement {agree:.4f}, confidence "
                  f"{float(conf[n]):.4f} against {float(c):.4f}, {int(masks[n].sum())} pixels")
    for n, (m, c) in enumerate(one):
        assert np.array_equal(m1[n].cpu().numpy(), np.asarray(m).astype(bool)), n
        assert abs(float(c1[n]) - float(c)) <= CONF_TOL, (n, float(c1[n]), float(c))
        agree = float((batched_result[0][n] == np.asarray(m).astype(bool)).mean())
        assert agree >= MIN_AGREE and abs(float(batched_result[1][n]) - float(c)) <= CONF_TOL, (n, agree)


def test_the_tail_scores_against_the_opened_mask(sam_dict, dev, monkeypatch):
    """What `_tail` receives is the kernel's opened mask and its box, (N, 1, 4) in pixels of the original image."""
    stack, attn = _pairs()
    r = _refiner(sam_dict, attn_box="device")
    seen = {}

    def tail(images, coarse, **prompt):
        seen.update(coarse=coarse.cpu().numpy(), prompt={k: v.cpu().numpy() for k, v in prompt.items()})
        return torch.zeros(4, 64, 64, dtype=torch.bool), torch.zeros(4)
    monkeypatch.setattr(r, "_tail", tail)
    r.attns(stack, attn)                                          # a list of arrays and host images are taken as well
    assert list(seen["prompt"]) == ["input_boxes"] and seen["prompt"]["input_boxes"].shape == (4, 1, 4)
    for n, a in enumerate(attn):
        w = bc.restate(a, BOX_KW["gaussian_sigma"], BOX_KW["mask_th_for_box"], BOX_KW["n_erode_dilate_mask_for_box"])
        assert np.array_equal(seen["coarse"][n].astype(bool), w["coarse"])
        assert seen["prompt"]["input_boxes"][n, 0].tolist() == [float(v) for v in w["box"]]


def test_chunks_of_the_model_do_not_change_an_item(sam_dict, dev, batched_result):
    stack, attn = _pairs()
    r = _refiner(sam_dict, attn_box="device")
    r.MODEL_CHUNK = 3                                             # 3 + 1
    m, c = r.attns(stack, attn)
    m, c = m.cpu().numpy(), c.cpu().numpy()
    for n in range(4):
        agree = float((m[n] == batched_result[0][n]).mean())
        print(f"[sam box prompt] chunks of 3 vs one chunk: item {n} agreement {agree:.4f}, confidence {float(c[n]):.4f} "
              f"against {float(batched_result[1][n]):.4f}")
        assert agree >= MIN_AGREE and abs(float(c[n]) - float(batched_result[1][n])) <= CONF_TOL, n


def test_an_empty_item_raises_and_the_model_is_not_called(sam_dict, dev):
    stack, attn = _pairs()
    maps = [attn[0], np.full((64, 64), 0.37, np.float32), attn[2], np.zeros((64, 64), np.float32)]
    maps[3][10, 10] = 1.0                                         # a lone pixel: gone after one erosion

    class Untouched:
        def __call__(self, *a, **k):
            raise AssertionError("the model ran")
    r = _refiner(dict(sam_model=Untouched(), sam_processor=sam_dict["sam_processor"]), attn_box="device")
    with pytest.raises(ValueError, match=r"\[1, 3\]"):
        r.attns(stack, maps)
    with pytest.raises(NotImplementedError):                      # and without the opt-in nothing has changed
        _refiner(sam_dict).attns(stack, attn)


# ---- the LMD pipeline
L = 32


@pytest.fixture(scope="module")
def tiny_lmd(dev):
    """The tiny run of tests/test_sam_batched_gpu.py (256 x 256, 2 boxes per layout), two layouts."""
    from lgd_amd.pipeline import CachedLayout
    from lgd_amd.sampler import LMDSampler
    from lgd_amd.scheduler import DDIMScheduler
    from lgd_amd.unet import UNetEngine
    from lgd_amd.vae import make_hip_vae
    cfg = weights.CONFIGS["tiny_gligen"]
    sm = LMDSampler(UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0)), DDIMScheduler(), vae=make_hip_vae(dev))
    lays = [CachedLayout.synthetic(cfg, [("a white deer", [74, 177, 183, 235]), ("a gray bear", [314, 193, 189, 216])], 3),
            CachedLayout.synthetic(cfg, [("a red fox", [60, 120, 200, 260]), ("a black cat", [300, 150, 170, 230])], 5)]
    return sm, lays


def test_lmd_pipeline_makes_one_attns_call_for_all_boxes_of_all_layouts(tiny_lmd, sam_dict, monkeypatch):
    """With attn_box="device" the box prompts of all four boxes of both layouts are ONE `attns` call on device tensors;
    the default refiner is still asked per box through `attn` (answered here with the box mask: `attn()` itself cannot
    serve a box prompt, see the module docstring).  n_erode_dilate_mask_for_box = 0 here: the 8 x 8 maps of a
    randomly initialised UNet need not survive an erosion, and an empty mask rightly raises."""
    from lgd_amd.pipeline import lmd_generate_batch
    sm, lays = tiny_lmd
    kw = dict(num_inference_steps=12, max_index_step=3, overall_max_index_step=3, so_center_box=False,
              align_with_overall_bboxes=False, height=8 * L, width=8 * L)
    calls = []
    real_attns = sam_refine.SamRefiner.attns

    def rec_attns(self, images, maps):
        calls.append(("attns", tuple(images.shape), images.is_cuda, tuple(maps.shape), maps.is_cuda))
        m, c = real_attns(self, images, maps)
        assert m.is_cuda and tuple(m.shape) == (4, L, L) and tuple(c.shape) == (4,)
        return m, c

    def rec_attn(self, image, token_attn):
        calls.append(("attn", image.shape, type(token_attn), token_attn.shape))
        return proportion_to_mask((0.25, 0.25, 0.75, 0.75), L, L, return_np=True).astype(bool), 1.0
    monkeypatch.setattr(sam_refine.SamRefiner, "attns", rec_attns)
    monkeypatch.setattr(sam_refine.SamRefiner, "attn", rec_attn)
    box = dict(height=8 * L, width=8 * L, use_box_input=True, n_erode_dilate_mask_for_box=0)
    out = lmd_generate_batch(sm, lays, mask_refiner=sam_refine.SamRefiner(sam_dict, attn_box="device", **box), **kw)
    assert calls == [("attns", (4, 8 * L, 8 * L, 3), True, (4, L // 4, L // 4), True)]
    assert len(out) == 2 and all(o["image"].shape == (8 * L, 8 * L, 3) and o["image"].dtype == np.uint8 for o in out)
    calls.clear()
    lmd_generate_batch(sm, lays, mask_refiner=sam_refine.SamRefiner(sam_dict, **box), **kw)
    assert calls == [("attn", (8 * L, 8 * L, 3), np.ndarray, (L // 4, L // 4))] * 4
