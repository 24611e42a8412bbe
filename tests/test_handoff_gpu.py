"""The three kernels of csrc/handoff.hip (placement, composition, reference maps) on the device, through
lgd_amd.handoff.run and lgd_amd.ops, against the host path they replace: hostprep.align_with_bboxes + hostprep.compose +
pipeline._align_stage_a + pipeline._ref_maps on the CPU (tests/handoff_cases.py), and against the reference's own
utilities (tests/golden/align_host.npz).  Copy work and integer work only, so every comparison is torch.equal.

Shapes: L = 16, C = 4, 3 steps, map sides 8 and 16 — the smallest at which the eighth-of-the-frame quantisation still
differs between latents (2 pixels) and maps (1 and 2 pixels).  Where the host raises (a mask that is empty after the
shift) the expected value is the rule of include/lgd_hip.h: the box is skipped and flagged, the others are untouched."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lgd_amd  # noqa: E402,F401
import handoff_cases as hc  # noqa: E402
from lgd_amd import handoff, ops, pipeline  # noqa: E402
from lgd_amd.hostprep import proportion_to_mask, shift_tensor  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "align_host.npz")
GOLD_KEYS = [("mid", 0, 0, 0), ("up", 1, 0, 0), ("up", 1, 1, 0), ("up", 1, 2, 0)]
GOLD_SIDES = {k: (8 if k[0] == "mid" else 16) for k in GOLD_KEYS}
BOXES_XYWH = [[74, 177, 183, 235], [314, 193, 189, 216], [20, 300, 120, 150]]
BBOXES = [[x / 512, y / 512, (x + w) / 512, (y + h) / 512] for x, y, w, h in BOXES_XYWH]


def run_device(dev, per_lay, targets, bgs, batches, *, align, horizontal_shift_only=False, keys=hc.KEYS, L=hc.L, T=hc.T,
               steps=hc.STEPS, heads=hc.HEADS, max_hw=256):
    """handoff.run on `dev` for CPU stage-A results (moved there; histories stay views of their batch tensors)."""
    moved, bg_d, keep = hc.to_device(per_lay, bgs, batches, dev)
    out = handoff.run(dev, masks=[d["masks"] for d in moved], targets=targets, histories=[d["latents_all"] for d in moved],
                      saved=[d["saved"] for d in moved], bgs=bg_d, keys=keys, L=L, T=T, steps=steps, align=align,
                      horizontal_shift_only=horizontal_shift_only, heads=heads, max_hw=max_hw)
    assert all(r[name].device.type == torch.device(dev).type for r in out for name in ("composed", "fg_idx", "plan"))
    return out


def check_layout(r, h, tag=""):
    assert hc.same(r["composed"], h["composed"]), f"{tag}: composed"
    assert hc.same(r["fg_idx"], h["fg_idx"]), f"{tag}: fg_idx"
    if h["ref_maps"] is not None:
        assert hc.same(r["ref_maps"], h["ref_maps"]), f"{tag}: ref_maps"
    assert len(r["latents_all"]) == len(h["latents_all"]), tag
    for b, (a, w) in enumerate(zip(r["latents_all"], h["latents_all"])):
        assert hc.same(a, w), f"{tag}: history of box {b}"
    assert [tuple(row) for row in r["plan"][:, :2].cpu().numpy()] == h["offsets"], f"{tag}: offsets"
    assert not r["plan"][:, 7].any(), tag


@pytest.mark.parametrize("horizontal_shift_only", [False, True])
def test_golden_of_the_reference_utilities(dev, horizontal_shift_only):
    """oracle/make_golden_align.py: 3 boxes, L = 64, 4 keys, compose_latents_with_alignment + shift_saved_attns."""
    g = np.load(GOLD)
    t = "h" if horizontal_shift_only else "xy"
    so = pipeline._centered_so_boxes(hc.Lay(BBOXES), True, horizontal_center_only=False,
                                     vertical_placement="floor_padding", floor_padding=0.2)
    hist = [torch.from_numpy(g[f"lall{i}"]).to(dev) for i in range(3)]
    saved = [{k: torch.from_numpy(g[f"saved_{i}_{ki}"]).to(dev) for ki, k in enumerate(GOLD_KEYS)} for i in range(3)]
    masks = [proportion_to_mask(b, 64, 64).bool() for b in so]                      # host masks: uploaded once
    r = handoff.run(dev, masks=[masks], targets=[BBOXES], histories=[hist], saved=[saved], bgs=[torch.from_numpy(g["bg"])],
                    keys=GOLD_KEYS, L=64, T=3, steps=3, align=True, horizontal_shift_only=horizontal_shift_only,
                    heads=2, max_hw=256)[0]
    assert np.array_equal(r["composed"].cpu().numpy(), g[f"composed_{t}"])
    assert r["fg_idx"].dtype == torch.int64 and np.array_equal(r["fg_idx"].cpu().numpy(), g[f"fg_idx_{t}"])
    ref = r["ref_maps"].cpu()
    assert tuple(ref.shape) == (3, 3, 4, 2, 256)
    for b in range(3):
        for ki, k in enumerate(GOLD_KEYS):
            hw = GOLD_SIDES[k] ** 2
            assert np.array_equal(ref[:, b, ki, :, :hw].numpy(), g[f"shifted_{t}_{b}_{ki}"][:, 0, :, :, 0]), (b, k)
            assert not ref[:, b, ki, :, hw:].any()
    offs = g[f"offsets_{t}"]                                                         # the reference's (x_off, y_off) per box
    assert [tuple(row) for row in r["plan"][:, :2].cpu().numpy()] == [(round(x * 8) * 8, round(y * 8) * 8) for x, y in offs]


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("seed", [11, 13])
def test_seeded_layouts_against_the_host_path(dev, seed, chunks, align):
    """3 layouts in one call with 0, 1 and 5 boxes, overlapping masks; histories are strided views of one or of two batch
    tensors and hold 2 rows more than the composition takes; the saved maps hold one row fewer than T."""
    masks, targets = hc.random_layouts(seed)
    lays, per_lay, bgs, batches = hc.stage_a(masks, targets, seed=seed, hist_rows=hc.STEPS + 3, map_rows=hc.T - 1,
                                             chunks=chunks)
    overlap = sum(m.long() for m in masks[2])
    assert int(overlap.max()) >= 2                                                   # the case has overlapping masks
    host = hc.host_path(lays, per_lay, bgs, align=align, horizontal_shift_only=False)
    assert hc.distinct_areas(host)                                                   # equal areas have their own test
    out = run_device(dev, per_lay, targets, bgs, batches, align=align)
    for l, (r, h) in enumerate(zip(out, host)):
        check_layout(r, h, f"layout {l}")
        assert tuple(r["ref_maps"].shape) == (hc.T, len(masks[l]), 2, hc.HEADS, 256)
        assert not r["ref_maps"][hc.T - 1:].any()
    assert all(tuple(a.shape) == (hc.STEPS + 3, 1, hc.C, hc.L, hc.L) for a in out[2]["latents_all"])


def _ties():
    """Rectangles of columns 4 .. 7 (centre 5.5 pixels = 0.34375) and dyadic target centres: x_off * 8 is exactly
    +-0.5, +-1.5, +-2.5, where Python rounds to the even neighbour (0, 2, 2); y_off * 8 likewise with the other sign.  The
    heights differ (2 .. 7 rows) so that no two areas are equal, and every shift stays inside the frame."""
    want = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5]
    tops = [5, 5, 6, 2, 6, 1]
    masks = [hc.rect(4, tops[i], 8, tops[i] + 2 + i) for i in range(6)]
    targets = []
    for i, v in enumerate(want):
        tc_x = (v + 5.5 / 2) / 8
        cy = tops[i] + (2 + i - 1) / 2
        tc_y = (-v + cy / 2) / 8
        targets.append((tc_x - 0.125, tc_y - 0.0625, tc_x + 0.125, tc_y + 0.0625))
        assert ((targets[-1][0] + targets[-1][2]) / 2 - 5.5 / 16) * 8 == v
        assert ((targets[-1][1] + targets[-1][3]) / 2 - cy / 16) * 8 == -v
    return masks, targets, want


def test_rounding_ties_go_to_the_even_neighbour_as_python_rounds(dev):
    masks, targets, want = _ties()
    lays, per_lay, bgs, batches = hc.stage_a([masks], [targets], seed=21)
    r = run_device(dev, per_lay, [targets], bgs, batches, align=True)[0]
    got = [tuple(row) for row in r["plan"][:, :2].cpu().numpy()]
    assert got == [(round(v) * 2, round(-v) * 2) for v in want] == [(0, 0), (0, 0), (4, -4), (-4, 4), (4, -4), (-4, 4)]
    assert r["plan"][:, 2].tolist() == [4 * (2 + i) for i in range(6)]
    check_layout(r, hc.host_path(lays, per_lay, bgs, align=True, horizontal_shift_only=False)[0], "ties")


def test_the_centre_is_one_fp32_division(dev):
    """Areas 3, 7 and 11 with non-dyadic quotients: the fp32 centre is not the fp64 one, and the offsets follow the fp32
    one as hostprep.binary_mask_to_center computes it."""
    masks, targets = [], []
    for n, tc in ((3, 0.37), (7, 0.61), (11, 0.45)):
        m = torch.zeros(hc.L, hc.L, dtype=torch.bool)
        cols = [0, 1, 3, 4, 6, 7, 9, 10, 12, 13, 15][:n]
        m[[2 + (i % 3) for i in range(n)], cols] = True
        sx, sy = sum(cols), sum(2 + (i % 3) for i in range(n))
        assert float(np.float32(sx) / np.float32(n)) != sx / n or float(np.float32(sy) / np.float32(n)) != sy / n
        masks.append(m)
        targets.append((tc - 0.1, tc - 0.2, tc + 0.1, tc + 0.2))
    lays, per_lay, bgs, batches = hc.stage_a([masks], [targets], seed=22)
    r = run_device(dev, per_lay, [targets], bgs, batches, align=True)[0]
    check_layout(r, hc.host_path(lays, per_lay, bgs, align=True, horizontal_shift_only=False)[0], "fp32 centre")


def test_a_shift_that_cuts_a_mask_counts_the_area_after_it(dev):
    """Box 0 (8 x 4 = 32 pixels at the left edge) moves 12 pixels to the right and keeps 4 x 4 = 16; box 1 has 20.  Before
    the shift box 0 is the larger and would be painted first; after it box 1 is, and box 0 wins the overlap.  The grown
    box of box 0 covers column 11, whose source column -1 is outside the frame: step 0 is 0 there, not the background
    (rows 3 and 4; from row 5 on box 1's mask owns that column)."""
    masks = [hc.rect(0, 4, 8, 8), hc.rect(10, 5, 15, 9)]
    targets = [(0.875, 0.25, 1.125, 0.5), (0.65625, 0.3125, 0.90625, 0.5625)]      # box 1 stays where it is
    lays, per_lay, bgs, batches = hc.stage_a([masks], [targets], seed=23)
    r = run_device(dev, per_lay, [targets], bgs, batches, align=True)[0]
    plan = r["plan"].cpu().numpy()
    assert plan[:, :3].tolist() == [[12, 0, 16], [0, 0, 20]]
    assert plan[0, 3:7].tolist() == [11, 3, 16, 8] and plan[:, 7].tolist() == [0, 0]
    fg = r["fg_idx"].cpu()
    assert (fg[5:8, 12:15] == 1).all() and (fg[8, 12:15] == 2).all()                # the later (smaller) box on top
    comp = r["composed"].cpu()
    assert not comp[0, 0, :, 3:5, 11].any() and bgs[0][0, :, 3:5, 11].all()         # zero fill, not background
    assert torch.equal(comp[0, 0, :, 0, :], bgs[0][0, :, 0, :])                      # background where no box reaches
    check_layout(r, hc.host_path(lays, per_lay, bgs, align=True, horizontal_shift_only=False)[0], "cut")


def test_a_mask_shifted_out_entirely_is_skipped_and_flagged(dev):
    """Box 2 (columns 0 .. 1) is sent 2 pixels to the left, box 3 has no pixel at all: the host raises ValueError('The
    mask is empty'); here both are flagged, own nothing, and boxes 0 and 1 compose exactly as without them."""
    masks, targets = hc.random_layouts(31, counts=(2,))
    masks[0] += [hc.rect(0, 6, 2, 9), torch.zeros(hc.L, hc.L, dtype=torch.bool)]
    targets[0] += [(-0.25, 0.3, 0.0, 0.6), (0.2, 0.2, 0.6, 0.6)]
    lays, per_lay, bgs, batches = hc.stage_a(masks, targets, seed=24)
    with pytest.raises(ValueError), np.errstate(invalid="ignore"):
        hc.host_path(lays, per_lay, bgs, align=True, horizontal_shift_only=False)
    r = run_device(dev, per_lay, targets, bgs, batches, align=True)[0]
    plan = r["plan"].cpu().numpy()
    assert plan[:, 7].tolist() == [0, 0, 1, 1] and plan[2, :3].tolist() == [-2, 0, 0] and plan[3, :3].tolist() == [0, 0, 0]
    two = [dict(latents_all=d["latents_all"][:2], masks=d["masks"][:2], saved=d["saved"][:2]) for d in per_lay]
    h = hc.host_path([hc.Lay(targets[0][:2])], two, bgs, align=True, horizontal_shift_only=False)[0]
    assert hc.same(r["composed"], h["composed"]) and hc.same(r["fg_idx"], h["fg_idx"])
    assert hc.same(r["ref_maps"][:, :2], h["ref_maps"])
    assert all(hc.same(a, b) for a, b in zip(r["latents_all"][:2], h["latents_all"]))
    assert hc.same(r["latents_all"][2], shift_tensor(per_lay[0]["latents_all"][2], -2, 0))   # the rule holds for it too
    assert hc.same(r["latents_all"][3], per_lay[0]["latents_all"][3])                # offset 0: the history itself


@pytest.mark.parametrize("align", [False, True])
def test_equal_areas_paint_the_lower_index_first(dev, align):
    """Two overlapping 4 x 5 and 5 x 4 masks (20 pixels each; under alignment both keep their area): a stable sort of the
    negated areas paints box 0 first, so box 1 owns the overlap — in the masks and in the grown boxes of step 0."""
    masks = [hc.rect(4, 4, 8, 9), hc.rect(6, 6, 11, 10)]
    targets = [(0.25, 0.25, 0.5, 0.5), (0.375, 0.375, 0.625, 0.625)]
    lays, per_lay, bgs, batches = hc.stage_a([masks], [targets], seed=25)
    r = run_device(dev, per_lay, [targets], bgs, batches, align=align)[0]
    plan = r["plan"].cpu().numpy()
    assert plan[:, 2].tolist() == [20, 20]
    (ox0, oy0), (ox1, oy1) = plan[0, :2], plan[1, :2]
    m0 = torch.roll(masks[0], (int(oy0), int(ox0)), (0, 1))                          # no pixel leaves the frame here
    m1 = torch.roll(masks[1], (int(oy1), int(ox1)), (0, 1))
    assert int(m0.sum()) == int(m1.sum()) == 20 and (m0 & m1).any()
    fg = r["fg_idx"].cpu()
    order = sorted(range(2), key=lambda i: -int(plan[i, 2]))                        # stable: [0, 1]
    want = torch.zeros(hc.L, hc.L, dtype=torch.long)
    for i in order:
        want[(m0, m1)[i]] = i + 1
    assert order == [0, 1] and torch.equal(fg, want) and (fg[m0 & m1] == 2).all()
    # step 0 next to the masks: the grown boxes overlap too, and box 1's is the later one
    hist = [h.clone() for h in per_lay[0]["latents_all"]]
    grown1 = torch.zeros(hc.L, hc.L, dtype=torch.bool)
    grown1[plan[1, 4]:plan[1, 6] + 1, plan[1, 3]:plan[1, 5] + 1] = True
    ring = grown1 & ~m0 & ~m1
    shifted = [torch.roll(hist[0], (int(oy0), int(ox0)), (3, 4)), torch.roll(hist[1], (int(oy1), int(ox1)), (3, 4))]
    assert ring.any() and torch.equal(r["composed"].cpu()[0, 0][:, ring], shifted[1][0, 0][:, ring])
    composed, fg_idx = hc.compose_in_order(shifted, [m0, m1], order, hc.STEPS, bgs[0])
    assert hc.same(r["composed"], composed) and hc.same(r["fg_idx"], fg_idx)


def _tables(dev, seed=41):
    masks, targets = hc.random_layouts(seed)
    lays, per_lay, bgs, batches = hc.stage_a(masks, targets, seed=seed)
    moved, bg_d, keep = hc.to_device(per_lay, bgs, batches, dev)
    counts = [len(m) for m in masks]
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    hist = np.array([[h.data_ptr(), h.stride(0)] for d in moved for h in d["latents_all"]], dtype=np.int64)
    maps = np.array([[s[k].data_ptr(), s[k].shape[0], hc.SIDES[k]] for d in moved for s in d["saved"] for k in hc.KEYS],
                    dtype=np.int64).reshape(-1, 2, 3)
    tgt = np.array([t for per in targets for t in per], dtype=np.float64)
    lay_of = np.repeat(np.arange(3, dtype=np.int32), counts)
    tabs = handoff.pack_tables([seg, lay_of, tgt, hist, maps], dev)
    m = torch.stack([x for d in moved for x in d["masks"]]).view(torch.uint8)
    return tabs, m, torch.cat(bg_d), max(counts), (moved, keep)


def _three_ops(tabs, m, bg, max_boxes):
    seg, lay_of, tgt, hist, maps = tabs
    plan, win = ops.handoff_place(m, tgt, seg, max_boxes, align=True, horizontal_shift_only=False)
    composed, fg_idx, aligned = ops.handoff_compose(plan, win, seg, hist, bg, hc.STEPS, rows=hc.STEPS + 1)
    ref = ops.handoff_ref_maps(plan, seg, lay_of, maps, hc.T, hc.HEADS, 256, hc.L)
    return plan, win, composed, fg_idx, aligned, ref


def test_two_runs_and_one_captured_graph_are_bit_identical(dev):
    tabs, m, bg, max_boxes, keep = _tables(dev)
    first = _three_ops(tabs, m, bg, max_boxes)
    second = _three_ops(tabs, m, bg, max_boxes)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _three_ops(tabs, m, bg, max_boxes)
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b, c in zip(("plan", "win", "composed", "fg_idx", "aligned", "ref_maps"), first, second, captured):
        assert torch.equal(a, b), f"second run: {name}"
        assert torch.equal(a, c), f"captured graph: {name}"


def test_what_the_library_refuses(dev):
    seg = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    tgt = torch.tensor([[0.25, 0.25, 0.75, 0.75]], dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="invalid argument"):                      # shift_tensor's assertion
        ops.handoff_place(torch.ones((1, 12, 12), dtype=torch.uint8, device=dev), tgt, seg, 1, align=True,
                          horizontal_shift_only=False)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.handoff_compose(torch.zeros((1, 8), dtype=torch.int32, device=dev),
                            torch.zeros((1, 2, 12, 12), dtype=torch.int32, device=dev), seg,
                            torch.zeros((1, 2), dtype=torch.int64, device=dev), torch.zeros((1, 4, 12, 12), device=dev), 3)
    many = torch.tensor([0, 65], dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="unsupported shape"):                     # the cap is 64 boxes per layout
        ops.handoff_place(torch.ones((65, 16, 16), dtype=torch.uint8, device=dev), tgt.repeat(65, 1), many, 65, align=True,
                          horizontal_shift_only=False)
    plan, win = ops.handoff_place(torch.ones((16, 16, 16), dtype=torch.uint8, device=dev), tgt.repeat(16, 1),
                                  torch.tensor([0, 16], dtype=torch.int32, device=dev), 16, align=True,
                                  horizontal_shift_only=False)                        # 16 boxes are within it
    assert (win.cpu() == 15).all() and plan.cpu()[:, 2].tolist() == [256] * 16


# -------------------------------------------------------------------------------------------------
# end to end: both pipelines, both hand-offs
# -------------------------------------------------------------------------------------------------
class BatchedBoxMasks:
    """A batched refiner that answers with the box masks as ONE device tensor (the hook alone: no SAM)."""
    batched = True

    def __init__(self, L):
        self.L = L

    def boxes(self, images, boxes):
        m = torch.stack([proportion_to_mask(b, self.L, self.L).bool() for b in boxes]).to(images.device)
        return m, torch.ones(len(boxes), device=images.device)

    def attns(self, images, maps):
        side = maps.shape[-1]
        m = (maps > maps.mean(dim=(1, 2), keepdim=True)).repeat_interleave(self.L // side, 1).repeat_interleave(self.L // side, 2)
        m[:, self.L // 2, self.L // 2] = True                                        # never empty
        return m, torch.ones(len(maps), device=images.device)


E2E_L = 64       # the 8 x 8 quantisation needs the mid-block map to be 8 x 8 (shift_tensor's assertion)
SAM_L = 32       # the run of tests/test_sam_batched_gpu.py, the size at which the helpers' SAM is known to leave masks


@pytest.fixture(scope="module")
def tiny(dev):
    from lgd_amd import weights
    from lgd_amd.pipeline import CachedLayout
    from lgd_amd.sampler import LMDSampler
    from lgd_amd.scheduler import DDIMScheduler
    from lgd_amd.unet import UNetEngine
    from lgd_amd.vae import make_hip_vae
    cfg = weights.CONFIGS["tiny_gligen"]
    sm = LMDSampler(UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0)), DDIMScheduler(), vae=make_hip_vae(dev))
    lays = [CachedLayout.synthetic(cfg, [("a white deer", [74, 177, 183, 235]), ("a gray bear", [314, 193, 189, 216])], 3),
            CachedLayout.synthetic(cfg, [("a cat", [20, 300, 120, 150]), ("a cat", [300, 60, 160, 200]),
                                         ("a dog", [180, 200, 200, 260])], 4)]
    return sm, lays


@pytest.fixture(scope="module")
def tiny_at_32(dev):
    """An engine of its own for the 32 x 32 run: one engine keeps to one latent size here."""
    from lgd_amd import weights
    from lgd_amd.sampler import LMDSampler
    from lgd_amd.scheduler import DDIMScheduler
    from lgd_amd.unet import UNetEngine
    from lgd_amd.vae import make_hip_vae
    cfg = weights.CONFIGS["tiny_gligen"]
    return LMDSampler(UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0)), DDIMScheduler(), vae=make_hip_vae(dev))


def _refiner(kind, dev):
    if kind == "none":
        return None
    if kind == "stand-in":
        return BatchedBoxMasks(E2E_L)
    import transformers
    import sam_cases
    from lgd_amd import sam_refine
    r = sam_refine.SamRefiner(sam_refine.wrap_sam(sam_cases.build_refine_hf(transformers), "device", device=dev),
                              height=8 * SAM_L, width=8 * SAM_L)
    assert r.batched
    return r


def _same_results(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same_results(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_results(x, y, f"{path}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and hc.same(a, b), path
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    else:
        assert a == b, (path, a, b)


@pytest.mark.parametrize("refiner", ["none", "stand-in", "sam"])
@pytest.mark.parametrize("method", ["lmd_plus", "lmd"])
def test_pipelines_return_the_same_under_both_handoffs(tiny, tiny_at_32, dev, method, refiner, monkeypatch):
    """2 layouts (2 and 3 boxes, one phrase with two boxes), centred per-box generations aligned back, 64 x 64 latents;
    without a refiner (host box masks, uploaded once) and with a batched one that leaves ONE device tensor.  With the
    helpers' SAM network (tests/sam_cases.py) the run is the one tests/test_sam_batched_gpu.py makes — 32 x 32 latents,
    no alignment (its mid-block map is 4 x 4), the first layout twice: on other inputs that synthetic network leaves
    empty masks, which the host path refuses."""
    sm, lays = tiny
    calls = []
    real_run = handoff.run
    monkeypatch.setattr(pipeline.device_handoff, "run", lambda *a, **kw: calls.append(kw["align"]) or real_run(*a, **kw))
    if refiner == "sam":
        sm, lays, align = tiny_at_32, [lays[0], lays[0]], False
        kw = dict(num_inference_steps=6, height=8 * SAM_L, width=8 * SAM_L, decode=True, overall_loss_threshold=0.0,
                  overall_max_index_step=3)
        if method == "lmd":
            kw = dict(num_inference_steps=12, max_index_step=3, overall_max_index_step=3, so_center_box=False,
                      align_with_overall_bboxes=False, height=8 * SAM_L, width=8 * SAM_L)
    else:
        align = True
        kw = dict(num_inference_steps=6, height=8 * E2E_L, width=8 * E2E_L, decode=refiner != "none", so_center_box=True,
                  align_with_overall_bboxes=True, overall_loss_threshold=0.0, overall_max_index_step=3, overall_max_iter=[1])
        if method == "lmd":
            kw.update(loss_threshold=0.0, max_index_step=2, max_iter=[1], attn_aggregation_step_start=2)
    fn = pipeline.lmd_generate_batch if method == "lmd" else pipeline.lmd_plus_generate_batch
    host = fn(sm, lays, mask_refiner=_refiner(refiner, dev), handoff="host", **kw)
    assert calls == []
    device = fn(sm, lays, mask_refiner=_refiner(refiner, dev), handoff="device", **kw)
    assert calls == [align]
    assert len(host) == len(device) == 2
    for l, (h, d) in enumerate(zip(host, device)):
        assert d["composed"].is_cuda and d["fg_idx"].is_cuda and d["fg_idx"].dtype == torch.int64
        assert h["guidance_iters"] == d["guidance_iters"] and h["so_guidance_iters"] == d["so_guidance_iters"]
        assert int((d["fg_idx"] != 0).sum()) > 0
        _same_results(h, d, f"layout {l}")
    if method == "lmd_plus":
        assert all(len(d["so_latents_all"]) == lay.n_boxes for d, lay in zip(device, lays))


def test_none_takes_the_device_path_exactly_when_the_masks_are_device_tensors(tiny, dev, monkeypatch):
    sm, lays = tiny
    calls = []
    real_run = handoff.run
    monkeypatch.setattr(pipeline.device_handoff, "run", lambda *a, **kw: calls.append(1) or real_run(*a, **kw))
    kw = dict(num_inference_steps=4, height=8 * E2E_L, width=8 * E2E_L, so_center_box=True, align_with_overall_bboxes=True,
              overall_loss_threshold=0.0, overall_max_index_step=2, overall_max_iter=[1])
    pipeline.lmd_plus_generate_batch(sm, lays[:1], decode=False, **kw)
    assert calls == []
    pipeline.lmd_plus_generate_batch(sm, lays[:1], decode=True, mask_refiner=BatchedBoxMasks(E2E_L), **kw)
    assert calls == ([1] if handoff.DEFAULT_WITH_DEVICE_MASKS == "device" else [])
