"""csrc/sam_tail.hip against the host code it replaces, on the same inputs.

Mask tail (lgd_sam_mask_tail_f32): the reference is `DeviceSamProcessor("cpu").post_process_masks`, the bilinear resize to
the latent grid with `.bool()`, `get_iou_with_resize` and `select_mask` (tests/sam_tail_cases.py) in fp32 on the CPU.
Candidates, the selected mask, areas, intersections, unions and the pick are equal EXACTLY; the confidence is the picked
entry of the model's IoU row.  Latent-grid pixels that an fp64 chain flips between the thresholds +1e-4 and -1e-4 are left
out; the test asserts that they are at most 0.1 % of a case (the seeded inputs have none).

Prompt kernel (lgd_sam_attn_prompt_f32): the reference is scipy.ndimage.gaussian_filter on float64, `preprocess_mask` and
np.unravel_index(argmax).  The smoothed map agrees within 1e-6 of its maximum (fp32 sums of 13 terms per axis against fp64;
first measured 1.81e-7 at worst); the point is exact (the inputs keep a relative gap >= 1e-3 between the two largest values,
asserted); mask pixels within 1e-4 of the threshold are left out, at most 0.1 % of a map."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import ndimage

pytestmark = pytest.mark.gpu

import lgd_amd  # noqa: E402,F401
import sam_cases  # noqa: E402
import sam_tail_cases as tc  # noqa: E402
from lgd_amd import _lib, ops, sam_refine  # noqa: E402

# (S, target, (h, w), grid)
SMALL = [(32, 128, (128, 128), (16, 16)), (32, 128, (96, 64), (12, 8)), (32, 128, (64, 96), (8, 12))]
PRODUCTION = (256, 1024, (512, 512), (64, 64))


def _coarse_shape(grid, quarter):
    return (grid[0] // 4, grid[1] // 4) if quarter else grid


def _below_iou(quarter):
    """On a coarse map of a few pixels the IoUs are small fractions (1/5 on a 3 x 2 map): a threshold that none of them
    comes within 1e-3 of."""
    return 0.22 if quarter else tc.BELOW_IOU


def _run(dev, logits, iou, geoms, target, grid, coarse, below_conf=tc.BELOW_CONF, below_iou=tc.BELOW_IOU):
    out = ops.sam_mask_tail(logits.to(dev), torch.from_numpy(iou).to(dev), torch.tensor(geoms, dtype=torch.int32).to(dev),
                            target, grid, torch.from_numpy(coarse).to(dev), below_conf, below_iou)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check(dev, logits, iou, geoms, target, grid, coarse, below_conf=tc.BELOW_CONF, below_iou=tc.BELOW_IOU):
    """One launch over all items against the host chain item by item -> the host results."""
    N, K = logits.shape[:2]
    mask, conf, stats, cand = _run(dev, logits, iou, geoms, target, grid, coarse, below_conf, below_iou)
    assert mask.shape == (N, *grid) and cand.shape == (N, K, *grid) and stats.shape == (N, 1 + 3 * K)
    assert set(np.unique(cand)) <= {0, 1} and set(np.unique(mask)) <= {0, 1}
    hosts = []
    for n in range(N):
        want = tc.host_candidates(logits[n], geoms[n], target, grid)
        amb = tc.ambiguous(logits[n], geoms[n], target, grid)
        n_amb = int(amb.sum())
        print(f"[sam tail] item {n} geom {geoms[n]} grid {grid} coarse {coarse.shape[1:]}: {n_amb} ambiguous of {amb.size}")
        assert n_amb <= tc.AMBIGUOUS_CAP * amb.size, (n, n_amb)
        assert np.array_equal(cand[n].astype(bool)[~amb], want[~amb]), (n, int((cand[n].astype(bool) != want)[~amb].sum()))
        # every confidence stays clear of its threshold: the comparison cannot hinge on a rounding
        assert np.abs(iou[n] - below_conf).min() >= 1e-3
        host = tc.host_select(want, iou[n], coarse[n], below_conf, below_iou)
        assert np.abs(host["ious"] - below_iou).min() >= 1e-3, host["ious"]
        hosts.append(host)
        got = dict(pick=int(stats[n, 0]), area=stats[n, 1:1 + K], inter=stats[n, 1 + K:1 + 2 * K], union=stats[n, 1 + 2 * K:])
        if n_amb == 0:
            for key in ("area", "inter", "union"):
                assert np.array_equal(got[key], host[key]), (n, key, got[key], host[key])
            assert got["pick"] == host["pick"], (n, got, host)
            assert np.array_equal(mask[n].astype(bool), host["mask"])
            assert conf[n] == host["conf"]
        else:                                                     # a pixel left out moves a count by at most one
            for key in ("area", "inter", "union"):
                assert np.abs(got[key] - host[key]).max() <= n_amb, (n, key, got[key], host[key])
        assert np.array_equal(mask[n], cand[n, got["pick"]]) and conf[n] == iou[n, got["pick"]]
    return hosts


def _iou_rows(N, seed):
    """Predicted IoUs on both sides of the confidence threshold, none within 1e-3 of it."""
    g = np.random.default_rng(seed)
    v = g.uniform(0.6, 0.99, size=(N, 3)).astype(np.float32)
    v[np.abs(v - tc.BELOW_CONF) < 2e-3] += 4e-3
    return v


@pytest.mark.parametrize("quarter", [False, True])
@pytest.mark.parametrize("case", range(len(SMALL)))
def test_mask_tail_one_item(dev, case, quarter):
    S, target, (h, w), grid = SMALL[case]
    hc, wc = _coarse_shape(grid, quarter)
    _check(dev, tc.make_logits(1, S, seed=10 + case), _iou_rows(1, case), [tc.geom_of(h, w, target)], target, grid,
           tc.box_coarse(hc, wc)[None], below_iou=_below_iou(quarter))


@pytest.mark.parametrize("quarter", [False, True])
@pytest.mark.parametrize("grid", [(16, 16), (12, 8)])
def test_mask_tail_three_geometries_in_one_launch(dev, grid, quarter):
    S, target = 32, 128
    geoms = [tc.geom_of(h, w, target) for _, _, (h, w), _ in SMALL]
    assert len({tuple(g) for g in geoms}) == 3
    hc, wc = _coarse_shape(grid, quarter)
    coarse = np.stack([tc.box_coarse(hc, wc), tc.box_coarse(hc, wc, (0.0, 0.0, 0.5, 1.0)), tc.box_coarse(hc, wc, (0.4, 0.4, 1.0, 1.0))])
    _check(dev, tc.make_logits(3, S, seed=20), _iou_rows(3, 7), geoms, target, grid, coarse, below_iou=_below_iou(quarter))


@pytest.mark.parametrize("quarter", [False, True])
def test_mask_tail_production_geometry(dev, quarter):
    """sam-vit-base: 256 x 256 logits, 1024 input side, 512 x 512 images, the 64 x 64 latent grid; LMD's coarse map is a
    quarter of that side."""
    S, target, (h, w), grid = PRODUCTION
    hc, wc = _coarse_shape(grid, quarter)
    coarse = np.stack([tc.box_coarse(hc, wc), tc.box_coarse(hc, wc, (0.1, 0.3, 0.6, 0.9))])
    _check(dev, tc.make_logits(2, S, seed=30), _iou_rows(2, 3), [tc.geom_of(h, w, target)] * 2, target, grid, coarse)


@pytest.fixture(scope="module")
def rule_inputs():
    """One 128 x 128 item on the 16 x 16 grid and its host candidates (nested: each offset shrinks the blob)."""
    S, target, (h, w), grid = SMALL[0]
    logits = tc.make_logits(1, S, seed=40)
    for k in range(1, 3):                                         # one blob, three levels
        logits[0, k] = logits[0, 0] + tc.OFFSETS[0] - tc.OFFSETS[k]
    geom = tc.geom_of(h, w, target)
    cand = tc.host_candidates(logits[0], geom, target, grid)
    area = cand.reshape(3, -1).sum(1)
    assert area[0] > area[1] > area[2] > 0, area
    return logits, geom, target, grid, cand


RULES = ["all_admissible", "largest_below_confidence", "all_below_coarse_iou", "equal_areas", "empty_candidate",
         "empty_coarse"]


@pytest.mark.parametrize("rule", RULES)
def test_mask_tail_selection_rules(dev, rule_inputs, rule):
    logits, geom, target, grid, cand = rule_inputs
    logits = logits.clone()
    iou = np.array([[0.9, 0.92, 0.94]], dtype=np.float32)
    coarse = cand[0].astype(np.uint8)
    if rule == "largest_below_confidence":
        iou[0, 0] = 0.5
    elif rule == "all_below_coarse_iou":
        coarse = (~cand[0]).astype(np.uint8)                     # disjoint from every (nested) candidate
        assert coarse.sum() > 0
    elif rule == "equal_areas":
        logits[0, 1] = logits[0, 0]
    elif rule == "empty_candidate":
        logits[0, 2] = -5.0
        iou[0] = (0.5, 0.6, 0.95)
    elif rule == "empty_coarse":
        coarse = np.zeros_like(coarse)
    host = _check(dev, logits, iou, [geom], target, grid, coarse[None])[0]
    want_pick = dict(all_admissible=0, largest_below_confidence=1, all_below_coarse_iou=0, equal_areas=0,
                     empty_candidate=0, empty_coarse=0)[rule]
    assert host["pick"] == want_pick, (rule, host)
    if rule == "all_admissible":
        assert (host["ious"] >= tc.BELOW_IOU).all()
    if rule in ("all_below_coarse_iou", "empty_coarse"):
        assert (host["ious"] < tc.BELOW_IOU).all() and (host["inter"] == 0).all()
    if rule == "equal_areas":
        assert host["area"][0] == host["area"][1]
    if rule == "empty_candidate":
        assert host["area"][2] == 0 and host["inter"][2] == 0 and host["union"][2] == coarse.sum()


def test_mask_tail_in_a_captured_graph_is_bit_identical(dev):
    S, target, (h, w), grid = SMALL[1]
    logits = tc.make_logits(3, S, seed=50).to(dev)
    iou = torch.from_numpy(_iou_rows(3, 5)).to(dev)
    geom = torch.tensor([tc.geom_of(hh, ww, target) for _, _, (hh, ww), _ in SMALL], dtype=torch.int32).to(dev)
    coarse = torch.from_numpy(np.stack([tc.box_coarse(3, 2)] * 3)).to(dev)
    maps = torch.from_numpy(np.stack(sam_cases.refine_inputs()[2])).to(dev)

    def both():
        return (*ops.sam_mask_tail(logits, iou, geom, target, grid, coarse, tc.BELOW_CONF, tc.BELOW_IOU),
                *ops.sam_attn_prompt(maps, 1.5, 0.25, 8, 8, want_smooth=True))
    eager = [t.clone() for t in both()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                                    # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = both()
    for t in captured:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


def _prompt_maps():
    big = sam_cases.refine_inputs()[2]
    return {"64x64": np.stack(big), "16x16": np.stack([tc.block_mean(a, 16, 16) for a in big]),
            "8x8": np.stack([tc.block_mean(a, 8, 8) for a in big]), "8x12": tc.block_mean(big[0][:, :48], 8, 12)[None]}


@pytest.mark.parametrize("sigma", [1.5, 0.1])
@pytest.mark.parametrize("name", ["64x64", "16x16", "8x8", "8x12"])
def test_attn_prompt_vs_scipy(dev, name, sigma):
    maps = _prompt_maps()[name]
    N, hm, wm = maps.shape
    up_w, up_h = 512 // wm, 512 // hm                             # sam_refine_attn's (w, h) naming
    coarse, points, smooth = ops.sam_attn_prompt(torch.from_numpy(maps).to(dev), sigma, 0.25, up_w, up_h, want_smooth=True)
    torch.cuda.synchronize()
    coarse, points, smooth = coarse.cpu().numpy(), points.cpu().numpy(), smooth.cpu().numpy()
    for n in range(N):
        want = ndimage.gaussian_filter(maps[n].astype(float), sigma=sigma)
        err = float(np.abs(smooth[n] - want).max() / np.abs(want).max())
        top = np.sort(want.ravel())[-2:]
        gap = float((top[1] - top[0]) / top[1])
        norm = (want - want.min()) / (want - want.min()).max()
        near = np.abs(norm - 0.25) < 1e-4
        print(f"[sam prompt] {name} sigma {sigma} map {n}: smooth err {err:.2e}, top-2 gap {gap:.2e}, {int(near.sum())} "
              f"pixels at the threshold")
        assert err <= 1e-6
        assert gap >= 1e-3
        peak_y, peak_x = np.unravel_index(want.argmax(), want.shape)
        assert points[n].tolist() == [float(peak_x * up_h), float(peak_y * up_w)]
        assert near.sum() <= 1e-3 * near.size
        want_mask = sam_refine.preprocess_mask(want, 0.25, n_erode_dilate_mask=0)
        assert np.array_equal(coarse[n].astype(bool)[~near], want_mask[~near])
    if sigma == 0.1:                                              # radius 0: the filter is the identity
        assert np.array_equal(smooth, maps)


def test_argument_checks(dev):
    lib = _lib.load()
    N, K, S, H, W = 1, 3, 32, 16, 16
    t = dict(logits=torch.zeros(N, 5, S, S), iou=torch.zeros(N, 5), geom=torch.tensor([[128, 128, 128, 128]], dtype=torch.int32),
             coarse=torch.zeros(N, H, W, dtype=torch.uint8), cand=torch.full((N, 5, H, W), 7, dtype=torch.uint8),
             mask=torch.full((N, H, W), 7, dtype=torch.uint8), conf=torch.full((N,), 7.0),
             stats=torch.full((N, 16), 7, dtype=torch.int32), ws=torch.full((4096,), 7, dtype=torch.int32))
    t = {k: v.to(dev) for k, v in t.items()}
    p = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}
    null = C.c_void_p(0)

    def tail(K=K, S=S, H=H, W=W, **over):
        q = dict(p, **over)
        return lib.lgd_sam_mask_tail_f32(q["logits"], q["iou"], q["geom"], q["coarse"], N, K, S, 128, H, W, H, W, 0.85, 0.2,
                                         q["cand"], q["mask"], q["conf"], q["stats"], q["ws"], null)
    before = {k: v.clone() for k, v in t.items()}
    for name in ("logits", "iou", "geom", "coarse", "mask", "conf", "stats", "ws"):
        assert tail(**{name: null}) == -1, name
    assert tail(K=5) == -1 and tail(K=0) == -1
    assert tail(S=0) == -1 and tail(H=0) == -1 and tail(W=0) == -1
    assert tail(H=8192) == -3

    a = torch.zeros(1, 8, 8, device=dev)
    co, pt = torch.full((1, 8, 8), 7, dtype=torch.uint8, device=dev), torch.full((1, 2), 7.0, device=dev)
    ap, cp, pp = (C.c_void_p(x.data_ptr()) for x in (a, co, pt))
    prompt = lib.lgd_sam_attn_prompt_f32
    assert prompt(null, 1, 8, 8, 1.5, 0.25, 64, 64, cp, pp, null, null) == -1
    assert prompt(ap, 1, 8, 8, 1.5, 0.25, 64, 64, null, pp, null, null) == -1
    assert prompt(ap, 1, 8, 8, 1.5, 0.25, 64, 64, cp, null, null, null) == -1
    assert prompt(ap, 1, 0, 8, 1.5, 0.25, 64, 64, cp, pp, null, null) == -1
    assert prompt(ap, 1, 8, 8, 0.0, 0.25, 64, 64, cp, pp, null, null) == -1
    assert prompt(ap, 1, 128, 128, 1.5, 0.25, 64, 64, cp, pp, null, null) == -3
    torch.cuda.synchronize()
    for k, v in t.items():                                        # nothing was launched: no operand changed
        assert torch.equal(v, before[k]), k
    assert bool((pt == 7).all()) and bool((co == 7).all())
