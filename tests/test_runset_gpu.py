"""lgd_amd.runset on the GPU.  batching="layout": an item's latents, image and iteration count are BIT-identical whether
it is generated alone on a new engine, in a set on one lane, on two lanes, by two ranks, or by a resumed run — every
launch shape is a function of the layout alone, and nothing a sampler keeps between calls reaches the next (the samplers
of the two-lane pool are used by one arm after another on purpose).  batching="share": a result equals the direct
`lmd_plus_generate_batch` call on the same chunk.  All engines here run the "throughput" GEMM table lanes.make_lanes gives
a multi-lane pool (the table is part of an engine's launch plans: the single-engine arms are given the same one)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import lgd_amd  # noqa: E402,F401
from lgd_amd import runset, weights  # noqa: E402
from lgd_amd.lanes import Lane, LanePool, make_lanes  # noqa: E402
from lgd_amd.pipeline import (CachedLayout, backward_guidance_generate_batch, lmd_generate_batch,  # noqa: E402
                              lmd_plus_generate_batch)
from lgd_amd.runset import Item, generate_set  # noqa: E402
from lgd_amd.sampler import LMDSampler  # noqa: E402
from lgd_amd.scheduler import DDIMScheduler  # noqa: E402
from lgd_amd.unet import UNetEngine  # noqa: E402
from lgd_amd.vae import HipVAEDecoder, synth_aekl_state_dict  # noqa: E402

L = 32
BOXES = [("a white deer", [74, 177, 183, 235]), ("a gray bear", [314, 193, 189, 216]), ("a red ball", [40, 60, 200, 180]),
         ("a blue cup", [250, 40, 120, 110])]
KW = dict(num_inference_steps=6, height=8 * L, width=8 * L, overall_loss_threshold=0.0, overall_max_index_step=3,
          overall_max_iter=[2])
FIELDS = ("latents", "image")
_S = {}


def _five_box_row():
    rows = runset.load_cache()
    return next(r for r in rows if len(r["gen_boxes"]) == 5)["gen_boxes"]


def _items():
    # 0, 1, 2, 3, 5, 2 boxes: other batch buckets, plans and guidance-loop lengths per item; distinct prompt indices
    boxes = [[], BOXES[:1], BOXES[:2], BOXES[1:4], [(n, b) for n, b in _five_box_row()], BOXES[2:4]]
    return [Item(ind, 0, len(b), b) for ind, b in zip((3, 5, 8, 13, 21, 34), boxes)]


def _make_layout(cfg):
    def make_layout(item, bg_seed, fg_seed_start):
        lay = CachedLayout.synthetic(cfg, item.payload, index=bg_seed)
        assert (lay.bg_seed, lay.fg_seed_start) == (bg_seed, fg_seed_start) == runset.seeds(item.ind, item.repeat)[:2]
        return lay
    return make_layout


def _new_lane(eng, make):
    """A lane of its own: a new engine on `eng`'s weights (what make_lanes builds for lane 1), nothing else shared."""
    e = UNetEngine(eng.cfg, eng.device, text_len=eng.text_len, max_text_batch=eng.max_text_batch, weights=eng.w)
    e.tuning_mode = "throughput"
    return Lane(0, make(e), torch.cuda.Stream(device=eng.device))


def setup(dev):
    if not _S:
        cfg = weights.CONFIGS["tiny_gligen"]
        eng = UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0))
        vae_sd = synth_aekl_state_dict(seed=0)
        make = lambda e: LMDSampler(e, DDIMScheduler(), vae=HipVAEDecoder(vae_sd, dev))      # noqa: E731
        items = _items()
        alone = []
        for it in items:                                   # (a) each item alone, on a lane nothing else ever ran on
            out = generate_set([_new_lane(eng, make)], [it], _make_layout(cfg), decode=True, **KW)
            alone.append(out[0])
        _S.update(cfg=cfg, eng=eng, make=make, items=items, alone=alone, lanes=make_lanes(eng, 2, make), dev=dev)
    return _S


def _same(got, want, what):
    assert got["guidance_iters"] == want["guidance_iters"], f"{what}: guidance_iters"
    for k in FIELDS:
        a, b = torch.as_tensor(got[k]), torch.as_tensor(want[k])
        assert torch.isfinite(a.float()).all()
        assert a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), f"{what}: {k} differs"


def _check(s, outs, what):
    assert [o["ind"] for o in outs] == [it.ind for it in s["items"]]
    for o, ref in zip(outs, s["alone"]):
        _same(o, ref, f"{what}, item {o['ind']}")


def test_alone_arm_is_sound(dev):
    s = setup(dev)
    assert [o["ind"] for o in s["alone"]] == [3, 5, 8, 13, 21, 34]
    iters = [o["guidance_iters"] for o in s["alone"]]
    assert iters[0] == 0 and all(i > 0 for i in iters[1:])         # guidance ran wherever there are boxes
    assert len({o["latents"].cpu().numpy().tobytes() for o in s["alone"]}) == 6
    assert s["alone"][4]["image"].shape == (8 * L, 8 * L, 3)


@pytest.mark.parametrize("n_lanes", [1, 2])
def test_layout_mode_set_equals_items_alone(dev, n_lanes):
    """(b), (c): the whole set on one lane and on two."""
    s = setup(dev)
    lanes_used = set()
    with LanePool(s["lanes"][:n_lanes], device=dev) as pool:
        outs = generate_set(pool, s["items"], _make_layout(s["cfg"]), decode=True, min_layouts_per_lane=1,
                            sink=lambda item, res: lanes_used.add(res["lane"]), **KW)
    assert lanes_used == set(range(n_lanes))
    _check(s, outs, f"{n_lanes} lane(s)")


def test_layout_mode_two_ranks_equal_items_alone(dev):
    """(d): the union of rank 0 and rank 1 of a world of two (one after the other on the same pool)."""
    s = setup(dev)
    with LanePool(s["lanes"], device=dev) as pool:
        parts = [generate_set(pool, s["items"], _make_layout(s["cfg"]), decode=True, min_layouts_per_lane=1, rank=r, world=2,
                              **KW) for r in range(2)]
    assert all(parts) and all(o["rank"] == r for r, p in enumerate(parts) for o in p)
    _check(s, sorted(parts[0] + parts[1], key=lambda o: o["ind"]), "two ranks")


def test_layout_mode_resumed_run_equals_items_alone(dev):
    """(e): a run that skips three items, then a run that skips the other three."""
    s = setup(dev)
    first = {3, 13, 34}
    with LanePool(s["lanes"], device=dev) as pool:
        a = generate_set(pool, s["items"], _make_layout(s["cfg"]), decode=True, min_layouts_per_lane=1,
                         skip=lambda it: it.ind not in first, **KW)
        b = generate_set(pool, s["items"], _make_layout(s["cfg"]), decode=True, min_layouts_per_lane=1,
                         skip=lambda it: it.ind in first, **KW)
    assert [o is not None for o in a] == [it.ind in first for it in s["items"]]
    assert [o is None for o in b] == [o is not None for o in a]
    _check(s, [x if x is not None else y for x, y in zip(a, b)], "resumed run")


def test_share_mode_equals_the_direct_call_on_the_same_chunk(dev):
    s = setup(dev)
    make_layout = _make_layout(s["cfg"])
    with LanePool(s["lanes"][:1], device=dev) as pool:
        outs = generate_set(pool, s["items"], make_layout, batching="share", group=2, decode=True, **KW)
    chunks = [s["items"][i:i + 2] for i in range(0, 6, 2)]
    with LanePool([_new_lane(s["eng"], s["make"])], device=dev) as pool:
        direct = pool.map(lambda lane, ch: lmd_plus_generate_batch(
            lane.sampler, [make_layout(it, *runset.seeds(it.ind)[:2]) for it in ch], decode=True, **KW), chunks)
    flat = [o for d in direct for o in d]
    worst = 0.0
    for o, d, ref in zip(outs, flat, s["alone"]):
        _same(o, d, f"share mode, item {o['ind']}")
        a, b = o["latents"].float().cpu(), ref["latents"].float().cpu()
        worst = max(worst, float((a - b).abs().max() / b.abs().max()))
    # reported, not gated: what sharing UNet calls with a neighbour does to an image (DESIGN.md d)
    print(f"[runset] share mode (group=2) vs layout mode: largest relative latent difference {worst:.3e}")


@pytest.mark.parametrize("method,direct", [("lmd", lmd_generate_batch), ("backward_guidance", backward_guidance_generate_batch)])
def test_other_methods_layout_mode_equals_the_direct_call(dev, method, direct):
    cfg = weights.CONFIGS["tiny"]
    if "tiny_lane" not in _S:
        eng = UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0))
        _S["tiny_lane"] = Lane(0, LMDSampler(eng, DDIMScheduler()), torch.cuda.Stream(device=dev))
    items = [Item(4, 0, 2, BOXES[:2]), Item(9, 1, 1, BOXES[2:3])]
    make_layout = lambda it, bg, fg: CachedLayout.synthetic(cfg, it.payload, index=bg)      # noqa: E731
    kw = dict(num_inference_steps=4, height=8 * L, width=8 * L, loss_threshold=0.0, max_index_step=2, max_iter=[1] if method == "lmd" else 1)
    if method == "lmd":
        kw.update(overall_loss_threshold=0.0, overall_max_index_step=2, overall_max_iter=[1])
    with LanePool([_S["tiny_lane"]], device=dev) as pool:
        want = pool.map(lambda lane, it: direct(lane.sampler, [make_layout(it, *runset.seeds(it.ind, it.repeat)[:2])],
                                                decode=False, **kw)[0], items)
        got = generate_set(pool, items, make_layout, method=method, decode=False, **kw)
    for g, w, it in zip(got, want, items):
        assert (g["ind"], g["repeat"]) == (it.ind, it.repeat) and g["guidance_iters"] > 0
        assert g["guidance_iters"] == w["guidance_iters"]
        assert torch.isfinite(g["latents"]).all() and torch.equal(g["latents"], w["latents"])
    assert not torch.equal(got[0]["latents"], got[1]["latents"])


def test_full_width_set_two_lanes_equal_one_lane_reversed(dev):
    """BASELINE config[3] at its own width: five layouts of the packaged cache (0, 1, 2, 3 and 5 boxes) on the sd14_gligen
    network, 3 steps, through two lanes, and through one lane in the reverse order."""
    cfg = weights.CONFIGS["sd14_gligen"]
    rows = runset.load_cache()
    inds = [next(i for i, r in enumerate(rows) if len(r["gen_boxes"]) == n) for n in (0, 1, 2, 3, 5)]
    items = runset.cache_items(rows, inds)
    eng = UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0))
    lanes = make_lanes(eng, 2, lambda e: LMDSampler(e, DDIMScheduler()))
    kw = dict(num_inference_steps=3, overall_loss_threshold=0.0, overall_max_index_step=2, overall_max_iter=[1], decode=False,
              min_layouts_per_lane=1)
    make_layout = runset.synthetic_layouts(cfg)
    used = set()
    with LanePool(lanes, device=dev) as pool:
        two = generate_set(pool, items, make_layout, sink=lambda it, res: used.add(res["lane"]), **kw)
    with LanePool(lanes[:1], device=dev) as pool:
        one = generate_set(pool, items[::-1], make_layout, **kw)
    assert used == {0, 1}
    assert [o["ind"] for o in two] == [o["ind"] for o in one] == inds
    for a, b, it in zip(two, one, items):
        assert a["guidance_iters"] == b["guidance_iters"] and (a["guidance_iters"] > 0) == (it.n_boxes > 0)
        assert torch.isfinite(a["latents"]).all()
        assert torch.equal(a["latents"], b["latents"]), f"item {it.ind} ({it.n_boxes} boxes)"
