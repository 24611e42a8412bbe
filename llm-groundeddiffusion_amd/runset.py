"""A whole prompt set through stage 2: cost-balanced shares over ranks and lanes, seeds from the global prompt index,
resumable output.

The reference walks its prompt list one `run(spec)` after another (generate.py:239-404) and is sharded by hand
(`--skip_first_prompts/--num_prompts`, generate.py:23-25,243-250).  Here the set is described once (`Item`s), shared out
by cost (`plan`: longest-processing-time first over the ranks, then over each rank's lanes — SURVEY.md 8e) and generated
by `generate_set`, one `*_generate_batch` call of lgd_amd.pipeline after another on every lane of a `lanes.LanePool`.

Two batchings:
  * "layout" (the default): every item is its own call.  All launch shapes are then a function of the layout alone, so
    an item's result is bit-identical whatever the number of ranks and lanes, the order, a resumed run or the item alone.
  * "share": one call per `group` consecutive items of a lane's share (None: the whole share).  Layouts of a call share
    UNet launches — fewer, fuller calls — and the GEMM tiles follow the batch (DESIGN.md d), so a result depends on what
    it was batched with: it equals the direct `*_generate_batch` call on the same chunk, nothing more.

Seeds follow generate.py:226-229,317-344 (`seeds`); the resume rule and the file names are the reference's
(`DirectorySink`: generate.py:275-278, vis.display).  Importable without a GPU: planning, seeds and the sink are plain
Python; device modules are imported by the functions that launch.
"""
import os
import threading
from dataclasses import dataclass, field
from typing import Any, List

# analytic 2*MAC TFLOP of one UNet call (sd14_gligen, 64x64 latents) —
# (CFG forward B=2 with the GLIGEN fuser on, off; guidance forward to up.1.2 + dgrad to the latents with it on, off)
TF_SD14_GLIGEN = (2.2736, 1.6065, 0.5872 + 0.6885, 0.4086 + 0.4585)

LARGE_CONSTANT, LARGE_CONSTANT2, LARGE_CONSTANT3, LARGE_CONSTANT4 = 123456789, 56789, 6789, 7890    # generate.py:226-229

METHODS = ("lmd_plus", "lmd", "backward_guidance", "boxdiff")


# ---- cost model and partition --------------------------------------------------------------------------------------------
def layout_cost(n_boxes, n_steps=50, beta=0.4, iters_on=55, iters_off=10, tf=TF_SD14_GLIGEN):
    """Cost of one layout = its algorithmic TFLOP: N + 1 generations (int(beta x steps) of them with the
    GLIGEN fuser on), plus the guidance iterations of the overall stage — which exist only when the layout has boxes
    (generation/lmd_plus.py:418-470).  tf: (main on, main off, guidance on, guidance off) TFLOP of one UNet call."""
    main_on, main_off, guide_on, guide_off = tf
    if n_boxes == 0:
        iters_on = iters_off = 0
    n_on = int(beta * n_steps)
    return (n_boxes + 1) * (n_on * main_on + (n_steps - n_on) * main_off) + iters_on * guide_on + iters_off * guide_off


def partition_by_cost(costs, parts):
    """Longest-processing-time-first assignment of items (cost_i) to `parts` bins; deterministic (ties: the lower item
    index first, into the lower bin).  Returns per-bin lists of item indices (ascending)."""
    load = [0.0] * parts
    mine = [[] for _ in range(parts)]
    for i in sorted(range(len(costs)), key=lambda i: (-costs[i], i)):
        r = min(range(parts), key=lambda r: (load[r], r))
        load[r] += costs[i]
        mine[r].append(i)
    return [sorted(m) for m in mine]


def lanes_for(n_items, max_lanes, min_layouts_per_lane=8):
    """Lanes a rank uses for `n_items` layouts: a lane with only a few layouts runs small, badly filled UNet calls, so a
    lane is only added per `min_layouts_per_lane` layouts."""
    return max(1, min(max_lanes, n_items // max(1, min_layouts_per_lane)))


def seeds(ind, repeat_ind=0, seed_offset=0, ind_override=None, regenerate_ind=0):
    """(bg_seed, fg_seed_start, refine_seed) of prompt `ind` (the GLOBAL index: generate.py counts skipped prompts too),
    generate.py:317-344,384.  A prompt's own `seed` (ind_override) replaces the index in the background seed only."""
    base = ind if ind_override is None else ind_override + regenerate_ind * LARGE_CONSTANT2
    off = repeat_ind * LARGE_CONSTANT3 + seed_offset
    bg_seed = base + off
    return bg_seed, ind + off + LARGE_CONSTANT, bg_seed + LARGE_CONSTANT4


# ---- the set and its plan ----------------------------------------------------------------------------------------------
@dataclass
class Item:
    """One image of the set.  ind: global prompt index; repeat: generate.py's repeat_ind; n_boxes: what the cost model
    reads; payload: whatever `make_layout` needs (a spec dict, a cache row, a gen_boxes list)."""
    ind: int
    repeat: int = 0
    n_boxes: int = 0
    payload: Any = None


@dataclass
class Plan:
    """shares[rank][lane] = ascending positions (into the item list) of what that lane generates."""
    shares: List[List[List[int]]]
    costs: List[float] = field(default_factory=list)

    @property
    def world(self):
        return len(self.shares)

    def lanes(self, rank):
        return len(self.shares[rank])

    def share(self, rank, lane):
        return list(self.shares[rank][lane])

    def rank_share(self, rank):
        return sorted(i for sh in self.shares[rank] for i in sh)

    def as_dict(self):
        return dict(world=self.world, lanes=[self.lanes(r) for r in range(self.world)], shares=self.shares,
                    rank_cost=[round(sum(self.costs[i] for sh in rk for i in sh), 3) for rk in self.shares])


def plan(items, *, world=1, max_lanes=4, min_layouts_per_lane=8, costs=None):
    """Pure and deterministic: LPT over the ranks, then LPT over the lanes `lanes_for` gives each rank."""
    items = list(items)
    costs = [layout_cost(it.n_boxes) for it in items] if costs is None else [float(c) for c in costs]
    if len(costs) != len(items):
        raise ValueError(f"{len(costs)} costs for {len(items)} items")
    if world < 1 or max_lanes < 1:
        raise ValueError("world and max_lanes must be at least 1")
    shares = []
    for mine in partition_by_cost(costs, world):
        n_lanes = lanes_for(len(mine), max_lanes, min_layouts_per_lane)
        shares.append([[mine[j] for j in sh] for sh in partition_by_cost([costs[i] for i in mine], n_lanes)])
    return Plan(shares, costs)


# ---- generation ----------------------------------------------------------------------------------------------------------
def _method(method):
    if callable(method):
        return method
    if method not in METHODS:
        raise ValueError(f"method={method!r}: one of {', '.join(METHODS)}")
    from . import pipeline
    return getattr(pipeline, f"{method}_generate_batch")


def _chunks(share, batching, group):
    if batching == "layout":
        return [[p] for p in share]
    if batching != "share":
        raise ValueError(f"batching={batching!r}: \"layout\" or \"share\"")
    if group is None:
        return [share] if share else []
    if int(group) < 1:
        raise ValueError("group must be at least 1 (or None: the whole share)")
    return [share[i:i + int(group)] for i in range(0, len(share), int(group))]


def generate_set(lanes, items, make_layout, *, method="lmd_plus", batching="layout", group=None, rank=0, world=1, skip=None,
                 sink=None, decode="device", min_layouts_per_lane=8, costs=None, seed_offset=0, **method_kwargs):
    """Generates this rank's part of `items` on `lanes` (a lanes.LanePool, or a sequence of lanes.Lane: a pool is then made
    for the call) and returns its results in ascending (ind, repeat) order, None for a skipped item.

    make_layout(item, bg_seed, fg_seed_start) -> pipeline.CachedLayout.  method: one of METHODS (the `*_generate_batch`
    function of lgd_amd.pipeline), or such a function itself; method_kwargs go to it unchanged, except that `mask_refiner`
    may be a callable lane -> refiner (a refiner's state is per lane).  make_layout receives the first two of
    `seeds(item.ind, item.repeat, seed_offset)`; a prompt's own seed override is its payload's business.

    The ranks split the whole set by cost (so every rank computes the same split whatever is on disk); `skip(item)` is then
    asked once per item of this rank, before any work for it, and what remains is split over the lanes — with nothing
    skipped, `plan(items, world=world, max_lanes=len(lanes), ...)`'s shares of this rank.  sink(item, result)
    runs on the lane's thread as soon as the item's call returns — it must be thread-safe; result = the method's dict plus
    ind, repeat, rank, lane.  The first exception of an item reaches the caller as LanePool.map delivers it; what finished
    before it has been sunk, lanes start no further call after it, nothing is retried."""
    from .lanes import LanePool
    items = list(items)
    fn = _method(method)
    _chunks([], batching, group)                                  # refuse bad arguments before anything runs
    costs = [layout_cost(it.n_boxes) for it in items] if costs is None else [float(c) for c in costs]     # as plan()
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} of {world}")
    mine = partition_by_cost(costs, world)[rank]
    todo = [p for p in mine if not (skip is not None and skip(items[p]))]
    pool = lanes if isinstance(lanes, LanePool) else LanePool(list(lanes))
    try:
        n_lanes = lanes_for(len(todo), len(pool), min_layouts_per_lane)
        shares = [[todo[j] for j in sh] for sh in partition_by_cost([costs[p] for p in todo], n_lanes)]
        results = {}
        failed = threading.Event()
        refiner_of = method_kwargs.pop("mask_refiner", None)
        per_lane_refiner = callable(refiner_of) and not hasattr(refiner_of, "box")

        def run_share(lane, k):
            kw = dict(method_kwargs)
            if refiner_of is not None:
                kw["mask_refiner"] = refiner_of(lane) if per_lane_refiner else refiner_of
            for chunk in _chunks(shares[k], batching, group):
                if failed.is_set():
                    return
                try:
                    lays = [make_layout(items[p], *seeds(items[p].ind, items[p].repeat, seed_offset)[:2]) for p in chunk]
                    outs = fn(lane.sampler, lays, decode=decode, **kw)
                    for p, out in zip(chunk, outs):
                        res = dict(out, ind=items[p].ind, repeat=items[p].repeat, rank=rank, lane=lane.index)
                        if sink is not None:
                            sink(items[p], res)
                        results[p] = res
                except BaseException:
                    failed.set()
                    raise
        pool.map(run_share, list(range(n_lanes)), pin=list(range(n_lanes)))
    finally:
        if pool is not lanes:
            pool.close()
    return [results.get(p) for p in sorted(mine, key=lambda p: (items[p].ind, items[p].repeat))]


# ---- resumable output ----------------------------------------------------------------------------------------------------
class DirectorySink:
    """{save_dir}/{ind}/img_{repeat}.png — the name vis.display(output, "img", repeat_ind, save_ind_in_filename=False)
    gives (generate.py:386) — written under a temporary name that does not start with "img" and renamed, so that a
    directory never holds half an image under a name the resume rule counts.  `skip` is that rule (generate.py:275-278): the
    directory exists and holds at least `repeats` names that start with "img".  A device image is copied to the host here."""

    def __init__(self, save_dir, repeats=1):
        self.save_dir = str(save_dir)
        self.repeats = int(repeats)

    def img_dir(self, item):
        return os.path.join(self.save_dir, str(item.ind))

    def path(self, item):
        return os.path.join(self.img_dir(item), f"img_{item.repeat}.png")

    def skip(self, item):
        d = self.img_dir(item)
        return os.path.isdir(d) and len([n for n in os.listdir(d) if n.startswith("img")]) >= self.repeats

    def __call__(self, item, result):
        import numpy as np
        from PIL import Image
        image = result["image"]
        if image is None:
            raise ValueError("DirectorySink needs decoded images (decode=True or decode=\"device\")")
        if hasattr(image, "detach"):
            image = image.detach().cpu().numpy()
        image = np.asarray(image)
        if image.ndim == 4 and image.shape[0] == 1:
            image = image[0]
        if image.dtype != np.uint8 or image.ndim != 3:
            raise ValueError(f"an image is uint8 (h, w, 3); got {image.dtype} {image.shape}")
        d = self.img_dir(item)
        os.makedirs(d, exist_ok=True)
        tmp = os.path.join(d, f"part_{item.repeat}_{os.getpid()}_{threading.get_ident()}")
        try:
            with open(tmp, "wb") as fh:
                Image.fromarray(image).save(fh, format="PNG")
            os.replace(tmp, self.path(item))
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)


# ---- the packaged cache as a set, and ready-made pools ---------------------------------------------------------------
CACHE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "layouts_lmd_v0.1_gpt-4.json")


def load_cache(path=None):
    """The rows of a stage-1 layout cache (prompt, gen_boxes, bg_prompt, neg_prompt); by default the packaged 400 layouts
    of the reference's lmd_v0.1 benchmark."""
    import json
    with open(path or CACHE) as fh:
        return json.load(fh)


def select(n_rows, num_prompts=None, skip_first=0, spread=False):
    """Global prompt indices of a run.  The reference's window (generate.py:243-250): rows skip_first .. skip_first +
    num_prompts - 1.  spread: num_prompts rows taken evenly from the whole file, whose prompt categories are stored in
    blocks — the selection of `bench.py --workload lmd_v0.1`."""
    if spread:
        n = min(n_rows if num_prompts is None else int(num_prompts), n_rows)
        return [(i * n_rows) // n for i in range(n)]
    stop = n_rows if num_prompts is None else min(n_rows, skip_first + int(num_prompts))
    return list(range(min(skip_first, n_rows), stop))


def cache_items(rows, indices, repeats=1):
    """One Item per selected row and repeat, in ascending (ind, repeat) order; payload = the row."""
    return [Item(i, r, len(rows[i]["gen_boxes"]), rows[i]) for i in sorted(indices) for r in range(int(repeats))]


def synthetic_layouts(cfg, height=None, width=None):
    """make_layout for cache rows with a synthetic text side (pipeline.CachedLayout.synthetic: seeded CLIP states, SURVEY.md
    8d), as bench.py builds its layouts.  The states are seeded by the background seed, so repeats differ."""
    side = 8 * cfg.sample_size

    def make_layout(item, bg_seed, fg_seed_start):
        from .pipeline import CachedLayout
        lay = CachedLayout.synthetic(cfg, [(n, b) for n, b in item.payload["gen_boxes"]], index=bg_seed,
                                     height=height or side, width=width or side)
        lay.bg_seed, lay.fg_seed_start = bg_seed, fg_seed_start
        return lay
    return make_layout


def synthetic_lanes(cfg, device, n_lanes, *, rank=0, broadcast=False, decode=True, max_batch=8, max_batch_guided=8, seed=0):
    """`n_lanes` lanes on seeded random weights of architecture `cfg` (no checkpoint needed), as bench.py sets them up (its
    defaults of 8 images per unguided and per guided UNet call included):
    rank 0 makes the weights, with `broadcast` the other ranks receive the two arenas (dist.broadcast_weights); every lane
    decodes with its own copy of the same seeded VAE.  Every engine runs the "throughput" GEMM table whatever `n_lanes` is,
    so that an image does not depend on the lane count."""
    from . import dist as ldist, weights
    from .lanes import make_lanes
    from .sampler import LMDSampler
    from .scheduler import DDIMScheduler
    from .unet import UNetEngine
    from .vae import HipVAEDecoder, synth_aekl_state_dict
    mb = max(1, int(max_batch))
    mbg = max(1, min(int(max_batch_guided), mb))
    eng = UNetEngine(cfg, device, weights.synth_state_dict(cfg, seed) if rank == 0 or not broadcast else None,
                     max_text_batch=max(32, 2 * mb))
    if broadcast:
        ldist.broadcast_weights(eng.w, src=0)
    vae_sd = synth_aekl_state_dict(seed=seed) if decode else None

    def make_sampler(e):
        return LMDSampler(e, DDIMScheduler(prediction_type=cfg.prediction_type),
                          vae=HipVAEDecoder(vae_sd, device) if decode else None, max_batch=mb, max_batch_guided=mbg)
    lanes = make_lanes(eng, n_lanes, make_sampler)
    for ln in lanes:
        # the GEMM table is part of an engine's launch plans, and make_lanes picks it by the lane count: a resumed run with
        # one lane left must launch what the four-lane run launched, so the shared-GPU table holds for every count
        ln.engine.tuning_mode = "throughput"
    return lanes
