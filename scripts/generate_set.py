#!/usr/bin/env python
"""Generate a prompt set with lgd_amd.runset: cost-balanced shares over ranks and lanes, resumable output.

    python scripts/generate_set.py --synthetic --num-prompts 12 --steps 4 --save-dir out/run0
    python -m torch.distributed.run --nproc-per-node 8 scripts/generate_set.py --synthetic --save-dir out/run0

Writes {save-dir}/{prompt index}/img_{repeat}.png; a prompt directory that already holds its images is skipped, so an
interrupted run is continued by running the same command again.  With --batching layout (the default) an image does not
depend on how the set was split; --batching share is faster and gives up exactly that (lgd_amd/runset.py).

One process per GPU: under torch.distributed.run the rank and the world size come from the environment (lgd_amd.dist) and
rank 0's weights are broadcast; the script starts no ranks itself.  --synthetic: seeded random weights and a synthetic text
side (no checkpoints needed).  Without it the drop-in must be importable (`models`, `generation`: run from a checkout of the
reference with lgd_amd's dropin/ in front) and the Hugging Face checkpoints present; that path
runs one lane per process.  --dry-run prints the plan as JSON and imports no device code.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cache", default=None, help="stage-1 layout cache (default: the packaged lmd_v0.1 layouts)")
    ap.add_argument("--run-model", default="lmd_plus", choices=["lmd_plus", "lmd", "backward_guidance", "boxdiff"])
    ap.add_argument("--num-prompts", type=int, default=None)
    ap.add_argument("--skip-first-prompts", type=int, default=0)
    ap.add_argument("--spread", action="store_true", help="take --num-prompts rows evenly from the cache (bench.py's selection)")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--seed-offset", type=int, default=0)
    ap.add_argument("--save-dir", default=None)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--min-layouts-per-lane", type=int, default=8)
    ap.add_argument("--batching", default="layout", choices=["layout", "share"])
    ap.add_argument("--group", type=int, default=None, help="items per call with --batching share (default: the whole share)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--config", default=None, help="architecture of --synthetic weights (default: the method's, as bench.py)")
    ap.add_argument("--dry-run", action="store_true")
    args = ap.parse_args(argv)
    if not args.dry_run and not args.save_dir:
        ap.error("--save-dir is needed (or --dry-run)")
    if not 1 <= args.lanes <= 16:
        ap.error("--lanes: 1 .. 16 (lanes are host threads)")
    return args


def main(argv=None):
    args = parse_args(argv)
    import lgd_amd  # noqa: F401
    from lgd_amd import runset
    rows = runset.load_cache(args.cache)
    items = runset.cache_items(rows, runset.select(len(rows), args.num_prompts, args.skip_first_prompts, args.spread), args.repeats)
    costs = [runset.layout_cost(it.n_boxes, args.steps) for it in items]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.dry_run:
        pl = runset.plan(items, world=world, max_lanes=args.lanes, min_layouts_per_lane=args.min_layouts_per_lane, costs=costs)
        print(json.dumps(dict(pl.as_dict(), items=[[it.ind, it.repeat, it.n_boxes] for it in items])))
        return 0

    import torch
    from lgd_amd import dist as ldist
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    ldist.pin_rank(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)), lanes=args.lanes)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        ldist.init(backend="nccl")
    rank, world = ldist.rank(), ldist.world()
    sink = runset.DirectorySink(args.save_dir, args.repeats)
    mine = runset.partition_by_cost(costs, world)[rank]
    n_lanes = runset.lanes_for(sum(1 for p in mine if not sink.skip(items[p])), args.lanes, args.min_layouts_per_lane)
    kw = dict(num_inference_steps=args.steps)
    if args.synthetic:
        from lgd_amd import weights
        cfg = weights.CONFIGS[args.config or {"backward_guidance": "sd21", "lmd": "sd15", "boxdiff": "sd15"}.get(args.run_model, "sd14_gligen")]
        lanes = runset.synthetic_lanes(cfg, dev, n_lanes, rank=rank, broadcast=world > 1)
        make_layout = runset.synthetic_layouts(cfg)
        kw.update(height=8 * cfg.sample_size, width=8 * cfg.sample_size)
    else:
        lanes, make_layout, more = checkpoint_lanes(args, dev)
        kw.update(more)
    from lgd_amd.lanes import LanePool
    with LanePool(lanes, device=dev) as pool:
        out = runset.generate_set(pool, items, make_layout, method=args.run_model, batching=args.batching, group=args.group,
                                  rank=rank, world=world, skip=sink.skip, sink=sink, decode="device",
                                  min_layouts_per_lane=args.min_layouts_per_lane, costs=costs, seed_offset=args.seed_offset, **kw)
    done = sum(o is not None for o in out)
    print(json.dumps(dict(rank=rank, world=world, lanes=len(lanes), generated=done, skipped=len(out) - done,
                          save_dir=args.save_dir)))
    ldist.shutdown()
    return 0


def checkpoint_lanes(args, dev):
    """Real checkpoints through the drop-in's loader (generate.py:104-127) — one lane: the VAE and the SAM refiner of
    `model_dict` exist once.  Unpinned: no checkpoint has been loaded by this project's tests."""
    import torch
    try:
        import models
        from generation import _common
        from models import sam
    except ImportError as e:
        raise SystemExit("without --synthetic the drop-in (`models`, `generation`) must be importable: run from a checkout of "
                         f"the reference with lgd_amd's dropin/ in front of it ({e})")
    from lgd_amd.lanes import Lane
    gligen = args.run_model == "lmd_plus"
    models.sd_key = "gligen/diffusers-generation-text-box" if gligen else "runwayml/stable-diffusion-v1-5"
    models.sd_version = "sdv1.4" if gligen else "sdv1.5"
    models.model_dict = models.load_sd(key=models.sd_key, use_fp16=True)
    more = {}
    if args.run_model in ("lmd", "lmd_plus"):
        models.model_dict.update(sam.load_sam())
        more["mask_refiner"] = _common.sam_refiner(models.model_dict, 512, 512, discourage_mask_below_coarse_iou=0.25)

    def make_layout(item, bg_seed, fg_seed_start):
        row = item.payload
        spec = dict(prompt=row["prompt"], gen_boxes=row["gen_boxes"], bg_prompt=row["bg_prompt"],
                    extra_neg_prompt=row.get("neg_prompt", ""))
        return _common.build_layout(spec, bg_seed, fg_seed_start, _common.DEFAULT_SO_NEGATIVE_PROMPT,
                                    _common.DEFAULT_OVERALL_NEGATIVE_PROMPT)
    return [Lane(0, models.model_dict.sampler, torch.cuda.Stream(device=dev))], make_layout, more


if __name__ == "__main__":
    sys.exit(main())
