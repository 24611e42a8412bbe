"""CPU suite for the device hand-off between the two stages of LMD / LMD+ (lgd_amd/handoff.py): everything except the
kernels.  The three ops of csrc/handoff.hip are replaced by the torch / numpy restatement of tests/handoff_cases.py, which
resolves the address tables back to the tensors they point into — so the packing (addresses, strides, rows, sides), the
layout segments, the per-layout views and the `handoff` keyword are checked against the host path, on the reference's own
golden (tests/golden/align_host.npz) and on seeded layouts.  The kernels against the same host path:
tests/test_handoff_gpu.py."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import lgd_amd  # noqa: F401
import handoff_cases as hc
from lgd_amd import _lib, handoff, ops, pipeline
from lgd_amd.hostprep import proportion_to_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "align_host.npz")
GOLD_KEYS = [("mid", 0, 0, 0), ("up", 1, 0, 0), ("up", 1, 1, 0), ("up", 1, 2, 0)]
GOLD_SIDES = {k: (8 if k[0] == "mid" else 16) for k in GOLD_KEYS}
BOXES_XYWH = [[74, 177, 183, 235], [314, 193, 189, 216], [20, 300, 120, 150]]
BBOXES = [[x / 512, y / 512, (x + w) / 512, (y + h) / 512] for x, y, w, h in BOXES_XYWH]


def test_three_symbols_are_declared_bound_and_built_without_contraction():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lgd_hip.h")).read(), flags=re.S)
    for name, nargs in (("lgd_handoff_place", 12), ("lgd_handoff_compose_f32", 15), ("lgd_handoff_ref_maps_f32", 12)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs == len(_lib.SIGNATURES[name]), name
    import importlib.util
    spec = importlib.util.spec_from_file_location("lgd_build_for_test", os.path.join(ROOT, "llm-groundeddiffusion_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "handoff.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA_FLAGS["handoff.hip"]
    for fn in ("handoff_place", "handoff_compose", "handoff_ref_maps"):
        assert callable(getattr(ops, fn))


def test_how_the_keyword_resolves():
    assert handoff.resolve("host", True) == "host" and handoff.resolve("host", False) == "host"
    assert handoff.resolve("device", True) == "device" and handoff.resolve("device", False) == "device"
    assert handoff.resolve(None, False) == "host"
    assert handoff.resolve(None, True) == handoff.DEFAULT_WITH_DEVICE_MASKS == "device"
    with pytest.raises(ValueError):
        handoff.resolve("gpu", True)
    for fn in (pipeline.lmd_plus_generate_batch, pipeline.lmd_generate_batch):
        assert inspect.signature(fn).parameters["handoff"].default is None


def test_the_module_reads_nothing_back():
    src = open(os.path.join(ROOT, "llm-groundeddiffusion_amd", "handoff.py")).read()
    code = re.sub(r'""".*?"""', "", src, flags=re.S)
    code = "\n".join(line.split("#")[0] for line in code.splitlines())
    for word in (".cpu(", ".item(", ".tolist(", ".numpy(", "synchronize"):
        assert word not in code, word


def test_pack_tables_keeps_shapes_types_values_and_alignment():
    arrays = [np.arange(5, dtype=np.int32), np.zeros((0, 2), dtype=np.int64), np.array([[1.5, -2.25]], dtype=np.float64),
              np.arange(6, dtype=np.int64).reshape(1, 2, 3) * (1 << 40), np.array([7], dtype=np.int32)]
    out = handoff.pack_tables(arrays, torch.device("cpu"))
    want = (torch.int32, torch.int64, torch.float64, torch.int64, torch.int32)
    for a, t, dt in zip(arrays, out, want):
        assert t.dtype == dt and tuple(t.shape) == a.shape and np.array_equal(t.numpy(), a)
        assert t.numel() == 0 or t.data_ptr() % 8 == 0


def test_masks_as_one_takes_rows_of_one_tensor_as_they_lie_and_stacks_the_rest():
    dev = torch.device("cpu")
    whole = torch.rand(4, 16, 16) > 0.5
    one = handoff.masks_as_one([whole[n] for n in range(4)], 16, dev)
    assert one.dtype == torch.uint8 and one.data_ptr() == whole.data_ptr() and torch.equal(one.bool(), whole)
    part = handoff.masks_as_one([whole[n] for n in (1, 2)], 16, dev)
    assert part.data_ptr() == whole[1].data_ptr() and torch.equal(part.bool(), whole[1:3])
    mixed = handoff.masks_as_one([whole[2], whole[0], whole[3].clone()], 16, dev)
    assert torch.equal(mixed.bool(), whole[[2, 0, 3]])
    floats = handoff.masks_as_one([whole[0].float() * 3, whole[1].float()], 16, dev)
    assert floats.dtype == torch.uint8 and torch.equal(floats.bool(), whole[:2])
    assert tuple(handoff.masks_as_one([], 16, dev).shape) == (0, 16, 16)
    with pytest.raises(ValueError):
        handoff.masks_as_one([whole[0, :8]], 16, dev)


def _golden_stage_a(g):
    so = pipeline._centered_so_boxes(hc.Lay(BBOXES), True, horizontal_center_only=False,
                                     vertical_placement="floor_padding", floor_padding=0.2)
    d = dict(latents_all=[torch.from_numpy(g[f"lall{i}"]) for i in range(3)],
             masks=[proportion_to_mask(b, 64, 64).bool() for b in so],
             saved=[{k: torch.from_numpy(g[f"saved_{i}_{ki}"]) for ki, k in enumerate(GOLD_KEYS)} for i in range(3)])
    return d, torch.from_numpy(g["bg"])


@pytest.mark.parametrize("horizontal_shift_only", [False, True])
def test_run_on_the_reference_golden(monkeypatch, horizontal_shift_only):
    """The reference's own utilities (oracle/make_golden_align.py): 3 boxes, L = 64, 4 keys, 3 steps."""
    g = np.load(GOLD)
    t = "h" if horizontal_shift_only else "xy"
    d, bg = _golden_stage_a(g)
    stand_in = hc.Restated(d["latents_all"] + [v for s in d["saved"] for v in s.values()])
    for fn in ("handoff_place", "handoff_compose", "handoff_ref_maps"):
        monkeypatch.setattr(ops, fn, getattr(stand_in, fn))
    out = handoff.run("cpu", masks=[d["masks"]], targets=[BBOXES], histories=[d["latents_all"]], saved=[d["saved"]],
                      bgs=[bg], keys=GOLD_KEYS, L=64, T=3, steps=3, align=True,
                      horizontal_shift_only=horizontal_shift_only, heads=2, max_hw=256)
    assert stand_in.calls == ["place", "compose", "ref_maps"] and len(out) == 1
    r = out[0]
    assert tuple(r["composed"].shape) == (4, 1, 4, 64, 64) and np.array_equal(r["composed"].numpy(), g[f"composed_{t}"])
    assert r["fg_idx"].dtype == torch.int64 and np.array_equal(r["fg_idx"].numpy(), g[f"fg_idx_{t}"])
    assert tuple(r["ref_maps"].shape) == (3, 3, 4, 2, 256)
    for b in range(3):
        for ki, k in enumerate(GOLD_KEYS):
            hw = GOLD_SIDES[k] ** 2
            want = g[f"shifted_{t}_{b}_{ki}"]                                        # [T, 1, heads, HW, 1]
            assert np.array_equal(r["ref_maps"][:, b, ki, :, :hw].numpy(), want[:, 0, :, :, 0]), (b, k)
            assert not r["ref_maps"][:, b, ki, :, hw:].any()
    # and the host path itself, field by field
    host = hc.host_path([hc.Lay(BBOXES)], [d], [bg], keys=GOLD_KEYS, L=64, T=3, steps=3, align=True,
                        horizontal_shift_only=horizontal_shift_only, sampler=hc.HostSampler(GOLD_SIDES))[0]
    assert hc.same(r["composed"], host["composed"]) and hc.same(r["fg_idx"], host["fg_idx"])
    assert hc.same(r["ref_maps"], host["ref_maps"])
    assert len(r["latents_all"]) == 3 and all(hc.same(a, b) for a, b in zip(r["latents_all"], host["latents_all"]))
    assert [tuple(row) for row in r["plan"][:, :2].numpy()] == host["offsets"]


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("chunks", [1, 2])
def test_run_segments_three_layouts_and_returns_views_per_layout(monkeypatch, align, chunks):
    """0, 1 and 5 boxes in one call; histories are strided views of one or two batch tensors and hold more rows than the
    composition takes; the saved maps hold fewer rows than T."""
    masks, targets = hc.random_layouts(11)
    lays, per_lay, bgs, batches = hc.stage_a(masks, targets, seed=3, hist_rows=hc.STEPS + 3, map_rows=hc.T - 1, chunks=chunks)
    assert len(batches) == chunks and not per_lay[2]["latents_all"][0].is_contiguous()
    stand_in = hc.Restated(batches + [v for d in per_lay for s in d["saved"] for v in s.values()])
    for fn in ("handoff_place", "handoff_compose", "handoff_ref_maps"):
        monkeypatch.setattr(ops, fn, getattr(stand_in, fn))
    out = handoff.run("cpu", masks=[d["masks"] for d in per_lay], targets=targets,
                      histories=[d["latents_all"] for d in per_lay], saved=[d["saved"] for d in per_lay], bgs=bgs,
                      keys=hc.KEYS, L=hc.L, T=hc.T, steps=hc.STEPS, align=align, horizontal_shift_only=False,
                      heads=hc.HEADS, max_hw=256)
    host = hc.host_path(lays, per_lay, bgs, align=align, horizontal_shift_only=False)
    assert stand_in.calls == ["place", "compose", "ref_maps"]
    for l, (r, h, n) in enumerate(zip(out, host, (0, 1, 5))):
        assert tuple(r["composed"].shape) == (hc.STEPS + 1, 1, hc.C, hc.L, hc.L) and tuple(r["plan"].shape) == (n, 8)
        assert hc.same(r["composed"], h["composed"]) and hc.same(r["fg_idx"], h["fg_idx"]), l
        assert tuple(r["ref_maps"].shape) == (hc.T, n, 2, hc.HEADS, 256)
        if n:
            assert hc.same(r["ref_maps"], h["ref_maps"]), l
            assert not r["ref_maps"][hc.T - 1:].any()                                # the maps ran one step short
        assert len(r["latents_all"]) == n and all(hc.same(a, b) for a, b in zip(r["latents_all"], h["latents_all"]))
        assert [tuple(row) for row in r["plan"][:, :2].numpy()] == h["offsets"]
        if not align:                                                                # the given views, untouched
            assert all(a is b for a, b in zip(r["latents_all"], per_lay[l]["latents_all"]))
    assert hc.same(out[0]["composed"][0], bgs[0]) and not out[0]["composed"][1:].any() and not out[0]["fg_idx"].any()


def test_run_without_reference_maps_makes_two_calls_and_refuses_what_the_host_refuses(monkeypatch):
    masks, targets = hc.random_layouts(5, counts=(2,))
    lays, per_lay, bgs, batches = hc.stage_a(masks, targets, seed=8)
    stand_in = hc.Restated(batches)
    for fn in ("handoff_place", "handoff_compose", "handoff_ref_maps"):
        monkeypatch.setattr(ops, fn, getattr(stand_in, fn))
    kw = dict(masks=[per_lay[0]["masks"]], targets=targets, histories=[per_lay[0]["latents_all"]], saved=[per_lay[0]["saved"]],
              bgs=bgs, keys=hc.KEYS, L=hc.L, T=hc.T, align=True, horizontal_shift_only=True)
    out = handoff.run("cpu", steps=hc.STEPS, **kw)
    assert stand_in.calls == ["place", "compose"] and out[0]["ref_maps"] is None
    host = hc.host_path(lays, per_lay, bgs, align=True, horizontal_shift_only=True)[0]
    assert hc.same(out[0]["composed"], host["composed"]) and hc.same(out[0]["fg_idx"], host["fg_idx"])
    with pytest.raises(ValueError):                                                  # a history shorter than the composition
        handoff.run("cpu", steps=hc.STEPS + 1, **kw)
    bad = dict(kw, saved=[[{k: v[:, :, :, :36] for k, v in s.items()} for s in per_lay[0]["saved"]]])
    with pytest.raises((AssertionError, ValueError)):                                # a 6 x 6 map: shift_tensor asserts
        handoff.run("cpu", steps=hc.STEPS, heads=hc.HEADS, max_hw=256, **bad)
