"""lgd_amd.runset without a GPU: seeds, the cost model and partition against bench.py's own, the plan's completeness and
balance, the resumable directory sink, the call grouping of `generate_set` on stub lanes with a stub method, and the
command line's --dry-run."""
import importlib.util
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import lgd_amd  # noqa: E402,F401
from lgd_amd import runset  # noqa: E402
from lgd_amd.runset import DirectorySink, Item, generate_set, plan  # noqa: E402


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod_runset", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_seeds_follow_generate_py():
    assert runset.seeds(7) == (7, 123456796, 7897)
    assert runset.seeds(7, repeat_ind=2, seed_offset=5) == (13590, 123470379, 21480)
    assert runset.seeds(7, ind_override=100, regenerate_ind=1) == (56889, 123456796, 64779)


def test_cost_and_partition_equal_bench(bench):
    cache = bench.load_cache()
    assert runset.load_cache() == cache
    assert runset.select(len(cache), 100, spread=True) == bench.select_prompts(cache, 100)
    assert runset.select(len(cache), 40, skip_first=30) == list(range(30, 70))
    for n in range(0, 9):
        for steps in (50, 20, 7):
            a, b = runset.layout_cost(n, steps), bench.layout_cost(n, steps)
            assert abs(a - b) <= 1e-9 * abs(b), (n, steps, a, b)
        assert abs(runset.layout_cost(n, 50, 0.3, 40, 7) - bench.layout_cost(n, 50, 0.3, 40, 7)) <= 1e-9 * bench.layout_cost(n)
    for sel in (bench.select_prompts(cache, 100), list(range(len(cache)))):
        costs = [runset.layout_cost(len(cache[i]["gen_boxes"])) for i in sel]
        for world in (1, 2, 4, 8):
            assert runset.partition_by_cost(costs, world) == bench.partition_by_cost(costs, world)
    ties = [3.0, 1.0, 3.0, 2.0, 2.0, 1.0, 3.0, 2.0, 1.0, 1.0, 0.0, 0.0]
    for parts in (1, 2, 3, 5, 12, 13):
        got = runset.partition_by_cost(ties, parts)
        assert got == bench.partition_by_cost(ties, parts)
        assert sorted(i for p in got for i in p) == list(range(len(ties)))
    assert runset.partition_by_cost(ties, 3)[0][0] == 0            # ties: the lower index first, into the lower bin
    for n in (0, 3, 8, 12, 13, 31, 32, 50, 400):
        for mx in (1, 2, 4):
            for per in (1, 8):
                assert runset.lanes_for(n, mx, per) == bench.lanes_for("lmd_v0.1", n, mx, per)


def test_plan_is_complete_deterministic_and_balanced():
    rows = runset.load_cache()
    items = runset.cache_items(rows, range(len(rows)))
    pl = plan(items, world=8, max_lanes=4)
    seen = sorted(p for r in range(8) for k in range(pl.lanes(r)) for p in pl.share(r, k))
    assert seen == list(range(400))
    assert pl.shares == plan(items, world=8, max_lanes=4).shares
    rank_load = [sum(pl.costs[p] for p in pl.rank_share(r)) for r in range(8)]
    assert max(rank_load) / (sum(rank_load) / 8) <= 1.02, rank_load
    for r in range(8):
        assert pl.lanes(r) == 4
        lane_load = [sum(pl.costs[p] for p in pl.share(r, k)) for k in range(4)]
        assert max(lane_load) / (sum(lane_load) / 4) <= 1.05, (r, lane_load)
        for k in range(4):
            assert pl.share(r, k) == sorted(pl.share(r, k))
    # 100 prompts over 8 ranks: 12-13 per rank is one lane, not four lanes of three
    small = plan(runset.cache_items(rows, runset.select(len(rows), 100, spread=True)), world=8, max_lanes=4)
    assert [small.lanes(r) for r in range(8)] == [1] * 8


def _image(seed):
    return np.random.default_rng(seed).integers(0, 256, (16, 16, 3), dtype=np.uint8)


def test_directory_sink_names_resume_rule_and_threads(tmp_path):
    from PIL import Image
    sink = DirectorySink(tmp_path, repeats=2)
    a0, a1 = Item(5, 0), Item(5, 1)
    assert not sink.skip(a0)
    (tmp_path / "5").mkdir()
    (tmp_path / "5" / "part_0_1_1").write_bytes(b"half an image")        # a leftover temporary file counts for nothing
    assert not sink.skip(a0)
    sink(a0, dict(image=_image(0)))
    assert sorted(os.listdir(tmp_path / "5")) == ["img_0.png", "part_0_1_1"]
    assert not sink.skip(a0) and not sink.skip(a1)                         # fewer than `repeats` images
    sink(a1, dict(image=_image(1)[None]))                                   # (1, h, w, 3) as well
    assert sink.skip(a0) and sink.skip(a1)
    assert DirectorySink(tmp_path, repeats=3).skip(a0) is False
    assert np.array_equal(np.asarray(Image.open(tmp_path / "5" / "img_1.png")), _image(1))
    with pytest.raises(ValueError):
        sink(Item(6, 0), dict(image=None))

    one = DirectorySink(tmp_path / "t")
    errors = []

    def write(lo):
        try:
            for i in range(lo, lo + 20):
                one(Item(i, 0), dict(image=_image(i)))
        except BaseException as e:                                          # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=write, args=(lo,)) for lo in (0, 20)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for i in range(40):
        assert os.listdir(tmp_path / "t" / str(i)) == ["img_0.png"] and one.skip(Item(i, 0))
        assert np.array_equal(np.asarray(Image.open(tmp_path / "t" / str(i) / "img_0.png")), _image(i))


# ---- generate_set on stub lanes ------------------------------------------------------------------------------------------
N_BOXES = [2, 0, 5, 1, 3, 2, 2, 0, 1, 4]


def _items():
    return [Item(10 + i, 0, n, ("payload", i)) for i, n in enumerate(N_BOXES)]


class Stub:
    def __init__(self, fail_on=None):
        self.calls, self.made, self.sunk, self.fail_on = [], [], [], fail_on
        self.lock = threading.Lock()

    def make_layout(self, item, bg_seed, fg_seed_start):
        assert (bg_seed, fg_seed_start) == runset.seeds(item.ind, item.repeat, 3)[:2]
        with self.lock:
            self.made.append(item.ind)
        return item.ind

    def method(self, sampler, lays, *, decode, tag):
        assert sampler is None and decode == "device" and tag == "kw"
        with self.lock:
            self.calls.append((threading.current_thread().name, list(lays)))
        if self.fail_on in lays:
            raise RuntimeError(f"boom at {self.fail_on}")
        return [dict(image=None, value=100 * ind) for ind in lays]

    def sink(self, item, result):
        with self.lock:
            self.sunk.append((result["lane"], item.ind, result["value"]))


def _run(stub, n_lanes=2, **kw):
    from lgd_amd.lanes import Lane
    lanes = [Lane(i, None) for i in range(n_lanes)]
    return generate_set(lanes, _items(), stub.make_layout, method=stub.method, sink=stub.sink, min_layouts_per_lane=1,
                        seed_offset=3, tag="kw", **kw)


def _expected_shares(n_lanes, positions=None):
    items = _items()
    pos = list(range(len(items))) if positions is None else positions
    costs = [runset.layout_cost(items[p].n_boxes) for p in pos]
    return [[items[pos[j]].ind for j in sh] for sh in runset.partition_by_cost(costs, n_lanes)]


@pytest.mark.parametrize("batching,group", [("layout", None), ("share", 2), ("share", None)])
def test_generate_set_call_grouping(batching, group):
    stub = Stub()
    out = _run(stub, batching=batching, group=group)
    shares = _expected_shares(2)
    assert shares == [[_items()[p].ind for p in plan(_items(), max_lanes=2, min_layouts_per_lane=1).share(0, k)] for k in range(2)]
    want = []
    for sh in shares:
        size = 1 if batching == "layout" else (group or len(sh))
        want += [sh[i:i + size] for i in range(0, len(sh), size)]
    assert sorted(c for _, c in stub.calls) == sorted(want)
    for k, sh in enumerate(shares):                                # a lane = one thread; its calls and sinks in share order
        names = {n for n, c in stub.calls if c[0] in sh}
        assert len(names) == 1
        assert [i for _, c in stub.calls if c[0] in sh for i in c] == sh
        assert [ind for lane, ind, _ in stub.sunk if lane == k] == sh == sorted(sh)
    assert [o["ind"] for o in out] == [it.ind for it in _items()]
    for o in out:
        assert o["value"] == 100 * o["ind"] and o["repeat"] == 0 and o["rank"] == 0 and o["lane"] in (0, 1)


def test_generate_set_ranks_cover_the_set_and_skip_comes_first():
    stub = Stub()
    halves = [_run(stub, rank=r, world=2) for r in range(2)]
    assert sorted(o["ind"] for h in halves for o in h) == [it.ind for it in _items()]
    assert all(o["rank"] == r for r, h in enumerate(halves) for o in h)
    assert [sorted(o["ind"] for o in h) for h in halves] == _expected_shares(2)      # the rank split is the plan's

    stub, asked = Stub(), []
    hidden = {11, 12, 17}

    def skip(item):
        asked.append(item.ind)
        return item.ind in hidden
    out = _run(stub, skip=skip)
    assert sorted(asked) == [it.ind for it in _items()]            # once per item
    assert not hidden & set(stub.made) and sorted(stub.made) == sorted(set(range(10, 20)) - hidden)
    assert [o is None for o in out] == [it.ind in hidden for it in _items()]
    left = [p for p, it in enumerate(_items()) if it.ind not in hidden]
    assert sorted(sorted(i for lane, i, _ in stub.sunk if lane == k) for k in range(2)) == sorted(_expected_shares(2, left))


def test_generate_set_exception_after_earlier_items_were_sunk():
    shares = _expected_shares(2)
    victim = shares[1][2]
    stub = Stub(fail_on=victim)
    with pytest.raises(RuntimeError, match=f"boom at {victim}"):
        _run(stub)
    sunk1 = [ind for lane, ind, _ in stub.sunk if lane == 1]
    assert sunk1 == shares[1][:2]                                  # what finished before it, nothing of or after it
    assert sum(1 for _, c in stub.calls if c == [victim]) == 1      # nothing is retried
    with pytest.raises(ValueError):
        _run(Stub(), batching="rank")
    with pytest.raises(ValueError):
        generate_set([], [], None, method="sd")


def test_cli_dry_run_prints_the_plan_and_imports_no_device_code():
    probe = ("import json, runpy, sys\n"
             "sys.argv = [sys.argv[1]] + sys.argv[2:]\n"
             "try:\n"
             "    runpy.run_path(sys.argv[0], run_name='__main__')\n"
             "except SystemExit as e:\n"
             "    assert not e.code, e.code\n"
             "print(json.dumps(sorted(m for m in sys.modules if m == 'torch' or m.startswith('lgd_amd'))))\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-c", probe, os.path.join(ROOT, "scripts", "generate_set.py"), "--synthetic", "--dry-run",
                        "--num-prompts", "40", "--lanes", "4"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("{", "["))]
    got, modules = json.loads(lines[0]), json.loads(lines[1])
    assert modules == ["lgd_amd", "lgd_amd.runset"]                # no torch, no engine, no library binding
    rows = runset.load_cache()
    items = runset.cache_items(rows, range(40))
    pl = plan(items, world=1, max_lanes=4, costs=[runset.layout_cost(it.n_boxes, 50) for it in items])
    assert got["shares"] == pl.shares and got["lanes"] == [4] and got["world"] == 1
    assert got["items"] == [[it.ind, it.repeat, it.n_boxes] for it in items]
    env["WORLD_SIZE"] = "2"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "generate_set.py"), "--dry-run", "--num-prompts", "40",
                        "--lanes", "4", "--spread"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    items = runset.cache_items(rows, runset.select(len(rows), 40, spread=True))
    assert json.loads(r.stdout)["shares"] == plan(items, world=2, max_lanes=4).shares
