"""The contracts of the two guidance-energy kernels (tests/energy_cases.py), checked where there is no GPU:

  * the tables are well formed, and every row meets the bit conditions of the reference (exact products and rankings for
    ca_energy; top-k gaps, arg-max leads and signs beyond their bounds or equal by construction for BoxDiff); the rows that
    are there for a tie have one;
  * an fp32 rendering of each kernel's arithmetic stays inside the derived bound on every row (the worst ratio is printed per
    kernel and kind), and every wrong answer of MUTATIONS falls outside;
  * every REFUSALS row answers LGD_ERR_ARG and every UNSUPPORTED row LGD_ERR_UNSUPPORTED through the library with placeholder
    pointers, before the device is touched; the optional operands stay optional;
  * the ops wrappers raise before the library is called;
  * the tables EnergyTables and BoxDiffTables build for the project's layouts are forms the rows cover.

test_accepted_calls_reach_the_launch makes calls the library accepts on placeholder pointers: it runs only on a host without a
GPU (there the launch fails with LGD_ERR_LAUNCH, the proof that every check was passed) and skips where one is present; on a
GPU machine the accepted forms are the rows of tests/test_energy_kernels_gpu.py."""
import functools
import os
import sys

import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import _lib, ops
from lgd_amd.energy import BoxDiffTables, EnergyTables

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_cases as ec  # noqa: E402

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
ERR_ARG, ERR_LAUNCH, ERR_UNSUPPORTED = -1, -2, -3
ROW_NAMES = sorted(ec.ROWS_BY_NAME)


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__ as ge
    ge.build()


@functools.lru_cache(maxsize=None)
def _reference(name):
    row = ec.ROWS_BY_NAME[name]
    return ec.reference(row, row.data())


def _answer(fn, change):
    return getattr(_lib.load(), fn)(*ec.call_args(fn, change))


# ---------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------
def _check_ca_tables(items, groups, n_items, n_groups, masks, map_hw, T, n_samples, *, mask_values):
    """the item layout of lgd_ca_energy_f32: [n][8], the items of a (map, image, token) column adjacent, the groups a partition
    of the items in order, one group per column, the columns sorted"""
    assert items.dtype == I32 and items.shape[1] == 8 and groups.dtype == I32 and groups.shape[1] == 2
    it, gr = items[:n_items].tolist(), groups[:n_groups].tolist()
    nxt, cols = 0, []
    for first, count in gr:
        assert first == nxt and count >= 1
        nxt += count
        col = {(r[0], r[7], r[2]) for r in it[first:first + count]}
        assert len(col) == 1
        cols.append(col.pop())
    assert nxt == n_items and len(set(cols)) == len(cols) and cols == sorted(cols)
    for mp, kind, tok, mid, k_fg, k_bg, rid, img in it:
        hw = int(map_hw[mp])
        assert kind in (0, 1, 2) and 0 <= tok < T and 0 <= mid < masks.shape[0] and 0 <= img < n_samples
        assert 1 <= k_fg <= hw and 1 <= k_bg <= hw
        assert set(masks[mid, :hw].tolist()) <= mask_values


def _check_bd_tables(items, groups, n_items, masks, side, T, max_items):
    assert items.dtype == I32 and items.shape[1] == 8 and groups.dtype == I32 and groups.shape[1] == 2
    nxt = 0
    for first, count in groups.tolist():
        assert first == nxt and 0 <= count <= max_items
        nxt += count
    assert nxt == n_items and tuple(masks.shape[1:]) == (3, side * side)
    for tok, mid, k_fg, k_bg, *rest in items[:n_items].tolist():
        assert 1 <= tok <= T - 2 and 0 <= mid < masks.shape[0] and 0 <= k_fg <= side * side and 0 <= k_bg <= side * side
        assert rest == [0, 0, 0, 0]
        assert set(masks[mid, 0].tolist()) <= {0.0, 0.5, 1.0} and set(masks[mid, 1:, :2 * side].reshape(-1).tolist()) <= {0.0, 1.0}


def test_the_tables_are_well_formed():
    assert set(ec.ARGS) == set(ec.BASE) == set(ec.RULES) == set(ec.OPTIONAL)
    labels = {}
    for fn, what, change in ec.REFUSALS + ec.UNSUPPORTED:
        assert set(change) <= {n[2:] if n.startswith("p:") else n for n in ec.ARGS[fn].split()}, (fn, what)
        assert what not in labels.setdefault(fn, set()), (fn, what)
        labels[fn].add(what)
    for fn, args in ec.ARGS.items():
        assert len(args.split()) == len(_lib.SIGNATURES[fn]), fn
        want = {f"{p} NULL" for p in ec.pointers(fn) if p not in ec.OPTIONAL[fn]} | {f"{p} off {ec.ALIGN[fn][p]} bytes" for p in ec.pointers(fn)}
        assert want <= labels[fn], (fn, sorted(want - labels[fn]))
    assert {"refs without dyn", "max_hw = 0", "T = 0", "refs_step_stride = -1"} <= labels["lgd_ca_energy_f32"]
    for row in ec.rows_of("ca_energy"):
        d, p = row.data(), row.p
        _check_ca_tables(d["items"], d["groups"], d["n_items"], d["n_groups"], d["masks"], d["map_hw"], p["T"], p["S"],
                         mask_values={0.0, 0.5, 1.0})
    for row in ec.rows_of("boxdiff"):
        d, p = row.data(), row.p
        _check_bd_tables(d["items"], d["groups"], d["n_items"], d["masks"], p["side"], p["T"], d["max_items"])
        assert ec.bd_lds(p["side"], d["max_items"]) <= ec.BD_LDS_BYTES
    # the shapes the rows are there for
    ca, bd = ec.rows_of("ca_energy"), ec.rows_of("boxdiff")
    assert {hw for r in ca for hw in r.hw} >= {7, 64, 256, 257, 576, 4096} and {r.H for r in ca} == {1, 3} and {r.T for r in ca} == {3, 77}
    assert {r.gscale for r in ca} == {1.0, 1024.0} and any(r.pad for r in ca) and any(r.dyn0 == 2 and r.gap for r in ca)
    orders = {tuple(k for k, _ in col[3]) for r in ca for col in r.cols if len(col[3]) == 3}
    assert orders >= {(0, 1, 2)[i:] + (0, 1, 2)[:i] for i in range(3)} | {(0, 2, 1), (2, 1, 0), (1, 0, 2)} | {(0, 1, 1)}
    assert {r.side for r in bd} == {2, 3, 16, 24, 32} and {r.T for r in bd} == {3, 64, 65, 77, 128}
    toks = {(r.T, t) for r in bd for objs in r.images for ts, _, _ in objs for t in ts}
    assert toks >= {(3, 1), (64, 62), (65, 63), (77, 63), (77, 64), (77, 75), (128, 63), (128, 64), (128, 126)}
    assert {(r.n_maps, r.H) for r in bd} >= {(1, 1), (5, 8)} and {r.smooth for r in bd} == {None, "gauss", "asym"}
    lds = sorted(ec.bd_lds(r.side, r.data()["max_items"]) for r in bd if r.side == 16)
    below = max(b for b in lds if b <= ec.LDS_DEFAULT)
    above = min(b for b in lds if b > ec.LDS_DEFAULT)
    assert above - below == 2 * 256 * 4 and lds[-1] + 2 * 256 * 4 > ec.BD_LDS_BYTES >= lds[-1]
    assert ec.bd_max_items(16) == 71 and ec.bd_max_items(32) == 15
    # the counts the k rows are there for, at a size past one pass of the block
    ks = lambda name: [(r[1], r[4], r[5]) for r in ec.ROWS_BY_NAME[name].data()["items"].tolist()]
    assert ec.ROWS_BY_NAME["ca_energy:kind0 k one"].hw[0] > 256 and ks("ca_energy:kind0 k one") == [(0, 1, 1)]
    both = ks("ca_energy:column 0 0 tied")
    assert both[1] == (0, 1, 1) and both[0][1] > 1 and both[0][2] > 1
    for name, which in (("ca_energy:kind0 k_fg the in-mask count", 4), ("ca_energy:kind0 k_bg the out-of-mask count", 5)):
        d = ec.ROWS_BY_NAME[name].data()
        m = d["masks"][0, :257]
        assert d["items"][0, which] == int(((m > 0) if which == 4 else (m < 1)).sum())
    with pytest.raises(ValueError):
        ec.ca_data(ec.Row("ca_energy", "an unknown k mode", cols=((0, 0, 5, ((0, "two"),)),)), torch.Generator().manual_seed(0))
    # every BoxDiff row at sides 2 and 3 (the token rows among them) drives the fg and the bg top-k gradient
    for r in bd:
        if r.side <= 3:
            assert all(k_fg >= 1 and k_bg >= 1 for _, _, k_fg, k_bg, *_ in r.data()["items"].tolist()), r.name


@pytest.mark.parametrize("name", ROW_NAMES)
def test_row_meets_the_conditions(name):
    row = ec.ROWS_BY_NAME[name]
    ref = _reference(name)
    cond = ref["_cond"]
    assert not cond.failed, cond.failed[:5]
    for out, (want, bound) in ec.outputs(ref).items():
        assert bool((bound >= 0).all()) and not bool(torch.isnan(bound).any()) and not bool(torch.isnan(want).any()), (name, out)
    if row.tie:
        assert cond.ties, f"{name} is there for a tie and has none"
    if "tied top-k and arg-max" in name:
        assert cond.ties == {"k", "argmax"}
    if "zeros selected" in name:                         # k reaches past the non-zero values of every head
        d = row.data()
        mp, _, tok, mid, k_fg, k_bg, _, img = d["items"][0].tolist()
        col, m = d["maps"][mp][img, :, :, tok], d["masks"][mid, :row.hw[mp]]
        assert k_fg > int(((col * m) != 0).sum(-1).max()) and k_bg > int(((col * (1 - m)) != 0).sum(-1).max())
    if "R equals A" in name:
        assert float(ref["partial"][0].abs().max()) == 0.0 and float(ref["loss"][0].abs().max()) == 0.0
        g = ref["gmap0"][0]
        assert float(g[g != ec.SENT].abs().max()) == 0.0
    if "middle without items" in name:
        assert float(ref["loss"][0][1]) == 0.0 and float(ref["loss"][1][1]) == 0.0
    if "no items" in name:
        assert float(ref["loss"][0].abs().max()) == 0.0 and bool((ref["gmap0"][0] == ec.SENT).all())


# ---------------------------------------------------------------------------------------------
# numerics
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("ca_energy", "boxdiff"))
def test_emulation_stays_inside_the_bound(entry):
    worst = {}
    for row in ec.rows_of(entry):
        d = row.data()
        ref, emu = ec.outputs(_reference(row.name)), ec.emulate(row, d)
        assert set(emu) == set(ref), row.name
        for out, (want, bound) in ref.items():
            r = ec.worst_ratio(emu[out].reshape(want.shape), want, bound, fp16=False)
            assert r < 1.0, (row.name, out, r)
            label = ec.kinds_of(row, d)
            worst[label] = max(worst.get(label, 0.0), r)
    for label, r in sorted(worst.items()):
        print(f"[emulation] {label}: worst error / bound {r:.3f}")
    print(f"[emulation] {entry}: worst error / bound {max(worst.values()):.3f}")
    assert ec.rows_of(entry)


@pytest.mark.parametrize("name", sorted(ec.MUTATIONS))
def test_wrong_answer_falls_outside(name):
    row_name, switch = ec.MUTATIONS[name]
    row = ec.ROWS_BY_NAME[row_name]
    ref = ec.outputs(_reference(row_name))
    wrong = ec.outputs(ec.reference(row, row.data(), **{switch: True}))
    r = max(ec.worst_ratio(wrong[out][0], want, bound, fp16=False) for out, (want, bound) in ref.items())
    print(f"[mutation] {name} on {row_name}: {r:.3e} of the bound")
    assert r > 1.0, name


def test_the_mutations_cover_the_list():
    assert len([n for n in ec.MUTATIONS if n.startswith("ca:")]) >= 12 and len([n for n in ec.MUTATIONS if n.startswith("boxdiff:")]) >= 10


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn,what,change", ec.REFUSALS, ids=[f"{f}:{w}" for f, w, _ in ec.REFUSALS])
def test_host_refusal(fn, what, change):
    assert _answer(fn, change) == ERR_ARG, (fn, what)


@pytest.mark.parametrize("fn,what,change", ec.UNSUPPORTED, ids=[f"{f}:{w}" for f, w, _ in ec.UNSUPPORTED])
def test_unsupported_stays_unsupported(fn, what, change):
    assert _answer(fn, change) == ERR_UNSUPPORTED, (fn, what)


def test_accepted_calls_reach_the_launch():
    """BASE, the optional operands left out (gmaps; smooth; refs together with dyn; dyn alone), the limits themselves and a
    launch without items pass every check (host without a GPU: the launch is reached and fails there)."""
    if torch.cuda.is_available():
        pytest.skip("the placeholder pointers would be launched on")
    for fn, change in ec.ACCEPTED:
        assert _answer(fn, change) == ERR_LAUNCH, (fn, change)


def _wrapper_faults():
    f = lambda *s: torch.zeros(*s, dtype=F32)
    i = lambda *s: torch.zeros(*s, dtype=I32)
    ptr = lambda n: torch.zeros(n, dtype=I64)

    def ca(**kw):
        a = dict(map_ptrs=ptr(1), gmap_ptrs=ptr(1), map_hw=i(1), items=i(3, 8), coefs=f(3, 4), masks=f(2, 256), refs=f(2, 1, 3, 256),
                 refs_step_stride=768, dyn=i(4), groups=i(2, 2), n_groups=2, n_items=3, H=3, T=77, max_hw=256, partial=f(9), loss=f(1))
        a.update(kw)
        return lambda: ops.ca_energy(**a)

    def bd(**kw):
        a = dict(map_ptrs=ptr(2), gmap_ptrs=ptr(2), n_maps=2, side=16, items=i(4, 8), masks=f(2, 3, 256), smooth=f(9), groups=i(1, 2),
                 n_samples=1, max_items=4, H=2, T=77, loss_scale=1.0, grad_scale=1.0, loss=f(1))
        a.update(kw)
        return lambda: ops.boxdiff_energy(**a)

    return [
        ("ca_energy: items count", ca(items=i(2, 8))), ("ca_energy: items dtype", ca(items=torch.zeros(3, 8, dtype=I64))),
        ("ca_energy: coefs count", ca(coefs=f(3, 3))), ("ca_energy: coefs dtype", ca(coefs=torch.zeros(3, 4, dtype=F64))),
        ("ca_energy: groups count", ca(groups=i(3, 2))), ("ca_energy: partial count", ca(partial=f(3))),
        ("ca_energy: loss count", ca(loss=f(2))), ("ca_energy: masks are no rows of max_hw", ca(masks=f(2, 250))),
        ("ca_energy: masks strided", ca(masks=f(2, 512)[:, :256])), ("ca_energy: refs without dyn", ca(dyn=None)),
        ("ca_energy: refs dtype", ca(refs=torch.zeros(768, dtype=F64))), ("ca_energy: refs below one reference", ca(refs=f(700))),
        ("ca_energy: dyn empty", ca(dyn=i(0))), ("ca_energy: map pointers dtype", ca(map_ptrs=i(1))),
        ("ca_energy: gmap pointers count", ca(gmap_ptrs=ptr(2))), ("ca_energy: map_hw count", ca(map_hw=i(2))),
        ("ca_energy: a table on another device", ca(coefs=torch.zeros(3, 4, dtype=F32, device="meta"))),
        ("boxdiff_energy: map pointers count", bd(map_ptrs=ptr(1))), ("boxdiff_energy: gmap pointers dtype", bd(gmap_ptrs=i(2))),
        ("boxdiff_energy: items are no [n][8] table", bd(items=i(30))), ("boxdiff_energy: masks are no [n][3][HW] table", bd(masks=f(2, 2, 256))),
        ("boxdiff_energy: smooth count", bd(smooth=f(3))), ("boxdiff_energy: smooth dtype", bd(smooth=torch.zeros(9, dtype=F64))),
        ("boxdiff_energy: groups count", bd(groups=i(2, 2))), ("boxdiff_energy: loss count", bd(loss=f(2))),
        ("boxdiff_energy: masks strided", bd(masks=f(2, 3, 512)[:, :, :256])),
        ("boxdiff_energy: a table on another device", bd(masks=torch.zeros(2, 3, 256, dtype=F32, device="meta"))),
    ]


_FAULTS = _wrapper_faults()


@pytest.mark.parametrize("what,call", _FAULTS, ids=[w for w, _ in _FAULTS])
def test_wrapper_check_raises_before_the_library(what, call, monkeypatch):
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail(f"{what}: the library was called"))
    with pytest.raises(RuntimeError):
        call()


def test_wrapper_accepts_what_the_tables_build(monkeypatch):
    """the checks pass on the project's own tables, placeholders of a launch without items included"""
    calls = []
    monkeypatch.setattr(ops, "_call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    t = _project_tables()
    dyn = torch.zeros(4, dtype=I32)
    for tab in t["ca"] + t["bd"]:
        maps = {k: torch.zeros(tab.n_samples, tab.heads, tab._map_hw[k] if hasattr(tab, "_map_hw") else tab.hw, tab.T) for k in tab.keys}
        tab.bind(maps, {k: torch.zeros_like(v) for k, v in maps.items()})
        tab.run(dyn, 1.0, True)
        tab.run(dyn, 1.0, False)
    assert len(calls) == 2 * len(t["ca"] + t["bd"])


# ---------------------------------------------------------------------------------------------
# the project's own tables are forms the rows cover
# ---------------------------------------------------------------------------------------------
def _project_tables():
    keys = [("down", 2, 0, 0), ("mid", 0, 0, 0), ("up", 1, 0, 0)]
    map_hw = {keys[0]: 256, keys[1]: 64, keys[2]: 256}
    boxes = [[(0.1, 0.2, 0.6, 0.7), (0.5, 0.5, 0.9, 0.95)], (0.0, 0.0, 0.4, 1.0)]
    pos = [[2, 3], [6]]
    ca = [EnergyTables("cpu", boxes, pos, keys, map_hw, 8, use_ratio_based_loss=False, ref_boxes=True),
          EnergyTables("cpu", boxes, pos, keys, map_hw, 8, use_ratio_based_loss=True, ref_boxes=True, ref_ca_last_token_only=False),
          EnergyTables("cpu", [], [], keys, map_hw, 8)]
    for t in ca[:2]:
        t.set_refs(torch.rand(3, t.n_refs, 8, t.max_hw))
    ca.append(EnergyTables.merged([ca[0], None, ca[1]]))
    bkeys = [keys[0], keys[2]]
    bd = [BoxDiffTables("cpu", boxes, pos, bkeys, map_hw, 8), BoxDiffTables("cpu", boxes, pos, bkeys, map_hw, 8, smooth_attentions=False)]
    bd.append(BoxDiffTables.merged([bd[0], None, bd[0]]))
    return {"ca": ca, "bd": bd}


def test_the_project_tables_are_covered_forms():
    t = _project_tables()
    ca_rows, bd_rows = ec.rows_of("ca_energy"), ec.rows_of("boxdiff")
    col_kinds = {tuple(k for k, _ in col[3]) for r in ca_rows for col in r.cols}
    for tab in t["ca"]:
        _check_ca_tables(tab.items, tab.groups, tab.n_items, tab.n_groups, tab.masks, tab.map_hw, tab.T, tab.n_samples, mask_values={0.0, 1.0})
        assert tab.masks.shape[1] == tab.max_hw and tab.partial.numel() == max(tab.n_items * tab.heads, 1) and tab.loss.numel() == tab.n_samples
        it = tab.items[:tab.n_items].tolist()
        for first, count in tab.groups[:tab.n_groups].tolist():
            kinds = tuple(r[1] for r in it[first:first + count])
            assert kinds in col_kinds, f"a column of kinds {kinds} is no row of energy_cases"
        if tab.refs is not None:
            assert tuple(tab.refs.shape[1:]) == (tab.n_refs, tab.heads, tab.max_hw)
    assert any(r.S == 3 and not any(c[1] == 1 for c in r.cols) for r in ca_rows) and any(not r.cols for r in ca_rows)
    assert any(len(r.hw) == 2 for r in ca_rows) and any(r.pad for r in ca_rows)
    for tab in t["bd"]:
        _check_bd_tables(tab.items, tab.groups, tab.n_items, tab.masks, tab.side, tab.T, tab.max_items)
        assert set(tab.masks[:, 0].reshape(-1).tolist()) <= {0.0, 1.0}
        assert tab.smooth is None or tab.smooth.numel() == 9
    assert any(len(r.images) == 3 and not r.images[1] for r in bd_rows)
