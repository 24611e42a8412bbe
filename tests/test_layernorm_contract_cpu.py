"""The LayerNorm launch contract and the norm variant table, checked where there is no GPU:

  * lgd_norm_variant enumerated to its end is the LGD_GN_* / LGD_LN_* macros of include/lgd_hip.h, and ops.GN_VARIANTS /
    ops.LN_VARIANTS are that table;
  * lgd_layernorm_plan answers, for every width, for row counts on both sides of every threshold, under both states of
    "ln_stream" and with the option passed as an argument, what the threshold table below says;
  * the three entry points refuse with exactly LGD_ERR_ARG, before the device is touched (a launch attempt on a host
    without a GPU would answer LGD_ERR_LAUNCH).  Only refused calls are made: the pointers are placeholders."""
import ctypes as C
import os
import re

import pytest

import lgd_amd  # noqa: F401
from lgd_amd import _lib, ops

P = 1 << 20                                             # an aligned placeholder address, never dereferenced
FWD, STATS, BWD = ops.LN_OP_FWD, ops.LN_OP_STATS, ops.LN_OP_BWD
# the thresholds of ln_plan (csrc/norm.hip), written out: (widest C served, code, rows per workgroup)
ROW_KERNELS = [(512, 514, 16), (1024, 524, 16), (1536, 532, 8), (2560, 550, 4)]
STREAM_KERNELS = [(320, 608, 128), (640, 616, 64), (1280, 632, 32), (2560, 664, 8)]
BWD_KERNEL = (2560, 700, 4)
STREAM_ELEMS = 8 << 20                                  # statistics only: the streaming kernel from this many elements


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__ as ge
    ge.build()
    yield
    ops.set_option("ln_stream", 1)


def expected(op, rows, width, stream):
    if width % 8 or width > 2560 or rows < 1:
        return -1
    pick = lambda table: next(code for widest, code, _ in table if width <= widest)
    if op == BWD:
        return BWD_KERNEL[1]
    if op == STATS:
        if stream and (rows * width >= STREAM_ELEMS or width > 1536):
            return pick(STREAM_KERNELS)
        if width > 1536:
            return -1
    return pick(ROW_KERNELS)


def test_the_variant_table_is_the_header():
    lib = _lib.load()
    code, name, rows = C.c_int(), C.create_string_buffer(128), []
    while lib.lgd_norm_variant(len(rows), C.byref(code), name, len(name)) == 0:
        assert 0 < len(name.value) < len(name) - 1
        rows.append((code.value, name.value.decode()))
    for bad in (-1, len(rows), len(rows) + 7):
        assert lib.lgd_norm_variant(bad, C.byref(code), name, len(name)) == -1, bad
    assert lib.lgd_norm_variant(0, None, None, 0) == 0                             # every output is optional
    short = C.create_string_buffer(b"#" * 8, 8)
    assert lib.lgd_norm_variant(0, None, short, 5) == 0
    assert short.raw[:5] == rows[0][1].encode()[:4] + b"\0" and short.raw[5:] == b"###"
    assert len({c for c, _ in rows}) == len(rows) == 20
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lgd_hip.h")).read()
    gn = {int(v) for v in re.findall(r"#define LGD_GN_(?!OP_)\w+ (\d+)", src)}
    ln = {int(v) for v in re.findall(r"#define LGD_LN_(?!OP_)\w+ (\d+)", src)}
    assert len(gn) == 11 and len(ln) == 9 and not (gn & ln)
    assert {c for c, _ in rows} == gn | ln
    assert ops.GN_VARIANTS == {c: nm for c, nm in rows if c in gn}
    assert ops.LN_VARIANTS == {c: nm for c, nm in rows if c in ln}
    table = ROW_KERNELS + STREAM_KERNELS + [BWD_KERNEL]
    assert {code for _, code, _ in table} == set(ops.LN_VARIANTS)
    assert re.findall(r"#define LGD_LN_OP_\w+ (\d+)", src) == [str(FWD), str(STATS), str(BWD)]


def _row_counts(width):
    edge = -(-STREAM_ELEMS // width)                     # the first row count that reaches STREAM_ELEMS elements
    per_wg = {n for _, _, n in ROW_KERNELS + STREAM_KERNELS + [BWD_KERNEL]}
    return sorted({1, edge - 1, edge, edge + 1} | {n + d for n in per_wg for d in (-1, 0, 1)})


def test_the_plan_follows_the_threshold_table():
    plan = _lib.load().lgd_layernorm_plan
    wrong, seen = [], set()
    try:
        for state in (0, 1):
            ops.set_option("ln_stream", state)
            for width in range(8, 2569, 8):
                for rows in _row_counts(width):
                    for op in (FWD, STATS, BWD):
                        for arg in (0, 1, -1):
                            got, want = plan(op, rows, width, arg), expected(op, rows, width, state if arg < 0 else arg)
                            seen.add(got)
                            if got != want:
                                wrong.append((state, width, rows, op, arg, got, want))
    finally:
        ops.set_option("ln_stream", 1)
    assert not wrong, wrong[:20]
    assert seen == set(ops.LN_VARIANTS) | {-1}
    for state in (0, 1):                                 # the statistics-only form under "ln_stream" = 0, whatever the option says
        ops.set_option("ln_stream", state)
        assert plan(STATS, 4096, 1536, 0) == 532 and plan(STATS, 4096, 1544, 0) == -1
        assert ops.layernorm_stats_served(4096, 1536) and not ops.layernorm_stats_served(4096, 1544)
    ops.set_option("ln_stream", 1)
    assert ops.layernorm_plan(STATS, 4096, 1544) == 664 and ops.layernorm_plan(STATS, 4096, 1544, ln_stream=1) == 664
    with pytest.raises(RuntimeError):
        ops.layernorm_plan(STATS, 4096, 1544, ln_stream=0)
    for op, rows, width in ((3, 8, 64), (-1, 8, 64), (FWD, 0, 64), (BWD, -4, 64), (FWD, 8, 2568), (BWD, 8, 2568), (FWD, 8, 68),
                            (STATS, 8, 12)):
        assert plan(op, rows, width, -1) == -1, (op, rows, width)


# ---------------------------------------------------------------------------------------------
# refusals: one changed argument of a call the library serves (B = 3 images of S = 100 rows, C = 320, every operand with
# a batch stride of its own — the fuser form of tests/test_layernorm_forms_gpu.py)
# ---------------------------------------------------------------------------------------------
ARGS = {
    "lgd_layernorm_f16": "x ldx y ldy rows C eps gamma beta stats rows_per_batch x_bs y_bs stream",
    "lgd_layernorm_pair_f16": "x ldx y ldy rows C eps gamma beta stats rows_per_batch x_bs y_bs pair stream",
    "lgd_layernorm_bwd_f16": "gy ldgy x ldx gx ldgx rows C gamma stats rows_per_batch gy_bs x_bs gx_bs accumulate stream",
}
BASE = dict(x=P, ldx=320, y=P, ldy=328, gy=P, ldgy=328, gx=P, ldgx=320, rows=300, C=320, eps=1e-5, gamma=P, beta=P, stats=P,
            rows_per_batch=100, x_bs=100 * 320, y_bs=130 * 328, gy_bs=130 * 328, gx_bs=100 * 320 + 24, pair=ops.PAIR_HALF,
            accumulate=0, stream=0)
STATS_ONLY = dict(y=0, gamma=0, beta=0)                 # on top of a change: the statistics-only form
_COMMON = [("C % 8", dict(C=324)), ("C > 2560", dict(C=2568)), ("rows < 1", dict(rows=0)),
           ("x NULL", dict(x=0)), ("x off 16 bytes", dict(x=P + 8)), ("ldx % 8", dict(ldx=324)), ("x_bs % 8", dict(x_bs=100 * 320 + 4))]
_FORWARD = _COMMON + [
    ("gamma NULL with y", dict(gamma=0)), ("beta NULL with y", dict(beta=0)), ("y off 16 bytes", dict(y=P + 2)),
    ("ldy % 8", dict(ldy=332)), ("y_bs % 8", dict(y_bs=130 * 328 + 4)),
    ("statistics only without stats", dict(STATS_ONLY, stats=0)), ("statistics only, x NULL", dict(STATS_ONLY, x=0)),
    ("statistics only, ldx % 8", dict(STATS_ONLY, ldx=324)),
]
REFUSALS = (
    [("lgd_layernorm_f16", w, c) for w, c in _FORWARD]
    + [("lgd_layernorm_pair_f16", w, c) for w, c in _FORWARD]
    + [("lgd_layernorm_pair_f16", w, c) for w, c in (
        ("odd rows", dict(rows=301, rows_per_batch=0)), ("rows < 2", dict(rows=0)), ("pair mode DUP", dict(pair=ops.PAIR_DUP)),
        ("pair mode 0", dict(pair=0)), ("the half is not whole images", dict(rows=300, rows_per_batch=100)))]
    + [("lgd_layernorm_bwd_f16", w, c) for w, c in _COMMON + [
        ("stats NULL", dict(stats=0)), ("gamma NULL", dict(gamma=0)), ("gy NULL", dict(gy=0)), ("gx NULL", dict(gx=0)),
        ("gy off 16 bytes", dict(gy=P + 4)), ("gx off 16 bytes", dict(gx=P + 6)), ("ldgy % 8", dict(ldgy=332)),
        ("ldgx % 8", dict(ldgx=324)), ("gy_bs % 8", dict(gy_bs=130 * 328 + 2)), ("gx_bs % 8", dict(gx_bs=100 * 320 + 4))]]
)


def _values(fn, change):
    v = dict(BASE)
    if fn == "lgd_layernorm_pair_f16":
        v.update(rows=400)                              # four images: the half is two of them
    v.update(change)
    return v


def test_the_refusal_table_is_well_formed():
    """Every row changes arguments its entry point has, the call it changes is one the plan serves with operands that move
    as 16-byte vectors, and every entry point has the refusals the contract lists."""
    for fn, what, change in REFUSALS:
        assert set(change) <= set(ARGS[fn].split()), (fn, what)
        assert len(ARGS[fn].split()) == len(_lib.SIGNATURES[fn]), fn
        v = _values(fn, {})
        assert ops.layernorm_plan(BWD if "bwd" in fn else FWD, v["rows"], v["C"]) in ops.LN_VARIANTS
        assert all(v[k] % 8 == 0 for k in ARGS[fn].split() if k.startswith("ld") or k.endswith("_bs"))
        assert v["rows"] > v["rows_per_batch"] >= 1 and ("pair" not in fn or (v["rows"] // 2) % v["rows_per_batch"] == 0)
    for fn in ARGS:
        assert {"C % 8", "C > 2560", "rows < 1", "x NULL", "x off 16 bytes", "ldx % 8", "x_bs % 8"} <= {w for f, w, _ in REFUSALS if f == fn}
    assert ("lgd_layernorm_pair_f16", "the half is not whole images", dict(rows=300, rows_per_batch=100)) in REFUSALS


@pytest.mark.parametrize("fn,what,change", REFUSALS, ids=[f"{f}:{w}" for f, w, _ in REFUSALS])
def test_host_refusal(fn, what, change):
    v = _values(fn, change)
    assert getattr(_lib.load(), fn)(*[v[k] for k in ARGS[fn].split()]) == -1, (fn, what)


def test_statistics_only_beyond_the_row_kernels_is_refused_without_the_stream():
    v = _values("lgd_layernorm_f16", dict(STATS_ONLY, C=1544, ldx=1544, x_bs=100 * 1544))
    ops.set_option("ln_stream", 0)
    try:
        assert _lib.load().lgd_layernorm_f16(*[v[k] for k in ARGS["lgd_layernorm_f16"].split()]) == -1
    finally:
        ops.set_option("ln_stream", 1)
