"""The GroupNorm launch contract, checked where there is no GPU (tests/groupnorm_conformance_cases.py):

  * every row of the case table selects the code it claims under its options, the table reaches every code of
    ops.GN_VARIANTS, a sweep over shapes and options answers nothing the table does not name, and the engine's own
    (C, HW) pairs get the kernels the comments of csrc/norm.hip promise;
  * the derived error bound is not too tight — an fp32 emulation of each path (two-pass and E[x^2] - mean^2, chunked as
    ops.gn_chunks chunks, fp16 outputs) stays inside on every row and data pass — and not too loose — eight wrong answers
    built from the fp64 reference fall outside on the rows flagged for them;
  * the host refusals are what the REFUSALS table says: exactly LGD_ERR_ARG, from the entry points themselves before the
    device is touched, and from lgd_groupnorm_plan where its arguments show the fault."""
import os
import sys

import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import _lib, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import groupnorm_conformance_cases as gcc  # noqa: E402

F32, F64, H16 = torch.float32, torch.float64, torch.float16
FWD_ROWS = [n for n, r in gcc.ROWS_BY_NAME.items() if r.op == "fwd"]
BWD_ROWS = [n for n, r in gcc.ROWS_BY_NAME.items() if r.op == "bwd"]


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__ as ge
    ge.build()
    yield
    gcc.set_options(gcc.DEFAULT_OPTS)


def _plan_under(row, pair=0):
    gcc.set_options(row.opts)
    try:
        return row.plan(pair)
    finally:
        gcc.set_options(gcc.DEFAULT_OPTS)


def test_every_row_selects_the_code_it_claims():
    wrong = [(r.name, _plan_under(r)) for r in gcc._ROW_LIST + gcc.PAIR_ROWS if _plan_under(r) != r.code]
    assert not wrong, wrong
    for r in gcc.PAIR_ROWS:                                 # the pair forms run the kernel of the full launch
        assert _plan_under(r, ops.PAIR_HALF) == r.code and _plan_under(r, ops.PAIR_DUP) == r.code, r.name


def test_the_table_reaches_every_code():
    assert set(gcc.CODES) == set(ops.GN_VARIANTS), set(gcc.CODES) ^ set(ops.GN_VARIANTS)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lgd_hip.h")).read()
    import re
    header = {int(v) for _, v in re.findall(r"#define (LGD_GN_(?!OP_)\w+) (\d+)", src)}
    assert header == set(ops.GN_VARIANTS), header ^ set(ops.GN_VARIANTS)


# the names the profiles and the gate messages carry, pinned: code, then the kernel instantiation(s) the code launches
PINNED_VARIANTS = """
104 gn_fused_kernel<4>
108 gn_fused_kernel<8>
116 gn_fused_kernel<16>
132 gn_fused_kernel<32>
201 gn_stats_kernel + gn_apply_kernel, one channel pass
202 gn_stats_kernel + gn_apply_kernel, two channel passes
300 gn_bwd_slab_kernel<256, 8, false>
301 gn_bwd_slab_kernel<256, 8, true>
310 gn_bwd_slab_kernel<512, 11, false>
311 gn_bwd_slab_kernel<512, 11, true>
400 gn_bwd_stats_kernel + gn_bwd_apply_kernel
"""


def test_the_variant_names_are_the_pinned_ones():
    """ops.GN_VARIANTS is read from the library's table (lgd_norm_variant; tests/test_layernorm_contract_cpu.py compares
    the whole table with the header): the 11 (code, name) pairs, byte for byte."""
    pinned = [ln.split(" ", 1) for ln in PINNED_VARIANTS.strip().splitlines()]
    assert list(ops.GN_VARIANTS.items()) == [(int(c), nm) for c, nm in pinned]
    assert isinstance(ops.GN_VARIANTS, dict) and len(pinned) == 11


_HWS = sorted(set(range(1, 42)) | {48, 63, 64, 65, 100, 136, 137, 200, 201, 255, 256, 257, 288, 300, 408, 409, 420, 512, 561, 562,
                                   576, 700, 1024, 1122, 1123, 2048, 4095, 4096})


def test_the_plan_answers_only_named_codes():
    """C = 8 .. 4096 in steps of 8, every G <= 64 that divides C, HW = 1 .. 4096 (every value to 41, then both sides of every
    threshold of the dispatch at the engine's widths), both ops, the option states that change the choice."""
    plan = _lib.load().lgd_groupnorm_plan
    fwd_codes, bwd_codes = {104, 108, 116, 132, 201, 202}, {300, 301, 310, 311, 400}
    seen = {}
    try:
        for fused, slab in ((256, 1), (4096, 1), (0, 0)):
            gcc.set_options({"gn_fused": fused, "gn_slab": slab})
            got_f, got_b = set(), set()
            for C in range(8, 4097, 8):
                for G in (g for g in range(1, 65) if C % g == 0):
                    for HW in _HWS:
                        got_f.add(plan(0, C, 0, 2, HW, G, 0, 0))
                        got_b.add(plan(1, C, 0, 2, HW, G, 0, 0))
                        got_b.add(plan(1, C, 0, 2, HW, G, 1, 0))
            seen[(fused, slab)] = (got_f, got_b)
            assert got_f <= fwd_codes and got_b <= bwd_codes, (fused, slab, got_f - fwd_codes, got_b - bwd_codes)
        assert seen[(0, 0)] == ({201, 202}, {400})
        assert seen[(4096, 1)] == (fwd_codes, bwd_codes)
        # the concat split, the batch and the pair mode do not move the choice
        gcc.set_options(gcc.DEFAULT_OPTS)
        for C, HW in ((2560, 256), (1920, 64), (960, 1024), (192, 256)):
            for op in (0, 1):
                base = plan(op, C, 0, 2, HW, 32, 1, 0)
                assert {plan(op, C - c1, c1, B, HW, 32, 1, 0) for c1 in (0, 64, C // 2 // 8 * 8) for B in (1, 2, 16)} == {base}
            assert plan(0, C, 0, 4, HW, 32, 1, ops.PAIR_HALF) == plan(0, C, 0, 4, HW, 32, 1, ops.PAIR_DUP) == plan(0, C, 0, 4, HW, 32, 1, 0)
    finally:
        gcc.set_options(gcc.DEFAULT_OPTS)


def test_the_engine_shapes_get_the_kernels_norm_hip_promises():
    """csrc/norm.hip: the forward runs in one launch on the 8x8 and 16x16 maps ("gn_fused" 256) and in two above; the backward
    holds its slab in registers on the 8x8 and 16x16 maps up to 96 KB of x and gy (measured there at C = 1280 and 2560) and
    stays on two launches above (16x16 at C = 1920, every 32x32 and 64x64 map)."""
    gcc.set_options(gcc.DEFAULT_OPTS)
    p = lambda op, C, HW, silu=True: ops.groupnorm_plan(op, C, 0, 2, HW, 32, silu=silu)
    for C in (1280, 2560):
        assert p(0, C, 64) == 104 and p(1, C, 64) == 301 and p(1, C, 64, False) == 300
    assert p(0, 640, 256) == 108 and p(0, 1280, 256) == 108 and p(0, 1920, 256) == 116 and p(0, 2560, 256) == 116
    assert p(1, 640, 256) == 301 and p(1, 1280, 256) == 301 and p(1, 2560, 256) == 311 and p(1, 2560, 256, False) == 310
    assert p(1, 1920, 256) == 400
    for C, HW in ((320, 4096), (640, 4096), (960, 4096), (320, 1024), (640, 1024), (960, 1024), (1280, 1024), (1920, 1024)):
        assert p(0, C, HW) == 201 and p(1, C, HW) == 400, (C, HW)
    assert p(0, 3072, 1024) == 202 and p(0, 2048, 1024) == 201                # the refiner's concat: two channel passes
    assert p(0, 128, 4096) == 201 and p(0, 512, 256) == 104                   # the VAE


# ---------------------------------------------------------------------------------------------
# the bound, shown by the reference alone
# ---------------------------------------------------------------------------------------------
def _ratio(got, ref, bound):
    assert bool(torch.isfinite(bound).all()) and bool((bound > 0).all())
    return float(((got.to(F64) - ref).abs() / bound).max())


def _fwd(row, ps, **mut):
    d = row.data(ps)
    return gcc.fwd_reference(d.x.to(F64), d.gamma.to(F64), d.beta.to(F64), row.G, row.eps, row.silu, depth=row.depth,
                             two_launch=row.two_launch, **mut)


def _bwd_inputs(row, ps):
    d = row.data(ps)
    x, gamma, beta = d.x.to(F64), d.gamma.to(F64), d.beta.to(F64)
    f = gcc.fwd_reference(x, gamma, beta, row.G, row.eps, row.silu, depth=row.depth, two_launch=True)
    return x, d.gy.to(F64), gamma, beta, f["mean"].to(F32), f["rstd"].to(F32), d.base.to(F64)


def _bwd(row, ps, accumulate=False, **mut):
    x, gy, gamma, beta, m32, r32, base = _bwd_inputs(row, ps)
    return gcc.bwd_reference(x, gy, gamma, beta, m32.to(F64), r32.to(F64), row.G, row.silu, depth=row.depth, slab=row.slab,
                             base=base if accumulate else None, **mut)


@pytest.mark.parametrize("name", FWD_ROWS)
def test_forward_emulation_stays_inside_the_bound(name):
    row = gcc.ROWS_BY_NAME[name]
    worst = {}
    for ps in gcc.PASSES:
        d = row.data(ps)
        ref = _fwd(row, ps)
        emu = gcc.fwd_emulation(row, d.x.to(F32), d.gamma, d.beta)
        for o in ("y", "mean", "rstd"):
            assert bool(torch.isfinite(emu[o]).all()), (ps, o)
            worst[(ps, o)] = _ratio(emu[o], ref[o], ref["bound_" + o])
        if ps == "flat":                                       # y = beta exactly in the flat group, and the bound there is small
            for b in range(row.B):
                g = gcc.flat_group(b, row.G)
                sl = slice(g * row.cpg, (g + 1) * row.cpg)
                assert float(ref["rstd"][b, g]) == row.eps ** -0.5
                if not row.silu:
                    assert torch.equal(ref["y"][b, :, sl], d.beta.to(F64)[sl].expand(row.HW, -1))
                assert float(ref["bound_y"][b, :, sl].max()) < 0.05
    print(f"[groupnorm bound] {name} D {row.depth}: emulation error / bound " + ", ".join(f"{p}.{o} {v:.3f}" for (p, o), v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("name", BWD_ROWS)
def test_backward_emulation_stays_inside_the_bound(name):
    row = gcc.ROWS_BY_NAME[name]
    worst = {}
    for ps in gcc.PASSES:
        x, gy, gamma, beta, m32, r32, base = _bwd_inputs(row, ps)
        for acc in (False, True):
            ref = _bwd(row, ps, acc)
            emu = gcc.bwd_emulation(row, x.to(F32), gy.to(F32), gamma.to(F32), beta.to(F32), m32, r32, base.to(F32) if acc else None)
            assert bool(torch.isfinite(emu["dx"]).all()), (ps, acc)
            worst[(ps, acc)] = _ratio(emu["dx"], ref["dx"], ref["bound_dx"])
    print(f"[groupnorm bound] {name} D {row.depth}: emulation error / bound " + ", ".join(f"{p}.acc{int(a)} {v:.3f}" for (p, a), v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def _stat_passes(row):
    """The passes a statistics fault must show on.  "plain" always.  On "offset" the missing pixel moves a group's mean by
    (that pixel's mean - the group's) / HW, a draw of 0.25 / sqrt(cpg) / HW N(0, 1) per (image, group) against
    e_m = (D + 2) w 4, and rstd only through the cancellation-limited bound: flagged where the row has at least 8 (image,
    group) pairs to take the largest of (the G = 1 row has one, and one draw can be small)."""
    return ("plain", "offset") if row.B * row.G >= 8 else ("plain",)


def _worst_fwd(mut, ref, outs=("y", "mean", "rstd")):
    return max(_ratio(mut[o], ref[o], ref["bound_" + o]) for o in outs)


@pytest.mark.parametrize("name", [n for n in FWD_ROWS if gcc.ROWS_BY_NAME[n].HW > 1])
def test_statistics_that_miss_the_last_pixel_are_outside_the_bound(name):
    """Every forward row: in the statistics output on every pass; in y as well on the maps of at most 256 pixels, where one
    pixel is more than 1 / 256 of a group (at 4096 pixels y moves by less than its fp16 rounding: 1.1e-4 in the old measure)."""
    row = gcc.ROWS_BY_NAME[name]
    pix = torch.arange(row.HW - 1)
    for ps in _stat_passes(row):
        ref, mut = _fwd(row, ps), _fwd(row, ps, pix=pix)
        assert _worst_fwd(mut, ref, ("mean", "rstd")) > 2.0, ps
        if row.HW <= 256:
            assert _worst_fwd(mut, ref, ("y",)) > 2.0, ps


@pytest.mark.parametrize("name", [n for n in FWD_ROWS if gcc.ROWS_BY_NAME[n].two_launch])
def test_statistics_that_miss_the_last_pixel_of_one_chunk_are_outside_the_bound(name):
    row = gcc.ROWS_BY_NAME[name]
    last = -(-row.HW // row.nchunk) - 1                                    # the last pixel of chunk 0
    pix = torch.tensor([p for p in range(row.HW) if p != last])
    for ps in _stat_passes(row):
        ref, mut = _fwd(row, ps), _fwd(row, ps, pix=pix)
        assert _worst_fwd(mut, ref, ("mean", "rstd")) > 2.0, ps


@pytest.mark.parametrize("name", FWD_ROWS)
def test_a_pixel_count_one_too_large_is_outside_the_bound(name):
    row = gcc.ROWS_BY_NAME[name]
    for ps in ("plain", "offset"):
        ref, mut = _fwd(row, ps), _fwd(row, ps, n_pixels=row.HW + 1)
        assert _worst_fwd(mut, ref, ("mean", "rstd")) > 2.0, ps
        if row.HW <= 256:
            assert _worst_fwd(mut, ref, ("y",)) > 2.0, ps


@pytest.mark.parametrize("name", [n for n in FWD_ROWS if gcc.ROWS_BY_NAME[n].cpg % 8])
def test_the_lower_groups_statistics_on_a_straddling_vector_are_outside_the_bound(name):
    """Rows whose groups do not end on a 16-byte vector (cpg % 8 != 0)."""
    row = gcc.ROWS_BY_NAME[name]
    for ps in gcc.PASSES:
        ref, mut = _fwd(row, ps), _fwd(row, ps, chan_group=gcc.first_vector_group(row.C, row.G))
        assert _ratio(mut["y"], ref["y"], ref["bound_y"]) > 2.0, ps


@pytest.mark.parametrize("name", BWD_ROWS)
def test_dx_without_m1_is_outside_the_bound(name):
    row = gcc.ROWS_BY_NAME[name]
    for ps in gcc.PASSES:
        ref, mut = _bwd(row, ps), _bwd(row, ps, no_m1=True)
        assert _ratio(mut["dx"], ref["dx"], ref["bound_dx"]) > 2.0, ps


@pytest.mark.parametrize("name", [n for n in BWD_ROWS if gcc.ROWS_BY_NAME[n].cpg % 8])
def test_the_neighbours_m2_on_a_straddling_vector_is_outside_the_bound(name):
    row = gcc.ROWS_BY_NAME[name]
    for ps in gcc.PASSES:
        ref, mut = _bwd(row, ps), _bwd(row, ps, m2_group=gcc.first_vector_group(row.C, row.G))
        assert _ratio(mut["dx"], ref["dx"], ref["bound_dx"]) > 2.0, ps


@pytest.mark.parametrize("name", [n for n in BWD_ROWS if gcc.ROWS_BY_NAME[n].silu])
def test_the_sigmoid_in_place_of_silus_derivative_is_outside_the_bound(name):
    row = gcc.ROWS_BY_NAME[name]
    for ps in gcc.PASSES:
        ref, mut = _bwd(row, ps), _bwd(row, ps, sigmoid_grad=True)
        assert _ratio(mut["dx"], ref["dx"], ref["bound_dx"]) > 2.0, ps


@pytest.mark.parametrize("name", BWD_ROWS)
def test_a_base_added_twice_is_outside_the_bound(name):
    row = gcc.ROWS_BY_NAME[name]
    ref, mut = _bwd(row, "plain", True), _bwd(row, "plain", True, base_twice=True)
    assert _ratio(mut["dx"], ref["dx"], ref["bound_dx"]) > 2.0


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_the_refusal_table_is_well_formed():
    """Every REFUSALS row names arguments its entry point has, and the call it changes is one the library accepts."""
    plan = _lib.load().lgd_groupnorm_plan
    for fn, what, change in gcc.REFUSALS:
        names = [n[2:] if n.startswith("p:") else n for n in gcc.ARGS[fn].split()]
        assert set(change) <= set(names), (fn, what)
        assert len(gcc.refusal_args(fn, change, gcc.P)) == len(_lib.SIGNATURES[fn]), fn
        v = gcc.refusal_values(fn, {})
        op, pair = (1 if "bwd" in fn else 0), (v["pair"] if "pair" in fn else 0)
        assert plan(op, v["c0"], v["c1"], v["B"], v["HW"], v["G"], v["silu"], pair) > 0, fn
    want = {"G > 64", "G = 0", "C > 4096", "C % G", "c0 % 8", "c1 % 8", "nchunk < 1", "B < 1", "HW < 1"}
    for fn in gcc.ARGS:
        assert want <= {w for f, w, _ in gcc.REFUSALS if f == fn}, fn


@pytest.mark.parametrize("fn,what,change", gcc.REFUSALS, ids=[f"{f}:{w}" for f, w, _ in gcc.REFUSALS])
def test_host_refusal(fn, what, change):
    """Exactly LGD_ERR_ARG (-1), not the code of a failed launch (-2); G = 0 used to end the process with SIGFPE, and the
    NULL pointers of the backward went to the device.  lgd_groupnorm_plan answers the same where it sees the argument."""
    lib = _lib.load()
    assert getattr(lib, fn)(*gcc.refusal_args(fn, change, gcc.P)) == -1, (fn, what)
    v = gcc.refusal_values(fn, change)
    op, pair = (1 if "bwd" in fn else 0), (v["pair"] if "pair" in fn else 0)
    code = lib.lgd_groupnorm_plan(op, v["c0"], v["c1"], v["B"], v["HW"], v["G"], v["silu"], pair)
    if set(change) & set(gcc.PLAN_ARGS) and what != "pair mode 0":       # pair = 0 is the plain call to the plan query
        assert code == -1, (fn, what, code)
    else:
        assert code in ops.GN_VARIANTS, (fn, what, code)


def test_the_plan_refuses_what_no_entry_point_serves():
    plan = _lib.load().lgd_groupnorm_plan
    assert plan(2, 64, 64, 2, 64, 32, 0, 0) == -1 and plan(-1, 64, 64, 2, 64, 32, 0, 0) == -1        # no such op
    assert plan(1, 64, 64, 2, 64, 32, 0, ops.PAIR_HALF) == -1                                        # no pair backward
    assert plan(0, 0, 64, 2, 64, 32, 0, 0) == -1 and plan(0, 64, -8, 2, 64, 32, 0, 0) == -1
    with pytest.raises(RuntimeError):
        ops.groupnorm_plan(ops.GN_OP_FWD, 64, 64, 2, 64, 0)


def test_statistics_together_with_pair_are_refused_before_the_library():
    x = torch.zeros(4 * 64, 64, dtype=H16)
    gb = torch.zeros(64)
    with pytest.raises(AssertionError):
        ops.groupnorm(x, 4, 64, 32, 1e-5, gb, gb, True, stats=torch.zeros(4, 32, 2), pair=ops.PAIR_HALF)
