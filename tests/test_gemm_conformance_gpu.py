"""Whatever lgd_gemm_check accepts, lgd_gemm_f16 computes: every tile code against every descriptor form of
tests/gemm_conformance_cases.py, one test per code.

Every accepted cell runs twice.  EXACT data (small integers and halves: every partial sum in any order is exact, proven
on the CPU by tests/test_gemm_conformance_cpu.py) must come back equal to the fp64 reference bit for bit.  ROUNDING data
(N(0, 1) activations) must stay inside the derived per-element bound of gemm_conformance_cases.Case:

    fp16 output   |y - ref| <= 2^-11 |ref| + 2^-25 + E32,   E32 = (K + 8) 2^-23 S
    fp32 output   |y - ref| <= 2^-24 |ref| + E32

with S the sum of the magnitudes of every term of the element, and E32 carried through v * gelu(g) for GEGLU.  The GEGLU
bound takes the erf bound common.h documents for erf_f (Abramowitz-Stegun 7.1.26, 1.5e-7); the fused epilogue evaluates
gelu2_f, a polynomial Phi documented at 1.2e-5 absolute, which that derivation does not contain — the E32 term of these
shapes (about 2e-4) is what covers it, see the printed ratios.

Both passes check that guard rows, pad columns and gaps between batches of C and of the split-K workspace keep their
sentinel bytes, that NaN pads and guards around every input do not reach the result, that a second launch is
bit-identical, that split-K gives the same bits through the reduce launch and through in-launch counters (which are all
zero again afterwards), and that the CFG pair modes equal the full launch on the duplicated batch.  Every refused cell
raises before anything is launched and leaves the output alone."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import lgd_amd  # noqa: E402,F401
from conftest import gate  # noqa: E402
from lgd_amd import ops  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_conformance_cases as gcc  # noqa: E402

F64 = torch.float64


@pytest.fixture(scope="module")
def cases(dev):
    """Operands, references and bounds of every form, built once and left unchanged (outputs are fresh clones)."""
    return {(n, m): f.case(m, dev) for n, f in gcc.FORMS.items() for m in f.modes}


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _launch(case, tile, *, pair=None, cnt=None, ws=None):
    out = case.fresh_out()
    ws = case.fresh_ws() if ws is None else ws
    ops.gemm_launch(case.desc(tile, out, ws=ws, cnt=cnt, pair=pair))
    return out, ws


def _check_values(case, out, rows=None):
    """(problem or None, largest error / bound) of the logical [.., M, n_out] block of `out` (its first `rows` rows)."""
    y = case.c.logical(out).to(F64)
    ref, bound = case.ref, case.bound
    if rows is not None:
        y, ref, bound = y[..., :rows, :], ref[..., :rows, :], bound[..., :rows, :]
    if not bool(torch.isfinite(y).all()):
        return "NaN / Inf in the result (a pad or guard element was read into it)", float("inf")
    if case.mode == "exact":
        bad = int((y != ref).sum())
        return (f"{bad} elements differ from the exact reference, max |err| {float((y - ref).abs().max())}" if bad else None), 0.0
    ratio = float(((y - ref).abs() / bound).max())
    return (f"error / bound = {ratio:.3f}" if ratio > 1.0 else None), ratio


def _run_cell(case, tile, cell):
    """Problems of one accepted cell (empty = conforms) and its largest error / bound ratio."""
    f, problems = case.form, []
    M, half = f.M, f.M // 2
    out, ws = _launch(case, tile)
    if not case.c.outside_untouched(out):
        problems.append("a guard / pad element of C was written")
    if ws is not None and not case.ws.outside_untouched(ws):
        problems.append("a guard element of the split-K workspace was written")
    y = case.c.logical(out)
    if f.pair:
        full, _ = _launch(case, tile, pair=0)
        yf = case.c.logical(full)
        if not torch.equal(_bits(y[..., :half, :]), _bits(yf[..., :half, :])):
            problems.append("pair launch differs from the full launch in rows < M / 2")
        second = _bits(y[..., half:, :])
        if f.pair == ops.PAIR_HALF and not torch.equal(second, _bits(case.c.logical(case.c.buf)[..., half:, :])):
            problems.append("PAIR_HALF wrote rows >= M / 2")
        if f.pair == ops.PAIR_DUP and not torch.equal(second, _bits(yf[..., half:, :])):
            problems.append("PAIR_DUP differs from the full launch in rows >= M / 2")
    problem, ratio = _check_values(case, out, rows=half if f.pair == ops.PAIR_HALF else None)
    if problem:
        problems.append(problem)
    again, _ = _launch(case, tile, ws=ws)                 # the workspace still holds the first launch's partials
    if not torch.equal(_bits(again), _bits(out)):
        problems.append("a second launch is not bit-identical")
    if f.splits > 1 and cell == "Y":
        cnt = torch.zeros(4096, dtype=torch.int32, device=out.device)
        counted, ws2 = _launch(case, tile, cnt=cnt)
        if not torch.equal(_bits(counted), _bits(out)):
            problems.append("in-launch split-K combine differs from the reduce launch")
        if bool(cnt.any()):
            problems.append("split-K counters are not all zero after the launch")
        if not case.ws.outside_untouched(ws2):
            problems.append("a guard element of the split-K workspace was written (in-launch combine)")
    return problems, ratio


def _run_refused(case, tile):
    out, ws = case.fresh_out(), case.fresh_ws()
    d = case.desc(tile, out, ws=ws)
    assert not ops.gemm_accepts(d)
    with pytest.raises(RuntimeError):                     # LGD_ERR_ARG from the host-side check: nothing is launched
        ops.gemm_launch(d)
    return [] if torch.equal(_bits(out), _bits(case.c.buf)) else ["a refused launch wrote to C"]


@pytest.mark.parametrize("tile", gcc.TILES)
def test_gemm_tile_conforms_on_every_form_it_accepts(dev, cases, tile):
    pinned = gcc.pinned()
    failures, worst, worst_at, worst_geglu, ran = [], 0.0, None, 0.0, 0
    for name, form in gcc.FORMS.items():
        cell = pinned[name][tile]
        for mode in form.modes:
            case = cases[(name, mode)]
            if cell == ".":
                problems = _run_refused(case, tile)
            else:
                problems, ratio = _run_cell(case, tile, cell)
                ran += 1
                if ratio > worst:
                    worst, worst_at = ratio, name
                if form.geglu:
                    worst_geglu = max(worst_geglu, ratio)
            failures += [f"{name} [{mode}]: {p}" for p in problems]
    print(f"[conformance] code {tile} ({ops.TILE_NAMES[tile]}): {ran} accepted cell passes, "
          f"largest error / bound at {worst_at}, over the GEGLU forms {worst_geglu:.3f}")
    for line in failures:
        print("[conformance] FAIL", line)
    assert ran >= gcc.MIN_FORMS_PER_CODE
    gate(f"gemm code {tile} rounding pass, max error / derived bound", worst, 1.0)
    assert not failures, failures
