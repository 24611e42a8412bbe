"""LayerNorm on the view forms the engine launches, for every kernel instantiation of the LayerNorm dispatch (ops.LN_VARIANTS):
before each launch the case asserts the code ops.layernorm_plan answers for it, and the last test of the module asserts that
the cases together claimed every code.

Forms: the GLIGEN fuser's — B = 3 images of S = 100 rows, x contiguous (x_bs = S C), y at the head of an [S + 30][ldy] block
per image with ldy wider than C (a workgroup's rows straddle two images; the 30 preset grounding rows and the pad columns
must keep their bytes) — its backward with `accumulate` on and off, the statistics-only form at a wider ldx, and
PAIR_HALF.  Every input pad holds NaN, every output pad a sentinel (tests/gemm_conformance_cases.Carved).

The bound, from the arithmetic of the kernels (u = 2^-11, w = 2^-24; statistics in fp32, two passes):
  mean     e_m = (C + 2) w mean|x|                                   (fp32 sum of C terms, one divide)
  var      relative (C + 6) w + e_m^2 / var                          (sum (x - m^)^2 = sum (x - m)^2 + C dm^2, each square 3 w)
  rstd     relative e_r = half of that + 2^-22                        (rsqrtf)
  y        |y^ - y| <= u |y| + 2^-25 + |x - m| rstd |gamma| (e_r + 3 w) + e_m rstd |gamma| + w |y|
  backward (mean / rstd as given): d = gy gamma, xh = (x - mean) rstd, s1 = mean d, s2 = mean d xh,
           |dx^ - dx| <= u |out| + 2^-25 + rstd ((C + 2) w mean|d| + |xh| (C + 4) w mean|d xh| + 6 w (|d| + |s1| + |xh s2|)) + 2 w |out|
           with out = dx (+ the fp16 base when accumulating: exact input)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import lgd_amd  # noqa: E402,F401
from conftest import gate  # noqa: E402
from lgd_amd import ops  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_conformance_cases import SENT16, SENT32, Carved  # noqa: E402
from layernorm_cases import EPS, fwd_ref as _fwd_ref, bwd_ref as _bwd_ref  # noqa: E402

H16, F32, F64 = torch.float16, torch.float32, torch.float64
U, W = 2.0 ** -11, 2.0 ** -24
NAN = float("nan")
WIDTHS = [64, 320, 640, 1280, 1536, 2560]
B, S, TAIL = 3, 100, 30
ROW_CODE = {64: 514, 320: 514, 640: 524, 1280: 532, 1536: 532, 2560: 550}        # the row kernels, the wave kernel at 2560
STREAM_CODE = {64: 608, 320: 608, 640: 616, 1280: 632, 1536: 664, 2560: 664}     # ln_stats_kernel: 8 / 16 / 32 / 64 lanes per row
BWD_CODE = 700
CLAIMED = set()


def _claim(code, op, rows, C):
    """The library answers `code` for the launch that follows (under the current option state)."""
    got = ops.layernorm_plan(op, rows, C)
    assert got == code, (op, rows, C, got, ops.LN_VARIANTS.get(got))
    CLAIMED.add(code)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _data(rows, C, seed):
    """x with a per-row offset and scale (means far from 0, spreads 0.1 .. 3), gamma / beta fp32, gy."""
    g = torch.Generator().manual_seed(seed)
    scale = 0.1 + 2.9 * torch.rand(rows, 1, generator=g)
    x = (torch.randn(rows, C, generator=g) * scale + 4.0 * torch.randn(rows, 1, generator=g)).to(H16).to(F64)
    gamma = (1.0 + 0.5 * torch.randn(C, generator=g)).to(F32).to(F64)
    beta = torch.randn(C, generator=g).to(F32).to(F64)
    gy = torch.randn(rows, C, generator=g).to(H16).to(F64)
    return x, gamma, beta, gy


def _ratio(y, ref, bound, what):
    assert bool(torch.isfinite(y).all()), f"NaN / Inf in {what}: a pad or a row of another image was read into it"
    return float(((y.to(F64) - ref).abs() / bound).max())


def _vec(t, dev, dtype=F32):
    return Carved(t, (1,), NAN, dtype, dev)


@pytest.mark.parametrize("C", WIDTHS)
def test_layernorm_fuser_form(dev, C):
    """y written at the head of every image's [S + 30][ldy] block; statistics out; then the pair launch on a duplicated
    batch of four images."""
    rows, ldy = B * S, C + 8
    x, gamma, beta, _ = _data(rows, C, 100 + C)
    ref = _fwd_ref(x, gamma, beta)
    dev_ref = {k: v.to(dev) for k, v in ref.items()}
    xc = Carved(x.reshape(B, S, C), (S * C, C, 1), NAN, H16, dev)
    gc, bc = _vec(gamma, dev), _vec(beta, dev)
    block = torch.full((B, S + TAIL, C), SENT16, dtype=F64)
    block[:, S:] = torch.randn(B, TAIL, C, generator=torch.Generator().manual_seed(C)).to(H16).to(F64)      # the preset grounding rows
    yc = Carved(block, ((S + TAIL) * ldy, ldy, 1), SENT16, H16, dev)
    sc = Carved(torch.full((rows, 2), SENT32, dtype=F64), (2, 1), SENT32, F32, dev)

    gamma_t = gc.ptr()[:C]                      # ops.layernorm reads C from gamma.shape[0]

    def launch():
        out, st = yc.fresh(), sc.fresh()
        _claim(ROW_CODE[C], ops.LN_OP_FWD, rows, C)
        ops.layernorm(xc.ptr(), gamma_t, bc.ptr(), EPS, out=yc.ptr(out), ldy=ldy, stats=sc.ptr(st), rows_per_batch=S,
                      x_bs=S * C, y_bs=(S + TAIL) * ldy, rows=rows, ldx=C)
        return out, st
    out, st = launch()
    assert yc.outside_untouched(out), "a pad column / gap / guard of y was written"
    got = yc.logical(out)
    assert torch.equal(_bits(got[:, S:]), _bits(yc.logical(yc.buf)[:, S:])), "the preset grounding rows changed"
    r_y = _ratio(got[:, :S].reshape(rows, C), dev_ref["y"], dev_ref["bound"], "y")
    assert sc.outside_untouched(st)
    stats = sc.logical(st)
    r_m = _ratio(stats[:, 0:1], dev_ref["mean"], dev_ref["bound_mean"], "mean")
    r_r = _ratio(stats[:, 1:2], dev_ref["rstd"], dev_ref["bound_rstd"], "rstd")
    out2, st2 = launch()
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(st2), _bits(st)), "a second launch is not bit-identical"
    print(f"[layernorm forms] C {C}: y {r_y:.3f}, mean {r_m:.3f}, rstd {r_r:.3f} of the bound")
    gate(f"layernorm fuser form C={C}: max error / derived bound (y, mean, rstd)", max(r_y, r_m, r_r), 1.0)

    # ---- PAIR_HALF: four images, the last two copies of the first two; the half is a whole number of images
    x4 = torch.cat([x[:2 * S], x[:2 * S]]).reshape(4, S, C)
    xc4 = Carved(x4, (S * C + 16, C, 1), NAN, H16, dev)
    yc4 = Carved(torch.full((4, S, C), SENT16, dtype=F64), (S * ldy + 8, ldy, 1), SENT16, H16, dev)
    outs = []
    for pair in (0, ops.PAIR_HALF):
        o = yc4.fresh()
        _claim(ROW_CODE[C], ops.LN_OP_FWD, 4 * S, C)            # chosen for the full call's rows, with and without pair
        ops.layernorm(xc4.ptr(), gamma_t, bc.ptr(), EPS, out=yc4.ptr(o), ldy=ldy, rows_per_batch=S, x_bs=S * C + 16,
                      y_bs=S * ldy + 8, rows=4 * S, ldx=C, pair=pair)
        assert yc4.outside_untouched(o)
        outs.append(yc4.logical(o))
    full, halfo = outs
    assert torch.equal(_bits(halfo[:2]), _bits(full[:2])), "PAIR_HALF differs from the full launch in the first half"
    assert torch.equal(_bits(halfo[2:]), _bits(yc4.logical(yc4.buf)[2:])), "PAIR_HALF wrote the second half"
    assert torch.equal(_bits(full[2:]), _bits(full[:2]))
    gate(f"layernorm pair form C={C}: max error / derived bound", _ratio(full[:2].reshape(2 * S, C), dev_ref["y"][:2 * S], dev_ref["bound"][:2 * S], "y"), 1.0)


@pytest.mark.parametrize("stream", [0, 1])
@pytest.mark.parametrize("C", WIDTHS)
def test_layernorm_statistics_only(dev, C, stream):
    """y = NULL, at a row stride wider than C and row counts that are no multiple of any kernel's rows per workgroup, one
    below and one above the 8 M elements from which "ln_stream" = 1 takes ln_stats_kernel (C = 2560: at every size)."""
    if stream == 0 and C > 1536:                   # the row kernels hold three vectors per lane: refused, not served
        ops.set_option("ln_stream", 0)
        try:
            with pytest.raises(RuntimeError):
                ops.layernorm_plan(ops.LN_OP_STATS, 8, C)
            with pytest.raises(RuntimeError):
                ops.layernorm_stats(torch.zeros(8, C, device=dev, dtype=H16), C)
        finally:
            ops.set_option("ln_stream", 1)
        return
    worst = 0.0
    ops.set_option("ln_stream", stream)
    try:
        for rows in (203, -(-(8 << 20) // C) + 3):
            x, _, _, _ = _data(rows, C, 300 + C + rows % 7)
            ref = {k: v.to(dev) for k, v in _fwd_ref(x, torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64)).items()}
            xc = Carved(x, (C + 16, 1), NAN, H16, dev)
            sc = Carved(torch.full((rows, 2), SENT32, dtype=F64), (2, 1), SENT32, F32, dev)
            st = sc.fresh()
            streams = stream and (rows * C >= 8 << 20 or C > 1536)
            _claim((STREAM_CODE if streams else ROW_CODE)[C], ops.LN_OP_STATS, rows, C)
            ops.layernorm_stats(xc.ptr(), C, EPS, stats=sc.ptr(st), rows=rows, ldx=C + 16)
            assert sc.outside_untouched(st), "a guard of the statistics was written"
            stats = sc.logical(st)
            worst = max(worst, _ratio(stats[:, 0:1], ref["mean"], ref["bound_mean"], "mean"),
                        _ratio(stats[:, 1:2], ref["rstd"], ref["bound_rstd"], "rstd"))
            st2 = sc.fresh()
            ops.layernorm_stats(xc.ptr(), C, EPS, stats=sc.ptr(st2), rows=rows, ldx=C + 16)
            assert torch.equal(_bits(st2), _bits(st))
    finally:
        ops.set_option("ln_stream", 1)
    gate(f"layernorm statistics C={C} ln_stream={stream}: max error / derived bound", worst, 1.0)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("C", WIDTHS)
def test_layernorm_bwd_fuser_form(dev, C, accumulate):
    """gy from the head of every image's [S + 30][ldgy] block (the tail rows hold NaN: the grounding rows carry no
    gradient here), x contiguous, gx contiguous with a gap between images; with `accumulate` gx holds a base on entry."""
    rows, ldgy = B * S, C + 8
    x, gamma, _, gy = _data(rows, C, 500 + C)
    f = _fwd_ref(x, gamma, torch.zeros(C, dtype=F64))
    mean, rstd = f["mean"].to(F32).to(F64), f["rstd"].to(F32).to(F64)           # the statistics as given
    base = torch.randn(rows, C, generator=torch.Generator().manual_seed(C + 1)).to(H16).to(F64) if accumulate else None
    ref, bound = _bwd_ref(x, gy, gamma, mean, rstd, base)
    ref, bound = ref.to(dev), bound.to(dev)
    gblock = torch.full((B, S + TAIL, C), NAN, dtype=F64)
    gblock[:, :S] = gy.reshape(B, S, C)
    gyc = Carved(gblock, ((S + TAIL) * ldgy, ldgy, 1), NAN, H16, dev)
    xc = Carved(x.reshape(B, S, C), (S * C, C, 1), NAN, H16, dev)
    gxc = Carved(base.reshape(B, S, C) if accumulate else torch.full((B, S, C), SENT16, dtype=F64), (S * C + 24, C, 1), SENT16, H16, dev)
    gc = _vec(gamma, dev)
    sc = Carved(torch.cat([mean, rstd], 1), (2, 1), NAN, F32, dev)
    gamma_t = gc.ptr()[:C]

    def launch():
        out = gxc.fresh()
        _claim(BWD_CODE, ops.LN_OP_BWD, rows, C)
        ops.layernorm_bwd(gyc.ptr(), xc.ptr(), gamma_t, sc.ptr(), gx=gxc.ptr(out), rows=rows, ldgy=ldgy, ldx=C, ldgx=C,
                          rows_per_batch=S, gy_bs=(S + TAIL) * ldgy, x_bs=S * C, gx_bs=S * C + 24, accumulate=accumulate)
        return out
    out = launch()
    assert gxc.outside_untouched(out), "a gap / guard of gx was written"
    r = _ratio(gxc.logical(out).reshape(rows, C), ref, bound, "gx")
    assert torch.equal(_bits(launch()), _bits(out)), "a second launch is not bit-identical"
    gate(f"layernorm backward fuser form C={C} accumulate={accumulate}: max error / derived bound", r, 1.0)


def test_the_cases_claimed_every_code():
    """Runs last: the cases above asserted, launch by launch, the code the library answers; together they reach every row of
    the LayerNorm variant table."""
    assert CLAIMED == set(ops.LN_VARIANTS), sorted(CLAIMED ^ set(ops.LN_VARIANTS))
