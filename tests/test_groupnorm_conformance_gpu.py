"""Every GroupNorm kernel on every form the launch accepts (tests/groupnorm_conformance_cases.py): one test per code of
ops.GN_VARIANTS.  Per row: the library answers the code the row claims, then the launch goes through ops.groupnorm /
ops.groupnorm_bwd on carved operands (NaN around every input, sentinels around y, gx0, gx1, the statistics and the
partial table) and

  * every element of y, mean, rstd, gx0 and gx1 is within its derived bound (the worst error / bound ratio and the
    (image, group) that holds it are printed and gated at 1.0), nothing written is NaN or Inf, every guard keeps its bytes,
    every (image, group) of the statistics is written, and a second launch is bit-identical;
  * forward rows run every data pass; backward rows every pass without `accumulate` and "plain" with it;
  * PAIR_HALF / PAIR_DUP are bit-equal to the full launch on the duplicated batch;
  * the refusal table raises and writes nothing (every row of it returns before any launch: the CPU suite shows that).

Measured on an MI355X, worst error / bound (y, mean, rstd): 104 0.990 0.012 0.127; 108 0.991 0.034 0.065; 116 0.992 0.051
0.066; 132 0.994 0.049 0.039; 201 0.996 0.057 0.105; 202 0.996 0.070 0.059; dx: 300 0.989, 301 0.994, 310 0.994, 311 0.996,
400 0.994 (y and dx sit at the fp16 half-ulp, the first term of their bounds).  Relative rstd error on "offset" at C = 1280,
8x8: two-launch 2.64e-5, fused 1.63e-7 — E[x^2] - mean^2 costs a factor of 162 there and stays below fp16 rounding."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import lgd_amd  # noqa: E402,F401
from conftest import gate  # noqa: E402
from lgd_amd import ops  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import groupnorm_conformance_cases as gcc  # noqa: E402
from groupnorm_conformance_cases import NAN, SENT16, SENT32, Carved  # noqa: E402

H16, F32, F64 = torch.float16, torch.float32, torch.float64


@pytest.fixture(autouse=True)
def _default_options():
    gcc.set_options(gcc.DEFAULT_OPTS)
    yield
    gcc.set_options(gcc.DEFAULT_OPTS)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _contig(values, fill, dtype, dev):
    strides, s = [], 1
    for n in reversed(values.shape):
        strides.insert(0, s)
        s *= n
    return Carved(values, tuple(strides), fill, dtype, dev)


def _worst(got, ref, bound, cpg, what):
    """(worst error / bound, image, group) of a [B][HW][C] output"""
    assert bool(torch.isfinite(got).all()), f"NaN / Inf in {what}: a guard or another image was read into it"
    r = (got.to(F64) - ref).abs() / bound
    i = int(r.argmax())
    C = got.shape[-1]
    return float(r.reshape(-1)[i]), i // (got.shape[1] * C), (i % C) // cpg


class _Inputs:
    """x0 | x1, gamma, beta of one (row, pass) on the device, carved, with the fp64 operands of the reference"""

    def __init__(self, row, ps, dev, x=None):
        d = row.data(ps)
        x = d.x if x is None else x
        self.row, self.dev, self.B = row, dev, x.shape[0]
        B, HW, c0, c1 = self.B, row.HW, row.c0, row.c1
        self.x0c = _contig(x[..., :c0].to(F64), NAN, H16, dev)
        self.x1c = _contig(x[..., c0:].to(F64), NAN, H16, dev) if c1 else None
        self.gc, self.bc = _contig(d.gamma.to(F64), NAN, F32, dev), _contig(d.beta.to(F64), NAN, F32, dev)
        self.x64, self.gamma64, self.beta64 = x.to(dev).to(F64), d.gamma.to(dev).to(F64), d.beta.to(dev).to(F64)
        self.x0 = self.x0c.ptr()[:B * HW * c0].view(B * HW, c0)
        self.x1 = self.x1c.ptr()[:B * HW * c1].view(B * HW, c1) if c1 else None
        self.gamma, self.beta = self.gc.ptr()[:row.C], self.bc.ptr()[:row.C]

    def reference(self):
        r = self.row
        return gcc.fwd_reference(self.x64, self.gamma64, self.beta64, r.G, r.eps, r.silu, depth=r.depth, two_launch=r.two_launch)


def _assert_plan(row, pair=0):
    gcc.set_options(row.opts)
    assert row.plan(pair) == row.code, (row.name, row.plan(pair), ops.GN_VARIANTS.get(row.plan(pair)))


def _forward(row, ps, dev):
    """-> worst ratios (y, mean, rstd) and the largest relative rstd error"""
    _assert_plan(row)
    inp = _Inputs(row, ps, dev)
    ref = inp.reference()
    B, HW, C, G = row.B, row.HW, row.C, row.G
    yc = _contig(torch.full((B, HW, C), SENT16, dtype=F64), SENT16, H16, dev)
    sc = _contig(torch.full((B, G, 2), SENT32, dtype=F64), SENT32, F32, dev)
    pc = _contig(torch.full((B, row.nchunk, G, 2), SENT32, dtype=F64), SENT32, F32, dev)

    def launch():
        yb, sb, pb = yc.fresh(), sc.fresh(), pc.fresh()
        ops.groupnorm(inp.x0, B, HW, G, row.eps, inp.gamma, inp.beta, row.silu, x1=inp.x1, out=yc.ptr(yb), part=pc.ptr(pb),
                      stats=sc.ptr(sb))
        return yb, sb, pb
    yb, sb, pb = launch()
    torch.cuda.synchronize()
    assert yc.outside_untouched(yb), "a guard of y was written"
    assert sc.outside_untouched(sb), "a guard of the statistics was written"
    assert pc.outside_untouched(pb), "a guard of the partial table was written"
    st = sc.logical(sb)
    assert bool((st != SENT32).all()), "an (image, group) of the statistics was not written"
    assert bool(torch.isfinite(st).all()), "NaN / Inf in the statistics"
    r_y, b_y, g_y = _worst(yc.logical(yb), ref["y"], ref["bound_y"], row.cpg, "y")
    rm = (st[..., 0].to(F64) - ref["mean"]).abs() / ref["bound_mean"]
    rr = (st[..., 1].to(F64) - ref["rstd"]).abs() / ref["bound_rstd"]
    r_m, r_r = float(rm.max()), float(rr.max())
    rel_r = float(((st[..., 1].to(F64) - ref["rstd"]).abs() / ref["rstd"]).max())
    if ps == "flat":
        for b in range(B):
            g = gcc.flat_group(b, G)
            assert bool(torch.isfinite(yc.logical(yb)[b, :, g * row.cpg:(g + 1) * row.cpg]).all())
    yb2, sb2, _ = launch()
    assert torch.equal(_bits(yb2), _bits(yb)) and torch.equal(_bits(sb2), _bits(sb)), "a second launch is not bit-identical"
    print(f"[groupnorm] {row.name} / {ps}: y {r_y:.3f} at (image {b_y}, group {g_y}), mean {r_m:.3f} at {divmod(int(rm.argmax()), G)}, "
          f"rstd {r_r:.3f} at {divmod(int(rr.argmax()), G)} of the bound; rstd relative error {rel_r:.3e}")
    return r_y, r_m, r_r, rel_r


def _backward(row, ps, dev, accumulate):
    _assert_plan(row)
    inp = _Inputs(row, ps, dev)
    d = row.data(ps)
    B, HW, C, G, c0, c1 = row.B, row.HW, row.C, row.G, row.c0, row.c1
    fwd = inp.reference()
    stats = torch.stack([fwd["mean"], fwd["rstd"]], -1).to(F32)                 # as given: the fp32-rounded reference statistics
    stc = _contig(stats.cpu().to(F64), NAN, F32, dev)
    gyc = _contig(d.gy.to(F64), NAN, H16, dev)
    base = d.base.to(F64)
    ref = gcc.bwd_reference(inp.x64, d.gy.to(dev).to(F64), inp.gamma64, inp.beta64, stats[..., 0].to(F64), stats[..., 1].to(F64), G,
                            row.silu, depth=row.depth, slab=row.slab, base=base.to(dev) if accumulate else None)
    fill = lambda lo, hi: base[..., lo:hi] if accumulate else torch.full((B, HW, hi - lo), SENT16, dtype=F64)
    g0c = _contig(fill(0, c0), SENT16, H16, dev)
    g1c = _contig(fill(c0, C), SENT16, H16, dev) if c1 else None
    pc = _contig(torch.full((B, row.nchunk, G, 2), SENT32, dtype=F64), SENT32, F32, dev)

    def launch():
        b0, b1, pb = g0c.fresh(), (g1c.fresh() if c1 else None), pc.fresh()
        ops.groupnorm_bwd(gyc.ptr()[:B * HW * C].view(B * HW, C), inp.x0, B, HW, G, inp.gamma, inp.beta, row.silu,
                          stc.ptr()[:B * G * 2], x1=inp.x1, gx0=g0c.ptr(b0), gx1=g1c.ptr(b1) if c1 else None, part=pc.ptr(pb),
                          accumulate=accumulate)
        return b0, b1, pb
    b0, b1, pb = launch()
    torch.cuda.synchronize()
    assert g0c.outside_untouched(b0), "a guard of gx0 was written"
    assert pc.outside_untouched(pb), "a guard of the partial table was written"
    got = g0c.logical(b0)
    if c1:
        assert g1c.outside_untouched(b1), "a guard of gx1 was written"
        got = torch.cat([got, g1c.logical(b1)], -1)
    if not accumulate:
        assert bool((got != SENT16).all()), "an element of dx was not written"
    r, b_, g_ = _worst(got, ref["dx"], ref["bound_dx"], row.cpg, "dx")
    c0_, c1_, _ = launch()
    assert torch.equal(_bits(c0_), _bits(b0)) and (not c1 or torch.equal(_bits(c1_), _bits(b1))), "a second launch is not bit-identical"
    print(f"[groupnorm] {row.name} / {ps} / accumulate {int(accumulate)}: dx {r:.3f} at (image {b_}, group {g_}) of the bound")
    return r


@pytest.mark.parametrize("code", gcc.CODES, ids=[str(c) for c in gcc.CODES])
def test_groupnorm_code(dev, code):
    rows = gcc.rows_of(code)
    assert rows
    worst = {"y": 0.0, "mean": 0.0, "rstd": 0.0, "dx": 0.0}
    for row in rows:
        for ps in gcc.PASSES:
            if row.op == "fwd":
                r_y, r_m, r_r, _ = _forward(row, ps, dev)
                worst["y"], worst["mean"], worst["rstd"] = max(worst["y"], r_y), max(worst["mean"], r_m), max(worst["rstd"], r_r)
            else:
                worst["dx"] = max(worst["dx"], _backward(row, ps, dev, False))
        if row.op == "bwd":
            worst["dx"] = max(worst["dx"], _backward(row, "plain", dev, True))
    outs = ("y", "mean", "rstd") if rows[0].op == "fwd" else ("dx",)
    for o in outs:
        gate(f"groupnorm {code} ({ops.GN_VARIANTS[code]}): worst {o} error / derived bound", worst[o], 1.0)


def test_fused_and_two_launch_forms_of_one_shape(dev):
    """C = 1280 at 8x8 under "gn_fused" 256 and 0: both inside their own bounds on every pass; the rstd error of
    E[x^2] - mean^2 against the centred two-pass form on the "offset" pass (mean^2 / var = 256) is printed."""
    fused = gcc.ROWS_BY_NAME["104:fwd:C1280+0:HW64:B2:G32:silu:the fused form of the gn_fused 0 row"]
    two = gcc.ROWS_BY_NAME["201:fwd:C1280+0:HW64:B2:G32:silu:a small map on the two-launch kernels"]
    for ps in gcc.PASSES:
        rf, rt = _forward(fused, ps, dev), _forward(two, ps, dev)
        gate(f"fused form / {ps}: worst (y, mean, rstd) error / bound", max(rf[:3]), 1.0)
        gate(f"two-launch form / {ps}: worst (y, mean, rstd) error / bound", max(rt[:3]), 1.0)
        print(f"[groupnorm rstd] {ps}: relative rstd error two-launch {rt[3]:.3e}, fused {rf[3]:.3e}, ratio {rt[3] / max(rf[3], 1e-30):.1f}")


def test_slab_and_two_launch_backward_of_one_shape(dev):
    """C = 1280 + 1280 at 8x8 under "gn_slab" 1 and 0: both inside their own bounds."""
    slab = gcc.ROWS_BY_NAME["301:bwd:C1280+1280:HW64:B2:G32:silu:the slab form of the gn_slab 0 row"]
    two = gcc.ROWS_BY_NAME["400:bwd:C1280+1280:HW64:B2:G32:silu:two channel passes"]
    for acc in (False, True):
        gate(f"slab form / accumulate {int(acc)}: dx error / bound", _backward(slab, "plain", dev, acc), 1.0)
        gate(f"two-launch form / accumulate {int(acc)}: dx error / bound", _backward(two, "plain", dev, acc), 1.0)


@pytest.mark.parametrize("name", [r.name for r in gcc.PAIR_ROWS])
def test_groupnorm_pair_forms(dev, name):
    """B = 4, images 2 and 3 copies of images 0 and 1: HALF and DUP are bit-equal to the full launch in images < 2; HALF keeps
    the sentinel in the second half, DUP repeats the first half there."""
    row = gcc.ROWS_BY_NAME[name]
    d = row.data("plain")
    x = torch.cat([d.x[:2], d.x[:2]])
    inp = _Inputs(row, "plain", dev, x=x)
    ref = inp.reference()
    B, HW, C, G = row.B, row.HW, row.C, row.G
    yc = _contig(torch.full((B, HW, C), SENT16, dtype=F64), SENT16, H16, dev)
    pc = _contig(torch.full((B, row.nchunk, G, 2), SENT32, dtype=F64), SENT32, F32, dev)
    outs = {}
    for pair in (0, ops.PAIR_HALF, ops.PAIR_DUP):
        _assert_plan(row, pair)
        yb, pb = yc.fresh(), pc.fresh()
        ops.groupnorm(inp.x0, B, HW, G, row.eps, inp.gamma, inp.beta, row.silu, x1=inp.x1, out=yc.ptr(yb), part=pc.ptr(pb), pair=pair)
        torch.cuda.synchronize()
        assert yc.outside_untouched(yb) and pc.outside_untouched(pb), pair
        outs[pair] = yc.logical(yb)
    full, half, dup = outs[0], outs[ops.PAIR_HALF], outs[ops.PAIR_DUP]
    r_y, b_y, g_y = _worst(full, ref["y"], ref["bound_y"], row.cpg, "y")
    assert torch.equal(_bits(half[:2]), _bits(full[:2])), "PAIR_HALF differs from the full launch in the first half"
    assert bool((half[2:] == SENT16).all()), "PAIR_HALF wrote the second half"
    assert torch.equal(_bits(dup[:2]), _bits(full[:2])), "PAIR_DUP differs from the full launch in the first half"
    assert torch.equal(_bits(dup[2:]), _bits(dup[:2])), "PAIR_DUP: the second half is not the first"
    gate(f"groupnorm pair {name}: worst y error / derived bound at (image {b_y}, group {g_y})", r_y, 1.0)


def test_refusals_raise_and_write_nothing(dev):
    """The REFUSALS table with real addresses inside a sentinel buffer (operands 1 MiB apart)."""
    buf = torch.full((10 << 19,), SENT16, dtype=H16, device=dev)
    want = buf.clone()
    for fn, what, change in gcc.REFUSALS:
        with pytest.raises(RuntimeError):
            ops._call(fn, *gcc.refusal_args(fn, change, buf.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(want)), "a refused call wrote"
