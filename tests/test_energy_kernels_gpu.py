"""Both guidance-energy kernels (lgd_ca_energy_f32, lgd_boxdiff_energy_f32) on every form their launches accept
(tests/energy_cases.py): one test per entry point and kind (ca_energy) or smoothing (BoxDiff).  Per row the launch goes through
the ops wrapper on carved operands built from the RAW tables (NaN in front of and behind every floating input, and in the
padding of the mask and reference rows; sentinels around every output; the gradient maps prefilled with the sentinel) and

  * every loss, every partial and every gradient element is within its derived bound (the worst error / bound ratio is printed
    and gated at 1.0), nothing written is NaN or Inf;
  * exactly the gradient elements the header names are stored — ca_energy: the HW positions of every group's (map, image, head,
    token) column; BoxDiff: tokens 1 .. T-2 of every (map, image, head, position) — and every other element of the gradient
    buffers keeps the sentinel's bits (the reference holds the sentinel there with bound 0);
  * every guard keeps its bytes, all inputs (the integer tables included) are unchanged, a second launch is bit-identical;
  * gmaps = NULL gives the bits of the loss (and partials) of the launch with gradients;
  * a column of several items against the same items launched as one column each and added in table order in fp32.  The
    kernel adds item j as s_g += x_j y_j, which the compiler contracts into one fma, so the merged sum rounds once where the
    separate launches round the product and the sum: bitwise equality holds only where the product is exact (kind 0 with a
    grad_scale that is a power of two: asserted bit for bit); for the other columns both sides are within the bound of the
    same reference, so they differ by at most twice the bound (asserted);
  * the refusal tables raise and write nothing (every row of them returns before any launch: the CPU suite shows that).

Measured on an MI355X, worst error / bound per entry point and kind: ca_energy kind 0 0.616, kinds 0+1 0.308, 0+2 0.325,
0+1+2 0.324, kind 1 0.084, kinds 1+2 0.108, kind 2 0.103, no items 0 (exact); BoxDiff smooth NULL 0.125, Gaussian 0.220,
asymmetric 0.235.  The ca_energy ratios equal the fp32 emulation's of the CPU suite to three digits (the emulation follows the
kernel's order of operations); BoxDiff's differ in the second digit (0.134, 0.202, 0.222 there: exp against __expf).  Kind 0
sits highest, in its partial term: a handful of roundings behind two short sums of selected elements; kinds 1 and 2 lowest
because their bounds are led by the worst case of the block sums behind 1 / sum (ten additions deep), of which
a sum of positive terms realises about a tenth."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import lgd_amd  # noqa: E402,F401
from conftest import gate  # noqa: E402
from lgd_amd import ops  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import energy_cases as ec  # noqa: E402
from energy_cases import NAN, SENT, SENT32, Carved  # noqa: E402

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64


def _bits(t):
    return t.view(torch.int32)


def _carve(values, fill, dev):
    values = values.to(F32)
    strides, s = [], 1
    for n in reversed(values.shape):
        strides.insert(0, s)
        s *= n
    c = Carved(values.to(F64), tuple(strides), fill, F32, dev)
    c.shape = tuple(values.shape)
    return c


def _view(c, buf):
    n = 1
    for s in c.shape:
        n *= s
    return c.ptr(buf)[:n].view(c.shape)


class Operands:
    """The carved inputs of one row (shared by all its launches) and the recipe of its outputs."""

    def __init__(self, row, d, dev):
        self.row, self.d, self.dev = row, d, dev
        self.ins = {f"map{k}": _carve(m, NAN, dev) for k, m in enumerate(d["maps"])}
        self.ins["masks"] = _carve(d["masks"], NAN, dev)
        if row.entry == "ca_energy":
            self.ins["coefs"] = _carve(d["coefs"], NAN, dev)
            if d["refs"] is not None:
                self.ins["refs"] = _carve(d["refs"], NAN, dev)
        elif d["smooth"] is not None:
            self.ins["smooth"] = _carve(d["smooth"], NAN, dev)
        self.ints = {k: d[k].to(dev) for k in ("items", "groups", "map_hw", "dyn") if d.get(k) is not None}
        self.map_ptrs = torch.tensor([_view(self.ins[f"map{k}"], self.ins[f"map{k}"].buf).data_ptr() for k in range(len(d["maps"]))],
                                     dtype=I64, device=dev)

    def outputs(self, n_items):
        row, d = self.row, self.d
        S = row.S if row.entry == "ca_energy" else d["S"]
        outs = {"loss": _carve(torch.full((S,), SENT32), SENT32, self.dev)}
        if row.entry == "ca_energy":
            outs["partial"] = _carve(torch.full((max(n_items * row.H, 1),), SENT32), SENT32, self.dev)
        for k, m in enumerate(d["maps"]):
            outs[f"gmap{k}"] = _carve(torch.full(tuple(m.shape), SENT32), SENT32, self.dev)
        return outs

    def view(self, name):
        return _view(self.ins[name], self.ins[name].buf) if name in self.ins else None

    def check_inputs(self):
        for name, c in self.ins.items():
            assert torch.equal(_bits(c.buf), _bits(c.host.to(self.dev))), f"{self.row.name}: input {name} was written"
        for name, t in self.ints.items():
            assert torch.equal(t.cpu(), self.d[name]), f"{self.row.name}: the {name} table was written"


class Launch:
    """One launch: fresh output buffers; `only` = one item of the table launched as a column of its own (ca_energy)."""

    def __init__(self, op, *, grads=True, only=None):
        row, d, dev = op.row, op.d, op.dev
        n_items = d["n_items"] if only is None else 1
        self.outs = op.outputs(n_items)
        self.bufs = {n: c.fresh() for n, c in self.outs.items()}
        self.out = {n: _view(c, self.bufs[n]) for n, c in self.outs.items()}
        n_maps = len(d["maps"])
        gp = torch.tensor([self.out[f"gmap{k}"].data_ptr() for k in range(n_maps)], dtype=I64, device=dev) if grads else None
        self.keep = gp
        if row.entry == "ca_energy":
            items, coefs, groups, n_groups = op.ints["items"], op.view("coefs"), op.ints["groups"], d["n_groups"]
            if only is not None:
                items, coefs = items[only:only + 1].contiguous(), coefs[only:only + 1]
                groups, n_groups = torch.tensor([[0, 1]], dtype=I32, device=dev), 1
            ops.ca_energy(op.map_ptrs, gp, op.ints["map_hw"], items, coefs, op.view("masks"), op.view("refs"), d["stride"],
                          op.ints.get("dyn"), groups, n_groups, n_items, row.H, row.T, d["max_hw"], self.out["partial"],
                          self.out["loss"], grad_scale=row.gscale, n_samples=row.S)
        else:
            ops.boxdiff_energy(op.map_ptrs, gp, n_maps, row.side, op.ints["items"], op.view("masks"), op.view("smooth"),
                               op.ints["groups"], d["S"], d["max_items"], row.H, row.T, row.ls, row.gs, self.out["loss"])
        torch.cuda.synchronize()

    def check_guards(self, name):
        for n, c in self.outs.items():
            assert c.outside_untouched(self.bufs[n]), f"{name}: a guard of {n} was written"


def _run(row, dev):
    """-> the worst error / bound over the outputs of one row"""
    d = row.data()
    ref = ec.outputs(ec.reference(row, d))
    op = Operands(row, d, dev)
    first = Launch(op)
    first.check_guards(row.name)
    op.check_inputs()
    worst = 0.0
    for name, (want, bound) in ref.items():
        got = first.out[name].cpu().reshape(want.shape)
        stored = want != SENT
        assert bool(torch.isfinite(got[stored]).all()), f"{row.name}: NaN or Inf in {name}: a guard or a padding was read into it"
        assert bool((got[stored] != SENT).all()), f"{row.name}: an element of {name} the header names was not stored"
        assert torch.equal(_bits(got[~stored].contiguous()), _bits(torch.full_like(got[~stored], SENT32))), \
            f"{row.name}: an element of {name} the header does not name was written"
        r = ec.worst_ratio(got, want, bound, fp16=False)
        if r >= 1.0:
            print(f"[energy kernels] {row.name}: {name} at {r:.4f} of the bound")
        worst = max(worst, r)
    if "partial" not in ref:                              # BoxDiff has none; ca_energy without items stores none
        assert "partial" not in first.out or bool((first.out["partial"] == SENT32).all()), f"{row.name}: partial was written"
    second = Launch(op)
    second.check_guards(row.name)
    for name in first.out:
        assert torch.equal(_bits(second.out[name]), _bits(first.out[name])), f"{row.name}: a second launch of {name} differs"
    value = Launch(op, grads=False)
    value.check_guards(row.name)
    for name in first.out:
        if name.startswith("gmap"):
            assert bool((value.out[name] == SENT32).all()), f"{row.name}: {name} was written by a launch without gmaps"
        else:
            assert torch.equal(_bits(value.out[name]), _bits(first.out[name])), f"{row.name}: {name} without gmaps differs"
    if row.entry == "ca_energy":
        _merged_columns(row, d, op, first, ref)
    op.check_inputs()
    return worst


def _merged_columns(row, d, op, merged, ref):
    pow2 = math.frexp(float(row.gscale))[0] == 0.5       # grad_scale a power of two: the product with it is exact
    items = d["items"].tolist()
    for first, count in d["groups"].tolist()[:d["n_groups"]]:
        if count < 2:
            continue
        mp, _, tok, _, _, _, _, img = items[first]
        acc = None
        for it in range(first, first + count):
            single = Launch(op, only=it)
            single.check_guards(row.name)
            col = single.out[f"gmap{mp}"][img, :, :, tok]
            assert torch.equal(_bits(single.out["partial"][:row.H]), _bits(merged.out["partial"][it * row.H:(it + 1) * row.H])), \
                f"{row.name}: the partial of item {it} depends on its column"
            acc = col.clone() if acc is None else acc + col
        got = merged.out[f"gmap{mp}"][img, :, :, tok]
        if pow2 and all(items[it][1] == 0 for it in range(first, first + count)):
            assert torch.equal(_bits(got.contiguous()), _bits(acc.contiguous())), f"{row.name}: the merged column differs from its items added in order"
        else:
            bound = ref[f"gmap{mp}"][1][img, :, :, tok]
            diff = (got.cpu().to(F64) - acc.cpu().to(F64)).abs()
            assert bool((diff <= 2.0 * bound).all()), f"{row.name}: the merged column is further than twice the bound from its items added in order"


@pytest.mark.parametrize("label", ec.LABELS)
def test_energy_kernel(dev, label):
    rows = [r for r in ec.rows_of(label.split()[0]) if ec.kinds_of(r) == label]
    assert rows
    worst, at = 0.0, None
    for row in rows:
        r = _run(row, dev)
        if r > worst:
            worst, at = r, row.name
    print(f"[energy kernels] {label}: worst error / bound {worst:.4f} at {at}")
    gate(f"{label}: worst error / derived bound", worst, 1.0)


def test_refused_calls_raise_and_write_nothing(dev):
    """REFUSALS and UNSUPPORTED with real addresses inside a sentinel buffer (operands 1 MiB apart)."""
    buf = torch.full((12 << 18,), SENT32, dtype=F32, device=dev)
    want = buf.clone()
    for fn, what, change in ec.REFUSALS + ec.UNSUPPORTED:
        with pytest.raises(RuntimeError):
            ops._call(fn, *ec.call_args(fn, change, buf.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(want)), "a refused call wrote"
