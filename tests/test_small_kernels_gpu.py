"""Every small kernel (csrc/misc.hip, lgd_act_f16) on every form its entry point accepts (tests/small_kernel_cases.py): one
test per entry point.  Per row and data pass the launch goes through the ops wrapper on carved operands (NaN in front of and
behind every input, sentinels around every output) and

  * every output element is within its derived bound (the worst error / bound ratio is printed and gated at 1.0), nothing
    written is NaN or Inf where the reference is finite, an overflowing fp16 result is the infinity of its sign;
  * every guard keeps its bytes, inputs that are not outputs are unchanged, every logical output element was written (no
    reference equals the sentinel), a second launch is bit-identical;
  * every in-place form the header allows gives the bits of the out-of-place launch;
  * the refusal table raises and writes nothing (every row of it returns before any launch: the CPU suite shows that).

Measured on an MI355X, worst error / bound per entry point: act_gelu 0.9995, act_relu 0 (exact), add 0.9994, axpy 0.832,
cfg_ddim 0.902, cfg_multistep 0.943, conv_in 0.957, conv_out 0.155, geglu_bwd 0.9988, geglu_fwd 0.9988, nchw_to_nhwc8 0 (bit-exact),
quick_gelu 0.9995, scale 0.993, scale_rows 0.729, select_row 0 (bit-exact), softmax_rows 0.9994, upsample2x_bwd 0.990.  The fp16
outputs sit at the half-ulp, the first term of their bounds; the fp32 outputs (the steps, axpy, scale_rows, the convolutions'
sums) at a fraction of the roundings the bound counts, conv_out lowest because its 9 Cin products spread over 64 lanes."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import lgd_amd  # noqa: E402,F401
from conftest import gate  # noqa: E402
from lgd_amd import ops  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_kernel_cases as skc  # noqa: E402
from small_kernel_cases import NAN, SENT16, SENT32, STEP, T_STEPS, Carved  # noqa: E402

H16, F32, F64, I32 = torch.float16, torch.float32, torch.float64, torch.int32


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _contig(values, fill, dtype, dev):
    strides, s = [], 1
    for n in reversed(values.shape):
        strides.insert(0, s)
        s *= n
    return Carved(values, tuple(strides), fill, dtype, dev)


def _view(c, buf, shape):
    n = 1
    for s in shape:
        n *= s
    return c.ptr(buf)[:n].view(shape)


class Spec:
    """How one entry point is launched: `ins` the floating operands of row.data it reads (None = left out), `outs` name ->
    (dtype, shape) of what it writes, `inout` outputs that are an input's buffer by definition, `alias(row)` outputs that are
    an input's buffer in this row's form, `call(row, d, T)` the wrapper call on the views T, `region(row, name, t)` the part of
    output `name` the reference describes."""
    inout = {}

    def alias(self, row):
        return {}

    def region(self, row, name, t):
        return t


def _maybe(d, *names):
    return [n for n in names if d.get(n) is not None]


class _Unary(Spec):
    def __init__(self, fn):
        self.fn = fn

    def ins(self, row, d):
        return _maybe(d, "a", "b")

    def outs(self, row, d):
        return {"y": (H16, d["a"].shape)}

    def alias(self, row):
        return {"y": row.inplace[0]} if row.inplace else {}

    def call(self, row, d, T):
        if row.entry == "add":
            b = T["a"] if row.inplace == "ab" else T["b"]
            ops.add(T["a"], b, T["y"])
        else:
            self.fn(T["a"], T["y"])


class _Geglu(Spec):
    def ins(self, row, d):
        return _maybe(d, "h", "gy")

    def outs(self, row, d):
        return {"gh": (H16, d["h"].shape)} if "gy" in d else {"y": (H16, d["v"].shape)}

    def call(self, row, d, T):
        if "gy" in d:
            ops.geglu_bwd(T["h"], T["gy"], T["gh"])
        else:
            ops.geglu_fwd(T["h"], T["y"])


class _Upsample(Spec):
    def ins(self, row, d):
        return ["gy"]

    def outs(self, row, d):
        return {"gx": (H16, (row.B * row.H * row.W, row.C))}

    def call(self, row, d, T):
        ops.upsample2x_bwd(T["gy"].view(-1, row.C), row.B, row.H, row.W, row.C, out=T["gx"])

    def region(self, row, name, t):
        return t.view(row.B, row.H * row.W, row.C)


class _Softmax(Spec):
    def ins(self, row, d):
        return ["x"]

    def outs(self, row, d):
        return {"y": (H16, d["x"].shape)}

    def alias(self, row):
        return {"y": "x"} if row.inplace else {}

    def call(self, row, d, T):
        ops.softmax_rows(T["x"], row.scale, out=T["y"])


class _Nhwc8(Spec):
    def ins(self, row, d):
        return ["x"]

    def outs(self, row, d):
        return {"y": (H16, (row.B * row.HW, 8))}

    def call(self, row, d, T):
        ops.nchw_to_nhwc8(T["x"].view(row.B, row.C, row.HW, 1), out=T["y"])


class _ConvOut(Spec):
    def ins(self, row, d):
        return _maybe(d, "x", "w", "bias")

    def outs(self, row, d):
        return {"y": (F32, (row.B, row.Cout, row.L, row.L))}

    def call(self, row, d, T):
        ops.conv_out(T["x"].view(-1, row.Cin), T["w"], T.get("bias"), row.B, row.L, out=T["y"], out_scale=row.out_scale)


class _ConvIn(Spec):
    def ins(self, row, d):
        return _maybe(d, "x", "w", "bias")

    def outs(self, row, d):
        return {"y": (H16, (row.B * row.L * row.L, row.Cout))}

    def call(self, row, d, T):
        ops.conv_in(T["x"], T["w"], T.get("bias"), out=T["y"])


class _Step(Spec):
    def __init__(self, multistep):
        self.multistep = multistep
        self.inout = {"x0_prev": "x0_prev"} if multistep else {}

    def ins(self, row, d):
        return _maybe(d, "eps", "x", "table", "frozen_ref", "mask", "x0_prev")

    def outs(self, row, d):
        o = {} if row.inplace else {"x_out": (F32, d["x"].shape)}
        if row.hist:
            o["hist"] = (F32, (T_STEPS + 1,) + tuple(d["x"].shape))
        return o

    def alias(self, row):
        return {"x_out": "x"} if row.inplace else {}

    def call(self, row, d, T):
        kw = dict(frozen_ref=T.get("frozen_ref"), mask=T.get("mask"), hist=T.get("hist"))
        if self.multistep:
            ops.cfg_multistep_step(T["eps"], T["x"], T["x_out"], T["x0_prev"], T["table"], T["dyn"], **kw)
        else:
            ops.cfg_ddim_step(T["eps"], T["x"], T["x_out"], T["table"], T["dyn"], **kw)

    def region(self, row, name, t):
        if name != "hist":
            return t
        rest = torch.cat([t[:STEP + 1], t[STEP + 2:]])
        assert bool((rest == SENT32).all()), "hist was written outside step + 1"
        return t[STEP + 1]


class _Axpy(Spec):
    inout = {"x": "x"}

    def ins(self, row, d):
        return _maybe(d, "g", "x", "table", "active")

    def outs(self, row, d):
        return {}

    def call(self, row, d, T):
        ops.axpy(T["g"], T["x"], T["table"], T["step_idx"], row.col, active=T.get("active"))


class _ScaleRows(Spec):
    def ins(self, row, d):
        return ["x", "table"]

    def outs(self, row, d):
        return {"out": (F32, (row.reps, row.n))}

    def call(self, row, d, T):
        ops.scale_rows(T["x"], T["out"], T["table"], T["dyn"], row.col, reps=row.reps)


class _SelectRow(Spec):
    def ins(self, row, d):
        return ["table"]

    def outs(self, row, d):
        return {"out": (F32, (row.n,))}

    def call(self, row, d, T):
        ops.select_row(T["table"], T["idx"], T["out"])


SPECS = {"add": _Unary(None), "scale": _Unary(lambda a, y: ops.scale(a, skc.ALPHA, y)), "quick_gelu": _Unary(lambda a, y: ops.quick_gelu(a, y)),
         "act_gelu": _Unary(lambda a, y: ops.act(a, ops.ACT_GELU, y)), "act_relu": _Unary(lambda a, y: ops.act(a, ops.ACT_RELU, y)),
         "geglu_fwd": _Geglu(), "geglu_bwd": _Geglu(), "upsample2x_bwd": _Upsample(), "softmax_rows": _Softmax(),
         "nchw_to_nhwc8": _Nhwc8(), "conv_out": _ConvOut(), "conv_in": _ConvIn(), "cfg_ddim": _Step(False),
         "cfg_multistep": _Step(True), "axpy": _Axpy(), "scale_rows": _ScaleRows(), "select_row": _SelectRow()}
assert set(SPECS) == set(skc.ENTRIES)


class _Launch:
    """One launch of (row, data) with the outputs named in `alias` living in an input's buffer."""

    def __init__(self, row, d, carved_in, carved_out, alias, dev):
        spec = SPECS[row.entry]
        written = dict(spec.inout, **alias)               # output -> the input whose buffer it is
        self.bufs, self.out = {}, {}
        T = {k: v.to(dev) for k, v in d.items() if isinstance(v, torch.Tensor) and v.dtype == I32}
        for name, c in carved_in.items():
            buf = c.fresh() if name in written.values() else c.buf
            self.bufs[name] = (c, buf)
            T[name] = _view(c, buf, d[name].shape)
        for name, c in carved_out.items():
            if name in written:
                continue
            buf = c.fresh()
            self.bufs["out:" + name] = (c, buf)
            T[name] = _view(c, buf, c.shape)
            self.out[name] = T[name]
        for o, i in written.items():
            T.setdefault(o, T[i])
            self.out[o] = T[i]
        spec.call(row, d, T)

    def check_guards(self, written_inputs):
        for name, (c, buf) in self.bufs.items():
            if name.startswith("out:") or name in written_inputs:
                assert c.outside_untouched(buf), f"a guard of {name} was written"
            else:
                assert torch.equal(_bits(buf), _bits(c.host.to(buf.device))), f"input {name} was written"


def _run(row, ps, dev):
    """-> the worst error / bound over the outputs of one (row, pass)"""
    spec = SPECS[row.entry]
    d = row.data(ps)
    ref = skc.reference(row, skc.on(d, dev))
    carved_in = {n: _contig(d[n].to(F64), NAN, d[n].dtype, dev) for n in spec.ins(row, d)}
    carved_out = {}
    for n, (dt, shape) in spec.outs(row, d).items():
        sent = SENT16 if dt == H16 else SENT32
        carved_out[n] = _contig(torch.full(tuple(shape), sent, dtype=F64), sent, dt, dev)
        carved_out[n].shape = tuple(shape)
    alias = spec.alias(row)
    written_inputs = set(dict(spec.inout, **alias).values())
    first = _Launch(row, d, carved_in, carved_out, alias, dev)
    torch.cuda.synchronize()
    first.check_guards(written_inputs)
    worst = 0.0
    for name, (want, bound) in ref.items():
        if name not in first.out:
            continue                                      # hist of a row without one
        fp16 = skc.ENTRIES[row.entry].outputs[name] == H16
        got = spec.region(row, name, first.out[name]).reshape(want.shape)
        finite = torch.isfinite(want) & ((want.abs() < 65520.0) if fp16 else torch.ones_like(want, dtype=torch.bool))
        assert bool(torch.isfinite(got[finite]).all()), f"{row.name} / {ps}: NaN or Inf in {name}: a guard was read into it"
        if name not in written_inputs and name not in spec.inout:
            assert bool((got != (SENT16 if fp16 else SENT32)).all()), f"{row.name} / {ps}: an element of {name} was not written"
        worst = max(worst, skc.worst_ratio(got, want, bound, fp16=fp16))
    second = _Launch(row, d, carved_in, carved_out, alias, dev)
    torch.cuda.synchronize()
    second.check_guards(written_inputs)
    for name in first.out:
        assert torch.equal(_bits(second.out[name]), _bits(first.out[name])), f"{row.name} / {ps}: a second launch of {name} differs"
    if alias:                                             # the in-place form against the out-of-place launch
        plain_outs = dict(carved_out)
        for o, i in alias.items():
            src = d[i]
            dt = skc.ENTRIES[row.entry].outputs[o]
            sent = SENT16 if dt == H16 else SENT32
            plain_outs[o] = _contig(torch.full(tuple(src.shape), sent, dtype=F64), sent, dt, dev)
            plain_outs[o].shape = tuple(src.shape)
        plain = _Launch(row, d, carved_in, plain_outs, {}, dev)
        torch.cuda.synchronize()
        plain.check_guards(set(spec.inout.values()))
        for name in first.out:
            assert torch.equal(_bits(plain.out[name]), _bits(first.out[name])), f"{row.name} / {ps}: in place, {name} differs from out of place"
    return worst


@pytest.mark.parametrize("entry", sorted(skc.ENTRIES))
def test_small_kernel(dev, entry):
    rows = skc.rows_of(entry)
    assert rows
    worst, at = 0.0, None
    for row in rows:
        for ps in row.passes:
            r = _run(row, ps, dev)
            if r > worst:
                worst, at = r, f"{row.name} / {ps}"
            if r >= 1.0:
                print(f"[small kernels] {row.name} / {ps}: {r:.4f} of the bound")
    print(f"[small kernels] {entry}: worst error / bound {worst:.4f} at {at}")
    gate(f"{entry}: worst error / derived bound", worst, 1.0)


def test_refused_calls_raise_and_write_nothing(dev):
    """The REFUSALS table with real addresses inside a sentinel buffer (operands 1 MiB apart)."""
    buf = torch.full((10 << 19,), SENT16, dtype=H16, device=dev)
    want = buf.clone()
    for fn, what, change in skc.REFUSALS + skc.UNSUPPORTED:
        with pytest.raises(RuntimeError):
            ops._call(fn, *skc.call_args(fn, change, buf.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(want)), "a refused call wrote"
