"""Every small kernel (csrc/misc.hip, csrc/sam.hip) on every form its entry point accepts (tests/small_kernel_cases.py): one
test per entry point.  Per row and data pass the launch goes through the ops wrapper on carved operands (NaN in front of and
behind every input, sentinels around every output) and

  * every output element is within its derived bound (the worst error / bound ratio is printed and gated at 1.0), nothing
    written is NaN or Inf where the reference is finite, an overflowing fp16 result is the infinity of its sign;
  * every guard keeps its bytes, inputs that are not outputs are unchanged, every logical output element was written (no
    reference equals the sentinel), a second launch is bit-identical;
  * every in-place form the header allows gives the bits of the out-of-place launch;
  * a form that writes nothing leaves the sentinel in every output element (dyn outside [0, n_steps), the value / count of a
    single chunk) and every bit of x_in (the last step); ring slots and the saved sample that are not pushed or saved keep their
    bits; a row of the views entry is the launches of all chunks of a step, and every chunking gives the same latent bits;
  * the refusal table raises and writes nothing (every row of it returns before any launch: the CPU suite shows that).

Measured on an MI355X, worst error / bound per entry point: act_gelu 0.9995, act_relu 0 (exact), add 0.9994, axpy 0.832,
cfg_ddim 0.902, cfg_multistep 0.943, conv_in 0.957, conv_out 0.155, geglu_bwd 0.9988, geglu_fwd 0.9988, nchw_to_nhwc8 0 (bit-exact),
quick_gelu 0.9995, scale 0.993, scale_rows 0.729, select_row 0 (bit-exact), softmax_rows 0.9994, upsample2x_bwd 0.990; cfg_plms
0.987, md_step 0.492, md_views 0.611, image_u8 0 (bit-exact), vae_sample 0.846 (expf over every finite fp16 log-variance: at
most 0.776 ulp), sam_relpos_qkv 0.978 (the fp16 half-ulp of a rel column), sam_window_merge 0 (bit-exact).  The fp16
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
from small_kernel_cases import MD_BOOT, MD_STEPS, NAN, PLMS_EVALS, SENT16, SENT32, STEP, T_STEPS, Carved  # noqa: E402

H16, F32, F64, I32 = torch.float16, torch.float32, torch.float64, torch.int32


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a.contiguous()).reshape(-1), _bits(b.to(a.device).contiguous()).reshape(-1))


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
    (dtype, shape) of what it writes, `inout` / `inout_of(row)` outputs that are an input's buffer by definition, `alias(row)`
    outputs that are an input's buffer in this row's form, `call(row, d, T)` the wrapper call(s) on the views T,
    `region(row, name, t)` the part of output `name` the reference describes, `unwritten(row)` the outputs that have to keep
    the sentinel in every element, `check(row, d, out)` what else a launch has to leave behind (bits that have to stay),
    `fill` what surrounds an input."""
    inout = {}
    fill = NAN

    def inout_of(self, row):
        return self.inout

    def alias(self, row):
        return {}

    def unwritten(self, row):
        return ()

    def check(self, row, d, out):
        pass

    def region(self, row, name, t):
        return t


def _hist_slot(t, slot):
    """hist[slot] of a history that keeps the sentinel everywhere else"""
    rest = torch.cat([t[:slot], t[slot + 1:]])
    assert bool((rest == SENT32).all()), "hist was written outside step + 1"
    return t[slot]


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
        return _hist_slot(t, STEP + 1) if name == "hist" else t


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


class _Plms(Spec):
    inout = {"ets": "ets", "cur_sample": "cur_sample"}

    def ins(self, row, d):
        return ["eps", "x", "table", "ets", "cur_sample"]

    def outs(self, row, d):
        o = {} if row.inplace else {"x_out": (F32, d["x"].shape)}
        if row.hist:
            o["hist"] = (F32, (PLMS_EVALS + 1,) + tuple(d["x"].shape))
        return o

    def alias(self, row):
        return {"x_out": "x"} if row.inplace else {}

    def call(self, row, d, T):
        ops.cfg_plms_step(T["eps"], T["x"], T["x_out"], T["ets"], T["cur_sample"], T["table"], T["dyn"], hist=T.get("hist"))

    def region(self, row, name, t):
        if name == "hist":
            return _hist_slot(t, row.k + 1)
        if name == "ets":
            return t[int(skc.plms_table(row.vpred)[row.k][7])]
        return t

    def check(self, row, d, out):
        c = skc.plms_table(row.vpred)[row.k]
        for s in range(3):
            if s != int(c[7]):
                assert _same_bits(out["ets"][s], d["ets"][s]), f"{row.name}: ring slot {s} was written"
        if float(c[9]) == 0.0:
            assert _same_bits(out["cur_sample"], d["cur_sample"]), f"{row.name}: cur_sample was written"
        else:
            assert _same_bits(out["cur_sample"], d["x"]), f"{row.name}: cur_sample is not x bit for bit"


class _MdStep(Spec):
    def _writes(self, row):
        return 0 <= row.step < MD_STEPS

    def ins(self, row, d):
        return _maybe(d, "eps", "latent", "masks", "bg", "noise", "table") + ([] if row.prep else ["x_in"])

    def inout_of(self, row):
        return {} if row.prep else {"x_in": "x_in"}

    def outs(self, row, d):
        if row.prep:
            return {"x_in": (F32, d["x_in"].shape)}
        o = {"latent": (F32, (row.C, row.HW, 1))}
        if row.hist:
            o["hist"] = (F32, (MD_STEPS + 1, row.C, row.HW, 1))
        return o

    def unwritten(self, row):
        return () if (row.prep or self._writes(row)) else (("latent", "hist") if row.hist else ("latent",))

    def call(self, row, d, T):
        ops.multidiffusion_step(T.get("eps"), T["x_in"], T["latent"], T["masks"], T["table"], T["dyn"], n_prompts=row.P,
                                n_steps=MD_STEPS, bg=T.get("bg"), noise=T.get("noise"), picks=T.get("picks"), n_boot=MD_BOOT,
                                hist=T.get("hist"), prep=bool(row.prep))

    def region(self, row, name, t):
        return _hist_slot(t, row.step + 1) if name == "hist" else t

    def check(self, row, d, out):
        x = out["x_in"]
        nxt = row.step if row.prep else row.step + 1
        if not self._writes(row) or nxt >= MD_STEPS:          # dyn out of range, the last step: x_in keeps every bit
            assert _same_bits(x, d["x_in"]), f"{row.name}: x_in was written"
            return
        Pp = row.Pp
        assert _same_bits(x[Pp:], x[:Pp]), f"{row.name}: the cond half of x_in is not the uncond half bit for bit"
        lat = d["latent"] if row.prep else out["latent"]
        for k in [0] + list(range(row.P, Pp)):                # row 0 and the padding rows are the latent itself
            assert _same_bits(x[k], lat), f"{row.name}: x_in row {k} is not the latent bit for bit"


class _MdViews(Spec):
    def __init__(self):
        self.latents = {}                                     # row key without nvc -> (row name, latent bits)

    def _geo(self, row):
        _, _, V_ = skc.md_views(row.Hp, row.Wp)
        return V_, skc.md_chunks(V_, row.nvc)

    def ins(self, row, d):
        return _maybe(d, "latent", "masks", "bg", "noise", "table", "eps", "x_in", "value", "count")

    def inout_of(self, row):
        return {"value": "value", "count": "count"} if (not row.prep and len(self._geo(row)[1]) > 1) else {}

    def outs(self, row, d):
        _, chunks = self._geo(row)
        if row.prep:
            return {"x_in": (F32, (len(chunks), 2 * row.nvc * row.Pp, row.C, 64, 64))}
        o = {"latent": (F32, (row.C, row.Hp, row.Wp))}
        if row.hist:
            o["hist"] = (F32, (MD_STEPS + 1, row.C, row.Hp, row.Wp))
        if len(chunks) == 1 and not row.nullvc:
            o["value"] = o["count"] = (F32, (row.C, row.Hp, row.Wp))
        return o

    def unwritten(self, row):
        return ("value", "count") if (not row.prep and len(self._geo(row)[1]) == 1 and not row.nullvc) else ()

    def call(self, row, d, T):
        V_, chunks = self._geo(row)
        kw = dict(n_prompts=row.P, rows_per_view=row.Pp, n_views=V_, n_steps=MD_STEPS, indep_uncond=bool(row.indep),
                  normalization=bool(row.norm), bg=T.get("bg"), noise=T.get("noise"), picks=T.get("picks"), n_boot=MD_BOOT)
        for ci, (v0, nv) in enumerate(chunks):
            if row.prep:
                ops.multidiffusion_views(None, T["x_in"][ci], T["latent"], None, None, T["masks"], T["table"], T["dyn"], v0=v0, nv=nv,
                                         prep=True, **kw)
            else:
                ops.multidiffusion_views(T["eps"][ci], T["x_in"][ci], T["latent"], T.get("value"), T.get("count"), T["masks"],
                                         T["table"], T["dyn"], v0=v0, nv=nv, hist=T.get("hist"), **kw)

    def region(self, row, name, t):
        if name == "hist":
            return _hist_slot(t, row.step + 1)
        if name != "x_in":
            return t
        Pp, nvc = row.Pp, row.nvc
        views, written = [], torch.zeros(t.shape[:2], dtype=torch.bool, device=t.device)
        for ci, (v0, nv) in enumerate(self._geo(row)[1]):
            for j in range(nv):
                views.append(torch.stack([t[ci, j * Pp:(j + 1) * Pp], t[ci, (nvc + j) * Pp:(nvc + j + 1) * Pp]]))
                written[ci, j * Pp:(j + 1) * Pp] = written[ci, (nvc + j) * Pp:(nvc + j + 1) * Pp] = True
        assert bool((t[~written] == SENT32).all()), f"{row.name}: x_in rows of views outside [0, nv) were written"
        return torch.stack(views)                             # [V][half][Pp][C][64][64]

    def check(self, row, d, out):
        if row.prep:
            return
        if len(self._geo(row)[1]) > 1 and not row.norm:
            assert _same_bits(out["count"], d["count"]), f"{row.name}: count was written without normalization"
        name, bits = self.latents.setdefault(skc.ENTRIES["md_views"].key(row), (row.name, _bits(out["latent"]).clone()))
        assert torch.equal(bits, _bits(out["latent"])), f"{row.name}: the latent differs from the chunking of {name}"


class _ImageU8(Spec):
    fill = 165.0

    def ins(self, row, d):
        return ["img"]

    def outs(self, row, d):
        return {"y": (H16, (row.B * row.HW, 8))}

    def call(self, row, d, T):
        ops.image_u8_to_nhwc8(T["img"].view(row.B, row.HW, 1, 3), out=T["y"])


class _VaeSample(Spec):
    def ins(self, row, d):
        return ["moments", "noise"]

    def outs(self, row, d):
        return {"out": (F32, d["noise"].shape)}

    def call(self, row, d, T):
        ops.vae_sample(T["moments"], T["noise"], row.scale, out=T["out"])

    def check(self, row, d, out):
        if row.sweep:                                         # mean 0, noise 1, scale 1: out is expf(0.5 clamp(lv)) itself
            h = 0.5 * d["moments"][:, row.z:].to(out["out"].device, F64).clamp(-30.0, 20.0)
            want = h.exp().reshape(row.B, row.HW, row.z).transpose(1, 2).reshape(-1)
            ulp = 2.0 ** (torch.floor(torch.log2(want)) - 23)
            err = ((out["out"].reshape(-1).to(F64) - want).abs() / ulp).max()
            print(f"[small kernels] expf over every finite fp16 log-variance: largest error {float(err):.3f} ulp")


class _SamRelpos(Spec):
    def ins(self, row, d):
        return ["qkv", "qkv_bias", "rel_h", "rel_w"]

    def outs(self, row, d):
        rows = skc.sam_geometry(row)[1].numel()
        return {n: (H16, (rows, row.NH * row.DA)) for n in ("qa", "ka", "va")}

    def call(self, row, d, T):
        ops.sam_relpos_qkv(T["qkv"], T["qkv_bias"], T["rel_h"], T["rel_w"], row.B, row.Hs, row.Ws, row.window, row.NH, row.d,
                           row.DA, skc.sam_scale(row), qa=T["qa"], ka=T["ka"], va=T["va"])


class _SamMerge(Spec):
    def ins(self, row, d):
        return ["oa"]

    def outs(self, row, d):
        return {"out": (H16, (row.B * row.Hs * row.Ws, row.NH * row.d))}

    def call(self, row, d, T):
        ops.sam_window_merge(T["oa"], row.B, row.Hs, row.Ws, row.window, row.NH, row.d, row.DA, out=T["out"])


SPECS = {"cfg_plms": _Plms(), "md_step": _MdStep(), "md_views": _MdViews(), "image_u8": _ImageU8(), "vae_sample": _VaeSample(),
         "sam_relpos_qkv": _SamRelpos(), "sam_window_merge": _SamMerge(),
         "add": _Unary(None), "scale": _Unary(lambda a, y: ops.scale(a, skc.ALPHA, y)), "quick_gelu": _Unary(lambda a, y: ops.quick_gelu(a, y)),
         "act_gelu": _Unary(lambda a, y: ops.act(a, ops.ACT_GELU, y)), "act_relu": _Unary(lambda a, y: ops.act(a, ops.ACT_RELU, y)),
         "geglu_fwd": _Geglu(), "geglu_bwd": _Geglu(), "upsample2x_bwd": _Upsample(), "softmax_rows": _Softmax(),
         "nchw_to_nhwc8": _Nhwc8(), "conv_out": _ConvOut(), "conv_in": _ConvIn(), "cfg_ddim": _Step(False),
         "cfg_multistep": _Step(True), "axpy": _Axpy(), "scale_rows": _ScaleRows(), "select_row": _SelectRow()}
assert set(SPECS) == set(skc.ENTRIES)


class _Launch:
    """One launch of (row, data) with the outputs named in `alias` living in an input's buffer."""

    def __init__(self, row, d, carved_in, carved_out, alias, dev):
        spec = SPECS[row.entry]
        written = dict(spec.inout_of(row), **alias)       # output -> the input whose buffer it is
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
    carved_in = {n: _contig(d[n].to(F64), spec.fill, d[n].dtype, dev) for n in spec.ins(row, d)}
    carved_out = {}
    for n, (dt, shape) in spec.outs(row, d).items():
        sent = SENT16 if dt == H16 else SENT32
        carved_out[n] = _contig(torch.full(tuple(shape), sent, dtype=F64), sent, dt, dev)
        carved_out[n].shape = tuple(shape)
    alias = spec.alias(row)
    inout = spec.inout_of(row)
    written_inputs = set(dict(inout, **alias).values())
    first = _Launch(row, d, carved_in, carved_out, alias, dev)
    torch.cuda.synchronize()
    first.check_guards(written_inputs)
    for name in spec.unwritten(row):
        assert bool((first.out[name] == SENT32).all()), f"{row.name} / {ps}: {name} was written"
    spec.check(row, d, first.out)
    worst = 0.0
    for name, (want, bound) in ref.items():
        if name not in first.out:
            continue                                      # hist of a row without one
        fp16 = skc.ENTRIES[row.entry].outputs[name] == H16
        got = spec.region(row, name, first.out[name]).reshape(want.shape)
        finite = torch.isfinite(want) & ((want.abs() < 65520.0) if fp16 else torch.ones_like(want, dtype=torch.bool))
        assert bool(torch.isfinite(got[finite]).all()), f"{row.name} / {ps}: NaN or Inf in {name}: a guard was read into it"
        if name not in written_inputs and name not in inout:
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
        plain.check_guards(set(inout.values()))
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
    buf = torch.full((13 << 19,), SENT16, dtype=H16, device=dev)     # 12 pointers (the views entry point) 1 MiB apart, and an extent
    want = buf.clone()
    for fn, what, change in skc.REFUSALS + skc.UNSUPPORTED:
        with pytest.raises(RuntimeError):
            ops._call(fn, *skc.call_args(fn, change, buf.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(want)), "a refused call wrote"
