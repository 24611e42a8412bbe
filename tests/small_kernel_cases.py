"""The launch contract of the small kernels (csrc/misc.hip, csrc/sam.hip) as test data.

A ROW is (entry point, shape, form).  `row.data(pass_name)` holds the logical operands on the host, `reference(row, d)` the
fp64 result and the derived bound of every output element, `emulate(row, d)` an fp32 rendering of the kernel's arithmetic
(CPU suite: the bound is not too tight), MUTATIONS wrong answers that have to fall outside.  The references follow the
definitions in include/lgd_hip.h (index arithmetic on the logical operands), not the kernels' code.  REFUSALS is one
changed argument per row of a call the library serves (BASE), each answered with LGD_ERR_ARG before the device is touched.

Shapes are the smallest at which a kernel can still go wrong: one vector, a ragged tail, more than one workgroup, and for
the grid-stride kernels one size past 2048 workgroups x 256 threads, where the loop iterates.

The bounds.  u = 2^-11 (fp16), w = 2^-24 (fp32).  `V` carries a real value v and a bound e on the error of its fp32
rendering through the operations the kernel performs, each rounding once:
    a + b, a - b:  e = e_a + e_b + w |v|         a b:  e = |a| e_b + |b| e_a + e_a e_b + w |v|      (a contracted fma rounds
    a / b:         e = (e_a + |v| e_b) / (|b| - e_b) + w |v|   (correctly rounded)                    once: the bound holds)
    sqrt a:        e = the image of [a - e_a, a + e_a] + w |v|
    rcp a:         v_rcp_f32, 1 ulp: as 1 / a with 2 w |v|
    __expf a:      v_exp_f32 at 2^-22 relative behind the rounded product a log2(e): e = v (expm1(e_a) + 2^-22 + w |a|) + 2^-126
    exact:         fp16 -> fp32, fp16 x fp16, x 0.5, |x|, max(x, 0), copysign
One fp32 -> fp16 rounding at the end: |y^ - y| <= u |y| + 2^-25 + (1 + u) e  (half an ulp, half the smallest subnormal, the
fp32 error carried through) — "R16(e)" below.  A result of magnitude >= 65520 is +-inf and has to compare equal.  The sign of
a zero is not checked.
  add            s = a + b is not always exact in fp32 (exponents 2^-24 .. 2^15 apart): R16(w |s|), not bit equality
  scale          R16(w |alpha x|)
  act RELU       exact: bound 0
  quick_gelu     z = 1.702 x, s = sigmoid(z), y = x s: e = |y| ((1 - s) (2^-22 + 2 w |z|) + 5 w)      (GroupNorm suite, S5); R16
  erf_f          t = rcp(0.3275911 |x| + 1); p = Horner(t); erf^ = 1 - (p t) __expf(-(|x| |x|)), all through V; plus E_P, the
                 polynomial's own error: ERF_POLY_ERR = max |A&S 7.1.26 with the fp32 coefficients, in fp64 - math.erf| on
                 60001 points of [0, 6], measured by erf_poly_error() = 1.455e-7 (printed by the CPU suite; common.h says
                 <= 1.5e-7: true)
  gelu_f         0.5 x (1 + erf^(x c)), c = fp32(2^-1/2) carried as V(2^-1/2, |c - 2^-1/2|); act GELU: R16
  gelu_grad_f    cdf + x pdf, cdf = 0.5 (1 + erf^), pdf = 0.39894228 __expf(-(0.5 x) x) through V
  geglu_fwd      R16 of v gelu(g);  geglu_bwd  R16 of gy gelu(g) and of (gy v) gelu'(g)   (gy v exact)
  upsample2x_bwd ((c00 + c01) + c10) + c11 through V, R16
  softmax_rows   s_i = fl(scale x_i); the kernel's maximum shifts numerator and denominator alike and cancels; t_i = s_i - mx:
                 d_i = w |s_i| + w |t_i|; e_i = __expf(t_i): relative r_i = d_i + 2^-22 + 2 w |t_i|; the sum chain is
                 D = 8 ceil(n / 512) terms per lane + 6 butterfly levels of positive terms: relative D w + sum_i p_i r_i;
                 1 / sum and the product: 3 w.  |p^ - p| <= R16(p (r_i + D w + sum p r + 3 w)); a -inf element is exactly 0
  nchw_to_nhwc8  bit-exact (x - fp16(x) is exact in fp32); select_row bit-exact
  conv_out       products exact; D = 9 ceil(9 Cin / 512) + 6 (per lane: 8 adds and one into the accumulator per vector; the
                 butterfly): e = |out_scale| (D w sum|x w| + w |sum + bias|) + w |y|, fp32 output
  conv_in        acc = bias, then K = 9 Cin sequential x w products (one rounding each, one per add):
                 e = (2 K + 1) w (|bias| + sum |x w|); R16
  cfg_ddim, cfg_multistep, axpy, scale_rows: the header's formulas through V, fp32 outputs.
  cfg_plms       m = eu + gs (ec - eu); comb = w_m m + w_0 ets[0] + w_1 ets[1] + w_2 ets[2] in slot order, zero weights skipped;
                 x' = a src + b comb, all through V with the fp32 coefficients of PNDMScheduler.plms_table; the pushed slot is m
                 within m's bound; the saved sample and every other slot bit for bit
  md_step        per prompt the cfg_ddim formula through V, times the mask, summed in prompt order; x_in rows are that latent
                 (bound carried over; the copies among them bit for bit), bootstrapped rows sqrt(a) bg + sqrt(1 - a) noise through V
                 where mask < 0.5 (the blend with b in {0, 1} is exact)
  md_views       the same per view: sum over prompts first, then into the panorama in ascending view order, through V; count
                 likewise; value / count through V's division where count > 0; uncovered elements exactly 0
  image_u8       bit-exact from the table: fp16(x), fp16(x - fp16(x)), zeros: bound 0;  sam_window_merge  a gather: bound 0
  vae_sample     0.5 lv and the clamp exact; expf at 1 ulp (2 w |v|), the accuracy the HIP documentation's table of math
                 functions publishes for expf — the published figure, not measured here: the GPU suite prints what the row with
                 every finite fp16 log-variance observes, for information; then scale (mean + sd noise) through V
  sam_relpos_qkv q, k, v at valid positions and the one-hot and zero columns: bound 0; at padded positions fp16 of the fp32 bias:
                 u |b| + 2^-25; a rel column: a sequential fp32 fma chain of d terms, e = d w sum |q R|, times fl(1 / scale)
                 carried as V(1 / scale, w / scale), then R16
Nothing above is fitted to kernel output."""
import functools
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_conformance_cases import GUARD, SENT16, SENT32, Carved, P  # noqa: E402,F401

H16, F32, F64, I32 = torch.float16, torch.float32, torch.float64, torch.int32
U, W = 2.0 ** -11, 2.0 ** -24
NAN, INF = float("nan"), float("inf")
GRID_VECS = 2048 * 256                                   # vectors one pass of the capped grid covers (ew_blocks)
ERF_COEF = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)   # a1 .. a5 of csrc/common.h
ERF_P = 0.3275911


def f32(x):
    return float(torch.tensor(x, dtype=F32))


@functools.lru_cache(maxsize=None)
def erf_poly_error():
    """max over [0, 6] of |the A&S polynomial with the kernel's fp32 coefficients, evaluated in fp64 - math.erf|"""
    a = [f32(c) for c in ERF_COEF]
    p0, worst = f32(ERF_P), 0.0
    for i in range(60001):
        x = i * 1e-4
        t = 1.0 / (1.0 + p0 * x)
        poly = ((((a[4] * t + a[3]) * t + a[2]) * t + a[1]) * t + a[0]) * t
        worst = max(worst, abs(1.0 - poly * math.exp(-x * x) - math.erf(x)))
    return worst


# ---------------------------------------------------------------------------------------------
# V: a value and the error bound of its fp32 rendering (docstring)
# ---------------------------------------------------------------------------------------------
def _t(x):
    return x if isinstance(x, torch.Tensor) else torch.tensor(x, dtype=F64)


class V:
    def __init__(self, v, e=None):
        self.v = _t(v).to(F64)
        self.e = torch.zeros_like(self.v) if e is None else _t(e).to(F64)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __add__(self, o):
        o = V.of(o)
        v = self.v + o.v
        return V(v, self.e + o.e + W * v.abs())

    __radd__ = __add__

    def __neg__(self):
        return V(-self.v, self.e)

    def __sub__(self, o):
        return self + (-V.of(o))

    def __rsub__(self, o):
        return V.of(o) + (-self)

    def __mul__(self, o):
        o = V.of(o)
        v = self.v * o.v
        return V(v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e + W * v.abs())

    __rmul__ = __mul__

    def times_exact(self, o):
        """a product that is exact in fp32 (a power of two, or two fp16 factors)"""
        o = V.of(o)
        return V(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = V.of(o)
        v = self.v / o.v
        return V(v, (self.e + v.abs() * o.e) / (o.v.abs() - o.e) + W * v.abs())

    def abs(self):
        return V(self.v.abs(), self.e)

    def sqrt(self):
        v = self.v.sqrt()
        lo, hi = (self.v - self.e).clamp_min(0.0).sqrt(), (self.v + self.e).sqrt()
        return V(v, torch.maximum(v - lo, hi - v) + W * v)

    def rcp(self):
        v = 1.0 / self.v
        return V(v, v.abs() * self.e / (self.v.abs() - self.e) + 2 * W * v.abs())

    def expf(self):
        v = self.v.exp()
        return V(v, v * (torch.expm1(self.e) + 2.0 ** -22 + W * self.v.abs()) + 2.0 ** -126)


def r16(x):
    """bound of the fp16 rendering of V x (docstring: R16)"""
    return U * x.v.abs() + 2.0 ** -25 + (1 + U) * x.e


def erf_v(x):
    ax = x.abs()
    t = (f32(ERF_P) * ax + 1.0).rcp()
    a = [f32(c) for c in ERF_COEF]
    p = a[4] * t + a[3]
    for c in (a[2], a[1], a[0]):
        p = p * t + c
    e = 1.0 - (p * t) * (-(ax * ax)).expf()
    return V(torch.erf(x.v), e.e + erf_poly_error())       # copysign is exact; e.v is the polynomial, erf the truth


_C = 2.0 ** -0.5
RSQRT2 = V(_C, abs(f32(_C) - _C))
_PDF = 1.0 / math.sqrt(2.0 * math.pi)
INV_SQRT_2PI = V(_PDF, abs(f32(0.39894228040143268) - _PDF))


def gelu_v(x):
    return x.times_exact(0.5) * (1.0 + erf_v(x * RSQRT2))


def gelu_grad_v(x):
    cdf = (1.0 + erf_v(x * RSQRT2)).times_exact(0.5)
    pdf = INV_SQRT_2PI * (-(x.times_exact(0.5) * x)).expf()
    return cdf + x * pdf


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound, *, fp16):
    """The largest |got - ref| / bound, `inf` for anything that is not inside (NaN, a wrong infinity, an error where the bound is
    0).  With fp16, a reference of magnitude >= 65520 has to be the infinity of its sign."""
    got, ref, bound = got.to(F64), ref.to(F64), bound.to(F64)
    if fp16:
        over = ref.abs() >= 65520.0
        want = torch.where(over, torch.sign(ref) * INF, ref)
    else:
        over = torch.zeros_like(ref, dtype=torch.bool)
        want = ref
    err = torch.where(over, torch.where(got == want, 0.0, INF), (got - want).abs())
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isnan(ratio) | torch.isnan(got), torch.full_like(ratio, INF), ratio)
    return float(ratio.max()) if ratio.numel() else 0.0


# ---------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------
class Row:
    def __init__(self, entry, shape, form=None, passes=("plain",)):
        self.entry, self.shape, self.form, self.passes = entry, dict(shape), dict(form or {}), tuple(passes)
        fmt = lambda d: ",".join(f"{k}={v}" for k, v in d.items())
        self.name = f"{entry}:{fmt(self.shape)}" + (":" + fmt(self.form) if self.form else "")

    def __getattr__(self, k):
        for d in (self.__dict__.get("shape", {}), self.__dict__.get("form", {})):
            if k in d:
                return d[k]
        raise AttributeError(k)

    def data(self, ps):
        return _data(self.name, ps)

    def seed(self, ps):
        return 7000 + sum(map(ord, self.name)) % 1000 + 17 * sum(map(ord, ps))


@functools.lru_cache(maxsize=2)
def _data(name, ps):
    row = ROWS_BY_NAME[name]
    g = torch.Generator().manual_seed(row.seed(ps))
    return ENTRIES[row.entry].data(row, ps, g)


def _randn(g, *shape, dtype=F32):
    return torch.randn(*shape, generator=g).to(dtype)


_S = 2.0 ** -24                                          # the smallest fp16 subnormal
EDGE_A = [0.0, -0.0, 65504.0, -65504.0, _S, -_S, 6.0, -6.0, 20.0, -20.0, 65504.0, 2.0 ** -14, 1023 * _S, -20.0, 1.0, 0.33325]
EDGE_B = [-0.0, 0.0, 65504.0, -65504.0, _S, _S, -6.0, 6.0, 20.0, 20.0, -65504.0, -_S, _S, 1e-3, 65504.0, _S]


def _edge(values, n):
    return torch.tensor(values, dtype=F64).repeat(-(-n // len(values)))[:n].to(H16)


# ---- elementwise: add, scale, quick_gelu, act ------------------------------------------------
ALPHA = f32(0.3)


class Elementwise:
    """y = f(a[, b]) over n fp16 elements; form inplace: the input(s) the output is ("", "a", "b", "ab": a is b is y)"""
    outputs = {"y": H16}

    def __init__(self, fn):
        self.fn = fn

    def data(self, row, ps, g):
        n = row.n
        a = _edge(EDGE_A, n) if ps == "edge" else _randn(g, n, dtype=H16)
        d = {"a": a}
        if self.fn == "add":
            d["b"] = a.clone() if row.inplace == "ab" else (_edge(EDGE_B, n) if ps == "edge" else _randn(g, n, dtype=H16))
        return d

    def reference(self, row, d):
        a = V(d["a"])
        if self.fn == "add":
            y = a + V(d["b"])
        elif self.fn == "scale":
            y = a * ALPHA
        elif self.fn == "relu":
            v = a.v.clamp_min(0.0)
            return {"y": (v, torch.zeros_like(v))}
        elif self.fn == "gelu":
            y = gelu_v(a)
        else:                                           # quick_gelu
            x = a.v
            z = 1.702 * x
            s = torch.sigmoid(z)
            v = x * s
            y = V(v, v.abs() * ((1.0 - s) * (2.0 ** -22 + 2 * W * z.abs()) + 5 * W))
        return {"y": (y.v, r16(y))}

    def emulate(self, row, d):
        a = d["a"].to(F32)
        if self.fn == "add":
            y = a + d["b"].to(F32)
        elif self.fn == "scale":
            y = a * torch.tensor(ALPHA, dtype=F32)
        elif self.fn == "relu":
            y = a.clamp_min(0.0)
        elif self.fn == "gelu":
            y = _gelu32(a)
        else:
            y = a / (1.0 + torch.exp(torch.tensor(-1.702, dtype=F32) * a))
        return {"y": y.to(H16)}


def _erf32(x):
    ax = x.abs()
    t = 1.0 / (torch.tensor(ERF_P, dtype=F32) * ax + 1.0)
    a = [torch.tensor(c, dtype=F32) for c in ERF_COEF]
    p = a[4] * t + a[3]
    for c in (a[2], a[1], a[0]):
        p = p * t + c
    return torch.copysign(1.0 - p * t * torch.exp(-ax * ax), x)


def _gelu32(x):
    return 0.5 * x * (1.0 + _erf32(x * torch.tensor(0.70710678118654752, dtype=F32)))


def _gelu_grad32(x):
    cdf = 0.5 * (1.0 + _erf32(x * torch.tensor(0.70710678118654752, dtype=F32)))
    return cdf + x * (torch.tensor(0.39894228040143268, dtype=F32) * torch.exp(-0.5 * x * x))


# ---- GEGLU -------------------------------------------------------------------------------------
def geglu_positions(n):
    """column of value j and of gate j inside a packed row of width 2n (lgd_hip.h)"""
    j = torch.arange(n)
    pv = (j // 16) * 32 + j % 16
    return pv, pv + 16


class Geglu:
    def __init__(self, bwd):
        self.bwd = bwd
        self.outputs = {"gh": H16} if bwd else {"y": H16}

    def data(self, row, ps, g):
        rows, n = row.rows, row.n
        v = _randn(g, rows, n, dtype=H16)
        gate = (12.0 * torch.rand(rows, n, generator=g) - 6.0).to(H16)
        gate[0, :2] = torch.tensor([-6.0, 6.0], dtype=H16)
        pv, pg = geglu_positions(n)
        h = torch.empty(rows, 2 * n, dtype=H16)
        h[:, pv], h[:, pg] = v, gate
        d = {"h": h, "v": v, "g": gate}
        if self.bwd:
            d["gy"] = _randn(g, rows, n, dtype=H16)
        return d

    def logical(self, row, d, out):
        """the packed gradient as (value part, gate part) [rows][n]"""
        pv, pg = geglu_positions(row.n)
        return out[:, pv.to(out.device)], out[:, pg.to(out.device)]

    def reference(self, row, d, swap=False, drop_offset=False):
        v, g = d["v"].to(F64), d["g"].to(F64)
        if swap:
            v, g = g, v
        if drop_offset:                                  # both vectors of a 16-block read its first 8 columns
            j = torch.arange(row.n, device=v.device)
            src = j - (j % 16 >= 8) * 8
            v, g = v[:, src], g[:, src]
        if not self.bwd:
            y = V(v) * gelu_v(V(g))
            return {"y": (y.v, r16(y))}
        gy = V(d["gy"])
        gv = gy * gelu_v(V(g))
        gg = gy.times_exact(V(v)) * gelu_grad_v(V(g))
        pv, pg = geglu_positions(row.n)
        ref, bnd = torch.empty_like(d["h"], dtype=F64), torch.empty_like(d["h"], dtype=F64)
        ref[:, pv], ref[:, pg] = gv.v, gg.v
        bnd[:, pv], bnd[:, pg] = r16(gv), r16(gg)
        return {"gh": (ref, bnd)}

    def emulate(self, row, d):
        v, g = d["v"].to(F32), d["g"].to(F32)
        if not self.bwd:
            return {"y": (v * _gelu32(g)).to(H16)}
        gy = d["gy"].to(F32)
        pv, pg = geglu_positions(row.n)
        out = torch.empty_like(d["h"])
        out[:, pv], out[:, pg] = (gy * _gelu32(g)).to(H16), (gy * v * _gelu_grad32(g)).to(H16)
        return {"gh": out}


# ---- upsample gradient ---------------------------------------------------------------------------
class Upsample:
    outputs = {"gx": H16}

    def data(self, row, ps, g):
        return {"gy": _randn(g, row.B, 2 * row.H * 2 * row.W, row.C, dtype=H16)}

    def children(self, row, d, swap_hw=False):
        B, H, W, C = row.B, row.H, row.W, row.C
        if swap_hw:
            H, W = W, H
        t = d["gy"].reshape(B, H, 2, W, 2, C)
        return [t[:, :, dy, :, dx].reshape(B, row.H * row.W, C) for dy in (0, 1) for dx in (0, 1)]

    def reference(self, row, d, swap_hw=False, children=4):
        c = [V(t) for t in self.children(row, d, swap_hw)][:children]
        s = c[0]
        for t in c[1:]:
            s = s + t
        return {"gx": (s.v, r16(s))}

    def emulate(self, row, d):
        c = [t.to(F32) for t in self.children(row, d)]
        return {"gx": (((c[0] + c[1]) + c[2]) + c[3]).to(H16)}


# ---- softmax -----------------------------------------------------------------------------------
def _butterfly(v):
    """wave_sum over the last dimension of 64 lanes, in the kernel's xor order"""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def _lane_vectors(t):
    """[..., n] -> [..., ceil(n / 512), 64, 8]: vector k of lane l is vector l + 64 k of the row (zeros behind the end)"""
    n = t.shape[-1]
    pad = (-n) % 512
    if pad:
        t = torch.cat([t, torch.zeros(*t.shape[:-1], pad, dtype=t.dtype)], -1)
    return t.reshape(*t.shape[:-1], -1, 64, 8)


def _kernel_sum(t):
    """per lane: its vectors in order, the 8 elements of each in order; then the butterfly"""
    lv = _lane_vectors(t)
    acc = torch.zeros(*lv.shape[:-3], 64, dtype=t.dtype)
    for k in range(lv.shape[-3]):
        for e in range(8):
            acc = acc + lv[..., k, :, e]
    return _butterfly(acc)


SOFTMAX_PASSES = ("plain", "spike", "flat", "masked")


class Softmax:
    outputs = {"y": H16}

    def data(self, row, ps, g):
        rows, n, sc = row.rows, row.n, f32(row.scale)
        if ps == "flat":
            x = torch.full((rows, n), 1.25) + torch.arange(rows).view(-1, 1)
        else:
            x = 3.0 * torch.randn(rows, n, generator=g)
        if ps == "spike":                               # every row on a level of its own, one element 40 above the rest
            x = (x.clamp(-4.0, 4.0) / 4.0 + 120.0 * torch.arange(rows).view(-1, 1)) / sc
            col = torch.randint(0, n, (rows,), generator=g)
            x[torch.arange(rows), col] = (120.0 * torch.arange(rows) + 41.0) / sc
        x = x.to(H16)
        if ps == "masked":
            drop = torch.rand(rows, n, generator=g) < 0.3
            drop[:, int(torch.randint(0, n, (1,), generator=g))] = False
            x[drop] = -INF
        return {"x": x}

    def reference(self, row, d, drop_tail=0):
        x = d["x"].to(F64)
        sc, n = f32(row.scale), row.n
        s = x * sc
        t = s - s.max(-1, keepdim=True).values
        live = torch.isfinite(t)
        e = t.exp()
        p = e / (e[:, :n - drop_tail] if drop_tail else e).sum(-1, keepdim=True)
        ta, sa = torch.where(live, t.abs(), 0.0), torch.where(live, s.abs(), 0.0)
        r = torch.where(live, W * sa + W * ta + 2.0 ** -22 + 2 * W * ta, 0.0)
        depth = 8 * -(-n // 512) + 6
        rel = r + depth * W + (p * r).sum(-1, keepdim=True) + 3 * W
        return {"y": (p, U * p + 2.0 ** -25 + (1 + U) * p * rel)}

    def emulate(self, row, d, drop_tail=0, wrong_max=False):
        x = d["x"].to(F32)
        s = x * torch.tensor(row.scale, dtype=F32)
        mx = torch.maximum(s.max(-1, keepdim=True).values, torch.tensor(-1.0e30))
        if wrong_max:
            mx = mx.roll(1, 0)
        e = torch.exp(s - mx)
        tot = _kernel_sum(e[:, :row.n - drop_tail] if drop_tail else e)
        return {"y": (e * (1.0 / tot).unsqueeze(-1)).to(H16)}


# ---- layout converter, row copy ------------------------------------------------------------------
class Nhwc8:
    outputs = {"y": H16}

    def data(self, row, ps, g):
        return {"x": _randn(g, row.B, row.C, row.HW)}

    def reference(self, row, d, remainder_always=False):
        x = d["x"]                                       # fp32
        B, C, HW = x.shape
        hi = x.to(H16)
        y = torch.zeros(B, HW, 8, dtype=F64, device=x.device)
        y[..., :C] = hi.to(F64).transpose(1, 2)
        if 2 * C <= 8 or remainder_always:
            k = min(C, 8 - C)
            y[..., C:C + k] = (x - hi.to(F32)).to(H16).to(F64).transpose(1, 2)[..., :k]
        return {"y": (y.reshape(B * HW, 8), torch.zeros(B * HW, 8, dtype=F64, device=x.device))}

    def emulate(self, row, d):
        return {"y": self.reference(row, d)["y"][0].to(H16)}


class SelectRow:
    outputs = {"out": F32}

    def data(self, row, ps, g):
        return {"table": _randn(g, 4, row.n), "idx": torch.tensor([2], dtype=I32)}

    def reference(self, row, d):
        v = d["table"][int(d["idx"][0])].to(F64)
        return {"out": (v, torch.zeros_like(v))}

    def emulate(self, row, d):
        return {"out": d["table"][int(d["idx"][0])].clone()}


# ---- boundary convolutions ------------------------------------------------------------------------
def _taps(x):
    """[B][L][L][C] -> [B][L][L][9][C]: tap (ky, kx) of pixel (oy, ox) is x[oy + ky - 1][ox + kx - 1], zero outside"""
    B, L, _, C = x.shape
    xp = torch.zeros(B, L + 2, L + 2, C, dtype=x.dtype, device=x.device)
    xp[:, 1:-1, 1:-1] = x
    return torch.stack([xp[:, ky:ky + L, kx:kx + L] for ky in range(3) for kx in range(3)], 3)


class ConvOut:
    """form: bias (given or NULL), out_scale, dgrad (the call of unet.py: conv_in's input gradient)"""
    outputs = {"y": F32}

    def data(self, row, ps, g):
        B, L, Cin, Cout = row.B, row.L, row.Cin, row.Cout
        x = _randn(g, B, L * L, Cin, dtype=H16)
        if row.dgrad:                                    # Cin gradient channels of conv_in's output, Cout latent channels
            from lgd_amd.weightstore import pack_conv_dgrad
            w_in = (_randn(g, Cin, Cout, 3, 3) * (9 * Cout) ** -0.5).to(H16)
            return {"x": x, "w": pack_conv_dgrad(w_in), "w_in": w_in, "bias": None}
        w = (_randn(g, Cout, 9 * Cin) * (9 * Cin) ** -0.5).to(H16)
        return {"x": x, "w": w, "bias": _randn(g, Cout) if row.bias else None}

    def terms(self, row, d, no_left_border=False):
        """[B][L][L][Cout][9][Cin] products in fp64"""
        B, L, Cin, Cout = row.B, row.L, row.Cin, row.Cout
        t = _taps(d["x"].to(F64).reshape(B, L, L, Cin))
        if no_left_border:                               # the tap that lands on column 0 from the right is skipped
            t[:, :, 1, [0, 3, 6]] = 0.0
        return t.unsqueeze(3) * d["w"].to(F64).reshape(1, 1, 1, Cout, 9, Cin)

    def reference(self, row, d, no_left_border=False, scale_first=False):
        B, L, Cin, Cout = row.B, row.L, row.Cin, row.Cout
        sc = f32(row.out_scale)
        terms = self.terms(row, d, no_left_border)
        acc = terms.sum((-1, -2))
        bias = d["bias"].to(F64) if d["bias"] is not None else torch.zeros(Cout, dtype=F64, device=acc.device)
        y = (acc * sc + bias) if scale_first else (acc + bias) * sc
        if row.dgrad and not (no_left_border or scale_first):
            y = self.autograd(row, d).to(acc.device).permute(0, 2, 3, 1) * sc
        depth = 9 * -(-(9 * Cin // 8) // 64) + 6
        e = abs(sc) * (depth * W * terms.abs().sum((-1, -2)) + W * (acc + bias).abs()) + W * y.abs()
        return {"y": (y.permute(0, 3, 1, 2), e.permute(0, 3, 1, 2))}

    def autograd(self, row, d):
        """d/dx of conv2d(x, w_in, padding=1) against the upstream gradient d["x"], by torch.autograd in fp64 on the host"""
        B, L, Cin, Cout = row.B, row.L, row.Cin, row.Cout
        lat = torch.zeros(B, Cout, L, L, dtype=F64, requires_grad=True)
        out = torch.nn.functional.conv2d(lat, d["w_in"].cpu().to(F64), padding=1)
        out.backward(d["x"].cpu().to(F64).reshape(B, L, L, Cin).permute(0, 3, 1, 2))
        return lat.grad

    def emulate(self, row, d):
        B, L, Cin, Cout = row.B, row.L, row.Cin, row.Cout
        t = (_taps(d["x"].to(F32).reshape(B, L, L, Cin)).unsqueeze(3) * d["w"].to(F32).reshape(1, 1, 1, Cout, 9, Cin))
        lv = _lane_vectors(t.reshape(B, L, L, Cout, 9 * Cin))
        acc = torch.zeros(B, L, L, Cout, 64)
        for k in range(lv.shape[-3]):
            s = torch.zeros(B, L, L, Cout, 64)
            for e in range(8):
                s = s + lv[..., k, :, e]
            acc = acc + s
        acc = _butterfly(acc)
        bias = d["bias"] if d["bias"] is not None else torch.zeros(Cout)
        return {"y": ((acc + bias) * torch.tensor(row.out_scale, dtype=F32)).permute(0, 3, 1, 2).contiguous()}


class ConvIn:
    outputs = {"y": H16}

    def data(self, row, ps, g):
        B, L, Cin, Cout = row.B, row.L, row.Cin, row.Cout
        return {"x": _randn(g, B, Cin, L, L), "w": (_randn(g, Cout, 9 * Cin) * (9 * Cin) ** -0.5).to(H16),
                "bias": _randn(g, Cout) if row.bias else None}

    def terms(self, row, d, dtype):
        B, L, Cin, Cout = row.B, row.L, row.Cin, row.Cout
        t = _taps(d["x"].to(dtype).permute(0, 2, 3, 1))
        return t.unsqueeze(3) * d["w"].to(dtype).reshape(1, 1, 1, Cout, 9, Cin)

    def reference(self, row, d):
        K = 9 * row.Cin
        terms = self.terms(row, d, F64)
        bias = d["bias"].to(F64) if d["bias"] is not None else torch.zeros(row.Cout, dtype=F64, device=terms.device)
        y = terms.sum((-1, -2)) + bias
        e = (2 * K + 1) * W * (bias.abs() + terms.abs().sum((-1, -2)))
        return {"y": (y.reshape(-1, row.Cout), (U * y.abs() + 2.0 ** -25 + (1 + U) * e).reshape(-1, row.Cout))}

    def emulate(self, row, d):
        terms = self.terms(row, d, F32).reshape(row.B, row.L, row.L, row.Cout, -1)
        acc = (d["bias"] if d["bias"] is not None else torch.zeros(row.Cout)).expand(row.B, row.L, row.L, row.Cout)
        for k in range(terms.shape[-1]):
            acc = acc + terms[..., k]
        return {"y": acc.reshape(-1, row.Cout).to(H16)}


# ---- the fused sampler steps ----------------------------------------------------------------------
T_STEPS, STEP = 3, 1


class Step:
    """form: vpred, blend ("on": step < frozen_steps; "off": frozen_ref and mask given, step >= frozen_steps; "none": both
    NULL), hist, inplace (x_out is x); multistep: second (C != 0; else x0_prev is NaN and unread)"""

    def __init__(self, multistep):
        self.multistep = multistep
        self.outputs = {"x_out": F32, "hist": F32}
        if multistep:
            self.outputs["x0_prev"] = F32

    def data(self, row, ps, g):
        B, C, L = row.B, row.C, row.L
        n = B * C * L * L
        d = {"eps": _randn(g, 2 * B, C, L, L), "x": _randn(g, B, C, L, L), "dyn": torch.tensor([STEP, 2 if row.blend == "on" else 1, 0, 0], dtype=I32)}
        i = torch.arange(T_STEPS, dtype=F32)
        a_t, a_p = 0.5 + 0.1 * i, 0.6 + 0.1 * i
        if self.multistep:
            al, sg = a_t.sqrt(), (1.0 - a_t).sqrt()
            c0, c1 = (al, -sg) if row.vpred else (1.0 / al, -sg / al)
            d["table"] = torch.stack([c0, c1, 0.3 + 0.1 * i, 0.9 - 0.1 * i, (0.25 + 0.1 * i) if row.second else 0 * i,
                                      7.5 + 0 * i, 0 * i, 0 * i], 1).contiguous()
            d["x0_prev"] = _randn(g, B, C, L, L) if row.second else torch.full((B, C, L, L), NAN)
        else:
            d["table"] = torch.stack([a_t, a_p, 7.5 + 0 * i, (1.0 if row.vpred else 0.0) + 0 * i], 1).contiguous()
        if row.blend != "none":
            d["frozen_ref"] = _randn(g, T_STEPS + 1, B, C, L, L)
            d["mask"] = ((torch.arange(B * L * L, dtype=F64) + 0.5) / (B * L * L)).to(F32).reshape(B, L * L)   # one value per (image, pixel)
        else:
            d["frozen_ref"] = d["mask"] = None
        return d

    def reference(self, row, d, other_mask=False, stale=False):
        B, C, L = row.B, row.C, row.L
        eu, ec, x = V(d["eps"][:B]), V(d["eps"][B:]), V(d["x"])
        c = d["table"][STEP].to(F64)
        out = {}
        if self.multistep:
            m = eu + float(c[5]) * (ec - eu)
            x0 = float(c[0]) * x + float(c[1]) * m
            xn = float(c[2]) * x + float(c[3]) * x0
            if float(c[4]) != 0.0:
                xn = xn + float(c[4]) * V(d["x0_prev"])
            out["x0_prev"] = (d["x0_prev"].to(F64), x0.e) if stale else (x0.v, x0.e)
        else:
            a_t, a_p, gs = V(c[0]), V(c[1]), float(c[2])
            sa, sb, pa, pb = a_t.sqrt(), (1.0 - a_t).sqrt(), a_p.sqrt(), (1.0 - a_p).sqrt()
            m = eu + gs * (ec - eu)
            if row.vpred:
                x0, e = sa * x - sb * m, sa * m + sb * x
            else:
                e = m
                x0 = (x - sb * e) / sa
            xn = pa * x0 + pb * e
        if row.blend == "on":
            mk = d["mask"].to(F64).reshape(B, 1, L, L)
            if other_mask:
                mk = mk.flip(0)
            mk = V(mk)
            xn = V(d["frozen_ref"][STEP + 1]) * mk + xn * (1.0 - mk)
        out["x_out"] = (xn.v, xn.e)
        out["hist"] = (xn.v, xn.e)
        return out

    def emulate(self, row, d):
        B, C, L = row.B, row.C, row.L
        eu, ec, x = d["eps"][:B], d["eps"][B:], d["x"]
        c = d["table"][STEP]
        out = {}
        if self.multistep:
            m = eu + c[5] * (ec - eu)
            x0 = c[0] * x + c[1] * m
            xn = c[2] * x + c[3] * x0
            if float(c[4]) != 0.0:
                xn = xn + c[4] * d["x0_prev"]
            out["x0_prev"] = x0
        else:
            sa, sb, pa, pb = c[0].sqrt(), (1.0 - c[0]).sqrt(), c[1].sqrt(), (1.0 - c[1]).sqrt()
            m = eu + c[2] * (ec - eu)
            if row.vpred:
                x0, e = sa * x - sb * m, sa * m + sb * x
            else:
                e = m
                x0 = (x - sb * e) / sa
            xn = pa * x0 + pb * e
        if row.blend == "on":
            mk = d["mask"].reshape(B, 1, L, L)
            xn = d["frozen_ref"][STEP + 1] * mk + xn * (1.0 - mk)
        out["x_out"] = out["hist"] = xn
        return out


# ---- guidance update, model-input scaling -----------------------------------------------------------
AXPY_ACTIVE = (1.0, 0.0, 0.5)


class Axpy:
    outputs = {"x": F32}

    def data(self, row, ps, g):
        return {"g": _randn(g, 3, 20), "x": _randn(g, 3, 20), "table": _randn(g, 4, 4), "step_idx": torch.tensor([2], dtype=I32),
                "active": torch.tensor(AXPY_ACTIVE, dtype=F32) if row.active else None}

    def reference(self, row, d, ignore_active=False):
        s = V(d["table"][2, row.col])
        a = V(d["active"].to(F64).view(3, 1)) if (row.active and not ignore_active) else V(1.0)
        y = V(d["x"]) - a * s * V(d["g"])
        return {"x": (y.v, y.e)}

    def emulate(self, row, d):
        a = d["active"].view(3, 1) if row.active else torch.tensor(1.0)
        return {"x": d["x"] - a * d["table"][2, row.col] * d["g"]}


class ScaleRows:
    outputs = {"out": F32}

    def data(self, row, ps, g):
        return {"x": _randn(g, row.n), "table": _randn(g, 3, row.row_stride), "dyn": torch.tensor([1, 0, 0, 0], dtype=I32)}

    def reference(self, row, d):
        y = V(d["x"]) * V(d["table"][1, row.col])
        return {"out": (y.v.expand(row.reps, -1), y.e.expand(row.reps, -1))}

    def emulate(self, row, d):
        return {"out": (d["x"] * d["table"][1, row.col]).expand(row.reps, -1).contiguous()}


# ---- one arithmetic for the reference (V) and the emulation (fp32 tensors) --------------------------
def _as(mode):
    return V if mode == "ref" else (lambda t: _t(t).to(F32))


def _sel(b, x, y):
    return V(torch.where(b, x.v, y.v), torch.where(b, x.e, y.e)) if isinstance(x, V) else torch.where(b, x, y)


def _res(x):
    return (x.v, x.e) if isinstance(x, V) else x


def _get(x, idx):
    return V(x.v[idx], x.e[idx]) if isinstance(x, V) else x[idx]


def _put(x, idx, y):
    if isinstance(x, V):
        x.v[idx], x.e[idx] = y.v, y.e
    else:
        x[idx] = y


def _ddim(m, x, vp, sa, sb, pa, pb):
    """cfg_ddim_kernel's step on the combined prediction m (lgd_hip.h)"""
    if vp:
        x0, e = sa * x - sb * m, sa * m + sb * x
    else:
        e = m
        x0 = (x - sb * e) / sa
    return pa * x0 + pb * e


# ---- PLMS ------------------------------------------------------------------------------------------
PLMS_EVALS = 7                                           # six steps make seven evaluations


@functools.lru_cache(maxsize=None)
def plms_table(vpred):
    from lgd_amd.scheduler import PNDMScheduler
    s = PNDMScheduler(prediction_type="v_prediction" if vpred else "epsilon")
    s.set_timesteps(PLMS_EVALS - 1)
    t = s.plms_table(7.5, "cpu")
    assert tuple(t.shape) == (PLMS_EVALS, 16)
    return t


class Plms:
    """form: k the evaluation (row of plms_table), vpred, hist, inplace (x_out is x).  A ring slot whose weight is 0 holds
    NaN, cur_sample holds NaN unless the row reads it.  Output `ets` is the pushed slot, `cur_sample` the saved sample."""
    outputs = {"x_out": F32, "hist": F32, "ets": F32, "cur_sample": F32}

    def data(self, row, ps, g):
        B, C, HW = row.B, row.C, row.HW
        tab = plms_table(row.vpred).clone()
        c = tab[row.k]
        ets = _randn(g, 3, B, C, HW, 1)
        for s in range(3):
            if float(c[1 + s]) == 0.0:
                ets[s] = NAN
        return {"eps": _randn(g, 2 * B, C, HW, 1), "x": _randn(g, B, C, HW, 1), "table": tab, "ets": ets,
                "cur_sample": _randn(g, B, C, HW, 1) if float(c[8]) != 0.0 else torch.full((B, C, HW, 1), NAN),
                "dyn": torch.tensor([row.k, 0, 0, 0], dtype=I32)}

    def _math(self, row, d, mode, push_first=False, ignore_cur=False):
        A, B = _as(mode), row.B
        c = [float(v) for v in d["table"][row.k]]
        eu, ec = A(d["eps"][:B]), A(d["eps"][B:])
        m = eu + c[6] * (ec - eu)
        push = int(c[7])
        comb = c[0] * m
        for s in range(3):
            if c[1 + s] != 0.0:
                comb = comb + c[1 + s] * (m if (push_first and s == push) else A(d["ets"][s]))
        src = A(d["cur_sample"]) if (c[8] != 0.0 and not ignore_cur) else A(d["x"])
        xn = c[4] * src + c[5] * comb
        out = {"x_out": _res(xn), "hist": _res(xn)}
        if push >= 0:
            out["ets"] = _res(m)
        if c[9] != 0.0:
            out["cur_sample"] = (d["x"].to(F64), torch.zeros_like(d["x"], dtype=F64)) if mode == "ref" else d["x"].clone()
        return out

    def reference(self, row, d, **wrong):
        return self._math(row, d, "ref", **wrong)

    def emulate(self, row, d):
        return self._math(row, d, "emu")


# ---- MultiDiffusion, one view ------------------------------------------------------------------------
MD_STEPS, MD_BOOT = 4, 2
MASK_BELOW_HALF = 0.49999997                             # the fp32 value in front of 0.5


def md_table(vpred):
    i = torch.arange(MD_STEPS, dtype=F32)
    return torch.stack([0.5 + 0.1 * i, 0.6 + 0.1 * i, 7.5 + 0 * i, (1.0 if vpred else 0.0) + 0 * i], 1).contiguous()


def _md_coefs(A, tab, step):
    c = tab[step]
    a_t, a_p = A(c[0]), A(c[1])
    return float(c[2]), float(c[3]) != 0.0, a_t.sqrt(), (1.0 - a_t).sqrt(), a_p.sqrt(), (1.0 - a_p).sqrt()


def _pick(pick, n_boot):
    return min(max(int(pick), 0), n_boot - 1)


class MdStep:
    """form: prep, step (dyn[0]; outside [0, MD_STEPS) nothing is written), vpred, hist.  Rows of eps and x_in the kernel has no
    business reading (k >= P, the cond half of x_in) hold NaN; with P = 1 bg, noise and picks are left out (NULL)."""
    outputs = {"x_in": F32, "latent": F32, "hist": F32}

    def data(self, row, ps, g):
        P, Pp, C, HW = row.P, row.Pp, row.C, row.HW
        masks = torch.rand(P, HW, generator=g)
        masks[:, 0], masks[:, 1] = 0.5, MASK_BELOW_HALF
        d = {"table": md_table(row.vpred), "dyn": torch.tensor([row.step, 0, 0, 0], dtype=I32), "masks": masks,
             "bg": None, "noise": None, "picks": None, "eps": None, "latent": None}
        if P > 1:
            d["bg"], d["noise"] = _randn(g, MD_BOOT, C, HW, 1), _randn(g, C, HW, 1)
            picks = torch.randint(0, MD_BOOT, (MD_STEPS, P - 1), generator=g).to(I32)
            picks[0, 0], picks[1, 0] = -3, MD_BOOT + 2       # clamped to 0 and to MD_BOOT - 1
            d["picks"] = picks
        x_in = torch.full((2 * Pp, C, HW, 1), NAN)
        if row.prep:
            d["latent"] = _randn(g, C, HW, 1)
        else:
            x_in[:P] = _randn(g, P, C, HW, 1)
            eps = torch.full((2 * Pp, C, HW, 1), NAN)
            eps[:P], eps[Pp:Pp + P] = _randn(g, P, C, HW, 1), _randn(g, P, C, HW, 1)
            d["eps"] = eps
        d["x_in"] = x_in
        return d

    def _math(self, row, d, mode, gt=False, picks_of_step=False, cond_at_P=False):
        A = _as(mode)
        P, Pp, C, HW, step = row.P, row.Pp, row.C, row.HW, row.step
        if step < 0 or step >= MD_STEPS:
            return {}
        tab, mk = d["table"], d["masks"]
        out = {}
        if row.prep:
            lat, nxt = A(d["latent"].reshape(C, HW)), step
        else:
            gs, vp, sa, sb, pa, pb = _md_coefs(A, tab, step)
            eps, xin = d["eps"].reshape(2 * Pp, C, HW), d["x_in"].reshape(2 * Pp, C, HW)
            lat = None
            for k in range(P):
                eu, ec = A(eps[k]), A(eps[(P if cond_at_P else Pp) + k])
                t = A(mk[k].view(1, HW)) * _ddim(eu + gs * (ec - eu), A(xin[k]), vp, sa, sb, pa, pb)
                lat = t if k == 0 else lat + t
            out["latent"] = out["hist"] = _res(lat)
            nxt = step + 1
        if nxt >= MD_STEPS:
            return out
        boot = nxt < MD_BOOT and P > 1
        rows = []
        for k in range(Pp):
            x = lat
            if boot and 1 <= k < P:
                pk = _pick(d["picks"][step if (picks_of_step and not row.prep) else nxt][k - 1], MD_BOOT)
                a_n = A(tab[nxt][0])
                noisy = a_n.sqrt() * A(d["bg"][pk].reshape(C, HW)) + (1.0 - a_n).sqrt() * A(d["noise"].reshape(C, HW))
                b = ((mk[k] > 0.5) if gt else (mk[k] >= 0.5)).view(1, HW).expand(C, HW)
                x = _sel(b, lat, noisy)                  # acc b + noisy (1 - b) with b in {0, 1}: exact
            rows.append(x)
        if mode == "ref":
            v, e = torch.stack([r.v for r in rows]), torch.stack([r.e for r in rows])
            out["x_in"] = (torch.cat([v, v]), torch.cat([e, e]))
        else:
            out["x_in"] = torch.cat([torch.stack(rows)] * 2)
        return out

    def reference(self, row, d, **wrong):
        return self._math(row, d, "ref", **wrong)

    def emulate(self, row, d):
        return self._math(row, d, "emu")


# ---- MultiDiffusion over views -----------------------------------------------------------------------
def md_views(Hp, Wp):
    """nbh, nbw, V of get_views (lgd_hip.h): 64 x 64 windows at stride 8"""
    nbh, nbw = (Hp - 64) // 8 + 1, (Wp - 64) // 8 + 1
    return nbh, nbw, nbh * nbw


def md_chunks(V_, nvc):
    return [(v0, min(nvc, V_ - v0)) for v0 in range(0, V_, nvc)]


class MdViews:
    """form: prep, step, nvc (views per UNet call), indep, norm, vpred, hist, nullvc (value = count = NULL).  A row is the
    launches of ALL chunks of one step, in order.  The data of a row does not depend on nvc: different chunkings see the same
    panorama.  eps / x_in hold one buffer [2 nvc Pp][C][64 x 64] per chunk; rows nobody may read hold NaN.  With several
    chunks value and count come in as NaN (the chunk with v0 == 0 starts from zero) and go out as the sums behind the last
    non-final chunk (the final chunk stores neither)."""
    outputs = {"x_in": F32, "latent": F32, "hist": F32, "value": F32, "count": F32}

    def key(self, row):
        return row.name.replace(f"nvc={row.nvc},", "")

    def data(self, row, ps, g):
        C, Hp, Wp, P, Pp, nvc = row.C, row.Hp, row.Wp, row.P, row.Pp, row.nvc
        g = torch.Generator().manual_seed(9000 + sum(map(ord, self.key(row))) % 1000)
        _, _, V_ = md_views(Hp, Wp)
        chunks = md_chunks(V_, nvc)
        masks = torch.rand(P, Hp, Wp, generator=g)
        masks[:, 10, 8:12] = 0.0                             # a covered element whose mask sum is exactly 0
        masks[:, 20, 8], masks[:, 20, 9] = 0.5, MASK_BELOW_HALF
        d = {"table": md_table(row.vpred), "dyn": torch.tensor([row.step, 0, 0, 0], dtype=I32), "masks": masks}
        for n in ("bg", "noise", "picks", "eps", "latent", "value", "count", "x_in"):
            d[n] = None
        if row.prep:
            d["latent"] = _randn(g, C, Hp, Wp)
            if P > 1:
                d["bg"], d["noise"] = _randn(g, MD_BOOT, C, 64, 64), _randn(g, C, Hp, Wp)
                picks = torch.randint(0, MD_BOOT, (MD_STEPS, V_, P - 1), generator=g).to(I32)
                picks[0, 0, 0], picks[0, V_ - 1, P - 2] = -3, MD_BOOT + 2
                d["picks"] = picks
            return d
        eps_l, xin_l = torch.full((V_, 2, Pp, C, 64, 64), NAN), torch.full((V_, Pp, C, 64, 64), NAN)
        eps_l[:, :, :P], xin_l[:, :P] = _randn(g, V_, 2, P, C, 64, 64), _randn(g, V_, P, C, 64, 64)
        eps = torch.full((len(chunks), 2 * nvc * Pp, C, 64, 64), NAN)
        x_in = torch.full((len(chunks), 2 * nvc * Pp, C, 64, 64), NAN)
        for ci, (v0, nv) in enumerate(chunks):
            for j in range(nv):
                eps[ci, j * Pp:(j + 1) * Pp] = eps_l[v0 + j, 0]
                eps[ci, (nvc + j) * Pp:(nvc + j + 1) * Pp] = eps_l[v0 + j, 1]
                x_in[ci, j * Pp:(j + 1) * Pp] = xin_l[v0 + j]
        d.update(eps=eps, x_in=x_in, eps_l=eps_l, xin_l=xin_l)
        if len(chunks) > 1:
            d["value"], d["count"] = torch.full((C, Hp, Wp), NAN), torch.full((C, Hp, Wp), NAN)
        return d

    def _math(self, row, d, mode, eu_k=False, div0=False, swap_origin=False, reread=False):
        A = _as(mode)
        C, Hp, Wp, P, Pp, step = row.C, row.Hp, row.Wp, row.P, row.Pp, row.step
        _, nbw, V_ = md_views(Hp, Wp)
        chunks = md_chunks(V_, row.nvc)
        tab, mk = d["table"], d["masks"]
        origin = (lambda v: ((v % nbw) * 8, (v // nbw) * 8)) if swap_origin else (lambda v: ((v // nbw) * 8, (v % nbw) * 8))
        if row.prep:
            boot = step < MD_BOOT and P > 1
            views = []
            for v in range(V_):
                hs, ws = origin(v)
                win = (slice(None), slice(hs, hs + 64), slice(ws, ws + 64))
                lat, rows = A(d["latent"][win]), []
                for k in range(Pp):
                    x = lat
                    if boot and 1 <= k < P:
                        pk = _pick(d["picks"][step][v][k - 1], MD_BOOT)
                        a_n = A(tab[step][0])
                        noisy = a_n.sqrt() * A(d["bg"][pk]) + (1.0 - a_n).sqrt() * A(d["noise"][win])
                        x = _sel((mk[k][win[1:]] >= 0.5).expand(C, 64, 64), lat, noisy)
                    rows.append(x)
                views.append(rows)
            if mode == "ref":
                v_ = torch.stack([torch.stack([r.v for r in rows]) for rows in views])
                e_ = torch.stack([torch.stack([r.e for r in rows]) for rows in views])
                return {"x_in": (torch.stack([v_, v_], 1), torch.stack([e_, e_], 1))}     # [V][half][Pp][C][64][64]
            x = torch.stack([torch.stack(rows) for rows in views])
            return {"x_in": torch.stack([x, x], 1)}
        gs, vp, sa, sb, pa, pb = _md_coefs(A, tab, step)
        zero = torch.zeros(C, Hp, Wp, dtype=F64, device=mk.device)
        val, cnt = A(zero.clone()), A(zero.clone())
        if reread:
            val = A(d["value"].clone())
        snap = None
        for v in range(V_):
            hs, ws = origin(v)
            win = (slice(None), slice(hs, min(hs + 64, Hp)), slice(ws, min(ws + 64, Wp)))
            h_, w_ = win[1].stop - hs, win[2].stop - ws
            eu0 = A(d["eps_l"][v, 0, 0])
            vs = cs = None
            for k in range(P):
                eu, ec = A(d["eps_l"][v, 0, k]), A(d["eps_l"][v, 1, k])
                m = (eu + gs * (ec - eu)) if row.indep else (gs * (ec - eu) + (eu if eu_k else eu0))
                dd = _get(_ddim(m, A(d["xin_l"][v, k]), vp, sa, sb, pa, pb), (slice(None), slice(0, h_), slice(0, w_)))
                mw = A(mk[k][win[1:]].expand(C, h_, w_))
                vs, cs = (mw * dd, mw) if k == 0 else (vs + mw * dd, cs + mw)
            _put(val, win, _get(val, win) + vs)
            _put(cnt, win, _get(cnt, win) + cs)
            if len(chunks) > 1 and v == chunks[-1][0] - 1:   # behind the last non-final chunk
                snap = tuple(V(s.v.clone(), s.e.clone()) if mode == "ref" else s.clone() for s in (val, cnt))
        if row.norm:
            cv = cnt.v if mode == "ref" else cnt
            pos = torch.ones_like(cv, dtype=torch.bool) if div0 else cv > 0
            val = _sel(pos, val / _sel(pos, cnt, A(torch.ones_like(zero))), val)
        out = {"latent": _res(val), "hist": _res(val)}
        if snap is not None:
            out["value"] = _res(snap[0])
            if row.norm:
                out["count"] = _res(snap[1])
        return out

    def reference(self, row, d, **wrong):
        return self._math(row, d, "ref", **wrong)

    def emulate(self, row, d):
        return self._math(row, d, "emu")


# ---- uint8 images, the VAE posterior sample ------------------------------------------------------------
def u8_table():
    u = torch.arange(256, dtype=F32)
    return 2.0 * (u / 255.0) - 1.0                           # the table of lgd_hip.h: fp32, true division


class ImageU8:
    outputs = {"y": H16}

    def data(self, row, ps, g):
        n = row.B * row.HW * 3
        img = torch.randint(0, 256, (n,), generator=g).to(torch.uint8)
        if n >= 256:
            img[:256] = torch.arange(256).to(torch.uint8)   # every byte value
        return {"img": img.reshape(row.B, row.HW, 3)}

    def reference(self, row, d, reverse=False, wrong_word=False):
        img = d["img"].reshape(-1, 12).clone()
        if wrong_word:                                       # byte 4 of a quad (word 1) taken from word 0
            img[:, 4] = img[:, 0]
        x = u8_table().to(img.device)[img.reshape(-1, 3).long()]
        if reverse:
            x = x.flip(-1)
        hi = x.to(H16)
        y = torch.zeros(x.shape[0], 8, dtype=F64, device=x.device)
        y[:, :3], y[:, 3:6] = hi.to(F64), (x - hi.to(F32)).to(H16).to(F64)
        return {"y": (y, torch.zeros_like(y))}

    def emulate(self, row, d):
        return {"y": self.reference(row, d)["y"][0].to(H16)}


def all_finite_f16():
    """every finite fp16 value once: 63 488 of them"""
    return torch.cat([torch.arange(0, 0x7C00), torch.arange(0x8000, 0xFC00) - 0x10000]).to(torch.int16).view(H16)


class VaeSample:
    """form: scale, sweep (the log-variances are every finite fp16 value once; mean 0 and noise 1, so that out is expf itself)"""
    outputs = {"out": F32}

    def data(self, row, ps, g):
        B, z, HW = row.B, row.z, row.HW
        mom = _randn(g, B * HW, 2 * z, dtype=H16)
        mom[:, z:] = (4.0 * torch.randn(B * HW, z, generator=g)).to(H16)
        noise = _randn(g, B, z, HW, 1)
        if row.sweep:
            assert B * HW * z == 63488
            mom[:, :z], noise = 0.0, torch.ones(B, z, HW, 1)
            mom[:, z:] = all_finite_f16()[torch.randperm(63488, generator=g)].reshape(B * HW, z)
        else:
            mom[0, z:z + 4] = torch.tensor([-30.0, -30.02, 20.0, 20.02], dtype=H16)      # both clamp edges
        return {"moments": mom, "noise": noise}

    def _math(self, row, d, mode, no_clamp=False, swap=False):
        B, z, HW = row.B, row.z, row.HW
        mom = d["moments"].reshape(B, HW, 2 * z).transpose(1, 2)       # [B][2z][HW]
        mean, lv = (mom[:, z:], mom[:, :z]) if swap else (mom[:, :z], mom[:, z:])
        h = 0.5 * (lv.to(F64) if no_clamp else lv.to(F64).clamp(-30.0, 20.0))   # exact in fp32
        nz = d["noise"].reshape(B, z, HW)
        if mode == "ref":
            sd = h.exp()
            y = f32(row.scale) * (V(mean) + V(sd, 2 * W * sd) * V(nz))           # expf: 1 ulp
            return {"out": (y.v, y.e)}
        return {"out": torch.tensor(row.scale, dtype=F32) * (mean.to(F32) + torch.exp(h.to(F32)) * nz)}

    def reference(self, row, d, **wrong):
        return self._math(row, d, "ref", **wrong)

    def emulate(self, row, d):
        return self._math(row, d, "emu")


# ---- SAM: window partition with the relative-position columns, window merge ---------------------------------
def sam_geometry(row, dev=None):
    """S, and per row of the window order: the raster token it gathers (clamped), valid, iy, ix"""
    B, Hs, Ws = row.B, row.Hs, row.Ws
    S = row.window or Hs
    nwy, nwx = -(-Hs // S), -(-Ws // S)
    wt = torch.arange(B * nwy * nwx * S * S, device=dev)
    ix, iy, win = wt % S, (wt // S) % S, wt // (S * S)
    wx, wy, b = win % nwx, (win // nwx) % nwy, win // (nwx * nwy)
    y, x = wy * S + iy, wx * S + ix
    valid = (y < Hs) & (x < Ws)
    tok = (b * Hs + y.clamp_max(Hs - 1)) * Ws + x.clamp_max(Ws - 1)
    return S, tok, valid, iy, ix


def sam_scale(row):
    return f32(row.d ** -0.5)


class SamRelpos:
    outputs = {"qa": H16, "ka": H16, "va": H16}

    def data(self, row, ps, g):
        S, C = row.window or row.Hs, row.NH * row.d
        return {"qkv": _randn(g, row.B * row.Hs * row.Ws, 3 * C, dtype=H16), "qkv_bias": _randn(g, 3 * C),
                "rel_h": 0.5 * _randn(g, 2 * S - 1, row.d), "rel_w": 0.5 * _randn(g, 2 * S - 1, row.d)}

    def reference(self, row, d, flip=False, w_with_iy=False, zero_pad=False, emu=False):
        NH, dd, DA = row.NH, row.d, row.DA
        dev = d["qkv"].device
        S, tok, valid, iy, ix = sam_geometry(row, dev)
        R, C = tok.numel(), NH * dd
        dt = F32 if emu else F64
        bias = d["qkv_bias"].to(dt) * (0.0 if zero_pad else 1.0)
        src = torch.where(valid.view(R, 1), d["qkv"][tok].to(dt), bias.view(1, 3 * C).expand(R, 3 * C))   # what the kernel reads
        q = src[:, :C].reshape(R, NH, dd)
        j = torch.arange(S, device=dev)
        sgn = -1 if flip else 1
        ih = (sgn * (iy.view(R, 1) - j) + S - 1).clamp(0, 2 * S - 2)
        iw = (sgn * ((iy if w_with_iy else ix).view(R, 1) - j) + S - 1).clamp(0, 2 * S - 2)
        tabs = torch.cat([d["rel_h"].to(dt)[ih], d["rel_w"].to(dt)[iw]], 1)          # [R][2S][d]
        prod = q.view(R, NH, 1, dd) * tabs.view(R, 1, 2 * S, dd)
        sc = sam_scale(row)
        ref = torch.zeros(3, R, NH, DA, dtype=dt, device=dev)
        bnd = torch.zeros(3, R, NH, DA, dtype=F64, device=dev)
        ref[:, :, :, :dd] = src.reshape(R, 3, NH, dd).transpose(0, 1)
        bnd[:, :, :, :dd] = (~valid).view(1, R, 1, 1) * (U * ref[:, :, :, :dd].abs().to(F64) + 2.0 ** -25)   # fp16(fp32 bias)
        if emu:
            acc = torch.zeros(R, NH, 2 * S, dtype=F32)
            for c in range(dd):
                acc = acc + prod[..., c]
            ref[0, :, :, dd:dd + 2 * S] = acc * (torch.tensor(1.0, dtype=F32) / torch.tensor(sc, dtype=F32))
        else:
            rel = V(prod.sum(-1), dd * W * prod.abs().sum(-1)) * V(1.0 / sc, W / sc)
            ref[0, :, :, dd:dd + 2 * S], bnd[0, :, :, dd:dd + 2 * S] = rel.v, r16(rel)
        ref[1, :, :, dd:dd + S] = (j.view(1, S) == iy.view(R, 1)).to(dt).view(R, 1, S)
        ref[1, :, :, dd + S:dd + 2 * S] = (j.view(1, S) == ix.view(R, 1)).to(dt).view(R, 1, S)
        if emu:
            return {n: ref[i].to(H16) for i, n in enumerate(("qa", "ka", "va"))}
        return {n: (ref[i], bnd[i]) for i, n in enumerate(("qa", "ka", "va"))}

    def emulate(self, row, d):
        return self.reference(row, d, emu=True)


class SamMerge:
    outputs = {"out": H16}

    def data(self, row, ps, g):
        _, _, valid, _, _ = sam_geometry(row)
        oa = _randn(g, valid.numel(), row.NH, row.DA, dtype=H16)
        oa[~valid] = NAN                                     # padded rows and the extra columns: a wrong gather shows
        oa[:, :, row.d:] = NAN
        return {"oa": oa.reshape(valid.numel(), row.NH * row.DA)}

    def reference(self, row, d, swap=False):
        B, Hs, Ws, NH, dd, DA = row.B, row.Hs, row.Ws, row.NH, row.d, row.DA
        S = row.window or Hs
        nwy, nwx = -(-Hs // S), -(-Ws // S)
        if swap:
            nwy, nwx = nwx, nwy
        t = torch.arange(B * Hs * Ws, device=d["oa"].device)
        x, y, b = t % Ws, (t // Ws) % Hs, t // (Ws * Hs)
        wt = ((((b * nwy + y // S) * nwx + x // S) * S + y % S) * S + x % S).clamp_max(d["oa"].shape[0] - 1)
        v = d["oa"].reshape(-1, NH, DA)[wt][:, :, :dd].reshape(-1, NH * dd).to(F64)
        return {"out": (v, torch.zeros_like(v))}

    def emulate(self, row, d):
        return {"out": self.reference(row, d)["out"][0].to(H16)}


ENTRIES = {"cfg_plms": Plms(), "md_step": MdStep(), "md_views": MdViews(), "image_u8": ImageU8(), "vae_sample": VaeSample(),
           "sam_relpos_qkv": SamRelpos(), "sam_window_merge": SamMerge(),
           "add": Elementwise("add"), "scale": Elementwise("scale"), "quick_gelu": Elementwise("quick_gelu"),
           "act_gelu": Elementwise("gelu"), "act_relu": Elementwise("relu"), "geglu_fwd": Geglu(False), "geglu_bwd": Geglu(True),
           "upsample2x_bwd": Upsample(), "softmax_rows": Softmax(), "nchw_to_nhwc8": Nhwc8(), "conv_out": ConvOut(),
           "conv_in": ConvIn(), "cfg_ddim": Step(False), "cfg_multistep": Step(True), "axpy": Axpy(), "scale_rows": ScaleRows(),
           "select_row": SelectRow()}


def reference(row, d, **wrong):
    return ENTRIES[row.entry].reference(row, d, **wrong)


def emulate(row, d, **wrong):
    return ENTRIES[row.entry].emulate(row, d, **wrong)


def on(d, device):
    """the operands of a row on `device`"""
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------
# the rows
# ---------------------------------------------------------------------------------------------
N_ONE, N_RAGGED, N_STRIDE = 8, 8 * 257, 8 * (GRID_VECS + 3)      # one vector; two workgroups, one lane in the second; the loop's tail
_ROW_LIST = []
for _e in ("add", "scale", "quick_gelu", "act_gelu", "act_relu"):
    for _n in (N_ONE, N_RAGGED, N_STRIDE):
        for _ip in (("", "a", "b", "ab") if _e == "add" else ("", "a")):
            _ROW_LIST.append(Row(_e, dict(n=_n), dict(inplace=_ip),
                                 ("plain",) if (_n == N_STRIDE or _ip == "ab") else ("plain", "edge")))
for _e in ("geglu_fwd", "geglu_bwd"):
    _ROW_LIST += [Row(_e, dict(rows=r, n=n)) for r, n in ((1, 16), (5, 48), (4100, 1024))]
_ROW_LIST += [Row("upsample2x_bwd", dict(B=2, H=3, W=5, C=8)), Row("upsample2x_bwd", dict(B=1, H=1, W=1, C=24))]
_ROW_LIST += [Row("softmax_rows", dict(rows=r, n=n), dict(scale=s, inplace=ip), SOFTMAX_PASSES)
              for r in (1, 5) for n in (8, 512, 520, 4096) for s in (1.0, 512 ** -0.5) for ip in ("", "x")]
_ROW_LIST += [Row("nchw_to_nhwc8", dict(B=B, C=C, HW=HW)) for C in (1, 3, 4, 5, 8) for B, HW in ((3, 1), (2, 50))]
_ROW_LIST += [Row("conv_out", dict(B=B, L=L, Cin=ci, Cout=co), dict(bias=b, out_scale=s, dgrad=0))
              for co in (4, 8) for ci in (8, 24, 320) for B, L in ((2, 1), (2, 3), (1, 5)) for b in (1, 0) for s in (1.0, 0.5)]
_ROW_LIST += [Row("conv_out", dict(B=B, L=L, Cin=24, Cout=4), dict(bias=0, out_scale=0.5, dgrad=1)) for B, L in ((2, 3), (1, 5))]
_ROW_LIST += [Row("conv_in", dict(B=2, Cin=4, L=5, Cout=70), dict(bias=1)), Row("conv_in", dict(B=1, Cin=8, L=3, Cout=64), dict(bias=0))]
for _e in ("cfg_ddim", "cfg_multistep"):
    for _sec in ((0, 1) if _e == "cfg_multistep" else (0,)):
        _extra = dict(second=_sec) if _e == "cfg_multistep" else {}
        _ROW_LIST += [Row(_e, dict(B=2, C=4, L=4), dict(vpred=v, blend=bl, hist=h, inplace=ip, **_extra))
                      for v in (0, 1) for bl in ("on", "off", "none") for h in (0, 1) for ip in (0, 1)]
        # 2 x 4 x 257 x 257 = 528 392 elements > 2048 x 256: the grid-stride loop iterates
        _ROW_LIST += [Row(_e, dict(B=2, C=4, L=257), dict(vpred=v, blend="on", hist=1, inplace=1, **_extra)) for v in (0, 1)]
_ROW_LIST += [Row("axpy", {}, dict(active=a, col=c)) for a in (0, 1) for c in range(4)]
_ROW_LIST += [Row("scale_rows", dict(n=7, row_stride=5), dict(reps=r, col=3)) for r in (1, 2)]
_ROW_LIST += [Row("select_row", dict(n=n)) for n in (1, 300)]
# PLMS: one evaluation kind per k (0 saves and pushes, 1 restarts from the saved sample, 2 and 3 the second and third order, 4 and
# 5 the fourth order on two ring slots); 2 x 4 x 512 x 513 / 4 = 525 312 vectors > 2048 x 256: the grid-stride loop iterates
N_PLMS_STRIDE = 512 * 513
_ROW_LIST += [Row("cfg_plms", dict(B=1, C=1, HW=4), dict(k=k, vpred=0, hist=1, inplace=0)) for k in range(6)]
_ROW_LIST += [Row("cfg_plms", dict(B=2, C=4, HW=16), dict(k=k, vpred=v, hist=h, inplace=ip))
              for k in range(6) for v in (0, 1) for h in (0, 1) for ip in (0, 1)]
_ROW_LIST += [Row("cfg_plms", dict(B=2, C=4, HW=N_PLMS_STRIDE), dict(k=4, vpred=0, hist=0, inplace=1))]
# MultiDiffusion step: the two prep forms (a bootstrapped and an unbootstrapped step), then step 0 (the next one bootstrapped),
# 1 (the first unbootstrapped input), 3 (the last: x_in keeps every bit), -1 and 4 (nothing is written); HW = 260 is 65 vectors
_MD_FORMS = [dict(prep=1, step=s, vpred=0, hist=0) for s in (0, 2)] + \
            [dict(prep=0, step=s, vpred=v, hist=h) for s in (0, 1, 3, -1, 4) for v in (0, 1) for h in (0, 1)]
_ROW_LIST += [Row("md_step", dict(P=P_, Pp=Pp, C=C, HW=HW), f)
              for P_, Pp, C, HW in ((1, 1, 1, 4), (2, 2, 4, 16), (3, 4, 4, 16), (2, 2, 1, 260)) for f in _MD_FORMS]


def _vrow(C, Hp, Wp, P_, Pp, **form):
    return Row("md_views", dict(C=C, Hp=Hp, Wp=Wp, P=P_, Pp=Pp), form)


# views: on the 72 x 72 panorama (V = 4) every chunking (one chunk; two of 2; 3 and a short last one) with every
# (normalization, indep_uncond); the prompts and the prediction hang on that pair, so that the chunkings of one pair share data
_VIEW_PAIRS = {(0, 0): (2, 2, 0), (0, 1): (3, 4, 1), (1, 0): (1, 1, 1), (1, 1): (3, 4, 0)}
for _nvc in (4, 2, 3):
    for (_norm, _indep), (_P, _Pp, _vp) in _VIEW_PAIRS.items():
        _ROW_LIST.append(_vrow(2, 72, 72, _P, _Pp, prep=0, step=1, nvc=_nvc, indep=_indep, norm=_norm, vpred=_vp, hist=1, nullvc=0))
    _ROW_LIST += [_vrow(2, 72, 72, 3, 4, prep=1, step=s, nvc=_nvc, indep=1, norm=0, vpred=0, hist=0, nullvc=0) for s in (0, 2)]
_ROW_LIST += [
    _vrow(1, 72, 72, 1, 1, prep=1, step=0, nvc=4, indep=1, norm=0, vpred=0, hist=0, nullvc=0),
    _vrow(1, 72, 72, 2, 2, prep=1, step=0, nvc=2, indep=1, norm=0, vpred=0, hist=0, nullvc=0),
    _vrow(1, 64, 64, 2, 2, prep=0, step=1, nvc=1, indep=1, norm=1, vpred=0, hist=1, nullvc=1),       # V = 1
    _vrow(1, 64, 64, 2, 2, prep=1, step=0, nvc=1, indep=1, norm=0, vpred=0, hist=0, nullvc=0),
    _vrow(2, 64, 72, 2, 2, prep=0, step=0, nvc=2, indep=0, norm=0, vpred=1, hist=1, nullvc=0),       # V = 2 in one chunk
    _vrow(2, 64, 72, 2, 2, prep=0, step=0, nvc=1, indep=0, norm=0, vpred=1, hist=1, nullvc=0),       # and in two
    _vrow(2, 64, 72, 2, 2, prep=1, step=0, nvc=1, indep=1, norm=0, vpred=0, hist=0, nullvc=0),
    _vrow(1, 68, 64, 3, 4, prep=0, step=3, nvc=1, indep=1, norm=1, vpred=0, hist=0, nullvc=0),       # rows 64 .. 67 uncovered
    _vrow(1, 68, 64, 2, 2, prep=1, step=0, nvc=1, indep=1, norm=0, vpred=0, hist=0, nullvc=0),
    _vrow(1, 64, 68, 2, 2, prep=0, step=1, nvc=1, indep=0, norm=1, vpred=1, hist=1, nullvc=1),       # columns 64 .. 67 uncovered
    _vrow(1, 64, 68, 2, 2, prep=1, step=1, nvc=1, indep=1, norm=0, vpred=0, hist=0, nullvc=0)]
_ROW_LIST += [Row("image_u8", dict(B=1, HW=4)), Row("image_u8", dict(B=2, HW=2 * 257)), Row("image_u8", dict(B=1, HW=4 * (GRID_VECS + 3)))]
_ROW_LIST += [Row("vae_sample", dict(B=1, z=4, HW=4), dict(scale=0.18215, sweep=0)),
              Row("vae_sample", dict(B=2, z=8, HW=20), dict(scale=0.18215, sweep=0)), Row("vae_sample", dict(B=2, z=8, HW=20), dict(scale=1.0, sweep=0)),
              Row("vae_sample", dict(B=1, z=4, HW=15872), dict(scale=1.0, sweep=1)),
              Row("vae_sample", dict(B=1, z=4, HW=4 * (GRID_VECS + 3)), dict(scale=0.18215, sweep=0))]
# SAM: the smallest global grid; a 5 x 7 grid in 2 x 3 windows of 3, padded both ways, with tail columns; a window larger than
# the grid; exact division; NH d = 320, NH 2S = 280 and NH DA = 640 > 256: each of the three thread loops iterates
_SAM_SHAPES = [dict(B=1, Hs=2, Ws=2, window=0, NH=1, d=8, DA=16), dict(B=2, Hs=5, Ws=7, window=3, NH=2, d=8, DA=16),
               dict(B=1, Hs=3, Ws=2, window=4, NH=1, d=8, DA=16), dict(B=1, Hs=4, Ws=4, window=2, NH=2, d=16, DA=24),
               dict(B=1, Hs=14, Ws=14, window=0, NH=10, d=32, DA=64)]
_ROW_LIST += [Row(e, s) for e in ("sam_relpos_qkv", "sam_window_merge") for s in _SAM_SHAPES]
ROWS_BY_NAME = {r.name: r for r in _ROW_LIST}
assert len(ROWS_BY_NAME) == len(_ROW_LIST)


def rows_of(entry):
    return [r for r in _ROW_LIST if r.entry == entry]


def grid_stride_rows():
    return [r for r in _ROW_LIST if r.shape.get("n") == N_STRIDE or r.shape.get("rows") == 4100 or r.shape.get("L") == 257
            or r.shape.get("HW") in (N_PLMS_STRIDE, 4 * (GRID_VECS + 3))]


# ---------------------------------------------------------------------------------------------
# wrong answers (CPU suite): name -> (row name, output, function(row, d) -> wrong output)
# ---------------------------------------------------------------------------------------------
def _ref_of(**wrong):
    return lambda row, d, out: reference(row, d, **wrong)[out][0]


def _emu_of(**wrong):
    return lambda row, d, out: emulate(row, d, **wrong)[out]


def _row(entry, **kv):
    hits = [r for r in rows_of(entry) if all(getattr(r, k) == v for k, v in kv.items())]
    assert hits, (entry, kv)
    return hits[0].name


MUTATIONS = {
    "geglu_fwd: value and gate halves swapped": (_row("geglu_fwd", rows=5), "y", "plain", _ref_of(swap=True)),
    "geglu_bwd: value and gate halves swapped": (_row("geglu_bwd", rows=5), "gh", "plain", _ref_of(swap=True)),
    "geglu_fwd: the j % 16 offset dropped": (_row("geglu_fwd", rows=1), "y", "plain", _ref_of(drop_offset=True)),
    "geglu_bwd: the j % 16 offset dropped": (_row("geglu_bwd", rows=1), "gh", "plain", _ref_of(drop_offset=True)),
    "upsample: H and W swapped": (_row("upsample2x_bwd", H=3), "gx", "plain", _ref_of(swap_hw=True)),
    "upsample: one child missing": (_row("upsample2x_bwd", H=1), "gx", "plain", _ref_of(children=3)),
    "softmax: normalised over n - 8 elements": (_row("softmax_rows", rows=5, n=520, scale=1.0, inplace=""), "y", "plain", _ref_of(drop_tail=8)),
    "softmax: the neighbouring row's maximum": (_row("softmax_rows", rows=5, n=520, scale=1.0, inplace=""), "y", "spike", _emu_of(wrong_max=True)),
    "nchw_to_nhwc8: a remainder written at C = 5": (_row("nchw_to_nhwc8", C=5, HW=50), "y", "plain", _ref_of(remainder_always=True)),
    "conv_out: the left border tap missing": (_row("conv_out", L=3, Cin=8, Cout=4, bias=1, out_scale=1.0), "y", "plain", _ref_of(no_left_border=True)),
    "conv_out: out_scale before the bias": (_row("conv_out", L=3, Cin=8, Cout=4, bias=1, out_scale=0.5), "y", "plain", _ref_of(scale_first=True)),
    "cfg_ddim: the mask of the other image": (_row("cfg_ddim", L=4, vpred=0, blend="on", hist=1, inplace=0), "x_out", "plain", _ref_of(other_mask=True)),
    "cfg_multistep: a stale x0_prev": (_row("cfg_multistep", L=4, vpred=0, blend="on", hist=1, inplace=0, second=1), "x0_prev", "plain", _ref_of(stale=True)),
    "axpy: active ignored": (_row("axpy", active=1, col=0), "x", "plain", _ref_of(ignore_active=True)),
    "plms: the ring slot pushed before it is read": (_row("cfg_plms", HW=16, k=4, vpred=0, hist=1, inplace=0), "x_out", "plain", _ref_of(push_first=True)),
    "plms: from_cur ignored": (_row("cfg_plms", HW=16, k=1, vpred=0, hist=1, inplace=0), "x_out", "plain", _ref_of(ignore_cur=True)),
    "md_step: > for >= at a mask of 0.5": (_row("md_step", P=2, HW=16, prep=1, step=0), "x_in", "plain", _ref_of(gt=True)),
    "md_step: the picks row of step i": (_row("md_step", P=2, HW=16, prep=0, step=0, vpred=0, hist=1), "x_in", "plain", _ref_of(picks_of_step=True)),
    "md_step: the cond half at row offset P": (_row("md_step", P=3, Pp=4, prep=0, step=1, vpred=0, hist=1), "latent", "plain", _ref_of(cond_at_P=True)),
    "views: the shared uncond taken from eu_k": (_row("md_views", Hp=64, Wp=72, prep=0, nvc=2), "latent", "plain", _ref_of(eu_k=True)),
    "views: division where count == 0": (_row("md_views", Hp=72, prep=0, nvc=4, norm=1, indep=1), "latent", "plain", _ref_of(div0=True)),
    "views: the view origin swapped": (_row("md_views", Hp=64, Wp=72, prep=0, nvc=2), "latent", "plain", _ref_of(swap_origin=True)),
    "views: value re-read in the chunk with v0 == 0": (_row("md_views", Hp=72, prep=0, nvc=2, norm=0, indep=1), "latent", "plain", _ref_of(reread=True)),
    "relpos: the sign of the rel index flipped": (_row("sam_relpos_qkv", Hs=5), "qa", "plain", _ref_of(flip=True)),
    "relpos: rel_w indexed with iy": (_row("sam_relpos_qkv", Hs=5), "qa", "plain", _ref_of(w_with_iy=True)),
    "relpos: zero instead of the bias at padded positions": (_row("sam_relpos_qkv", Hs=5), "va", "plain", _ref_of(zero_pad=True)),
    "window_merge: nwx and nwy swapped": (_row("sam_window_merge", Hs=5), "out", "plain", _ref_of(swap=True)),
    "vae: the clamp missing": (_row("vae_sample", sweep=1), "out", "plain", _ref_of(no_clamp=True)),
    "vae: mean and log-variance halves swapped": (_row("vae_sample", HW=20, scale=1.0), "out", "plain", _ref_of(swap=True)),
    "image_u8: channel order reversed": (_row("image_u8", HW=514), "y", "plain", _ref_of(reverse=True)),
    "image_u8: the straddling byte from the wrong word": (_row("image_u8", HW=514), "y", "plain", _ref_of(wrong_word=True)),
}


# ---------------------------------------------------------------------------------------------
# host refusals.  ARGS names every argument; "p:" marks a pointer.  BASE is a call the library serves; the pointers of a
# call sit 1 MiB apart, a pointer value being None (NULL), a byte offset inside the operand's own MiB, or (operand,
# byte offset) for an address inside another operand.  ALIGN: the alignment each pointer needs; OPTIONAL: may be NULL.
# ---------------------------------------------------------------------------------------------
ARGS = {
    "lgd_add_f16": "p:a p:b p:y n stream",
    "lgd_scale_f16": "p:x p:y alpha n stream",
    "lgd_quick_gelu_f16": "p:x p:y n stream",
    "lgd_act_f16": "p:x p:y n mode stream",
    "lgd_geglu_fwd_f16": "p:h p:y rows n stream",
    "lgd_geglu_bwd_f16": "p:h p:gy p:gh rows n stream",
    "lgd_upsample2x_bwd_f16": "p:gy p:gx B H W C stream",
    "lgd_softmax_rows_f16": "p:x p:y rows n scale stream",
    "lgd_nchw_to_nhwc8_f16": "p:x p:y B C HW stream",
    "lgd_conv_out_f16": "p:x p:w p:bias p:y B Cin L Cout out_scale stream",
    "lgd_conv_in_f16": "p:x p:w p:bias p:y B Cin L Cout stream",
    "lgd_cfg_ddim_step_f32": "p:eps p:x p:x_out p:coef_table p:dyn p:frozen_ref p:mask p:hist B C HW stream",
    "lgd_cfg_multistep_step_f32": "p:eps p:x p:x_out p:x0_prev p:coef_table p:dyn p:frozen_ref p:mask p:hist B C HW stream",
    "lgd_axpy_f32": "p:g p:x p:coef_table p:step_idx col p:active per_sample n stream",
    "lgd_select_row_f32": "p:table p:idx p:out n stream",
    "lgd_scale_rows_f32": "p:x p:out p:table p:dyn row_stride col n reps stream",
    "lgd_cfg_plms_step_f32": "p:eps p:x p:x_out p:ets p:cur_sample p:coef_table p:dyn p:hist B C HW stream",
    "lgd_multidiffusion_step_f32": "p:eps p:x_in p:latent p:masks p:bg p:noise p:picks p:coef_table p:dyn p:hist P Pp C HW n_steps n_boot prep stream",
    "lgd_multidiffusion_views_f32": "p:eps p:x_in p:latent p:value p:count p:masks p:bg p:noise p:picks p:coef_table p:dyn p:hist "
                                    "P Pp C Hp Wp V v0 nv nvc n_steps n_boot indep_uncond normalization prep stream",
    "lgd_image_u8_to_nhwc8_f16": "p:img p:table p:y B HW stream",
    "lgd_vae_sample_f32": "p:moments p:noise p:out B z HW scale stream",
    "lgd_sam_relpos_qkv_f16": "p:qkv p:qkv_bias p:rel_h p:rel_w B Hs Ws window NH d DA scale p:qa p:ka p:va stream",
    "lgd_sam_window_merge_f16": "p:oa p:out B Hs Ws window NH d DA stream",
}
BASE = {
    "lgd_add_f16": dict(n=64), "lgd_scale_f16": dict(alpha=0.5, n=64), "lgd_quick_gelu_f16": dict(n=64),
    "lgd_act_f16": dict(n=64, mode=1), "lgd_geglu_fwd_f16": dict(rows=4, n=32), "lgd_geglu_bwd_f16": dict(rows=4, n=32),
    "lgd_upsample2x_bwd_f16": dict(B=2, H=3, W=5, C=16), "lgd_softmax_rows_f16": dict(rows=5, n=64, scale=1.0),
    "lgd_nchw_to_nhwc8_f16": dict(B=2, C=4, HW=50), "lgd_conv_out_f16": dict(B=2, Cin=16, L=3, Cout=4, out_scale=1.0),
    "lgd_conv_in_f16": dict(B=2, Cin=4, L=5, Cout=64), "lgd_cfg_ddim_step_f32": dict(B=2, C=4, HW=16),
    "lgd_cfg_multistep_step_f32": dict(B=2, C=4, HW=16), "lgd_axpy_f32": dict(col=1, per_sample=20, n=60),
    "lgd_select_row_f32": dict(n=300), "lgd_scale_rows_f32": dict(row_stride=5, col=3, n=7, reps=2),
    "lgd_cfg_plms_step_f32": dict(B=2, C=4, HW=16),
    "lgd_multidiffusion_step_f32": dict(P=2, Pp=2, C=4, HW=16, n_steps=4, n_boot=2, prep=0),
    # the first of two chunks of an accumulate call with normalization: eps, value and count are all needed
    "lgd_multidiffusion_views_f32": dict(P=2, Pp=2, C=1, Hp=72, Wp=72, V=4, v0=0, nv=2, nvc=2, n_steps=4, n_boot=2, indep_uncond=1,
                                         normalization=1, prep=0),
    "lgd_image_u8_to_nhwc8_f16": dict(B=2, HW=50), "lgd_vae_sample_f32": dict(B=2, z=4, HW=20, scale=0.18215),
    "lgd_sam_relpos_qkv_f16": dict(B=2, Hs=5, Ws=7, window=3, NH=2, d=8, DA=16, scale=8 ** -0.5),
    "lgd_sam_window_merge_f16": dict(B=2, Hs=5, Ws=7, window=3, NH=2, d=8, DA=16),
}
_V16 = dict.fromkeys("a b y x h gy gh gx".split(), 16)
ALIGN = {fn: {n[2:]: _V16.get(n[2:], 4) for n in a.split() if n.startswith("p:")} for fn, a in ARGS.items()}
ALIGN["lgd_nchw_to_nhwc8_f16"]["x"] = 4                  # fp32 scalars in, vectors out
ALIGN["lgd_conv_out_f16"].update(x=16, w=16, y=4)
ALIGN["lgd_conv_in_f16"].update(x=4, w=2, y=2)
ALIGN["lgd_axpy_f32"].update(x=4)
ALIGN["lgd_scale_rows_f32"].update(x=4)
ALIGN["lgd_cfg_ddim_step_f32"].update(x=4)
ALIGN["lgd_cfg_multistep_step_f32"].update(x=4)
_V16F = dict.fromkeys("eps x x_in x_out ets cur_sample latent value count masks bg noise hist".split(), 16)   # fp32 in vectors of 4
ALIGN["lgd_cfg_plms_step_f32"].update({k: v for k, v in _V16F.items() if k in ALIGN["lgd_cfg_plms_step_f32"]})
ALIGN["lgd_multidiffusion_step_f32"].update({k: v for k, v in _V16F.items() if k in ALIGN["lgd_multidiffusion_step_f32"]})
ALIGN["lgd_multidiffusion_views_f32"].update({k: v for k, v in _V16F.items() if k in ALIGN["lgd_multidiffusion_views_f32"]})
ALIGN["lgd_vae_sample_f32"].update(moments=8, noise=16, out=16)
ALIGN["lgd_sam_relpos_qkv_f16"].update(qkv=2, qa=2, ka=2, va=2)      # scalar accesses
ALIGN["lgd_sam_window_merge_f16"].update(oa=16, out=16)
OPTIONAL = {"bias", "frozen_ref", "mask", "hist", "active"}
# the entry points whose operand names mean something else elsewhere (noise, eps) say themselves what may be NULL in their BASE
OPTIONAL_OF = {"lgd_cfg_plms_step_f32": {"hist"}, "lgd_multidiffusion_step_f32": {"hist"},
               "lgd_multidiffusion_views_f32": {"bg", "noise", "picks", "hist"}, "lgd_image_u8_to_nhwc8_f16": set(),
               "lgd_vae_sample_f32": set(), "lgd_sam_relpos_qkv_f16": set(), "lgd_sam_window_merge_f16": set()}


def optional(fn):
    return OPTIONAL_OF.get(fn, OPTIONAL)


COUNTS = {fn: [n for n in a.split() if n in ("n", "rows", "B", "H", "W", "L", "HW", "C", "Cin", "reps")] for fn, a in ARGS.items()}
COUNTS["lgd_conv_in_f16"].append("Cout")                 # conv_out answers LGD_ERR_UNSUPPORTED for a Cout outside {4, 8}
COUNTS["lgd_multidiffusion_step_f32"] += ["P", "n_steps"]
COUNTS["lgd_multidiffusion_views_f32"] += ["P", "Hp", "Wp", "nv", "n_steps"]
COUNTS["lgd_vae_sample_f32"].append("z")
COUNTS["lgd_sam_relpos_qkv_f16"] += ["Hs", "Ws", "NH", "d"]
COUNTS["lgd_sam_window_merge_f16"] += ["Hs", "Ws", "NH", "d"]
# what each entry point has beyond NULL / alignment / counts: (class, label, change)
_STEP_RULES = [("entry", "frozen_ref without mask", dict(mask=None)), ("entry", "mask without frozen_ref", dict(frozen_ref=None)),
               ("alias", "x_out partly over x", dict(x_out=("x", 64))), ("alias", "x_out inside eps", dict(x_out=("eps", 512))),
               ("alias", "x_out over the mask", dict(x_out=("mask", 0)))]
RULES = {
    "lgd_add_f16": [("divisibility", "n % 8", dict(n=68)), ("entry", "n = -8", dict(n=-8)), ("entry", "a off by 2 bytes", dict(a=2)), ("alias", "y partly over a", dict(y=("a", 16))),
                    ("alias", "y partly over b", dict(y=("b", 112)))],
    "lgd_scale_f16": [("divisibility", "n % 8", dict(n=68)), ("alias", "y partly over x", dict(y=("x", 16)))],
    "lgd_quick_gelu_f16": [("divisibility", "n % 8", dict(n=68)), ("alias", "y partly over x", dict(y=("x", 16)))],
    "lgd_act_f16": [("divisibility", "n % 8", dict(n=68)), ("alias", "y partly over x", dict(y=("x", 112))), ("entry", "mode 0", dict(mode=0)),
                    ("entry", "mode 3", dict(mode=3))],
    "lgd_geglu_fwd_f16": [("divisibility", "n % 16", dict(n=40)), ("alias", "y is h", dict(y=("h", 0))), ("alias", "y in the tail of h", dict(y=("h", 496)))],
    "lgd_geglu_bwd_f16": [("divisibility", "n % 16", dict(n=40)), ("alias", "gh is h", dict(gh=("h", 0))), ("alias", "gh over gy", dict(gh=("gy", 240)))],
    "lgd_upsample2x_bwd_f16": [("divisibility", "C % 8", dict(C=12)), ("alias", "gx is gy", dict(gx=("gy", 0))),
                               ("alias", "gx in the tail of gy", dict(gx=("gy", 3824)))],
    "lgd_softmax_rows_f16": [("divisibility", "n % 8", dict(n=68)), ("divisibility", "n % 8 with rows n % 8 == 0", dict(rows=4, n=68)),
                             ("divisibility", "n = 12, two rows", dict(rows=2, n=12)), ("alias", "y partly over x", dict(y=("x", 128)))],
    "lgd_nchw_to_nhwc8_f16": [("divisibility", "C > 8", dict(C=9)), ("alias", "y is x", dict(y=("x", 0))), ("alias", "y in the tail of x", dict(y=("x", 1584)))],
    "lgd_conv_out_f16": [("divisibility", "Cin % 8", dict(Cin=20)), ("entry", "x off by 2 bytes", dict(x=2)), ("alias", "y is x", dict(y=("x", 0))), ("alias", "y over w", dict(y=("w", 1136))),
                         ("alias", "y over bias", dict(y=("bias", 12)))],
    "lgd_conv_in_f16": [("divisibility", "Cin > 8", dict(Cin=9)), ("alias", "y is x", dict(y=("x", 0))), ("alias", "y over w", dict(y=("w", 4606))),
                        ("alias", "y over bias", dict(y=("bias", 254)))],
    "lgd_cfg_ddim_step_f32": _STEP_RULES,
    "lgd_cfg_multistep_step_f32": _STEP_RULES + [("alias", "x0_prev is x", dict(x0_prev=("x", 0))), ("alias", "x0_prev is x_out", dict(x0_prev=("x_out", 0))),
                                                 ("alias", "x0_prev inside eps", dict(x0_prev=("eps", 1020)))],
    "lgd_axpy_f32": [("divisibility", "n % per_sample with active", dict(n=70)), ("alias", "x over g", dict(x=("g", 236))),
                     ("entry", "col 4", dict(col=4)), ("entry", "col -1", dict(col=-1)), ("entry", "per_sample -1", dict(per_sample=-1))],
    "lgd_select_row_f32": [],
    # B C HW = 128 floats: x, x_out, cur_sample 512 bytes, eps 1024, ets 1536
    "lgd_cfg_plms_step_f32": [("divisibility", "B C HW % 4", dict(B=1, C=1, HW=6)), ("alias", "x_out 64 bytes into x", dict(x_out=("x", 64))),
                              ("alias", "x_out inside eps", dict(x_out=("eps", 512))), ("alias", "x_out over ets", dict(x_out=("ets", 1520))),
                              ("alias", "x_out is cur_sample", dict(x_out=("cur_sample", 0))), ("alias", "ets inside eps", dict(ets=("eps", 16))),
                              ("alias", "ets over x", dict(ets=("x", 496))), ("alias", "ets over x_out", dict(ets=("x_out", 0))),
                              ("alias", "ets over cur_sample", dict(ets=("cur_sample", 256))), ("alias", "cur_sample is x", dict(cur_sample=("x", 0))),
                              ("alias", "cur_sample in the tail of eps", dict(cur_sample=("eps", 1008)))],
    # a plane C HW is 256 bytes: x_in and eps 1024, latent and noise 256, masks 128, bg 512
    "lgd_multidiffusion_step_f32": [("entry", "Pp < P", dict(Pp=1)), ("entry", "prep = 2", dict(prep=2)), ("entry", "prep = -1", dict(prep=-1)),
                                    ("divisibility", "HW % 4", dict(HW=18)), ("entry", "n_boot = -1", dict(n_boot=-1)),
                                    ("alias", "latent inside x_in", dict(latent=("x_in", 768))), ("alias", "x_in in the tail of eps", dict(x_in=("eps", 1008))),
                                    ("alias", "latent is eps", dict(latent=("eps", 0))), ("alias", "x_in in the tail of masks", dict(x_in=("masks", 112))),
                                    ("alias", "latent is masks", dict(latent=("masks", 0))), ("alias", "x_in in the tail of bg", dict(x_in=("bg", 496))),
                                    ("alias", "latent inside bg", dict(latent=("bg", 256))), ("alias", "x_in is noise", dict(x_in=("noise", 0))),
                                    ("alias", "latent in the tail of noise", dict(latent=("noise", 240)))],
    # a view row C 4096 is 16 384 bytes: eps and x_in 131 072; a panorama plane 20 736: latent, value, count, noise; masks 41 472; bg 32 768
    "lgd_multidiffusion_views_f32": [("entry", "V != nbh nbw", dict(V=3)), ("entry", "v0 + nv > V", dict(v0=3)), ("entry", "v0 = -1", dict(v0=-1)),
                                     ("entry", "nvc < nv", dict(nvc=1)), ("divisibility", "Wp % 4", dict(Wp=74)), ("entry", "Hp < 64", dict(Hp=56)),
                                     ("entry", "Wp < 64", dict(Wp=60)), ("entry", "C > 64", dict(C=65)),
                                     ("entry", "a multi-chunk call without value", dict(normalization=0, value=None)),
                                     ("entry", "normalization without count", dict(count=None)),
                                     ("entry", "bootstrapping without picks", dict(prep=1, picks=None)),
                                     ("entry", "bootstrapping without bg", dict(prep=1, bg=None)),
                                     ("entry", "bootstrapping without noise", dict(prep=1, noise=None)),
                                     ("entry", "Pp < P", dict(Pp=1)), ("entry", "prep = 2", dict(prep=2)), ("entry", "n_boot = -1", dict(n_boot=-1)),
                                     ("alias", "latent is value", dict(latent=("value", 0))), ("alias", "value in the tail of count", dict(value=("count", 20720))),
                                     ("alias", "count is latent", dict(count=("latent", 0))), ("alias", "latent inside eps", dict(latent=("eps", 4096))),
                                     ("alias", "value in the tail of x_in", dict(value=("x_in", 131056))), ("alias", "count in the tail of masks", dict(count=("masks", 41456))),
                                     ("alias", "latent is masks", dict(latent=("masks", 0))), ("alias", "value is eps", dict(value=("eps", 0))),
                                     ("alias", "prep: x_in is latent", dict(prep=1, x_in=("latent", 0))),
                                     ("alias", "prep: x_in in the tail of masks", dict(prep=1, x_in=("masks", 41456))),
                                     ("alias", "prep: x_in in the tail of bg", dict(prep=1, x_in=("bg", 32752))),
                                     ("alias", "prep: x_in is noise", dict(prep=1, x_in=("noise", 0)))],
    # 100 pixels: img 300 bytes, y 1600, the table 1024
    "lgd_image_u8_to_nhwc8_f16": [("divisibility", "B HW % 4", dict(HW=5)), ("alias", "y is img", dict(y=("img", 0))),
                                  ("alias", "y in the tail of img", dict(y=("img", 288))), ("alias", "y in the tail of the table", dict(y=("table", 1008)))],
    # moments, noise and out are 640 bytes each
    "lgd_vae_sample_f32": [("divisibility", "z % 4", dict(z=6)), ("divisibility", "HW % 4", dict(HW=22)), ("alias", "out is moments", dict(out=("moments", 0))),
                           ("alias", "out in the tail of moments", dict(out=("moments", 624))), ("alias", "out is noise", dict(out=("noise", 0))),
                           ("alias", "out in the tail of noise", dict(out=("noise", 624)))],
    # 108 window rows: qa, ka, va 6912 bytes each; qkv 6720, qkv_bias 192, rel_h and rel_w 160
    "lgd_sam_relpos_qkv_f16": [("entry", "DA < d + 2S", dict(DA=8)), ("entry", "window = 0 with Hs != Ws", dict(window=0)), ("entry", "window = -1", dict(window=-1)),
                               ("divisibility", "d % 8", dict(d=12, DA=24)), ("divisibility", "DA % 8", dict(DA=20)), ("entry", "scale = 0", dict(scale=0.0)),
                               ("entry", "scale = NaN", dict(scale=NAN)), ("entry", "scale = -1", dict(scale=-1.0)),
                               ("alias", "ka is qa", dict(ka=("qa", 0))), ("alias", "va in the tail of qa", dict(va=("qa", 6910))),
                               ("alias", "ka is va", dict(ka=("va", 0))), ("alias", "qa in the tail of qkv", dict(qa=("qkv", 6718))),
                               ("alias", "ka in the tail of qkv_bias", dict(ka=("qkv_bias", 190))), ("alias", "va in the tail of rel_h", dict(va=("rel_h", 158))),
                               ("alias", "qa is rel_w", dict(qa=("rel_w", 0)))],
    # oa 6912 bytes, out 70 x 16 halfs = 2240
    "lgd_sam_window_merge_f16": [("divisibility", "d % 8", dict(d=12)), ("divisibility", "DA % 8", dict(DA=20)), ("entry", "DA < d", dict(d=24)),
                                 ("entry", "window = 0 with Hs != Ws", dict(window=0)), ("entry", "window = -1", dict(window=-1)),
                                 ("entry", "oa off by 2 bytes", dict(oa=2)), ("alias", "out is oa", dict(out=("oa", 0))),
                                 ("alias", "out in the tail of oa", dict(out=("oa", 6896)))],
    "lgd_scale_rows_f32": [("alias", "out is x", dict(out=("x", 0))), ("alias", "the second copy over x", dict(x=("out", 28))),
                           ("entry", "col = row_stride", dict(col=5)), ("entry", "col -1", dict(col=-1)), ("entry", "row_stride 0", dict(row_stride=0))],
}
NEEDS = {fn: {"alias", "divisibility"} for fn in ARGS}   # the rule classes an entry point has beyond NULL / alignment / counts
NEEDS["lgd_select_row_f32"] = set()                      # the table's extent is not an argument: nothing to overlap with, no divisibility
NEEDS["lgd_scale_rows_f32"] = {"alias"}
for _fn in ("lgd_cfg_ddim_step_f32", "lgd_cfg_multistep_step_f32"):
    NEEDS[_fn] = {"alias", "entry"}
for _fn in ("lgd_axpy_f32", "lgd_act_f16", "lgd_multidiffusion_step_f32", "lgd_multidiffusion_views_f32", "lgd_sam_relpos_qkv_f16",
            "lgd_sam_window_merge_f16"):
    NEEDS[_fn] = {"alias", "divisibility", "entry"}


def pointers(fn):
    return [n[2:] for n in ARGS[fn].split() if n.startswith("p:")]


def _generated(fn):
    rows = []
    for p in pointers(fn):
        if p not in optional(fn):
            rows.append((fn, f"{p} NULL", {p: None}))
        a = ALIGN[fn][p]
        rows.append((fn, f"{p} off {a} bytes", {p: a // 2}))
    for c in COUNTS[fn]:
        rows += [(fn, f"{c} = 0", {c: 0}), (fn, f"{c} = -1", {c: -1})]
    return rows


REFUSALS = [r for fn in ARGS for r in _generated(fn) + [(fn, label, change) for _, label, change in RULES[fn]]]
UNSUPPORTED = [("lgd_conv_out_f16", "Cout 5", dict(Cout=5)), ("lgd_conv_out_f16", "Cout 0", dict(Cout=0)),
               ("lgd_conv_in_f16", "the filter and the patches past 64 KB of LDS", dict(Cin=8, Cout=400)),
               ("lgd_sam_relpos_qkv_f16", "more than 2^31 - 1 window rows", dict(B=1 << 28)),
               ("lgd_sam_relpos_qkv_f16", "the query and its rel columns past 64 KB of LDS", dict(NH=2048))]


def call_args(fn, change, base=P):
    """The argument list of BASE[fn] with `change` applied; operands 1 MiB apart from `base`, a NULL stream."""
    vals = dict(BASE[fn], stream=None)
    ptrs = pointers(fn)
    vals.update({p: 0 for p in ptrs})
    vals.update(change)
    out = []
    for n in ARGS[fn].split():
        if not n.startswith("p:"):
            out.append(vals[n])
            continue
        v = vals[n[2:]]
        if v is None:
            out.append(None)
        else:
            slot, off = (v[0], v[1]) if isinstance(v, tuple) else (n[2:], v)
            out.append(base + (ptrs.index(slot) << 20) + off)
    return out
