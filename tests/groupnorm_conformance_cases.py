"""The GroupNorm launch contract as test data: one row per form the GroupNorm entry points accept, each claiming the code of
the kernel instantiation (ops.GN_VARIANTS, lgd_groupnorm_plan) it runs under the option state it names.

A ROW names the code, the shape and the options; `row.data(pass_name)` holds the logical operands, `fwd_reference` /
`bwd_reference` the fp64 results and the derived per-element error bounds, `fwd_emulation` / `bwd_emulation` an fp32
rendering of each path's arithmetic (CPU suite: the bound is not too tight).  The GPU suite carves every operand
(tests/gemm_conformance_cases.Carved): NaN in front of and behind every input, sentinels around every output.

Geometry (csrc/norm.hip): cpg = C / G; kg = smallest count with kg cpg % 8 == 0 (groups per workgroup of the one-launch
kernels), nv = kg cpg / 8 vector columns, pl = threads / nv pixel lanes, npx = ceil(HW / pl) pixels per thread.  The
two-launch kernels: vs = min(C / 8, 256) columns, pl = 256 / vs, nchunk = ops.gn_chunks(B, HW) pixel chunks of
p_per = ceil(HW / nchunk), n_pass = ceil(C / 2048) channel passes.

Data passes
  "plain"   unit-scale x with a scale of 0.1 .. 3 per (image, group);
  "offset"  x = +-4 per (image, group) + 0.25 N(0, 1): group mean^2 / var = 256, which E[x^2] - mean^2 has to cancel;
  "flat"    as plain, one group of each image constant (group (21 + b) % G: variance exactly 0, y = beta exactly).
  gamma = 1 +- 0.5, beta ~ N(0, 1) (SiLU sees both tails); gy = a_g + b_g xhat + 0.5 N(0, 1) with |a_g|, |b_g| in 0.75 .. 1.25,
  so mean(dxhat) and mean(dxhat xhat) carry as much of dx as dxhat does; the accumulate base is N(0, 1) in fp16.

The bound.  u = 2^-11 (fp16), w = 2^-24 (fp32); n = HW cpg; m, var, r = (var + eps)^-1/2 the fp64 statistics of a group,
A = mean|x|, E2 = mean x^2 over it.  An fp32 sum in a fixed tree whose longest chain of additions is D errs by at most
D w sum|terms|.  D, read from the kernels:
  fused forward      D = npx + pl + cpg                 (thread: its pixels; thread j < W: the pixel lanes; thread < kg: channels)
  two-launch         D = ceil(p_per / pl) + ceil(cpg pl / T) + log2 T + n_pass + ceil(nchunk / nsl) + min(nsl, nchunk),
                     T = the largest power of two <= min(64, 256 / G) lanes per group, nsl = 256 / G slices of the partial table
                     (a slice past the last chunk holds 0, and adding 0 is exact)
  slab backward      D = npx + 8 + ceil(pl / 64) + 6 + cpg / 8 + 2     (pixels, the 8 channels, lane stride, butterfly, columns)
 forward
  S1  mean: e_m = (D + 2) w A                                                    (the sum, one divide)
  S2  variance.  fused (two passes, centred): dv = (D + 5) w var + e_m^2       (sum (x - m^)^2 = sum (x - m)^2 + n dm^2)
                 two launches (E[x^2] - mean^2): dv = (D + 3) w E2 + 2 e_m |m| + 2 w m^2 + w var, then clamped at 0
  S3  rstd = rsqrtf(v^ + eps): with q = var + eps, v^ + eps in [max(q - dv, eps), q + dv] (the clamp keeps it >= eps), so
      e_r = max(sqrt(q / max(q - dv, eps)) - 1, 1 - sqrt(q / (q + dv))) + w + 2^-22 relative — finite for the flat group,
      where it is the cancellation term dv / eps ~ D w E2 / eps that decides;
      statistics output: |mean^ - m| <= e_m + w |m|, |rstd^ - r| <= r (e_r + w)
  S4  z^ = x sa + sb, sa = rstd^ gamma, sb = beta - mean^ sa:
      e_z = |x - m| r |gamma| (e_r + 2 w) + e_m r |gamma| (1 + e_r) + w ((|x| + 2 |m|) r |gamma| + |beta| + |z|)
  S5  SiLU = z / (1 + __expf(-z)): v_exp_f32 at 2^-22 relative and the fp32 rounding of its argument, e_E = 2^-22 + 2 w |z|;
      s = sigmoid: e_y = (|silu'(z)| + e_z) e_z + |y| ((1 - s) e_E + 5 w)        (add, divide)
  S6  one fp16 rounding: |y^ - y| <= u |y| + 2^-25 + (1 + u) e_y                  (e_y = e_z without SiLU)
 backward (mean, rstd AS GIVEN: the fp32-rounded reference statistics; the reference uses the same)
  B1  xhat: two launches (x - mean) rstd: e_x = 2 w |xh|; slab x ra + rb, rb = -mean rstd: e_x = w (|x| + |mean|) rstd + w |xh|
  B2  z = gamma xh + beta: e_z = |gamma| e_x + w |gamma xh| + w |z|
  B3  silu'(z) = s (1 + z (1 - s)), s = 1 / (1 + __expf(-z)): e_s = (1 - s) e_E + 5 w relative,
      e_g = (|g| + s |z|) (e_s + 3 w) + 0.5 e_z + w                               (|silu''| <= 0.5)
  B4  dz = gy g: e_dz = |gy| e_g + w |dz| (0 without SiLU);  d = dz gamma: e_d = |gamma| e_dz + w |d|
  B5  m1 = mean d: e_1 = (D + 3) w mean|d| + mean e_d;  m2 = mean d xh: e_2 = (D + 4) w mean|d xh| + mean(e_d |xh| + |d| e_x)
  B6  t = d - m1 - xh m2: e_t = e_d + e_1 + |xh| e_2 + |m2| e_x + 3 w (|d| + |m1| + |xh m2|);  dx = rstd t
  B7  out = dx (+ the fp16 base, exact): |out^ - out| <= u |out| + 2^-25 + (1 + u) (rstd e_t + w |dx| + w |out|)

Nothing above is fitted to kernel output; tests/test_groupnorm_conformance_cpu.py shows with the reference alone that an
fp32 emulation of each path stays inside and that eight wrong answers fall outside."""
import functools
import math
import os
import sys

import torch

from lgd_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_conformance_cases import GUARD, SENT16, SENT32, Carved, P  # noqa: E402,F401

H16, F32, F64 = torch.float16, torch.float32, torch.float64
U, W = 2.0 ** -11, 2.0 ** -24
NAN = float("nan")
DEFAULT_OPTS = {"gn_fused": 256, "gn_slab": 1}
PASSES = ("plain", "offset", "flat")
FUSED = {104: 4, 108: 8, 116: 16, 132: 32}
SLAB = {300: (256, 8), 301: (256, 8), 310: (512, 11), 311: (512, 11)}


def set_options(opts):
    for k, v in opts.items():
        ops.set_option(k, v)


def slab_geometry(C, G):
    cpg = C // G
    kg = 1
    while (kg * cpg) % 8:
        kg *= 2
    return cpg, kg, kg * cpg // 8


class Row:
    def __init__(self, code, op, c0, c1, HW, B, *, G=32, silu=False, opts=None, note=""):
        self.code, self.op, self.c0, self.c1, self.HW, self.B, self.G, self.silu = code, op, c0, c1, HW, B, G, silu
        self.opts = dict(DEFAULT_OPTS, **(opts or {}))
        self.C = c0 + c1
        self.cpg = self.C // G
        self.eps = 1e-5 if silu else 1e-6                    # the resnets' and the transformers' GroupNorm of the UNet
        self.nchunk = ops.gn_chunks(B, HW)
        self.note = note
        self.name = f"{code}:{op}:C{c0}+{c1}:HW{HW}:B{B}:G{G}" + (":silu" if silu else "") + (":" + note if note else "")

    @property
    def two_launch(self):
        return self.code in (201, 202, 400)

    @property
    def slab(self):
        return self.code in SLAB

    @property
    def depth(self):
        """D of the docstring for the kernel this row claims."""
        C, G, HW, cpg = self.C, self.G, self.HW, self.cpg
        _, kg, nv = slab_geometry(C, G)
        if self.code in FUSED:
            pl = 256 // nv
            return -(-HW // pl) + pl + cpg
        if self.code in SLAB:
            pl = SLAB[self.code][0] // nv
            return -(-HW // pl) + 8 + -(-pl // 64) + 6 + cpg // 8 + 2
        vs = min(C // 8, 256)
        pl = 256 // vs
        p_per = -(-HW // self.nchunk)
        T = 1
        while T * 2 * G <= 256 and T < 64:
            T *= 2
        nsl = 256 // G
        return (-(-p_per // pl) + -(-(cpg * pl) // T) + int(math.log2(T)) + -(-(C // 8) // vs)
                + -(-self.nchunk // nsl) + min(nsl, self.nchunk))

    def plan(self, pair=0):
        """The code the library answers for this row under the current option state."""
        return ops.groupnorm_plan(ops.GN_OP_FWD if self.op == "fwd" else ops.GN_OP_BWD, self.c0, self.c1, self.B, self.HW,
                                  self.G, silu=self.silu, pair=pair)

    def data(self, pass_name):
        return _data(self.name, pass_name)


@functools.lru_cache(maxsize=2)
def _data(row_name, pass_name):
    return Data(ROWS_BY_NAME[row_name], pass_name)


def flat_group(b, G):
    return (21 + b) % G


class Data:
    """x [B][HW][C] and gy / base (backward rows) as fp16, gamma / beta as fp32, on the host."""

    def __init__(self, row, pass_name):
        r = row
        g = torch.Generator().manual_seed(9000 + sum(map(ord, r.name)) % 1000 + PASSES.index(pass_name))
        B, HW, G, cpg, C = r.B, r.HW, r.G, r.cpg, r.C
        noise = torch.randn(B, HW, G, cpg, generator=g)
        if pass_name == "offset":
            sign = torch.where(torch.rand(B, 1, G, 1, generator=g) < 0.5, -1.0, 1.0)
            x = 4.0 * sign + 0.25 * noise
        else:
            x = noise * (0.1 + 2.9 * torch.rand(B, 1, G, 1, generator=g))
            if pass_name == "flat":
                for b in range(B):
                    x[b, :, flat_group(b, G), :] = 1.375 + 0.25 * b
        self.x = x.reshape(B, HW, C).to(H16)
        self.gamma = (1.0 + 0.5 * (2.0 * torch.rand(C, generator=g) - 1.0)).to(F32)
        self.beta = torch.randn(C, generator=g).to(F32)
        self.gy = self.base = None
        if r.op == "bwd":
            xg = self.x.to(F64).view(B, HW, G, cpg)
            m = xg.mean((1, 3), keepdim=True)
            xh = (xg - m) * (((xg - m) ** 2).mean((1, 3), keepdim=True) + r.eps) ** -0.5
            ab = (0.75 + 0.5 * torch.rand(2, B, 1, G, 1, generator=g)) * torch.where(torch.rand(2, B, 1, G, 1, generator=g) < 0.5, -1.0, 1.0)
            self.gy = (ab[0] + ab[1] * xh + 0.5 * torch.randn(B, HW, G, cpg, generator=g)).reshape(B, HW, C).to(H16)
            self.base = torch.randn(B, HW, C, generator=g).to(H16)


# ---------------------------------------------------------------------------------------------
# fp64 references and derived bounds; x [B][HW][C] fp64 (fp16 values), gamma / beta [C] fp64 (fp32 values)
# ---------------------------------------------------------------------------------------------
def _grp(t, G):
    if t.dim() == 4:
        return t
    B, HW, C = t.shape
    return t.reshape(B, HW, G, C // G)


def _gmean(t, G):
    """mean over the pixels and channels of every (image, group): [B][G]"""
    return _grp(t, G).mean((1, 3))


def _per_channel(stat, chan_group):
    """[B][G] -> [B][1][C] through the group index of every channel"""
    return stat[:, chan_group].unsqueeze(1)


def _sigmoid(z):
    return 1.0 / (1.0 + torch.exp(-z))


def fwd_reference(x, gamma, beta, G, eps, silu, *, depth, two_launch, pix=None, n_pixels=None, chan_group=None):
    """dict(y, mean, rstd [B][G], bound_y, bound_mean, bound_rstd) — docstring S1 .. S6.
    Wrong answers (CPU suite): pix = the pixels the statistics see (index tensor), n_pixels = the pixel count they divide by,
    chan_group = the group whose statistics each channel is normalised with."""
    B, HW, C = x.shape
    cpg = C // G
    xs = x if pix is None else x[:, pix]
    n = (xs.shape[1] if n_pixels is None else n_pixels) * cpg
    s1 = _grp(xs, G).sum((1, 3))
    mean = s1 / n
    if pix is None and n_pixels is None:
        var = _gmean((_grp(x, G) - mean[:, None, :, None]) ** 2, G)
    else:
        var = ((_grp(xs, G) ** 2).sum((1, 3)) / n - mean ** 2).clamp_min(0.0)
    q = var + eps
    rstd = q ** -0.5
    A, E2 = _gmean(x.abs(), G), _gmean(x * x, G)
    e_m = (depth + 2) * W * A
    dv = ((depth + 3) * W * E2 + 2 * e_m * mean.abs() + 2 * W * mean ** 2 + W * var) if two_launch else ((depth + 5) * W * var + e_m ** 2)
    e_r = torch.maximum((q / (q - dv).clamp_min(eps)).sqrt() - 1.0, 1.0 - (q / (q + dv)).sqrt()) + W + 2.0 ** -22
    cg = torch.arange(C, device=x.device) // cpg if chan_group is None else chan_group
    m_c, r_c, em_c, er_c = (_per_channel(t, cg) for t in (mean, rstd, e_m, e_r))
    ag, ab = gamma.abs(), beta.abs()
    z = (x - m_c) * r_c * gamma + beta
    e_z = ((x - m_c).abs() * r_c * ag * (er_c + 2 * W) + em_c * r_c * ag * (1.0 + er_c)
           + W * ((x.abs() + 2 * m_c.abs()) * r_c * ag + ab + z.abs()))
    if silu:
        s = _sigmoid(z)
        y = z * s
        d1 = (s * (1.0 + z * (1.0 - s))).abs()
        e_y = (d1 + e_z) * e_z + y.abs() * ((1.0 - s) * (2.0 ** -22 + 2 * W * z.abs()) + 5 * W)
    else:
        y, e_y = z, e_z
    return dict(y=y, mean=mean, rstd=rstd, bound_y=U * y.abs() + 2.0 ** -25 + (1 + U) * e_y,
                bound_mean=e_m + W * mean.abs(), bound_rstd=rstd * (e_r + W))


def bwd_reference(x, gy, gamma, beta, mean32, rstd32, G, silu, *, depth, slab, base=None, no_m1=False, m2_group=None,
                  sigmoid_grad=False, base_twice=False):
    """dict(dx, bound_dx) from the statistics as given ([B][G], fp32 values) — docstring B1 .. B7.
    Wrong answers (CPU suite): no_m1, m2_group (the group whose m2 each channel takes), sigmoid_grad, base_twice."""
    B, HW, C = x.shape
    cpg = C // G
    cg = torch.arange(C, device=x.device) // cpg
    m_c, r_c = _per_channel(mean32, cg), _per_channel(rstd32, cg)
    ag = gamma.abs()
    xh = (x - m_c) * r_c
    e_x = (W * (x.abs() + m_c.abs()) * r_c + W * xh.abs()) if slab else 2 * W * xh.abs()
    if silu:
        z = gamma * xh + beta
        e_z = ag * e_x + W * (gamma * xh).abs() + W * z.abs()
        s = _sigmoid(z)
        gsl = s if sigmoid_grad else s * (1.0 + z * (1.0 - s))
        e_s = (1.0 - s) * (2.0 ** -22 + 2 * W * z.abs()) + 5 * W
        e_g = (gsl.abs() + s * z.abs()) * (e_s + 3 * W) + 0.5 * e_z + W
        dz = gy * gsl
        e_dz = gy.abs() * e_g + W * dz.abs()
    else:
        dz, e_dz = gy, torch.zeros_like(gy)
    d = dz * gamma
    e_d = ag * e_dz + W * d.abs()
    m1, m2 = _gmean(d, G), _gmean(d * xh, G)
    e_1 = (depth + 3) * W * _gmean(d.abs(), G) + _gmean(e_d, G)
    e_2 = (depth + 4) * W * _gmean((d * xh).abs(), G) + _gmean(e_d * xh.abs() + d.abs() * e_x, G)
    m1_c, e1_c, e2_c = (_per_channel(t, cg) for t in (m1, e_1, e_2))
    m2_c = _per_channel(m2, cg if m2_group is None else m2_group)
    if no_m1:
        m1_c = torch.zeros_like(m1_c)
    dx = r_c * (d - m1_c - xh * m2_c)
    e_t = e_d + e1_c + xh.abs() * e2_c + m2_c.abs() * e_x + 3 * W * (d.abs() + m1_c.abs() + (xh * m2_c).abs())
    out = dx if base is None else dx + base * (2.0 if base_twice else 1.0)
    bound = U * out.abs() + 2.0 ** -25 + (1 + U) * (r_c * e_t + W * dx.abs() + W * out.abs())
    return dict(dx=out, bound_dx=bound)


def first_vector_group(C, G):
    """The group of the first channel of every channel's 16-byte vector: differs from the channel's own group exactly on the
    upper channels of a vector that straddles two groups."""
    return (torch.arange(C) // 8 * 8) // (C // G)


# ---------------------------------------------------------------------------------------------
# fp32 emulations of each path's arithmetic (CPU suite: the bound is not too tight)
# ---------------------------------------------------------------------------------------------
def _r16(t):
    return t.to(H16).to(F32)


def _lane_sum(t, lanes):
    """fp32 sum over the pixels of t [B][P][G][cpg] in the kernels' structure: each of `lanes` pixel lanes adds its pixels
    (p, p + lanes, ..), then the lanes are added, then the channels -> [B][G]"""
    B, Pn, G, cpg = t.shape
    pad = (-Pn) % lanes
    if pad:
        t = torch.cat([t, torch.zeros(B, pad, G, cpg, dtype=t.dtype)], 1)
    return t.view(B, -1, lanes, G, cpg).sum(1).sum(1).sum(-1)


def _chunked_sum(t, lanes, nchunk):
    """as gn_stats_kernel + the partial table of gn_apply_kernel: nchunk chunks of ceil(HW / nchunk) pixels (some short, some
    empty), each summed over its pixel lanes, then the partials"""
    HW = t.shape[1]
    p_per = -(-HW // nchunk)
    tot = torch.zeros(t.shape[0], t.shape[2], dtype=F32)
    for ch in range(nchunk):
        lo, hi = ch * p_per, min(HW, (ch + 1) * p_per)
        if hi > lo:
            tot = tot + _lane_sum(t[:, lo:hi], lanes)
    return tot


def _silu32(z):
    return z / (1.0 + torch.exp(-z))


def fwd_emulation(row, x, gamma, beta):
    """x [B][HW][C] fp32 (fp16 values), gamma / beta fp32 -> dict(y fp16 values, mean, rstd fp32 [B][G])"""
    G, cpg, HW = row.G, row.cpg, row.HW
    n = torch.tensor(float(HW * cpg), dtype=F32)
    eps = torch.tensor(row.eps, dtype=F32)
    xg = _grp(x, G)
    if row.two_launch:
        lanes = 256 // min(row.C // 8, 256)
        mean = _chunked_sum(xg, lanes, row.nchunk) / n
        var = (_chunked_sum(xg * xg, lanes, row.nchunk) / n - mean * mean).clamp_min(0.0)
    else:
        lanes = 256 // slab_geometry(row.C, G)[2]
        mean = _lane_sum(xg, lanes) / n
        var = _lane_sum((xg - mean[:, None, :, None]) ** 2, lanes) / n
    rstd = torch.rsqrt(var + eps)
    sa = (rstd[:, None, :, None] * gamma.view(G, cpg))
    sb = beta.view(G, cpg) - mean[:, None, :, None] * sa
    z = xg * sa + sb
    y = _silu32(z) if row.silu else z
    return dict(y=_r16(y).reshape(x.shape), mean=mean, rstd=rstd)


def bwd_emulation(row, x, gy, gamma, beta, mean32, rstd32, base=None):
    G, cpg, HW = row.G, row.cpg, row.HW
    n = torch.tensor(float(HW * cpg), dtype=F32)
    xg, gg = _grp(x, G), _grp(gy, G)
    m, r = mean32[:, None, :, None], rstd32[:, None, :, None]
    gm, bt = gamma.view(G, cpg), beta.view(G, cpg)
    xh = (xg * r + (-m * r)) if row.slab else (xg - m) * r
    dz = gg
    if row.silu:
        z = gm * xh + bt
        s = 1.0 / (1.0 + torch.exp(-z))
        dz = gg * (s * (1.0 + z * (1.0 - s)))
    d = dz * gm
    if row.slab:
        lanes = SLAB[row.code][0] // slab_geometry(row.C, G)[2]
        inv_n = 1.0 / n
        m1, m2 = _lane_sum(d, lanes) * inv_n, _lane_sum(d * xh, lanes) * inv_n
    else:
        lanes = 256 // min(row.C // 8, 256)
        m1, m2 = _chunked_sum(d, lanes, row.nchunk) / n, _chunked_sum(d * xh, lanes, row.nchunk) / n
    dx = r * (d - m1[:, None, :, None] - xh * m2[:, None, :, None])
    if base is not None:
        dx = dx + _grp(base, G)
    return dict(dx=_r16(dx).reshape(x.shape))


# ---------------------------------------------------------------------------------------------
# the rows
# ---------------------------------------------------------------------------------------------
_F0, _F512, _F1024, _S0 = {"gn_fused": 0}, {"gn_fused": 512}, {"gn_fused": 1024}, {"gn_slab": 0}
_ROW_LIST = [
    # ---- forward, one launch
    Row(104, "fwd", 320, 0, 64, 3, silu=True, note="four groups per workgroup, vectors straddle groups"),
    Row(104, "fwd", 32, 0, 7, 1, note="cpg 1, 249 idle pixel lanes, one chunk"),
    Row(104, "fwd", 128, 64, 256, 2, note="cpg 6, the seam inside group 21"),
    Row(104, "fwd", 1280, 0, 64, 2, silu=True, note="the fused form of the gn_fused 0 row"),
    Row(108, "fwd", 1280, 0, 256, 2, silu=True),
    Row(108, "fwd", 960, 0, 100, 1, note="ragged, cpg 30, pl 17"),
    Row(116, "fwd", 1280, 1280, 256, 2, silu=True),
    Row(116, "fwd", 1536, 768, 256, 1, silu=True, note="cpg 72, the seam inside group 21"),
    Row(132, "fwd", 1280, 1280, 420, 1, silu=True, opts=_F512),
    Row(132, "fwd", 1280, 0, 1024, 1, opts=_F1024),
    # ---- forward, two launches
    Row(201, "fwd", 320, 0, 300, 2, silu=True, note="37 chunks of 9 pixels: one part filled, three empty"),
    Row(202, "fwd", 1536, 1536, 288, 1, silu=True, note="two channel passes, group 21 straddles channel 2048"),
    Row(201, "fwd", 128, 0, 1024, 1, silu=True, note="cpg 4"),
    Row(201, "fwd", 1280, 0, 64, 2, silu=True, opts=_F0, note="a small map on the two-launch kernels"),
    Row(201, "fwd", 320, 0, 4096, 2, note="64 chunks"),
    Row(201, "fwd", 960, 0, 300, 1, G=24, silu=True),
    Row(201, "fwd", 512, 0, 300, 1, G=64, note="cpg 8"),
    Row(201, "fwd", 64, 0, 300, 1, G=8, silu=True),
    Row(201, "fwd", 64, 0, 300, 1, G=1),
    # ---- backward
    Row(301, "bwd", 1280, 0, 64, 4, silu=True),
    Row(300, "bwd", 320, 0, 256, 2, note="cpg 10, kg 4: vectors straddle groups"),
    Row(301, "bwd", 960, 0, 100, 2, silu=True, note="ragged"),
    Row(301, "bwd", 1280, 640, 64, 2, silu=True, note="cpg 60, kg 2: the seam inside a slab and a group"),
    Row(301, "bwd", 1280, 1280, 64, 2, silu=True, note="the slab form of the gn_slab 0 row"),
    Row(310, "bwd", 1280, 1280, 256, 2),
    Row(311, "bwd", 1280, 0, 576, 1, silu=True, note="24x24"),
    Row(400, "bwd", 128, 64, 256, 2, silu=True, note="cpg 6"),
    Row(400, "bwd", 1280, 640, 256, 2, silu=True, note="slab over 96 KB"),
    Row(400, "bwd", 320, 0, 700, 2, note="ragged, past both slab limits"),
    Row(400, "bwd", 1280, 1280, 64, 2, silu=True, opts=_S0, note="two channel passes"),
    Row(301, "bwd", 960, 0, 100, 2, G=24, silu=True),
]
ROWS_BY_NAME = {r.name: r for r in _ROW_LIST}
assert len(ROWS_BY_NAME) == len(_ROW_LIST)
CODES = sorted({r.code for r in _ROW_LIST})
# pair forms: B = 4, images 2 and 3 copies of images 0 and 1
PAIR_ROWS = [Row(104, "fwd", 320, 0, 64, 4, silu=True, note="pair"), Row(108, "fwd", 1280, 0, 256, 4, silu=True, note="pair"),
             Row(201, "fwd", 320, 0, 300, 4, silu=True, note="pair")]
for _r in PAIR_ROWS:
    ROWS_BY_NAME[_r.name] = _r


def rows_of(code):
    return [r for r in _ROW_LIST if r.code == code]


# ---------------------------------------------------------------------------------------------
# host refusals: every row differs in ONE respect from a call the library accepts and is answered with LGD_ERR_ARG before
# the device is touched (the CPU suite asks the entry points themselves with placeholder pointers and a NULL stream; the
# GPU suite passes addresses inside a sentinel buffer and checks that nothing was written).
# ("stats together with pair" is not a row: lgd_groupnorm_pair_f16 has no statistics argument; ops.groupnorm refuses it.)
# ---------------------------------------------------------------------------------------------
ARGS = {
    "lgd_groupnorm_f16": "p:x0 p:x1 c0 c1 B HW G eps p:gamma p:beta silu p:y p:part nchunk p:stats",
    "lgd_groupnorm_pair_f16": "p:x0 p:x1 c0 c1 B HW G eps p:gamma p:beta silu p:y p:part nchunk pair",
    "lgd_groupnorm_bwd_f16": "p:gy p:x0 p:x1 c0 c1 B HW G p:gamma p:beta silu p:stats p:gx0 p:gx1 p:part nchunk accumulate",
}
_FWD, _PAIR, _BWD = ARGS
_COMMON = [("G > 64", dict(G=128)), ("G = 0", dict(G=0)), ("G < 0", dict(G=-1)), ("C > 4096", dict(c0=4096)),
           ("C % G", dict(G=24)), ("c0 % 8", dict(c0=68, G=4)), ("c1 % 8", dict(c1=68, G=4)), ("nchunk < 1", dict(nchunk=0)),
           ("B < 1", dict(B=0)), ("HW < 1", dict(HW=0)), ("NULL x0", dict(x0=None)), ("NULL x1 with c1 > 0", dict(x1=None)),
           ("NULL gamma", dict(gamma=None)), ("NULL beta", dict(beta=None)), ("NULL part", dict(part=None))]
REFUSALS = ([(fn, w, c) for fn in (_FWD, _PAIR, _BWD) for w, c in _COMMON]
            + [(fn, "NULL y", dict(y=None)) for fn in (_FWD, _PAIR)]
            + [(_PAIR, "pair mode 0", dict(pair=0)), (_PAIR, "pair mode 3", dict(pair=3)), (_PAIR, "odd B", dict(B=3)),
               (_BWD, "NULL gy", dict(gy=None)), (_BWD, "NULL stats", dict(stats=None)), (_BWD, "NULL gx0", dict(gx0=None)),
               (_BWD, "NULL gx1 with c1 > 0", dict(gx1=None))])
PLAN_ARGS = ("c0", "c1", "B", "HW", "G", "pair")        # what lgd_groupnorm_plan sees of a call


def refusal_values(fn, change):
    vals = dict(c0=64, c1=64, B=2, HW=64, G=32, eps=1e-5, silu=1, nchunk=8, pair=1, accumulate=0)
    vals.update({n[2:]: 0 for n in ARGS[fn].split() if n.startswith("p:")})
    vals.update(change)
    return vals


def refusal_args(fn, change, base):
    """The ctypes argument list of REFUSALS row (fn, .., change): an accepted call with `change` applied and a NULL stream.
    Operands sit 1 MiB apart from `base`."""
    import ctypes
    vals = refusal_values(fn, change)
    names = ARGS[fn].split()
    ptrs = [n[2:] for n in names if n.startswith("p:")]
    out = []
    for n in names:
        if n.startswith("p:"):
            v = vals[n[2:]]
            out.append(ctypes.c_void_p(None if v is None else base + (ptrs.index(n[2:]) << 20) + v))
        elif n == "eps":
            out.append(ctypes.c_float(vals[n]))
        else:
            out.append(vals[n])
    return out + [ctypes.c_void_p(None)]
