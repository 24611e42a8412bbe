"""The attention launch contract as test data: one row per variant code of the attention dispatch (ops.ATTN_VARIANTS,
lgd_attn_plan), at the smallest shape that selects it, with every view form its op is asked to serve.

A ROW names the code, the option state and the shape; `row.data(pass_name)` holds the logical operands (fp16 values),
`reference(...)` the fp64 result and the derived per-element error bound of a group of (image, head) pairs, `views(form,
...)` the operands carved into larger buffers (tests/gemm_conformance_cases.Carved: guards in front and behind, NaN in
every input element the strides skip, sentinels in every output element).  The reference never reads the strided buffers.

Shapes are ragged on purpose: Sq = 300 (two 128-row blocks and a tail, five 64-row tiles with a 44-row tail), Sk = 330 (five
64-key tiles and a 10-key tail), Sk_grad = 300; B * H is what crosses the workgroup-count thresholds of the dispatch.

Data passes
  "heads"    N(0, 1) operands; the magnitude of v and go differs by 100x and that of q by 12x across heads (h % 4), so an
             error confined to a small head is as visible as one in a large head — every check is per element;
  "spiked"   a few keys are 6 x one query each (logits near 6 sqrt(d): the running-max rescale, the -inf / large-exponent
             paths), among them the LAST key and one key in the ragged tail tile;
  "voffset"  v = per-channel offset of magnitude 4 .. 8 plus a spread of 0.25, q small: |O| is close to sum_j p_j |v_j|, so
             a wrong normaliser (a pad key counted, a key dropped) is not hidden behind cancellation.

The bound.  Notation: u = 2^-11 (half an ulp of fp16, relative), w = 2^-24 (fp32), t = scale log2(e) q.k (the kernels work
in the log2 domain), A_ij = scale log2(e) sum_e |q_ie| |k_je|, p = softmax.  Rounding points, found by reading the kernels:

 forward (csrc/attn.hip, attn_w4.hip)
  F1  fp16 inputs are exact; QK^T accumulates in fp32: |dt| <= (DP + 2) w (A + |m|), m the running reference exponent,
      |m| <= max_j |t_j| + 9 (the reference lags the row max by at most 2^8 = 8 in the exponent, and is itself an fp16 number);
  F2  the kernels with a row of ones (attn_self_kernel ONES, attn_self32_kernel, attn_w4_kernel: `ones`) pre-multiply Q by
      scale log2(e) and round it to fp16 again: |dt| <= u A.  (This point is not in the issue's list; it is in the code:
      `qf = (half_t)((float)qf * a.scale_log2)`.)  The other kernels scale the fp32 logit: 2 w (|t| + |m|);
  F3  exp2 (v_exp_f32): 2^-22 relative.  Together eps_arith_j = ln2 dt_j + 2^-22;
  F4  P is rounded to fp16 before P.V: u relative, 2^-24 absolute per key for subnormal P (in units of the normalised p);
  F5  the row sum: the `ones` kernels take it from the SAME rounded P through the MFMA (so it carries u as well); the others
      sum the fp32 p.  eps_l = sum_j p_j eps_j + (Sk + 16) w with eps_j = eps_arith_j + (u if ones);
  F6  P.V accumulates in fp32, each running-max rescale multiplies the accumulator once: (Sk + 2 tiles + 16) w S,
      S = sum_j p_j |v_j|;
  F7  one fp16 rounding of O: u |O| + 2^-25.
      |O^ - O| <= u |O| + 2^-25 + sum_j p_j (eps_arith_j + u) |v_j| + eps_l |O| + (2 Sk + 32) w S + 2^-24 sum_j |v_j|
  lse (log2 domain) = m + log2(l):  |d lse| <= log2(e) eps_l + 2 w (|m| + |log2 l|) + 2^-21 (1 + |log2 l|)   (log2f)
  probs (two-pass kernel, fp32): |dp| <= p (eps_arith + eps_l + 3 * 2^-22) + 2^-126

 backward (csrc/attn_bwd.hip); the inputs are q, k, v, go, the fp16 O and the fp32 lse AS GIVEN (the reference uses the same)
  B1  delta = sum_e go_e O_e in fp32 from the fp16 O: e_delta = (d + 6) w sum_e |go_e O_e|;
  B2  the logit and P = exp2(t - lse) as F1 / F3 (no pre-scaled Q here): eps_p = ln2 (DP w A + 2 w (|t| + |lse|)) + 2^-22;
  B3  dP = go.v in fp32: e_dp = (DP + 2) w sum_e |go_e| |v_e|;
  B4  dS = P (dP - delta), then rounded to fp16: r_dS = P (eps_p |dP - delta| + e_dp + e_delta) + (u + 3 w) |dS| + 2^-25;
  B5  P rounded to fp16 for dV: r_P = P (eps_p + u) + 2^-25;
  B6  fp32 accumulation over the contraction (keys for dQ, queries for dK / dV), one multiply by scale;
  B7  one fp16 rounding of each gradient.
      |dQ^ - dQ| <= u |dQ| + 2^-25 + scale (r_dS |k| + (Sk + 16) w |dS| |k|) + 2 w |dQ|      (sums over keys)
      |dK^ - dK| <= u |dK| + 2^-25 + scale (r_dS^T |q| + (Sq + 16) w |dS|^T |q|) + 2 w |dK|  (sums over queries)
      |dV^ - dV| <= u |dV| + 2^-25 + r_P^T |go| + (Sq + 16) w P^T |go|
      |delta^ - delta| <= e_delta + w |delta|

 cross-attention backward (dQ only; softmax recomputed exactly in the kernel, dP = go.v + gp)
  X1  eps_p = ln2 (DP w A + 3 w (|t| + |t_max|)) + 2^-22 + eps_l,  eps_l = sum_j p_j (that) + (Sk + 18) w;
  X2  e_dp = (DP + 2) w (sum_e |go_e| |v_e| + |gp|);  dot = sum_j p_j dP_j: e_dot = sum_j p_j (eps_p |dP_j| + e_dp) + (Sk + 16) w sum_j p_j |dP_j|;
  X3  dS = scale p (dP - dot) rounded to fp16 (MFMA kernel; the row kernel keeps fp32):
      r_dS = scale p (eps_p |dP - dot| + e_dp + e_dot) + 4 w |dS| + (u |dS| + 2^-25 for the MFMA kernel only);
  X4  |dQ^ - dQ| <= u |dQ| + 2^-25 + r_dS |k| + (Sk + 16) w |dS| |k|.

Nothing above is fitted to kernel output; tests/test_attn_conformance_cpu.py shows with the reference alone that an fp32
emulation with exactly these rounding points stays inside, and that six wrong answers fall outside."""
import functools
import os
import sys

import torch

from lgd_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_conformance_cases import GUARD, SENT16, SENT32, Carved, P  # noqa: E402

H16, F32, F64 = torch.float16, torch.float32, torch.float64
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
U, W = 2.0 ** -11, 2.0 ** -24
NAN = float("nan")
DEFAULT_OPTS = {"attn32": 1, "attn32_nw": 8, "attn32_var": 0, "attn_w4": 1, "attn_w4_pipe": 1}
PASSES = ("heads", "spiked", "voffset")
SQ, SK = 300, 330


class Row:
    def __init__(self, code, op, B, H, d, *, Sq=SQ, Sk=SK, sk_grad=None, opts=None, causal=False, aligned=True, note=""):
        # op: "self" (lgd_attn_fwd_f16 / _pair_), "map" (lgd_cross_attn_fwd_f16 with a map, lgd_attn_causal_fwd_f16),
        #     "bwd" (lgd_attn_bwd_keys_f16), "xbwd" (lgd_cross_attn_bwd_f16)
        self.code, self.op, self.B, self.H, self.d, self.Sq, self.Sk = code, op, B, H, d, Sq, Sk
        self.sk_grad = (min(Sk, SQ) if sk_grad is None else sk_grad) if op == "bwd" else Sk
        self.opts = dict(DEFAULT_OPTS, **(opts or {}))
        self.causal, self.aligned, self.note = causal, aligned, note
        self.C = H * d
        self.scale = d ** -0.5
        fam, sub = code // 100000, code % 100
        self.DP = (code // 100) % 1000 or ((d + 31) // 32 * 32)
        self.ds16 = fam != 7                                                  # X3: only the MFMA kernel rounds dS to fp16
        self.ones = fam in (2, 3) or (fam == 1 and sub // 10 in (1, 2))       # F2 / F5: pre-scaled Q, row sum from rounded P
        self.name = f"{code}:{op}:B{B}H{H}S{Sq}x{Sk}d{d}" + (":" + note if note else "")

    @property
    def forms(self):
        if self.op == "self":
            return ("contig", "fused3", "kv2", "gaps") + (("pair_half", "pair_dup") if self.B % 2 == 0 else ())
        if self.op == "map":
            return ("causal_fused",) if self.causal else ("contig", "kv2", "gaps", "tok", "cond_only")
        if self.op == "bwd":
            return ("contig", "fused3", "gaps", "skgrad")
        return ("odd_ld",) if not self.aligned else ("contig", "kv2", "gaps", "no_go", "no_gp")

    def plan(self):
        """The code the library answers for this row under its option state (the caller sets and restores the options)."""
        opn = {"self": ops.ATTN_OP_FWD, "map": ops.ATTN_OP_FWD, "bwd": ops.ATTN_OP_BWD, "xbwd": ops.ATTN_OP_CROSS_BWD}[self.op]
        return ops.attn_plan(opn, self.B, self.H, self.Sq, self.Sk, self.d, sk_grad=self.sk_grad,
                             probs=self.op == "map" and not self.causal, causal=self.causal, aligned=self.aligned)

    def data(self, pass_name):
        return _data(self.name, pass_name)


def set_options(opts):
    for k, v in opts.items():
        ops.set_option(k, v)


@functools.lru_cache(maxsize=4)
def _data(row_name, pass_name):
    return Data(ROWS_BY_NAME[row_name], pass_name)


class Data:
    """Logical operands of one row, [B][H][S][d] fp16 on the host (duplicated halves are made by the pair forms)."""

    def __init__(self, row, pass_name):
        r = row
        g = torch.Generator().manual_seed(7000 + sum(map(ord, r.name)) % 1000 + PASSES.index(pass_name))
        B, H, Sq, Sk, d = r.B, r.H, r.Sq, r.Sk, r.d
        hs = torch.arange(H) % 4
        vmag = torch.tensor([0.03, 0.3, 1.0, 3.0])[hs].view(1, H, 1, 1)
        gmag = torch.tensor([1.0, 3.0, 0.03, 0.3])[hs].view(1, H, 1, 1)
        qmag = torch.tensor([1.0, 0.25, 3.0, 1.5])[hs].view(1, H, 1, 1)
        rn = lambda *s: torch.randn(*s, generator=g)
        q, k, v, go = rn(B, H, Sq, d), rn(B, H, Sk, d), rn(B, H, Sk, d), rn(B, H, Sq, d)
        if pass_name == "heads":
            q, v, go = q * qmag, v * vmag, go * gmag
        elif pass_name == "spiked":
            q = q.half().float()
            for qi, ki in [(5 % Sq, Sk - 1), (Sq // 2 + 1, min(Sk - 1, Sk // 2 + 70)), (Sq - 1, min(Sk - 1, 200)), (Sq // 3, Sk - 3)]:
                if Sk >= 8 and not (r.causal and ki > qi):
                    k[:, :, ki] = q[:, :, qi] * 6.0
            if r.causal and Sk >= 8:
                k[:, :, 3] = q[:, :, Sq - 2] * 6.0
        else:
            off = (4.0 + 4.0 * torch.rand(d, generator=g)) * torch.where(torch.rand(d, generator=g) < 0.5, -1.0, 1.0)
            v = off.view(1, 1, 1, d) + 0.25 * v
            q = q * 0.25
            go = off.flip(0).view(1, 1, 1, d) * 0.125 + go
        self.q, self.k, self.v, self.go = q.to(H16), k.to(H16), v.to(H16), go.to(H16)
        # the map gradient of the cross-attention backward: fp32 [B][H][Sq][Sk]
        self.gp = (rn(B, H, Sq, Sk) * gmag).to(F32) if r.op == "xbwd" else None


# ---------------------------------------------------------------------------------------------
# fp64 reference and derived bounds of a group of (image, head) pairs: every operand [N][S][d] fp64
# ---------------------------------------------------------------------------------------------
def fwd_reference(q, k, v, scale, *, DP, ones, causal=False, want_probs=False):
    """dict(o, lse, bound_o, bound_lse[, p, bound_p]) — docstring F1 .. F7."""
    Sk = k.shape[-2]
    sl2 = scale * LOG2E
    t = (q @ k.transpose(-1, -2)) * sl2
    A = (q.abs() @ k.abs().transpose(-1, -2)) * sl2
    if causal:
        keep = torch.ones(t.shape[-2:], dtype=torch.bool, device=t.device).tril()
        t = t.masked_fill(~keep, float("-inf"))
        A = A * keep
    tmax = t.amax(-1, keepdim=True)
    pt = torch.exp2(t - tmax)
    L = pt.sum(-1, keepdim=True)
    p = pt / L
    o = p @ v
    log2l = torch.log2(L)
    lse = tmax + log2l
    m_abs = t.masked_fill(torch.isinf(t), 0.0).abs().amax(-1, keepdim=True) + 9.0
    t_abs = t.masked_fill(torch.isinf(t), 0.0).abs()
    dt = (DP + 2) * W * (A + m_abs) + (U * A if ones else 2 * W * (t_abs + m_abs))
    eps_arith = LN2 * dt + 2.0 ** -22
    eps = eps_arith + (U if ones else 0.0)
    eps_l = (p * eps).sum(-1, keepdim=True) + (Sk + 16) * W
    S = p @ v.abs()
    bound_o = (U * o.abs() + 2.0 ** -25 + (p * (eps_arith + U)) @ v.abs() + eps_l * o.abs() + (2 * Sk + 32) * W * S
               + 2.0 ** -24 * v.abs().sum(-2, keepdim=True))
    bound_lse = LOG2E * eps_l + 2 * W * (m_abs + log2l.abs()) + 2.0 ** -21 * (1 + log2l.abs())
    out = dict(o=o, lse=lse.squeeze(-1), bound_o=bound_o, bound_lse=bound_lse.squeeze(-1))
    if want_probs:
        out["p"] = p
        out["bound_p"] = p * (eps_arith + eps_l + 3 * 2.0 ** -22) + 2.0 ** -126
    return out


def bwd_reference(q, k, v, go, o16, lse32, scale, *, DP, sk_grad=None):
    """dict(gq, gk, gv, delta and their bounds) from the inputs as given — docstring B1 .. B7."""
    Sq, Sk, d = q.shape[-2], k.shape[-2], q.shape[-1]
    sl2 = scale * LOG2E
    t = (q @ k.transpose(-1, -2)) * sl2
    A = (q.abs() @ k.abs().transpose(-1, -2)) * sl2
    lse = lse32.unsqueeze(-1)
    Pm = torch.exp2(t - lse)
    dP = go @ v.transpose(-1, -2)
    delta = (go * o16).sum(-1, keepdim=True)
    dS = Pm * (dP - delta)
    gq = scale * (dS @ k)
    gk = scale * (dS.transpose(-1, -2) @ q)
    gv = Pm.transpose(-1, -2) @ go
    e_delta = (d + 6) * W * (go * o16).abs().sum(-1, keepdim=True)
    eps_p = LN2 * (DP * W * A + 2 * W * (t.abs() + lse.abs())) + 2.0 ** -22
    e_dp = (DP + 2) * W * (go.abs() @ v.abs().transpose(-1, -2))
    r_dS = Pm * (eps_p * (dP - delta).abs() + e_dp + e_delta) + (U + 3 * W) * dS.abs() + 2.0 ** -25
    r_P = Pm * (eps_p + U) + 2.0 ** -25
    bound_gq = U * gq.abs() + 2.0 ** -25 + scale * (r_dS @ k.abs() + (Sk + 16) * W * (dS.abs() @ k.abs())) + 2 * W * gq.abs()
    bound_gk = (U * gk.abs() + 2.0 ** -25 + scale * (r_dS.transpose(-1, -2) @ q.abs() + (Sq + 16) * W * (dS.abs().transpose(-1, -2) @ q.abs()))
                + 2 * W * gk.abs())
    bound_gv = U * gv.abs() + 2.0 ** -25 + r_P.transpose(-1, -2) @ go.abs() + (Sq + 16) * W * (Pm.transpose(-1, -2) @ go.abs())
    out = dict(gq=gq, gk=gk, gv=gv, delta=delta.squeeze(-1), bound_gq=bound_gq, bound_gk=bound_gk, bound_gv=bound_gv,
               bound_delta=(e_delta + W * delta.abs()).squeeze(-1))
    if sk_grad is not None:
        for n in ("gk", "gv", "bound_gk", "bound_gv"):
            out[n] = out[n][..., :sk_grad, :]
    return out


def xbwd_reference(q, k, v, go, gp, scale, *, DP, ds16=True):
    """dict(gq, bound_gq) of the cross-attention backward (go or gp may be None) — docstring X1 .. X4.  ds16: dS is rounded to
    fp16 (the MFMA kernel); the one-wave-per-row kernel keeps it in fp32."""
    Sk = k.shape[-2]
    sl2 = scale * LOG2E
    t = (q @ k.transpose(-1, -2)) * sl2
    A = (q.abs() @ k.abs().transpose(-1, -2)) * sl2
    tmax = t.amax(-1, keepdim=True)
    pt = torch.exp2(t - tmax)
    p = pt / pt.sum(-1, keepdim=True)
    dP = torch.zeros_like(t)
    dP_abs = torch.zeros_like(t)
    if go is not None:
        dP = dP + go @ v.transpose(-1, -2)
        dP_abs = dP_abs + go.abs() @ v.abs().transpose(-1, -2)
    if gp is not None:
        dP = dP + gp
        dP_abs = dP_abs + gp.abs()
    dot = (p * dP).sum(-1, keepdim=True)
    dS = scale * p * (dP - dot)
    gq = dS @ k
    eps0 = LN2 * (DP * W * A + 3 * W * (t.abs() + tmax.abs())) + 2.0 ** -22
    eps_l = (p * eps0).sum(-1, keepdim=True) + (Sk + 18) * W
    eps_p = eps0 + eps_l
    e_dp = (DP + 2) * W * dP_abs
    e_dot = (p * (eps_p * dP.abs() + e_dp)).sum(-1, keepdim=True) + (Sk + 16) * W * (p * dP.abs()).sum(-1, keepdim=True)
    r_dS = scale * p * (eps_p * (dP - dot).abs() + e_dp + e_dot) + 4 * W * dS.abs() + ((U * dS.abs() + 2.0 ** -25) if ds16 else 0.0)
    bound = U * gq.abs() + 2.0 ** -25 + r_dS @ k.abs() + (Sk + 16) * W * (dS.abs() @ k.abs())
    return dict(gq=gq, bound_gq=bound)


# ---------------------------------------------------------------------------------------------
# fp32 emulations with the documented rounding points (CPU suite: the bound is not too tight)
# ---------------------------------------------------------------------------------------------
def _r16(x):
    return x.to(H16).to(F32)


def fwd_emulation(q, k, v, scale, *, ones, causal=False):
    """fp32 arithmetic, fp16 roundings at F2 / F4 / F5 / F7; operands fp32 [N][S][d] holding fp16 values."""
    sl2 = torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    t = (_r16(q * sl2) @ k.transpose(-1, -2)) if ones else (q @ k.transpose(-1, -2)) * sl2
    if causal:
        t = t.masked_fill(~torch.ones(t.shape[-2:], dtype=torch.bool).tril(), float("-inf"))
    m = _r16(t.amax(-1, keepdim=True)) if ones else t.amax(-1, keepdim=True)
    pt = torch.exp2(t - m)
    pr = _r16(pt)
    l = (pr if ones else pt).sum(-1, keepdim=True)
    o = _r16((pr @ v) / l)
    return dict(o=o, lse=(m + torch.log2(l)).squeeze(-1), p=pt / pt.sum(-1, keepdim=True))


def bwd_emulation(q, k, v, go, o16, lse32, scale, *, sk_grad=None):
    sl2 = torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    sc = torch.tensor(scale, dtype=F32)
    Pm = torch.exp2((q @ k.transpose(-1, -2)) * sl2 - lse32.unsqueeze(-1))
    delta = (go * o16).sum(-1, keepdim=True)
    dS = _r16(Pm * (go @ v.transpose(-1, -2) - delta))
    out = dict(gq=_r16((dS @ k) * sc), gk=_r16((dS.transpose(-1, -2) @ q) * sc), gv=_r16(_r16(Pm).transpose(-1, -2) @ go),
               delta=delta.squeeze(-1))
    if sk_grad is not None:
        out["gk"], out["gv"] = out["gk"][..., :sk_grad, :], out["gv"][..., :sk_grad, :]
    return out


def xbwd_emulation(q, k, v, go, gp, scale, *, ds16=True):
    sc = torch.tensor(scale, dtype=F32)
    t = (q @ k.transpose(-1, -2)) * (sc * torch.tensor(LOG2E, dtype=F32))
    pt = torch.exp2(t - t.amax(-1, keepdim=True))
    p = pt / pt.sum(-1, keepdim=True)
    dP = torch.zeros_like(t)
    if go is not None:
        dP = dP + go @ v.transpose(-1, -2)
    if gp is not None:
        dP = dP + gp
    dS = p * (dP - (p * dP).sum(-1, keepdim=True)) * sc
    dS = _r16(dS) if ds16 else dS
    return dict(gq=_r16(dS @ k))


# ---------------------------------------------------------------------------------------------
# view forms
# ---------------------------------------------------------------------------------------------
def _bshd(t):
    """[B][H][S][d] -> [B][S][H*d]: head h at column offset h * d."""
    B, H, S, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, S, H * d)


class View:
    """One operand as the entry points take it: a carved buffer, an element offset into it, a row stride and a per-image
    stride; `cols` is the column block [c0, c0 + C) of the carved logical tensor that holds it and `rows` its row count."""

    def __init__(self, carved, off, ld, bs, c0, C, rows):
        self.carved, self.off, self.ld, self.bs, self.c0, self.C, self.rows = carved, off, ld, bs, c0, C, rows

    def ptr(self, buf=None):
        if self.carved.device is None:
            return P + 2 * self.off
        return (self.carved.buf if buf is None else buf)[GUARD + self.off:]

    @property
    def view(self):
        return (self.ld, self.bs)

    def logical(self, buf):
        """[B][rows][C] of `buf` (a clone of the carved buffer)."""
        return self.carved.logical(buf)[:, :self.rows, self.c0:self.c0 + self.C]


def _carve_in(parts, rows_total, ld, bs, device):
    """Input tensors [B][rows_i][C_i] side by side in one [B][rows_total][sum C_i] block (NaN below a shorter part), carved
    at row stride ld / image stride bs with NaN pads.  Returns the Views."""
    B = parts[0].shape[0]
    width = sum(p.shape[2] for p in parts)
    block = torch.full((B, rows_total, width), NAN, dtype=F64)
    c0 = 0
    for p in parts:
        block[:, :p.shape[1], c0:c0 + p.shape[2]] = p.to(F64)
        c0 += p.shape[2]
    cv = Carved(block, (bs, ld, 1), NAN, H16, device)
    views, c0 = [], 0
    for p in parts:
        views.append(View(cv, c0, ld, bs, c0, p.shape[2], p.shape[1]))
        c0 += p.shape[2]
    return views


def _carve_out(B, rows, widths, ld, bs, device, dtype=H16):
    sent = SENT16 if dtype == H16 else SENT32
    cv = Carved(torch.full((B, rows, sum(widths)), sent, dtype=F64), (bs, ld, 1), sent, dtype, device)
    views, c0 = [], 0
    for wd in widths:
        views.append(View(cv, c0, ld, bs, c0, wd, rows))
        c0 += wd
    return views


def _stat(B, H, Sq, values, device, fill):
    """fp32 [B][H][Sq] statistics buffer (contiguous: the entry points take no stride for it) with guards."""
    t = torch.full((B, H, Sq), fill, dtype=F64) if values is None else values.to(F64)
    return Carved(t, (H * Sq, Sq, 1), fill, F32, device)


class Views:
    pass


def views(row, form, data, device, *, o16=None, lse32=None):
    """The operands of `row` laid out as `form` asks.  Backward rows take the forward results (o16 [B][H][Sq][d] fp16
    values, lse32 [B][H][Sq]) as inputs."""
    r, B, H, Sq, Sk, C = row, row.B, row.H, row.Sq, row.Sk, row.C
    q, k, v = _bshd(data.q), _bshd(data.k), _bshd(data.v)
    vw = Views()
    vw.form, vw.pair, vw.tok, vw.cond_only, vw.sk_grad = form, 0, -1, False, row.sk_grad
    vw.use_go, vw.use_gp = True, True
    if form in ("pair_half", "pair_dup"):
        h = B // 2
        q, k, v = (torch.cat([t[:h], t[:h]]) for t in (q, k, v))
        vw.pair = ops.PAIR_HALF if form == "pair_half" else ops.PAIR_DUP
    wide = form in ("gaps", "fused3")                           # outputs at a wider row stride, images apart
    R3 = max(Sq, Sk)                                             # rows of a fused block (Sk in the engine: Sq <= Sk there)
    if form in ("fused3", "causal_fused"):                       # [B][R3][3C]: q (its first Sq rows) | k | v
        vw.q, vw.k, vw.v = _carve_in([q, k, v], R3, 3 * C, R3 * 3 * C, device)
    elif form == "kv2":                                          # k | v of one [B][T][2C] projection; q: images apart
        vw.q, = _carve_in([q], Sq, C, Sq * C + 64, device)
        vw.k, vw.v = _carve_in([k, v], Sk, 2 * C, Sk * 2 * C, device)
    elif form == "gaps":
        vw.q, = _carve_in([q], Sq, C + 8, Sq * (C + 8) + 40, device)
        vw.k, = _carve_in([k], Sk, C + 16, Sk * (C + 16) + 24, device)
        vw.v, = _carve_in([v], Sk, C + 24, Sk * (C + 24) + 8, device)
    elif form == "odd_ld":                                       # q / go / gq rows 2 elements apart from a multiple of 8
        vw.q, = _carve_in([q], Sq, C + 2, Sq * (C + 2) + 2, device)
        vw.k, = _carve_in([k], Sk, C, Sk * C, device)
        vw.v, = _carve_in([v], Sk, C, Sk * C, device)
    else:
        vw.q, = _carve_in([q], Sq, C, Sq * C, device)
        vw.k, = _carve_in([k], Sk, C, Sk * C, device)
        vw.v, = _carve_in([v], Sk, C, Sk * C, device)
    ldo, obs = (C + 8, Sq * (C + 8) + 24) if wide else (C, Sq * C)
    if r.op in ("self", "map"):
        vw.o, = _carve_out(B, Sq, [C], ldo, obs, device)
        vw.lse = _stat(B, H, Sq, None, device, SENT32) if r.op == "self" else None
        vw.probs = None
        if r.op == "map" and not r.causal:
            vw.tok = 5 % Sk if form == "tok" else -1
            vw.cond_only = form == "cond_only"
            Bp, Tp = (B // 2 if vw.cond_only else B), (1 if vw.tok >= 0 else Sk)
            vw.probs = Carved(torch.full((Bp, H, Sq, Tp), SENT32, dtype=F64), (H * Sq * Tp, Sq * Tp, Tp, 1), SENT32, F32, device)
        return vw
    go = _bshd(data.go)
    if r.op == "bwd":
        vw.sk_grad = Sk if form in ("contig", "gaps") else row.sk_grad
        o = _bshd(o16)
        if wide:
            vw.o, = _carve_in([o], Sq, C + 8, Sq * (C + 8) + 16, device)
            vw.go, = _carve_in([go], Sq, C + 16, Sq * (C + 16) + 8, device)
        else:
            vw.o, = _carve_in([o], Sq, C, Sq * C, device)
            vw.go, = _carve_in([go], Sq, C, Sq * C, device)
        vw.lse = _stat(B, H, Sq, lse32, device, NAN)
        vw.delta = _stat(B, H, Sq, None, device, SENT32)
        if form == "fused3":                                     # each gradient's neighbours are the other two gradients
            vw.gq, vw.gk, vw.gv = _carve_out(B, R3, [C, C, C], 3 * C, R3 * 3 * C, device)
            vw.gq.rows = Sq
        elif form == "gaps":
            vw.gq, = _carve_out(B, Sq, [C], C + 4, Sq * (C + 4) + 12, device)
            vw.gk, = _carve_out(B, Sk, [C], C + 8, Sk * (C + 8) + 4, device)
            vw.gv, = _carve_out(B, Sk, [C], C + 12, Sk * (C + 12) + 20, device)
        else:
            vw.gq, = _carve_out(B, Sq, [C], C, Sq * C, device)
            vw.gk, = _carve_out(B, Sk, [C], C, Sk * C, device)
            vw.gv, = _carve_out(B, Sk, [C], C, Sk * C, device)
        return vw
    # cross-attention backward
    vw.use_go, vw.use_gp = form != "no_go", form != "no_gp"
    if form == "odd_ld":
        vw.go, = _carve_in([go], Sq, C + 6, Sq * (C + 6) + 2, device)
        vw.gq, = _carve_out(B, Sq, [C], C + 2, Sq * (C + 2) + 6, device)
    elif form == "gaps":
        vw.go, = _carve_in([go], Sq, C + 16, Sq * (C + 16) + 8, device)
        vw.gq, = _carve_out(B, Sq, [C], C + 4, Sq * (C + 4) + 12, device)
    else:
        vw.go, = _carve_in([go], Sq, C, Sq * C, device)
        vw.gq, = _carve_out(B, Sq, [C], C, Sq * C, device)
    vw.gp = Carved(data.gp, (H * Sq * Sk, Sq * Sk, Sk, 1), NAN, F32, device)
    return vw


# ---------------------------------------------------------------------------------------------
# the rows: one per reachable variant code (and a few more for the edge shapes), smallest selecting shape
# ---------------------------------------------------------------------------------------------
# forward thresholds at Sq = 300: two query tiles per wave from 3 B H >= 1024 (B H = 344), which at the 8-wave-eligible head
# dims is 8 waves as well (2 B H = 688 >= 512); the wide d = 160 form from 5 B H > 256 (B H = 52).
# backward: wgs = (300 / 128) B H = 2 B H: two tiles per wave from B H = 256, 8 waves from B H = 512.
_W4OFF, _A32OFF, _A32ALL = {"attn_w4": 0}, {"attn32": 0}, {"attn32": 2}
_ROW_LIST = [
    # ---- attn_self_kernel: (mode, shape) per DP; d padded and exact
    Row(103210, "self", 2, 3, 24), Row(103211, "self", 2, 172, 8),
    Row(103200, "self", 2, 3, 32), Row(103201, "self", 2, 172, 32),
    Row(106420, "self", 2, 3, 40), Row(106422, "self", 2, 172, 40, opts=_W4OFF),
    Row(106420, "self", 2, 3, 40, Sk=1, note="one key"), Row(106420, "self", 3, 3, 40, Sq=48, Sk=77, note="one query tile, odd B"),
    Row(106410, "self", 2, 3, 56), Row(106411, "self", 2, 172, 56),
    Row(106400, "self", 2, 3, 64), Row(106401, "self", 2, 172, 64),
    Row(109610, "self", 2, 3, 80), Row(109612, "self", 2, 172, 88, opts=_A32OFF),
    Row(109600, "self", 2, 3, 96), Row(109602, "self", 2, 172, 96),
    Row(112810, "self", 2, 3, 104), Row(112800, "self", 2, 3, 128),
    Row(116010, "self", 2, 3, 136), Row(116000, "self", 2, 3, 160), Row(116002, "self", 2, 26, 160, note="wide form"),
    Row(119210, "self", 2, 3, 176), Row(119200, "self", 2, 3, 192, note="SAM global attention"),
    # ---- attn_self32_kernel ("attn32" = 2: for every problem size)
    Row(204800, "self", 2, 3, 40, opts=dict(_A32ALL, attn32_nw=4)), Row(204801, "self", 2, 3, 40, opts=_A32ALL),
    Row(204802, "self", 2, 3, 40, opts=dict(_A32ALL, attn32_var=1)), Row(204803, "self", 2, 3, 40, opts=dict(_A32ALL, attn32_var=2)),
    Row(209600, "self", 2, 3, 80, opts=dict(_A32ALL, attn32_nw=4)), Row(209601, "self", 2, 3, 88, opts=_A32ALL),
    Row(209602, "self", 2, 3, 80, opts=dict(_A32ALL, attn32_var=1)), Row(209603, "self", 2, 3, 88, opts=dict(_A32ALL, attn32_var=2)),
    Row(209601, "self", 2, 3, 80, Sk=77, opts=_A32ALL, note="77 keys"),
    # ---- attn_w4_kernel ("attn_w4" = 2)
    Row(306401, "self", 2, 3, 40, opts={"attn_w4": 2}), Row(306400, "self", 2, 3, 40, opts={"attn_w4": 2, "attn_w4_pipe": 0}),
    Row(306401, "self", 2, 3, 40, Sk=77, opts={"attn_w4": 2}, note="77 keys"),
    # ---- attn_fwd_kernel: map capture over the text tokens, and causal
    Row(403200, "map", 2, 3, 24, Sk=77), Row(406400, "map", 2, 3, 40, Sk=77), Row(406400, "map", 2, 3, 64, Sk=130, note="three key tiles"),
    Row(406400, "map", 2, 3, 40, Sk=1, note="one key"),
    Row(409600, "map", 2, 3, 80, Sk=77), Row(412800, "map", 2, 3, 104, Sk=77), Row(412800, "map", 2, 3, 128, Sk=77, note="exact d"),
    Row(416000, "map", 2, 3, 160, Sk=77), Row(416000, "map", 2, 3, 136, Sk=77, note="padded d"), Row(419200, "map", 2, 3, 192, Sk=77, note="exact d"),
    Row(403200, "map", 2, 3, 32, Sk=77, note="exact d"), Row(409600, "map", 2, 3, 96, Sk=77, note="exact d"),
    Row(419200, "map", 2, 3, 176, Sk=77),
    Row(406400, "map", 3, 4, 64, Sq=77, Sk=77, causal=True, note="causal"), Row(403200, "map", 2, 3, 32, Sq=150, Sk=150, causal=True, note="causal"),
    # ---- attn_bwd_dq / dkv kernels
    Row(503200, "bwd", 2, 3, 24), Row(503201, "bwd", 2, 128, 32),
    Row(506410, "bwd", 2, 3, 40), Row(506412, "bwd", 2, 128, 40), Row(506413, "bwd", 2, 256, 40),
    Row(506410, "bwd", 2, 3, 40, Sk=1, note="one key"), Row(506410, "bwd", 3, 3, 40, Sq=40, Sk=77, note="one query tile"),
    Row(506400, "bwd", 2, 3, 56), Row(506401, "bwd", 2, 128, 64),
    Row(509600, "bwd", 2, 3, 80), Row(509601, "bwd", 2, 128, 88),
    Row(512800, "bwd", 2, 3, 104), Row(512800, "bwd", 2, 3, 128, note="exact d"),
    Row(516000, "bwd", 2, 3, 136), Row(516000, "bwd", 2, 3, 160, note="exact d"),
    # ---- cross-attention backward
    Row(603200, "xbwd", 2, 3, 24, Sk=77), Row(606400, "xbwd", 2, 3, 40, Sk=77), Row(606400, "xbwd", 2, 3, 64, Sk=96, note="96 keys"),
    Row(606400, "xbwd", 2, 3, 40, Sk=1, note="one key"),
    Row(603200, "xbwd", 2, 3, 32, Sk=77, note="exact d"), Row(609600, "xbwd", 2, 3, 80, Sk=77), Row(609600, "xbwd", 2, 3, 96, Sk=77, note="exact d"),
    Row(612800, "xbwd", 2, 3, 128, Sk=77), Row(612800, "xbwd", 2, 3, 104, Sk=77, note="padded d"),
    Row(616000, "xbwd", 2, 3, 160, Sk=77), Row(616000, "xbwd", 2, 3, 136, Sk=77, note="padded d"),
    Row(700000, "xbwd", 2, 3, 40, Sk=100, note="97..128 keys"), Row(700000, "xbwd", 2, 3, 40, Sk=77, aligned=False, note="ld % 8 != 0"),
    Row(700000, "xbwd", 2, 3, 192, Sk=77, note="d > 160"),
]
ROWS_BY_NAME = {r.name: r for r in _ROW_LIST}
assert len(ROWS_BY_NAME) == len(_ROW_LIST)
CODES = sorted({r.code for r in _ROW_LIST})


def rows_of(code):
    return [r for r in _ROW_LIST if r.code == code]


# ---------------------------------------------------------------------------------------------
# host refusals: every row differs in ONE argument from a call the library accepts and is answered with a negative code
# before the device is touched (so the CPU suite asks the entry points themselves, with a NULL stream and placeholder
# pointers; the GPU suite passes addresses inside a sentinel buffer and checks that nothing was written)
# ---------------------------------------------------------------------------------------------
_RB, _RH, _RSQ, _RSK, _RD = 2, 2, 64, 80, 40
_RC = _RH * _RD
_ARGS = {      # argument names in ABI order; "p:" pointers take base + offset, the rest are numbers
    "lgd_attn_fwd_f16": "p:q ldq q_bs p:k ldk k_bs p:v ldv v_bs p:o ldo o_bs p:lse B H Sq Sk d scale",
    "lgd_attn_fwd_pair_f16": "p:q ldq q_bs p:k ldk k_bs p:v ldv v_bs p:o ldo o_bs p:lse B H Sq Sk d scale pair",
    "lgd_cross_attn_fwd_f16": "p:q ldq q_bs p:k ldk k_bs p:v ldv v_bs p:o ldo o_bs p:probs tok cond_only B H Sq Sk d scale",
    "lgd_attn_causal_fwd_f16": "p:q ldq q_bs p:k ldk k_bs p:v ldv v_bs p:o ldo o_bs B H Sq d scale",
    "lgd_attn_bwd_keys_f16": "p:q ldq q_bs p:k ldk k_bs p:v ldv v_bs p:o ldo o_bs p:go ldgo go_bs p:lse p:delta p:gq ldgq gq_bs "
                             "p:gk ldgk gk_bs p:gv ldgv gv_bs B H Sq Sk Sk_grad d scale",
    "lgd_cross_attn_bwd_f16": "p:q ldq q_bs p:k ldk k_bs p:v ldv v_bs p:go ldgo go_bs p:gp p:gq ldgq gq_bs B H Sq Sk d scale",
}
REFUSALS = [   # (entry point, what is wrong, {argument: value}); pointer values are byte offsets from an aligned base, None = NULL
    ("lgd_attn_fwd_f16", "ldq % 8", dict(ldq=_RC + 4)), ("lgd_attn_fwd_f16", "ldk % 8", dict(ldk=_RC + 2)),
    ("lgd_attn_fwd_f16", "ldv % 8", dict(ldv=_RC + 4)), ("lgd_attn_fwd_f16", "ldo % 4", dict(ldo=_RC + 2)),
    ("lgd_attn_fwd_f16", "d % 8", dict(d=36)), ("lgd_attn_fwd_f16", "d > 192", dict(d=200, ldq=400, ldk=400, ldv=400, ldo=400)),
    ("lgd_attn_fwd_f16", "q base 8-byte aligned", dict(q=8)), ("lgd_attn_fwd_f16", "k base 2-byte aligned", dict(k=2)),
    ("lgd_attn_fwd_f16", "v base 4-byte aligned", dict(v=4)), ("lgd_attn_fwd_f16", "o base 4-byte aligned", dict(o=4)),
    ("lgd_attn_fwd_f16", "q_bs % 8", dict(q_bs=_RSQ * _RC + 4)), ("lgd_attn_fwd_f16", "k_bs % 8", dict(k_bs=_RSK * _RC + 2)),
    ("lgd_attn_fwd_f16", "o_bs % 4", dict(o_bs=_RSQ * _RC + 2)), ("lgd_attn_fwd_f16", "Sk < 1", dict(Sk=0)),
    ("lgd_attn_fwd_pair_f16", "odd B", dict(B=3)), ("lgd_attn_fwd_pair_f16", "pair mode 3", dict(pair=3)),
    ("lgd_attn_fwd_pair_f16", "pair mode 0", dict(pair=0)), ("lgd_attn_fwd_pair_f16", "ldq % 8", dict(ldq=_RC + 4)),
    ("lgd_cross_attn_fwd_f16", "ldk % 8", dict(ldk=2 * _RC + 4)), ("lgd_cross_attn_fwd_f16", "d % 8", dict(d=44)),
    ("lgd_cross_attn_fwd_f16", "d > 192", dict(d=200, ldq=400, ldk=400, ldv=400, ldo=400)), ("lgd_cross_attn_fwd_f16", "tok >= Sk", dict(tok=_RSK)),
    ("lgd_cross_attn_fwd_f16", "cond_only with odd B", dict(B=3, cond_only=1)), ("lgd_cross_attn_fwd_f16", "k base 8-byte aligned", dict(k=8)),
    ("lgd_attn_causal_fwd_f16", "ldq % 8", dict(ldq=3 * _RC + 4)), ("lgd_attn_causal_fwd_f16", "d % 8", dict(d=20)),
    ("lgd_attn_causal_fwd_f16", "q base 2-byte aligned", dict(q=2)),
    ("lgd_attn_bwd_keys_f16", "ldq % 8", dict(ldq=_RC + 4)), ("lgd_attn_bwd_keys_f16", "ldo % 8", dict(ldo=_RC + 4)),
    ("lgd_attn_bwd_keys_f16", "ldgo % 8", dict(ldgo=_RC + 4)), ("lgd_attn_bwd_keys_f16", "ldgq % 4", dict(ldgq=_RC + 2)),
    ("lgd_attn_bwd_keys_f16", "ldgk % 4", dict(ldgk=_RC + 2)), ("lgd_attn_bwd_keys_f16", "ldgv % 4", dict(ldgv=_RC + 2)),
    ("lgd_attn_bwd_keys_f16", "d % 8", dict(d=36)), ("lgd_attn_bwd_keys_f16", "d > 160", dict(d=168, **{n: 336 for n in ("ldq", "ldk", "ldv", "ldo", "ldgo", "ldgq", "ldgk", "ldgv")})),
    ("lgd_attn_bwd_keys_f16", "Sk_grad > Sk", dict(Sk_grad=_RSK + 1)), ("lgd_attn_bwd_keys_f16", "Sk_grad < 1", dict(Sk_grad=0)),
    ("lgd_attn_bwd_keys_f16", "NULL lse", dict(lse=None)), ("lgd_attn_bwd_keys_f16", "NULL delta", dict(delta=None)),
    ("lgd_attn_bwd_keys_f16", "go base 8-byte aligned", dict(go=8)), ("lgd_attn_bwd_keys_f16", "o base 2-byte aligned", dict(o=2)),
    ("lgd_attn_bwd_keys_f16", "gk base 4-byte aligned", dict(gk=4)), ("lgd_attn_bwd_keys_f16", "q_bs % 8", dict(q_bs=_RSQ * _RC + 4)),
    ("lgd_attn_bwd_keys_f16", "gq_bs % 4", dict(gq_bs=_RSQ * _RC + 2)), ("lgd_attn_bwd_keys_f16", "gv_bs % 4", dict(gv_bs=_RSK * _RC + 2)),
    ("lgd_cross_attn_bwd_f16", "ldk % 8", dict(ldk=2 * _RC + 4)), ("lgd_cross_attn_bwd_f16", "ldv % 8", dict(ldv=2 * _RC + 4)),
    ("lgd_cross_attn_bwd_f16", "d % 8", dict(d=36)), ("lgd_cross_attn_bwd_f16", "d > 192", dict(d=200)),
    ("lgd_cross_attn_bwd_f16", "Sk > 128", dict(Sk=129)), ("lgd_cross_attn_bwd_f16", "k base 8-byte aligned", dict(k=8)),
    ("lgd_cross_attn_bwd_f16", "v_bs % 8", dict(v_bs=_RSK * 2 * _RC + 4)), ("lgd_cross_attn_bwd_f16", "NULL gq", dict(gq=None)),
]


def refusal_args(fn, change, base):
    """The ctypes argument list of REFUSALS row (fn, .., change): an accepted call of that entry point with `change` applied
    and a NULL stream.  Operands sit 1 MiB apart from `base` (an address aligned to 16 bytes)."""
    import ctypes
    cross = fn.startswith("lgd_cross")
    kv_ld = 2 * _RC if cross else _RC
    fused = fn == "lgd_attn_causal_fwd_f16"
    vals = dict(B=_RB, H=_RH, Sq=_RSQ, Sk=_RSK, Sk_grad=_RSK, d=_RD, scale=0.125, pair=1, tok=-1, cond_only=0,
                ldq=3 * _RC if fused else _RC, q_bs=_RSQ * (3 * _RC if fused else _RC),
                ldk=3 * _RC if fused else kv_ld, k_bs=_RSQ * 3 * _RC if fused else _RSK * kv_ld,
                ldv=3 * _RC if fused else kv_ld, v_bs=_RSQ * 3 * _RC if fused else _RSK * kv_ld,
                ldo=_RC, o_bs=_RSQ * _RC, ldgo=_RC, go_bs=_RSQ * _RC, ldgq=_RC, gq_bs=_RSQ * _RC,
                ldgk=_RC, gk_bs=_RSK * _RC, ldgv=_RC, gv_bs=_RSK * _RC)
    names = _ARGS[fn].split()
    ptrs = [n[2:] for n in names if n.startswith("p:")]
    for i, n in enumerate(ptrs):
        vals[n] = 0
    vals.update(change)
    out = []
    for n in names:
        if n.startswith("p:"):
            v = vals[n[2:]]
            out.append(ctypes.c_void_p(None if v is None else base + (ptrs.index(n[2:]) << 20) + v))
        else:
            out.append(vals[n])
    return out + [ctypes.c_void_p(None)]
