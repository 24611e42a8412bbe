"""lgd_attn_wide_f16 (csrc/attn_wide.hip) as test data: shapes, data passes, view forms, the fp32 emulation of the kernel's
rounding points, the "hot" operands and the refusal table (test_attn_wide_cpu.py, test_attn_wide_gpu.py).

The reference and the bound are attn_conformance_cases.fwd_reference(..., DP = padded width, ones = False): F1, F3 - F7 of
that module's docstring.  Read against the kernel:
  F1  Q K^T accumulates in fp32 over DP products; the running max is EXACT per 32-key tile (it does not lag), so |m| <=
      max |t| holds with room to the bound's max |t| + 9;
  F2  does not apply: scale log2(e) multiplies the fp32 logit (2 w (|t| + |m|));
  F3  v_exp_f32;  F4  P rounded to fp16 for P V;  F5  the row sum is taken from the fp32 p, per lane and tile, and the four
      lanes of a query are added at the end: fewer than Sk + 16 additions;
  F6  P V accumulates in fp32 and is multiplied by exp2(m_old - m_new) at most once per tile of 32 keys: Sk / 32 + 1
      multiplications, inside the bound's (2 Sk + 32) w S;
  F7  one fp16 rounding of O.
The kernel adds NO rounding point to that list (no key split, no combine), so the bound has no extra term.

Data passes are attn_conformance_cases.Data with H = 1 ("heads": N(0, 1); "spiked": among the spiked keys the last one and
one in the ragged tail tile; "voffset").  The "hot" operands put one logit per query row above the fp16 range."""
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_conformance_cases as acc  # noqa: E402

H16, F32, F64 = torch.float16, torch.float32, torch.float64
KT = 32                                  # keys per tile of the kernel
PASSES = acc.PASSES
FORMS = ("packed", "qk_halves", "gaps")


def dp_of(d):
    """The padded width the launcher instantiates for d: its only dispatch thresholds."""
    return 64 if d <= 64 else 128 if d <= 128 else 256 if d <= 256 else 512


class Case:
    def __init__(self, B, Sq, Sk, d, note=""):
        self.B, self.Sq, self.Sk, self.d, self.note = B, Sq, Sk, d, note
        self.H, self.causal, self.op = 1, False, "self"          # what acc.Data reads of a row
        self.scale = d ** -0.5
        self.DP = dp_of(d)
        self.name = f"wide:B{B}S{Sq}x{Sk}d{d}"

    def data(self, pass_name):
        return acc.Data(self, pass_name)


# d: the test nets' width, a width that is only % 8, SD's; (Sq, Sk): one element, one ragged tile (40 = 32 + 8), ten tiles
# and a ragged tail with five query blocks of 64 and a 44-row tail; B 1 and 3
CASES = [Case(B, Sq, Sk, d) for d in (64, 72, 512) for Sq, Sk in ((1, 1), (40, 40), (300, 330)) for B in (1, 3)]
# both sides of every dispatch threshold of the launcher (DP 64 | 128 | 256 | 512; d = 64 | 72 are above)
CASES += [Case(1, 300, 330, d, "DP threshold") for d in (128, 136, 256, 264)]
CASES += [Case(1, 40, 40, 8, "smallest d")]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FULL = Case(1, 4096, 4096, 512, "the real mid-block shape")      # GPU only: about 34 GFLOP


def _r16(x):
    return x.to(H16).to(F32)


def emulation(q, k, v, scale, *, drop_last=False, pad_key=False, no_scale=False):
    """fp32 arithmetic with the kernel's rounding points and its order: keys in tiles of 32, an exact running max per tile,
    the accumulator and the row sum multiplied by exp2(m_old - m_new), P rounded to fp16 for P V only, one rounding of O.
    Operands fp32 [N][S][d] holding fp16 values.  The three switches build the wrong answers the bound must catch."""
    if drop_last:
        k, v = k[:, :-1], v[:, :-1]
    if pad_key:
        z = torch.zeros_like(k[:, :1])
        k, v = torch.cat([k, z], 1), torch.cat([v, z], 1)
    sl2 = torch.tensor(1.0 if no_scale else scale, dtype=F32) * torch.tensor(acc.LOG2E, dtype=F32)
    t = (q @ k.transpose(-1, -2)) * sl2
    N, Sq, Sk = t.shape
    m = torch.full((N, Sq, 1), -1.0e30, dtype=F32)
    l = torch.zeros((N, Sq, 1), dtype=F32)
    o = torch.zeros((N, Sq, v.shape[-1]), dtype=F32)
    for j in range(0, Sk, KT):
        tt = t[..., j:j + KT]
        m_new = torch.maximum(m, tt.amax(-1, keepdim=True))
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(tt - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + _r16(p) @ v[:, j:j + KT]
        m = m_new
    return _r16(o / l)


def reference(case, q, k, v, scale=None):
    """fwd_reference over fp64 [N][S][d], in blocks of query rows (rows are independent; 32 MiB per fp64 temporary)."""
    step = max(1, (1 << 22) // max(1, q.shape[0] * k.shape[1]))
    outs = [acc.fwd_reference(q[:, i:i + step], k, v, case.scale if scale is None else scale, DP=case.DP, ones=False)
            for i in range(0, q.shape[1], step)]
    return {n: torch.cat([o[n] for o in outs], dim=1) for n in ("o", "bound_o")}


def ratio(got, ref):
    return float(((got.to(F64) - ref["o"]).abs() / ref["bound_o"]).max())


# ---------------------------------------------------------------------------------------------
# view forms
# ---------------------------------------------------------------------------------------------
def views(case, form, data, device):
    """q, k, v, o as attn_conformance_cases.View: "packed" contiguous [B][S][d]; "qk_halves" q and k the halves of one
    [B][max(Sq, Sk)][2 d] buffer with v apart (what vae._Blocks._attn passes); "gaps" wider rows and images apart, with NaN
    in everything the strides skip.  Guards around every buffer, sentinels in every output element."""
    B, Sq, Sk, d = case.B, case.Sq, case.Sk, case.d
    q, k, v = (t[:, 0] for t in (data.q, data.k, data.v))        # [B][S][d]
    vw = types.SimpleNamespace(form=form)
    if form == "qk_halves":
        R = max(Sq, Sk)
        vw.q, vw.k = acc._carve_in([q, k], R, 2 * d, R * 2 * d, device)
        vw.v, = acc._carve_in([v], Sk, d, Sk * d, device)
    elif form == "gaps":
        vw.q, = acc._carve_in([q], Sq, d + 8, Sq * (d + 8) + 40, device)
        vw.k, = acc._carve_in([k], Sk, d + 16, Sk * (d + 16) + 24, device)
        vw.v, = acc._carve_in([v], Sk, d + 24, Sk * (d + 24) + 8, device)
    else:
        vw.q, = acc._carve_in([q], Sq, d, Sq * d, device)
        vw.k, = acc._carve_in([k], Sk, d, Sk * d, device)
        vw.v, = acc._carve_in([v], Sk, d, Sk * d, device)
    ldo, obs = (d + 8, Sq * (d + 8) + 24) if form == "gaps" else (d, Sq * d)
    vw.o, = acc._carve_out(B, Sq, [d], ldo, obs, device)
    return vw


# ---------------------------------------------------------------------------------------------
# the "hot" operands: one logit per row above the fp16 range
# ---------------------------------------------------------------------------------------------
HOT_S, HOT_D, HOT_GAIN, HOT_NORM = 200, 64, 70.0, 32.0


def hot_target(i):
    return (7 * i + 3) % HOT_S                                   # injective: gcd(7, 200) = 1


def hot_operands():
    """q [S][d] rows of norm 32, k[j(i)] = 70 q[i], v N(0, 1); fp16 values.  With scale = 1 (what the VAE passes: its
    weights carry the scale) the target logit is 70 * 32^2 = 71680 > 65504 and every other logit of the row 70 q_i.q_i',
    about half of it at most."""
    g = torch.Generator().manual_seed(4242)
    q = torch.randn(HOT_S, HOT_D, generator=g)
    q = (q / q.norm(dim=1, keepdim=True) * HOT_NORM).to(H16)
    k = torch.empty_like(q)
    k[[hot_target(i) for i in range(HOT_S)]] = (q.float() * HOT_GAIN).to(H16)
    v = torch.randn(HOT_S, HOT_D, generator=g).to(H16)
    return q, k, v


# ---------------------------------------------------------------------------------------------
# refusals: one argument away from a call the library accepts
# ---------------------------------------------------------------------------------------------
_RB, _RSQ, _RSK, _RD = 2, 64, 80, 64
ARGS = "p:q p:k p:v p:o B Sq Sk d ldq ldk ldv ldo bsq bsk bsv bso scale"
_WIDE = dict(d=520, ldq=520, ldk=520, ldv=520, ldo=520, bsq=_RSQ * 520, bsk=_RSK * 520, bsv=_RSK * 520, bso=_RSQ * 520)
REFUSALS = [       # (what is wrong, {argument: value}, code); pointer values are byte offsets from their operand's slot, None = NULL
    ("NULL q", dict(q=None), -1), ("NULL k", dict(k=None), -1), ("NULL v", dict(v=None), -1), ("NULL o", dict(o=None), -1),
    ("B < 1", dict(B=0), -1), ("Sq < 1", dict(Sq=0), -1), ("Sk < 1", dict(Sk=0), -1), ("Sk negative", dict(Sk=-5), -1),
    ("d < 8", dict(d=0), -1), ("d = 4", dict(d=4), -1), ("d % 8", dict(d=36), -1),
    ("q base 8-byte aligned", dict(q=8), -1), ("k base 2-byte aligned", dict(k=2), -1), ("v base 4-byte aligned", dict(v=4), -1),
    ("o base 4-byte aligned", dict(o=4), -1),
    ("ldq % 8", dict(ldq=_RD + 4), -1), ("ldk % 8", dict(ldk=_RD + 2), -1), ("ldv % 8", dict(ldv=_RD + 4), -1), ("ldo % 4", dict(ldo=_RD + 2), -1),
    ("bsq % 8", dict(bsq=_RSQ * _RD + 4), -1), ("bsk % 8", dict(bsk=_RSK * _RD + 2), -1), ("bsv % 8", dict(bsv=_RSK * _RD + 4), -1),
    ("bso % 4", dict(bso=_RSQ * _RD + 2), -1),
    ("ldq < d", dict(ldq=_RD - 8), -1), ("ldk < d", dict(ldk=_RD - 8), -1), ("ldv < d", dict(ldv=_RD - 8), -1), ("ldo < d", dict(ldo=_RD - 4), -1),
    ("o is q", dict(o="q"), -1), ("o is k", dict(o="k"), -1), ("o is v", dict(o="v"), -1),
    ("o starts in the last row of q", dict(o=("q", 2 * ((_RB * _RSQ - 1) * _RD + 8))), -1),
    ("o ends in the first row of v", dict(o=("v", -2 * (_RB * _RSQ * _RD - 8))), -1),
    ("images of o overlap", dict(bso=_RD), -1),
    ("d > 512", _WIDE, -3),
]


def refusal_args(change, base):
    """The ctypes argument list of an accepted call (B = 2, Sq = 64, Sk = 80, d = 64, packed operands 1 MiB apart from
    `base`, an address aligned to 16 bytes, NULL stream) with `change` applied."""
    import ctypes
    vals = dict(B=_RB, Sq=_RSQ, Sk=_RSK, d=_RD, ldq=_RD, ldk=_RD, ldv=_RD, ldo=_RD, bsq=_RSQ * _RD, bsk=_RSK * _RD, bsv=_RSK * _RD,
                bso=_RSQ * _RD, scale=0.125, q=0, k=0, v=0, o=0)
    vals.update(change)
    slot = {n: base + (i << 20) for i, n in enumerate("qkvo")}
    out = []
    for n in ARGS.split():
        if n.startswith("p:"):
            x = vals[n[2:]]
            if isinstance(x, str):
                x = (x, 0)
            addr = None if x is None else slot[x[0]] + x[1] if isinstance(x, tuple) else slot[n[2:]] + x
            out.append(ctypes.c_void_p(addr))
        else:
            out.append(vals[n])
    return out + [ctypes.c_void_p(None)]
