"""The GEMM launch contract as test data: every descriptor form lgd_gemm_f16 is asked to serve, for every tile code.

A FORM is a named descriptor shape (strides, epilogue, gather, batching, split-K, CFG pair).  `FORMS[name].case(mode,
device)` holds its tensors — every operand carved out of a larger buffer, guard elements before and after and pad columns
where a row stride is wider than the data — the fp64 reference and the derived error bound; `case.desc(tile, out)`
builds the LgdGemmDesc.  With `device=None` the operands live on the host and the descriptor carries placeholder
addresses: lgd_gemm_check only looks at NULL-ness and alignment, so the acceptance matrix needs no GPU.

Two data modes:
  "exact"  A and W in {-1, 0, 1}, integer biases / residuals, alpha 0.5 or 1, row statistics in {-1, 0, 1} x {0.5, 1, 2}:
           every product, every partial sum in any order and the final value are exactly representable, so the output
           must equal the fp64 reference bit for bit (GEGLU forms have no exact mode);
  "round"  N(0, 1) activations, weights scaled by K^-0.5; the per-element bound is derived below (Case.bound), not measured.

The reference never touches the strided buffers: it is computed from the logical operands (explicit index arithmetic
for the 3x3 gather, the two-source concat, the batch and the GEGLU packing), then one fp64 matmul.

ACCEPTANCE pins what lgd_gemm_check answers for every (form, code) cell; a launch-contract change is a diff of it.
"""
import functools
import math

import torch

import __graft_entry__
from lgd_amd import ops

__graft_entry__.build()         # TILES below is read from the library's tile table

P = 1 << 20                     # an aligned placeholder address: descriptors are only checked with it
GUARD = 4096                    # guard elements in front of and behind every carved operand
H16, F32, F64 = torch.float16, torch.float32, torch.float64
SENT16 = 23456.0                # output sentinels: finite, exactly representable, far from any result of these cases
SENT32 = 3.0e33
TILES = sorted(ops.TILE_NAMES)
M0, N0, NG = 300, 328, 352      # two row tiles at bm = 256 with a ragged tail (ten at bm = 32); an 8-column last tile at
                                # bn = 320; N = 352 = 11 GEGLU blocks of [16 value | 16 gate]


def _flat_index(shape, strides):
    idx = torch.zeros(shape, dtype=torch.long)
    for dim, (n, s) in enumerate(zip(shape, strides)):
        view = [1] * len(shape)
        view[dim] = n
        idx = idx + (torch.arange(n, dtype=torch.long) * s).view(view)
    return idx


class Carved:
    """A logical tensor placed at `strides` inside a flat buffer: GUARD elements of `fill` in front and behind, and
    `fill` in every element between that the strides skip (pad columns, gaps between batches)."""

    def __init__(self, values, strides, fill, dtype, device):
        self.idx = _flat_index(values.shape, strides) + GUARD
        span = (int(self.idx.max()) - GUARD + 1 + 7) // 8 * 8
        host = torch.full((GUARD + span + GUARD,), fill, dtype=dtype)
        host[self.idx.reshape(-1)] = values.to(dtype).reshape(-1)
        self.host = host
        self.device = device
        self.buf = host.to(device) if device is not None else host
        self.idx_dev = self.idx.to(device) if device is not None else self.idx
        written = torch.zeros(host.numel(), dtype=torch.bool)
        written[self.idx.reshape(-1)] = True
        self.outside = (~written).to(device) if device is not None else ~written      # guards and pads

    def ptr(self, buf=None):
        """The operand's base address (element GUARD of the buffer), or the placeholder on a host without a GPU."""
        if self.device is None:
            return P
        return (self.buf if buf is None else buf)[GUARD:]

    def fresh(self):
        return self.buf.clone()

    def logical(self, buf):
        return buf[self.idx_dev]

    def outside_untouched(self, buf):
        """Guards and pads of `buf` still hold the bytes this operand was carved with."""
        bits = {2: torch.int16, 4: torch.int32}[buf.element_size()]
        return torch.equal(buf.view(bits)[self.outside], self.buf.view(bits)[self.outside])


class Form:
    def __init__(self, name, M=M0, N=N0, K=192, *, conv=None, c0=None, c1=0, bias=True, bias2=False, res=None,
                 alpha=1.0, geglu=False, out_f32=False, rownorm=False, lda0=None, lda1=None, ldw=None, ldc=None,
                 ldr=None, batched=False, splits=1, pair=0, base=None):
        # conv = (B, hin, win, hout, wout, stride, ups); res in (None, "f16", "f32", "inplace")
        self.name, self.M, self.N, self.K = name, M, N, K
        self.conv, self.taps = conv, (9 if conv else 1)
        self.cin = K // self.taps
        self.c1 = c1
        self.c0 = self.cin - c1 if c0 is None else c0
        self.bias, self.bias2, self.res, self.alpha = bias, bias2, res, alpha
        self.geglu, self.out_f32, self.rownorm = geglu, out_f32, rownorm
        self.n_out = N // 2 if geglu else N
        self.lda0 = self.c0 if lda0 is None else lda0
        self.lda1 = self.c1 if lda1 is None else lda1
        self.ldw = K if ldw is None else ldw
        self.ldc = self.n_out if ldc is None else ldc
        self.ldr = (self.ldc if res == "inplace" else self.n_out) if ldr is None else ldr
        self.batched, self.splits, self.pair, self.base = batched, splits, pair, base
        self.nb = (2, 3) if batched else (1, 1)
        self.exact = not geglu
        self.seed = 0

    @property
    def modes(self):
        return ("exact", "round") if self.exact else ("round",)

    def case(self, mode, device=None):
        return _case(self.name, mode, None if device is None else str(device))

    def accepts(self, tile):
        """(accepted, accepted with in-launch split-K counters) by lgd_gemm_check; host only."""
        c = self.case(self.modes[0])
        d = c.desc(tile)
        ok = ops.gemm_accepts(d)
        ok_cnt = ok
        if self.splits > 1:
            d.cnt = P
            ok_cnt = ops.gemm_accepts(d)
        return ok, ok_cnt


@functools.lru_cache(maxsize=None)
def _case(name, mode, device):
    return Case(FORMS[name], mode, None if device is None else torch.device(device))


def _gather3x3(x, B, hin, win, hout, wout, stride, ups):
    """A(m, k) of the 3x3 gather, from the definition in include/lgd_hip.h: x [B * hin * win][C] is the stored map; the
    LOGICAL input is x itself, its nearest-2x upsampling (ups = 1) or the zero-inserted map with data at even coordinates
    (ups = 2); output pixel (oy, ox) reads logical pixel (oy * stride + ky - 1, ox * stride + kx - 1), zero outside."""
    C = x.shape[1]
    x = x.reshape(B, hin, win, C)
    if ups == 0:
        hl, wl, logical = hin, win, x
    else:
        hl, wl = 2 * hin, 2 * win
        logical = torch.zeros(B, hl, wl, C, dtype=x.dtype)
        for iy in range(hl):
            for ix in range(wl):
                if ups == 1 or (iy % 2 == 0 and ix % 2 == 0):
                    logical[:, iy, ix] = x[:, iy // 2, ix // 2]
    assert hout == (hl - 1) // stride + 1 and wout == (wl - 1) // stride + 1
    A = torch.zeros(B, hout, wout, 9, C, dtype=x.dtype)
    for oy in range(hout):
        for ox in range(wout):
            for ky in range(3):
                for kx in range(3):
                    iy, ix = oy * stride + ky - 1, ox * stride + kx - 1
                    if 0 <= iy < hl and 0 <= ix < wl:
                        A[:, oy, ox, ky * 3 + kx] = logical[:, iy, ix]
    return A.reshape(B * hout * wout, 9 * C)


def _gelu(g):
    return 0.5 * g * (1.0 + torch.erf(g / math.sqrt(2.0)))


class Case:
    def __init__(self, f, mode, device):
        self.form, self.mode, self.device = f, mode, device
        g = torch.Generator().manual_seed(1000 + f.seed)
        exact = mode == "exact"
        nb_o, nb_i = f.nb
        M, N, K = f.M, f.N, f.K
        # alpha 0.5 keeps half-integers exact up to 1024; the longest contractions (K > 448) take 1
        self.alpha = f.alpha if not (exact and K > 448) else 1.0

        def draw(shape, scale=1.0, lo=-1, hi=1, dtype=H16):
            if exact:
                return torch.randint(lo, hi + 1, shape, generator=g).to(F64)
            return (torch.randn(shape, generator=g) * scale).to(dtype).to(F64)

        def dup_rows(t):                       # CFG pair: the two halves of the rows (images) are identical
            if f.pair or f.base:
                h = t.shape[-2] // 2
                t[..., h:, :] = t[..., :h, :]
            return t

        # ---- A: stored source rows [nb_i][rows][c] (the outer batch stride of A is 0: both outer batches read the same rows)
        rows = f.conv[0] * f.conv[1] * f.conv[2] if f.conv else M
        a0 = dup_rows(draw((1, nb_i, rows, f.c0)))
        a1 = dup_rows(draw((1, nb_i, rows, f.c1))) if f.c1 else None
        w = draw((nb_o, nb_i, N, K), scale=K ** -0.5)
        a_bs = (0, rows * f.lda0 + 64) if f.batched else (0, 0)
        w_bs = (nb_i * N * f.ldw + 128, N * f.ldw) if f.batched else (0, 0)
        nan = float("nan")
        self.a0 = Carved(a0, (a_bs[0], a_bs[1], f.lda0, 1), nan, H16, device)
        # both sources are addressed with the batch offset of a0
        self.a1 = Carved(a1, (a_bs[0], a_bs[1], f.lda1, 1), nan, H16, device) if f.c1 else None
        self.w = Carved(w, (w_bs[0], w_bs[1], f.ldw, 1), nan, H16, device)
        self.a_bs, self.w_bs = a_bs, w_bs

        # ---- logical A(m, k): the gather of each source, then the channel concat inside every tap
        def logical_a(b_i):
            srcs = [a0[0, b_i]] + ([a1[0, b_i]] if f.c1 else [])
            if f.conv:
                srcs = [_gather3x3(s, *f.conv).reshape(M, 9, -1) for s in srcs]
                return torch.cat(srcs, dim=2).reshape(M, K)
            return torch.cat(srcs, dim=1)
        A = torch.stack([logical_a(b_i) for b_i in range(nb_i)])[None].expand(nb_o, nb_i, M, K)
        acc = A @ w.transpose(-1, -2)                                          # [nb_o][nb_i][M][N]
        s_acc = A.abs() @ w.abs().transpose(-1, -2)                            # sum of |products|
        v, s = acc, s_acc

        # ---- epilogue, in the header's order: rownorm, biases, GEGLU, alpha, residual
        self.rowstat = self.colsum = None
        if f.rownorm:
            if exact:
                mean = torch.randint(-1, 2, (M, 1), generator=g).to(F64)
                rstd = torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, (M, 1), generator=g)]
                colsum = torch.randint(-3, 4, (N,), generator=g).to(F64)
            else:
                mean = (torch.randn((M, 1), generator=g) * 0.5).to(F32).to(F64)
                rstd = (0.5 + 1.5 * torch.rand((M, 1), generator=g)).to(F32).to(F64)
                colsum = torch.randn((N,), generator=g).to(F32).to(F64)
            stat = dup_rows(torch.cat([mean, rstd], dim=1))
            mean, rstd = stat[:, 0:1], stat[:, 1:2]
            self.rowstat = Carved(stat, (2, 1), nan, F32, device)
            self.colsum = Carved(colsum, (1,), nan, F32, device)
            v = rstd * (v - mean * colsum)
            s = rstd.abs() * (s + (mean * colsum).abs())
        self.b1 = self.b2 = None
        for which in ("bias", "bias2"):
            if getattr(f, which):
                b = draw((N,), lo=-4, hi=4, dtype=F32)
                c = Carved(b, (1,), nan, F32, device)
                if which == "bias":
                    self.b1 = c
                else:
                    self.b2 = c
                v, s = v + b, s + b.abs()
        e32 = (K + 8) * 2.0 ** -23 * s           # fp32 accumulation, every operation allowed to truncate
        if f.geglu:
            j = torch.arange(N // 2)
            vi = (j // 16) * 32 + j % 16                                       # [16 value | 16 gate] column blocks
            val, gate, ev, eg = v[..., vi], v[..., vi + 16], e32[..., vi], e32[..., vi + 16]
            gl = _gelu(gate)
            # |gelu'| <= 1.13; erf of common.h: Abramowitz-Stegun 7.1.26, |eps| <= 1.5e-7, plus one ulp of its reciprocal;
            # gelu = 0.5 g (1 + erf): two multiplies and an add on top
            e_gelu = 1.13 * eg + 0.5 * gate.abs() * (1.5e-7 + 2.0 ** -23) + 3 * 2.0 ** -24 * gl.abs()
            v = val * gl
            e32 = ev * gl.abs() + val.abs() * e_gelu + ev * e_gelu + 2.0 ** -24 * v.abs()
        v, e32 = v * self.alpha, e32 * abs(self.alpha)
        n_out = f.n_out
        self.res = None
        c_bs = (nb_i * (M * f.ldc + 40) + 16, M * f.ldc + 40) if f.batched else (0, 0)
        r_bs = (nb_i * (M * f.ldr + 24) + 48, M * f.ldr + 24) if f.batched else (0, 0)
        self.c_bs, self.r_bs = c_bs, r_bs
        out_dtype = F32 if f.out_f32 else H16
        sentinel = SENT32 if f.out_f32 else SENT16
        if f.res:
            rdt = F32 if f.res == "f32" else H16
            r = dup_rows(draw((nb_o, nb_i, M, n_out), lo=-8, hi=8, dtype=rdt))
            if f.res == "inplace":               # C holds the residual on entry; its pads hold the sentinel
                self.c = Carved(r, (c_bs[0], c_bs[1], f.ldc, 1), sentinel, out_dtype, device)
            else:
                self.res = Carved(r, (r_bs[0], r_bs[1], f.ldr, 1), nan, rdt, device)
            v, e32 = v + r, e32 + (K + 8) * 2.0 ** -23 * r.abs()
        if f.res != "inplace":
            self.c = Carved(torch.full((nb_o, nb_i, M, n_out), sentinel, dtype=F64), (c_bs[0], c_bs[1], f.ldc, 1),
                            sentinel, out_dtype, device)
        self.ws = None
        if f.splits > 1:                         # fp32 [batch][splits][M][N]; NaN until a split writes its partial
            self.ws = Carved(torch.full((nb_o * nb_i * f.splits * M * N,), nan, dtype=F64), (1,), SENT32, F32, device)
        self.ref = v                                                            # fp64 [nb_o][nb_i][M][n_out]
        self.s_max = float(s.max())
        # |y - ref| per element: fp16 rounding of the value (half an ulp, or half the smallest subnormal) on top of the
        # fp32 accumulation error; fp32 outputs round once more in fp32
        self.bound = (2.0 ** -24 * v.abs() + e32) if f.out_f32 else (2.0 ** -11 * v.abs() + 2.0 ** -25 + e32)
        if device is not None:
            self.ref, self.bound = self.ref.to(device), self.bound.to(device)

    def rounded_ref(self):
        """The reference rounded to the output type (exact forms: equal to the reference itself)."""
        return self.ref.to(F32 if self.form.out_f32 else H16).to(F64)

    def fresh_out(self):
        return self.c.fresh()

    def fresh_ws(self):
        return self.ws.fresh() if self.ws is not None else None

    def desc(self, tile, out=None, ws=None, cnt=None, pair=None):
        f = self.form
        kw = {}
        if f.conv:
            B, hin, win, hout, wout, stride, ups = f.conv
            kw.update(taps=9, hin=hin, win=win, hout=hout, wout=wout, stride=stride, ups=ups)
        if f.batched:
            kw.update(nb_o=f.nb[0], nb_i=f.nb[1], a_bs=self.a_bs, w_bs=self.w_bs, c_bs=self.c_bs, r_bs=self.r_bs)
        if f.rownorm:
            kw.update(rowstat=self.rowstat.ptr(), colsum=self.colsum.ptr())
        c_ptr = self.c.ptr(out)
        res_ptr = c_ptr if f.res == "inplace" else (self.res.ptr() if self.res is not None else None)
        epi = (ops.EPI_GEGLU if f.geglu else 0) | (ops.EPI_OUT_F32 if f.out_f32 else 0) | \
              (ops.EPI_RES_F32 if f.res == "f32" else 0)
        ws_ptr = None
        if f.splits > 1:
            ws_ptr = self.ws.ptr(ws)
        d = ops.gemm_desc(self.a0.ptr(), self.w.ptr(), c_ptr, f.M, f.N, f.K,
                          a1=self.a1.ptr() if self.a1 is not None else None, lda0=f.lda0, lda1=f.lda1, c0=f.c0, c1=f.c1,
                          ldw=f.ldw, bias=self.b1.ptr() if self.b1 is not None else None,
                          bias2=self.b2.ptr() if self.b2 is not None else None, res=res_ptr,
                          ldr=f.ldr if f.res else 0, alpha=self.alpha, epi=epi, ldc=f.ldc, splits=f.splits, ws=ws_ptr,
                          tile=tile, **kw)
        if cnt is not None:
            d.cnt = cnt.data_ptr() if torch.is_tensor(cnt) else cnt
        d.pair = f.pair if pair is None else pair
        if cnt is None:
            d.cnt = 0
        return d


def _conv(B, hin, win, hout, wout, stride=1, ups=0):
    return dict(M=B * hout * wout, conv=(B, hin, win, hout, wout, stride, ups))


_BATCH = dict(batched=True, res="f16")          # nb_o = 2, nb_i = 3, eight distinct batch strides (Case), a_bs_o = 0
_FORM_LIST = [
    # plain: bias, alpha = 0.5, fp16 residual.  K = one tile / fewer than every ring depth / more than the six-stage ring;
    # K = 72: K % 64 != 0 (register loop; the DMA codes fall back to it)
    Form("plain_k64", K=64, res="f16", alpha=0.5),
    Form("plain_k192", K=192, res="f16", alpha=0.5),
    Form("plain_k448", K=448, res="f16", alpha=0.5),
    Form("plain_k72", K=72, res="f16", alpha=0.5),
    Form("plain_k200", K=200, res="f16", alpha=0.5),
    Form("plain_n4", N=324, res="f16", alpha=0.5),
    Form("tiny_m", M=30, res="f16", alpha=0.5),
    # strides and epilogues
    Form("strided", lda0=208, ldw=200, ldc=344, ldr=336, res="f16"),
    Form("inplace", ldc=336, res="inplace", bias=False),
    Form("res_f32", res="f32", bias=False),
    Form("out_f32_bias2", out_f32=True, bias2=True),
    Form("f16_bias2_alpha", bias2=True, alpha=0.5, res="f16", ldr=344),
    Form("geglu", N=NG, geglu=True, alpha=0.5),
    Form("geglu_res", N=NG, geglu=True, alpha=0.5, res="f16", ldr=184),
    Form("rownorm", rownorm=True),
    Form("rownorm_geglu", N=NG, geglu=True, rownorm=True),
    Form("two_src", c0=64, c1=128, lda1=136, bias=False),
    Form("two_src_small", K=64, c0=24, c1=40, bias=False),
    # 3x3 gathers: 64 channels, hin != win everywhere
    Form("conv_same", K=576, **_conv(5, 6, 10, 6, 10)),
    Form("conv_s2", K=576, **_conv(13, 8, 12, 4, 6, stride=2)),
    Form("conv_ups1", K=576, **_conv(5, 3, 5, 6, 10, ups=1)),
    Form("conv_ups2", K=576, **_conv(5, 3, 5, 6, 10, ups=2)),
    Form("conv_two_src", K=1152, c0=64, c1=64, bias=False, **_conv(5, 6, 10, 6, 10)),
    Form("conv_c8", K=72, c0=8, bias=False, **_conv(5, 6, 10, 6, 10)),
    Form("conv_split", K=576, splits=3, **_conv(5, 6, 10, 6, 10)),
    Form("conv_strided", K=576, lda0=72, ldw=584, ldc=336, res="f16", ldr=344, **_conv(5, 6, 10, 6, 10)),
    Form("batched", **_BATCH),
    Form("batched_split", splits=2, **_BATCH),
    # split-K
    Form("split2", splits=2, res="f16"),
    Form("split4of5", K=320, splits=4, res="f16"),          # five K tiles over four splits: the library drops the empty fourth
    Form("split_geglu", N=NG, geglu=True, splits=3),
    Form("split_out_f32", splits=2, out_f32=True),
]
# CFG pair: rows m and m + M / 2 of A / res / rowstat are identical.  "dupdata:X" is the full launch on that data (the
# reference of both pair modes), "half:X" / "dup:X" the pair launches.  For the convolution M / 2 is a whole number of
# images (six images)
_PAIR_BASES = {
    "plain_k192": dict(K=192, res="f16", alpha=0.5),
    "strided": dict(lda0=208, ldw=200, ldc=344, ldr=336, res="f16"),
    "conv_same": dict(K=576, **_conv(6, 6, 10, 6, 10)),
    "geglu": dict(N=NG, geglu=True, alpha=0.5),
    "rownorm": dict(rownorm=True),
}
for _n, _kw in _PAIR_BASES.items():
    _FORM_LIST.append(Form("dupdata:" + _n, base=True, **_kw))
    _FORM_LIST.append(Form("half:" + _n, pair=ops.PAIR_HALF, **_kw))
    _FORM_LIST.append(Form("dup:" + _n, pair=ops.PAIR_DUP, **_kw))
FORMS = {f.name: f for f in _FORM_LIST}
for _i, _f in enumerate(_FORM_LIST):            # the three forms of a pair group share their data
    _f.seed = _i if ":" not in _f.name else 500 + list(_PAIR_BASES).index(_f.name.split(":")[1])


def acceptance_row(form):
    """One row of ACCEPTANCE as lgd_gemm_check answers now: Y accepted (split-K forms: with in-launch counters as well),
    y accepted with the reduce launch only, . refused."""
    cells = []
    for t in TILES:
        ok, ok_cnt = form.accepts(t)
        cells.append("." if not ok else ("Y" if ok_cnt else "y"))
    return cells


def acceptance_table():
    head = "form".ljust(20) + " ".join(f"{t:2d}" for t in TILES)
    rows = [f.name.ljust(20) + " ".join(" " + c for c in acceptance_row(f)) for f in _FORM_LIST]
    return "\n".join([head] + rows)


# The pinned answer of lgd_gemm_check, one row per form, one column per tile code (print(acceptance_table()) rewrites
# it).  Floors of this table (tests/test_gemm_conformance_cpu.py): every code is accepted on at least MIN_FORMS_PER_CODE
# forms and every form by at least MIN_CODES_PER_FORM codes.
ACCEPTANCE = """
form                 1  2  3  4  5  6  7 17 18 19 20 21 22 23 25 26 33 34 35 37 38 39 40 41 42 44 45 46 47
plain_k64            Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
plain_k192           Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
plain_k448           Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
plain_k72            Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  .  .  .  .  .  .  .  .  .  .  .  .  .
plain_k200           Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  .  .  .  .  .  .  .  .  .  .  .  .  .
plain_n4             Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  Y  .  .
tiny_m               Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
strided              Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
inplace              Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
res_f32              Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  Y  .  .
out_f32_bias2        Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  Y  .  .
f16_bias2_alpha      Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
geglu                Y  Y  Y  Y  Y  .  .  Y  Y  Y  Y  Y  .  .  .  Y  .  Y  Y  .  Y  Y  .  Y  Y  Y  Y  Y  .
geglu_res            Y  Y  Y  Y  Y  .  .  Y  Y  Y  Y  Y  .  .  .  Y  .  Y  Y  .  Y  Y  .  Y  Y  .  Y  .  .
rownorm              Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
rownorm_geglu        Y  Y  Y  Y  Y  .  .  Y  Y  Y  Y  Y  .  .  .  Y  .  Y  Y  .  Y  Y  .  Y  Y  Y  Y  Y  .
two_src              Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  .  .
two_src_small        Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  .  .  .  .  .  .  .  .  .  .  .
conv_same            Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  Y  Y
conv_s2              Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  .  .
conv_ups1            Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  .  .
conv_ups2            Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  .  .
conv_two_src         Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  .  .
conv_c8              Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  .  .  .  .  .  .  .  .  .  .  .  .  .
conv_split           Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  y  y
conv_strided         Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  Y  Y
batched              Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .
batched_split        Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  Y  .  .
split2               Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  Y  y  y
split4of5            Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  Y  y  y
split_geglu          Y  Y  Y  Y  Y  .  .  Y  Y  Y  Y  Y  .  .  .  Y  .  Y  Y  .  Y  Y  .  Y  Y  .  Y  y  .
split_out_f32        Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  Y  y  y
dupdata:plain_k192   Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
half:plain_k192      Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
dup:plain_k192       Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
dupdata:strided      Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
half:strided         Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
dup:strided          Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
dupdata:conv_same    Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  Y  Y
half:conv_same       Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  Y  Y
dup:conv_same        Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  .  .  Y  Y
dupdata:geglu        Y  Y  Y  Y  Y  .  .  Y  Y  Y  Y  Y  .  .  .  Y  .  Y  Y  .  Y  Y  .  Y  Y  Y  Y  Y  .
half:geglu           Y  Y  Y  Y  Y  .  .  Y  Y  Y  Y  Y  .  .  .  Y  .  Y  Y  .  Y  Y  .  Y  Y  Y  Y  Y  .
dup:geglu            Y  Y  Y  Y  Y  .  .  Y  Y  Y  Y  Y  .  .  .  Y  .  Y  Y  .  Y  Y  .  Y  Y  Y  Y  Y  .
dupdata:rownorm      Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
half:rownorm         Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
dup:rownorm          Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y  Y
"""
MIN_FORMS_PER_CODE = 23      # code 44
MIN_CODES_PER_FORM = 14      # plain_k72, plain_k200, conv_c8: K % 64 != 0


def pinned():
    """{form name: {tile code: cell}} of ACCEPTANCE."""
    lines = [ln for ln in ACCEPTANCE.strip("\n").split("\n")]
    codes = [int(c) for c in lines[0].split()[1:]]
    table = {}
    for ln in lines[1:]:
        parts = ln.split()
        assert len(parts) == len(codes) + 1, ln
        table[parts[0]] = dict(zip(codes, parts[1:]))
    return table
