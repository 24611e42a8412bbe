"""Whatever variant lgd_attn_plan names, the attention entry points compute: every variant code of the dispatch on every
view form its op is asked to serve (tests/attn_conformance_cases.py), one test per code.

Every row first asserts that the library selects the code under the row's option state, then runs its forms on the
"heads" data (per-head magnitudes 100x apart) and its first form on the "spiked" and "voffset" data.  Per launch:

  * every element of O, lse, the probability map, dQ, dK, dV and delta within the per-element bound derived in the case
    module's docstring from the rounding points of the kernels — the worst error / bound ratio and the (image, head) that
    holds it are printed, and gated at 1.0;
  * no NaN / Inf in anything that was to be written: every input pad, gap between images, row past Sk (or past Sq in a
    fused buffer) and guard holds NaN;
  * every guard, pad and gap of every output buffer, rows >= Sk_grad of dK / dV, the rows of a fused gradient buffer no
    gradient owns and the second half under PAIR_HALF bit-identical to their sentinels;
  * PAIR_HALF / PAIR_DUP bit-equal to the full launch on the duplicated batch; Sk_grad < Sk bit-equal to the full backward
    in dQ and the first rows of dK / dV; a second launch bit-identical to the first.

The refusals of the REFUSALS table raise before anything is launched and write nothing."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import lgd_amd  # noqa: E402,F401
from conftest import gate  # noqa: E402
from lgd_amd import _lib, ops  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_conformance_cases as acc  # noqa: E402

F32, F64, H16 = torch.float32, torch.float64, torch.float16
CHUNK_ELEMS = 1 << 22            # Sq * Sk * pairs per reference chunk (32 MiB per fp64 temporary)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _heads(t, H):
    """[B][S][H*d] -> [B][H][S][d]"""
    B, S, C = t.shape
    return t.reshape(B, S, H, C // H).permute(0, 2, 1, 3)


def _chunked(fn, tensors, row):
    """fn over groups of (image, head) pairs; tensors [B][H][..] (None passes through); concatenated back to [B][H][..]."""
    B, H = row.B, row.H
    flat = [None if t is None else t.reshape(B * H, *t.shape[2:]) for t in tensors]
    step = max(1, CHUNK_ELEMS // (row.Sq * row.Sk))
    outs = []
    for i in range(0, B * H, step):
        outs.append(fn(*[None if t is None else t[i:i + step] for t in flat]))
    return {k: torch.cat([o[k] for o in outs]).reshape(B, H, *outs[0][k].shape[1:]) for k in outs[0]}


class Tally:
    def __init__(self, row):
        self.row, self.problems, self.worst = row, [], {}

    def values(self, what, y, ref, bound, where):
        """y, ref, bound [B'][H][..]: NaN check and the worst error / bound per (image, head)."""
        if not bool(torch.isfinite(y).all()):
            self.problems.append(f"{where}: NaN / Inf in {what} (a pad, a gap or a row past the end was read into it)")
            return
        ratio = ((y.to(F64) - ref).abs() / bound).flatten(2).amax(-1)          # [B'][H]
        worst = float(ratio.max())
        b, h = divmod(int(ratio.argmax()), ratio.shape[1])
        if worst > self.worst.get(what, (0.0,))[0]:
            self.worst[what] = (worst, f"{where} image {b} head {h}")
        if worst > 1.0:
            self.problems.append(f"{where}: {what} error / bound = {worst:.3f} at image {b} head {h} "
                                 f"({int((ratio > 1.0).sum())} of {ratio.numel()} (image, head) pairs outside)")

    def untouched(self, what, carved, buf, where):
        if not carved.outside_untouched(buf):
            self.problems.append(f"{where}: a guard / pad / gap element of {what} was written")

    def sentinel(self, what, got, carved_logical, where):
        if not torch.equal(_bits(got), _bits(carved_logical)):
            self.problems.append(f"{where}: {what} was written")

    def same(self, what, a, b, where):
        if not torch.equal(_bits(a), _bits(b)):
            self.problems.append(f"{where}: {what}")


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
def _launch_fwd(row, vw, pair=None):
    out, lse, probs = vw.o.carved.fresh(), None, None
    if row.op == "self":
        lse = vw.lse.fresh()
        ops.attn_fwd(vw.q.ptr(), vw.k.ptr(), vw.v.ptr(), vw.o.ptr(out), row.B, row.H, row.Sq, row.Sk, row.d, row.scale,
                     lse=vw.lse.ptr(lse), q_view=vw.q.view, k_view=vw.k.view, v_view=vw.v.view, o_view=vw.o.view,
                     pair=vw.pair if pair is None else pair)
    elif row.causal:
        ops.attn_causal_fwd(vw.q.ptr(), vw.k.ptr(), vw.v.ptr(), vw.o.ptr(out), row.B, row.H, row.Sq, row.d, row.scale, view=vw.q.view)
    else:
        probs = vw.probs.fresh()
        ops.cross_attn_fwd(vw.q.ptr(), vw.k.ptr(), vw.v.ptr(), vw.o.ptr(out), row.B, row.H, row.Sq, row.Sk, row.d, row.scale,
                           probs=vw.probs.ptr(probs), tok=vw.tok, cond_only=vw.cond_only, q_view=vw.q.view, k_view=vw.k.view,
                           v_view=vw.v.view, o_view=vw.o.view)
    return out, lse, probs


def _run_fwd(row, ps, forms, dev, tally):
    data = row.data(ps)
    B, H, half = row.B, row.H, row.B // 2
    q, k, v = (t.to(dev).to(F64) for t in (data.q, data.k, data.v))
    ref = _chunked(lambda a, b, c: acc.fwd_reference(a, b, c, row.scale, DP=row.DP, ones=row.ones, causal=row.causal,
                                                     want_probs=row.op == "map" and not row.causal), [q, k, v], row)
    for form in forms:
        where = f"{row.name} [{ps}, {form}]"
        vw = acc.views(row, form, data, dev)
        out, lse, probs = _launch_fwd(row, vw)
        tally.untouched("O", vw.o.carved, out, where)
        y = _heads(vw.o.logical(out), H)
        sent_o = _heads(vw.o.logical(vw.o.carved.buf), H)
        img = list(range(B)) if not vw.pair else [b % half for b in range(B)]        # pair forms: duplicated images
        n = half if vw.pair == ops.PAIR_HALF else B
        tally.values("O", y[:n], ref["o"][img[:n]], ref["bound_o"][img[:n]], where)
        if lse is not None:
            tally.untouched("lse", vw.lse, lse, where)
            l = vw.lse.logical(lse)
            tally.values("lse", l[:n, :, :, None], ref["lse"][img[:n], :, :, None], ref["bound_lse"][img[:n], :, :, None], where)
        if vw.pair:
            full_o, full_lse, _ = _launch_fwd(row, vw, pair=0)
            yf, lf = _heads(vw.o.logical(full_o), H), vw.lse.logical(full_lse)
            tally.same("pair launch differs from the full launch in images < B / 2", y[:half], yf[:half], where)
            tally.same("pair launch differs from the full launch in lse of images < B / 2", l[:half], lf[:half], where)
            if vw.pair == ops.PAIR_HALF:
                tally.sentinel("O of images >= B / 2 under PAIR_HALF", y[half:], sent_o[half:], where)
                tally.sentinel("lse of images >= B / 2 under PAIR_HALF", l[half:], vw.lse.logical(vw.lse.buf)[half:], where)
            else:
                tally.same("PAIR_DUP differs from the full launch in images >= B / 2", y[half:], yf[half:], where)
                tally.same("PAIR_DUP differs from the full launch in lse of images >= B / 2", l[half:], lf[half:], where)
        if probs is not None:
            tally.untouched("the probability map", vw.probs, probs, where)
            pm = vw.probs.logical(probs)
            sel = slice(half, B) if vw.cond_only else slice(0, B)
            cols = slice(vw.tok, vw.tok + 1) if vw.tok >= 0 else slice(None)
            tally.values("probs", pm, ref["p"][sel][..., cols], ref["bound_p"][sel][..., cols], where)
        out2, lse2, probs2 = _launch_fwd(row, vw)
        tally.same("a second launch is not bit-identical (O)", out2, out, where)
        if lse is not None:
            tally.same("a second launch is not bit-identical (lse)", lse2, lse, where)
        if probs is not None:
            tally.same("a second launch is not bit-identical (probs)", probs2, probs, where)


# ---------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------
def _launch_bwd(row, vw, sk_grad=None):
    bufs = {}
    for name in ("gq", "gk", "gv"):
        c = getattr(vw, name).carved
        bufs.setdefault(id(c), c.fresh())
    g = {n: bufs[id(getattr(vw, n).carved)] for n in ("gq", "gk", "gv")}
    delta = vw.delta.fresh()
    ops.attn_bwd(vw.q.ptr(), vw.k.ptr(), vw.v.ptr(), vw.o.ptr(), vw.go.ptr(), vw.lse.ptr(), vw.delta.ptr(delta),
                 vw.gq.ptr(g["gq"]), vw.gk.ptr(g["gk"]), vw.gv.ptr(g["gv"]), row.B, row.H, row.Sq, row.Sk, row.d, row.scale,
                 q_view=vw.q.view, k_view=vw.k.view, v_view=vw.v.view, o_view=vw.o.view, go_view=vw.go.view,
                 gq_view=vw.gq.view, gk_view=vw.gk.view, gv_view=vw.gv.view, sk_grad=vw.sk_grad if sk_grad is None else sk_grad)
    return g, delta


def _run_bwd(row, ps, forms, dev, tally):
    data = row.data(ps)
    H = row.H
    q, k, v, go = (t.to(dev).to(F64) for t in (data.q, data.k, data.v, data.go))
    fwd = _chunked(lambda a, b, c: {n: t for n, t in acc.fwd_reference(a, b, c, row.scale, DP=row.DP, ones=False).items() if n in ("o", "lse")},
                   [q, k, v], row)
    o16, lse32 = fwd["o"].to(H16), fwd["lse"].to(F32)          # the inputs of the backward, as a forward would leave them
    ref = _chunked(lambda a, b, c, e, f, g_: acc.bwd_reference(a, b, c, e, f, g_, row.scale, DP=row.DP),
                   [q, k, v, go, o16.to(F64), lse32.to(F64)], row)
    o16_h, lse32_h = o16.cpu(), lse32.cpu()
    full = None
    for form in forms:
        where = f"{row.name} [{ps}, {form}]"
        vw = acc.views(row, form, data, dev, o16=o16_h, lse32=lse32_h)
        g, delta = _launch_bwd(row, vw)
        skg = vw.sk_grad
        got = {}
        for name in ("gq", "gk", "gv"):
            view = getattr(vw, name)
            tally.untouched(name, view.carved, g[name], where)
            whole = view.carved.logical(g[name])[:, :, view.c0:view.c0 + view.C]        # every row of the buffer's block
            pristine = view.carved.logical(view.carved.buf)[:, :, view.c0:view.c0 + view.C]
            rows = row.Sq if name == "gq" else skg
            got[name] = _heads(whole[:, :rows], H)
            tally.values(name, got[name], ref[name][:, :, :rows], ref["bound_" + name][:, :, :rows], where)
            if whole.shape[1] > rows:
                tally.sentinel(f"{name} rows >= {rows}", whole[:, rows:], pristine[:, rows:], where)
        tally.untouched("delta", vw.delta, delta, where)
        dl = vw.delta.logical(delta)
        tally.values("delta", dl[..., None], ref["delta"][..., None], ref["bound_delta"][..., None], where)
        if form == "contig":
            full = (got, dl)
        if form == "skgrad" and full is not None and skg < row.Sk:
            tally.same("Sk_grad < Sk differs from the full backward in dQ", got["gq"], full[0]["gq"], where)
            tally.same("Sk_grad < Sk differs from the full backward in dK", got["gk"], full[0]["gk"][:, :, :skg], where)
            tally.same("Sk_grad < Sk differs from the full backward in dV", got["gv"], full[0]["gv"][:, :, :skg], where)
            tally.same("Sk_grad < Sk differs from the full backward in delta", dl, full[1], where)
        g2, delta2 = _launch_bwd(row, vw)
        for name in ("gq", "gk", "gv"):
            tally.same(f"a second launch is not bit-identical ({name})", g2[name], g[name], where)
        tally.same("a second launch is not bit-identical (delta)", delta2, delta, where)


def _launch_xbwd(row, vw):
    gq = vw.gq.carved.fresh()
    ops.cross_attn_bwd(vw.q.ptr(), vw.k.ptr(), vw.v.ptr(), vw.go.ptr() if vw.use_go else None, vw.gp.ptr() if vw.use_gp else None,
                       vw.gq.ptr(gq), row.B, row.H, row.Sq, row.Sk, row.d, row.scale, q_view=vw.q.view, k_view=vw.k.view,
                       v_view=vw.v.view, go_view=vw.go.view, gq_view=vw.gq.view)
    return gq


def _run_xbwd(row, ps, forms, dev, tally):
    data = row.data(ps)
    q, k, v, go, gp = (t.to(dev).to(F64) for t in (data.q, data.k, data.v, data.go, data.gp))
    refs = {}
    for form in forms:
        where = f"{row.name} [{ps}, {form}]"
        vw = acc.views(row, form, data, dev)
        key = (vw.use_go, vw.use_gp)
        if key not in refs:
            refs[key] = _chunked(lambda a, b, c, e, f: acc.xbwd_reference(a, b, c, e, f, row.scale, DP=row.DP, ds16=row.ds16),
                                 [q, k, v, go if vw.use_go else None, gp if vw.use_gp else None], row)
        gq = _launch_xbwd(row, vw)
        tally.untouched("gq", vw.gq.carved, gq, where)
        tally.values("gq", _heads(vw.gq.logical(gq), row.H), refs[key]["gq"], refs[key]["bound_gq"], where)
        tally.same("a second launch is not bit-identical (gq)", _launch_xbwd(row, vw), gq, where)


_RUN = {"self": _run_fwd, "map": _run_fwd, "bwd": _run_bwd, "xbwd": _run_xbwd}


@pytest.mark.parametrize("code", acc.CODES)
def test_attn_variant_conforms_on_every_form(dev, code):
    failures, worst = [], {}
    for row in acc.rows_of(code):
        tally = Tally(row)
        acc.set_options(row.opts)
        try:
            assert row.plan() == code, f"{row.name}: the library selects {row.plan()}"
            for ps in acc.PASSES:
                _RUN[row.op](row, ps, row.forms if ps == "heads" else row.forms[:1], dev, tally)
            torch.cuda.synchronize()
        finally:
            acc.set_options(acc.DEFAULT_OPTS)
        failures += tally.problems
        for what, (ratio, at) in tally.worst.items():
            print(f"[attn conformance] code {code} {row.name}: {what} worst error / bound {ratio:.3f} at {at}")
            if ratio > worst.get(what, 0.0):
                worst[what] = ratio
    for line in failures:
        print("[attn conformance] FAIL", line)
    for what, ratio in worst.items():
        gate(f"attention code {code} ({ops.ATTN_VARIANTS[code]}): {what}, max error / derived bound", ratio, 1.0)
    assert worst, "nothing was compared"
    assert not failures, failures


def test_refused_calls_raise_and_write_nothing(dev):
    """Every row of the REFUSALS table: the entry point answers a negative code before anything is launched; the memory
    its pointers name keeps its sentinel bytes."""
    lib = _lib.load()
    buf = torch.full((12 << 19,), acc.SENT16, dtype=H16, device=dev)          # 12 MiB: the operands sit 1 MiB apart
    pristine = buf.clone()
    base = buf.data_ptr()
    assert base % 256 == 0
    for fn, what, change in acc.REFUSALS:
        rc = getattr(lib, fn)(*acc.refusal_args(fn, change, base))
        assert rc < 0, (fn, what, rc)
        with pytest.raises(RuntimeError):
            _lib.check(rc, fn)
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(pristine))
