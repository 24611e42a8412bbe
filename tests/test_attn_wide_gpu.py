"""lgd_attn_wide_f16 on the GPU (tests/attn_wide_cases.py), against fp64 from the fp16 operands, per element, gated at
1.0 of the bound derived in attn_conformance_cases from the kernel's rounding points.

Per case: the three data passes on packed operands, and the "heads" pass on the two other view forms (q and k as halves of
one [B][S][2 d] buffer, what the VAE passes; wider rows with gaps between the images).  Per launch: no NaN / Inf in O (every
pad, gap, row past the end and guard of the inputs holds NaN), every guard, pad and gap of the output bit-identical to its
sentinel, a second launch bit-identical to the first.  Then the real mid-block shape once, the hot operands (one logit per
row beyond fp16: the materialised sequence loses them, the kernel returns the one-hot result), eager against a captured
graph, and the refusals."""
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
import attn_wide_cases as awc  # noqa: E402

F32, F64, H16 = torch.float32, torch.float64, torch.float16


def _bits(t):
    return t.view(torch.int16)


def _launch(case, vw):
    out = vw.o.carved.fresh()
    ops.attn_wide(vw.q.ptr(), vw.k.ptr(), vw.v.ptr(), vw.o.ptr(out), case.B, case.Sq, case.Sk, case.d, case.scale,
                  q_view=vw.q.view, k_view=vw.k.view, v_view=vw.v.view, o_view=vw.o.view)
    return out


@pytest.mark.parametrize("name", list(awc.BY_NAME))
def test_attn_wide_conforms_on_every_pass_and_form(dev, name):
    case = awc.BY_NAME[name]
    problems, worst = [], 0.0
    for ps in awc.PASSES:
        data = case.data(ps)
        ref = awc.reference(case, *(t[:, 0].to(dev).to(F64) for t in (data.q, data.k, data.v)))
        for form in (awc.FORMS if ps == "heads" else awc.FORMS[:1]):
            where = f"{name} [{ps}, {form}]"
            vw = awc.views(case, form, data, dev)
            out = _launch(case, vw)
            if not vw.o.carved.outside_untouched(out):
                problems.append(f"{where}: a guard / pad / gap element of O was written")
            y = vw.o.logical(out)
            if not bool(torch.isfinite(y).all()):
                problems.append(f"{where}: NaN / Inf in O (a pad, a gap or a row past the end was read into it)")
                continue
            r = awc.ratio(y, ref)
            print(f"[attn_wide] {where}: worst error / bound {r:.3f}")
            worst = max(worst, r)
            if not torch.equal(_bits(_launch(case, vw)), _bits(out)):
                problems.append(f"{where}: a second launch is not bit-identical")
    torch.cuda.synchronize()
    for line in problems:
        print("[attn_wide] FAIL", line)
    gate(f"attn_wide {name}: O, max error / derived bound", worst, 1.0)
    assert not problems, problems


def test_the_real_mid_block_shape(dev):
    """S = 4096, d = 512, B = 1: 64 query blocks, 128 key tiles, every column block of the widest instantiation."""
    case = awc.FULL
    data = case.data("heads")
    vw = awc.views(case, "qk_halves", data, dev)
    out = _launch(case, vw)
    ref = awc.reference(case, *(t[:, 0].to(dev).to(F64) for t in (data.q, data.k, data.v)))
    y = vw.o.logical(out)
    assert vw.o.carved.outside_untouched(out) and bool(torch.isfinite(y).all())
    gate(f"attn_wide {case.name}: O, max error / derived bound", awc.ratio(y, ref), 1.0)


def _materialised(q, k, v):
    """The existing sequence of vae._Blocks._attn on these operands: gemm -> softmax_rows over fp16 scores -> gemm."""
    S, d = q.shape
    sc = torch.empty((S, S), device=q.device, dtype=H16)
    ops.gemm_launch(ops.gemm_desc(q, k, sc, S, S, d, lda0=d, ldw=d, ldc=S))
    pr = ops.softmax_rows(sc, 1.0, out=sc)
    vt = v.t().contiguous()
    a = torch.empty((S, d), device=q.device, dtype=H16)
    ops.gemm_launch(ops.gemm_desc(pr, vt, a, S, d, S, lda0=S, ldw=S, ldc=d))
    return a


def test_hot_logits_are_one_hot_where_the_materialised_sequence_is_lost(dev):
    """Target logits of 71680 (scale 1): stored in fp16 they are +inf and the row's softmax is inf - inf — the existing
    behaviour, arithmetic and not a fault.  In fp32 the softmax is exactly one-hot (the runner-up is 100+ below), so the
    only rounding left is O's: |o[i] - v[j(i)]| <= 2^-11 |v| + 2^-25."""
    q, k, v = (t.to(dev) for t in awc.hot_operands())
    S, d = q.shape
    lost = _materialised(q, k, v)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(lost).all())                         # the precondition
    o = torch.full((S, d), acc.SENT16, device=dev, dtype=H16)
    ops.attn_wide(q, k, v, o, 1, S, S, d, 1.0)
    torch.cuda.synchronize()
    want = v[[awc.hot_target(i) for i in range(S)]].to(F64)
    assert bool(torch.isfinite(o).all())
    err = (o.to(F64) - want).abs() / (2.0 ** -11 * want.abs() + 2.0 ** -25)
    gate("attn_wide hot logits: |o - v[j]| / (2^-11 |v| + 2^-25)", float(err.max()), 1.0 + 1e-12)


def test_eager_and_a_captured_graph_are_bit_identical(dev):
    case = awc.BY_NAME["wide:B3S300x330d512"]
    data = case.data("spiked")
    vw = awc.views(case, "qk_halves", data, dev)
    eager = _launch(case, vw)
    again = _launch(case, vw)
    out = vw.o.carved.fresh()
    args = (vw.q.ptr(), vw.k.ptr(), vw.v.ptr(), vw.o.ptr(out), case.B, case.Sq, case.Sk, case.d, case.scale)
    kw = dict(q_view=vw.q.view, k_view=vw.k.view, v_view=vw.v.view, o_view=vw.o.view)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attn_wide(*args, **kw)                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    out.copy_(vw.o.carved.buf)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.attn_wide(*args, **kw)
    out.copy_(vw.o.carved.buf)                                          # only a replay writes what is compared
    cg.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(again), _bits(eager))
    assert torch.equal(_bits(out), _bits(eager))


def test_refused_calls_raise_and_write_nothing(dev):
    lib = _lib.load()
    buf = torch.full((4 << 19,), acc.SENT16, dtype=H16, device=dev)     # 4 MiB: the operands sit 1 MiB apart
    pristine = buf.clone()
    base = buf.data_ptr()
    assert base % 256 == 0
    for what, change, code in awc.REFUSALS:
        rc = lib.lgd_attn_wide_f16(*awc.refusal_args(change, base))
        assert rc == code, (what, rc)
        with pytest.raises(RuntimeError):
            _lib.check(rc, "lgd_attn_wide_f16")
    q = torch.zeros((1, 8, 16), dtype=H16, device=dev)
    with pytest.raises(RuntimeError):
        ops.attn_wide(q, q, q, buf, 1, 8, 8, 12, 1.0)                   # the wrapper raises on a non-zero status
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(pristine))
    # and the call the table starts from is accepted: q, k, v zeros -> O = 0 in the rows it owns
    buf[: 3 << 19] = 0
    args = awc.refusal_args({}, base)
    args[-1] = ops._stream()
    assert lib.lgd_attn_wide_f16(*args) == 0
    torch.cuda.synchronize()
    o = buf[3 << 19:]
    n = 2 * 64 * 64
    assert bool((o[:n] == 0).all()) and torch.equal(_bits(o[n:]), _bits(pristine[3 << 19:][n:]))
