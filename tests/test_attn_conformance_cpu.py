"""The attention launch contract, checked where there is no GPU (tests/attn_conformance_cases.py):

  * the case table reaches every variant code the library can answer without the process-wide A/B switches of the
    environment, every row selects the code it claims under the option state it names, and a sweep of shapes answers
    nothing ops.ATTN_VARIANTS does not name;
  * the derived error bound is not too tight — an fp32 emulation with fp16 roundings at the documented points stays inside
    on every row — and not too loose — six wrong answers built from the fp64 reference fall outside on the rows flagged
    for them;
  * the host refusals are what the REFUSALS table says, answered by the entry points themselves before the device is
    touched."""
import os
import sys

import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import _lib, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_conformance_cases as acc  # noqa: E402

F32, F64, H16 = torch.float32, torch.float64, torch.float16


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__ as ge
    ge.build()
    yield
    acc.set_options(acc.DEFAULT_OPTS)


def _plan_under(row):
    acc.set_options(row.opts)
    try:
        return row.plan()
    finally:
        acc.set_options(acc.DEFAULT_OPTS)


def test_every_row_selects_the_code_it_claims():
    wrong = [(r.name, _plan_under(r)) for r in acc._ROW_LIST if _plan_under(r) != r.code]
    assert not wrong, wrong


def test_the_variant_table_of_the_library():
    """lgd_attn_variant enumerated to its end: unique codes that decode to a family 1..7, names that fit the buffer, and
    LGD_ERR_ARG past the end; ops.ATTN_VARIANTS / ATTN_VARIANTS_ENV_ONLY are that table."""
    import ctypes as C
    lib = _lib.load()
    code, env_only, name = C.c_int(), C.c_int(), C.create_string_buffer(128)
    rows = []
    while lib.lgd_attn_variant(len(rows), C.byref(code), C.byref(env_only), name, len(name)) == 0:
        rows.append((code.value, env_only.value, name.value.decode()))
        assert len(rows) <= 1000
    n = len(rows)
    assert n == 66
    for bad in (n, n + 1, 1 << 20, -1):
        assert lib.lgd_attn_variant(bad, C.byref(code), C.byref(env_only), name, len(name)) == -1, bad
    assert lib.lgd_attn_variant(0, None, None, None, 0) == 0                       # every output is optional
    codes = [c for c, _, _ in rows]
    assert len(set(codes)) == n
    for c, env, nm in rows:
        fam, dp, sub = c // 100000, (c // 100) % 1000, c % 100
        assert 1 <= fam <= 7 and fam * 100000 + dp * 100 + sub == c, c
        assert dp in ((0,) if fam == 7 else (48, 96) if fam == 2 else (32, 64, 96, 128, 160, 192)), c
        assert env in (0, 1), c
        assert 0 < len(nm) < len(name) - 1, c
    short = C.create_string_buffer(b"x" * 8, 8)
    assert lib.lgd_attn_variant(0, None, None, short, 5) == 0
    assert short.raw[:5] == rows[0][2].encode()[:4] + b"\0" and short.raw[5:] == b"xxx"    # cut to the capacity given, not beyond
    assert ops.ATTN_VARIANTS == {c: nm for c, _, nm in rows}
    assert ops.ATTN_VARIANTS_ENV_ONLY == frozenset(c for c, env, _ in rows if env)
    assert isinstance(ops.ATTN_VARIANTS, dict) and isinstance(ops.ATTN_VARIANTS_ENV_ONLY, frozenset)
    assert len(ops.ATTN_VARIANTS_ENV_ONLY) == 12


def test_every_reachable_code_has_a_row():
    assert set(acc.CODES) <= set(ops.ATTN_VARIANTS)
    missing = sorted(set(ops.ATTN_VARIANTS) - ops.ATTN_VARIANTS_ENV_ONLY - set(acc.CODES))
    assert not missing, [(c, ops.ATTN_VARIANTS[c]) for c in missing]
    assert not (set(acc.CODES) & ops.ATTN_VARIANTS_ENV_ONLY)
    assert ops.ATTN_VARIANTS_ENV_ONLY <= set(ops.ATTN_VARIANTS)


def test_the_plan_answers_only_named_codes():
    """A sweep over shapes, head dims and every option state lgd_set_option reaches: each answer is a key of
    ops.ATTN_VARIANTS that is not marked environment-only (this process runs with the default environment)."""
    env_set = any(k in os.environ for k in ("LGD_ATTN_NW", "LGD_ATTN_BWD"))
    allowed = set(ops.ATTN_VARIANTS) - (set() if env_set else ops.ATTN_VARIANTS_ENV_ONLY)
    seen = set()
    states = [{}, {"attn32": 0}, {"attn32": 2}, {"attn32": 2, "attn32_nw": 4}, {"attn32": 2, "attn32_var": 1}, {"attn32": 2, "attn32_var": 2},
              {"attn_w4": 0}, {"attn_w4": 2}, {"attn_w4": 2, "attn_w4_pipe": 0}]
    try:
        for st in states:
            acc.set_options(dict(acc.DEFAULT_OPTS, **st))
            for d in range(8, 200, 8):
                for B, H in ((1, 1), (2, 8), (8, 8), (16, 8), (2, 172), (2, 256), (16, 64)):
                    for Sq, Sk in ((300, 330), (64, 77), (256, 286), (1024, 1054), (4096, 4126), (300, 1)):
                        for probs, causal in ((0, 0), (1, 0)) + (((0, 1),) if Sq == Sk else ()):
                            if d <= 192:
                                seen.add(ops.attn_plan(ops.ATTN_OP_FWD, B, H, Sq, Sk, d, probs=probs, causal=causal))
                        if d <= 160:
                            seen.add(ops.attn_plan(ops.ATTN_OP_BWD, B, H, Sq, Sk, d, sk_grad=min(Sq, Sk)))
                        if Sk <= 128 and d <= 192:
                            seen.add(ops.attn_plan(ops.ATTN_OP_CROSS_BWD, B, H, Sq, Sk, d))
                            seen.add(ops.attn_plan(ops.ATTN_OP_CROSS_BWD, B, H, Sq, Sk, d, aligned=False))
    finally:
        acc.set_options(acc.DEFAULT_OPTS)
    assert seen <= allowed, sorted(seen - allowed)
    assert ops.attn_plan(ops.ATTN_OP_FWD, 16, 8, 4096, 4096, 40) == 306401
    assert ops.attn_plan(ops.ATTN_OP_FWD, 16, 8, 4096, 4096, 40, aligned=False) == 306401      # `aligned` is read by the cross backward only
    for bad in (dict(d=36), dict(d=200), dict(B=3, pair=ops.PAIR_HALF), dict(sk_grad=400, op=ops.ATTN_OP_BWD), dict(Sk=129, op=ops.ATTN_OP_CROSS_BWD)):
        a = dict(op=ops.ATTN_OP_FWD, B=2, H=2, Sq=300, Sk=330, d=40)
        a.update(bad)
        with pytest.raises(RuntimeError):
            ops.attn_plan(a.pop("op"), a.pop("B"), a.pop("H"), a.pop("Sq"), a.pop("Sk"), a.pop("d"), **a)


# ---------------------------------------------------------------------------------------------
# the bound, shown by the reference alone
# ---------------------------------------------------------------------------------------------
def _pairs(row, n=6):
    """(image, head) pairs the CPU checks look at: all of a small row, else n spread over images and the four head
    magnitudes (the data of every pair is drawn the same way; the GPU suite checks all of them)."""
    all_pairs = [(b, h) for b in range(row.B) for h in range(row.H)]
    if len(all_pairs) <= n:
        return all_pairs
    step = (len(all_pairs) - 1) / (n - 1)
    return [all_pairs[round(i * step)] for i in range(n)]


def _take(t, pairs, dtype):
    return torch.stack([t[b, h] for b, h in pairs]).to(dtype)


def _ratio(got, ref, bound):
    return float(((got.to(F64) - ref).abs() / bound).max())


def _fwd_inputs(row, pass_name, pairs, dtype):
    d = row.data(pass_name)
    return _take(d.q, pairs, dtype), _take(d.k, pairs, dtype), _take(d.v, pairs, dtype)


def _bwd_inputs(row, pass_name, pairs):
    """q, k, v, go and the forward results the backward takes as inputs (fp16 O, fp32 lse from the fp64 forward)."""
    d = row.data(pass_name)
    q, k, v = _fwd_inputs(row, pass_name, pairs, F64)
    f = acc.fwd_reference(q, k, v, row.scale, DP=row.DP, ones=False)
    return q, k, v, _take(d.go, pairs, F64), f["o"].to(H16).to(F64), f["lse"].to(F32).to(F64)


@pytest.mark.parametrize("name", list(acc.ROWS_BY_NAME))
def test_emulation_with_the_documented_roundings_stays_inside_the_bound(name):
    row = acc.ROWS_BY_NAME[name]
    pairs = _pairs(row)
    worst = {}
    for ps in acc.PASSES:
        if row.op in ("self", "map"):
            q, k, v = _fwd_inputs(row, ps, pairs, F64)
            ref = acc.fwd_reference(q, k, v, row.scale, DP=row.DP, ones=row.ones, causal=row.causal, want_probs=row.op == "map")
            emu = acc.fwd_emulation(q.to(F32), k.to(F32), v.to(F32), row.scale, ones=row.ones, causal=row.causal)
            outs = ("o", "lse") + (("p",) if row.op == "map" else ())
        elif row.op == "bwd":
            q, k, v, go, o16, lse32 = _bwd_inputs(row, ps, pairs)
            ref = acc.bwd_reference(q, k, v, go, o16, lse32, row.scale, DP=row.DP, sk_grad=row.sk_grad)
            emu = acc.bwd_emulation(*(t.to(F32) for t in (q, k, v, go, o16, lse32)), row.scale, sk_grad=row.sk_grad)
            outs = ("gq", "gk", "gv", "delta")
        else:
            q, k, v = _fwd_inputs(row, ps, pairs, F64)
            d = row.data(ps)
            go, gp = _take(d.go, pairs, F64), _take(d.gp, pairs, F64)
            ref = acc.xbwd_reference(q, k, v, go, gp, row.scale, DP=row.DP, ds16=row.ds16)
            emu = acc.xbwd_emulation(q.to(F32), k.to(F32), v.to(F32), go.to(F32), gp.to(F32), row.scale, ds16=row.ds16)
            outs = ("gq",)
        for o in outs:
            assert bool(torch.isfinite(ref[o]).all()) and bool((ref["bound_" + o] > 0).all()), (ps, o)
            worst[(ps, o)] = _ratio(emu[o], ref[o], ref["bound_" + o])
    print(f"[attn bound] {name}: emulation error / bound " + ", ".join(f"{p}.{o} {v:.3f}" for (p, o), v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


_FWD_ROWS = [n for n, r in acc.ROWS_BY_NAME.items() if r.op in ("self", "map") and not r.causal]
_BWD_ROWS = [n for n, r in acc.ROWS_BY_NAME.items() if r.op == "bwd"]


def _fwd_ref(row, ps, pairs, **mut):
    q, k, v = _fwd_inputs(row, ps, pairs, F64)
    if mut.get("drop_last"):
        k, v = k[:, :-1], v[:, :-1]
    if mut.get("pad_key"):
        z = torch.zeros_like(k[:, :1])
        k, v = torch.cat([k, z], 1), torch.cat([v, z], 1)
    return acc.fwd_reference(q, k, v, row.scale, DP=row.DP, ones=row.ones)


@pytest.mark.parametrize("name", [n for n in _FWD_ROWS if acc.ROWS_BY_NAME[n].Sk >= 8])
def test_a_dropped_last_key_is_outside_the_bound(name):
    """Spiked data: one query puts nearly all its weight on the last key."""
    row = acc.ROWS_BY_NAME[name]
    pairs = _pairs(row)
    ref, mut = _fwd_ref(row, "spiked", pairs), _fwd_ref(row, "spiked", pairs, drop_last=True)
    assert _ratio(mut["o"], ref["o"], ref["bound_o"]) > 2.0
    assert _ratio(mut["lse"], ref["lse"], ref["bound_lse"]) > 2.0


@pytest.mark.parametrize("name", [n for n in _FWD_ROWS if acc.ROWS_BY_NAME[n].Sk <= 77])
def test_a_counted_pad_key_is_outside_the_bound(name):
    """Rows with at most 77 keys, offset V and small logits: a zero pad key takes 1 / (Sk + 1) of the weight, which moves O
    by that fraction of sum p |v| — several times the bound.  (At 330 keys the fraction, 0.3 %, is of the size of the
    worst-case rounding of a `ones` kernel, so those rows are not flagged; their lse still shows it.)"""
    row = acc.ROWS_BY_NAME[name]
    pairs = _pairs(row)
    ref, mut = _fwd_ref(row, "voffset", pairs), _fwd_ref(row, "voffset", pairs, pad_key=True)
    assert _ratio(mut["o"], ref["o"], ref["bound_o"]) > 2.0


@pytest.mark.parametrize("name", _FWD_ROWS)
def test_a_counted_pad_key_shows_in_the_lse(name):
    row = acc.ROWS_BY_NAME[name]
    pairs = _pairs(row)
    ref, mut = _fwd_ref(row, "voffset", pairs), _fwd_ref(row, "voffset", pairs, pad_key=True)
    assert _ratio(mut["lse"], ref["lse"], ref["bound_lse"]) > 2.0


@pytest.mark.parametrize("name", _FWD_ROWS)
@pytest.mark.parametrize("ps", acc.PASSES)
def test_the_output_of_the_next_head_is_outside_the_bound(name, ps):
    """Also for the smallest head (|v| 100 times below the largest): the bound is per element."""
    row = acc.ROWS_BY_NAME[name]
    pairs = [(0, h) for h in range(min(row.H, 5))]
    ref = _fwd_ref(row, ps, pairs)
    for i in range(len(pairs) - 1):
        assert _ratio(ref["o"][i + 1], ref["o"][i], ref["bound_o"][i]) > 2.0, (ps, i)


def _bwd_ref(row, ps, pairs, *, drop_q=0, delta_cols=None):
    q, k, v, go, o16, lse32 = _bwd_inputs(row, ps, pairs)
    if drop_q:                          # the last queries contribute nothing to dK / dV
        q, go, o16, lse32 = q[:, :-drop_q], go[:, :-drop_q], o16[:, :-drop_q], lse32[:, :-drop_q]
    if delta_cols is not None:          # delta from the first delta_cols head-dim columns only
        o16 = o16.clone()
        o16[..., delta_cols:] = 0.0
    return acc.bwd_reference(q, k, v, go, o16, lse32, row.scale, DP=row.DP, sk_grad=row.sk_grad)


@pytest.mark.parametrize("name", [n for n in _BWD_ROWS if acc.ROWS_BY_NAME[n].Sq > 64])
@pytest.mark.parametrize("ps", acc.PASSES)
def test_sixteen_missing_queries_are_outside_the_bound_of_dk_dv(name, ps):
    row = acc.ROWS_BY_NAME[name]
    pairs = _pairs(row)
    ref, mut = _bwd_ref(row, ps, pairs), _bwd_ref(row, ps, pairs, drop_q=16)
    if row.Sk > 1:                      # with one key P = 1 and dS = dP - delta = 0: dQ and dK are zero whatever is summed
        assert _ratio(mut["gk"], ref["gk"], ref["bound_gk"]) > 2.0
    assert _ratio(mut["gv"], ref["gv"], ref["bound_gv"]) > 2.0


@pytest.mark.parametrize("name", [n for n in _BWD_ROWS if acc.ROWS_BY_NAME[n].Sk > 1])
@pytest.mark.parametrize("ps", acc.PASSES)
def test_dq_without_the_scale_is_outside_the_bound(name, ps):
    row = acc.ROWS_BY_NAME[name]
    ref = _bwd_ref(row, ps, _pairs(row))
    assert _ratio(ref["gq"] / row.scale, ref["gq"], ref["bound_gq"]) > 2.0


@pytest.mark.parametrize("name", _BWD_ROWS)
def test_delta_without_the_last_column_is_outside_the_bound(name):
    """In delta itself on every pass; in dQ and dK on the pass with offset V and go (the dropped product is of the size
    of the others there, and every key carries weight)."""
    row = acc.ROWS_BY_NAME[name]
    pairs = _pairs(row)
    for ps in acc.PASSES:
        ref, mut = _bwd_ref(row, ps, pairs), _bwd_ref(row, ps, pairs, delta_cols=row.d - 1)
        assert _ratio(mut["delta"], ref["delta"], ref["bound_delta"]) > 2.0, ps
        if ps == "voffset" and row.Sk > 1:
            assert _ratio(mut["gq"], ref["gq"], ref["bound_gq"]) > 2.0
            assert _ratio(mut["gk"], ref["gk"], ref["bound_gk"]) > 2.0


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_accepted_base_calls_of_the_refusal_table_are_well_formed():
    """Every REFUSALS row names arguments its entry point has (a typo would otherwise test nothing)."""
    for fn, what, change in acc.REFUSALS:
        names = [n[2:] if n.startswith("p:") else n for n in acc._ARGS[fn].split()]
        assert set(change) <= set(names), (fn, what)
        assert len(acc.refusal_args(fn, change, acc.P)) == len(_lib.SIGNATURES[fn]), fn


@pytest.mark.parametrize("fn,what,change", acc.REFUSALS, ids=[f"{f}:{w}" for f, w, _ in acc.REFUSALS])
def test_host_refusal(fn, what, change):
    lib = _lib.load()
    rc = getattr(lib, fn)(*acc.refusal_args(fn, change, acc.P))
    assert rc in (-1, -3), (fn, what, rc)
    assert rc == (-3 if what.startswith("d > ") and fn != "lgd_cross_attn_bwd_f16" else -1), (fn, what, rc)
