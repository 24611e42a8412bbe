"""The small-kernel contract (tests/small_kernel_cases.py), checked where there is no GPU:

  * every REFUSALS row answers exactly LGD_ERR_ARG through the library with placeholder pointers — a launch attempt on a host
    without a GPU would answer LGD_ERR_LAUNCH, so the refusal happens before the device — and the BASE call of every entry
    point is well formed (it is the one call that does reach the launch);
  * every check of the ops wrappers raises on host tensors;
  * an fp32 rendering of each kernel's arithmetic stays inside the derived bound on every row and pass, and every wrong answer
    of MUTATIONS falls outside;
  * the erf polynomial's own error, which the bounds use, is measured and printed.

test_base_calls_are_well_formed and test_optional_operands_stay_optional make calls the library accepts, on placeholder
pointers: they run only on a host without a GPU (there the launch fails with LGD_ERR_LAUNCH, which is the proof that every
check was passed) and skip where one is present, where the launch would run on those addresses.  On a GPU machine the
accepted forms are the rows of tests/test_small_kernels_gpu.py."""
import os
import sys

import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import _lib, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_kernel_cases as skc  # noqa: E402

H16, F32, F64, I32 = torch.float16, torch.float32, torch.float64, torch.int32
ERR_ARG, ERR_LAUNCH, ERR_UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__ as ge
    ge.build()


def _answer(fn, change):
    return getattr(_lib.load(), fn)(*skc.call_args(fn, change))


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_the_refusal_table_is_well_formed():
    assert set(skc.ARGS) == set(skc.BASE) == set(skc.RULES) and len(skc.ARGS) == 16
    labels = {}
    for fn, what, change in skc.REFUSALS:
        assert set(change) <= {n[2:] if n.startswith("p:") else n for n in skc.ARGS[fn].split()}, (fn, what)
        assert what not in labels.setdefault(fn, set()), (fn, what)
        labels[fn].add(what)
    for fn, args in skc.ARGS.items():
        names = args.split()
        assert len(names) == len(_lib.SIGNATURES[fn]), fn
        ptrs = skc.pointers(fn)
        want = {f"{p} NULL" for p in ptrs if p not in skc.OPTIONAL}
        want |= {f"{p} off {skc.ALIGN[fn][p]} bytes" for p in ptrs}
        counts = [n for n in names if n in ("n", "rows", "B", "H", "W", "L", "HW", "C", "Cin", "reps")]
        want |= {f"{c} = {v}" for c in counts for v in (0, -1)}
        assert want <= labels[fn], (fn, sorted(want - labels[fn]))
        assert skc.NEEDS[fn] <= {cls for cls, _, _ in skc.RULES[fn]}, fn
        vec = [p for p in ptrs if skc.ALIGN[fn][p] == 16]
        assert all(isinstance(v, tuple) and (v[1] % skc.ALIGN[fn][k] == 0) for cls, _, ch in skc.RULES[fn] if cls == "alias"
                   for k, v in ch.items()), fn           # an alias row is refused for the overlap, not for its alignment
        assert fn in ("lgd_cfg_ddim_step_f32", "lgd_cfg_multistep_step_f32", "lgd_axpy_f32", "lgd_select_row_f32",
                      "lgd_scale_rows_f32", "lgd_conv_in_f16") or vec, fn
    step = {w for f, w, _ in skc.REFUSALS if f == "lgd_cfg_ddim_step_f32"}
    assert {"frozen_ref without mask", "mask without frozen_ref"} <= step
    assert {"col 4", "col -1", "per_sample -1", "n % per_sample with active"} <= labels["lgd_axpy_f32"]


def test_base_calls_are_well_formed():
    """The BASE call of every entry point passes every check: it reaches the launch, which a host without a GPU answers with
    LGD_ERR_LAUNCH (on a GPU machine it would run on placeholder addresses, so it is only made where there is none)."""
    if torch.cuda.is_available():
        pytest.skip("the placeholder pointers would be launched on")
    for fn in skc.ARGS:
        assert _answer(fn, {}) == ERR_LAUNCH, fn


@pytest.mark.parametrize("fn,what,change", skc.REFUSALS, ids=[f"{f}:{w}" for f, w, _ in skc.REFUSALS])
def test_host_refusal(fn, what, change):
    assert _answer(fn, change) == ERR_ARG, (fn, what)


@pytest.mark.parametrize("fn,what,change", skc.UNSUPPORTED, ids=[f"{f}:{w}" for f, w, _ in skc.UNSUPPORTED])
def test_unsupported_stays_unsupported(fn, what, change):
    assert _answer(fn, change) == ERR_UNSUPPORTED, (fn, what)


def test_optional_operands_stay_optional():
    """bias; hist; frozen_ref and mask together; active: NULL passes every check (host without a GPU: the launch is reached)."""
    if torch.cuda.is_available():
        pytest.skip("the placeholder pointers would be launched on")
    for fn, change in (("lgd_conv_out_f16", dict(bias=None)), ("lgd_conv_in_f16", dict(bias=None)),
                       ("lgd_cfg_ddim_step_f32", dict(hist=None)), ("lgd_cfg_ddim_step_f32", dict(frozen_ref=None, mask=None)),
                       ("lgd_cfg_multistep_step_f32", dict(frozen_ref=None, mask=None, hist=None)),
                       ("lgd_axpy_f32", dict(active=None)), ("lgd_axpy_f32", dict(active=None, per_sample=0)),
                       ("lgd_axpy_f32", dict(per_sample=0)), ("lgd_axpy_f32", dict(active=None, per_sample=7)),
                       ("lgd_add_f16", dict(y=("a", 0))), ("lgd_add_f16", dict(y=("b", 0))), ("lgd_add_f16", dict(y=("a", 0), b=("a", 0))),
                       ("lgd_add_f16", dict(b=("a", 16))), ("lgd_scale_f16", dict(y=("x", 0))), ("lgd_quick_gelu_f16", dict(y=("x", 0))),
                       ("lgd_act_f16", dict(y=("x", 0))), ("lgd_act_f16", dict(mode=2)), ("lgd_softmax_rows_f16", dict(y=("x", 0))),
                       ("lgd_cfg_ddim_step_f32", dict(x_out=("x", 0))), ("lgd_cfg_multistep_step_f32", dict(x_out=("x", 0)))):
        assert _answer(fn, change) == ERR_LAUNCH, (fn, change)


def _wrapper_faults():
    h = lambda *s: torch.zeros(*s, dtype=H16)
    f = lambda *s: torch.zeros(*s, dtype=F32)
    i = lambda *s: torch.zeros(*s, dtype=I32)
    wide = h(8, 32)[:, :16]                               # not contiguous
    x4 = f(2, 4, 4, 4)
    return [
        ("add: counts disagree", lambda: ops.add(h(64), h(56))),
        ("add: out count", lambda: ops.add(h(64), h(64), h(72))),
        ("add: dtype", lambda: ops.add(h(64), f(64))),
        ("add: strided", lambda: ops.add(wide, h(8, 16))),
        ("scale: dtype", lambda: ops.scale(f(64), 0.5)),
        ("scale: out count", lambda: ops.scale(h(64), 0.5, h(32))),
        ("quick_gelu: dtype", lambda: ops.quick_gelu(f(64))),
        ("quick_gelu: strided", lambda: ops.quick_gelu(wide)),
        ("act: dtype", lambda: ops.act(f(64), ops.ACT_GELU)),
        ("act: out strided", lambda: ops.act(h(8, 16), ops.ACT_RELU, wide)),
        ("geglu_fwd: strided", lambda: ops.geglu_fwd(h(4, 128)[:, :64])),
        ("geglu_fwd: out count", lambda: ops.geglu_fwd(h(4, 64), h(4, 64))),
        ("geglu_bwd: gy count", lambda: ops.geglu_bwd(h(4, 64), h(4, 64))),
        ("geglu_bwd: dtype", lambda: ops.geglu_bwd(h(4, 64), f(4, 32))),
        ("softmax_rows: dtype", lambda: ops.softmax_rows(f(4, 64))),
        ("softmax_rows: out strided", lambda: ops.softmax_rows(h(8, 16), 1.0, wide)),
        ("upsample2x_bwd: gy count", lambda: ops.upsample2x_bwd(h(2 * 15, 16), 2, 3, 5, 16)),
        ("upsample2x_bwd: dtype", lambda: ops.upsample2x_bwd(f(2 * 60, 16), 2, 3, 5, 16)),
        ("nchw_to_nhwc8: dtype", lambda: ops.nchw_to_nhwc8(h(2, 4, 5, 5))),
        ("nchw_to_nhwc8: strided", lambda: ops.nchw_to_nhwc8(f(2, 8, 5, 5)[:, :4])),
        ("nchw_to_nhwc8: out count", lambda: ops.nchw_to_nhwc8(f(2, 4, 5, 5), h(50, 4))),
        ("conv_out: w count", lambda: ops.conv_out(h(18, 16), h(4, 72), None, 2, 3)),
        ("conv_out: x count", lambda: ops.conv_out(h(9, 16), h(4, 144), None, 2, 3)),
        ("conv_out: bias dtype", lambda: ops.conv_out(h(18, 16), h(4, 144), h(4), 2, 3)),
        ("conv_in: x dtype", lambda: ops.conv_in(h(2, 4, 5, 5), h(64, 36), f(64))),
        ("conv_in: bias count", lambda: ops.conv_in(f(2, 4, 5, 5), h(64, 36), f(32))),
        ("cfg_ddim_step: eps is not the pair", lambda: ops.cfg_ddim_step(f(2, 4, 4, 4), x4, x4, f(3, 4), i(4))),
        ("cfg_ddim_step: mask count", lambda: ops.cfg_ddim_step(f(4, 4, 4, 4), x4, x4, f(3, 4), i(4), frozen_ref=f(4, 2, 4, 4, 4), mask=f(2, 8))),
        ("cfg_ddim_step: dyn dtype", lambda: ops.cfg_ddim_step(f(4, 4, 4, 4), x4, x4, f(3, 4), torch.zeros(4, dtype=torch.int64))),
        ("cfg_ddim_step: table width", lambda: ops.cfg_ddim_step(f(4, 4, 4, 4), x4, x4, f(3, 3), i(4))),
        ("cfg_ddim_step: hist is no whole latents", lambda: ops.cfg_ddim_step(f(4, 4, 4, 4), x4, x4, f(3, 4), i(4), hist=f(100))),
        ("cfg_multistep_step: x0_prev count", lambda: ops.cfg_multistep_step(f(4, 4, 4, 4), x4, x4, f(2, 4, 4, 2), f(3, 8), i(4))),
        ("cfg_multistep_step: x_out dtype", lambda: ops.cfg_multistep_step(f(4, 4, 4, 4), x4, h(2, 4, 4, 4), f(2, 4, 4, 4), f(3, 8), i(4))),
        ("axpy: g count", lambda: ops.axpy(f(3, 10), f(3, 20), f(4, 4), i(1), 0)),
        ("axpy: active count", lambda: ops.axpy(f(3, 20), f(3, 20), f(4, 4), i(1), 0, active=f(2))),
        ("axpy: step_idx dtype", lambda: ops.axpy(f(3, 20), f(3, 20), f(4, 4), f(1), 0)),
        ("scale_rows: out count", lambda: ops.scale_rows(f(7), f(7), f(3, 5), i(4), 3, reps=2)),
        ("scale_rows: dtype", lambda: ops.scale_rows(h(8), f(8), f(3, 5), i(4), 3)),
        ("select_row: no rows of that length", lambda: ops.select_row(f(4, 300), i(1), f(299))),
        ("select_row: idx dtype", lambda: ops.select_row(f(4, 300), torch.zeros(1, dtype=torch.int64), f(300))),
        # the two guidance energies: tests/test_energy_kernels_cpu.py holds the full list
        ("ca_energy: partial count", lambda: ops.ca_energy(torch.zeros(1, dtype=torch.int64), None, i(1), i(3, 8), f(3, 4), f(2, 256), None, 0,
                                                           None, i(2, 2), 2, 3, 3, 77, 256, f(3), f(1))),
        ("boxdiff_energy: smooth count", lambda: ops.boxdiff_energy(torch.zeros(2, dtype=torch.int64), None, 2, 16, i(4, 8), f(2, 3, 256), f(3),
                                                                    i(1, 2), 1, 4, 2, 77, 1.0, 1.0, f(1))),
    ]


_FAULTS = _wrapper_faults()


@pytest.mark.parametrize("what,call", _FAULTS, ids=[w for w, _ in _FAULTS])
def test_wrapper_check_raises_before_the_library(what, call, monkeypatch):
    monkeypatch.setattr(ops, "_call", lambda *a: pytest.fail(f"{what}: the library was called"))
    with pytest.raises(RuntimeError):
        call()


def test_every_wrapper_has_a_check():
    heads = {w.split(":")[0] for w, _ in _FAULTS}
    assert heads == {"add", "scale", "quick_gelu", "act", "geglu_fwd", "geglu_bwd", "softmax_rows", "upsample2x_bwd", "nchw_to_nhwc8",
                     "conv_out", "conv_in", "cfg_ddim_step", "cfg_multistep_step", "axpy", "scale_rows", "select_row", "ca_energy",
                     "boxdiff_energy"}


# ---------------------------------------------------------------------------------------------
# numerics
# ---------------------------------------------------------------------------------------------
def test_erf_polynomial_error():
    e = skc.erf_poly_error()
    print(f"[erf] the A&S 7.1.26 polynomial with the fp32 coefficients, in fp64 against math.erf on [0, 6]: {e:.4e}")
    assert 5e-8 < e <= 1.5e-7                              # csrc/common.h claims 1.5e-7; far below means the grid missed the extrema


def _is16(entry, out):
    return skc.ENTRIES[entry].outputs[out] == H16


ENTRY_NAMES = sorted(skc.ENTRIES)


@pytest.mark.parametrize("entry", ENTRY_NAMES)
def test_emulation_stays_inside_the_bound(entry):
    worst = 0.0
    for row in skc.rows_of(entry):
        for ps in row.passes:
            d = row.data(ps)
            ref, emu = skc.reference(row, d), skc.emulate(row, d)
            for out, (want, bound) in ref.items():
                assert bool((bound >= 0).all()) and not bool(torch.isnan(bound).any()), (row.name, ps, out)
                r = skc.worst_ratio(emu[out].reshape(want.shape), want, bound, fp16=_is16(entry, out))
                assert r < 1.0, (row.name, ps, out, r)
                worst = max(worst, r)
    print(f"[emulation] {entry}: worst error / bound {worst:.3f}")
    assert skc.rows_of(entry)


@pytest.mark.parametrize("name", sorted(skc.MUTATIONS))
def test_wrong_answer_falls_outside(name):
    row_name, out, ps, wrong = skc.MUTATIONS[name]
    row = skc.ROWS_BY_NAME[row_name]
    d = row.data(ps)
    want, bound = skc.reference(row, d)[out]
    got = wrong(row, d, out)
    r = skc.worst_ratio(got.reshape(want.shape), want, bound, fp16=_is16(row.entry, out))
    print(f"[mutation] {name} on {row_name} / {ps}: {r:.3e} of the bound")
    assert r > 1.0, name


def test_grid_stride_tail_left_unwritten_falls_outside():
    rows = skc.grid_stride_rows()
    assert {r.entry for r in rows} >= {"add", "scale", "quick_gelu", "act_gelu", "act_relu", "geglu_fwd", "geglu_bwd", "cfg_ddim", "cfg_multistep"}
    row = skc.ROWS_BY_NAME[f"add:n={skc.N_STRIDE}:inplace="]
    assert row.n // 8 > skc.GRID_VECS                      # the loop iterates
    d = row.data("plain")
    want, bound = skc.reference(row, d)["y"]
    got = skc.emulate(row, d)["y"]
    got[-24:] = skc.SENT16                                # the last three vectors keep the sentinel
    assert skc.worst_ratio(got, want, bound, fp16=True) > 1.0
