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
    assert set(skc.ARGS) == set(skc.BASE) == set(skc.RULES) and len(skc.ARGS) == 23
    labels = {}
    for fn, what, change in skc.REFUSALS:
        assert set(change) <= {n[2:] if n.startswith("p:") else n for n in skc.ARGS[fn].split()}, (fn, what)
        assert what not in labels.setdefault(fn, set()), (fn, what)
        labels[fn].add(what)
    for fn, args in skc.ARGS.items():
        names = args.split()
        assert len(names) == len(_lib.SIGNATURES[fn]), fn
        ptrs = skc.pointers(fn)
        want = {f"{p} NULL" for p in ptrs if p not in skc.optional(fn)}
        want |= {f"{p} off {skc.ALIGN[fn][p]} bytes" for p in ptrs}
        counts = [n for n in names if n in ("n", "rows", "B", "H", "W", "L", "HW", "C", "Cin", "reps")]
        want |= {f"{c} = {v}" for c in counts for v in (0, -1)}
        assert want <= labels[fn], (fn, sorted(want - labels[fn]))
        assert skc.NEEDS[fn] <= {cls for cls, _, _ in skc.RULES[fn]}, fn
        vec = [p for p in ptrs if skc.ALIGN[fn][p] == 16]
        for cls, what, ch in skc.RULES[fn]:              # an alias row is refused for the overlap, not for its alignment or its form
            if cls == "alias":
                moved = {k: v for k, v in ch.items() if isinstance(v, tuple)}
                assert moved and all(v[1] % skc.ALIGN[fn][k] == 0 for k, v in moved.items()), (fn, what)
                assert set(ch) - set(moved) <= {"prep"}, (fn, what)       # test_alias_rows_change_a_served_form
        assert fn in ("lgd_cfg_ddim_step_f32", "lgd_cfg_multistep_step_f32", "lgd_axpy_f32", "lgd_select_row_f32",
                      "lgd_scale_rows_f32", "lgd_conv_in_f16", "lgd_sam_relpos_qkv_f16") or vec, fn
    step = {w for f, w, _ in skc.REFUSALS if f == "lgd_cfg_ddim_step_f32"}
    assert {"frozen_ref without mask", "mask without frozen_ref"} <= step
    assert {"col 4", "col -1", "per_sample -1", "n % per_sample with active"} <= labels["lgd_axpy_f32"]
    assert {"V != nbh nbw", "v0 + nv > V", "nvc < nv", "Wp % 4", "Hp < 64", "C > 64", "a multi-chunk call without value",
            "normalization without count", "bootstrapping without picks"} <= labels["lgd_multidiffusion_views_f32"]
    assert {"Pp < P", "prep = 2", "HW % 4"} <= labels["lgd_multidiffusion_step_f32"]
    assert {"DA < d + 2S", "window = 0 with Hs != Ws", "d % 8", "scale = 0", "scale = NaN"} <= labels["lgd_sam_relpos_qkv_f16"]
    assert {f for f, _, _ in skc.UNSUPPORTED} >= {"lgd_sam_relpos_qkv_f16"}
    # the calls a probe of the parent commit saw reach the launch
    assert {"qkv NULL", "ka is qa"} <= labels["lgd_sam_relpos_qkv_f16"]
    assert {"out NULL", "oa off by 2 bytes", "out is oa"} <= labels["lgd_sam_window_merge_f16"]
    assert {"x_out 64 bytes into x", "cur_sample is x", "ets inside eps", "coef_table off 4 bytes"} <= labels["lgd_cfg_plms_step_f32"]
    assert "out is moments" in labels["lgd_vae_sample_f32"] and "y is img" in labels["lgd_image_u8_to_nhwc8_f16"]


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


def test_alias_rows_change_a_served_form():
    """An alias row that also switches the form (views: prep = 1) overlaps operands of a call the library serves."""
    if torch.cuda.is_available():
        pytest.skip("the placeholder pointers would be launched on")
    forms = {(fn, tuple(sorted((k, v) for k, v in ch.items() if not isinstance(v, tuple))))
             for fn in skc.RULES for cls, _, ch in skc.RULES[fn] if cls == "alias"}
    assert any(form for _, form in forms)
    for fn, form in forms:
        assert _answer(fn, dict(form)) == ERR_LAUNCH, (fn, form)


def test_optional_operands_stay_optional():
    """bias; hist; frozen_ref and mask together; active; eps with prep; bg, noise and picks with one prompt; value and count with
    one chunk: NULL passes every check (host without a GPU: the launch is reached)."""
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
                       ("lgd_cfg_ddim_step_f32", dict(x_out=("x", 0))), ("lgd_cfg_multistep_step_f32", dict(x_out=("x", 0))),
                       ("lgd_cfg_plms_step_f32", dict(x_out=("x", 0))), ("lgd_cfg_plms_step_f32", dict(hist=None)),
                       ("lgd_cfg_multistep_step_f32", dict(hist=None)), ("lgd_multidiffusion_step_f32", dict(hist=None)),
                       ("lgd_multidiffusion_views_f32", dict(hist=None)), ("lgd_multidiffusion_step_f32", dict(prep=1, eps=None)),
                       ("lgd_multidiffusion_step_f32", dict(P=1, Pp=1, bg=None, noise=None, picks=None)),
                       ("lgd_multidiffusion_step_f32", dict(n_boot=0, bg=None, noise=None, picks=None)),
                       ("lgd_multidiffusion_views_f32", dict(nv=4, nvc=4, value=None, count=None)),
                       ("lgd_multidiffusion_views_f32", dict(normalization=0, count=None)),
                       ("lgd_multidiffusion_views_f32", dict(bg=None, noise=None, picks=None)),
                       ("lgd_multidiffusion_views_f32", dict(prep=1, eps=None, value=None, count=None, hist=None)),
                       ("lgd_multidiffusion_views_f32", dict(prep=1, P=1, Pp=1, bg=None, noise=None, picks=None)),
                       ("lgd_multidiffusion_views_f32", dict(v0=2)), ("lgd_multidiffusion_views_f32", dict(nvc=3, nv=3))):
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
        ("cfg_plms_step: ets count", lambda: ops.cfg_plms_step(f(4, 4, 4, 4), x4, x4, f(2, 2, 4, 4, 4), f(2, 4, 4, 4), f(7, 16), i(4))),
        ("cfg_plms_step: table width", lambda: ops.cfg_plms_step(f(4, 4, 4, 4), x4, x4, f(3, 2, 4, 4, 4), f(2, 4, 4, 4), f(7, 10), i(4))),
        ("cfg_plms_step: cur_sample dtype", lambda: ops.cfg_plms_step(f(4, 4, 4, 4), x4, x4, f(3, 2, 4, 4, 4), h(2, 4, 4, 4), f(7, 16), i(4))),
        ("cfg_plms_step: eps strided", lambda: ops.cfg_plms_step(f(4, 4, 4, 8)[..., :4], x4, x4, f(3, 2, 4, 4, 4), f(2, 4, 4, 4), f(7, 16), i(4))),
        ("multidiffusion_step: eps count", lambda: ops.multidiffusion_step(f(2, 4, 4, 4), f(4, 4, 4, 4), f(4, 4, 4), f(2, 16), f(4, 4), i(4), n_prompts=2, n_steps=4)),
        ("multidiffusion_step: masks rows", lambda: ops.multidiffusion_step(f(4, 4, 4, 4), f(4, 4, 4, 4), f(4, 4, 4), f(1, 16), f(4, 4), i(4), n_prompts=2, n_steps=4)),
        ("multidiffusion_step: latent is no row", lambda: ops.multidiffusion_step(f(4, 4, 4, 4), f(4, 4, 4, 4), f(4, 4, 2), f(2, 16), f(4, 4), i(4), n_prompts=2, n_steps=4)),
        ("multidiffusion_step: picks dtype", lambda: ops.multidiffusion_step(f(4, 4, 4, 4), f(4, 4, 4, 4), f(4, 4, 4), f(2, 16), f(4, 4), i(4), n_prompts=2, n_steps=4,
                                                                              bg=f(2, 4, 4, 4), noise=f(4, 4, 4), picks=torch.zeros(4, 1, dtype=torch.int64), n_boot=2)),
        ("multidiffusion_step: bg rows", lambda: ops.multidiffusion_step(f(4, 4, 4, 4), f(4, 4, 4, 4), f(4, 4, 4), f(2, 16), f(4, 4), i(4), n_prompts=2, n_steps=4,
                                                                          bg=f(1, 4, 4, 4), noise=f(4, 4, 4), picks=i(4, 1), n_boot=2)),
        ("multidiffusion_views: value count", lambda: ops.multidiffusion_views(f(4, 1, 64, 64), f(4, 1, 64, 64), f(1, 72, 72), f(1, 72, 64), None, f(2, 72, 72), f(4, 4), i(4),
                                                                                n_prompts=2, rows_per_view=2, n_views=4, v0=0, nv=1, n_steps=4)),
        ("multidiffusion_views: window", lambda: ops.multidiffusion_views(f(4, 1, 32, 32), f(4, 1, 32, 32), f(1, 72, 72), None, None, f(2, 72, 72), f(4, 4), i(4),
                                                                           n_prompts=2, rows_per_view=2, n_views=4, v0=0, nv=1, n_steps=4)),
        ("multidiffusion_views: masks dtype", lambda: ops.multidiffusion_views(f(4, 1, 64, 64), f(4, 1, 64, 64), f(1, 72, 72), None, None, h(2, 72, 72), f(4, 4), i(4),
                                                                                n_prompts=2, rows_per_view=2, n_views=4, v0=0, nv=1, n_steps=4)),
        ("image_u8_to_nhwc8: dtype", lambda: ops.image_u8_to_nhwc8(f(2, 5, 10, 3))),
        ("image_u8_to_nhwc8: channels", lambda: ops.image_u8_to_nhwc8(torch.zeros(2, 5, 10, 4, dtype=torch.uint8))),
        ("image_u8_to_nhwc8: strided", lambda: ops.image_u8_to_nhwc8(torch.zeros(2, 5, 20, 3, dtype=torch.uint8)[:, :, :10])),
        ("vae_sample: moments count", lambda: ops.vae_sample(h(40, 4), f(2, 4, 4, 5), 1.0)),
        ("vae_sample: noise dtype", lambda: ops.vae_sample(h(40, 8), h(2, 4, 4, 5), 1.0)),
        ("vae_sample: out count", lambda: ops.vae_sample(h(40, 8), f(2, 4, 4, 5), 1.0, f(2, 4, 4, 4))),
        ("sam_relpos_qkv: qkv count", lambda: ops.sam_relpos_qkv(h(70, 24), f(48), f(5, 8), f(5, 8), 2, 5, 7, 3, 2, 8, 16, 0.35)),
        ("sam_relpos_qkv: rel_h rows", lambda: ops.sam_relpos_qkv(h(70, 48), f(48), f(6, 8), f(5, 8), 2, 5, 7, 3, 2, 8, 16, 0.35)),
        ("sam_relpos_qkv: qa count", lambda: ops.sam_relpos_qkv(h(70, 48), f(48), f(5, 8), f(5, 8), 2, 5, 7, 3, 2, 8, 16, 0.35, qa=h(70, 32))),
        ("sam_relpos_qkv: bias dtype", lambda: ops.sam_relpos_qkv(h(70, 48), h(48), f(5, 8), f(5, 8), 2, 5, 7, 3, 2, 8, 16, 0.35)),
        ("sam_window_merge: oa count", lambda: ops.sam_window_merge(h(70, 32), 2, 5, 7, 3, 2, 8, 16)),
        ("sam_window_merge: out strided", lambda: ops.sam_window_merge(h(108, 32), 2, 5, 7, 3, 2, 8, 16, out=h(70, 32)[:, :16])),
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
                     "boxdiff_energy", "cfg_plms_step", "multidiffusion_step", "multidiffusion_views", "image_u8_to_nhwc8", "vae_sample",
                     "sam_relpos_qkv", "sam_window_merge"}


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


def test_views_chunkings_share_one_panorama():
    """The GPU suite asks every chunking of a views form for the same latent bits: the rows that differ only in nvc hold the same
    logical operands, and all three chunkings of V = 4 (one chunk, two of 2, 3 and a short last one) are among them."""
    groups = {}
    for row in skc.rows_of("md_views"):
        if not row.prep:
            groups.setdefault(skc.ENTRIES["md_views"].key(row), []).append(row)
    assert sum(1 for g in groups.values() if {r.nvc for r in g} == {4, 2, 3}) == 4
    assert any({r.nvc for r in g} == {2, 1} for g in groups.values())
    for g in groups.values():
        first = g[0].data("plain")
        for row in g[1:]:
            d = row.data("plain")
            assert all(torch.equal(d[n].view(torch.int32), first[n].view(torch.int32)) for n in ("eps_l", "xin_l", "masks")), row.name


def test_grid_stride_tail_left_unwritten_falls_outside():
    rows = skc.grid_stride_rows()
    assert {r.entry for r in rows} >= {"add", "scale", "quick_gelu", "act_gelu", "act_relu", "geglu_fwd", "geglu_bwd", "cfg_ddim", "cfg_multistep",
                                       "cfg_plms", "image_u8", "vae_sample"}
    for entry, vecs in (("cfg_plms", lambda r: r.B * r.C * r.HW // 4), ("image_u8", lambda r: r.B * r.HW // 4),
                        ("vae_sample", lambda r: r.B * (r.z // 4) * (r.HW // 4))):
        assert [r for r in rows if r.entry == entry and vecs(r) > skc.GRID_VECS], entry      # the loop iterates
    row = skc.ROWS_BY_NAME[f"add:n={skc.N_STRIDE}:inplace="]
    assert row.n // 8 > skc.GRID_VECS                      # the loop iterates
    d = row.data("plain")
    want, bound = skc.reference(row, d)["y"]
    got = skc.emulate(row, d)["y"]
    got[-24:] = skc.SENT16                                # the last three vectors keep the sentinel
    assert skc.worst_ratio(got, want, bound, fp16=True) > 1.0
