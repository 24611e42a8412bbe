"""The range plan of lgd_amd/vae.py where there is no GPU: RangePlan.from_peaks against known answers; the plan's
semantics restated in torch fp64 from RangePlan.ops alone (exact in real arithmetic; with fp16-rounded storage the hot
nets are lost without a plan and finite with one); every launch-contract refusal of lgd_range_f16 answered by the built
library before the device; the rule that picks a VAE's plan; and that no plan and uniform(0) pack the same operands."""
import ctypes
import os
import sys

import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import _lib, vae
from lgd_amd.vae import RangePlan, Site

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_range_cases as rc  # noqa: E402

ERR_ARG, ERR_LAUNCH, ERR_UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__ as ge
    ge.build()


# ---------------------------------------------------------------------------------------------
# from_peaks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("peak,bits,want", [
    (0.0, 4, 0), (1.0, 4, 0), (4096.0, 4, 0), (4096.5, 4, 1), (8192.0, 4, 1), (8193.0, 4, 2), (5.3e5, 4, 8),
    (65504.0 * 256, 4, 12), (2.0 ** 36, 4, 24),
    (0.0, 0, 0), (65536.0, 0, 0), (65537.0, 0, 1), (5.3e5, 0, 4), (2.0 ** 20, 0, 4), (2.0 ** 20 + 1, 0, 5)])
def test_exponent_known_answers(peak, bits, want):
    k = RangePlan.exponent(peak, bits)
    assert k == want
    assert peak / 2.0 ** k <= 2.0 ** (16 - bits) and (k == 0 or peak / 2.0 ** (k - 1) > 2.0 ** (16 - bits))


def test_from_peaks_takes_segment_and_resnet_maxima():
    a, b, r = "decoder.conv_in", "decoder.up_blocks.0.upsamplers.0.conv", "decoder.mid_block.resnets.0"
    peaks = {Site("stream", a, a): 5000.0, Site("stream", a, r): 3.0e5, Site("stream", a, "decoder.mid_block.attentions.0"): 9.0e4,
             Site("stream", b, b): 0.0, Site("inner", r, r + ".conv1"): 1.0e6, Site("inner", "x", "x.conv1"): 4096.0,
             Site("free", "att", "att.a"): 1.0e9}                                  # a free site carries no scale
    p = RangePlan.from_peaks(peaks)
    assert p == RangePlan({a: 7, b: 0}, {r: 8, "x": 0}) and p.default == 0
    assert RangePlan.from_peaks(peaks, headroom_bits=0) == RangePlan({a: 3, b: 0}, {r: 4, "x": 0})
    assert p.segment(a) == 7 and p.segment("elsewhere") == 0 and p.resnet(r) == 8 and not p.is_identity()
    assert RangePlan.from_peaks({}).is_identity() and RangePlan.uniform(0).is_identity() and RangePlan() == RangePlan.uniform(0)
    u = RangePlan.uniform(8)
    assert u.segment("anything") == 8 and u.resnet("anything") == 8 and not u.is_identity()
    for bad in (-1, 25, 1.0, True):
        with pytest.raises(ValueError, match="range exponent"):
            RangePlan.uniform(bad)
    for bad in (float("inf"), float("nan"), -1.0):
        with pytest.raises(ValueError, match="finite magnitude"):
            RangePlan.exponent(bad)


def test_segments_start_where_the_issue_says():
    """conv_in, every sampler convolution and every resnet with a conv_shortcut start a segment; the rest stay."""
    sd = rc.nets()["benign"]
    for part, sampler in (("decoder", "up_blocks.{}.upsamplers.0.conv"), ("encoder", "down_blocks.{}.downsamplers.0.conv")):
        layout = vae.stream_layout(sd, part)
        rs = RangePlan().ops(layout)
        starts = [f"{part}.conv_in"] + [f"{part}." + sampler.format(i) for i in range(3)] + \
                 [n for n in (k[:-len(".conv_shortcut.weight")] for k in sd if k.endswith("conv_shortcut.weight")) if n.startswith(part)]
        assert len(starts) == 5
        assert {r.seg_out for r in rs.values() if r.kind != "norm_out"} == set(starts)
        for kind, n in layout:
            assert (rs[n].seg_out == n) == (n in starts), n
            if n not in starts:
                assert rs[n].seg_out == rs[n].seg_in and rs[n].k_out == rs[n].k_in
        sites = vae.sites_of(layout)
        assert len(sites) == len(set(sites)) == len(layout) + sum(k.startswith("res") for k, _ in layout) + 1
        assert [s.name for s in sites if s.kind == "free"] == [f"{part}.mid_block.attentions.0.a"]


# ---------------------------------------------------------------------------------------------
# plan semantics, restated from RangePlan.ops alone
# ---------------------------------------------------------------------------------------------
def _non_uniform(part):
    layout = vae.stream_layout(rc.nets()["benign"], part)
    segs = [n for k, n in layout if k in ("conv_in", "sampler", "res_sc")]
    ress = [n for k, n in layout if k.startswith("res")]
    return RangePlan({n: (9, 3, 0, 11, 6)[i % 5] for i, n in enumerate(segs)}, {n: (5, 0, 12, 2)[i % 4] for i, n in enumerate(ress)}, default=1)


PARTS = [("decoder", rc.latent), ("encoder", rc.image)]


@pytest.mark.parametrize("part,x", PARTS, ids=["decoder", "encoder"])
def test_scaled_forward_is_the_unscaled_one_in_fp64(part, x):
    sd = rc.nets()["benign"]
    with torch.no_grad():
        plain = rc.forward(sd, part, x().double())
        # the helper's unscaled forward is the oracle's
        ref = rc.X.vae_decode({k: v.double() for k, v in sd.items()}, x().double()) if part == "decoder" else \
            torch.cat(rc.X.vae_encode_moments({k: v.double() for k, v in sd.items()}, x().double()), dim=1)
        assert rc.rel_l2(plain.clamp(-30, 20) if part == "encoder" else plain, ref) <= 1e-12
        for plan in (_non_uniform(part), RangePlan.uniform(9), RangePlan({}, {}, 5)):
            assert rc.rel_l2(rc.forward(sd, part, x().double(), plan=plan), plain) <= 1e-12, plan


@pytest.mark.parametrize("part,x", PARTS, ids=["decoder", "encoder"])
def test_fp16_storage_needs_the_plan_on_the_hot_net(part, x):
    sd = rc.nets()["hot_" + part]
    peaks = {}
    with torch.no_grad():
        exact = rc.forward(sd, part, x().double(), peaks=peaks)
        assert max(peaks.values()) > 4 * rc.FP16_MAX
        lost = rc.forward(sd, part, x().double(), store=rc.fp16_store)
        assert not bool(torch.isfinite(lost).all())
        fitted = RangePlan.from_peaks(peaks)
        assert not fitted.is_identity() and max(fitted.segments.values()) >= 6 and max(fitted.inner.values()) >= 6
        for plan in (RangePlan.uniform(8), fitted):
            seen = {}
            y = rc.forward(sd, part, x().double(), plan=plan, store=rc.fp16_store, peaks=seen)
            assert bool(torch.isfinite(y).all()), plan
            err = rc.rel_l2(y, exact)
            print(f"[measured] hot {part} under {'uniform(8)' if plan is not fitted else 'from_peaks'}: rel-L2 {err:.3e} against fp64")
            assert err < 2 ** -8                     # fp16 storage: 2^-11 per rounding, a few dozen roundings deep
        # the fitted plan stores every peak of these inputs at or below 2^12 (seen holds true magnitudes of the fp16-stored
        # run, the plan was fitted to the fp64 ones: they differ by the rounding error bounded above)
        ops = fitted.ops(vae.stream_layout(sd, part))
        for site, p in seen.items():
            k = 0 if site.kind == "free" else ops[site.key].j if site.kind == "inner" else ops[site.name].k_out
            assert p / 2.0 ** k <= 2.0 ** 12 * (1 + 2 ** -8), (site, p, k)


# ---------------------------------------------------------------------------------------------
# lgd_range_f16: refusals, answered before the device
# ---------------------------------------------------------------------------------------------
X0, OUT0 = 0x10000000, 0x20000000                  # placeholder addresses: a refusal never reads them
BASE = dict(x=X0, rows=5, cols=24, ld=40, out2=OUT0)
REFUSALS = [
    ("x NULL", dict(x=0), ERR_ARG), ("out2 NULL", dict(out2=0), ERR_ARG),
    ("rows = 0", dict(rows=0), ERR_ARG), ("rows = -1", dict(rows=-1), ERR_ARG),
    ("cols = 0", dict(cols=0), ERR_ARG), ("cols = -1", dict(cols=-1), ERR_ARG),
    ("ld < cols", dict(ld=23), ERR_ARG), ("ld = 0", dict(ld=0), ERR_ARG),
    ("x off 1 byte", dict(x=X0 + 1), ERR_ARG), ("out2 off 2 bytes", dict(out2=OUT0 + 2), ERR_ARG),
    ("out2 off 1 byte", dict(out2=OUT0 + 1), ERR_ARG),
    ("out2 at the start of x", dict(out2=X0), ERR_ARG),
    ("out2 in the padding of x", dict(out2=X0 + 2 * 32), ERR_ARG),
    ("out2 on the last element of x", dict(out2=X0 + 2 * (4 * 40 + 22)), ERR_ARG),
    ("out2 ends where x starts, one word short", dict(out2=X0 - 4), ERR_ARG),
    ("rows * ld beyond the address space", dict(rows=1 << 30, cols=8, ld=1 << 40), ERR_ARG),
    ("2^40 + 2^20 elements", dict(rows=(1 << 20) + 1, cols=1 << 20, ld=1 << 20, out2=8), ERR_UNSUPPORTED),
    ("2^62 elements", dict(rows=1 << 31, cols=1 << 31, ld=1 << 31, out2=8), ERR_UNSUPPORTED),
]


def _answer(change):
    a = dict(BASE, **change)
    return _lib.load().lgd_range_f16(a["x"], a["rows"], a["cols"], a["ld"], a["out2"], None)


@pytest.mark.parametrize("what,change,want", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_range_f16_refusals(what, change, want):
    assert _lib.SIGNATURES["lgd_range_f16"] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                                ctypes.c_void_p]
    assert _answer(change) == want
    if not torch.cuda.is_available():
        # the unchanged call passes every check: without a device it gets as far as the launch, and fails there
        assert _answer({}) == ERR_LAUNCH
        assert _answer(dict(out2=X0 - 8)) == ERR_LAUNCH and _answer(dict(out2=X0 + 2 * (4 * 40 + 24))) == ERR_LAUNCH


def test_range_f16_wrapper_refusals():
    from lgd_amd import ops
    t = torch.zeros((3, 2), dtype=torch.int32)
    for x, tab, site, msg in [(torch.zeros(4, 4), t, 0, "reads fp16 rows"), (torch.zeros(16, dtype=torch.float16), t, 0, "reads fp16 rows"),
                              (torch.zeros((4, 8), dtype=torch.float16)[:, ::2], t, 0, "reads fp16 rows"),
                              (torch.zeros((4, 4), dtype=torch.float16), t.float(), 0, "table is torch.float32"),
                              (torch.zeros((4, 4), dtype=torch.float16), t, 3, "no pair 3"),
                              (torch.zeros((4, 4), dtype=torch.float16), t, -1, "no pair -1"),
                              (torch.zeros((4, 4), dtype=torch.float16), t.view(2, 3), 0, "no pair 0")]:
        with pytest.raises(RuntimeError, match=msg):
            ops.range_f16(x, tab, site)


# ---------------------------------------------------------------------------------------------
# which plan a VAE gets
# ---------------------------------------------------------------------------------------------
class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("flag", [None, False, True])
@pytest.mark.parametrize("override", [None, RangePlan.uniform(3)])
@pytest.mark.parametrize("env", [{}, {"LGD_SDXL_VAE_FP16": "1"}, {"LGD_SDXL_VAE_FP16": ""}])
def test_vae_ranges_rule(flag, override, env):
    sys.path.insert(0, os.path.join(rc.ROOT, "llm-groundeddiffusion_amd", "dropin"))
    from generation.sdxl_refinement import _vae_ranges
    want = None if env.get("LGD_SDXL_VAE_FP16") else override if override is not None else RangePlan.uniform(8) if flag else None
    for cfg in (_Cfg(**({} if flag is None else dict(force_upcast=flag))), {} if flag is None else dict(force_upcast=flag)):
        got = _vae_ranges(cfg, override, env)
        assert got == want and (got is override or override is None or want is None)
    assert vae.FORCE_UPCAST_EXPONENT == 8


def test_the_flag_no_longer_refuses_and_the_backstops_name_the_remedy():
    import inspect

    from lgd_amd import sdxl
    sys.path.insert(0, os.path.join(rc.ROOT, "llm-groundeddiffusion_amd", "dropin"))
    from generation import sdxl_refinement as sr
    assert "raise" not in inspect.getsource(sr.from_diffusers)
    assert "vae_ranges" in inspect.signature(sr.from_diffusers).parameters
    assert "vae_ranges" in inspect.signature(sdxl.build_synthetic).parameters
    src = inspect.getsource(sdxl.SDXLRefiner.refine)
    assert src.count("non-finite") == 2 and src.count("vae_ranges") == 2 and src.count("calibrate_ranges") == 2


# ---------------------------------------------------------------------------------------------
# constructors
# ---------------------------------------------------------------------------------------------
def _tensors(obj, path=""):
    if torch.is_tensor(obj):
        yield path, obj
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            yield from _tensors(obj[k], f"{path}.{k}")
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _tensors(v, f"{path}[{i}]")
    elif hasattr(obj, "__dict__") and not isinstance(obj, type) and type(obj).__module__ in ("types", vae.__name__):
        if not isinstance(obj, RangePlan):
            yield from _tensors({k: v for k, v in vars(obj).items() if k not in ("ops", "ranges")}, path)


def _scalars(rs):
    return {n: {k: v for k, v in vars(r).items() if isinstance(v, (int, float, tuple, str, type(None)))} for n, r in rs.items()}


@pytest.mark.parametrize("cls", [vae.HipVAEDecoder, vae.HipVAEEncoder, vae.HipVAE])
def test_no_plan_and_uniform_zero_pack_identical_operands(cls):
    sd = rc.nets()["benign"]
    none, zero = cls(sd, "cpu"), cls(sd, "cpu", ranges=RangePlan.uniform(0))
    halves = [(none, zero)] + ([(none.encoder, zero.encoder)] if cls is vae.HipVAE else [])
    for a, b in halves:
        ta, tb = dict(_tensors(a)), dict(_tensors(b))
        assert len(ta) > 40 and sorted(ta) == sorted(tb)
        for k in ta:
            assert ta[k].dtype == tb[k].dtype and torch.equal(ta[k], tb[k]), k
        assert _scalars(a.rs) == _scalars(b.rs) and a.eps == b.eps
        for r in a.rs.values():                          # every factor is one, and no bias was rebuilt
            assert all(v == 1.0 for k, v in vars(r).items() if k in ("alpha", "a1", "a2", "a_out", "eps", "eps1", "eps2", "bias"))
            assert getattr(r, "sc_bias", None) is None and getattr(r, "bias_t", None) is None
            assert r.kind != "res_sc" or r.sc == (1.0, 1.0)
        if hasattr(a, "_bias_map"):
            assert torch.equal(a._bias_map(2, 8, 8), b._bias_map(2, 8, 8))


def test_a_plan_reaches_both_halves_and_scales_the_right_operands():
    sd = rc.nets()["benign"]
    plan = RangePlan({"decoder.conv_in": 3, "decoder.up_blocks.2.resnets.0": 1, "encoder.conv_in": 2, "encoder.down_blocks.2.resnets.0": 4},
                     {"decoder.mid_block.resnets.0": 5})
    v, plain = vae.HipVAE(sd, "cpu", ranges=plan), vae.HipVAE(sd, "cpu")
    assert v.ranges is plan and v.encoder.ranges is plan
    assert vae.HipVAE.from_state_dict(sd, "cpu", ranges=plan).ranges is plan
    # the folded bias map: built in fp32 at 2^-3 and rounded once (an inner pixel: all nine taps carry post_quant_conv's bias)
    inner = torch.einsum("okl,ky,lx->yxo", torch.einsum("ockl,c->okl", sd["decoder.conv_in.weight"], sd["post_quant_conv.bias"]),
                         torch.ones(3, 1), torch.ones(3, 1))[0, 0] + sd["decoder.conv_in.bias"]
    assert torch.equal(v._bias_map(1, 4, 4).view(4, 4, -1)[1, 2], (inner * 0.125).half())
    assert torch.equal(plain._bias_map(1, 4, 4).view(4, 4, -1)[1, 2], inner.half())
    r = v.rs["decoder.up_blocks.2.resnets.0"]            # reads the segment of the sampler before it (0), writes its own (1)
    assert (r.k_in, r.k_out, r.sc, r.sc_bias) == (0, 1, (0.5, 1.0), None)
    s = v.rs["decoder.up_blocks.0.upsamplers.0.conv"]    # reads conv_in's segment (3), writes its own (0)
    assert (s.k_in, s.k_out, s.alpha, s.bias) == (3, 0, 8.0, 0.125)
    assert torch.equal(s.bias_t, sd["decoder.up_blocks.0.upsamplers.0.conv.bias"] * 0.125)
    m = v.rs["decoder.mid_block.resnets.0"]
    assert (m.eps1, m.a1, m.eps2, m.a2) == (2.0 ** -6, 2.0 ** -5, 2.0 ** -10, 2.0 ** -3)
    a = v.rs["decoder.mid_block.attentions.0"]
    assert (a.eps, a.a_out) == (2.0 ** -6, 2.0 ** -3)
    e = v.encoder.rs["encoder.down_blocks.2.resnets.0"]  # reads the sampler's segment (0), writes its own (4)
    assert (e.k_in, e.k_out, e.sc) == (0, 4, (2.0 ** -4, 1.0))
    d = v.encoder.rs["encoder.down_blocks.2.downsamplers.0.conv"]
    assert (d.k_in, d.k_out, d.alpha, d.bias) == (4, 0, 16.0, 2.0 ** -4) and v.encoder.rs["norm_out"].eps == 1.0
    assert vae.HipVAEEncoder(sd, "cpu", ranges=RangePlan.uniform(4)).rs["norm_out"].eps == 2.0 ** -8
    with pytest.raises(TypeError, match="RangePlan or None"):
        vae.HipVAEDecoder(sd, "cpu", ranges=8)
    with pytest.raises(ValueError, match="decoder.mid_block.resnets.0, which is no segment of this decoder"):
        vae.HipVAEDecoder(sd, "cpu", ranges=RangePlan({"decoder.mid_block.resnets.0": 2}))      # identity residual: no start
    with pytest.raises(ValueError, match="encoder.conv_in, which is no resnet of this encoder"):
        vae.HipVAE(sd, "cpu", ranges=RangePlan({}, {"encoder.conv_in": 2})).encoder
