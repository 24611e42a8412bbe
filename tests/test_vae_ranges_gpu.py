"""The range plan of lgd_amd/vae.py on the GPU: lgd_range_f16 against torch (both words, exactly); no plan and uniform(0)
bit for bit; what the scaling costs on a benign net; the hot nets (tests/vae_range_cases.py), which are lost without a plan,
against the fp32 restatement with one; the condition calibrate_ranges guarantees, re-probed; and the refiner end to end on
a hot VAE."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lgd_amd  # noqa: E402,F401
from conftest import gate  # noqa: E402
from lgd_amd import ops, vae  # noqa: E402
from lgd_amd.vae import RangePlan  # noqa: E402
import vae_range_cases as rc  # noqa: E402

F16, I32 = torch.float16, torch.int32
INF, NAN = float("inf"), float("nan")
SUB = 2.0 ** -24                                     # the smallest fp16 subnormal


# ---------------------------------------------------------------------------------------------
# lgd_range_f16
# ---------------------------------------------------------------------------------------------
def _want(x):
    """(bits of the fp32 value of the largest finite |x|, number of non-finite elements) of the logical matrix x."""
    x = x.float().cpu()
    fin = torch.isfinite(x)
    top = x[fin].abs().max() if bool(fin.any()) else torch.zeros(())
    return int(top.reshape(1).view(I32)), int((~fin).sum())


def _got(table, site=0):
    torch.cuda.synchronize()
    t = table.cpu()
    return int(t[site, 0]), int(t[site, 1]) & 0xffffffff


def _rand(shape, seed, dev):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).half().to(dev)


def _planted(dev, rows, cols, seed, plants, base=None):
    x = _rand((rows, cols), seed, dev) if base is None else torch.full((rows, cols), base, dtype=F16, device=dev)
    flat = x.view(-1)
    n = flat.numel()
    for where, vals in zip((0, n // 2 - len(plants) // 2, n - len(plants)), (plants, plants, plants)):
        flat[where:where + len(vals)] = torch.tensor(vals, dtype=F16, device=dev)
    return x


def _cases(dev):
    out = {}
    out["1x1"] = torch.tensor([[-3.5]], dtype=F16, device=dev)
    out["1x1 NaN"] = torch.tensor([[NAN]], dtype=F16, device=dev)
    out["3x7, odd base offset"] = _rand((22,), 1, dev)[1:].view(3, 7)
    pad = torch.full((5, 40), NAN, dtype=F16, device=dev)
    pad[:, :24] = _rand((5, 24), 2, dev)
    out["5x24 in ld = 40, NaN in the padding"] = pad[:, :24]
    pad2 = torch.full((5, 40), INF, dtype=F16, device=dev)
    pad2[:, :23] = _rand((5, 23), 3, dev)
    pad2[3, 22] = -INF
    out["5x23 in ld = 40 (element loads)"] = pad2[:, :23]
    out["5x24 in ld = 40, base off 8 bytes (element loads)"] = torch.cat([pad.view(-1), pad.view(-1)])[4:4 + 200].view(5, 40)[:, :24]
    out["1031x264 planted"] = _planted(dev, 1031, 264, 4, [INF, -INF, NAN, -65504.0, SUB, -3 * SUB])
    out["1031x264 subnormals only"] = _planted(dev, 1031, 264, 5, [SUB, -5 * SUB, 1023 * SUB, 0.0], base=0.0)
    out["1031x264 nothing finite"] = _planted(dev, 1031, 264, 6, [INF, -INF, NAN], base=NAN)
    out["all zeros"] = torch.zeros((64, 64), dtype=F16, device=dev)
    out["negative zeros"] = torch.full((3, 8), -0.0, dtype=F16, device=dev)
    big = _rand((2048, 2048), 7, dev)                                   # 2^22 elements
    big[2047, 2047], big[1024, 5] = 77.0, NAN
    out["2^22 elements"] = big
    huge = _rand((6144, 2048), 8, dev) * 0.5                            # 3 * 2^22: several passes of the full grid
    huge[6143, 2040:] = torch.tensor([99.0, -INF, NAN, 1.0, 2.0, -101.0, INF, 3.0], dtype=F16, device=dev)
    out["3 * 2^22 elements, the top in the last vector"] = huge
    wide = torch.zeros((40000, 72), dtype=F16, device=dev)              # padded rows, more vectors than one pass of 2^18
    wide[:, :64] = _rand((40000, 64), 9, dev)
    wide[:, 64:] = NAN
    wide[39999, 63], wide[17, 0] = -1234.0, INF
    out["40000x64 in ld = 72"] = wide[:, :64]
    return out


def test_range_f16_against_torch(dev):
    cases = _cases(dev)
    table = torch.zeros((len(cases), 2), dtype=I32, device=dev)
    for i, x in enumerate(cases.values()):
        ops.range_f16(x, table, i)
    torch.cuda.synchronize()
    host = table.cpu()
    for i, (name, x) in enumerate(cases.items()):
        assert (int(host[i, 0]), int(host[i, 1]) & 0xffffffff) == _want(x), name
    # what the cases are there for
    assert _want(cases["5x24 in ld = 40, NaN in the padding"])[1] == 0 and _want(cases["1031x264 planted"]) == (0x477fe000, 9)
    assert _want(cases["1031x264 subnormals only"]) == (int(torch.tensor([1023 * SUB]).view(I32)), 0)
    assert _want(cases["1031x264 nothing finite"]) == (0, 1031 * 264) and _want(cases["all zeros"]) == (0, 0)
    assert _want(cases["3 * 2^22 elements, the top in the last vector"]) == (int(torch.tensor([101.0]).view(I32)), 3)
    assert float(host.view(torch.float32)[list(cases).index("1031x264 planted"), 0]) == 65504.0


def test_range_f16_calls_accumulate_and_the_count_saturates(dev):
    a, b = _rand((33, 40), 1, dev), _rand((7, 5), 2, dev) * 3
    a[3, 3], b[0, 0], b[6, 4] = NAN, INF, 50.0
    table = torch.zeros((3, 2), dtype=I32, device=dev)
    ops.range_f16(a, table, 1)
    assert _got(table, 1) == _want(a)
    ops.range_f16(b, table, 1)
    assert _got(table, 1) == (max(_want(a)[0], _want(b)[0]), 2)
    ops.range_f16(a, table, 1)                                          # a smaller peak changes nothing
    assert _got(table, 1) == (_want(b)[0], 3)
    assert _got(table, 0) == (0, 0) and _got(table, 2) == (0, 0)        # the neighbours are untouched
    table[2, 1] = -3                                                    # 2^32 - 3
    ops.range_f16(torch.full((1, 2), NAN, dtype=F16, device=dev), table, 2)
    assert _got(table, 2) == (0, 0xffffffff)
    ops.range_f16(torch.full((300, 8), INF, dtype=F16, device=dev), table, 2)      # two workgroups, both past the top
    assert _got(table, 2) == (0, 0xffffffff)


def test_range_f16_in_a_captured_graph(dev):
    x = _planted(dev, 257, 24, 3, [INF, 9.0, -300.0, NAN])
    table = torch.zeros((2, 2), dtype=I32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.range_f16(x, table, 0)                                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        ops.range_f16(x, table, 1)
    for n in (1, 2):
        cg.replay()
        assert _got(table, 1) == (_want(x)[0], n * _want(x)[1])
    assert _got(table, 0) == _want(x)


# ---------------------------------------------------------------------------------------------
# the VAE under a plan
# ---------------------------------------------------------------------------------------------
def _run(name, part, dev, ranges):
    sd = rc.nets()[name]
    if part == "decoder":
        return vae.HipVAEDecoder(sd, dev, ranges=ranges).decode(rc.latent()).cpu()
    return torch.cat(vae.HipVAEEncoder(sd, dev, ranges=ranges).encode_moments(rc.image()), dim=1).cpu()


def _calibrated(name, dev):
    return vae.calibrate_ranges(rc.nets()[name], dev, latents=rc.latent(), images=rc.image())


PARTS = ["decoder", "encoder"]


@pytest.mark.parametrize("part", PARTS)
def test_no_plan_is_uniform_zero_bit_for_bit(dev, part):
    a, b = _run("benign", part, dev, None), _run("benign", part, dev, RangePlan.uniform(0))
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert not torch.equal(a, _run("benign", part, dev, RangePlan.uniform(4)))         # and a plan does reach the launches


@pytest.mark.parametrize("part", PARTS)
def test_benign_net_pays_little_for_the_scaling(dev, part):
    """<= 1.25 x the error of the same run without a plan: scaling down moves small values into the fp16 subnormals, which
    the CPU emulation prices at 2-4 % of the rounding error that is there anyway."""
    ref = rc.reference("benign", part)
    plain = rc.rel_l2(_run("benign", part, dev, None), ref)
    fitted = _calibrated("benign", dev)
    print(f"[measured] benign {part}: rel-L2 without a plan {plain:.4e}; calibrated plan {fitted}")
    for label, plan in (("uniform(8)", RangePlan.uniform(8)), ("calibrated", fitted)):
        gate(f"benign {part} under {label} (x no plan)", rc.rel_l2(_run("benign", part, dev, plan), ref) / plain, 1.25)


# rel-L2 against the fp32 restatement as first measured on an MI355X, under uniform(8) and under the calibrated plan alike
# (the gates are 3 x that measurement; the CPU emulation of fp16 storage gets 5.3e-4 on these nets; DESIGN.md (c), "fp16
# range of the VAE")
HOT_MEASURED = {"decoder": 7.9009e-4, "encoder": 7.4722e-4}


@pytest.mark.parametrize("part", PARTS)
def test_hot_net_needs_the_plan_and_matches_the_restatement_with_it(dev, part):
    name = "hot_" + part
    ref = rc.reference(name, part)
    assert bool(torch.isfinite(ref).all())
    assert not bool(torch.isfinite(_run(name, part, dev, None)).all())                 # the premise: plain fp16 loses this net
    fitted = _calibrated(name, dev)
    assert not fitted.is_identity()
    print(f"[measured] {name}: calibrated plan {fitted}")
    errs = {}
    for label, plan in (("uniform(8)", RangePlan.uniform(8)), ("calibrated", fitted)):
        y = _run(name, part, dev, plan)
        assert bool(torch.isfinite(y).all()), label
        errs[label] = rc.rel_l2(y, ref)
        print(f"[measured] {name} under {label}: rel-L2 {errs[label]:.4e}")
    for label, e in errs.items():
        gate(f"{name} under {label}", e, 3 * HOT_MEASURED[part])


def test_calibration_condition_holds_when_reprobed(dev):
    """Under the plan calibrate_ranges returns, every stored tensor of the calibration inputs is finite and peaks at or
    below 2^12, and a segment or resnet with a non-zero exponent peaks above 2^10: the plan is not merely huge."""
    for name in ("hot_decoder", "hot_encoder", "benign"):
        sd = rc.nets()[name]
        plan = _calibrated(name, dev)
        seen = vae.probe_ranges(sd, dev, plan, latents=rc.latent(), images=rc.image())
        layouts = [vae.stream_layout(sd, p) for p in PARTS]
        assert list(seen) == [s for lay in layouts for s in vae.sites_of(lay)]
        tops = {}
        for site, (peak, bad) in seen.items():
            assert bad == 0, (name, site)
            if site.kind != "free":
                assert peak <= 2.0 ** 12, (name, site, peak)
                tops[(site.kind, site.key)] = max(tops.get((site.kind, site.key), 0.0), peak)
        exps = {("stream", k): v for k, v in plan.segments.items()}
        exps.update({("inner", k): v for k, v in plan.inner.items()})
        assert set(exps) == set(tops)
        for key, k in exps.items():
            assert k == 0 or tops[key] > 2.0 ** 10, (name, key, k, tops[key])
        if name == "benign":
            assert plan.is_identity()
        else:
            assert max(plan.segments.values()) >= 6 and max(plan.inner.values()) >= 6


def test_calibration_refuses_what_no_plan_can_hold(dev):
    sd = rc.heat(rc.nets()["benign"], ["decoder.conv_in"], 1.0e12)       # 65504 * 2^12 = 2.7e8 is the most exponent 12 can hold
    with pytest.raises(RuntimeError, match="non-finite values at exponent 12.*decoder.conv_in"):
        vae.calibrate_ranges(sd, dev, latents=rc.latent())
    with pytest.raises(ValueError, match="nothing to measure"):
        vae.calibrate_ranges(sd, dev)


def test_refiner_end_to_end_on_a_hot_vae(dev):
    """tiny_xl refiner, 64 x 64 image, 4 steps, the VAE hot in both halves."""
    from lgd_amd import sdxl, weights
    from lgd_amd.unet import UNetEngine
    cfg = weights.CONFIGS["tiny_xl"]
    sd = rc.heat(rc.nets()["benign"], rc.HOT_DECODER + rc.HOT_ENCODER, rc.GAIN)
    eng = UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0), max_text_batch=2)
    g = torch.Generator().manual_seed(3)
    img = torch.randn((1, 3, 64, 64), generator=g).clamp(-1, 1)
    pe, pooled = torch.randn((2, 77, cfg.cross_attention_dim), generator=g), torch.randn((2, cfg.pooled_dim), generator=g)
    kw = dict(seed=5, strength=0.5, num_inference_steps=8)

    def refiner(ranges):
        return sdxl.SDXLRefiner(eng, vae.HipVAEEncoder(sd, dev, ranges=ranges), vae.HipVAEDecoder(sd, dev, ranges=ranges))
    with pytest.raises(RuntimeError, match="non-finite latents from the VAE encoder.*vae_ranges.*calibrate_ranges"):
        refiner(None).refine(img, pe, pooled, **kw)
    for plan in (RangePlan.uniform(8), vae.calibrate_ranges(sd, dev, latents=rc.latent()[:1], images=img)):
        r = refiner(plan)
        assert r.scheduler.img2img_start(8, 0.5) == 4
        f = r.refine(img, pe, pooled, output="float", **kw)
        assert f.shape == (1, 3, 64, 64) and bool(torch.isfinite(f).all())
        u8 = r.refine(img, pe, pooled, **kw)
        assert u8.dtype == np.uint8 and u8.shape == (64, 64, 3) and 0 < u8.std()
        lat = r.refine(img, pe, pooled, output="latent", **kw)
        r.use_graphs = False
        assert torch.equal(r.refine(img, pe, pooled, output="latent", **kw), lat)        # eager = graph replays, bit for bit
        assert np.array_equal(r.refine(img, pe, pooled, **kw), u8)
