"""Nets, inputs and a functional restatement for the range-plan tests of lgd_amd/vae.py (test_vae_ranges_cpu.py,
test_vae_ranges_gpu.py).

The net is `synth_aekl_state_dict(ch=(32, 32, 64, 64), layers=1)`: the smallest with 32-channel groups, a conv_shortcut in
the encoder and in the decoder, three samplers in each half and the attention.  The HOT nets multiply weight and bias of
conv_in and of one conv1 by GAIN, so that the residual stream and one conv1 output leave the fp16 range (the
restatement's fp32 peak is beyond 4 x 65504) while the result stays of order one: every GroupNorm removes the scale again.

`forward` restates a half in torch from `RangePlan.ops` ALONE (alpha, bias factor and eps factor per op) — the plan's
semantics written out a second time — with an optional rounding of every stored tensor (`store`)."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
import lgd_amd  # noqa: E402,F401
from lgd_amd import vae  # noqa: E402
import restate_sdxl as X  # noqa: E402

CH, LAYERS = (32, 32, 64, 64), 1
GAIN = 3.0e5
HOT_DECODER = ("decoder.conv_in", "decoder.up_blocks.1.resnets.0.conv1")
HOT_ENCODER = ("encoder.conv_in", "encoder.down_blocks.1.resnets.0.conv1")
FP16_MAX = 65504.0


def heat(sd, names, gain):
    """A copy of `sd` with weight and bias of the convolutions `names` multiplied by `gain`."""
    out = dict(sd)
    for n in names:
        out[f"{n}.weight"], out[f"{n}.bias"] = sd[f"{n}.weight"] * gain, sd[f"{n}.bias"] * gain
    return out


def fp16_store(t):
    """What the engine does to every tensor it stores: one rounding to fp16 (an overflow becomes Inf)."""
    return t.half().to(t.dtype)


def forward(sd, part, x, plan=None, store=None, peaks=None, eps=1e-6):
    """The `part` ("decoder": latent -> image; "encoder": image -> moments before the clamp) under `plan`, in x's dtype.
    peaks: a dict that takes {Site: largest TRUE magnitude} (stored magnitude times the site's scale)."""
    sd = {k: v.to(x.dtype) for k, v in sd.items() if k.startswith((part, "quant_conv", "post_quant_conv"))}
    store = store or (lambda t: t)
    layout = vae.stream_layout(sd, part)
    rs = (plan or vae.RangePlan()).ops(layout)

    def see(site, t, k):
        if peaks is not None:
            peaks[site] = max(peaks.get(site, 0.0), float(t.abs().max()) * 2.0 ** k)
        return t

    def gn(t, n, factor, silu=True):
        y = F.group_norm(t, 32, sd[f"{n}.weight"], sd[f"{n}.bias"], eps * factor)
        return F.silu(y) if silu else y

    def conv(t, n, alpha=1.0, bias=1.0, **kw):
        return alpha * F.conv2d(t, sd[f"{n}.weight"], sd[f"{n}.bias"] * bias, **kw)

    h = x
    for kind, n in layout:
        r = rs[n]
        if kind == "conv_in":
            if part == "decoder":
                h = conv(h, "post_quant_conv")
            h = store(conv(h, n, r.alpha, padding=1))
        elif kind == "sampler":
            if part == "decoder":
                h = store(conv(F.interpolate(h, scale_factor=2.0, mode="nearest"), n, r.alpha, r.bias, padding=1))
            else:
                h = store(conv(F.pad(h, (0, 1, 0, 1)), n, r.alpha, r.bias, stride=2))
        elif kind == "attn":
            B, C, H, W = h.shape
            t = gn(h, f"{n}.group_norm", r.eps, silu=False).reshape(B, C, H * W).transpose(1, 2)
            lin = lambda m, v: F.linear(v, sd[f"{n}.{m}.weight"].reshape(C, C), sd[f"{n}.{m}.bias"])
            q, k, v = lin("to_q", t), lin("to_k", t), lin("to_v", t)
            a = see(r.site_a, store(torch.softmax(q @ k.transpose(1, 2) * C ** -0.5, dim=-1) @ v), 0)
            h = store(r.a_out * lin("to_out.0", a).transpose(1, 2).reshape(B, C, H, W) + h)
        else:
            t = see(r.site_inner, store(conv(gn(h, f"{n}.norm1", r.eps1), f"{n}.conv1", r.a1, padding=1)), r.j)
            sc = h if r.sc is None else store(conv(h, f"{n}.conv_shortcut", r.sc[0], r.sc[1]))
            h = store(conv(gn(t, f"{n}.norm2", r.eps2), f"{n}.conv2", r.a2, padding=1) + sc)
        see(r.site, h, r.k_out)
    h = conv(gn(h, f"{part}.conv_norm_out", rs["norm_out"].eps), f"{part}.conv_out", padding=1)
    return conv(h, "quant_conv") if part == "encoder" else h


@functools.lru_cache(maxsize=None)
def nets():
    """{"benign" | "hot_decoder" | "hot_encoder": state dict}; the hot ones are checked to be hot (fp32 restatement:
    peak beyond 4 x 65504) with a result of order one."""
    sd = vae.synth_aekl_state_dict(CH, LAYERS, seed=1)
    out = dict(benign=sd, hot_decoder=heat(sd, HOT_DECODER, GAIN), hot_encoder=heat(sd, HOT_ENCODER, GAIN))
    for name, part, x in (("hot_decoder", "decoder", latent()), ("hot_encoder", "encoder", image())):
        peaks = {}
        with torch.no_grad():
            y = forward(out[name], part, x, peaks=peaks)
        hot = [s for s, p in peaks.items() if p > 4 * FP16_MAX]
        assert {s.kind for s in hot} == {"stream", "inner"}, (name, hot)
        assert 0.1 < float(y.abs().max()) < 10.0, (name, float(y.abs().max()))
    return out


def latent():
    return torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(11))


def image():
    return torch.randn((2, 3, 64, 64), generator=torch.Generator().manual_seed(12)).clamp(-1, 1)


@functools.lru_cache(maxsize=None)
def reference(name, part):
    """The oracle's fp32 restatement (oracle/restate_sdxl.py) of net `name`: the decoded image, or the moments
    (mean, then the log-variance clamped to [-30, 20], as `encode_moments` hands them out).  Computed once; do not
    write to it."""
    with torch.no_grad():
        if part == "decoder":
            return X.vae_decode(nets()[name], latent())
        return torch.cat(X.vae_encode_moments(nets()[name], image()), dim=1)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm())
