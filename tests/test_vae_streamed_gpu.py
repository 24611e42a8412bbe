"""attention = "streamed" of lgd_amd/vae.py on the GPU: the mid-block attention through lgd_attn_wide_f16 (fp32 logits, no
score matrix) against the default materialised sequence — parity on the benign nets with and without a range plan, a
rectangular latent with a ragged key tile, the SD decoder at full size, the peak memory of the mid block, a VAE whose logits
leave the fp16 range, the refiner built with the keyword, and the default's bytes."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lgd_amd  # noqa: E402,F401
from conftest import gate  # noqa: E402
from lgd_amd import vae  # noqa: E402
from lgd_amd.vae import RangePlan  # noqa: E402
import vae_range_cases as rc  # noqa: E402  (puts oracle/ on the path)

F16 = torch.float16
PARTS = ["decoder", "encoder"]
ATTN = "decoder.mid_block.attentions.0"


def _run(sd, part, dev, ranges=None, **kw):
    if part == "decoder":
        return vae.HipVAEDecoder(sd, dev, ranges=ranges, **kw).decode(rc.latent()).cpu()
    return torch.cat(vae.HipVAEEncoder(sd, dev, ranges=ranges, **kw).encode_moments(rc.image()), dim=1).cpu()


@pytest.mark.parametrize("part", PARTS)
def test_benign_net_pays_little_for_streaming(dev, part):
    """<= 1.25 x the rel-L2 of the materialised arm against the fp32 restatement, measured here, without a plan and under
    uniform(8): the project's margin for a change of arithmetic that should cost nothing."""
    sd, ref = rc.nets()["benign"], rc.reference("benign", part)
    for label, plan in (("no plan", None), ("uniform(8)", RangePlan.uniform(8))):
        mat = rc.rel_l2(_run(sd, part, dev, plan, attention="materialised"), ref)
        stm = rc.rel_l2(_run(sd, part, dev, plan, attention="streamed"), ref)
        print(f"[measured] benign {part}, {label}: rel-L2 materialised {mat:.4e}, streamed {stm:.4e}")
        gate(f"benign {part}, {label}: streamed (x materialised)", stm / mat, 1.25)


def test_leaving_the_keyword_out_is_the_materialised_arm(dev):
    sd = rc.nets()["benign"]
    for part in PARTS:
        a, b = _run(sd, part, dev), _run(sd, part, dev, attention="materialised")
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
        assert not torch.equal(a, _run(sd, part, dev, attention="streamed"))          # and the keyword does reach the launches
    z = rc.latent()
    assert torch.equal(vae.HipVAE(sd, dev).decode(z), vae.HipVAE(sd, dev, attention="materialised").decode(z))


def test_rectangular_decode_with_a_ragged_key_tile(dev):
    """Latent 6 x 10: S = 60, one full tile of 32 keys and one of 28, one query block.  The limit is
    test_rectangular_decode_vs_torch's for the materialised arm — which does not serve this latent at all: its row
    softmax takes row lengths that are multiples of 8 (lgd_softmax_rows_f16), the streamed arm any Hl x Wl."""
    from restate_vae import VAEDecoder        # oracle/restate_vae.py (test infrastructure)
    torch.manual_seed(7)
    net = VAEDecoder(ch=(128, 128, 64, 64), layers=1).float().eval()
    z = torch.randn((1, 4, 6, 10), generator=torch.Generator().manual_seed(10))
    with torch.no_grad():
        ref = net.decode(z)
    out = vae.HipVAEDecoder(net, dev, attention="streamed").decode(z)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(ref.shape) == (1, 3, 48, 80)
    gate("VAE decode rel-L2 (reduced width, latent 6 x 10, streamed)", rc.rel_l2(out, ref), 4.2e-3)
    with pytest.raises(RuntimeError, match="lgd_softmax_rows_f16"):
        vae.HipVAEDecoder(net, dev).decode(z)


def test_full_size_decode(dev):
    """The SD decoder (512 / 512 / 256 / 128 channels, 64 x 64 latent: S = 4096 at width 512) against the fp32 module, at
    test_hip_vae_decoder_full_size_from_autoencoderkl_state_dict's limit."""
    from restate_vae import VAEDecoder
    torch.manual_seed(11)
    net = VAEDecoder().float().eval()
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    z = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(3)) * 0.9
    with torch.no_grad():
        ref = net.decode(z)
    sd = net.aekl_state_dict()
    err = {}
    for mode in vae.ATTENTION_MODES:
        out = vae.HipVAEDecoder.from_state_dict(sd, dev, attention=mode).decode(z)
        torch.cuda.synchronize()
        assert out.shape == (1, 3, 512, 512) and bool(torch.isfinite(out).all())
        err[mode] = rc.rel_l2(out, ref)
    print(f"[measured] VAE decode full size: rel-L2 materialised {err['materialised']:.4e}, streamed {err['streamed']:.4e} "
          f"(x {err['streamed'] / err['materialised']:.3f})")
    gate("VAE decode full size, streamed", err["streamed"], 1.5e-2)


def test_peak_memory_of_the_mid_block(dev):
    """_attn alone on a [B * S, 64] input, S = 4096, B = 2.  Streamed: the temporaries are the GroupNorm output, the
    [B * S, 128] q | k projection, v, a and the result, six [B * S, 64] fp16 tensors = 6 MB, below ONE image's score
    matrix of S * S * 2 = 33.5 MB.  Materialised: the batch's score matrix alone is B * S * S * 2."""
    B, L = 2, 64
    S = L * L
    sd = rc.nets()["benign"]
    x = (torch.randn((B * S, 64), generator=torch.Generator().manual_seed(5)) * 0.5).to(dev, F16)
    peaks = {}
    for mode in vae.ATTENTION_MODES:
        hip = vae.HipVAEDecoder(sd, dev, attention=mode)
        y = hip._attn(hip.attn, x, B, L, L)                             # first call: workspaces, caches
        torch.cuda.synchronize()
        assert y.shape == x.shape and bool(torch.isfinite(y).all())
        del y
        torch.cuda.reset_peak_memory_stats(dev)
        start = torch.cuda.memory_allocated(dev)
        y = hip._attn(hip.attn, x, B, L, L)
        torch.cuda.synchronize()
        peaks[mode] = torch.cuda.max_memory_allocated(dev) - start
        del y
    print(f"[measured] mid-block peak above the starting level: materialised {peaks['materialised'] / 2 ** 20:.1f} MiB, "
          f"streamed {peaks['streamed'] / 2 ** 20:.1f} MiB (one score matrix: {S * S * 2 / 2 ** 20:.1f} MiB)")
    assert peaks["streamed"] < S * S * 2, peaks
    assert peaks["materialised"] >= B * S * S * 2, peaks


def _largest_logit(sd, monkeypatch):
    """The largest attention logit of the fp32 restatement of the decoder on rc.latent(), and the decoded image."""
    seen = []
    softmax = torch.softmax
    monkeypatch.setattr(torch, "softmax", lambda t, dim: (seen.append(float(t.max())), softmax(t, dim=dim))[1])
    try:
        with torch.no_grad():
            y = rc.forward(sd, "decoder", rc.latent())
    finally:
        monkeypatch.undo()
    assert len(seen) == 1
    return seen[0], y


def test_logits_beyond_fp16_are_lost_materialised_and_finite_streamed(dev, monkeypatch):
    """to_q and to_k scaled up (found here, on the CPU) until the restatement's largest logit passes 1e5.  No parity
    gate: at such logits the softmax is an arg-max and the fp16 storage of q and k decides ties, not the attention kernel
    (DESIGN.md (c)); the kernel's parity at hot logits is test_attn_wide_gpu's hot test."""
    sd = rc.nets()["benign"]
    top, _ = _largest_logit(sd, monkeypatch)
    assert top > 0
    g = (1.2e5 / top) ** 0.5                                            # the logits are bilinear in (to_q, to_k)
    hot = rc.heat(sd, [f"{ATTN}.to_q", f"{ATTN}.to_k"], g)
    top_hot, y_ref = _largest_logit(hot, monkeypatch)
    print(f"[measured] largest logit {top:.3f}; to_q, to_k x {g:.1f}: {top_hot:.4e}")
    assert top_hot > 1.0e5 and bool(torch.isfinite(y_ref).all())
    lost = vae.HipVAEDecoder(hot, dev, attention="materialised").decode(rc.latent())
    assert not bool(torch.isfinite(lost).all())                          # the precondition: the existing arm loses the image
    out = vae.HipVAEDecoder(hot, dev, attention="streamed").decode(rc.latent())
    assert out.shape == y_ref.shape and bool(torch.isfinite(out).all())
    seen = vae.probe_ranges(hot, dev, None, latents=rc.latent(), attention="streamed")     # the probes work under either setting
    assert all(bad == 0 for _, bad in seen.values())
    assert any(bad for _, bad in vae.probe_ranges(hot, dev, None, latents=rc.latent()).values())


def test_refiner_built_with_the_keyword(dev):
    """tiny_xl refiner, 64 x 64 image, both VAE halves streamed."""
    from lgd_amd import sdxl, weights
    r, _ = sdxl.build_synthetic("tiny_xl", dev, 0, vae_ch=rc.CH, vae_layers=rc.LAYERS, vae_attention="streamed")
    assert r.enc.attention == r.dec.attention == "streamed"
    r0, _ = sdxl.build_synthetic("tiny_xl", dev, 0, vae_ch=rc.CH, vae_layers=rc.LAYERS)
    assert r0.enc.attention == r0.dec.attention == "materialised"
    cfg = weights.CONFIGS["tiny_xl"]
    g = torch.Generator().manual_seed(3)
    img = torch.randn((1, 3, 64, 64), generator=g).clamp(-1, 1)
    pe, pooled = torch.randn((2, 77, cfg.cross_attention_dim), generator=g), torch.randn((2, cfg.pooled_dim), generator=g)
    f = r.refine(img, pe, pooled, output="float", seed=5, strength=0.5, num_inference_steps=8)
    assert f.shape == (1, 3, 64, 64) and bool(torch.isfinite(f).all()) and 0 < float(f.std())
