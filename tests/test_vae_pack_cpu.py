"""What lgd_amd/vae.py packs from an AutoencoderKL state dict (no GPU): every operand of the decoder and of the encoder
against the expression written out here from the state dict alone, bit for bit; the shape read off the keys; and how
the three classes relate."""
import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import vae
from lgd_amd.weightstore import pack_conv

CH = (32, 32, 64, 64)
LEGACY = ("query", "key", "value", "proj_attn")
NEW = ("to_q", "to_k", "to_v", "to_out.0")


def h16(t):
    return t.to(torch.float16).contiguous()


def f32(t):
    return t.to(torch.float32).contiguous()


def state_dict(legacy=False, folds=True, layers=1):
    sd = vae.synth_aekl_state_dict(CH, layers, seed=1, legacy_attention_names=legacy)
    if not folds:
        sd = {k: v for k, v in sd.items() if not k.startswith(("quant_conv.", "post_quant_conv."))}
    return sd


def same(got, want, path=""):
    """Equal structure, and per tensor equal dtype, shape and bits."""
    if torch.is_tensor(want):
        assert torch.is_tensor(got) and got.dtype == want.dtype and got.shape == want.shape, path
        assert got.is_contiguous() and torch.equal(got, want), path
    elif isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), path
        for k in want:
            same(got[k], want[k], f"{path}.{k}")
    elif isinstance(want, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, f"{path}[{i}]")
    else:
        assert got == want and type(got) is type(want), path


def conv(sd, n):
    return h16(pack_conv(sd[f"{n}.weight"])), f32(sd[f"{n}.bias"])


def norm(sd, n):
    return f32(sd[f"{n}.weight"]), f32(sd[f"{n}.bias"])


def lin(sd, n):
    return h16(sd[f"{n}.weight"].reshape(sd[f"{n}.weight"].shape[0], -1)), f32(sd[f"{n}.bias"])


def res(sd, n, shortcut):
    assert (f"{n}.conv_shortcut.weight" in sd) == shortcut
    return dict(n1=norm(sd, f"{n}.norm1"), c1=conv(sd, f"{n}.conv1"), n2=norm(sd, f"{n}.norm2"), c2=conv(sd, f"{n}.conv2"),
                sc=lin(sd, f"{n}.conv_shortcut") if shortcut else None)


def attn(sd, a, names, C):
    q, k, v, o = names
    s4 = float(C) ** -0.25
    return dict(n=norm(sd, f"{a}.group_norm"),
                qk=(h16(torch.cat([sd[f"{a}.{q}.weight"].reshape(C, -1) * s4, sd[f"{a}.{k}.weight"].reshape(C, -1) * s4])),
                    f32(torch.cat([sd[f"{a}.{q}.bias"], sd[f"{a}.{k}.bias"]]) * s4)),
                v=h16(sd[f"{a}.{v}.weight"].reshape(C, -1)), vb=f32(sd[f"{a}.{v}.bias"]), o=lin(sd, f"{a}.{o}"))


def value_remainder8(w):
    """A 3x3 weight over c <= 4 channels, laid out for the operand that holds c values, their c rounding remainders and
    8 - 2c zeros."""
    return h16(pack_conv(torch.cat([w, w, torch.zeros(w.shape[0], 8 - 2 * w.shape[1], 3, 3)], dim=1)))


def blocks(sd, prefix, sampler, widths, n_res):
    out, cin = [], widths[0]
    for i, c in enumerate(widths):
        s = f"{prefix}.{i}.{sampler}.0.conv"
        out.append(([res(sd, f"{prefix}.{i}.resnets.{j}", shortcut=(j == 0 and cin != c)) for j in range(n_res)],
                    conv(sd, s) if i < len(widths) - 1 else None))
        assert (f"{s}.weight" in sd) == (i < len(widths) - 1)
        cin = c
    return out


CASES = [pytest.param(legacy, folds, id=("legacy" if legacy else "new") + ("-folds" if folds else "-plain"))
         for legacy in (False, True) for folds in (True, False)]


@pytest.mark.parametrize("legacy,folds", CASES)
def test_decoder_operands(legacy, folds):
    sd = state_dict(legacy, folds)
    d = vae.HipVAEDecoder(sd, "cpu")
    w_in = sd["decoder.conv_in.weight"]
    C = CH[-1]
    if folds:
        same(d._tap_bias, torch.einsum("ockl,c->okl", w_in, sd["post_quant_conv.bias"]), "_tap_bias")
        w_in = torch.einsum("ockl,cd->odkl", w_in, sd["post_quant_conv.weight"].reshape(4, 4))
    else:
        same(d._tap_bias, torch.zeros(C, 3, 3), "_tap_bias")
    same(d._b_in, sd["decoder.conv_in.bias"], "_b_in")
    same(d.conv_in_w8, value_remainder8(w_in), "conv_in_w8")
    assert d.conv_in_w8.shape == (C, 72) and d.c_mid == C
    same(d.attn, attn(sd, "decoder.mid_block.attentions.0", LEGACY if legacy else NEW, C), "attn")
    same(d.mid, [res(sd, f"decoder.mid_block.resnets.{j}", False) for j in range(2)], "mid")
    same(d.ups, blocks(sd, "decoder.up_blocks", "upsamplers", tuple(reversed(CH)), 2), "ups")
    same(d.norm_out, norm(sd, "decoder.conv_norm_out"), "norm_out")
    w = pack_conv(sd["decoder.conv_out.weight"])
    same(d.conv_out, (h16(torch.cat([w, torch.zeros(1, 9 * CH[0])])), f32(torch.cat([sd["decoder.conv_out.bias"], torch.zeros(1)]))),
         "conv_out")
    assert d.conv_out[0].shape == (4, 9 * CH[0]) and not d.conv_out[0][3].any() and d.conv_out[1][3] == 0


@pytest.mark.parametrize("legacy,folds", CASES)
def test_encoder_operands(legacy, folds):
    sd = state_dict(legacy, folds)
    e = vae.HipVAEEncoder(sd, "cpu")
    same(e.conv_in, (value_remainder8(sd["encoder.conv_in.weight"]), f32(sd["encoder.conv_in.bias"])), "conv_in")
    assert e.conv_in[0].shape == (CH[0], 72) and not e.conv_in[0].view(CH[0], 9, 8)[:, :, 6:].any()
    same(e.downs, blocks(sd, "encoder.down_blocks", "downsamplers", CH, 1), "downs")
    same(e.mid, [res(sd, f"encoder.mid_block.resnets.{j}", False) for j in range(2)], "mid")
    same(e.attn, attn(sd, "encoder.mid_block.attentions.0", LEGACY if legacy else NEW, CH[-1]), "attn")
    same(e.norm_out, norm(sd, "encoder.conv_norm_out"), "norm_out")
    w_o, b_o = sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"]
    if folds:
        w_o, b_o = vae.fold_pointwise_after(w_o, b_o, sd["quant_conv.weight"], sd["quant_conv.bias"])
    same(e.conv_out, (h16(pack_conv(w_o)), f32(b_o)), "conv_out")
    assert e.n_moments == 8


def test_bias_map_borders_and_its_one_entry_cache():
    """The folded post_quant_conv bias reaches a pixel only through the conv_in taps that lie inside the image."""
    sd = state_dict()
    d = vae.HipVAEDecoder(sd, "cpu")
    t = torch.einsum("ockl,c->okl", sd["decoder.conv_in.weight"], sd["post_quant_conv.bias"])
    b = sd["decoder.conv_in.bias"]
    m = d._bias_map(2, 3, 5)
    assert m.dtype == torch.float16 and m.shape == (2 * 3 * 5, CH[-1]) and torch.equal(m[:15], m[15:])
    m = m[:15].view(3, 5, -1).float()
    tol = dict(rtol=2 ** -10, atol=2 ** -12)                          # the map is stored in fp16
    torch.testing.assert_close(m[1, 2], t.sum((1, 2)) + b, **tol)                     # inside: all nine taps
    torch.testing.assert_close(m[0, 0], t[:, 1:, 1:].sum((1, 2)) + b, **tol)          # y - 1 and x - 1 are outside
    torch.testing.assert_close(m[2, 4], t[:, :2, :2].sum((1, 2)) + b, **tol)
    torch.testing.assert_close(m[1, 0], t[:, :, 1:].sum((1, 2)) + b, **tol)
    assert d._bias_map(2, 3, 5) is d._bias_map(2, 3, 5) and list(d._bias_maps) == [(2, 3, 5)]
    d._bias_map(1, 4, 4)
    assert list(d._bias_maps) == [(1, 4, 4)]


@pytest.mark.parametrize("layers", [1, 2])
def test_shape_is_read_off_the_keys(layers):
    sd = state_dict(layers=layers)
    d, e = vae.HipVAEDecoder(sd, "cpu"), vae.HipVAEEncoder(sd, "cpu")
    assert [len(r) for r, _ in d.ups] == [layers + 1] * 4 and [len(r) for r, _ in e.downs] == [layers] * 4
    assert [s is not None for _, s in d.ups] == [True, True, True, False]
    assert [s is not None for _, s in e.downs] == [True, True, True, False]
    assert [r[0]["c1"][0].shape[0] for r, _ in d.ups] == list(reversed(CH))
    assert [r[0]["c1"][0].shape[0] for r, _ in e.downs] == list(CH)


def test_the_encoder_is_no_decoder():
    e = vae.HipVAEEncoder(state_dict(), "cpu")
    assert not isinstance(e, vae.HipVAEDecoder)
    for name in ("decode", "_bias_map", "from_state_dict"):
        assert not hasattr(e, name)


def test_constructor_errors():
    sd = state_dict()
    with pytest.raises(RuntimeError, match="not an AutoencoderKL state dict: decoder.conv_in.weight"):
        vae.HipVAEDecoder({k: v for k, v in sd.items() if k.startswith("encoder.")}, "cpu")
    with pytest.raises(RuntimeError, match="not an AutoencoderKL state dict: encoder.conv_in.weight"):
        vae.HipVAEEncoder({k: v for k, v in sd.items() if k.startswith("decoder.")}, "cpu")
    wide = vae.synth_aekl_state_dict(CH, 1, latent_channels=5, seed=1)
    wide = {k: v for k, v in wide.items() if not k.startswith("post_quant_conv.")}
    with pytest.raises(RuntimeError, match="8-channel conv_in operand"):
        vae.HipVAEDecoder(wide, "cpu")
    sd["encoder.conv_in.weight"] = torch.zeros(CH[0], 5, 3, 3)
    with pytest.raises(RuntimeError, match="8-channel conv_in operand"):
        vae.HipVAEEncoder(sd, "cpu")


def test_hip_vae_is_a_decoder_with_a_lazy_encoder():
    sd = state_dict()
    v = vae.HipVAE(sd, "cpu", scaling_factor=0.5)
    assert isinstance(v, vae.HipVAEDecoder) and v._encoder is None and v.config.scaling_factor == 0.5
    same(v.conv_in_w8, vae.HipVAEDecoder(sd, "cpu").conv_in_w8, "conv_in_w8")
    e = v.encoder
    assert isinstance(e, vae.HipVAEEncoder) and v._encoder is e and v.encoder is e
    same(e.conv_out, vae.HipVAEEncoder(sd, "cpu").conv_out, "conv_out")
    half = vae.HipVAE({k: t for k, t in sd.items() if k.startswith(("decoder.", "post_quant_conv."))}, "cpu")
    with pytest.raises(RuntimeError, match="without encoder weights: it cannot encode"):
        half.encoder


def test_a_module_source_is_read_once():
    class Source:
        calls = 0

        def aekl_state_dict(self):
            self.calls += 1
            return state_dict()

    src = Source()
    v = vae.HipVAE(src, "cpu")
    assert src.calls == 1
    assert v.encoder.n_moments == 8 and src.calls == 1
    src = Source()
    vae.HipVAEDecoder(src, "cpu")
    assert src.calls == 1
