"""The VAE ([ext] diffusers AutoencoderKL, SD 1.x / 2.x / SDXL config) on the lgd_hip kernels: implicit-GEMM convolutions,
GroupNorm+SiLU, and for the single mid-block attention three batched GEMM launches + a row softmax for the whole batch
(attention="streamed": the projections + one lgd_attn_wide_f16 launch with fp32 logits and no score matrix).
HipVAEDecoder sits inside the images/s window because pipelines.decode (models/pipelines.py:117-127, 588-595) runs once
per box and once per image; HipVAEEncoder serves the refiner, the inversion and the
MultiDiffusion background passes; HipVAE is the `vae` of `model_dict`: the decoder, with its encoder built on first use.
Both halves pack their parameters through _Pack and run the blocks of _Blocks.

Parity note: AutoencoderKL itself (diffusers 0.18.0) is absent from the sandbox, so the checkers are plain PyTorch fp32
restatements from the published architecture (oracle/restate_vae.py, oracle/restate_sdxl.py: test infrastructure) —
"parity unpinned" at that boundary; what the tests pin is this module against those restatements at the
full SD size, through the AutoencoderKL key map.

Architecture (SD config: block_out_channels (128,256,512,512), layers_per_block 2, 32 groups, eps 1e-6):
post_quant_conv 4->4 (1x1), conv_in 4->512, mid (resnet, 1-head attention, resnet), 4 up blocks
(512,512,256,128) x 3 resnets with 3 nearest-2x upsamplers, GroupNorm+SiLU, conv_out 128->3.
"""
import collections
import math
import re
import types

import torch


def _state_dict(source):
    """An AutoencoderKL state dict, or a module that hands one out through `aekl_state_dict()`."""
    return source.aekl_state_dict() if hasattr(source, "aekl_state_dict") else source


# ---------------------------------------------------------------------------------------------------------------------
# Range plan: an overflow-prone VAE (SDXL: config.force_upcast) in fp16.
#
# Between its GroupNorms the network is scale-covariant: GroupNorm(x / s) with eps / s^2 equals GroupNorm(x) with eps.
# Every tensor that can grow is the residual stream or a resnet's conv1 output, and each of them is written by a GEMM
# whose epilogue computes alpha * (acc + bias) + res.  So the stream is STORED as x / 2^k and a conv1 output as h / 2^j:
# exact in real arithmetic, no launch and no pass more than without a plan, and no weight is rescaled (no fp16 weight
# turns subnormal).  Scores, q / k / v, GroupNorm outputs, conv_out and the moments sit behind a normalisation and keep
# their scale.  Results under a plan with k > 0 are NOT bit-identical to those without: small stored values enter the
# fp16 subnormals ("fp16 range of the VAE").
# ---------------------------------------------------------------------------------------------------------------------
Site = collections.namedtuple("Site", "kind key name")
Site.__doc__ = """One fp16 tensor the blocks store.  kind "stream": the residual stream behind module `name`, key = the
segment it belongs to; "inner": the conv1 output of resnet `key`; "free": the attention's `a` (behind a softmax: it carries
no scale and is probed for non-finite values only)."""


def stream_layout(keys, part):
    """The run order of the `part` ("decoder" | "encoder") of an AutoencoderKL, read off the state dict's keys:
    [(kind, name)] with kind "conv_in", "res" (identity residual), "res_sc" (conv_shortcut), "attn" or "sampler"."""
    keys = set(keys)

    def count(prefix):
        return 1 + max(int(m.group(1)) for k in keys for m in [re.match(re.escape(prefix) + r"\.(\d+)\.", k)] if m)

    def res(n):
        return ("res_sc" if f"{n}.conv_shortcut.weight" in keys else "res", n)

    mid = [res(f"{part}.mid_block.resnets.0"), ("attn", f"{part}.mid_block.attentions.0"), res(f"{part}.mid_block.resnets.1")]
    prefix, sampler = (f"{part}.up_blocks", "upsamplers") if part == "decoder" else (f"{part}.down_blocks", "downsamplers")
    blocks = []
    for i in range(count(prefix)):
        blocks += [res(f"{prefix}.{i}.resnets.{j}") for j in range(count(f"{prefix}.{i}.resnets"))]
        s = f"{prefix}.{i}.{sampler}.0.conv"
        if f"{s}.weight" in keys:
            blocks.append(("sampler", s))
    return [("conv_in", f"{part}.conv_in")] + (mid + blocks if part == "decoder" else blocks + mid)


class RangePlan:
    """Integer exponents (powers of two only) for the tensors of a VAE that can grow: one per stream SEGMENT (the stream
    is stored as x / 2^k) and one per resnet (`inner`: its conv1 output is stored as h / 2^j).  A segment starts at
    conv_in's output, at the output of every up / down-sampler convolution and at the output of every resnet with a
    conv_shortcut, and carries that module's name; resnets with an identity residual and the attention stay in their
    input's segment.  Names are AutoencoderKL's, so one plan serves the decoder and the encoder; a name the plan does
    not list gets `default`."""
    MAX_EXPONENT = 24        # eps * 2^-48 is still a normal fp32 number for every eps a VAE uses

    def __init__(self, segments=None, inner=None, default=0):
        self.segments, self.inner, self.default = dict(segments or {}), dict(inner or {}), default
        for k in [default, *self.segments.values(), *self.inner.values()]:
            if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k <= self.MAX_EXPONENT:
                raise ValueError(f"a range exponent is an integer in [0, {self.MAX_EXPONENT}], got {k!r}")

    @classmethod
    def uniform(cls, k):
        return cls(default=k)

    @staticmethod
    def exponent(peak, headroom_bits=4):
        """max(0, ceil(log2(peak / 2^(16 - headroom_bits)))): the smallest exponent that stores `peak` at or below
        2^(16 - headroom_bits).  Exact (frexp, not a rounded logarithm)."""
        peak = float(peak)
        if not 0.0 <= peak < math.inf:
            raise ValueError(f"a peak is a finite magnitude, got {peak}")
        if peak == 0.0:
            return 0
        m, e = math.frexp(peak)                      # peak = m 2^e with 0.5 <= m < 1
        return max(0, (e - 1 if m == 0.5 else e) - (16 - int(headroom_bits)))

    @classmethod
    def from_peaks(cls, peaks, headroom_bits=4):
        """peaks: {Site: largest TRUE magnitude seen there} -> the plan whose stored peaks are <= 2^(16 - headroom_bits)
        for these inputs (2^12 by default: 16x room below 65504 for hotter ones): per segment the maximum over its
        stream sites of `exponent(peak)`, the same per resnet for `inner`.  A pure host function."""
        seg, inner = {}, {}
        for site, peak in peaks.items():
            to = seg if site.kind == "stream" else inner if site.kind == "inner" else None
            if to is not None:
                to[site.key] = max(to.get(site.key, 0), cls.exponent(peak, headroom_bits))
        return cls(seg, inner)

    def segment(self, name):
        return self.segments.get(name, self.default)

    def resnet(self, name):
        return self.inner.get(name, self.default)

    def is_identity(self):
        return not (self.default or any(self.segments.values()) or any(self.inner.values()))

    # the three rules every launch under a plan follows
    @staticmethod
    def alpha_out(k_out):
        """GEMM that reads a GroupNorm output (unscaled) and writes a tensor stored at exponent k_out: alpha."""
        return 2.0 ** -k_out

    @staticmethod
    def carry(k_in, k_out):
        """GEMM that reads a tensor stored at k_in and writes one stored at k_out (shortcut, sampler):
        (alpha, factor of the fp32 bias) = (2^(k_in - k_out), 2^-k_in), since alpha * (W x / 2^k_in + b / 2^k_in)."""
        return 2.0 ** (k_in - k_out), 2.0 ** -k_in

    @staticmethod
    def eps_scale(k):
        """GroupNorm that reads a tensor stored at exponent k: the factor of its eps."""
        return 2.0 ** (-2 * k)

    def ops(self, layout):
        """The scales of every op of `layout` (stream_layout), by module name — all a forward pass needs of the plan:
          conv_in   k_out, alpha
          res(_sc)  k_in, k_out, j, eps1 (factor of norm1's eps), a1 (conv1's alpha), eps2, a2 (conv2's alpha),
                    sc = (alpha, bias factor) of the conv_shortcut | None
          attn      k, eps (factor), a_out (to_out's alpha)
          sampler   k_in, k_out, alpha, bias (factor)
        and under "norm_out" the eps factor of conv_norm_out.  Each record names its segment(s) and its Sites."""
        out, seg, k = {}, None, 0
        for kind, name in layout:
            rec = types.SimpleNamespace(kind=kind, name=name, k_in=k, seg_in=seg)
            if kind in ("conv_in", "sampler", "res_sc"):
                seg, k = name, self.segment(name)
            rec.seg_out, rec.k_out, rec.site = seg, k, Site("stream", seg, name)
            if kind == "conv_in":
                rec.alpha = self.alpha_out(k)
            elif kind == "sampler":
                rec.alpha, rec.bias = self.carry(rec.k_in, k)
            elif kind == "attn":
                rec.k, rec.eps, rec.a_out, rec.site_a = k, self.eps_scale(k), self.alpha_out(k), Site("free", name, name + ".a")
            else:
                rec.j = self.resnet(name)
                rec.eps1, rec.a1, rec.eps2, rec.a2 = self.eps_scale(rec.k_in), self.alpha_out(rec.j), self.eps_scale(rec.j), self.alpha_out(k)
                rec.sc = self.carry(rec.k_in, k) if kind == "res_sc" else None
                rec.site_inner = Site("inner", name, name + ".conv1")
            out[name] = rec
        out["norm_out"] = types.SimpleNamespace(kind="norm_out", k=k, eps=self.eps_scale(k))
        return out

    def __eq__(self, other):
        return isinstance(other, RangePlan) and (self.segments, self.inner, self.default) == (other.segments, other.inner, other.default)

    def __repr__(self):
        return f"RangePlan(segments={self.segments}, inner={self.inner}, default={self.default})"


def sites_of(layout):
    """Every Site of `layout`, in run order (what calibrate_ranges probes)."""
    out = []
    for rec in list(RangePlan().ops(layout).values())[:-1]:
        out += [s for s in (getattr(rec, "site_inner", None), getattr(rec, "site_a", None), rec.site) if s is not None]
    return out


_NO_PLAN = RangePlan()
# what _Blocks._res / _attn run under when a caller hands them no record: no scale, nothing probed
_RES_1 = types.SimpleNamespace(eps1=1.0, a1=1.0, eps2=1.0, a2=1.0, sc=None, sc_bias=None, site=None, site_inner=None)
_ATTN_1 = types.SimpleNamespace(eps=1.0, a_out=1.0, site=None, site_a=None)
# how the mid-block attention runs: over a materialised fp16 score matrix (the default), or through lgd_attn_wide_f16
ATTENTION_MODES = ("materialised", "streamed")


def attention_kw(vae_attention):
    """The keyword a builder's `vae_attention=` (None: the class default) hands to the VAE classes."""
    return {} if vae_attention is None else {"attention": vae_attention}


class _Pack:
    """The `part` half ("decoder" | "encoder") of an AutoencoderKL state dict, with the 1x1 convolution `extra` next to
    it, packed for the kernels: fp16 weights (3x3 as pack_conv lays them out, 1x1 as [Cout, Cin]), fp32 biases and norms."""

    def __init__(self, state_dict, device, part, extra):
        from .weightstore import pack_conv
        self.pack_conv = pack_conv
        self.h16 = lambda t: t.to(device, torch.float16).contiguous()
        self.f32 = lambda t: t.to(device, torch.float32).contiguous()
        self.sd = {k: v.detach().float().cpu() for k, v in dict(state_dict).items() if k.startswith((part + ".", extra + "."))}
        if f"{part}.conv_in.weight" not in self.sd:
            raise RuntimeError(f"not an AutoencoderKL state dict: {part}.conv_in.weight is missing")

    def conv(self, n):
        return self.h16(self.pack_conv(self.sd[f"{n}.weight"])), self.f32(self.sd[f"{n}.bias"])

    def lin(self, n):
        w = self.sd[f"{n}.weight"]
        return self.h16(w.reshape(w.shape[0], -1)), self.f32(self.sd[f"{n}.bias"])

    def norm(self, n):
        return self.f32(self.sd[f"{n}.weight"]), self.f32(self.sd[f"{n}.bias"])

    def res(self, n):
        return dict(n1=self.norm(f"{n}.norm1"), c1=self.conv(f"{n}.conv1"), n2=self.norm(f"{n}.norm2"), c2=self.conv(f"{n}.conv2"),
                    sc=self.lin(f"{n}.conv_shortcut") if f"{n}.conv_shortcut.weight" in self.sd else None)

    def attn(self, a):
        sd = self.sd
        legacy = f"{a}.query.weight" in sd
        nq, nk, nv, no = ("query", "key", "value", "proj_attn") if legacy else ("to_q", "to_k", "to_v", "to_out.0")
        C = sd[f"{a}.group_norm.weight"].shape[0]
        # the softmax scale C^-1/2 is split over the q and k projections, so the fp16 score matrix holds scaled logits
        # (raw 512-term dot products of a real VAE can leave the fp16 range)
        s4 = float(C) ** -0.25
        wq, wk = sd[f"{a}.{nq}.weight"].reshape(C, -1) * s4, sd[f"{a}.{nk}.weight"].reshape(C, -1) * s4
        return dict(n=self.norm(f"{a}.group_norm"),
                    qk=(self.h16(torch.cat([wq, wk])), self.f32(torch.cat([sd[f"{a}.{nq}.bias"], sd[f"{a}.{nk}.bias"]]) * s4)),
                    v=self.h16(sd[f"{a}.{nv}.weight"].reshape(C, -1)), vb=self.f32(sd[f"{a}.{nv}.bias"]), o=self.lin(f"{a}.{no}"))

    def in8(self, w, what):
        """conv_in over the 8-channel operand of lgd_nchw_to_nhwc8_f16 / lgd_image_u8_to_nhwc8_f16: channels 0..ci-1 =
        fp16 value, ci..2ci-1 = its rounding remainder, rest zero."""
        ci = w.shape[1]
        if ci > 4:
            raise RuntimeError(f"{what} = {ci}: the 8-channel conv_in operand holds value + remainder of <= 4 channels")
        return self.h16(self.pack_conv(torch.cat([w, w, w.new_zeros(w.shape[0], 8 - 2 * ci, 3, 3)], dim=1)))

    def count(self, prefix):
        """1 + the largest i among the keys `<prefix>.<i>.`: how many blocks or resnets there are."""
        return 1 + max(int(m.group(1)) for k in self.sd for m in [re.match(re.escape(prefix) + r"\.(\d+)\.", k)] if m)

    def blocks(self, prefix, sampler):
        """[(resnets, conv of `<sampler>.0.conv` | None)] of `<prefix>.<i>`: the shape is read off the keys."""
        out = []
        for i in range(self.count(prefix)):
            b, s = f"{prefix}.{i}", f"{prefix}.{i}.{sampler}.0.conv"
            out.append(([self.res(f"{b}.resnets.{j}") for j in range(self.count(f"{b}.resnets"))],
                        self.conv(s) if f"{s}.weight" in self.sd else None))
        return out


class _Blocks:
    """What the decoder and the encoder share at run time: the kernels, the device, the GroupNorm constants and the two
    blocks over a channels-last fp16 map x [B*H*W, C]."""

    def __init__(self, device, groups, eps, attention="materialised"):
        from . import ops
        if attention not in ATTENTION_MODES:
            raise ValueError(f"attention is one of {ATTENTION_MODES}, got {attention!r}")
        self.ops = ops
        self.dev = torch.device(device)
        self.groups, self.eps, self.attention = groups, eps, attention
        self._probe = None                   # calibration only (probe_ranges): called with (Site, stored tensor)

    def _plan(self, pk, part, ranges):
        """The scale records of `ranges` (None: no plan) for this half, with the fp32 biases of the GEMMs that read a
        scaled tensor (shortcuts, samplers) multiplied by their factor; a factor of one keeps the packed bias itself."""
        self.ranges = _NO_PLAN if ranges is None else ranges
        if not isinstance(self.ranges, RangePlan):
            raise TypeError(f"ranges is a vae.RangePlan or None, got {type(ranges).__name__}")
        self.layout = stream_layout(pk.sd, part)
        starts = {n for k, n in self.layout if k in ("conv_in", "sampler", "res_sc")}
        resnets = {n for k, n in self.layout if k in ("res", "res_sc")}
        for what, names, known in (("segment", self.ranges.segments, starts), ("resnet", self.ranges.inner, resnets)):
            for n in names:                  # a name of the other half is that half's business; a misspelt one of ours is not
                if n.startswith(part + ".") and n not in known:
                    raise ValueError(f"the range plan names {n}, which is no {what} of this {part}")
        self.sites = sites_of(self.layout)
        self.rs = self.ranges.ops(self.layout)
        for rec in self.rs.values():
            if rec.kind in ("res", "res_sc"):
                rec.sc_bias = None
                if rec.sc is not None and rec.sc[1] != 1.0:
                    rec.sc_bias = pk.f32(pk.sd[f"{rec.name}.conv_shortcut.bias"] * rec.sc[1])
            elif rec.kind == "sampler":
                rec.bias_t = pk.f32(pk.sd[f"{rec.name}.bias"] * rec.bias) if rec.bias != 1.0 else None

    def _see(self, site, t):
        if self._probe is not None and site is not None:
            self._probe(site, t)
        return t

    def _res(self, p, x, B, H, W, r=_RES_1):
        """r: the resnet's record of RangePlan.ops — x arrives as x / 2^k_in, conv1's output is stored as h / 2^j, the
        result leaves as (shortcut(x) + h) / 2^k_out."""
        ops = self.ops
        HW = H * W
        h = ops.groupnorm(x, B, HW, self.groups, self.eps * r.eps1, p["n1"][0], p["n1"][1], True)
        h = self._see(r.site_inner, ops.conv3x3(h, p["c1"][0], B, H, W, bias=p["c1"][1], alpha=r.a1))
        h = ops.groupnorm(h, B, HW, self.groups, self.eps * r.eps2, p["n2"][0], p["n2"][1], True)
        if p["sc"] is None:
            sc = x
        elif r.sc is None:
            sc = ops.linear(x, p["sc"][0], p["sc"][1])
        else:
            sc = ops.linear(x, p["sc"][0], p["sc"][1] if r.sc_bias is None else r.sc_bias, alpha=r.sc[0])
        return self._see(r.site, ops.conv3x3(h, p["c2"][0], B, H, W, bias=p["c2"][1], res=sc, alpha=r.a2))

    def _sampler(self, c, x, B, H, W, r, ups):
        """The 3x3 convolution of an up / down-sampler: reads the stream at k_in, starts the segment stored at k_out."""
        return self._see(r.site, self.ops.conv3x3(x, c[0], B, H, W, bias=c[1] if r.bias_t is None else r.bias_t, ups=ups,
                                                  alpha=r.alpha))

    def _attn(self, p, x, B, H, W, r=_ATTN_1):
        """Single-head attention over the H*W positions at width C (512): the head is wider than the flash kernels'
        160.  attention = "materialised": the batch runs as three BATCHED GEMM launches + one row softmax:
            scores[b] = q[b] k[b]^T      ->  P = softmax(scores)      (q, k carry C^-1/4 each)
            vt[b]     = Wv n[b]^T        (V^T directly from the projection: no transpose pass)
            out[b]    = P[b] vt[b]^T + bv   (rows of P sum to 1, so V's bias is added once, behind the product)
        attention = "streamed": v = n Wv^T + bv in row layout from the same packed weights, then ONE lgd_attn_wide_f16
        launch that reads q and k as the halves of the [B*S, 2C] projection (scale 1: the weights carry it): fp32 logits,
        no score matrix, memory linear in S."""
        ops = self.ops
        S = H * W
        C = x.shape[1]
        F16 = torch.float16
        n = ops.groupnorm(x, B, S, self.groups, self.eps * r.eps, p["n"][0], p["n"][1], False)
        qk = ops.linear(n, p["qk"][0], p["qk"][1])                                  # [B*S, 2C]
        if self.attention == "streamed":
            v = ops.linear(n, p["v"], p["vb"])                                      # [B*S, C]
            a = torch.empty((B * S, C), device=self.dev, dtype=F16)
            ops.attn_wide(qk, qk[:, C:], v, a, B, S, S, C, 1.0, q_view=(2 * C, S * 2 * C), k_view=(2 * C, S * 2 * C))
            return self._see(r.site, ops.linear(self._see(r.site_a, a), p["o"][0], p["o"][1], res=x, alpha=r.a_out))
        sc = torch.empty((B * S, S), device=self.dev, dtype=F16)
        ops.gemm_launch(ops.gemm_desc(qk, qk[:, C:], sc, S, S, C, lda0=2 * C, ldw=2 * C, ldc=S, nb_o=B,
                                      a_bs=(S * 2 * C, 0), w_bs=(S * 2 * C, 0), c_bs=(S * S, 0)))
        pr = ops.softmax_rows(sc, 1.0, out=sc)
        vt = torch.empty((B * C, S), device=self.dev, dtype=F16)
        ops.gemm_launch(ops.gemm_desc(p["v"], n, vt, C, S, C, lda0=C, ldw=C, ldc=S, nb_o=B,
                                      a_bs=(0, 0), w_bs=(S * C, 0), c_bs=(C * S, 0)))
        a = torch.empty((B * S, C), device=self.dev, dtype=F16)
        ops.gemm_launch(ops.gemm_desc(pr, vt, a, S, C, S, lda0=S, ldw=S, ldc=C, bias=p["vb"], nb_o=B,
                                      a_bs=(S * S, 0), w_bs=(C * S, 0), c_bs=(S * C, 0)))
        # q, k, v, the scores and a sit behind the GroupNorm: only to_out meets the (scaled) stream again
        return self._see(r.site, ops.linear(self._see(r.site_a, a), p["o"][0], p["o"][1], res=x, alpha=r.a_out))


class HipVAEDecoder(_Blocks):
    """AutoencoderKL.decode (the `.sample` tensor) on the lgd_hip kernels: channels-last fp16, fp32 accumulate.

    HipVAEDecoder(state_dict | module with `aekl_state_dict()`, device).  The state dict is AutoencoderKL's (encoder keys are ignored);
    the decoder's shape (channels per up block, resnets per block, which blocks upsample) is read off the keys.
    ranges: a RangePlan for a VAE whose activations leave the fp16 range (None = RangePlan.uniform(0): plain fp16).
    attention: "materialised" (default) or "streamed" — how the mid-block attention runs (_Blocks._attn)."""

    def __init__(self, source, device, groups: int = 32, eps: float = 1e-6, ranges=None, attention="materialised"):
        super().__init__(device, groups, eps, attention)
        pk = _Pack(_state_dict(source), self.dev, "decoder", "post_quant_conv")
        sd = pk.sd
        self._plan(pk, "decoder", ranges)
        # post_quant_conv (1x1, 4 -> 4) folded into conv_in: conv_in(W1 z + b1) = conv_in'(z) + border-aware bias map
        # (the zero padding of conv_in does not carry b1, so the folded bias depends on which taps lie inside the image)
        w_in, self._b_in = sd["decoder.conv_in.weight"], sd["decoder.conv_in.bias"]
        if "post_quant_conv.weight" in sd:
            w1 = sd["post_quant_conv.weight"].reshape(sd["post_quant_conv.weight"].shape[0], -1)
            b1 = sd["post_quant_conv.bias"]
            self._tap_bias = torch.einsum("ockl,c->okl", w_in, b1)                   # [Cout,3,3]
            w_in = torch.einsum("ockl,cd->odkl", w_in, w1)
        else:
            self._tap_bias = torch.zeros(w_in.shape[0], 3, 3)
        self.conv_in_w8 = pk.in8(w_in, "latent_channels")
        self.c_mid = w_in.shape[0]
        self._bias_maps = {}
        self.attn = pk.attn("decoder.mid_block.attentions.0")
        self.mid = [pk.res("decoder.mid_block.resnets.0"), pk.res("decoder.mid_block.resnets.1")]
        self.ups = pk.blocks("decoder.up_blocks", "upsamplers")
        self.norm_out = pk.norm("decoder.conv_norm_out")
        w = pk.pack_conv(sd["decoder.conv_out.weight"])                              # [3, 9*C]
        self.conv_out = (pk.h16(torch.cat([w, torch.zeros(1, w.shape[1])])),          # pad to 4 output channels
                         pk.f32(torch.cat([sd["decoder.conv_out.bias"], torch.zeros(1)])))

    @classmethod
    def from_state_dict(cls, state_dict, device, **kw):
        """`AutoencoderKL.state_dict()` (models/models.py:41) -> decoder on the HIP kernels."""
        return cls(state_dict, device, **kw)

    def _bias_map(self, B, H, W):
        """conv_in bias + what post_quant_conv's bias contributes through the taps that lie inside the image:
        fp16 [B*H*W, C] (residual operand of the conv_in GEMM); under a range plan the map of the stream's first segment,
        scaled in fp32 and rounded once."""
        key = (B, H, W)
        if key not in self._bias_maps:
            vy, vx = torch.ones(3, H), torch.ones(3, W)
            vy[0, 0] = vx[0, 0] = 0          # tap row ky = 0 reads y - 1: outside at y = 0
            vy[2, H - 1] = vx[2, W - 1] = 0
            m = torch.einsum("okl,ky,lx->yxo", self._tap_bias, vy, vx) + self._b_in          # [H, W, C]
            m = m * self.rs["decoder.conv_in"].alpha
            self._bias_maps = {key: m.reshape(1, H * W, -1).expand(B, -1, -1).reshape(B * H * W, -1)
                               .to(self.dev, torch.float16).contiguous()}
        return self._bias_maps[key]

    @torch.no_grad()
    def decode(self, z):
        """z (B, C, Hl, Wl) -> (B, 3, 8 Hl, 8 Wl); Hl and Wl need not be equal (a MultiDiffusion panorama).  The mid-block
        attention runs over all Hl*Wl positions.  Under attention = "materialised" (the default) that is a materialised
        fp16 score matrix of (Hl*Wl)^2 elements per image — 32 MB at 64 x 64, 512 MB at the 64 x 256 latent of a
        512 x 2048 panorama — whose logits are STORED in fp16: a logit above 65504 turns its row, and the image, into NaN.
        Under attention = "streamed" one lgd_attn_wide_f16 launch keeps the logits in fp32 and stores no scores at all:
        the temporaries of the attention are six [B*Hl*Wl, C] fp16 tensors."""
        ops, rs = self.ops, self.rs
        z = z.to(self.dev, torch.float32).contiguous()
        B, _, H, W = z.shape
        lat8 = ops.nchw_to_nhwc8(z)
        h = torch.empty((B * H * W, self.c_mid), device=self.dev, dtype=torch.float16)
        ops.gemm_launch(ops.gemm_desc(lat8, self.conv_in_w8, h, B * H * W, self.c_mid, 72, c0=8, lda0=8, taps=9, hin=H,
                                      win=W, hout=H, wout=W, res=self._bias_map(B, H, W), ldr=self.c_mid,
                                      ldc=self.c_mid, splits=1, alpha=rs["decoder.conv_in"].alpha))
        self._see(rs["decoder.conv_in"].site, h)
        h = self._res(self.mid[0], h, B, H, W, rs["decoder.mid_block.resnets.0"])
        h = self._attn(self.attn, h, B, H, W, rs["decoder.mid_block.attentions.0"])
        h = self._res(self.mid[1], h, B, H, W, rs["decoder.mid_block.resnets.1"])
        for i, (blk, up) in enumerate(self.ups):
            for j, r in enumerate(blk):
                h = self._res(r, h, B, H, W, rs[f"decoder.up_blocks.{i}.resnets.{j}"])
            if up is not None:
                h = self._sampler(up, h, B, H, W, rs[f"decoder.up_blocks.{i}.upsamplers.0.conv"], 1)
                H, W = 2 * H, 2 * W
        h = ops.groupnorm(h, B, H * W, self.groups, self.eps * rs["norm_out"].eps, self.norm_out[0], self.norm_out[1], True)
        # conv_out (128 -> 3, padded to 4 channels) on the matrix cores as well: at 512 x 512 the one-wave-per-pixel
        # kernel took 1.7 ms per image, the implicit GEMM (N = 4 inside a 64-wide tile) a few tens of microseconds
        y = ops.conv3x3(h, self.conv_out[0], B, H, W, bias=self.conv_out[1])            # [B*H*W, 4] fp16
        return y.view(B, H, W, 4)[..., :3].permute(0, 3, 1, 2).float()


def make_hip_vae(device, seed=0):
    """Random-init SD VAE decoder (seeded AutoencoderKL state dict of the SD architecture) running on the HIP kernels."""
    return HipVAEDecoder(synth_aekl_state_dict(seed=seed), device)


def make_hip_vae_pair(device, seed=0):
    """make_hip_vae's decoder with the encoder of the same seeded state dict behind it (HipVAE: built on first use)."""
    return HipVAE(synth_aekl_state_dict(seed=seed), device)


def synth_aekl_state_dict(ch=(128, 256, 512, 512), layers=2, latent_channels=4, seed=0, legacy_attention_names=False):
    """A full AutoencoderKL state dict (encoder + quant_conv + post_quant_conv + decoder, diffusers key names) with
    seeded random parameters of the SD / SDXL VAE architecture: there are no checkpoints in the sandbox."""
    g = torch.Generator().manual_seed(4321 + seed)
    out = {}

    def conv(name, cout, cin, k):
        out[f"{name}.weight"] = (torch.rand((cout, cin, k, k), generator=g) * 2 - 1) * (cin * k * k) ** -0.5
        out[f"{name}.bias"] = 0.05 * torch.randn((cout,), generator=g)

    def norm(name, c):
        out[f"{name}.weight"] = 1.0 + 0.1 * torch.randn((c,), generator=g)
        out[f"{name}.bias"] = 0.05 * torch.randn((c,), generator=g)

    def res(name, cin, cout):
        norm(f"{name}.norm1", cin); conv(f"{name}.conv1", cout, cin, 3)
        norm(f"{name}.norm2", cout); conv(f"{name}.conv2", cout, cout, 3)
        if cin != cout:
            conv(f"{name}.conv_shortcut", cout, cin, 1)

    def attn(name, c):
        norm(f"{name}.group_norm", c)
        for n in (("query", "key", "value", "proj_attn") if legacy_attention_names else ("to_q", "to_k", "to_v", "to_out.0")):
            out[f"{name}.{n}.weight"] = (torch.rand((c, c), generator=g) * 2 - 1) * c ** -0.5
            out[f"{name}.{n}.bias"] = 0.05 * torch.randn((c,), generator=g)

    conv("encoder.conv_in", ch[0], 3, 3)
    cin = ch[0]
    for i, c in enumerate(ch):
        for j in range(layers):
            res(f"encoder.down_blocks.{i}.resnets.{j}", cin if j == 0 else c, c)
        cin = c
        if i < len(ch) - 1:
            conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", c, c, 3)
    res("encoder.mid_block.resnets.0", cin, cin); attn("encoder.mid_block.attentions.0", cin); res("encoder.mid_block.resnets.1", cin, cin)
    norm("encoder.conv_norm_out", cin); conv("encoder.conv_out", 2 * latent_channels, cin, 3)
    conv("quant_conv", 2 * latent_channels, 2 * latent_channels, 1)
    conv("post_quant_conv", latent_channels, latent_channels, 1)
    rev = tuple(reversed(ch))
    conv("decoder.conv_in", rev[0], latent_channels, 3)
    res("decoder.mid_block.resnets.0", rev[0], rev[0]); attn("decoder.mid_block.attentions.0", rev[0]); res("decoder.mid_block.resnets.1", rev[0], rev[0])
    cin = rev[0]
    for i, c in enumerate(rev):
        for j in range(layers + 1):
            res(f"decoder.up_blocks.{i}.resnets.{j}", cin if j == 0 else c, c)
        cin = c
        if i < len(rev) - 1:
            conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", c, c, 3)
    norm("decoder.conv_norm_out", cin); conv("decoder.conv_out", 3, cin, 3)
    return out


def fold_pointwise_after(w, b, w1, b1):
    """A 1x1 convolution (w1 [P, C, 1, 1], b1) applied AFTER a k x k convolution (w [C, D, k, k], b) is one k x k
    convolution: weights sum_c w1[p, c] w[c, d, ky, kx], bias w1 b + b1 (exact: no padding interaction on this side)."""
    m = w1.reshape(w1.shape[0], -1)
    return torch.einsum("pc,cdkl->pdkl", m, w), m @ b + b1


class HipVAEEncoder(_Blocks):
    """AutoencoderKL.encode(image).latent_dist on the lgd_hip kernels — the first half of the SDXL-refiner img2img
    pass (generation/sdxl_refinement.py:29 -> [ext] StableDiffusionXLImg2ImgPipeline.prepare_latents): conv_in 3 -> C0,
    down blocks (resnets without time embedding, Downsample2D = pad right/bottom by one + 3x3 stride 2), mid block
    (resnet, one-head attention, resnet), GroupNorm + SiLU, conv_out -> 2 x latent channels, quant_conv (1x1).

    Downsample2D's asymmetric padding: the implicit-GEMM gather pads symmetrically, so the stride-2 output is taken
    from the ODD positions of the stride-1 'same' convolution (out[o] = sum_k x[2o + k] w[k] = same[2o + 1]; the
    position past the border reads the zero the asymmetric pad adds) — 4x the flops of three small convolutions,
    once per image."""

    def __init__(self, state_dict, device, groups: int = 32, eps: float = 1e-6, ranges=None, attention="materialised"):
        super().__init__(device, groups, eps, attention)
        pk = _Pack(state_dict, self.dev, "encoder", "quant_conv")
        sd = pk.sd
        self._plan(pk, "encoder", ranges)
        self.conv_in = (pk.in8(sd["encoder.conv_in.weight"], "image channels"), pk.f32(sd["encoder.conv_in.bias"]))
        self.downs = pk.blocks("encoder.down_blocks", "downsamplers")
        self.mid = [pk.res("encoder.mid_block.resnets.0"), pk.res("encoder.mid_block.resnets.1")]
        self.attn = pk.attn("encoder.mid_block.attentions.0")
        self.norm_out = pk.norm("encoder.conv_norm_out")
        # conv_out (C -> 2z) followed by quant_conv (1x1, 2z -> 2z): composed exactly into one 3x3 convolution
        w_o, b_o = sd["encoder.conv_out.weight"], sd["encoder.conv_out.bias"]
        if "quant_conv.weight" in sd:
            w_o, b_o = fold_pointwise_after(w_o, b_o, sd["quant_conv.weight"], sd["quant_conv.bias"])
        self.n_moments = w_o.shape[0]
        self.conv_out = (pk.h16(pk.pack_conv(w_o)), pk.f32(b_o))

    @torch.no_grad()
    def moments_nhwc(self, x8, B, H):
        """The encoder from its conv_in operand x8 (fp16 [B*H*H, 8]: value, rounding remainder, zeros; what
        lgd_nchw_to_nhwc8_f16 / lgd_image_u8_to_nhwc8_f16 write) -> fp16 moments [B*(H/8)^2, 2z], channels-last: z means,
        then z log-variances (unclamped) per latent pixel."""
        ops, rs = self.ops, self.rs
        c0 = self.conv_in[0].shape[0]
        h = torch.empty((B * H * H, c0), device=self.dev, dtype=torch.float16)
        ops.gemm_launch(ops.gemm_desc(x8, self.conv_in[0], h, B * H * H, c0, 72, c0=8, lda0=8, taps=9,
                                      hin=H, win=H, hout=H, wout=H, bias=self.conv_in[1], ldc=c0, splits=1,
                                      alpha=rs["encoder.conv_in"].alpha))
        self._see(rs["encoder.conv_in"].site, h)
        for i, (blk, down) in enumerate(self.downs):
            for j, r in enumerate(blk):
                h = self._res(r, h, B, H, H, rs[f"encoder.down_blocks.{i}.resnets.{j}"])
            if down is not None:
                full = self._sampler(down, h, B, H, H, rs[f"encoder.down_blocks.{i}.downsamplers.0.conv"], False)
                C = full.shape[1]
                h = full.view(B, H, H, C)[:, 1::2, 1::2].reshape(B * (H // 2) * (H // 2), C).contiguous()
                H //= 2
        h = self._res(self.mid[0], h, B, H, H, rs["encoder.mid_block.resnets.0"])
        h = self._attn(self.attn, h, B, H, H, rs["encoder.mid_block.attentions.0"])
        h = self._res(self.mid[1], h, B, H, H, rs["encoder.mid_block.resnets.1"])
        h = ops.groupnorm(h, B, H * H, self.groups, self.eps * rs["norm_out"].eps, self.norm_out[0], self.norm_out[1], True)
        return ops.conv3x3(h, self.conv_out[0], B, H, H, bias=self.conv_out[1])       # [B*H*H, 2z] fp16

    @torch.no_grad()
    def encode_moments(self, image):
        """image [B, 3, H, W] fp32 in [-1, 1] -> (mean, logvar) fp32 [B, z, H/8, W/8]; logvar clamped to [-30, 20]
        (DiagonalGaussianDistribution)."""
        x = image.to(self.dev, torch.float32).contiguous()
        B, _, H, W = x.shape
        if H != W:
            raise RuntimeError("square images only (the refiner pass resizes to 1024 x 1024, sdxl_refinement.py:26)")
        m = self.moments_nhwc(self.ops.nchw_to_nhwc8(x), B, H)
        H = int(round((m.shape[0] // B) ** 0.5))
        m = m.view(B, H, H, self.n_moments).permute(0, 3, 1, 2).float()
        mean, logvar = m.chunk(2, dim=1)
        return mean.contiguous(), logvar.clamp(-30.0, 20.0).contiguous()


class _Config(dict):
    __getattr__ = dict.__getitem__


class HipLatentDist:
    """`vae.encode(image).latent_dist` as far as models/pipelines.py:110 reads it ([ext] diffusers
    DiagonalGaussianDistribution): the encoder's fp16 moments, still on the device and channels-last; `sample` draws the
    noise as [ext] randn_tensor does — by torch, from the caller's generator on the generator's own device, shaped like
    the mean — and one lgd_vae_sample_f32 launch does the rest."""

    def __init__(self, ops, moments, shape):
        self.ops, self.moments, self.shape = ops, moments, tuple(shape)        # shape: (B, z, H, W) of the mean

    def _nchw(self):
        B, z, H, W = self.shape
        return self.moments.view(B, H, W, 2 * z).permute(0, 3, 1, 2).float()

    @property
    def mean(self):
        return self._nchw()[:, :self.shape[1]].contiguous()

    @property
    def logvar(self):
        return self._nchw()[:, self.shape[1]:].clamp(-30.0, 20.0).contiguous()

    def mode(self):
        return self.mean

    def sample(self, generator=None, scale=1.0):
        """mean + std * noise; `scale` (not in diffusers' signature) folds vae.config.scaling_factor into the launch."""
        dev = self.moments.device
        rand_dev = generator.device if generator is not None else dev
        noise = torch.randn(self.shape, generator=generator, device=rand_dev, dtype=torch.float32)
        return self.ops.vae_sample(self.moments, noise.to(dev).contiguous(), scale)


class HipEncoderOutput:
    def __init__(self, latent_dist):
        self.latent_dist = latent_dist


class HipVAE(HipVAEDecoder):
    """The VAE object of `model_dict` (models/models.py:41): HipVAEDecoder's `decode`, unchanged, plus `encode(image)
    .latent_dist.sample(generator)` and `config.scaling_factor` as models/pipelines.py:84-114 (`encode`) reads them.  The
    encoder is a HipVAEEncoder over the same AutoencoderKL state dict, built on first use (a generation-only run never
    packs it)."""

    def __init__(self, source, device, groups: int = 32, eps: float = 1e-6, scaling_factor: float = 0.18215, ranges=None,
                 attention="materialised"):
        sd = _state_dict(source)
        super().__init__(sd, device, groups, eps, ranges=ranges, attention=attention)
        self._encoder_sd = {k: v for k, v in sd.items() if k.startswith(("encoder.", "quant_conv."))}
        self._encoder = None
        self.config = _Config(scaling_factor=scaling_factor)

    @property
    def encoder(self) -> "HipVAEEncoder":
        if self._encoder is None:
            if "encoder.conv_in.weight" not in self._encoder_sd:
                raise RuntimeError("this VAE was built from a state dict without encoder weights: it cannot encode")
            # (a plan names AutoencoderKL's modules: the encoder takes its half by name)
            self._encoder = HipVAEEncoder(self._encoder_sd, self.dev, self.groups, self.eps, ranges=self.ranges,
                                          attention=self.attention)
            self._encoder_sd = None
        return self._encoder

    @torch.no_grad()
    def encode(self, image):
        """image: uint8 (B, H, W, 3) — the bytes go to the device as they are and lgd_image_u8_to_nhwc8_f16 writes the
        conv_in operand — or float (B, 3, H, W) in [-1, 1] (lgd_nchw_to_nhwc8_f16, as the refiner pass does).  Square
        images with a side that is a multiple of 8."""
        ops, enc = self.ops, self.encoder
        image = torch.as_tensor(image)
        if image.dim() != 4:
            raise RuntimeError(f"encode takes a batch of images, got shape {tuple(image.shape)}")
        if image.dtype == torch.uint8:
            B, H, W, _ = image.shape
            x8 = ops.image_u8_to_nhwc8(image.to(self.dev).contiguous()) if H == W and H % 8 == 0 else None
        else:
            B, _, H, W = image.shape
            x8 = ops.nchw_to_nhwc8(image.to(self.dev, torch.float32).contiguous()) if H == W and H % 8 == 0 else None
        if x8 is None:
            raise RuntimeError(f"square images with a side that is a multiple of 8 only (got {H} x {W})")
        m = enc.moments_nhwc(x8, B, H)
        return HipEncoderOutput(HipLatentDist(ops, m, (B, enc.n_moments // 2, H // 8, W // 8)))


# The plan a VAE with config.force_upcast gets when its caller brings none: RangePlan.uniform(8).  True magnitudes up to
# 65504 * 2^8 = 1.6e7 stay finite, and on the synthetic nets the scaling costs a few per cent of the fp16 rounding error
# that is there anyway ("fp16 range of the VAE").  Whether 8 suffices for the real SDXL checkpoint is
# UNMEASURED: no real checkpoint has been loaded.  calibrate_ranges is the answer for a user who has it.
FORCE_UPCAST_EXPONENT = 8
CALIBRATION_EXPONENT = 12        # true magnitudes up to 65504 * 2^12 = 2.7e8 stay finite while they are measured


@torch.no_grad()
def probe_ranges(source, device, ranges, latents=None, images=None, attention="materialised"):
    """Runs the decoder on `latents` (B, z, H, W) and / or the encoder on `images` (B, 3, S, S in [-1, 1]) eagerly under
    `ranges` and measures every fp16 tensor the blocks store — the stream behind each block, each conv1 output, the
    attention's `a` — with lgd_range_f16: {Site: (largest finite STORED magnitude, number of non-finite elements)}.
    The probes write into one device table; there is one download, at the end.  attention: as the VAE classes take it
    (the sites are the same under either setting)."""
    from . import ops
    sd, dev = _state_dict(source), torch.device(device)
    halves = []
    if latents is not None:
        halves.append((HipVAEDecoder(sd, dev, ranges=ranges, attention=attention), "decode", latents))
    if images is not None:
        halves.append((HipVAEEncoder(sd, dev, ranges=ranges, attention=attention), "encode_moments", images))
    if not halves:
        raise ValueError("nothing to measure: pass latents for the decoder, images for the encoder, or both")
    sites = [s for half, _, _ in halves for s in half.sites]
    row = {s: i for i, s in enumerate(sites)}
    table = torch.zeros((len(sites), 2), device=dev, dtype=torch.int32)
    for half, run, x in halves:
        half._probe = lambda site, t: ops.range_f16(t, table, row[site])
        getattr(half, run)(x)
    host = table.cpu()
    peaks, bad = host.view(torch.float32)[:, 0].tolist(), (host[:, 1].to(torch.int64) & 0xffffffff).tolist()
    return {s: (peaks[i], bad[i]) for s, i in row.items()}


def calibrate_ranges(source, device, latents=None, images=None, headroom_bits=4, attention="materialised") -> RangePlan:
    """The plan for a VAE whose checkpoint is at hand: runs the given inputs once at RangePlan.uniform(12), takes the
    peak of every stored tensor (probe_ranges) and returns RangePlan.from_peaks of the true magnitudes, peak * 2^12 —
    stored peaks of these inputs then are <= 2^(16 - headroom_bits).  An eager, offline call: nothing of it runs inside
    a product path.  Raises if a tensor is non-finite even at that exponent."""
    k = CALIBRATION_EXPONENT
    seen = probe_ranges(source, device, RangePlan.uniform(k), latents, images, attention=attention)
    bad = [f"{s.name} ({n})" for s, (_, n) in seen.items() if n]
    if bad:
        raise RuntimeError(f"non-finite values at exponent {k}, no power-of-two range plan holds this VAE on these inputs: "
                           + ", ".join(bad))
    return RangePlan.from_peaks({s: p * 2.0 ** k for s, (p, _) in seen.items() if s.kind != "free"}, headroom_bits)
