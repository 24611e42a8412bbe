"""OWL-ViT open-vocabulary detector on the HIP kernels: the stage-2 EVALUATOR.

The reference scores its generated images with scripts/owl_vit_eval.py -> utils/eval/eval.py:120-174 (`eval_prompt`):
the Hugging Face `OwlViTForObjectDetection` ([ext] transformers, google/owlvit-base-patch32 and relatives),
`processor.post_process`, a score threshold, `nms` / `class_aware_nms` (eval.py:11-105), then the prompt's predicate.
This module runs the network and the detection tail on the C-ABI kernels, fp16 with fp32 accumulation:

  text tower     `clip.HipCLIPTextEncoder` with OWL-ViT's `text_model.*` weights and `text_projection` (causal CLIP
                 tower; pooled state at argmax(input_ids)).  The padding mask is NOT forwarded: the tower is causal, so
                 the pooled state never sees the padding behind it.  query_embeds = the projected pooled state
                 normalised once (OwlViTModel.forward); the class head normalises again with its +1e-6.
  vision tower   patch embedding as one GEMM over unfolded patches (no bias), class token, position table,
                 pre_layernorm, N pre-LN layers (fused QKV GEMM, non-causal flash attention over P + 1 tokens,
                 quick-GELU MLP), post_layernorm on every token, the merge `tokens[1:] * tokens[:1]`, layer_norm.
  heads          class head: `dense0` (fp16 GEMM) and the two 1-wide linears (one fp32-output GEMM) feed
                 `lgd_owl_heads_f32` (csrc/detect.hip); box head: three linears with exact GELU, the last one in fp32,
                 into the same kernel with the host-computed box-bias table.
  detect()       the forward, then `lgd_detect_nms_f32` in mode 0: post_process + score filter + greedy NMS per image
                 in one launch; one host read (the counts) at the end.

`HipOwlViTDetector(config, state_dict)` takes the parameter names of `OwlViTForObjectDetection.state_dict()` and is
callable like the Hugging Face module as far as eval_prompt uses it: `model(**processor_output)` -> object with
`.logits`, `.pred_boxes`, `.image_embeds`, `.text_embeds`, `.class_embeds`.  Image resizing / normalisation and
tokenisation stay with the processor object.  No real OWL-ViT checkpoint has been loaded by this project's tests: they
run seeded synthetic weights against transformers' own module.
"""
from dataclasses import dataclass

import torch

from . import ops, vit
from .clip import CLIPTextConfig, HipCLIPTextEncoder

F16, F32 = torch.float16, torch.float32

# state-dict entries the detector does not read: OwlViTModel's image-level CLIP projection and temperature (contrastive
# image-text logits, not part of detection) and the position-index buffers of older transformers versions
UNUSED_KEYS = ("owlvit.visual_projection.weight", "owlvit.logit_scale", "owlvit.text_model.embeddings.position_ids",
               "owlvit.vision_model.embeddings.position_ids")


@dataclass(frozen=True)
class OwlViTConfig:
    """The fields of transformers' OwlViTConfig that shape the computation (defaults: google/owlvit-base-patch32)."""
    image_size: int = 768
    patch_size: int = 32
    num_channels: int = 3
    hidden_size: int = 768
    intermediate_size: int = 3072
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    layer_norm_eps: float = 1e-5
    projection_dim: int = 512
    text_vocab_size: int = 49408
    text_hidden_size: int = 512
    text_intermediate_size: int = 2048
    text_num_hidden_layers: int = 12
    text_num_attention_heads: int = 8
    text_max_position_embeddings: int = 16
    text_layer_norm_eps: float = 1e-5

    @classmethod
    def from_hf(cls, c):
        v, t = c.vision_config, c.text_config
        if v.hidden_act != "quick_gelu" or t.hidden_act != "quick_gelu":
            raise RuntimeError("only the quick_gelu towers of google/owlvit-* are implemented")
        return cls(image_size=v.image_size, patch_size=v.patch_size, num_channels=v.num_channels,
                   hidden_size=v.hidden_size, intermediate_size=v.intermediate_size,
                   num_hidden_layers=v.num_hidden_layers, num_attention_heads=v.num_attention_heads,
                   layer_norm_eps=v.layer_norm_eps, projection_dim=c.projection_dim, text_vocab_size=t.vocab_size,
                   text_hidden_size=t.hidden_size, text_intermediate_size=t.intermediate_size,
                   text_num_hidden_layers=t.num_hidden_layers, text_num_attention_heads=t.num_attention_heads,
                   text_max_position_embeddings=t.max_position_embeddings, text_layer_norm_eps=t.layer_norm_eps)


def compute_box_bias(num_patches_height, num_patches_width):
    """[ext] OwlViTForObjectDetection.compute_box_bias: fp32 [h*w, 4] — the box centre is biased to the token's position
    on the grid and the box size to the patch size (logit of both).  Host table, computed once at load."""
    x = torch.arange(1, num_patches_width + 1, dtype=F32) / num_patches_width
    y = torch.arange(1, num_patches_height + 1, dtype=F32) / num_patches_height
    xx, yy = torch.meshgrid(x, y, indexing="xy")
    coords = torch.stack((xx, yy), dim=-1).reshape(-1, 2).clip(0.0, 1.0)
    coord_bias = torch.log(coords + 1e-4) - torch.log1p(-coords + 1e-4)
    size = torch.ones_like(coord_bias)
    size[..., 0] /= num_patches_width
    size[..., 1] /= num_patches_height
    size_bias = torch.log(size + 1e-4) - torch.log1p(-size + 1e-4)
    return torch.cat([coord_bias, size_bias], dim=-1)


class OwlViTDetectionOutput:
    """`.class_embeds` is what transformers returns under that name: the NORMALISED `dense0` output."""

    def __init__(self, logits, pred_boxes, image_embeds, text_embeds, class_embeds):
        self.logits, self.pred_boxes, self.image_embeds = logits, pred_boxes, image_embeds
        self.text_embeds, self.class_embeds = text_embeds, class_embeds


class Detections:
    """Result of `detect()`: device tensors in picking order, rows < counts[b] of image b valid.  boxes fp32 [B, P, 4]
    xyxy normalised to [0, 1]; scores fp32 [B, P]; labels (query index) and index (image token) int32 [B, P]; counts a
    host list of B ints."""

    def __init__(self, boxes, scores, labels, index, counts):
        self.boxes, self.scores, self.labels, self.index, self.counts = boxes, scores, labels, index, counts

    def image(self, b):
        n = self.counts[b]
        return self.boxes[b, :n], self.scores[b, :n], self.labels[b, :n]


class HipOwlViTDetector(vit.Tower):
    def __init__(self, config: OwlViTConfig, state_dict, device="cuda"):
        cfg = self.cfg = config
        self.dev = dev = torch.device(device)
        sd = state_dict
        w = vit.Weights(sd, dev)
        self.consumed = w.consumed
        h16, f32, lin, ln = w.h16, w.f32, w.lin, w.ln
        C, NH = cfg.hidden_size, cfg.num_attention_heads
        if C % NH or (C // NH) % 8:
            raise RuntimeError("head width must be a multiple of 8")
        if cfg.image_size % cfg.patch_size or (cfg.num_channels * cfg.patch_size ** 2) % 8:
            raise RuntimeError("the image must be whole patches and the patch vector a multiple of 8 long")
        if cfg.projection_dim % 8 or cfg.text_hidden_size % 8:
            raise RuntimeError("text width and projection width must be multiples of 8")
        self.grid = g = cfg.image_size // cfg.patch_size
        self.P = g * g
        self.d = C // NH

        # ---- text tower (CLIP, causal) + projection
        tp = "owlvit.text_model."
        text_sd = {k[len("owlvit."):]: w[k] for k in list(sd) if k.startswith(tp) and not k.endswith("position_ids")}
        text_sd["text_projection.weight"] = w["owlvit.text_projection.weight"]
        self.text = HipCLIPTextEncoder(CLIPTextConfig(
            vocab_size=cfg.text_vocab_size, hidden_size=cfg.text_hidden_size,
            intermediate_size=cfg.text_intermediate_size, num_hidden_layers=cfg.text_num_hidden_layers,
            num_attention_heads=cfg.text_num_attention_heads,
            max_position_embeddings=cfg.text_max_position_embeddings, layer_norm_eps=cfg.text_layer_norm_eps,
            hidden_act="quick_gelu", eos_token_id=2), text_sd, dev)     # 2: pooled at argmax(input_ids), as OwlViTTextTransformer

        # ---- vision tower
        v = "owlvit.vision_model."
        self.patch = h16(w[v + "embeddings.patch_embedding.weight"].reshape(C, -1))
        pos = f32(w[v + "embeddings.position_embedding.weight"])                      # [P + 1, C]
        if pos.shape[0] != self.P + 1:
            raise RuntimeError("position table does not match the image grid (interpolate_pos_encoding is not implemented)")
        self.cls_pos = f32(w[v + "embeddings.class_embedding"]) + pos[0]              # row 0 of every image
        self.pos = h16(pos[1:])
        self.pre_ln, self.post_ln = ln(v + "pre_layernorm"), ln(v + "post_layernorm")
        self.layers = []
        for i in range(cfg.num_hidden_layers):
            p = f"{v}encoder.layers.{i}."
            self.layers.append(vit.Layer(ln1=ln(p + "layer_norm1"), qkv=w.qkv(p + "self_attn"),
                                         out=lin(p + "self_attn.out_proj"), ln2=ln(p + "layer_norm2"),
                                         fc1=lin(p + "mlp.fc1"), fc2=lin(p + "mlp.fc2")))
        self.merge_ln = ln("layer_norm")

        # ---- heads
        self.dense0 = lin("class_head.dense0")
        ss_w = torch.cat([w["class_head.logit_shift.weight"], w["class_head.logit_scale.weight"]])
        ss_b = torch.cat([w["class_head.logit_shift.bias"], w["class_head.logit_scale.bias"]])
        pad = lambda t: torch.cat([t, t.new_zeros((8 - t.shape[0],) + tuple(t.shape[1:]))])   # GEMM columns: 2 -> 8
        self.shift_scale = (h16(pad(ss_w)), f32(pad(ss_b)))
        self.box = [lin(f"box_head.dense{i}") for i in range(3)]
        self.box_bias = compute_box_bias(g, g).to(dev).contiguous()
        self.unused = sorted(k for k in sd if k not in self.consumed)
        extra = [k for k in self.unused if k not in UNUSED_KEYS]
        if extra:
            raise RuntimeError(f"state-dict entries the detector does not know: {extra}")

    # ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_image(self, pixel_values):
        """pixel_values (B, 3, S, S) -> image_embeds fp16 [B*P, C]: [ext] OwlViTVisionTransformer.forward followed by
        OwlViTForObjectDetection.image_text_embedder's post_layernorm, class-token merge and layer_norm."""
        cfg, P = self.cfg, self.P
        B, Cin, Hh, Ww = pixel_values.shape
        if (Cin, Hh, Ww) != (cfg.num_channels, cfg.image_size, cfg.image_size):
            raise ValueError(f"Input image size ({Hh}*{Ww}) doesn't match model ({cfg.image_size}*{cfg.image_size}).")
        C, S = cfg.hidden_size, P + 1
        eps = cfg.layer_norm_eps
        y = vit.clip_vision_trunk(self, pixel_values, patch_size=cfg.patch_size, heads=cfg.num_attention_heads,
                                  eps=eps).reshape(B, S, C)
        merged = (y[:, 1:].float() * y[:, :1].float()).to(F16).reshape(B * P, C).contiguous()
        return ops.layernorm(merged, self.merge_ln[0], self.merge_ln[1], eps)

    @torch.no_grad()
    def encode_queries(self, input_ids, B):
        """input_ids (B*Q, S) -> (query_embeds fp32 [B, Q, D] normalised once, query_mask int32 [B, Q])."""
        ids = input_ids.to(self.dev)
        if ids.shape[0] % B:
            raise ValueError("input_ids must hold the same number of queries for every image")
        Q = ids.shape[0] // B
        te = self.text(ids).text_embeds.float()
        te = te / torch.linalg.norm(te, ord=2, dim=-1, keepdim=True)
        mask = (ids.reshape(B, Q, -1)[..., 0] > 0).to(torch.int32).contiguous()
        return te.reshape(B, Q, -1).contiguous(), mask

    def _heads(self, feats, query_embeds, query_mask, B):
        e = ops.linear(feats, self.dense0[0], self.dense0[1])                           # [B*P, D] fp16
        ss = ops.linear(feats, self.shift_scale[0], self.shift_scale[1], out_f32=True)  # [B*P, 8] fp32: shift, scale, 0..
        h = ops.act(ops.linear(feats, self.box[0][0], self.box[0][1]), ops.ACT_GELU)
        h = ops.act(ops.linear(h, self.box[1][0], self.box[1][1]), ops.ACT_GELU)
        raw = ops.linear(h, self.box[2][0], self.box[2][1], out_f32=True)               # [B*P, 4] fp32
        logits, boxes = ops.owl_heads(e, query_embeds, query_mask, ss[:, 0], ss[:, 1], raw, self.box_bias, B, self.P)
        return logits, boxes, e

    def _forward(self, pixel_values, input_ids, attention_mask, kw):
        if kw.get("interpolate_pos_encoding"):
            raise NotImplementedError("interpolate_pos_encoding is not implemented (eval_prompt does not use it)")
        for k in ("query_pixel_values", "output_attentions", "output_hidden_states"):
            if kw.get(k) is not None and kw.get(k) is not False:
                raise NotImplementedError(f"{k} is not implemented (image-guided detection and intermediate outputs are "
                                          "not used by eval_prompt)")
        if pixel_values is None or input_ids is None:
            raise ValueError("pixel_values and input_ids must be provided")
        B = pixel_values.shape[0]
        feats = self.encode_image(pixel_values)
        query_embeds, query_mask = self.encode_queries(input_ids, B)
        logits, boxes, e = self._heads(feats, query_embeds, query_mask, B)
        return feats, query_embeds, logits, boxes, e

    @torch.no_grad()
    def __call__(self, pixel_values=None, input_ids=None, attention_mask=None, **kw):
        """[ext] OwlViTForObjectDetection.forward as eval.py:127 calls it (`model(**processor_output)`).  B is taken from
        pixel_values and Q = input_ids.shape[0] // B; query_mask = input_ids[..., 0] > 0.  attention_mask is accepted and
        not applied (module docstring).  Outputs are fp32 and shaped as transformers shapes them: logits (B, P, Q) with
        finfo(float32).min at masked queries, pred_boxes (B, P, 4) cxcywh, image_embeds (B, g, g, C), text_embeds
        (B, Q, D), class_embeds (B, P, D)."""
        feats, query_embeds, logits, boxes, e = self._forward(pixel_values, input_ids, attention_mask, kw)
        B, g = pixel_values.shape[0], self.grid
        ef = e.float()
        class_embeds = (ef / (torch.linalg.norm(ef, dim=-1, keepdim=True) + 1e-6)).reshape(B, self.P, -1)
        return OwlViTDetectionOutput(logits, boxes, feats.float().reshape(B, g, g, -1), query_embeds, class_embeds)

    forward = __call__

    @torch.no_grad()
    def detect(self, pixel_values, input_ids, score_threshold=0.1, nms_threshold=0.5, class_aware=False,
               attention_mask=None):
        """The forward, then post_process + score filter + NMS (`ops.detect_nms`, mode 0) -> `Detections`.  One host
        read, of the counts, at the end."""
        _, _, logits, boxes, _ = self._forward(pixel_values, input_ids, attention_mask, {})
        ob, osc, ol, oi, oc = ops.detect_nms(logits, boxes, score_threshold=score_threshold,
                                             nms_threshold=nms_threshold, class_aware=class_aware)
        return Detections(ob, osc, ol, oi, oc.tolist())


def from_hf(hf_model, device="cuda"):
    """A loaded transformers `OwlViTForObjectDetection` -> the HIP detector with the same call surface; what
    scripts/owl_vit_eval.py passes to `eval_prompt` as `model`."""
    return HipOwlViTDetector(OwlViTConfig.from_hf(hf_model.config), hf_model.state_dict(), device)
