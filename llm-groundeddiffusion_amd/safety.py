"""The safety checker of the `sd` baseline on the HIP kernels.

The reference's generation/stable_diffusion_generate.py:14,44-49 builds StableDiffusionPipeline with its default
`StableDiffusionSafetyChecker` ([ext, unpinned] diffusers 0.18.0 pipelines/stable_diffusion/safety_checker.py) and returns
`images[0]`: an image the checker flags comes back black.  The checker is

  processor      CLIPImageProcessor: Pillow BICUBIC resize, centre crop, rescale, normalise (clip_processor.py, on
                 `ops.resample_u8`)
  vision tower   a CLIP ViT (ViT-L/14 in the released checkpoints): `vit.clip_vision_trunk`, the tower OWL-ViT's detector
                 runs, pooled at the class token; ViT-L/14's patch vector of 3*14*14 = 588 values is zero-padded to 592 at
                 load (the GEMM reads K in multiples of 8)
  projection     `visual_projection`, one GEMM with an fp32 output
  head           `lgd_safety_head_f32` (csrc/safety.hip): cosines against the 3 special-care and 17 concept embeddings,
                 thresholds, the 0.01 adjustment behind a special-care hit, the decision
  blanking       `lgd_blank_flagged_u8`: flagged images are zeroed in place

`check_device` runs all of it on a uint8 batch that is already on the GPU, device to device with no host read, and (for
square images, after one warm call) inside one captured graph.  `HipSafetyChecker(config, state_dict)` takes the parameter
names of diffusers' module.  No real checkpoint has been loaded by this project's tests: they run seeded weights against
transformers' `CLIPVisionModelWithProjection` and an fp64 restatement of the head."""
from dataclasses import dataclass

import numpy as np
import torch

from . import ops, vit
from .clip_processor import DeviceClipProcessor

F16, F32 = torch.float16, torch.float32

# state-dict entries the checker does not read: the position-index buffer of older transformers versions
UNUSED_KEYS = ("vision_model.vision_model.embeddings.position_ids",)

# [ext] transformers CLIPImageProcessor's defaults: what a Stable Diffusion checkpoint's feature_extractor holds
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def default_processor_config(edge=224):
    return dict(do_resize=True, size={"shortest_edge": edge}, resample=3, do_center_crop=True,
                crop_size={"height": edge, "width": edge}, do_rescale=True, rescale_factor=1.0 / 255.0, do_normalize=True,
                image_mean=CLIP_MEAN, image_std=CLIP_STD)


@dataclass(frozen=True)
class SafetyConfig:
    """The fields of transformers' CLIPVisionConfig that shape the computation (defaults: ViT-L/14, the checker of
    CompVis/stable-diffusion-safety-checker) and the two concept counts."""
    image_size: int = 224
    patch_size: int = 14
    num_channels: int = 3
    hidden_size: int = 1024
    intermediate_size: int = 4096
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    layer_norm_eps: float = 1e-5
    projection_dim: int = 768
    n_concepts: int = 17
    n_special: int = 3

    @classmethod
    def from_hf(cls, v, projection_dim=None, **kw):
        if getattr(v, "hidden_act", "quick_gelu") != "quick_gelu":
            raise RuntimeError("only the quick_gelu CLIP vision tower is implemented")
        return cls(image_size=v.image_size, patch_size=v.patch_size, num_channels=v.num_channels, hidden_size=v.hidden_size,
                   intermediate_size=v.intermediate_size, num_hidden_layers=v.num_hidden_layers,
                   num_attention_heads=v.num_attention_heads, layer_norm_eps=v.layer_norm_eps,
                   projection_dim=projection_dim or v.projection_dim, **kw)


def synth_state_dict(cfg: SafetyConfig, seed=0, concept_threshold=None, special_threshold=None):
    """Seeded weights under diffusers' key names.  concept_threshold / special_threshold: one value for every
    `concept_embeds_weights` / `special_care_embeds_weights` entry (cosines lie in [-1, 1]: -1 flags every image, +1
    none); None draws them around 0.2, where the released checkpoint's lie."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=0.02: torch.randn(*s, generator=g) * std
    C, I, K = cfg.hidden_size, cfg.intermediate_size, cfg.num_channels * cfg.patch_size ** 2
    P = (cfg.image_size // cfg.patch_size) ** 2
    v = "vision_model.vision_model."
    sd = {v + "embeddings.class_embedding": rn(C), v + "embeddings.position_embedding.weight": rn(P + 1, C),
          v + "embeddings.patch_embedding.weight": rn(C, K, std=K ** -0.5).reshape(C, cfg.num_channels, cfg.patch_size,
                                                                                   cfg.patch_size)}

    def ln(p):
        sd[p + ".weight"], sd[p + ".bias"] = 1.0 + rn(C, std=0.1), rn(C, std=0.1)

    def lin(p, n, k):
        sd[p + ".weight"], sd[p + ".bias"] = rn(n, k, std=k ** -0.5), rn(n)
    ln(v + "pre_layrnorm")
    ln(v + "post_layernorm")
    for i in range(cfg.num_hidden_layers):
        p = f"{v}encoder.layers.{i}."
        ln(p + "layer_norm1")
        ln(p + "layer_norm2")
        for n in "qkv":
            lin(f"{p}self_attn.{n}_proj", C, C)
        lin(p + "self_attn.out_proj", C, C)
        lin(p + "mlp.fc1", I, C)
        lin(p + "mlp.fc2", C, I)
    sd["visual_projection.weight"] = rn(cfg.projection_dim, C, std=C ** -0.5)
    sd["concept_embeds"] = rn(cfg.n_concepts, cfg.projection_dim, std=1.0)
    sd["special_care_embeds"] = rn(cfg.n_special, cfg.projection_dim, std=1.0)
    fill = lambda n, t: 0.2 + rn(n, std=0.02) if t is None else torch.full((n,), float(t))
    sd["concept_embeds_weights"] = fill(cfg.n_concepts, concept_threshold)
    sd["special_care_embeds_weights"] = fill(cfg.n_special, special_threshold)
    return sd


class HipSafetyChecker(vit.Tower):
    def __init__(self, config: SafetyConfig, state_dict, device="cuda", processor=None):
        """processor: a DeviceClipProcessor, a CLIPImageProcessor or its configuration (a pipeline's `feature_extractor`);
        None: CLIPImageProcessor's defaults at the tower's image size."""
        cfg = self.cfg = config
        self.dev = dev = torch.device(device)
        sd = state_dict
        w = vit.Weights(sd, dev)
        self.consumed = w.consumed
        h16, f32, lin, ln = w.h16, w.f32, w.lin, w.ln
        C, NH = cfg.hidden_size, cfg.num_attention_heads
        if C % NH or (C // NH) % 8:
            raise RuntimeError("head width must be a multiple of 8")
        if cfg.image_size % cfg.patch_size:
            raise RuntimeError("the image must be whole patches")
        self.grid = g = cfg.image_size // cfg.patch_size
        self.P = g * g

        v = "vision_model.vision_model."
        patch = w[v + "embeddings.patch_embedding.weight"].reshape(C, -1)
        self.patch = h16(torch.nn.functional.pad(patch, (0, -patch.shape[1] % 8)))       # K: 588 -> 592 for ViT-L/14
        pos = f32(w[v + "embeddings.position_embedding.weight"])                         # [P + 1, C]
        if pos.shape[0] != self.P + 1:
            raise RuntimeError("position table does not match the image grid (interpolate_pos_encoding is not implemented)")
        self.cls_pos = f32(w[v + "embeddings.class_embedding"]) + pos[0]
        self.pos = h16(pos[1:])
        self.pre_ln, self.post_ln = ln(v + "pre_layrnorm"), ln(v + "post_layernorm")     # transformers' own spelling
        self.layers = []
        for i in range(cfg.num_hidden_layers):
            p = f"{v}encoder.layers.{i}."
            self.layers.append(vit.Layer(ln1=ln(p + "layer_norm1"), qkv=w.qkv(p + "self_attn"),
                                         out=lin(p + "self_attn.out_proj"), ln2=ln(p + "layer_norm2"),
                                         fc1=lin(p + "mlp.fc1"), fc2=lin(p + "mlp.fc2")))
        self.proj = h16(w["visual_projection.weight"])                                   # [D, C], no bias
        if self.proj.shape[0] % 8 or self.proj.shape[1] != C:
            raise RuntimeError("visual_projection maps the hidden width to a multiple of 8 columns")
        self.concepts, self.concept_w = f32(w["concept_embeds"]), f32(w["concept_embeds_weights"])
        self.special, self.special_w = f32(w["special_care_embeds"]), f32(w["special_care_embeds_weights"])
        if self.special.shape[0] == 0:
            self.special = self.special_w = None
        self.unused = sorted(k for k in sd if k not in self.consumed)
        extra = [k for k in self.unused if k not in UNUSED_KEYS]
        if extra:
            raise RuntimeError(f"state-dict entries the safety checker does not know: {extra}")
        if processor is None:
            processor = default_processor_config(cfg.image_size)
        self.processor = processor if isinstance(processor, DeviceClipProcessor) else DeviceClipProcessor(processor)
        if self.processor.edge != cfg.image_size:
            raise RuntimeError(f"the processor makes {self.processor.edge} x {self.processor.edge} images, the tower takes "
                               f"{cfg.image_size} x {cfg.image_size}")

    # ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def embed(self, pixel_values):
        """pixel_values (B, 3, S, S) -> `image_embeds` fp32 [B, D]: [ext] CLIPVisionModel's pooler_output (post_layernorm
        of the class token) through `visual_projection`."""
        cfg = self.cfg
        B, Cin, Hh, Ww = pixel_values.shape
        if (Cin, Hh, Ww) != (cfg.num_channels, cfg.image_size, cfg.image_size):
            raise ValueError(f"Input image size ({Hh}*{Ww}) doesn't match model ({cfg.image_size}*{cfg.image_size}).")
        pooled = vit.clip_vision_trunk(self, pixel_values, patch_size=cfg.patch_size, heads=cfg.num_attention_heads,
                                       eps=cfg.layer_norm_eps, pooled=True)
        return ops.linear(pooled, self.proj, None, out_f32=True)

    @torch.no_grad()
    def scores(self, pixel_values):
        """-> (scores fp32 [B, n_special + n_concepts], special rows first; flags int32 [B, 2] = (has_nsfw, a
        special-care row hit)), on the device."""
        return ops.safety_head(self.embed(pixel_values), self.special, self.special_w, self.concepts, self.concept_w)

    @torch.no_grad()
    def check_device(self, images_u8):
        """uint8 (N, h, w, 3) on the GPU -> (images_u8 with the flagged images zeroed IN PLACE, flags int32 [N, 2]):
        processor, tower, head and blanking with no host read."""
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3 or not images_u8.is_contiguous():
            raise RuntimeError("check_device: images_u8 is a contiguous uint8 (N, h, w, 3) batch on the device")
        _, flags = self.scores(self.processor.pixel_values(images_u8))
        ops.blank_flagged(images_u8, flags[:, 0])
        return images_u8, flags

    @torch.no_grad()
    def __call__(self, images, clip_input):
        """[ext] StableDiffusionSafetyChecker.forward(images, clip_input) -> (images, has_nsfw_concepts): clip_input is
        the feature extractor's pixel_values; the flagged entries of `images` (a tensor or a numpy array, any dtype,
        batch first) are set to zero as the reference sets them, and has_nsfw_concepts is a host list of bools (one host
        read)."""
        _, flags = self.scores(clip_input)
        has_nsfw = [bool(f) for f in flags[:, 0].tolist()]
        if torch.is_tensor(images) and images.is_cuda and images.dtype == torch.uint8 and images.is_contiguous():
            ops.blank_flagged(images, flags[:, 0])
        else:
            for i, hit in enumerate(has_nsfw):
                if hit:
                    images[i] = torch.zeros_like(images[i]) if torch.is_tensor(images) else np.zeros(images[i].shape)
        return images, has_nsfw

    forward = __call__

    @classmethod
    def synthetic(cls, config: SafetyConfig = None, seed=0, device="cuda", **thresholds):
        """Seeded weights of `config` (default: ViT-L/14 geometry with 2 layers), for tests and offline use."""
        config = config or SafetyConfig(num_hidden_layers=2)
        return cls(config, synth_state_dict(config, seed, **thresholds), device)


def from_diffusers(module, device="cuda", processor=None):
    """A loaded diffusers `StableDiffusionSafetyChecker` (and the pipeline's `feature_extractor` as processor) -> the HIP
    checker with the same call surface.  Like owlvit.from_hf this has never run in this project's tests: they have no
    diffusers and no checkpoint."""
    sd = module.state_dict()
    cfg = SafetyConfig.from_hf(module.config.vision_config, projection_dim=sd["visual_projection.weight"].shape[0],
                               n_concepts=sd["concept_embeds"].shape[0], n_special=sd["special_care_embeds"].shape[0])
    return HipSafetyChecker(cfg, sd, device, processor)


HipSafetyChecker.from_diffusers = staticmethod(from_diffusers)
