"""What the transformer towers outside the UNet share: the CLIP text tower (clip.py; also OWL-ViT's and SDXL's text
towers), the OWL-ViT vision tower (owlvit.py) and the SAM image encoder (sam.py).

  Weights      a state dict on a device: `h16` / `f32` conversion, `lin` / `ln` / fused `qkv` parameter pairs, and the
               record of the keys handed out (`consumed`), from which a tower may refuse entries it does not know
  Layer, block one pre-LN transformer layer: LayerNorm -> fused QKV GEMM -> the tower's own attention -> out-projection
               with residual -> LayerNorm -> fc1 -> activation -> fc2 with residual.  The field names are this module's;
               each tower maps its checkpoint's names when it loads.
  patch_rows   the unfolding of an image into the rows of the patch-embedding GEMM
  clip_vision_trunk  the CLIP vision transformer both OWL-ViT's detector (owlvit.py) and the safety checker (safety.py)
               run: patch GEMM, class token + position table, pre_layernorm, the layers, post_layernorm
  Tower        the `to` / `eval` call surface of an nn.Module user and the cache of tables repeated once per image
"""
from collections import namedtuple

import torch

from . import ops

F16, F32 = torch.float16, torch.float32


class Weights:
    def __init__(self, state_dict, dev):
        self.sd, self.dev, self.consumed = state_dict, dev, set()

    def __getitem__(self, key):
        self.consumed.add(key)
        return self.sd[key]

    def h16(self, t):
        return t.detach().to(self.dev, F16).contiguous()

    def f32(self, t):
        return t.detach().to(self.dev, F32).contiguous()

    def lin(self, p):
        """(W fp16, b fp32) of the linear layer `p`."""
        return self.h16(self[p + ".weight"]), self.f32(self[p + ".bias"])

    def ln(self, p):
        """(gamma, beta) fp32 of the LayerNorm `p`."""
        return self.f32(self[p + ".weight"]), self.f32(self[p + ".bias"])

    def qkv(self, p, names="qkv"):
        """The projections `p.{n}_proj` for n in names as one linear layer: rows [q; k; v]."""
        return (self.h16(torch.cat([self[f"{p}.{n}_proj.weight"] for n in names])),
                self.f32(torch.cat([self[f"{p}.{n}_proj.bias"] for n in names])))


Layer = namedtuple("Layer", "ln1 qkv out ln2 fc1 fc2")


def block(x, L, eps, attend, act):
    """x [rows, C] fp16 -> the layer's output.  `attend(qkv) -> o` is the tower's attention over the fused projection
    [rows, 3C]; act is "quick_gelu" or "gelu" (exact)."""
    h = ops.layernorm(x, L.ln1[0], L.ln1[1], eps)
    o = attend(ops.linear(h, L.qkv[0], L.qkv[1]))
    x = ops.linear(o, L.out[0], L.out[1], res=x)
    h = ops.layernorm(x, L.ln2[0], L.ln2[1], eps)
    h = ops.linear(h, L.fc1[0], L.fc1[1])
    h = ops.quick_gelu(h) if act == "quick_gelu" else ops.act(h, ops.ACT_GELU)
    return ops.linear(h, L.fc2[0], L.fc2[1], res=x)


def patch_rows(pixel_values, grid, patch, dev):
    """(B, Cin, grid*patch, grid*patch) -> [B*grid^2, Cin*patch^2] fp16: one row per patch, in (channel, y, x) order as a
    stride-`patch` convolution's weight reads it."""
    B, Cin = pixel_values.shape[:2]
    return (pixel_values.to(dev, F16).reshape(B, Cin, grid, patch, grid, patch).permute(0, 2, 4, 1, 3, 5)
            .reshape(B * grid * grid, Cin * patch * patch).contiguous())


def clip_vision_trunk(tower, pixel_values, *, patch_size, heads, eps, pooled=False):
    """[ext] transformers CLIPVisionTransformer / OwlViTVisionTransformer.forward up to and including post_layernorm.
    pixel_values (B, Cin, g*patch_size, g*patch_size) -> fp16 [B*(P + 1), C], every token normalised; pooled=True ->
    [B, C], the class token alone (CLIP's pooler_output: LayerNorm is per row, so the other rows are not computed).

    `tower` (a Tower) holds what its loader made of the checkpoint: `patch` fp16 [C, K] (K may be zero-padded past
    Cin*patch_size^2 to a multiple of 8: the rows are padded to match), `pos` fp16 [P, C], `cls_pos` fp32 [C] (class
    embedding + position row 0), `pre_ln`, `post_ln`, `layers` (Layer, quick_gelu), `grid`, `dev`."""
    g, dev = tower.grid, tower.dev
    B = pixel_values.shape[0]
    C = tower.patch.shape[0]
    P, d = g * g, C // heads
    S = P + 1
    rows = patch_rows(pixel_values, g, patch_size, dev)
    if rows.shape[1] != tower.patch.shape[1]:
        rows = torch.nn.functional.pad(rows, (0, tower.patch.shape[1] - rows.shape[1]))
    emb = ops.linear(rows, tower.patch, None, res=tower.rep_rows("pos", tower.pos, B))     # [B*P, C] + position
    x = torch.empty((B, S, C), device=dev, dtype=F16)
    x[:, 0] = tower.cls_pos.to(F16)
    x[:, 1:] = emb.reshape(B, P, C)
    x = ops.layernorm(x.reshape(B * S, C), tower.pre_ln[0], tower.pre_ln[1], eps)
    view = (3 * C, S * 3 * C)

    def attend(qkv):                                                                    # [B*S, 3C]
        o = torch.empty((B * S, C), device=dev, dtype=F16)
        return ops.attn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], o, B, heads, S, S, d, d ** -0.5, q_view=view, k_view=view,
                            v_view=view)
    for L in tower.layers:
        x = block(x, L, eps, attend, "quick_gelu")
    if pooled:
        x = x.reshape(B, S, C)[:, 0].contiguous()
    return ops.layernorm(x, tower.post_ln[0], tower.post_ln[1], eps)


class Tower:
    REP_LIMIT = 32      # SAM keeps six tables per batch size (position + five pre-projected ones): five batch sizes

    def to(self, *_a, **_k):            # call-surface compatibility with nn.Module users
        return self

    def eval(self):
        return self

    def rep_rows(self, key, t, n):
        """`t` repeated n times along its rows (a GEMM's residual operand covers every image), kept per (key, n)."""
        cache = self.__dict__.setdefault("_rep", {})
        if (key, n) not in cache:
            if len(cache) >= self.REP_LIMIT:
                cache.clear()
            cache[key, n] = t.repeat(n, 1).contiguous()
        return cache[key, n]
