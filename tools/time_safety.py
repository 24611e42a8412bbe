"""Time per call of `HipSafetyChecker.check_device` — processor, CLIP ViT-L/14 tower, projection, concept head and
blanking of a uint8 batch that is already on the GPU — at the released checker's geometry (224 x 224, 257 tokens, 1024
wide, 24 layers, 768-wide projection, 3 + 17 concepts) with seeded synthetic weights (no checkpoint is loaded), on
512 x 512 images, B = 1 and B = 8: eager, and replayed from one captured graph.  In the same process transformers' own
`CLIPVisionModelWithProjection` runs in fp16 on the same GPU on pixel_values that are already there, followed by the
reference's host rule (`.cpu().float().numpy()`, the Python loop per image and concept): the reference's path without
its CLIPImageProcessor, which runs on the host.  The three ALTERNATE window by window after untimed warm-up calls; a
window is `--iters` calls between device synchronisations, timed on the host clock (the reference's rule ends on the
host).  Medians and the spread over `--windows` windows are printed, one JSON line at the end.

    python tools/time_safety.py [--batches 1 8] [--iters 20] [--windows 5] [--layers 24]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lgd_amd  # noqa: E402,F401
from lgd_amd.safety import HipSafetyChecker, SafetyConfig, synth_state_dict  # noqa: E402


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def host_rule(image_embeds, special, special_w, concepts, concept_w):
    """[ext] StableDiffusionSafetyChecker.forward behind the projection, as diffusers 0.18.0 writes it."""
    n = lambda x: x / x.norm(dim=-1, keepdim=True)
    special_cos = (n(image_embeds) @ n(special).t()).cpu().float().numpy()
    cos = (n(image_embeds) @ n(concepts).t()).cpu().float().numpy()
    flags = []
    for i in range(cos.shape[0]):
        adjustment, hit = 0.0, False
        for j in range(special_cos.shape[1]):
            if round(special_cos[i][j] - special_w[j] + adjustment, 3) > 0:
                adjustment = 0.01
        for j in range(cos.shape[1]):
            hit = hit or round(cos[i][j] - concept_w[j] + adjustment, 3) > 0
        flags.append(hit)
    return flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU")
    import transformers
    dev = torch.device("cuda:0")
    cfg = SafetyConfig(num_hidden_layers=a.layers)
    sd = synth_state_dict(cfg, seed=3)
    ours = HipSafetyChecker(cfg, sd, dev)
    hf = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(
        image_size=cfg.image_size, patch_size=cfg.patch_size, hidden_size=cfg.hidden_size,
        intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
        num_attention_heads=cfg.num_attention_heads, projection_dim=cfg.projection_dim))
    hf.load_state_dict({k[len("vision_model."):] if k.startswith("vision_model.vision_model.") else k: v
                        for k, v in sd.items() if "embeds" not in k})
    hf = hf.to(dev).half().eval()
    special, concepts = sd["special_care_embeds"].to(dev).half(), sd["concept_embeds"].to(dev).half()
    special_w, concept_w = sd["special_care_embeds_weights"].numpy(), sd["concept_embeds_weights"].numpy()
    result = dict(geometry="ViT-L/14", layers=a.layers, tokens=ours.P + 1, image=512, iters=a.iters, windows=a.windows,
                  batches={})
    for B in a.batches:
        images = torch.from_numpy(np.random.default_rng(B).integers(0, 256, (B, 512, 512, 3), dtype=np.uint8)).to(dev)
        static = images.clone()
        pv16 = ours.processor.pixel_values(images, dtype=torch.float16)

        def eager():
            return ours.check_device(static)

        def theirs():
            with torch.no_grad():
                return host_rule(hf(pixel_values=pv16).image_embeds, special, special_w, concepts, concept_w)
        for _ in range(3):                                         # every shape of the timed windows, untimed
            eager()
            theirs()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eager()
        graph.replay()
        t = dict(eager=[], graph=[], theirs=[])
        for _ in range(a.windows):
            t["eager"].append(window(eager, a.iters))
            t["graph"].append(window(graph.replay, a.iters))
            t["theirs"].append(window(theirs, a.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        result["batches"][str(B)] = dict(
            check_device_eager_ms=med["eager"] * 1e3, eager_ms_min_max=[min(t["eager"]) * 1e3, max(t["eager"]) * 1e3],
            check_device_graph_ms=med["graph"] * 1e3, graph_ms_min_max=[min(t["graph"]) * 1e3, max(t["graph"]) * 1e3],
            transformers_fp16_plus_host_rule_ms=med["theirs"] * 1e3,
            transformers_ms_min_max=[min(t["theirs"]) * 1e3, max(t["theirs"]) * 1e3],
            ratio_transformers_over_graph=med["theirs"] / med["graph"], ratio_transformers_over_eager=med["theirs"] / med["eager"])
        print(f"# B={B}: check_device eager {med['eager'] * 1e3:.3f} ms/call [{min(t['eager']) * 1e3:.3f}, "
              f"{max(t['eager']) * 1e3:.3f}], from one graph {med['graph'] * 1e3:.3f} ms/call [{min(t['graph']) * 1e3:.3f}, "
              f"{max(t['graph']) * 1e3:.3f}]; transformers fp16 forward + host rule {med['theirs'] * 1e3:.3f} ms/call "
              f"[{min(t['theirs']) * 1e3:.3f}, {max(t['theirs']) * 1e3:.3f}]", flush=True)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
