import os
os.environ["HF_HUB_OFFLINE"] = "1"          # never reach a network, whatever is imported below
os.environ["TRANSFORMERS_OFFLINE"] = "1"
"""ORACLE TEST INFRASTRUCTURE (needs the reference tree; CPU) — golden of MultiDiffusion over several views.

Imports the reference's OWN, unmodified generation/multidiffusion.py with the stand-ins of
tools/make_golden_multidiffusion.py (tiny UNet, tests/fake_text.py, md_golden_cases.StandInVAE), and for every case of
tests/md_pano_golden_cases.py calls seed_everything(seed) and then `sd.generate(...)` directly on CPU.

Recorded per case: the view list (asserted against the case's hand-counted number), colours, picks (T_boot, V, P-1),
the start latent (sample + checksum), the encoded backgrounds (sample + checksum), every step's per-view UNet input rows
as a seeded element sample (T, V, P, SAMPLE), the final latent whole, the uint8 image (every 8th pixel + checksum), and for
the teacher-forced case the whole latents before TF_STEPS.  Plus the signatures of generate() and get_views() (read with
ast, nothing executed) in multidiffusion_panorama_surface.json.

    python tools/make_golden_multidiffusion_panorama.py [--out PATH] [--surface-out PATH]
"""
import argparse
import ast
import json
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import make_golden_multidiffusion as base  # noqa: E402  (puts the repository, oracle/ and tests/ on sys.path)
from lgd_amd import weights  # noqa: E402
import ref_harness as rh  # noqa: E402
import md_golden_cases as md_cases  # noqa: E402
import md_pano_golden_cases as cases  # noqa: E402


def _signature(fn, skip_self=False):
    params = [a.arg for a in fn.args.args][1 if skip_self else 0:]
    defaults = [ast.literal_eval(d) for d in fn.args.defaults]
    return dict(params=params, defaults=dict(zip(params[len(params) - len(defaults):], defaults)))


def surface(ref_root):
    tree = ast.parse(open(os.path.join(ref_root, "generation", "multidiffusion.py")).read())
    views = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "get_views")
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MultiDiffusion")
    gen = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "generate")
    return dict(source="generation/multidiffusion.py", get_views=_signature(views),
                generate=_signature(gen, skip_self=True))


def run_case(ref_md, rec, c):
    rec["inputs"].clear()
    sd = ref_md.sd
    spy = dict(picks=[], latents=[])
    orig = dict(rand=torch.rand, randint=torch.randint, where=torch.where, bg=sd.get_random_background,
                dec=sd.decode_latents)

    def rand(*a, **k):
        out = orig["rand"](*a, **k)
        spy["colours"] = out.clone()
        return out

    def randint(*a, **k):
        out = orig["randint"](*a, **k)
        spy["picks"].append(out.clone())
        return out

    def where(*a, **k):                                     # line 280: the latent after each step
        out = orig["where"](*a, **k)
        spy["latents"].append(out.clone())
        return out

    def get_random_background(n):
        out = orig["bg"](n)
        spy["bg"] = out.clone()
        return out

    def decode_latents(latents):
        spy["final"] = latents.clone()
        return orig["dec"](latents)
    masks = cases.build_masks(c)
    P, T, n_boot, seed = len(c["prompts"]), c["steps"], c["n_boot"], c["seed"]
    views = ref_md.get_views(c["height"], c["width"])
    assert len(views) == c["views"], (c["name"], len(views), c["views"])
    V = len(views)
    torch.rand, torch.randint, torch.where = rand, randint, where
    sd.get_random_background, sd.decode_latents = get_random_background, decode_latents
    try:
        with torch.no_grad():
            ref_md.seed_everything(seed)
            img = sd.generate(masks, c["prompts"], cases.negatives(c), c["height"], c["width"], T,
                              guidance_scale=cases.GUIDANCE, bootstrapping=n_boot, indep_uncond=c["indep_uncond"],
                              normalization=c["normalization"], seed=seed)
    finally:
        torch.rand, torch.randint, torch.where = orig["rand"], orig["randint"], orig["where"]
        sd.get_random_background, sd.decode_latents = orig["bg"], orig["dec"]
    hp, wp = c["height"] // 8, c["width"] // 8
    inputs = torch.stack(rec["inputs"]).reshape(T, V, P, 4, 64, 64)          # one UNet call per step and view
    assert len(spy["latents"]) == T and torch.equal(spy["latents"][-1], spy["final"])
    start = torch.randn((1, 4, hp, wp), generator=torch.Generator().manual_seed(seed))
    img = np.asarray(img)
    assert img.shape == (c["height"], c["width"], 3)
    idx = md_cases.sample_index(4 * 64 * 64, n=cases.SAMPLE)
    sidx = md_cases.sample_index(4 * hp * wp)
    n_pick = min(n_boot, T)
    r = {
        "views": np.array(views, dtype=np.int64).reshape(V, 4),
        "colours": spy["colours"].numpy() if n_boot else np.zeros((0, 3), np.float32),
        "picks": (torch.stack(spy["picks"]).reshape(n_pick, V, P - 1) if spy["picks"]
                  else torch.zeros((0, V, P - 1), dtype=torch.int64)).numpy(),
        "start_checksum": md_cases.checksum(start), "start_sample": start.reshape(-1)[sidx].numpy(),
        "inputs_sample": inputs.reshape(T, V, P, -1)[..., idx].numpy(),
        "final": spy["final"].numpy(),
        "image_sub": img[::8, ::8].copy(), "image_checksum": base.checksum_u8(img),
    }
    if n_boot:
        b = spy["bg"]
        assert tuple(b.shape) == (n_boot, 4, 64, 64)
        r["bg_sample"] = b.reshape(n_boot, -1)[:, idx].numpy()
        r["bg_checksum"] = md_cases.checksum(b)
    if c["name"] == cases.TF_CASE:
        for s in cases.TF_STEPS:
            r[f"latent_before_{s}"] = spy["latents"][s - 1].numpy()
    return r


def build_arrays():
    torch.set_num_threads(8)
    cfg = weights.CONFIGS[cases.UNET]
    rec = dict(inputs=[])
    ref_md = base.load_reference(cfg, rec)
    arrs = dict(sample_index=md_cases.sample_index(4 * 64 * 64, n=cases.SAMPLE))
    for c in cases.CASES:
        r = run_case(ref_md, rec, c)
        for k, v in r.items():
            arrs[f"{c['name']}/{k}"] = v
        print(f"{c['name']}: V={len(r['views'])} P={len(c['prompts'])} steps={c['steps']} "
              f"final |x| max {np.abs(r['final']).max():.4f}")
    return arrs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "run_multidiffusion_panorama_tiny.npz"))
    ap.add_argument("--surface-out",
                    default=os.path.join(ROOT, "tests", "golden", "multidiffusion_panorama_surface.json"))
    a = ap.parse_args()
    json.dump(surface(rh.REF_ROOT), open(a.surface_out, "w"), indent=1)
    np.savez_compressed(a.out, **build_arrays())
    print("wrote", a.out, a.surface_out)
