import os
os.environ["HF_HUB_OFFLINE"] = "1"          # never reach a network, whatever is imported below
os.environ["TRANSFORMERS_OFFLINE"] = "1"
"""ORACLE TEST INFRASTRUCTURE (needs the reference tree; CPU) — golden of the MultiDiffusion baseline.

Imports the reference's OWN, unmodified generation/multidiffusion.py through oracle/ref_harness.py and calls its run()
on CPU, with stand-ins for what its import loads from the hub:
  * torchvision (not installed): a stub module whose transforms.ToPILImage is torchvision's float path,
    pic.mul(255).byte() -> PIL image;
  * CLIPTokenizer / CLIPTextModel.from_pretrained -> tests/fake_text.py objects (checked before the import);
  * diffusers (the oracle stub module, extended at runtime): UNet2DConditionModel.from_pretrained -> the reference UNet
    with the seeded `tiny` weights (ref_harness.build_ref_unet), AutoencoderKL.from_pretrained -> the CPU stand-in VAE
    of tests/md_golden_cases.py with a DiagonalGaussian posterior, DDIMScheduler.from_pretrained -> the stub DDIM with
    diffusers 0.18.0's add_noise and a subscriptable step output.
show_boxes / show_masks (matplotlib files) are replaced by no-ops after the import; nothing else is touched.

Recorded per case (tests/md_golden_cases.py): colours, picks, the start latent (sample + checksum), masks, prompts and negative prompts, the
encoded backgrounds as a seeded element sample with checksums, every step's UNet input rows as a seeded element sample,
the final latent whole and the uint8 image (every 8th pixel + checksum); for
the teacher-forced case the whole latents before TF_STEPS.  Plus the reference's run() signature and string constants
(read with ast).

    python tools/make_golden_multidiffusion.py [--out PATH]   # default tests/golden/run_multidiffusion_tiny.npz
"""
import argparse
import ast
import json
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lgd_amd  # noqa: E402,F401
from lgd_amd import weights  # noqa: E402
import ref_harness as rh  # noqa: E402
import md_golden_cases as cases  # noqa: E402
from fake_text import FakeTextEncoder, FakeTokenizer  # noqa: E402


def surface(ref_root):
    """run()'s parameters and defaults and the module's string constants, read with ast (nothing executed)."""
    tree = ast.parse(open(os.path.join(ref_root, "generation", "multidiffusion.py")).read())
    constants = {n.targets[0].id: n.value.value for n in tree.body
                 if isinstance(n, ast.Assign) and isinstance(n.value, ast.Constant) and isinstance(n.value.value, str)}
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "run")
    params = [a.arg for a in fn.args.args]
    defaults = [ast.literal_eval(d) for d in fn.args.defaults]
    return dict(constants=constants, params=params, defaults=dict(zip(params[len(params) - len(defaults):], defaults)))


def _install_stubs(cfg, rec):
    tv = types.ModuleType("torchvision")
    tr = types.ModuleType("torchvision.transforms")

    class ToPILImage:
        def __call__(self, pic):
            return Image.fromarray(pic.mul(255).byte().permute(1, 2, 0).numpy())
    tr.ToPILImage = ToPILImage
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr

    import transformers
    cx = cfg.cross_attention_dim

    def tok_from_pretrained(*a, **k):
        return FakeTokenizer()

    def te_from_pretrained(*a, **k):
        te = FakeTextEncoder(cx, device="cpu")
        te.to = lambda *a, **k: te
        return te
    transformers.CLIPTokenizer.from_pretrained = staticmethod(tok_from_pretrained)
    transformers.CLIPTextModel.from_pretrained = staticmethod(te_from_pretrained)

    import diffusers
    from diffusers import DDIMScheduler as _StubDDIM

    class _StepOut(dict):
        __getattr__ = dict.__getitem__

    class DDIM(_StubDDIM):
        def step(self, model_output, timestep, sample, eta=0.0, **kw):
            o = super().step(model_output, timestep, sample, eta=eta)
            return _StepOut(prev_sample=o.prev_sample, pred_original_sample=o.pred_original_sample)

        def add_noise(self, original_samples, noise, timesteps):      # [ext] diffusers 0.18.0
            alphas_cumprod = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)
            timesteps = timesteps.to(original_samples.device)
            sqrt_alpha_prod = alphas_cumprod[timesteps] ** 0.5
            sqrt_alpha_prod = sqrt_alpha_prod.flatten()
            while len(sqrt_alpha_prod.shape) < len(original_samples.shape):
                sqrt_alpha_prod = sqrt_alpha_prod.unsqueeze(-1)
            sqrt_one_minus_alpha_prod = (1 - alphas_cumprod[timesteps]) ** 0.5
            sqrt_one_minus_alpha_prod = sqrt_one_minus_alpha_prod.flatten()
            while len(sqrt_one_minus_alpha_prod.shape) < len(original_samples.shape):
                sqrt_one_minus_alpha_prod = sqrt_one_minus_alpha_prod.unsqueeze(-1)
            return sqrt_alpha_prod * original_samples + sqrt_one_minus_alpha_prod * noise

    class UNetLoader:
        @staticmethod
        def from_pretrained(*a, **k):
            unet = rh.build_ref_unet(cfg)
            unet.to = lambda *a, **k: unet
            inner = unet.forward

            def fwd(x, t, encoder_hidden_states=None, **kw):
                rec["inputs"].append(x[: x.shape[0] // 2].clone())
                return inner(x, t, encoder_hidden_states=encoder_hidden_states, **kw)
            unet.forward = fwd
            return unet

    class VAELoader:
        @staticmethod
        def from_pretrained(*a, **k):
            vae = cases.StandInVAE()
            return vae

    diffusers.UNet2DConditionModel = UNetLoader
    diffusers.AutoencoderKL = VAELoader
    diffusers.DDIMScheduler = types.SimpleNamespace(from_pretrained=lambda *a, **k: DDIM(
        prediction_type=cfg.prediction_type))
    # every from_pretrained the module's import runs must be one of the replacements above
    assert transformers.CLIPTokenizer.from_pretrained is tok_from_pretrained
    assert transformers.CLIPTextModel.from_pretrained is te_from_pretrained
    assert diffusers.AutoencoderKL is VAELoader and diffusers.UNet2DConditionModel is UNetLoader


def load_reference(cfg, rec):
    rh.setup()
    _install_stubs(cfg, rec)
    import models
    models.sd_key = "tiny-oracle"
    from generation import multidiffusion as ref_md
    ref_md.show_boxes = lambda *a, **k: None
    ref_md.show_masks = lambda *a, **k: None
    ref_md.device = torch.device("cpu")
    ref_md.sd.device = torch.device("cpu")
    return ref_md


def run_case(ref_md, rec, case):
    name, boxes, bg_prompt, steps, n_boot, first_top, neg, seed = case
    rec["inputs"].clear()
    spy = {}
    sd = ref_md.sd
    orig_gen, orig_rand = sd.generate, torch.rand

    def generate(masks, prompts, negative_prompts, *a, **k):
        spy.update(masks=masks.clone(), prompts=list(prompts), negs=list(negative_prompts))
        return orig_gen(masks, prompts, negative_prompts, *a, **k)

    def rand(*a, **k):
        out = orig_rand(*a, **k)
        spy["colours"] = out.clone()
        return out
    orig_randint, picks = torch.randint, []

    def randint(*a, **k):
        out = orig_randint(*a, **k)
        picks.append(out.clone())
        return out
    sd.generate, torch.rand, torch.randint = generate, rand, randint
    try:
        with torch.no_grad():
            out = ref_md.run(boxes, bg_prompt, original_ind_base=seed, bootstrapping=n_boot, first_top=first_top,
                             steps=steps, guidance_scale=cases.GUIDANCE, extra_neg_prompt=neg)
    finally:
        sd.generate, torch.rand, torch.randint = orig_gen, orig_rand, orig_randint
    P = len(spy["prompts"])
    inputs = torch.stack(rec["inputs"])                                   # (T, P, C, L, L): uncond half = x_k
    start = torch.randn((1, 4, 64, 64), generator=torch.Generator().manual_seed(seed))
    # the latent after step i is what step i+1 feeds prompt 0 (never bootstrapped); the last one is the final latent
    final = rec["final"]
    img = np.asarray(out.image)
    idx = cases.sample_index(4 * 64 * 64)
    r = {
        "colours": spy["colours"].numpy() if n_boot else np.zeros((0, 3), np.float32),
        "picks": (torch.stack(picks) if picks else torch.zeros((0, P - 1), dtype=torch.int64)).numpy(),
        "start_checksum": cases.checksum(start), "start_sample": start.reshape(-1)[idx].numpy(),
        "masks": spy["masks"].numpy(),
        "prompts": np.array(spy["prompts"]), "negative_prompts": np.array(spy["negs"]),
        "inputs_sample": inputs.reshape(inputs.shape[0], P, -1)[:, :, idx].numpy(),
        "final": final.numpy(),
        "image_sub": img[::8, ::8].copy(), "image_checksum": checksum_u8(img),
        "steps": np.int64(steps), "n_boot": np.int64(n_boot), "seed": np.int64(seed),
    }
    if rec.get("bg_latents") is not None:
        b = rec["bg_latents"]
        r["bg_sample"] = b.reshape(b.shape[0], -1)[:, idx].numpy()
        r["bg_checksum"] = cases.checksum(b)
    if name == cases.TF_CASE:
        for s in cases.TF_STEPS:
            r[f"latent_before_{s}"] = inputs[s, 0:1].numpy()                 # x_0 of step s = latent before step s
    return r


def checksum_u8(img):
    a = np.asarray(img, dtype=np.float64)
    return np.array([a.sum(), (a * a).sum()])


def build_arrays():
    torch.set_num_threads(8)
    cfg = weights.CONFIGS[cases.UNET]
    rec = dict(inputs=[])
    ref_md = load_reference(cfg, rec)
    # the encoded backgrounds and the final latent, read at the reference's own boundaries
    sd = ref_md.sd
    orig_bg, orig_dec = sd.get_random_background, sd.decode_latents

    def get_random_background(n):
        out = orig_bg(n)
        rec["bg_latents"] = out.clone()
        return out

    def decode_latents(latents):
        rec["final"] = latents.clone()
        return orig_dec(latents)
    sd.get_random_background, sd.decode_latents = get_random_background, decode_latents
    arrs = dict(sample_index=cases.sample_index(4 * 64 * 64))
    for case in cases.CASES:
        rec["bg_latents"] = None
        r = run_case(ref_md, rec, case)
        for k, v in r.items():
            arrs[f"{case[0]}/{k}"] = v
        print(f"{case[0]}: P={len(r['prompts'])} steps={int(r['steps'])} final |x| max {np.abs(r['final']).max():.4f}")
    return arrs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "run_multidiffusion_tiny.npz"))
    ap.add_argument("--surface-out", default=os.path.join(ROOT, "tests", "golden", "multidiffusion_surface.json"))
    a = ap.parse_args()
    s = surface(rh.REF_ROOT)
    json.dump(dict(source="generation/multidiffusion.py", **s), open(a.surface_out, "w"), indent=1)
    np.savez_compressed(a.out, **build_arrays())
    print("wrote", a.out, a.surface_out)
