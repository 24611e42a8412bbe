"""TEST INFRASTRUCTURE — the cases of tests/golden/run_multidiffusion_panorama_tiny.npz
(tools/make_golden_multidiffusion_panorama.py): the reference's own MultiDiffusion.generate over several views, with the
`tiny` UNet, the tests/fake_text.py text side and md_golden_cases.StandInVAE.  Masks are built here at latent size, so
both sides read the same arrays; everything else is regenerated from the recorded seeds."""
import torch

UNET = "tiny"
GUIDANCE = 7.5
SAMPLE = 64            # elements kept per UNet input row (seeded index into C * 64 * 64)
BG_SIZE = (512, 512)   # get_random_background encodes 512 x 512 images whatever the panorama's size

# pixels (height, width) -> latent (height / 8, width / 8); views = get_views(height, width), checked by the tool
# boxes: per foreground prompt (y0, x0, y1, x1) at latent size; `soft`: that prompt's mask is 0.7 inside its box and 0.3
# on a 4-wide frame around it, so the >= 0.5 binarisation of the bootstrapping blend and the raw blend weight differ
CASES = [
    dict(name="grid", height=576, width=640, views=6, prompts=["a wide valley", "a red barn", "a tall oak"],
         boxes=[(10, 6, 50, 40), (20, 44, 66, 76)], soft=0, steps=8, n_boot=3, indep_uncond=False, normalization=True,
         seed=81),
    dict(name="strip", height=512, width=768, views=5, prompts=["a sea shore", "a lighthouse", "a sail boat"],
         boxes=[(4, 8, 60, 36), (24, 52, 56, 92)], soft=None, steps=8, n_boot=3, indep_uncond=True, normalization=True,
         seed=82),
    dict(name="sum", height=512, width=576, views=2, prompts=["a meadow", "a white horse"],
         boxes=[(12, 20, 52, 60)], soft=None, steps=2, n_boot=1, indep_uncond=True, normalization=False, seed=83),
    dict(name="uncovered", height=512, width=544, views=1, prompts=["a quiet lake"], boxes=[], soft=None, steps=4,
         n_boot=0, indep_uncond=False, normalization=True, seed=84),
]
NEGATIVE = "blurry, dark"
TF_CASE, TF_STEPS = "grid", (2, 3)       # teacher-forced steps: whole latents before these are kept


def case(name):
    return next(c for c in CASES if c["name"] == name)


def build_masks(c):
    """(P, 1, Hp, Wp) float32: row 0 the background = 1 - sum of the foreground masks, clamped at 0."""
    hp, wp = c["height"] // 8, c["width"] // 8
    fg = torch.zeros((len(c["boxes"]), 1, hp, wp), dtype=torch.float32)
    for i, (y0, x0, y1, x1) in enumerate(c["boxes"]):
        if c["soft"] == i:
            fg[i, 0, max(y0 - 4, 0):y1 + 4, max(x0 - 4, 0):x1 + 4] = 0.3
            fg[i, 0, y0:y1, x0:x1] = 0.7
        else:
            fg[i, 0, y0:y1, x0:x1] = 1.0
    for i in range(1, len(c["boxes"])):                      # disjoint: an earlier box keeps its pixels
        fg[i] = fg[i] * (fg[:i].sum(0) == 0)
    bg = (1 - fg.sum(dim=0, keepdim=True)).clamp_min(0)
    return torch.cat([bg, fg])


def negatives(c):
    return [NEGATIVE] * len(c["prompts"])
