"""generation/stable_diffusion_generate.py of the reference: plugin `sd`, the plain Stable Diffusion baseline
(`generate.py --run-model sd`), on the HIP engine.  The reference builds StableDiffusionPipeline.from_pretrained(sd_key)
(stable_diffusion_generate.py:13); here the engine and weights already in `models.model_dict` (generate.py:118-123 loads
the same key) run the pipeline's loop — classifier-free guidance and the checkpoint's own PNDMScheduler (PLMS,
skip_prk_steps; lgd_amd.scheduler.PNDMScheduler.from_config) — through models.pipelines.generate's sampler.

The pipeline's safety checker (a CLIP vision model that blanks the images it flags) runs when `models.model_dict` carries
one (`models.load_sd(..., safety_checker=True)` or LGD_SAFETY_CHECKER=1; lgd_amd.safety.HipSafetyChecker, on the device
between the VAE and the host copy): a flagged image comes back black, as from the reference, and the result says so in
`nsfw_content_detected`.  Without one, the default, images are returned as the pipeline returns them with the checker
switched off."""
import torch
from PIL import Image

import models
from lgd_amd.pipeline import sd_generate_batch
from lgd_amd.scheduler import PNDMScheduler

from ._common import DEFAULT_OVERALL_NEGATIVE_PROMPT, EasyDict

version = "sd"

latent_ratio = 8
num_total_steps = 50                    # stable_diffusion_generate.py:24-26
generate_guidance_scale = 7.5

bg_negative = DEFAULT_OVERALL_NEGATIVE_PROMPT


def image_scale():
    """(h, w): the pipeline's default size, unet.config.sample_size * vae_scale_factor (512 x 512 for SD 1.5)."""
    s = models.model_dict.unet.config.sample_size * latent_ratio
    return s, s


def negative_prompt(extra_neg_prompt=""):
    """stable_diffusion_generate.py:39-42."""
    return extra_neg_prompt + ", " + bg_negative if extra_neg_prompt else bg_negative


def start_latents(seed, in_channels, h, w):
    """What the fp32 pipeline's prepare_latents draws: randn_tensor with torch.Generator("cuda").manual_seed(seed) on
    the device (init_noise_sigma is 1 for PNDM)."""
    generator = torch.Generator("cuda").manual_seed(seed)
    return torch.randn((1, in_channels, h // latent_ratio, w // latent_ratio), generator=generator, device="cuda",
                       dtype=torch.float32)


def run(prompt, seed=100, extra_neg_prompt=""):
    """stable_diffusion_generate.py:32-51 -> EasyDict(image=<PIL.Image>), with a checker in model_dict
    EasyDict(image=<PIL.Image>, nsfw_content_detected=<bool>)."""
    md = models.model_dict
    print(f"prompt: {prompt}")
    text = models.encode_prompts(tokenizer=md.tokenizer, text_encoder=md.text_encoder, prompts=[prompt],
                                 negative_prompt=negative_prompt(extra_neg_prompt), return_full_only=True)
    h, w = image_scale()
    scheduler = PNDMScheduler.from_config(md.scheduler)
    lat = start_latents(seed, md.unet.config.in_channels, h, w) * scheduler.init_noise_sigma
    checker = md.get("safety_checker")
    if checker is None:
        _, images = sd_generate_batch(md.sampler, [text.float()], lat, num_total_steps,
                                      guidance_scale=generate_guidance_scale, scheduler=scheduler)
        return EasyDict(image=Image.fromarray(images[0]))
    _, images, flags = sd_generate_batch(md.sampler, [text.float()], lat, num_total_steps,
                                         guidance_scale=generate_guidance_scale, scheduler=scheduler, safety_checker=checker)
    return EasyDict(image=Image.fromarray(images[0]), nsfw_content_detected=bool(flags[0, 0]))
