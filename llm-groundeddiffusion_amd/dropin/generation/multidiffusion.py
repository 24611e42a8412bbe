"""generation/multidiffusion.py of the reference: plugin `multidiffusion`, the MultiDiffusion region-prompt baseline
(`generate.py --run-model multidiffusion`), on the HIP engine (lgd_amd.multidiffusion).

generate.py does not call models.load_sd for this method (it is one of its `custom_models`): the reference builds its
own networks from `models.sd_key` at import.  Here `init()` builds them from the same key through models.load_sd (it
needs diffusers and the checkpoint), `init_synthetic()` builds seeded random networks of the same architecture, and
`run()` calls `init()` the first time when neither was called.

run() reaches one 512 x 512 view with indep_uncond and no normalization; `sd.generate`, the public method of the
reference's MultiDiffusion class, serves panoramas (64 x 64 latent windows at stride 8, get_views) with its defaults
indep_uncond=False and normalization=True.  DDIM.  The image is converted like the reference's T.ToPILImage
(truncating), not rounded like the other plugins'.

One deviation in sd.generate: the background colours come from a device generator seeded with `seed`, which is what
run()'s seed_everything(seed) amounts to; the reference's bare generate() leaves them to the global RNG state."""
from PIL import Image

import models
from lgd_amd import multidiffusion as md_core

from ._common import EasyDict

version = "multidiffusion"

bg_negative = "artifacts, blurry, smooth texture, bad quality, distortions, unrealistic, distorted image, bad proportions, duplicate, headshot, close-up, partial, large, large, huge, gigantic"
fg_negative_prompt = "artifacts, blurry, smooth texture, bad quality, distortions, unrealistic, distorted image, bad proportions, duplicate, headshot, close-up, partial, large, large, huge, gigantic, cut-out, partial, occluded, weird"

sd_kw = dict(H=512, W=512)

get_views = md_core.get_views


class MultiDiffusion(EasyDict):
    """`sd`: EasyDict(sampler, encoder, tokenizer, text_encoder, device) with the reference class's generate()."""

    def generate(self, masks, prompts, negative_prompts="", height=512, width=2048, num_inference_steps=50,
                 guidance_scale=7.5, bootstrapping=20, indep_uncond=False, normalization=True, seed=None):
        """generation/multidiffusion.py:161-285 -> PIL image (width x height).  masks: (P, 1, height/8, width/8) float,
        row 0 the background; prompts: P strings; negative_prompts: P strings, or one string for all of them.  seed is
        required (the reference's torch.manual_seed(None) fails too)."""
        if seed is None:
            raise TypeError("seed is required: the reference seeds the start latent with torch.manual_seed(seed)")
        if self.tokenizer is None or self.text_encoder is None:
            raise RuntimeError("no tokenizer / text encoder: init_synthetic() needs stand-ins for them")
        prompts = [prompts] if isinstance(prompts, str) else list(prompts)
        P = len(prompts)
        negs = [negative_prompts] * P if isinstance(negative_prompts, str) else list(negative_prompts)
        print(f"With bootstrapping ({bootstrapping} steps)" if bootstrapping else "No bootstrapping")
        print(prompts)
        draws = md_core.draw_randomness(self.encoder, self.device, seed, bootstrapping, P, num_inference_steps,
                                        in_channels=self.sampler.eng.cfg.in_channels, size=(height, width),
                                        n_views=len(get_views(height, width)), bg_size=md_core.SIZE)
        texts = md_core.encode_texts(self.tokenizer, self.text_encoder, prompts, negs, self.device)
        out = md_core.multidiffusion_generate(self.sampler, texts, masks, draws["start_latent"], draws["bg_latents"],
                                              draws["picks"], steps=num_inference_steps, guidance_scale=guidance_scale,
                                              n_boot=bootstrapping, indep_uncond=indep_uncond,
                                              normalization=normalization)
        return Image.fromarray(out["image"])


sd = None          # MultiDiffusion(sampler, encoder, tokenizer, text_encoder, device) once init() / init_synthetic() ran


def init(device="cuda"):
    """Builds the networks of models.sd_key (generation/multidiffusion.py:353-356): UNet, text tower and VAE decoder
    through models.load_sd, the VAE encoder of the same checkpoint on the HIP kernels."""
    global sd
    try:
        from diffusers import AutoencoderKL
    except ImportError as e:
        raise RuntimeError("generation.multidiffusion.init() loads models.sd_key through diffusers, which is not "
                           "installed here; use init_synthetic() for seeded random weights") from e
    if not models.sd_key:
        raise RuntimeError("models.sd_key is not set (generate.py sets it before importing the plugin)")
    from lgd_amd.vae import HipVAEEncoder
    md = models.load_sd(models.sd_key)
    vae = AutoencoderKL.from_pretrained(models.sd_key, subfolder="vae")
    sd = MultiDiffusion(sampler=md.sampler, encoder=HipVAEEncoder(vae.state_dict(), device), tokenizer=md.tokenizer,
                        text_encoder=md.text_encoder, device=device)
    return sd


def init_synthetic(name="sd15", seed=0, device="cuda", tokenizer=None, text_encoder=None):
    """Offline stand-in for init(): the UNet config `name` and the SD VAE with seeded random parameters (the decoder
    and encoder of one seeded AutoencoderKL state dict).  There is no tokenizer or text tower offline: pass stand-ins."""
    global sd
    from lgd_amd import vae as _vae
    md = models.load_synthetic(name, seed=seed, device=device, with_vae=False)
    state = _vae.synth_aekl_state_dict(seed=seed)
    md.sampler.vae = _vae.HipVAEDecoder(state, device)
    sd = MultiDiffusion(sampler=md.sampler, encoder=_vae.HipVAEEncoder(state, device), tokenizer=tokenizer,
                        text_encoder=text_encoder, device=device)
    return sd


def run(gen_boxes, bg_prompt, original_ind_base=None, bootstrapping=20, generate_kw=None, first_top=False, steps=50,
        guidance_scale=10.0, extra_neg_prompt=""):
    """generation/multidiffusion.py:383-451 -> EasyDict(image=<PIL.Image>)."""
    if generate_kw:
        # the reference passes every key of generate() explicitly and spreads generate_kw after them: any key is a
        # "got multiple values for keyword argument" TypeError there
        raise TypeError(f"generate() got multiple values for keyword argument '{next(iter(generate_kw))}'")
    if sd is None:
        init()
    if sd.tokenizer is None or sd.text_encoder is None:
        raise RuntimeError("no tokenizer / text encoder: init_synthetic() needs stand-ins for them")
    print(f"gen_boxes = {gen_boxes}")
    print(f'bg_prompt = "{bg_prompt}"')
    print(f'extra_neg_prompt = "{extra_neg_prompt}"')
    prep = md_core.prepare(gen_boxes, bg_prompt, bg_negative, fg_negative_prompt, extra_neg_prompt=extra_neg_prompt,
                           first_top=first_top)
    P = len(prep["prompts"])
    if original_ind_base is None:
        raise TypeError("original_ind_base (the seed) is required: the reference seeds generate() with it")
    draws = md_core.draw_randomness(sd.encoder, sd.device, original_ind_base, bootstrapping, P, steps,
                                    in_channels=sd.sampler.eng.cfg.in_channels, size=(sd_kw["H"], sd_kw["W"]))
    texts = md_core.encode_texts(sd.tokenizer, sd.text_encoder, prep["prompts"], prep["negative_prompts"], sd.device)
    out = md_core.multidiffusion_generate(sd.sampler, texts, prep["masks"], draws["start_latent"], draws["bg_latents"],
                                          draws["picks"], steps=steps, guidance_scale=guidance_scale,
                                          n_boot=bootstrapping)
    return EasyDict(image=Image.fromarray(out["image"]))

