"""models/models.py of the reference: process-global model handles (`sd_key`, `sd_version`,
`model_dict`), prompt encoding and the loader.  `encode_prompts` / `process_input_embeddings` are boundary glue
whose behaviour the callers prescribe (tokenise, pad to 77, encode uncond + cond, concatenate): they follow
models/models.py:63-109 closely by necessity.  `model_dict.unet` is the HIP engine wrapped in the
reference's UNet2DConditionModel call surface."""
import torch

from lgd_amd import weights as _weights
from lgd_amd.sampler import LMDSampler
from lgd_amd.scheduler import (DDIMInverseScheduler, DDIMScheduler, DPMSolverMultistepScheduler, EulerDiscreteScheduler,
                               LMSDiscreteScheduler)
from lgd_amd.unet import UNetEngine
from utils import torch_device  # noqa: F401

from .unet_2d_condition import UNet2DConditionModel

# set by generate.py (generate.py:104-123)
sd_key = ""
sd_version = ""
model_dict = None


class _EasyDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


# `generate.py --scheduler NAME` -> load_sd(scheduler_cls=diffusers.schedulers.NAME) (models/models.py:50-53): what the HIP
# path serves, and what it refuses by name with the reason
SERVED_SCHEDULERS = ("DDIMScheduler", "DPMSolverMultistepScheduler", "EulerDiscreteScheduler", "LMSDiscreteScheduler")
_TWO_EVALUATIONS = "takes two UNet evaluations per step, which the one-evaluation denoising loop of the HIP path does not run"
_UNSEEDED_NOISE = ("adds noise in every step from a generator the reference does not seed (scheduler.step is called without "
                   "one), so its output is not reproducible there either")
REFUSED_SCHEDULERS = {"HeunDiscreteScheduler": _TWO_EVALUATIONS, "KDPM2DiscreteScheduler": _TWO_EVALUATIONS,
                      "EulerAncestralDiscreteScheduler": _UNSEEDED_NOISE, "KDPM2AncestralDiscreteScheduler": _UNSEEDED_NOISE,
                      "DPMSolverSDEScheduler": _UNSEEDED_NOISE}


def resolve_scheduler(scheduler_cls=None, use_dpm_multistep_scheduler=False, scheduler_config=None,
                      prediction_type="epsilon"):
    """models/models.py:45-53 on the HIP path: (scheduler_cls — a class or its name —, use_dpm_multistep_scheduler, the
    checkpoint's scheduler_config.json fields, the UNet's prediction type) -> one of lgd_amd.scheduler's objects, as
    `scheduler_cls.from_pretrained(key, subfolder="scheduler")` configures that class.  Pure: no device, no checkpoint.
    DDIM honours only what its eta = 0 path uses, anything else must match; the sigma-space classes go through their
    `from_config`, so a config without `timestep_spacing` gives the class default "linspace"."""
    sc = dict(scheduler_config or {})
    name = None if scheduler_cls is None else getattr(scheduler_cls, "__name__", str(scheduler_cls))
    if name is not None and use_dpm_multistep_scheduler:
        raise AssertionError("`use_dpm_multistep_scheduler` cannot be used with `scheduler_cls`")     # models.py:52
    if name is None:
        name = "DPMSolverMultistepScheduler" if use_dpm_multistep_scheduler else "DDIMScheduler"      # models.py:46-49
    if name in REFUSED_SCHEDULERS:
        raise RuntimeError(f"scheduler {name} {REFUSED_SCHEDULERS[name]}")
    if name not in SERVED_SCHEDULERS:
        raise RuntimeError(f"scheduler {name} is not implemented on the HIP path (served: {', '.join(SERVED_SCHEDULERS)})")
    for k, want in (("beta_schedule", "scaled_linear"), ("clip_sample", False), ("set_alpha_to_one", False)):
        if k in sc and sc[k] != want and (k == "beta_schedule" or name == "DDIMScheduler"):
            raise RuntimeError(f"scheduler_config.{k}={sc[k]!r} is not supported on the HIP path (expects {want!r})")
    if "prediction_type" in sc and sc["prediction_type"] != prediction_type:
        raise RuntimeError("scheduler prediction_type disagrees with the UNet config")
    skw = dict(num_train_timesteps=sc.get("num_train_timesteps", 1000), beta_start=sc.get("beta_start", 0.00085),
               beta_end=sc.get("beta_end", 0.012), prediction_type=prediction_type)
    if name == "DPMSolverMultistepScheduler":
        return DPMSolverMultistepScheduler(**skw)
    if name == "DDIMScheduler":
        return DDIMScheduler(steps_offset=sc.get("steps_offset", 1), **skw)
    cls = EulerDiscreteScheduler if name == "EulerDiscreteScheduler" else LMSDiscreteScheduler
    return cls.from_config(dict(sc, beta_schedule="scaled_linear", **skw))


def build_model_dict(cfg, state_dict, vae=None, tokenizer=None, text_encoder=None, device="cuda",
                     dtype=torch.float16, scheduler_config=None, use_dpm_multistep_scheduler=False,
                     load_inverse_scheduler=False, scheduler_cls=None):
    """model_dict contract of models/models.py:55: vae, tokenizer, text_encoder, unet, scheduler, dtype, and with
    load_inverse_scheduler (models/models.py:57-59) `inverse_scheduler` = DDIMInverseScheduler.from_config(scheduler.config).
    scheduler_config: the checkpoint's own scheduler_config.json fields (models/models.py:49 reads them through
    DDIMScheduler.from_pretrained); scheduler_cls / use_dpm_multistep_scheduler: `resolve_scheduler`."""
    sched = resolve_scheduler(scheduler_cls, use_dpm_multistep_scheduler, scheduler_config, cfg.prediction_type)
    eng = UNetEngine(cfg, device, state_dict)
    unet = UNet2DConditionModel(eng)
    md = _EasyDict(vae=vae, tokenizer=tokenizer, text_encoder=text_encoder, unet=unet, scheduler=sched, dtype=dtype)
    md["sampler"] = LMDSampler(eng, sched, vae=vae)
    if load_inverse_scheduler:
        md["inverse_scheduler"] = DDIMInverseScheduler.from_config(sched.config)
    return md


def _with_checker(md, checker):
    """model_dict entries of the `sd` baseline's safety checker: the HIP checker and the device processor it runs behind."""
    md["safety_checker"], md["safety_processor"] = checker, checker.processor
    return md


def load_synthetic(name="sd14_gligen", seed=0, device="cuda", with_vae=True, load_inverse_scheduler=False,
                   safety_checker=False, scheduler_cls=None, scheduler_config=None):
    """Seeded random weights of the exact architecture (no checkpoints in the sandbox).  The VAE is make_hip_vae's decoder
    with the encoder of the same state dict behind it (built when pipelines.encode first asks for it).  safety_checker:
    True puts a seeded checker of ViT-L/14 geometry with 2 layers (lgd_amd.safety.HipSafetyChecker.synthetic) and its
    processor into model_dict, an instance built with that constructor is taken as it is; False (the default): none.
    scheduler_cls / scheduler_config: as load_sd takes the class (or its name) and reads the checkpoint's config
    (`resolve_scheduler`); without a config the SD 1.x fields apply."""
    from lgd_amd.safety import HipSafetyChecker
    from lgd_amd.vae import make_hip_vae_pair
    if not isinstance(safety_checker, (bool, HipSafetyChecker)):
        raise TypeError("safety_checker: True, False or a lgd_amd.safety.HipSafetyChecker")
    cfg = _weights.CONFIGS[name]
    md = build_model_dict(cfg, _weights.synth_state_dict(cfg, seed), vae=make_hip_vae_pair(device) if with_vae else None,
                          device=device, load_inverse_scheduler=load_inverse_scheduler, scheduler_cls=scheduler_cls,
                          scheduler_config=scheduler_config)
    if safety_checker is False:
        return md
    if safety_checker is True:
        safety_checker = HipSafetyChecker.synthetic(seed=seed, device=device)
    return _with_checker(md, safety_checker)


def load_sd(key="runwayml/stable-diffusion-v1-5", use_fp16=False, load_inverse_scheduler=False,
            use_dpm_multistep_scheduler=False, scheduler_cls=None, vae_ranges=None, safety_checker=False,
            vae_attention=None):
    """models/models.py:16-62.  Needs the Hugging Face checkpoint (diffusers + network/cache); the UNet
    state dict is repacked into the HIP engine's arenas, the CLIP text tower runs on the HIP kernels
    (lgd_amd.clip), the VAE's state dict is repacked for the HIP kernels (lgd_amd.vae.HipVAE: the decoder at once, the
    encoder when pipelines.encode first needs it; LGD_HF_VAE=1 in the environment keeps the Hugging Face module, for A/B
    checks against it).  load_inverse_scheduler (models/models.py:57-59): model_dict.inverse_scheduler for
    pipelines.invert.  vae_ranges: the range plan of a VAE whose config sets force_upcast (the SDXL VAE), by the rule
    of generation.sdxl_refinement._vae_ranges: RangePlan.uniform(8) when none is given, none for an fp16-safe VAE.
    vae_attention: "materialised" | "streamed", the HIP VAE's mid-block attention (None: HipVAE's default).
    safety_checker=True, or LGD_SAFETY_CHECKER=1 in the environment: the checkpoint's `safety_checker` and
    `feature_extractor` subfolders are loaded and model_dict carries `safety_checker` (lgd_amd.safety.HipSafetyChecker)
    and `safety_processor`; generation.stable_diffusion_generate.run then blanks what the checker flags, as the
    reference's pipeline does.  The default runs no checker."""
    if not use_fp16:      # models/models.py:33-38: the reference then loads fp32 weights ("run final results in fp32")
        from generation._common import note_precision
        note_precision("models.load_sd", "use_fp16=False")
    try:
        from diffusers import AutoencoderKL, DDIMScheduler as HFDDIM, UNet2DConditionModel as HFUNet
        from transformers import CLIPTextModel, CLIPTokenizer
    except ImportError as e:
        raise RuntimeError("load_sd needs `diffusers` and HF checkpoints; use load_synthetic() offline") from e
    resolve_scheduler(scheduler_cls, use_dpm_multistep_scheduler)        # refuse before anything is loaded
    hf = HFUNet.from_pretrained(key, subfolder="unet")
    c = hf.config
    heads = c.attention_head_dim if isinstance(c.attention_head_dim, (list, tuple)) else (c.attention_head_dim,) * 4
    sched_cfg = dict(HFDDIM.from_pretrained(key, subfolder="scheduler").config)      # models/models.py:49
    # models/models.py:53 builds `scheduler_cls` from the checkpoint's scheduler_config.json alone: keys the file lacks take
    # THAT class's defaults, not DDIM's (timestep_spacing: "leading" for DDIM, "linspace" for Euler / LMS), so another class
    # gets the file's own fields (unpinned: no checkpoint has been loaded through this branch)
    raw_cfg = sched_cfg
    if scheduler_cls is not None and getattr(scheduler_cls, "__name__", str(scheduler_cls)) != "DDIMScheduler":
        raw_cfg = {k: v for k, v in HFDDIM.load_config(key, subfolder="scheduler").items() if not k.startswith("_")}
    cfg = _weights.UNetConfig(name=key, block_out_channels=tuple(c.block_out_channels), cross_attention_dim=c.cross_attention_dim,
                              attention_head_dim=tuple(heads), use_linear_projection=getattr(c, "use_linear_projection", False),
                              use_gated_attention="gligen" in key, sample_size=c.sample_size,
                              prediction_type=sched_cfg.get("prediction_type", "epsilon"))
    vae = AutoencoderKL.from_pretrained(key, subfolder="vae").to(torch_device)
    tok = CLIPTokenizer.from_pretrained(key, subfolder="tokenizer")
    import os as _os
    from lgd_amd.clip import from_hf as _hip_text_encoder
    te = CLIPTextModel.from_pretrained(key, subfolder="text_encoder")
    if _os.environ.get("LGD_HF_TEXT", "0") == "1":       # keep the Hugging Face tower (A/B against the fp16-compute HIP one)
        te = te.to(torch_device)
    else:
        te = _hip_text_encoder(te, torch_device)         # HIP kernels: fp16 compute, 2-3e-3 of the fp32 tower's states

    class _HFVae:
        config = vae.config

        def decode(self, z):
            return vae.decode(z.to(vae.dtype)).sample

        def encode(self, image):
            return vae.encode(image.to(vae.dtype))
    if _os.environ.get("LGD_HF_VAE", "0") == "1":
        dec = _HFVae()
    else:
        from generation.sdxl_refinement import _vae_ranges
        from lgd_amd.vae import HipVAE, attention_kw
        dec = HipVAE.from_state_dict(vae.state_dict(), torch_device,             # models/models.py:41 on the HIP kernels
                                     scaling_factor=getattr(vae.config, "scaling_factor", 0.18215),
                                     ranges=_vae_ranges(vae.config, vae_ranges, _os.environ), **attention_kw(vae_attention))
    md = build_model_dict(cfg, {k: v.float() for k, v in hf.state_dict().items()}, vae=dec, tokenizer=tok,
                          text_encoder=te, scheduler_config=raw_cfg,
                          use_dpm_multistep_scheduler=use_dpm_multistep_scheduler,
                          load_inverse_scheduler=load_inverse_scheduler, scheduler_cls=scheduler_cls)
    if safety_checker or _os.environ.get("LGD_SAFETY_CHECKER", "0") == "1":
        from diffusers.pipelines.stable_diffusion.safety_checker import StableDiffusionSafetyChecker
        from transformers import CLIPImageProcessor
        from lgd_amd.safety import from_diffusers
        _with_checker(md, from_diffusers(StableDiffusionSafetyChecker.from_pretrained(key, subfolder="safety_checker"),
                                         torch_device,
                                         CLIPImageProcessor.from_pretrained(key, subfolder="feature_extractor")))
    return md


def encode_prompts(tokenizer, text_encoder, prompts, negative_prompt="", return_full_only=False,
                   one_uncond_input_only=False):
    """models/models.py:63-89."""
    if negative_prompt == "":
        print("Note that negative_prompt is an empty string")
    text_input = tokenizer(prompts, padding="max_length", max_length=tokenizer.model_max_length, truncation=True,
                           return_tensors="pt")
    max_length = text_input.input_ids.shape[-1]
    n_unc = 1 if one_uncond_input_only else len(prompts)
    uncond_input = tokenizer([negative_prompt] * n_unc, padding="max_length", max_length=max_length, return_tensors="pt")
    with torch.no_grad():
        uncond_embeddings = text_encoder(uncond_input.input_ids.to(torch_device))[0]
        cond_embeddings = text_encoder(text_input.input_ids.to(torch_device))[0]
    if one_uncond_input_only:
        return uncond_embeddings, cond_embeddings
    text_embeddings = torch.cat([uncond_embeddings, cond_embeddings])
    if return_full_only:
        return text_embeddings
    return text_embeddings, uncond_embeddings, cond_embeddings


def process_input_embeddings(input_embeddings):
    """models/models.py:91-109: 2-tuple (uncond, cond) or 3-tuple (text, uncond, cond)."""
    assert isinstance(input_embeddings, (tuple, list))
    if len(input_embeddings) == 3:
        _, unc, cond = input_embeddings
        assert unc.shape[0] == cond.shape[0], f"{unc.shape[0]} != {cond.shape[0]}"
        return input_embeddings
    if len(input_embeddings) == 2:
        unc, cond = input_embeddings
        if unc.shape[0] == 1:
            unc = unc.expand(cond.shape)
        return torch.cat((unc, cond), dim=0), unc, cond
    raise ValueError(f"input_embeddings length: {len(input_embeddings)}")
