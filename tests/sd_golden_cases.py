"""TEST INFRASTRUCTURE — the cases of tests/golden/run_sd_generate_tiny.npz (tools/make_golden_sd.py) and how their inputs
are drawn, shared by the golden script and the tests.  Start latents and text embeddings are regenerated from their seeds
(the file keeps float64 checksums of both, which the CPU suite compares); every evaluation's input sample is kept as a
fixed, seeded sample of SAMPLE of its elements (the same indices for every evaluation and case), the final latents whole."""
import numpy as np
import torch

# name, UNet config, scheduler, steps, latent seed
CASES = [("tiny_pndm", "tiny", "pndm", 50, 21),
         ("tiny_ddim", "tiny", "ddim", 50, 22),
         ("tiny_sd21_pndm", "tiny_sd21", "pndm", 20, 23)]
TEXT_SEED = 1
SAMPLE = 256
GUIDANCE = 7.5


def case_inputs(cfg, seed):
    """(start latents (1,C,L,L), text (2,77,Cx) = [uncond; cond]) of a case, fp32 on the CPU."""
    from lgd_amd import weights
    L = cfg.sample_size
    lat = torch.randn((1, cfg.in_channels, L, L), generator=torch.Generator().manual_seed(seed))
    unc, cond = weights.synth_embeddings(cfg, 1, seed=TEXT_SEED)
    return lat, torch.cat([unc, cond])


def sample_index(numel):
    """Sorted element indices of the per-evaluation sample (seeded, the same for every run)."""
    return np.sort(np.random.default_rng(0).choice(numel, SAMPLE, replace=False)).astype(np.int32)


def checksum(t):
    t = torch.as_tensor(t).double()
    return np.array([float(t.sum()), float((t * t).sum())])
