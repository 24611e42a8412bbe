"""TEST INFRASTRUCTURE — the cases of tests/golden/run_invert_tiny.npz (tools/make_golden_invert.py) and how their inputs
are drawn, shared by the golden script and the tests.  The clean latents and the text embeddings are regenerated from their
seeds (the file keeps float64 checksums of both); every row of the inverted stack is kept as a fixed, seeded sample of
SAMPLE of its elements (sd_golden_cases.sample_index: the same indices for every row and case), the noisiest row whole.
The chain case adds the reference's own generate_partial_frozen on the scale-0 case's inverted stack."""
import torch

from sd_golden_cases import SAMPLE, TEXT_SEED, checksum, sample_index  # noqa: F401  (shared with the sd golden)

# name, UNet config, steps, guidance scale, latent seed
CASES = [("tiny_g7.5", "tiny", 10, 7.5, 31),
         ("tiny_g0", "tiny", 10, 0.0, 32),
         ("tiny_sd21_g1", "tiny_sd21", 10, 1.0, 33)]
CHAIN_CASE = "tiny_g0"            # generate_partial_frozen on this case's stack (inverted without guidance, generated with)
CHAIN_FROZEN_STEPS = 4
CHAIN_GUIDANCE = 7.5
CHAIN_BOX = (8, 24, 4, 20)        # rows y0:y1, columns x0:x1 of the latent grid that stay frozen


def case_inputs(cfg, seed):
    """(clean latents (1,C,L,L) — 0.8 * N(0, 1), about the spread of scaled SD latents —, text (2,77,Cx) = [uncond; cond]),
    fp32 on the CPU."""
    from lgd_amd import weights
    L = cfg.sample_size
    lat = 0.8 * torch.randn((1, cfg.in_channels, L, L), generator=torch.Generator().manual_seed(seed))
    unc, cond = weights.synth_embeddings(cfg, 1, seed=TEXT_SEED)
    return lat, torch.cat([unc, cond])


def chain_mask(L):
    y0, y1, x0, x1 = CHAIN_BOX
    m = torch.zeros((L, L))
    m[y0:y1, x0:x1] = 1.0
    return m
