"""TEST INFRASTRUCTURE — the cases of tests/golden/run_multidiffusion_tiny.npz (tools/make_golden_multidiffusion.py) and
the CPU stand-in VAE both sides use.  The reference's own generation/multidiffusion.py runs with the `tiny` UNet, the
tests/fake_text.py text side and this VAE; the tests regenerate every input from the recorded seeds.

The stand-in VAE: encoder = 8x8 average pooling and a seeded 1x1 convolution to (mean, logvar) (logvar clamped to
[-30, 20] as DiagonalGaussianDistribution does), decoder = oracle/restate_vae.VAEDecoder at small width with seeded
parameters.  Only the call surface matters here: the reference draws through `vae.encode(x).latent_dist.sample()`
and decodes through `vae.decode(z).sample`."""
import numpy as np
import torch

SEED_BASE = 70
SAMPLE = 256
UNET = "tiny"

# name, boxes, bg prompt, steps, bootstrapping, first_top, extra negative prompt, seed
CASES = [
    ("none", [], "a quiet meadow", 12, 5, False, "", 71),
    ("two", [("a red apple", [40, 60, 150, 160]), ("a blue cup", [300, 200, 140, 180])], "a kitchen table", 50, 20,
     False, "", 72),
    ("three_back", [("a cat", [50, 100, 250, 250]), ("a dog", [200, 150, 250, 250]), ("a ball", [150, 50, 200, 200])],
     "a garden", 12, 5, False, "dark", 73),
    ("three_top", [("a cat", [50, 100, 250, 250]), ("a dog", [200, 150, 250, 250]), ("a ball", [150, 50, 200, 200])],
     "a garden", 12, 5, True, "", 73),
    ("oob", [("a boat.", [-40, 300, 300, 260])], "a lake", 12, 5, False, "", 74),
]
TF_CASE, TF_STEPS = "two", (19, 20)      # teacher-forced steps: whole latents before these are kept
GUIDANCE = 10.0


class _Posterior:
    def __init__(self, mean, logvar):
        self.mean, self.logvar = mean, logvar
        self.std = torch.exp(0.5 * logvar)

    def sample(self, generator=None):
        """DiagonalGaussianDistribution.sample ([ext] diffusers 0.18.0): mean + std * randn on the moments' device."""
        e = torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)
        return self.mean + self.std * e


class _Out:
    def __init__(self, **k):
        self.__dict__.update(k)


class StandInVAE:
    def __init__(self, seed=5):
        import restate_vae
        g = torch.Generator().manual_seed(seed)
        self.w = torch.randn(8, 3, generator=g) * 0.5
        self.b = torch.randn(8, generator=g) * 0.1
        with torch.random.fork_rng():
            torch.manual_seed(seed)
            self.dec = restate_vae.VAEDecoder(ch=(32, 32, 32, 32), layers=1).eval()

    def to(self, *a, **k):
        return self

    @torch.no_grad()
    def encode_moments(self, image):
        x = torch.nn.functional.avg_pool2d(image.float(), 8)
        m = torch.einsum("oc,bchw->bohw", self.w, x) + self.b[None, :, None, None]
        mean, logvar = m.chunk(2, dim=1)
        return mean.contiguous(), logvar.clamp(-30.0, 20.0).contiguous()

    def encode(self, image):
        return _Out(latent_dist=_Posterior(*self.encode_moments(image)))

    @torch.no_grad()
    def decode(self, z):
        return _Out(sample=self.dec.decode(z.float()))


def sample_index(numel, n=SAMPLE, seed=0):
    return np.sort(np.random.default_rng(seed).choice(numel, n, replace=False)).astype(np.int64)


def checksum(t):
    t = torch.as_tensor(t).double()
    return np.array([float(t.sum()), float((t * t).sum())])
