"""The image degradation of visual contrastive decoding (Leng et al., CVPR 2024, section 3.2): the forward diffusion process applied to the
preprocessed image, whose result is what generate(images_cd=...) decodes the contrast row from.  Plain torch, off the hot path; callers may
hand generate any images_cd instead."""
import torch

NOISE_STEPS = 1000


def _alphas_cumprod(device):
    """abar_t, t < 1000, of the sigmoid beta schedule from 1e-5 to 5e-3: beta_t = sigmoid(linspace(-6, 6, 1000)) * (5e-3 - 1e-5) + 1e-5."""
    betas = torch.sigmoid(torch.linspace(-6, 6, NOISE_STEPS, dtype=torch.float32, device=device)) * (5e-3 - 1e-5) + 1e-5
    return torch.cumprod(1.0 - betas, 0)


def add_diffusion_noise(images, noise_step, generator=None):
    """q(x_t | x_0) at t = noise_step in [0, 1000): sqrt(abar_t) * images + sqrt(1 - abar_t) * eps, eps ~ N(0, I) drawn in fp32 from
    `generator` (on the images' device; None = the default one) -> a tensor of the images' shape and dtype.  Step 0 is the image up to
    noise of standard deviation 3e-3; step 999 is close to pure noise."""
    t = int(noise_step)
    if not 0 <= t < NOISE_STEPS:
        raise ValueError("add_diffusion_noise: noise_step=%r (needs an int in [0, %d))" % (noise_step, NOISE_STEPS))
    abar = _alphas_cumprod(images.device)[t]
    eps = torch.randn(images.shape, dtype=torch.float32, device=images.device, generator=generator)
    return (abar.sqrt() * images.float() + (1.0 - abar).sqrt() * eps).to(images.dtype)
