"""A torch restatement of the splat training loss (splatfacto.py:848-903 with pytorch_msssim's SSIM, v1.x `ssim` / `_ssim` / `gaussian_filter`),
the reference the GPU tests hold tn_image_loss to.  Works in any dtype (the tests use float64) and differentiates through plain autograd.

SSIM: an 11-tap Gaussian window with sigma 1.5 (normalised in fp32, as pytorch_msssim builds it), applied separably as a VALID correlation with
groups = C; C1 = 0.01^2, C2 = 0.03^2 (data range 1); the map is averaged over the valid pixels and then the channels (nonnegative_ssim off).
Images are [H,W,C] (the model's layout)."""
import torch
import torch.nn.functional as F

WIN_SIZE = 11
WIN_SIGMA = 1.5
C1 = 0.01 ** 2
C2 = 0.03 ** 2


def gauss_window(dtype=torch.float64, device="cpu") -> torch.Tensor:
    """pytorch_msssim's _fspecial_gauss_1d: built in fp32, then cast."""
    coords = torch.arange(WIN_SIZE, dtype=torch.float32) - WIN_SIZE // 2
    g = torch.exp(-(coords ** 2) / (2 * WIN_SIGMA ** 2))
    g /= g.sum()
    return g.to(dtype=dtype, device=device)


def gaussian_filter(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """[1,C,H,W] -> [1,C,H-10,W-10]: the window along H, then along W, as valid grouped correlations."""
    c = x.shape[1]
    out = F.conv2d(x, g.view(1, 1, -1, 1).repeat(c, 1, 1, 1), groups=c)
    return F.conv2d(out, g.view(1, 1, 1, -1).repeat(c, 1, 1, 1), groups=c)


def ssim(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """SSIM of two [H,W,C] images (mean over valid pixels and channels)."""
    x = pred.permute(2, 0, 1)[None]
    y = gt.permute(2, 0, 1)[None]
    g = gauss_window(x.dtype, x.device)
    mu_x, mu_y = gaussian_filter(x, g), gaussian_filter(y, g)
    s_xx = gaussian_filter(x * x, g) - mu_x * mu_x
    s_yy = gaussian_filter(y * y, g) - mu_y * mu_y
    s_xy = gaussian_filter(x * y, g) - mu_x * mu_y
    cs = (2 * s_xy + C2) / (s_xx + s_yy + C2)
    lum = (2 * mu_x * mu_y + C1) / (mu_x * mu_x + mu_y * mu_y + C1)
    return (lum * cs).flatten(2).mean(-1).mean()


def l1(pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    return (pred - gt).abs().mean()


def main_loss(pred: torch.Tensor, gt: torch.Tensor, ssim_lambda: float = 0.2, weight: float = 1.0) -> torch.Tensor:
    """weight * ((1 - ssim_lambda) * L1 + ssim_lambda * (1 - SSIM))"""
    return weight * ((1 - ssim_lambda) * l1(pred, gt) + ssim_lambda * (1 - ssim(pred, gt)))


def correlated_pair(h: int, w: int, c: int, seed: int = 0, dtype=torch.float64):
    """Two images in [0, 1] that share a smooth structure (a ground truth and a noisy, biased prediction of it), [H,W,C]."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.rand((1, c, h // 4 + 2, w // 4 + 2), generator=gen, dtype=torch.float64)
    base = F.interpolate(base, size=(h, w), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    gt = (base + 0.1 * torch.rand((h, w, c), generator=gen, dtype=torch.float64)).clamp(0, 1)
    pred = (0.8 * gt + 0.1 + 0.15 * torch.randn((h, w, c), generator=gen, dtype=torch.float64)).clamp(0, 1)
    return pred.to(dtype), gt.to(dtype)
