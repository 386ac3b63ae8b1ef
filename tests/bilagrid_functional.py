"""The bilateral grid (nerfstudio_thermal_amd.splat_image.bilateral_slice / bilateral_grid_tv) restated in plain torch, in whatever dtype its inputs
have: the definition the HIP kernels are held to.  gsplat's Python source is not part of this tree, so the restatement follows the published
operation: a frame's grid G [K, L, GH, GW], K = C (C + 1), of affine colour transforms is sampled at (x, y, guidance) by
F.grid_sample(mode="bilinear", padding_mode="border", align_corners=True) and applied as out = A pixel + b."""
import torch
import torch.nn.functional as F

LUMA = (0.299, 0.587, 0.114)


def guidance(image: torch.Tensor) -> torch.Tensor:
    """[H,W]: 0.299 r + 0.587 g + 0.114 b of an [H,W,3] image, channel 0 of an [H,W,1] one."""
    if image.shape[2] == 1:
        return image[..., 0]
    return (LUMA[0] * image[..., 0] + LUMA[1] * image[..., 1]) + LUMA[2] * image[..., 2]


def slice(grid: torch.Tensor, image: torch.Tensor) -> torch.Tensor:  # noqa: A001
    """grid [K,L,GH,GW] applied to image [H,W,C] -> [H,W,C]; differentiable in both."""
    H, W, C = image.shape
    assert grid.shape[0] == C * (C + 1), (tuple(grid.shape), C)
    x = ((torch.arange(W, dtype=image.dtype, device=image.device) + 0.5) / W).expand(H, W)
    y = ((torch.arange(H, dtype=image.dtype, device=image.device) + 0.5) / H).reshape(H, 1).expand(H, W)
    coords = torch.stack([x, y, guidance(image)], dim=-1) * 2 - 1  # grid_sample's (x, y, z) order: GW, GH, L
    coef = F.grid_sample(grid[None], coords[None, None], mode="bilinear", padding_mode="border", align_corners=True)  # [1,K,1,H,W]
    coef = coef[0, :, 0].permute(1, 2, 0).reshape(H, W, C, C + 1)
    return (coef[..., :C] * image[..., None, :]).sum(-1) + coef[..., C]


def tv(grids: torch.Tensor) -> torch.Tensor:
    """Total variation of grids [F,K,L,GH,GW]: per grid axis the sum of squared first differences over the entries of ONE frame's difference
    tensor; the three terms added and divided by F."""
    n_frames = grids.shape[0]
    total = 0
    for dim in (2, 3, 4):
        d = grids.narrow(dim, 1, grids.shape[dim] - 1) - grids.narrow(dim, 0, grids.shape[dim] - 1)
        total = total + (d * d).sum() / d[0].numel()
    return total / n_frames


def identity_grids(num_frames: int, channels: int, grid_shape, dtype=torch.float32) -> torch.Tensor:
    """[F, C (C + 1), L, GH, GW] with grid_shape = (GW, GH, L): the matrix's diagonal (the gain) 1, the rest 0."""
    GW, GH, L = grid_shape
    eye = torch.eye(channels, channels + 1, dtype=dtype).reshape(1, channels * (channels + 1), 1, 1, 1)
    return eye.repeat(num_frames, 1, L, GH, GW).contiguous()


def constant_grids(num_frames: int, affine: torch.Tensor, grid_shape) -> torch.Tensor:
    """Every vertex holds the same [A | b] (a [C, C + 1] tensor)."""
    GW, GH, L = grid_shape
    return affine.reshape(1, -1, 1, 1, 1).repeat(num_frames, 1, L, GH, GW).contiguous()


def random_image(H: int, W: int, C: int, seed: int) -> torch.Tensor:
    """[H,W,C] float32, uniform in [0.02, 0.98]: no pixel on the brightness clamp."""
    g = torch.Generator().manual_seed(seed)
    return 0.02 + 0.96 * torch.rand((H, W, C), generator=g)


def random_grids(num_frames: int, channels: int, grid_shape, seed: int, spread: float = 0.3) -> torch.Tensor:
    """The identity plus uniform noise in [-spread, spread] on every entry, float32."""
    g = torch.Generator().manual_seed(seed)
    base = identity_grids(num_frames, channels, grid_shape)
    return base + spread * (2 * torch.rand(base.shape, generator=g) - 1)


def random_upstream(H: int, W: int, C: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn((H, W, C), generator=g)


def near_planes(image: torch.Tensor, L: int, tol: float = 1e-4) -> torch.Tensor:
    """[H,W] bool: pixels whose brightness coordinate g (L - 1) lies within `tol` of an integer -- a plane of the grid, where the image gradient's
    guidance path jumps and two precisions may take different sides."""
    z = guidance(image.double()) * (L - 1)
    return (z - z.round()).abs() <= tol
