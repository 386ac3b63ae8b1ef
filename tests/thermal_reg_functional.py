"""A torch restatement of the splat model's thermal regularisers, the reference the GPU tests hold tn_thermal_reg to: ThermalNeRF's tv_pixel_loss
and cross_channel_loss (model_components/losses.py:602-651) applied to the batch of all (H-1) x (W-1) overlapping 2 x 2 windows of one frame --
stride 1, row-major, each window flattened as (top-left, top-right, bottom-left, bottom-right).  Works in any dtype (the tests use float64) and
differentiates through plain autograd (torch.abs: sign(0) = 0).  Images are [H,W,C] (the model's layout)."""
import torch
import torch.nn.functional as F

# the four terms of a window: (earlier pixel, later pixel) as (row, column) offsets inside it, in the reference's order
TERMS = (((0, 0), (0, 1)), ((0, 0), (1, 0)), ((0, 1), (1, 1)), ((1, 0), (1, 1)))


def windows(img: torch.Tensor) -> torch.Tensor:
    """[H,W] -> [(H-1)(W-1), 4]: every 2 x 2 window, row-major, flattened (top-left, top-right, bottom-left, bottom-right)."""
    return torch.stack([img[:-1, :-1], img[:-1, 1:], img[1:, :-1], img[1:, 1:]], dim=-1).reshape(-1, 4)


def grey(gt_rgb: torch.Tensor) -> torch.Tensor:
    return gt_rgb.mean(-1)


def tv(pred_thermal: torch.Tensor) -> torch.Tensor:
    p = windows(pred_thermal[..., 0])
    return 0.25 * torch.mean((p[:, 0] - p[:, 1]).abs() + (p[:, 0] - p[:, 2]).abs() + (p[:, 1] - p[:, 3]).abs() + (p[:, 2] - p[:, 3]).abs())


def _pixel_grad(p: torch.Tensor) -> torch.Tensor:
    return torch.stack((p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 3] - p[:, 1], p[:, 3] - p[:, 2]))


def cross(pred_thermal: torch.Tensor, gt_rgb: torch.Tensor) -> torch.Tensor:
    diff = (_pixel_grad(windows(pred_thermal[..., 0])) - _pixel_grad(windows(grey(gt_rgb)))).abs()
    return 0.25 * (diff[0] + diff[1] + diff[2] + diff[3]).mean()


def regularizers(pred_thermal: torch.Tensor, gt_rgb: torch.Tensor, tv_mult: float, cross_mult: float):
    """(tv_mult * tv, cross_mult * cc); a multiplier of 0 gives an exact 0 that does not depend on the inputs."""
    zero = torch.zeros((), dtype=pred_thermal.dtype, device=pred_thermal.device)
    return (tv_mult * tv(pred_thermal) if tv_mult else zero), (cross_mult * cross(pred_thermal, gt_rgb) if cross_mult else zero)


def near_ties(pred_thermal: torch.Tensor, gt_rgb: torch.Tensor, tv_mult: float, cross_mult: float, eps: float = 1e-5):
    """Where a sign decided in fp32 may differ from this dtype's: (mask [H,W] of the pixels one of whose live terms has an |argument| below eps,
    share of such terms among all live window terms)."""
    t, q = pred_thermal[..., 0], grey(gt_rgb)
    H, W = t.shape
    mask = torch.zeros((H, W), dtype=torch.bool, device=t.device)
    near_terms, terms = 0, 0
    for (ay, ax), (by, bx) in TERMS:
        a = lambda m, y=ay, x=ax: m[y:y + H - 1, x:x + W - 1]  # noqa: E731
        b = lambda m, y=by, x=bx: m[y:y + H - 1, x:x + W - 1]  # noqa: E731
        args = ([a(t) - b(t)] if tv_mult else []) + ([(b(t) - a(t)) - (b(q) - a(q))] if cross_mult else [])
        for arg in args:
            near = arg.abs() < eps
            a(mask).logical_or_(near)
            b(mask).logical_or_(near)
            near_terms += int(near.sum())
            terms += near.numel()
    return mask, near_terms / max(terms, 1)


def random_pair(h: int, w: int, seed: int = 0, dtype=torch.float64):
    """A thermal prediction [H,W,1] and an RGB ground truth [H,W,3], independent and uniform in [0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    pred = torch.rand((h, w, 1), generator=gen, dtype=torch.float64)
    gt = torch.rand((h, w, 3), generator=gen, dtype=torch.float64)
    return pred.to(dtype), gt.to(dtype)


def smooth_pair(h: int, w: int, seed: int = 0, dtype=torch.float64):
    """random_pair smoothed with a 9 x 9 box (replicated borders): neighbouring pixels differ by ~1e-2, like a render's, and not by ~0.3."""
    pred, gt = random_pair(h, w, seed)

    def box(img):
        x = F.pad(img.permute(2, 0, 1)[None], (4, 4, 4, 4), mode="replicate")
        return F.avg_pool2d(x, 9, stride=1)[0].permute(1, 2, 0).contiguous()

    return box(pred).to(dtype), box(gt).to(dtype)
