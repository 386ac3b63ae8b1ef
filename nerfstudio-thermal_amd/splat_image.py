"""The image kernels of the splat path (splat.py), each one HIP call on the current stream without a host synchronisation.  The objective is
splatfacto's (splatfacto.py:848-903): (1 - ssim_lambda) * L1 + ssim_lambda * (1 - SSIM) of the frame's spectrum in one fused HIP call (`image_loss`:
tn_image_loss, the loss and d loss / d prediction, no host synchronisation), with pytorch_msssim's SSIM.  Under the resolution schedule the ground
truth -- uint8 or float -- is shrunk by one HIP bilinear resize with torchvision's resize(antialias=None) semantics (`resize_image`: tn_image_resize).
ThermalNeRF's two cross-spectrum regularisers (model_components/losses.py:602-651, used at models/thermal_nerfacto.py:346-354) are there for RGB
frames: `tv_pixel_loss` -- the 2 x 2-patch total variation of the thermal render at the RGB camera -- and `cross_channel_loss` -- that render's pixel
differences against those of the RGB ground truth's grey value -- over every stride-1 window of the frame, in one fused HIP call
(`thermal_regularizers`: tn_thermal_reg), so the thermal channel gets a gradient from RGB frames too.  Two geometric priors act on the depth render
where it is covered (`depth_losses`: tn_depth_loss): the L1 distance to a sensor depth and the 2 x 2 total variation of the depth.  Distorted frames are resampled once into
pinhole frames: `undistort_image` is the frame `splat_camera.undistorted_camera` sees (tn_image_undistort, uint8 or fp32 in and out);
splat_datamanager.ThermalFullImageDatamanager caches the undistorted frames on the device and serves (camera, batch).  Per-frame colour correction
is gsplat's bilateral grid: `bilateral_slice` applies one frame's grid of affine colour transforms to a training render (tn_bilagrid_slice, its
backward a gather without atomics) and `bilateral_grid_tv` is the grids' total-variation regulariser (tn_bilagrid_tv).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib, splat_calls
from .splat_camera import PinholeCamera, _coefficients, undistorted_camera


class _ImageLoss(torch.autograd.Function):
    """tn_image_loss as an autograd node: forward computes [weight * main loss, L1, SSIM] and d main / d pred in one call; backward scales that
    gradient.  Only entry 0 of the output is differentiable (image_loss hands out the other two detached)."""

    @staticmethod
    def forward(ctx, pred, gt, ssim_lambda, weight):
        out, grad = _image_loss_call(pred, gt, ssim_lambda, weight, True)
        ctx.save_for_backward(grad)
        return out

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g[0], None, None, None


def _image_view(t: Tensor, name: str, dtypes=(torch.float32,), kind: str = "an fp32") -> Tuple[Tensor, int]:
    """An [H,W,C] HIP image (fp32 unless `dtypes` / `kind` say otherwise) as (tensor, pixel stride): pixels may be further apart than C (a view into an
    [H,W,4] buffer), rows must follow pixels and channels must be adjacent; anything else is made contiguous."""
    if not isinstance(t, Tensor) or not t.is_cuda or t.dtype not in dtypes:
        raise ValueError(f"{name} must be {kind} HIP tensor (the splat path has no CPU fallback)")
    if t.dim() != 3:
        raise ValueError(f"{name} must be [H, W, C], got {tuple(t.shape)}")
    H, W, Cc = t.shape
    if not (t.stride(2) == 1 or Cc == 1) or t.stride(1) < Cc or t.stride(0) != W * t.stride(1):
        t = t.contiguous()
    return t, t.stride(1)


def _image_loss_call(pred: Tensor, gt: Tensor, ssim_lambda: float, weight: float, want_grad: bool) -> Tuple[Tensor, Optional[Tensor]]:
    if pred.shape != gt.shape:
        raise ValueError(f"prediction {tuple(pred.shape)} and ground truth {tuple(gt.shape)} differ")
    pred, ps = _image_view(pred.detach(), "prediction")
    gt, gs = _image_view(gt.detach(), "ground truth")
    H, W, Cc = pred.shape
    if H < 11 or W < 11:
        raise ValueError(f"the SSIM loss needs images of at least 11 x 11 pixels (its window), got {H} x {W}")
    if not 1 <= Cc <= 4:
        raise ValueError(f"the SSIM loss takes 1..4 channels, got {Cc}")
    dev = pred.device
    out = torch.empty(3, device=dev)
    grad = torch.empty((H, W, Cc), device=dev) if want_grad else None
    splat_calls.image_loss_call(pred, ps, gt, gs, H, W, Cc, ssim_lambda, weight, out, grad)
    return out, grad


def image_loss(pred: Tensor, gt: Tensor, ssim_lambda: float = 0.2, weight: float = 1.0) -> Tuple[Tensor, Tensor, Tensor]:
    """splatfacto's training loss of one [H,W,C] frame (C = 1..4, H and W >= 11) on the device, without a host synchronisation:
    (weight * ((1 - ssim_lambda) * L1 + ssim_lambda * (1 - SSIM)), L1, SSIM).  SSIM is pytorch_msssim's (11-tap Gaussian window, sigma 1.5, valid
    filtering, data range 1); gt gets no gradient.  The first entry is differentiable in pred when gradients are on."""
    if torch.is_grad_enabled() and pred.requires_grad:
        out = _ImageLoss.apply(pred, gt, ssim_lambda, weight)
        return out[0], out[1].detach(), out[2].detach()
    out, _ = _image_loss_call(pred, gt, ssim_lambda, weight, False)
    return out[0], out[1], out[2]


MAX_IMAGE_SIDE = 1 << 15  # tn_image_resize's (and tn_image_undistort's, tn_image_loss's, tn_thermal_reg's) largest side


def resize_image(image: Tensor, size: Tuple[int, int]) -> Tensor:
    """torchvision.transforms.functional.resize(image, size, antialias=None) of one [H,W,C] image (C = 1..4) to [h,w,C] fp32 -- that is
    torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=False), what splatfacto's _downscale_if_required does
    (splatfacto.py:648-657) -- in one tn_image_resize call on the current stream, without a host synchronisation.  image: uint8 or fp32 on the
    device; a uint8 value v enters as float(v) / 255.0f (get_gt_img's conversion, fused: the bits of resizing image.float() / 255).  A view whose
    pixels are further apart than C (rgbt[..., :3]) is read in place.  No gradient."""
    image, ps = _image_view(image, "image", (torch.uint8, torch.float32), "a uint8 or fp32")
    image = image.detach()
    H, W, Cc = image.shape
    if len(size) != 2:
        raise ValueError(f"resize_image: size must be (h, w), got {tuple(size)}")
    h, w = int(size[0]), int(size[1])
    if not 1 <= Cc <= 4:
        raise ValueError(f"resize_image takes 1..4 channels, got {Cc}")
    if not all(1 <= v <= MAX_IMAGE_SIDE for v in (H, W, h, w)):
        raise ValueError(f"resize_image: {H} x {W} -> {h} x {w}, every side must be in 1..{MAX_IMAGE_SIDE}")
    out = torch.empty((h, w, Cc), device=image.device)
    splat_calls.image_resize(image, ps, out)
    return out


def undistort_image(image: Tensor, camera: PinholeCamera, distortion, new_camera: Optional[PinholeCamera] = None,
                    out_dtype: Optional[torch.dtype] = None) -> Tuple[Tensor, PinholeCamera]:
    """One frame of `camera` with `distortion` (k1, k2, k3, k4, p1, p2) resampled into the pinhole frame of `new_camera` (default:
    `undistorted_camera(camera, distortion)`, whose docstring has the model and the pixel convention) -> (image', camera'), in one
    tn_image_undistort call on the current stream, without a host synchronisation.  image: [H,W,C] uint8 or fp32 on the device, C = 1..4; a view
    whose pixels are further apart than C (rgbt[..., :3]) is read in place; a uint8 value v enters as float(v) / 255.0f.  image': contiguous
    [H,W,C] of `out_dtype` (torch.uint8 or torch.float32, default the input's); a uint8 output is rint(255 clamp(value, 0, 1)), so a uint8 cache
    stays uint8.  Each output pixel is the bilinear interpolation of the source at the distorted position of its viewing direction (taps clamped
    to the frame).  With all six coefficients zero the input tensor and camera come back themselves and nothing is launched.  No gradient.
    ValueError when the image's size and the camera's width / height disagree."""
    k = _coefficients(distortion)
    image, ps = _image_view(image, "image", (torch.uint8, torch.float32), "a uint8 or fp32")
    H, W, Cc = image.shape
    if (H, W) != (int(camera.height), int(camera.width)):
        raise ValueError(f"undistort_image: the image is {H} x {W}, the camera {camera.height} x {camera.width}")
    out_dtype = image.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"undistort_image: out_dtype {out_dtype} (torch.uint8 or torch.float32)")
    if not any(k):
        return image, camera
    if not 1 <= Cc <= 4:
        raise ValueError(f"undistort_image takes 1..4 channels, got {Cc}")
    if not all(1 <= v <= MAX_IMAGE_SIDE for v in (H, W)):
        raise ValueError(f"undistort_image: {H} x {W}, every side must be in 1..{MAX_IMAGE_SIDE}")
    new_camera = undistorted_camera(camera, k) if new_camera is None else new_camera
    if (int(new_camera.height), int(new_camera.width)) != (H, W):
        raise ValueError(f"undistort_image: the new camera is {new_camera.height} x {new_camera.width}, the image {H} x {W}")
    image = image.detach()
    p = _lib.TnUndistort()
    p.fx, p.fy, p.cx, p.cy = float(camera.fx), float(camera.fy), float(camera.cx), float(camera.cy)
    p.new_fx, p.new_fy, p.new_cx, p.new_cy = float(new_camera.fx), float(new_camera.fy), float(new_camera.cx), float(new_camera.cy)
    for i, v in enumerate(k):
        p.k[i] = v
    out = torch.empty((H, W, Cc), dtype=out_dtype, device=image.device)
    splat_calls.image_undistort(image, ps, out, p)
    return out, new_camera


class _ThermalRegularizers(torch.autograd.Function):
    """tn_thermal_reg as an autograd node: forward computes (tv_mult * tv, cross_mult * cc) and the gradient of their sum in one call and saves it;
    backward scales it.  Summed with one upstream gradient -- a loss dict's sum -- that is all.  Upstream gradients that differ between the two
    outputs (or reach only one of them while both terms are on) need each term's own gradient: one more call per term, with the other's multiplier 0."""

    @staticmethod
    def forward(ctx, pred, gt, tv_mult, cross_mult):
        out, grad = _thermal_reg_call(pred, gt, tv_mult, cross_mult, True)
        ctx.save_for_backward(grad, pred, gt)
        ctx.mults = (tv_mult, cross_mult)
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_tv, g_cc):
        grad, pred, gt = ctx.saved_tensors
        tv_mult, cross_mult = ctx.mults
        if tv_mult == 0 or cross_mult == 0:  # the saved gradient is the one live term's
            g = g_cc if tv_mult == 0 else g_tv
            return (None if g is None else grad * g), None, None, None
        if g_tv is not None and g_cc is not None and g_tv.shape == g_cc.shape and g_tv.data_ptr() == g_cc.data_ptr():  # one upstream gradient
            return grad * g_tv, None, None, None
        total = None
        for g, mults in ((g_tv, (tv_mult, 0.0)), (g_cc, (0.0, cross_mult))):
            if g is not None:
                term = _thermal_reg_call(pred, gt, *mults, True)[1] * g
                total = term if total is None else total + term
        return total, None, None, None


def _thermal_reg_call(pred: Tensor, gt: Tensor, tv_mult: float, cross_mult: float, want_grad: bool) -> Tuple[Tensor, Optional[Tensor]]:
    if pred.dim() != 3 or gt.dim() != 3 or pred.shape[2] != 1 or gt.shape[2] != 3 or pred.shape[:2] != gt.shape[:2]:
        raise ValueError(f"thermal_regularizers takes a thermal prediction [H,W,1] and an RGB ground truth [H,W,3] of one size, got "
                         f"{tuple(pred.shape)} and {tuple(gt.shape)}")
    if tv_mult < 0 or cross_mult < 0:
        raise ValueError(f"thermal_regularizers: multipliers {tv_mult} / {cross_mult}, a loss multiplier cannot be negative")
    pred, ps = _image_view(pred.detach(), "thermal prediction")
    gt, gs = _image_view(gt.detach(), "RGB ground truth")
    H, W, _ = pred.shape
    if not all(2 <= v <= MAX_IMAGE_SIDE for v in (H, W)):
        raise ValueError(f"thermal_regularizers: {H} x {W}, every side must be in 2..{MAX_IMAGE_SIDE} (the windows are 2 x 2)")
    dev = pred.device
    out = torch.empty(2, device=dev)
    grad = torch.empty((H, W, 1), device=dev) if want_grad else None
    splat_calls.thermal_reg(pred, ps, gt, gs, H, W, tv_mult, cross_mult, out, grad)
    return out, grad


def thermal_regularizers(pred_thermal: Tensor, gt_rgb: Tensor, tv_mult: float, cross_mult: float) -> Tuple[Tensor, Tensor]:
    """ThermalNeRF's regularisers of a thermal render [H,W,1] at an RGB camera with ground truth [H,W,3] (H and W >= 2), on the device and without a
    host synchronisation: (tv_mult * tv_pixel_loss, cross_mult * cross_channel_loss) of model_components/losses.py:602-651, applied to all
    (H-1) x (W-1) stride-1 2 x 2 windows of the frame -- the total variation of the prediction, and its pixel differences against those of the mean
    over gt_rgb's channels.  A multiplier of 0 gives exactly 0 and skips that term.  Views whose pixels are further apart (rgbt[..., 3:],
    image[..., :3] of an [H,W,4] image) are read in place.  Both entries are differentiable in pred_thermal when gradients are on (sign(0) = 0, as
    torch.abs has it); gt_rgb gets no gradient."""
    if torch.is_grad_enabled() and isinstance(pred_thermal, Tensor) and pred_thermal.requires_grad:
        return _ThermalRegularizers.apply(pred_thermal, gt_rgb, float(tv_mult), float(cross_mult))
    out, _ = _thermal_reg_call(pred_thermal, gt_rgb, tv_mult, cross_mult, False)
    return out[0], out[1]


class _DepthLosses(torch.autograd.Function):
    """tn_depth_loss as an autograd node, built as _ThermalRegularizers is: forward computes (depth_mult * depth_loss, tv_mult * depth_tv_loss) and
    the gradient of their sum in depth in one call and saves it; backward scales it, or -- for upstream gradients that differ between the two
    outputs -- asks for each term's own gradient with the other's multiplier 0.  Accumulation and sensor depth get no gradient."""

    @staticmethod
    def forward(ctx, depth, accumulation, depth_image, depth_mult, tv_mult):
        out, grad = _depth_loss_call(depth, accumulation, depth_image, depth_mult, tv_mult, True)
        ctx.save_for_backward(grad, depth, accumulation, *([depth_image] if depth_image is not None else []))
        ctx.mults = (depth_mult, tv_mult)
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_d, g_tv):
        grad, depth, accumulation, *sensor = ctx.saved_tensors
        sensor = sensor[0] if sensor else None
        depth_mult, tv_mult = ctx.mults
        if depth_mult == 0 or tv_mult == 0 or sensor is None:  # the saved gradient is the one live term's
            g = g_tv if (depth_mult == 0 or sensor is None) else g_d
            return (None if g is None else grad * g), None, None, None, None
        if g_d is not None and g_tv is not None and g_d.shape == g_tv.shape and g_d.data_ptr() == g_tv.data_ptr():  # one upstream gradient
            return grad * g_d, None, None, None, None
        total = None
        for g, mults in ((g_d, (depth_mult, 0.0)), (g_tv, (0.0, tv_mult))):
            if g is not None:
                term = _depth_loss_call(depth, accumulation, sensor, *mults, True)[1] * g
                total = term if total is None else total + term
        return total, None, None, None, None


def _depth_loss_call(depth: Tensor, accumulation: Tensor, depth_image: Optional[Tensor], depth_mult: float, tv_mult: float,
                     want_grad: bool) -> Tuple[Tensor, Optional[Tensor]]:
    maps = [("depth", depth), ("accumulation", accumulation)] + ([("depth_image", depth_image)] if depth_image is not None else [])
    for name, t in maps:
        if not isinstance(t, Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise ValueError(f"depth_losses: {name} must be an fp32 HIP tensor (the splat path has no CPU fallback)")
        if t.dim() != 3 or t.shape[2] != 1 or t.shape != depth.shape:
            raise ValueError(f"depth_losses takes depth, accumulation and depth_image [H,W,1] of one size, got {name} {tuple(t.shape)} for depth {tuple(depth.shape)}")
    if depth_mult < 0 or tv_mult < 0:
        raise ValueError(f"depth_losses: multipliers {depth_mult} / {tv_mult}, a loss multiplier cannot be negative")
    H, W, _ = depth.shape
    if not all(2 <= v <= MAX_IMAGE_SIDE for v in (H, W)):
        raise ValueError(f"depth_losses: {H} x {W}, every side must be in 2..{MAX_IMAGE_SIDE} (the windows are 2 x 2)")
    dev = depth.device
    out = torch.empty(2, device=dev)
    grad = torch.empty((H, W, 1), device=dev) if want_grad else None
    splat_calls.depth_loss(depth.detach().contiguous(), accumulation.detach().contiguous(), None if depth_image is None else depth_image.detach().contiguous(),
                           H, W, depth_mult, tv_mult, out, grad)
    return out, grad


def depth_losses(depth: Tensor, accumulation: Tensor, depth_image: Optional[Tensor], depth_mult: float, tv_mult: float) -> Tuple[Tensor, Tensor]:
    """Two geometric priors on a depth render [H,W,1] with its accumulation [H,W,1] (H and W >= 2), on the device and without a host synchronisation,
    in one fused call (tn_depth_loss): (depth_mult * depth_loss, tv_mult * depth_tv_loss).  depth_loss = mean |depth - depth_image| over the pixels
    with accumulation > 0 and a finite, positive depth_image [H,W,1] (a sensor depth in scene units; None, or no such pixel: 0).  depth_tv_loss =
    0.25 * mean of the four absolute differences of every stride-1 2 x 2 window of the depth whose four pixels all have accumulation > 0 (no such
    window: 0) -- uncovered pixels hold the frame's fill value, which would otherwise put an edge on every silhouette.  A multiplier of 0 gives
    exactly 0 and skips that term.  Both entries are differentiable in `depth` when gradients are on (sign(0) = 0); the accumulation only selects, and
    like depth_image gets no gradient."""
    if torch.is_grad_enabled() and isinstance(depth, Tensor) and depth.requires_grad:
        return _DepthLosses.apply(depth, accumulation, depth_image, float(depth_mult), float(tv_mult))
    out, _ = _depth_loss_call(depth, accumulation, depth_image, depth_mult, tv_mult, False)
    return out[0], out[1]


class _BilateralSlice(torch.autograd.Function):
    """tn_bilagrid_slice as an autograd node: forward applies row `row` of `grids` to the image; backward is one tn_bilagrid_slice_backward call --
    the image's gradient and a dense gradient for `grids`, the row's own entries from the kernel's gather and zeros in every other row."""

    @staticmethod
    def forward(ctx, grids, row, image):
        out, g, img = _bilateral_slice_call(grids, row, image)
        ctx.save_for_backward(g, img)
        ctx.row = row
        return out

    @staticmethod
    def backward(ctx, v_out):
        g, img = ctx.saved_tensors
        img, ps = _image_view(img, "image")
        v_image = torch.empty(tuple(img.shape), device=img.device)
        v_grids = torch.zeros_like(g) if g.shape[0] > 1 else torch.empty_like(g)
        splat_calls.bilagrid_slice_backward(g, ctx.row, img, ps, v_out.float().contiguous(), v_image, v_grids[ctx.row])
        return (v_grids if ctx.needs_input_grad[0] else None), None, (v_image if ctx.needs_input_grad[2] else None)


def _bilateral_check(grids: Tensor, what: str) -> Tensor:
    if not isinstance(grids, Tensor) or not grids.is_cuda or grids.dtype != torch.float32:
        raise ValueError(f"{what}: grids must be an fp32 HIP tensor (the splat path has no CPU fallback)")
    splat_calls._bilagrid_sizes(grids, what)
    return grids.detach().contiguous()


def _bilateral_slice_call(grids: Tensor, row: int, image: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    g = _bilateral_check(grids, "bilateral_slice")
    img, ps = _image_view(image.detach() if isinstance(image, Tensor) else image, "image")
    H, W, Cc = img.shape
    if Cc not in (1, 3) or g.shape[1] != Cc * (Cc + 1):
        raise ValueError(f"bilateral_slice: an image of {Cc} channels and grids of {g.shape[1]} coefficients; RGB [H,W,3] takes 12, thermal [H,W,1] takes 2")
    if not 0 <= int(row) < g.shape[0]:
        raise ValueError(f"bilateral_slice: row {row} of {g.shape[0]} grids")
    if not all(1 <= v <= MAX_IMAGE_SIDE for v in (H, W)):
        raise ValueError(f"bilateral_slice: {H} x {W}, every side must be in 1..{MAX_IMAGE_SIDE}")
    out = torch.empty((H, W, Cc), device=img.device)
    splat_calls.bilagrid_slice(g, int(row), img, ps, out)
    return out, g, img


def bilateral_slice(grids: Tensor, row: int, image: Tensor) -> Tensor:
    """Bilateral-grid colour correction of one frame ("Bilateral Guided Radiance Field Processing", gsplat's bil_grids): row `row` (a host int) of
    `grids` [F,K,L,GH,GW] applied to `image` [H,W,C] -> [H,W,C], one tn_bilagrid_slice call on the current stream, without a host synchronisation.
    C = 3 with K = 12 (a row-major 3 x 4 affine matrix [A | b] per vertex) or C = 1 with K = 2 (gain, offset).  Pixel (i, j) reads the grid at
    ((j + 0.5) / W, (i + 0.5) / H, g), g = 0.299 r + 0.587 g + 0.114 b (C = 1: the value), trilinearly, as
    F.grid_sample(mode="bilinear", padding_mode="border", align_corners=True) does at 2 (x, y, g) - 1; out = A pixel + b.  The interpolation is
    nested lerps, so the identity grid returns the image bit for bit.  Every grid side is in 2..256.  A view whose pixels are further apart than C
    (rgbt[..., :3], rgbt[..., 3:]) is read in place.  Differentiable in `grids` (dense: zeros in the other rows) and in `image` (both paths: A^T v
    and the guidance coordinate; 0 through the clamp at g (L - 1) <= 0 or >= L - 1), bit-reproducibly, without float atomics."""
    if torch.is_grad_enabled() and ((isinstance(grids, Tensor) and grids.requires_grad) or (isinstance(image, Tensor) and image.requires_grad)):
        _bilateral_check(grids, "bilateral_slice")
        return _BilateralSlice.apply(grids, int(row), image)
    return _bilateral_slice_call(grids, row, image)[0]


class _BilateralTV(torch.autograd.Function):
    """tn_bilagrid_tv as an autograd node: value and gradient come from the one forward call; backward scales the saved gradient."""

    @staticmethod
    def forward(ctx, grids, mult):
        out, grad = _bilateral_tv_call(grids, mult, True)
        ctx.save_for_backward(grad)
        return out

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


def _bilateral_tv_call(grids: Tensor, mult: float, want_grad: bool) -> Tuple[Tensor, Optional[Tensor]]:
    g = _bilateral_check(grids, "bilateral_grid_tv")
    out = torch.empty(1, device=g.device)
    grad = torch.empty_like(g) if want_grad else None
    splat_calls.bilagrid_tv(g, float(mult), out, grad)
    return out[0], grad


def bilateral_grid_tv(grids: Tensor, mult: float = 1.0) -> Tensor:
    """mult * the total variation of bilateral grids [F,K,L,GH,GW] (gsplat's total_variation_loss), a device scalar from one tn_bilagrid_tv call
    without a host synchronisation: for each of the three grid axes the sum of squared first differences along it over the entries of one frame's
    difference tensor, the three added and divided by F.  Constant grids give exactly 0.  Differentiable in `grids` (the gradient is written by the
    same call)."""
    if torch.is_grad_enabled() and isinstance(grids, Tensor) and grids.requires_grad:
        _bilateral_check(grids, "bilateral_grid_tv")
        return _BilateralTV.apply(grids, float(mult))
    return _bilateral_tv_call(grids, mult, False)[0]


def ssim(pred: Tensor, gt: Tensor) -> Tensor:
    """pytorch_msssim's SSIM(data_range=1) of two [H,W,C] images (mean over channels), a device scalar; no gradient."""
    return image_loss(pred.detach(), gt, 1.0, 1.0)[2]


def _psnr(pred: Tensor, gt: Tensor) -> Tensor:
    """PeakSignalNoiseRatio(data_range=1.0)."""
    return -10.0 * torch.log10(torch.mean((pred - gt) ** 2))
