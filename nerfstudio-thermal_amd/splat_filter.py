"""Mip-Splatting's 3D smoothing filter for thermal splats ("Mip-Splatting: Alias-free 3D Gaussian Splatting", eq. 6-7 and 9): the world-space
companion of rasterize_mode "antialiased" (the paper's 2D Mip filter).  One set of Gaussians is trained against cameras whose sampling rates differ
by large factors -- a 640 x 480 RGB frame beside a 160 x 120 thermal frame of the same rig, less again early in the resolution schedule -- and is
then looked at from distances no training frame had.  The filter band-limits every Gaussian to the highest frequency any training camera could
have sampled: each scale is convolved with an isotropic Gaussian of standard deviation filter_3D[k] and the opacity is compensated, so that no
Gaussian can grow thinner than what was observable.

  filter_3D[k] = sqrt(variance) / nu_k,   nu_k = max over the cameras that see k of max(fx, fy) / depth      (`compute_3d_filter`)
  log s'_i = 1/2 log(s_i^2 + f^2),   o' = logit(sigmoid(o) sqrt(prod_i s_i^2 / (s_i^2 + f^2)))                 (`apply_3d_filter`)

The maximum is taken per camera, as the paper states it; the official code's shortcut (one global focal length over each Gaussian's smallest depth)
is wrong by the ratio of the focal lengths on an RGB + thermal rig and is not reproduced.  The published implementation is this per-Gaussian
pre-transform, not a change to the rasteriser: the model hands the filtered log-scales and logits to the calls it already makes.

All three operations are HIP (csrc/tn_splat_filter3d.hip; `splat_calls.filter3d_*` know the argument order): evaluated in double and rounded once,
no atomics, no read-back, the same bits on every run; there is no CPU fallback.  `filter_camera_table` is host code in float64.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import splat_calls
from .splat_calls import FILTER_CAMERA_FLOATS
from .splat_camera import PinholeCamera

F64 = torch.float64


def filter_camera_table(cameras: Sequence[PinholeCamera], device=None) -> Tensor:
    """[C,18] fp32 rows of tn_filter3d_splat_compute: the 12 entries of the world -> camera matrix in TnSplatCamera.viewmat's convention (gsplat's:
    x right, y down, z forward -- camera_struct's flip and analytic inverse), then fx, fy, cx, cy, width, height.  Built in float64 from the
    cameras' poses and rounded once; on the host unless `device` is given."""
    flip = torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=F64))
    rows = []
    for cam in cameras:
        c2w = cam.camera_to_world.detach().to("cpu", F64)
        R_inv = (c2w[:3, :3] @ flip).T
        view = torch.cat([R_inv, -R_inv @ c2w[:3, 3:4]], 1)
        rows.append(torch.cat([view.reshape(-1), torch.tensor([cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height], dtype=F64)]))
    table = torch.stack(rows).float() if rows else torch.zeros((0, FILTER_CAMERA_FLOATS), dtype=torch.float32)
    return table if device is None else table.to(device)


def compute_3d_filter(means: Tensor, camera_table: Tensor, near: float = 0.2, variance: float = 0.2, out: Optional[Tensor] = None) -> Tensor:
    """filter_3D [N] fp32 of means [N,3] under the cameras of `camera_table` [C,18] (both contiguous fp32 on the device): two launches on the
    current stream, nothing read back.  A Gaussian no camera sees takes the largest filter of the seen ones; when none is seen (or C == 0) every
    row is 0, which `apply_3d_filter` passes through bit for bit."""
    m = means.detach()
    if out is None:
        out = torch.empty((m.shape[0],), dtype=torch.float32, device=m.device)
    if m.shape[0] > 0:
        splat_calls.filter3d_compute(m, camera_table, near, variance, out)
    return out


class _Filter3D(torch.autograd.Function):
    """(scales, opacities[, opacities_thermal]) -> the filtered ones; filter_3D takes no gradient."""

    @staticmethod
    def forward(ctx, filter_3d, scales, opacities, opacities_thermal=None):
        s, o = scales.detach().contiguous(), opacities.detach().contiguous()
        th = None if opacities_thermal is None else opacities_thermal.detach().contiguous()
        s_out, o_out = torch.empty_like(s), torch.empty_like(o)
        th_out = None if th is None else torch.empty_like(th)
        if s.shape[0] > 0:
            splat_calls.filter3d_apply(s, o, filter_3d, s_out, o_out, th, th_out)
        ctx.save_for_backward(filter_3d, s, o, *([] if th is None else [th]))
        return (s_out, o_out) if th is None else (s_out, o_out, th_out)

    @staticmethod
    def backward(ctx, v_s_out, v_o_out, v_th_out=None):
        filter_3d, s, o, *th = ctx.saved_tensors
        th = th[0] if th else None
        v_s_out, v_o_out = v_s_out.float().contiguous(), v_o_out.float().contiguous()
        v_s, v_o = torch.empty_like(s), torch.empty_like(o)
        v_th = None
        if th is not None:
            v_th_out, v_th = v_th_out.float().contiguous(), torch.empty_like(th)
        if s.shape[0] > 0:
            splat_calls.filter3d_apply_backward(s, o, filter_3d, v_s_out, v_o_out, v_s, v_o, th, v_th_out if th is not None else None, v_th)
        return (None, v_s, v_o) if th is None else (None, v_s, v_o, v_th)


def apply_3d_filter(scales: Tensor, opacities: Tensor, filter_3d: Tensor, opacities_thermal: Optional[Tensor] = None) -> Tuple[Tensor, ...]:
    """(scales' [N,3], opacities' [N,1][, opacities_thermal' [N,1]]): log-scales and opacity logits convolved with the per-Gaussian filter
    `filter_3d` [N], differentiable in all but the filter (one launch each way).  Rows with filter_3d == 0 pass through bit for bit, values and
    gradients alike."""
    N = scales.shape[0]
    if tuple(scales.shape) != (N, 3) or opacities.numel() != N or tuple(filter_3d.shape) != (N,) or \
            (opacities_thermal is not None and opacities_thermal.numel() != N):
        raise ValueError(f"apply_3d_filter: scales [N,3], opacities [N,1] and filter_3D [N] of one N expected, got {tuple(scales.shape)}, "
                         f"{tuple(opacities.shape)} and {tuple(filter_3d.shape)}")
    f = filter_3d.detach()
    if opacities_thermal is None:
        return _Filter3D.apply(f, scales, opacities)
    return _Filter3D.apply(f, scales, opacities, opacities_thermal)
