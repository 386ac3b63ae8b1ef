"""Which Gaussians matter: every Gaussian scored by what it contributes to the training rays, and trained splats pruned by that score.

Opacity is a poor proxy for importance: an opaque Gaussian buried behind a wall contributes to no frame, a faint one that is alone on its rays is
all a pixel shows, and a Gaussian may matter only to the quarter-resolution thermal frames.  RadSplat ("RadSplat: Radiance Field-Informed Gaussian
Splatting", section 4.2) scores a Gaussian by the maximum over all training rays of its blending weight alpha T and prunes below 0.01; LightGaussian
uses the hit-weighted sum.  `score_gaussians` computes both, and the hit and view counts, in one walk per training frame
(tn_splat_raster_contrib: the forward rasteriser's walk reduced per Gaussian instead of per pixel, without atomics, accumulated on the device),
per spectrum: an RGB frame is walked on the chain its loss trains, a thermal frame of a separate-mode model on the thermal chain.
`prune_mask` turns the scores into a keep mask (a threshold on the importance, or a ratio to keep), `prune_gaussians` removes the others from the
model and from every optimiser, Adam moments and step counts carried along.

A zero score does NOT mean that removing the Gaussian leaves every frame unchanged: a Gaussian at which a pixel stops (the 1e-4 transmittance
rule) is not blended there and scores nothing there, yet it ends that pixel's list; without it the pixel goes on to whatever lies behind.  Fine-tuning
after a prune, LightGaussian's volume term and SH distillation, and pruning inside the MCMC strategy are not built."""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Optional, Sequence

import torch
from torch import Tensor

from . import splat_calls
from .splat_camera import PinholeCamera, camera_struct, pose_camera_record

RADSPLAT_MIN_CONTRIBUTION = 0.01  # RadSplat's pruning threshold on max over rays of alpha T


@dataclass
class GaussianScores:
    """Per Gaussian [N], on the device, over the frames of each spectrum: the largest ray weight (fp32), the sum of the ray weights (fp64), the
    number of pixels it was blended into with a positive weight (int64) and the number of frames that saw it (int32)."""

    max_rgb: Tensor
    sum_rgb: Tensor
    hits_rgb: Tensor
    views_rgb: Tensor
    max_thermal: Tensor
    sum_thermal: Tensor
    hits_thermal: Tensor
    views_thermal: Tensor

    @classmethod
    def zeros(cls, n: int, device) -> "GaussianScores":
        z = lambda dt: torch.zeros(n, dtype=dt, device=device)  # noqa: E731
        return cls(*(z(dt) for _ in range(2) for dt in (torch.float32, torch.float64, torch.int64, torch.int32)))

    def spectrum(self, thermal: bool):
        """(max, sum, hits, views) of one spectrum."""
        s = "thermal" if thermal else "rgb"
        return tuple(getattr(self, f"{k}_{s}") for k in ("max", "sum", "hits", "views"))

    def importance(self) -> Tensor:
        """maximum(max_rgb, max_thermal): a Gaussian only the thermal frames see survives an RGB-only view of importance."""
        return torch.maximum(self.max_rgb, self.max_thermal)

    def combined(self, other: "GaussianScores") -> "GaussianScores":
        """The scores of both sets of frames: elementwise max of the maxima, sums of the rest."""
        return GaussianScores(*(torch.maximum(a, b) if f.name.startswith("max") else a + b
                                for f, a, b in ((f, getattr(self, f.name), getattr(other, f.name)) for f in fields(self))))


@torch.no_grad()
def score_gaussians(model, cameras: Sequence[PinholeCamera], pixel_weights: Optional[Sequence[Optional[Tensor]]] = None) -> GaussianScores:
    """The ray contribution of every Gaussian of `model` over `cameras` (the datamanager's train_cameras).  Each frame is projected and binned as
    `get_outputs` does it -- `_render_params()`, so the 3D filter is in; the eval render's pose rule, so a shared rig row applies and per-frame rows
    do not; the SH degree of the moment; no crop -- and walked on the chain its loss trains: the thermal chain iff camera.is_thermal and the model is
    in separate mode, else the RGB chain.  RGB cameras accumulate into the *_rgb fields, thermal cameras into the *_thermal fields.
    `pixel_weights`: per camera an [H,W] non-negative tensor or None (1 everywhere): region-of-interest or error-weighted scoring.  The scores stay on
    the device and are not read back; the only host synchronisation per frame is tn_splat_bin's own pair count."""
    from .splat import _project_and_bin  # (splat imports this module's functions lazily, in its refinement callback)

    cameras = list(cameras)
    if pixel_weights is not None and len(pixel_weights) != len(cameras):
        raise ValueError(f"score_gaussians: {len(pixel_weights)} pixel weights for {len(cameras)} cameras")
    N, dev = model.num_points, model.means.device
    scores = GaussianScores.zeros(N, dev)
    if N == 0 or not cameras:
        return scores
    aa, deg = model._frame_settings()
    params = [p.detach() for p in model._render_params()]
    for i, camera in enumerate(cameras):
        H, W = int(camera.height), int(camera.width)
        pw = pixel_weights[i] if pixel_weights is not None else None
        if pw is not None:
            if tuple(pw.shape) != (H, W):
                raise ValueError(f"score_gaussians: pixel_weights[{i}] must be [{H},{W}], got {tuple(pw.shape)}")
            pw = pw.to(device=dev, dtype=torch.float32).contiguous()
        cam = camera_struct(camera)
        pose, row = model._pose_row(camera, training=False)
        rec = pose_camera_record(camera, cam, pose.detach(), row) if row is not None else None
        _, ws, cap, total = _project_and_bin(model, cam, params, H, W, deg, aa, max(model._cap, 1 << 16), model._workspace, None, rec)
        if total == 0:  # nothing on screen: the frame scores nothing
            continue
        thermal = bool(camera.is_thermal)
        splat_calls.raster_contrib(cam, N, ws, cap, aa, int(thermal and model.separate), pw, *scores.spectrum(thermal))
    return scores


def prune_mask(scores: GaussianScores, min_contribution: Optional[float] = None, keep_ratio: Optional[float] = None) -> Tensor:
    """The Gaussians to keep, a bool [N] on the scores' device.  Exactly one rule: `min_contribution` keeps importance() >= min_contribution
    (RadSplat's rule; 0.01 is its value); `keep_ratio` keeps the ceil(keep_ratio * N) largest by importance, ties going to the lower index."""
    if (min_contribution is None) == (keep_ratio is None):
        raise ValueError("prune_mask: exactly one of min_contribution and keep_ratio")
    imp = scores.importance()
    if min_contribution is not None:
        if not min_contribution >= 0:
            raise ValueError(f"prune_mask: min_contribution = {min_contribution}: a number >= 0")
        return imp >= min_contribution
    if not 0 <= keep_ratio <= 1:
        raise ValueError(f"prune_mask: keep_ratio = {keep_ratio}: a ratio in [0, 1]")
    N = imp.shape[0]
    k = min(N, math.ceil(round(keep_ratio * N, 9)))  # (0.1 * 30 is 3.0000000000000004 in binary: the ratio's own rounding must not add a Gaussian)
    order = torch.sort(imp, descending=True, stable=True).indices  # stable: equal scores stay in index order
    keep = torch.zeros(N, dtype=torch.bool, device=imp.device)
    keep[order[:k]] = True
    return keep


@torch.no_grad()
def prune_gaussians(model, keep: Tensor, optimizers=None) -> int:
    """Remove the Gaussians outside `keep` (bool [N]) from `model`; returns how many were removed (one host synchronisation: that count).  Every
    gauss_params tensor (opacities_thermal too) is gathered with `keep` in the Gaussians' order, both Adam moments of every group likewise, and
    all are installed as a refinement installs them (`_swap_params`): every optimiser's param_groups point at the new parameters, step counts
    and the other state keys are kept, the 3D filter's buffer is recomputed before the next render, and the refinement statistics start again.
    Pose-optimiser rows and bilateral grids are untouched.  `optimizers`: an `Optimizers`, a dict group -> optimiser, or None.  An all-false mask
    leaves a model without Gaussians, which renders the background."""
    N = model.num_points
    if not isinstance(keep, Tensor) or keep.dtype != torch.bool or tuple(keep.shape) != (N,):
        got = f"{keep.dtype} {tuple(keep.shape)}" if isinstance(keep, Tensor) else type(keep).__name__
        raise ValueError(f"prune_gaussians: keep must be a bool tensor [{N}], got {got}")
    keep = keep.to(model.means.device)
    removed = N - int(keep.sum())
    if removed == 0:
        return 0
    opts = getattr(optimizers, "optimizers", optimizers) or {}
    gather = lambda t: t.detach()[keep].contiguous()  # noqa: E731  (a boolean gather in torch: this runs a handful of times per training)
    new = {k: gather(model.gauss_params[k]) for k in model.param_names}
    new_moments = {k: (gather(m), gather(v)) for k, (m, v) in model._adam_moments(opts).items()}
    model._swap_params(optimizers, opts, new, new_moments)
    # what the last training frame and the statistics so far refer to are other Gaussians now
    model.xys_grad_norm = model.vis_counts = model.max_2Dsize = None
    model.last_radii = None
    model.last_xys_grad = model.last_xys_absgrad = None
    return removed
