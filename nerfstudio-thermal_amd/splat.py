"""N4: forward Gaussian-splat render with an RGB + thermal colour per Gaussian ("thermal-splatfacto", BASELINE config 4).

The reference has no thermal-splatfacto method; the boundary mirrored here is stock `SplatfactoModel.get_outputs(camera)`
(nerfstudio/models/splatfacto.py:659-822) with the parameter names of its `gauss_params` (means, scales, quats, opacities, features_dc,
features_rest) plus a second set of SH coefficients with one channel (features_dc_thermal / features_rest_thermal) rendered through the
same rasteriser -- the splat analogue of thermal-nerfacto's shared density (`thermal_opacity_mode` "shared", the default).  With
`thermal_opacity_mode` "separate" -- the analogue of ThermalNerfactoModelConfig.density_mode "separate", the reference's default -- every
Gaussian also has `opacities_thermal` [N,1] (logits, started at logit(0.1) like `opacities`, its own optimiser group): RGB, accumulation and
depth composite with sigmoid(opacities), the thermal channel with sigmoid(opacities_thermal) through a transmittance chain of its own over the
same depth-sorted tile lists (its own 1e-4 stop, its background weighted by its own final transmittance; `accumulation_thermal` [H,W,1] is its
accumulation), so glass can be clear in RGB and opaque in thermal.  That mode gives every entry point its thermal group; its backward is as exact and
bit-reproducible, `last_xys_grad` sums both chains; refinement culls a Gaussian for low opacity only when BOTH opacities are below
`cull_alpha_thresh`, and carries, copies and resets the thermal logits exactly as the opacities.  `opacity_loss_mult` > 0 adds the NeRF model's
`density_loss` (models/thermal_nerfacto.py:328-344) on the two opacities.  With `removal_min_opacity_diff` = thr set (separate mode only; None = off)
the eval render also returns ThermalNeRF's removal renders (models/thermal_nerfacto.py:460-487, scripts/render.py:737-765, opacities for densities):
`removal` [H,W,3], the RGB colour composited only from the Gaussians with |o - o_th| < thr * o, and `removal_thermal` [H,W,1], the thermal colour
from those with |o_th - o| < thr * o_th (o, o_th the two sigmoids; strict, so thr = 0 is the background), each with a transmittance chain, stop
and background weight of its own -- what sits behind glass or an IR-transparent cover -- from ONE more rasteriser launch
(tn_splat_raster_removal_sep) over the tile lists the frame already has; training renders never carry them.
`get_outputs` is the eval render.  `get_train_outputs` is the same render as a differentiable function of every `gauss_params` tensor: its
backward (tn_splat_raster_backward / tn_splat_project_backward) is the exact, bit-reproducible derivative of the forward this file computes,
and it leaves dL/d xys per Gaussian in `last_xys_grad` (what splatfacto's densification reads as `self.xys.grad`, splatfacto.py:355).
Depth is returned detached unless `differentiable_depth` is on (classic mode): then `depth` [H,W,1] carries gradients too -- depth = D / accumulation
where the pixel is covered, D riding the RGB chain as a fifth channel; the fill value elsewhere takes none -- through the depth groups of tn_splat_raster_backward /
tn_splat_project_backward, as exact and atomic-free as the rest; a backward whose loss never touched depth leaves the groups out and gives the
bits of before.  `depth_loss_mult` / `depth_tv_loss_mult` above 0 (both default 0) add `depth_loss` -- the L1 distance to the batch's `depth_image`, a
sensor depth -- and `depth_tv_loss` -- the depth's 2 x 2 total variation -- over the covered pixels, on RGB and thermal frames alike (`depth_losses`:
tn_depth_loss).  Training follows splatfacto's refinement (splatfacto.py:346-498): `after_train` accumulates the gradient
statistics (tn_splat_grad_stats), `refinement_after` splits, duplicates and culls the Gaussians (tn_splat_refine_plan / tn_splat_refine_apply)
and carries every optimiser's parameter and Adam moments along, and resets the opacities now and then.  The objective is splatfacto's
(splatfacto.py:848-903): `get_loss_dict` takes the image loss of the frame's spectrum; `background_color = "random"` draws
a random RGB + thermal background per training frame.  Construction follows splatfacto's populate_modules (splatfacto.py:190-242): from
`seed_points` (the dataparser's points3D_xyz / points3D_rgb, dataparser.py `load_3D_points`) one Gaussian per point, its log-scale the log of the
mean distance to its 3 nearest neighbours (`knn_distances`: tn_knn, an exact HIP search), or -- without seeds or with `random_init` -- the random
cube of before.  Under the resolution schedule the eval render is always full size.  With `tv_pixel_loss_mult` / `cross_channel_loss_mult` above 0
(both default 0: stock splatfacto has neither) `get_loss_dict` adds `tv_pixel_loss` and `cross_channel_loss` on RGB frames.  The eval render takes
splatfacto's crop box: `set_crop(box)` / `crop_box` and `get_outputs_for_camera(camera, obb_box)`, the door of the viewer, ns-render and the
exporter.  With a box set `get_outputs` renders only the Gaussians whose mean is strictly inside it, bit for bit the frame of a model holding those
alone -- rgb, thermal, depth, the accumulations and the removal renders.  The reference gathers six parameter tensors through a boolean index per
frame; here the box test is the first thing the projection kernel does (tn_splat_project with its box): a Gaussian outside leaves with radius 0
and no tiles, as one behind the camera, a block of Gaussians that are all outside never reads its SH coefficients, and nothing is copied, allocated or
read back.  The training render never crops (the reference crops only outside training), and the box is neither a parameter nor in the state dict.
With a pose row `get_train_outputs` is differentiable in it: the pose instantiations of the projection kernels read the corrected camera
(the pose groups of tn_splat_project / tn_splat_project_backward), and the backward reduces dL/d view' over the Gaussians without atomics, bit-reproducibly;
the SH view directions take the corrected position as a value (splatfacto.py:770).  Densification has a second strategy,
`strategy` = "mcmc" ("3D Gaussian Splatting as Markov Chain Monte Carlo": gsplat's MCMCStrategy, current splatfacto's strategy "mcmc" with
`max_gs_num`): a fixed budget of Gaussians instead of gradient thresholds.  Every `refine_every` steps (between warmup_length and stop_split_at)
the refinement callback relocates the dead Gaussians -- visible opacity (the larger of the two sigmoids in separate mode) <= `mcmc_min_opacity` --
onto live ones drawn with probability proportional to their visible opacity (torch.multinomial of the model's noise_generator), correcting the
opacity and the scale of source and copies so that the render is preserved, then grows the population by `mcmc_grow_factor` up to `max_gs_num`
in the same way; both go through tn_splat_mcmc_relocate, in place on every parameter tensor and both Adam moments (source rows lose their
moments, as in gsplat), with the relocation values evaluated in double.  One more callback adds position noise after every step,
means += Sigma (randn * g * noise_lr * lr of the means), g = sigmoid(100 ((1 - o_vis) - 0.995)), in one tn_splat_mcmc_noise launch, and
`get_loss_dict` adds `mcmc_opacity_reg` * mean(sigmoid(opacities)) (+ the thermal mean in separate mode) and `mcmc_scale_reg` * mean(exp(scales)).
No gradient statistics, no cull, no opacity reset; `last_refine_counts` = (dead, relocated, added).  "default" (the default) takes the code path
of before, untouched.  Whether "mcmc" trains thermal scenes better is not established (profiles/splat_mcmc.md).  With `use_bilateral_grid` every training frame has a bilateral grid
("Bilateral Guided Radiance Field Processing"; gsplat's bil_grids, current splatfacto's use_bilateral_grid / grid_shape / tv_loss): a small 3-D grid
of affine colour transforms, indexed by pixel position and brightness, that `get_train_outputs` applies to the render of the frame's spectrum
after the clamp (`bilateral_slice`: tn_bilagrid_slice, its backward a gather without atomics) and `get_loss_dict` regularises by its total
variation (`tv_loss`, `bilateral_grid_tv`: tn_bilagrid_tv), so that gain, offset and vignetting that drift from frame to frame -- a thermal
camera's automatic gain control and flat-field corrections, an RGB camera's auto-exposure -- go into the grid instead of into floaters.
`bil_grids` [F_rgb,12,L,GH,GW] holds 3 x 4 matrices for the RGB frames, `bil_grids_thermal` [F_th,2,L,GH,GW] a gain and an offset for the thermal
ones (this project's addition), both the identity at first, which returns the render bit for bit; their groups are bilateral_grid /
bilateral_grid_thermal (optim.SPLAT_BILAGRID_OPTIMIZERS, splatfacto's rates; its 1000-step warm-up of the group is not built:
ExponentialDecayLR has none).  Eval renders are never corrected.  What the grid is worth on a drifting scene is an observation in
profiles/splat_bilagrid.md, not a claim.  With `use_3d_filter` every render -- training, eval, cropped, removal, and so the TSDF exporter and
the camera paths -- reads Mip-Splatting's 3D smoothing filter (splat_filter.py; the world-space companion of "antialiased"): `filter_3D` [N], a
buffer computed from the cameras given to `set_filter_cameras` (tn_filter3d_splat_compute; again every `filter_3d_every` training steps and whenever
the cameras or the Gaussians change), widens the log-scales and compensates the opacity logits in one launch before the projection
(tn_filter3d_splat_apply, its backward closed form), so the gradients reach the raw parameters, which refinement, culls, the opacity reset and the
scale regulariser keep reading.  Without cameras the render is the unfiltered one, bit for bit; strategy "mcmc" refuses the switch (its relocation
preserves the render of raw parameters: out of scope).  Whether the filter improves a real RGB + thermal capture is not claimed.  Masks are not built.  Parity is unpinned (gsplat is a third-party package outside the reference
tree; oracle/splat_oracle.py restates its published algorithm).  No CPU path.

splat_calls.py: the C entry points, their names and argument order, the workspaces, `knn_distances`, `mcmc_relocate`, `mcmc_noise`.
splat_camera.py: `PinholeCamera`, `camera_struct`, the resolution schedule's camera, `undistorted_camera`, `OrientedBox`, the pose optimiser.
splat_prune.py: `score_gaussians`, `prune_mask`, `prune_gaussians` -- every Gaussian's ray contribution (tn_splat_raster_contrib) and pruning by it;
                `prune_at_steps` / `set_prune_cameras` run it from the refinement callback (off by default).
splat_image.py: `image_loss`, `resize_image`, `undistort_image`, `thermal_regularizers`, `depth_losses`, `bilateral_slice`, `bilateral_grid_tv`, `ssim`.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib, splat_calls
from .config import CameraOptimizerConfig
from .splat_calls import KNN_MAX_K, _PARAM_NAMES, knn_distances, mcmc_noise, mcmc_relocate, param_names  # noqa: F401
from .splat_camera import (CAMERA_OPTIMIZER_MODES, OrientedBox, PinholeCamera, SplatCameraOptimizer, camera_struct, downscale_factor,  # noqa: F401
                           pose_camera_record, projection_matrix, rescaled_camera, undistorted_camera)
from .splat_filter import apply_3d_filter, compute_3d_filter, filter_camera_table  # noqa: F401
from .splat_image import (MAX_IMAGE_SIDE, _psnr, bilateral_grid_tv, bilateral_slice, depth_losses, image_loss, resize_image, ssim,  # noqa: F401
                          thermal_regularizers, undistort_image)

BLOCK_WIDTH = 16  # splatfacto.py:738
STRATEGIES = ("default", "mcmc")  # densification: splatfacto's gradient-threshold refinement, or gsplat's MCMCStrategy
MCMC_N_MAX = 51  # the relocation ratio's cap (gsplat's n_max; tn_splat_mcmc_relocate's)


@dataclass
class ThermalSplatfactoModelConfig:
    """The fields of SplatfactoModelConfig (splatfacto.py:103-172) that the render and the refinement read, with the reference's defaults."""

    sh_degree: int = 3
    sh_degree_interval: int = 1000
    rasterize_mode: str = "classic"  # or "antialiased"
    background_color: str = "black"  # "black" | "white" | "random" (a random RGB + thermal background per training frame; eval: the viewer colour)
    background_thermal: float = 0.0
    # loss (splatfacto.py:146-160); thermal_loss_mult weights a thermal frame's loss (this project's: the reference has no thermal splat model)
    ssim_lambda: float = 0.2
    use_scale_regularization: bool = False
    max_gauss_ratio: float = 10.0
    thermal_loss_mult: float = 1.0
    # ThermalNeRF's regularisers of the thermal render on RGB frames (ThermalNerfactoModelConfig's names; the NeRF path runs both at 1e-6); 0 = off
    tv_pixel_loss_mult: float = 0.0
    cross_channel_loss_mult: float = 0.0
    # the training render's depth as a differentiable output (splatfacto's is: splatfacto.py:805-820); classic mode only -- in antialiased mode the
    # depth is blended by a chain of its own whose final transmittance and last contributor the training forward does not keep.  Off: depth is detached
    differentiable_depth: bool = False
    # geometric priors on the depth render over its covered pixels (need differentiable_depth; 0 = off): depth_loss = mean |depth - batch["depth_image"]|
    # (a sensor depth [H,W,1] in scene units, nerfstudio's DepthDataset key; 0 for a batch without one), depth_tv_loss = the depth's 2 x 2 total variation
    depth_loss_mult: float = 0.0
    depth_tv_loss_mult: float = 0.0
    # "shared": one opacity blends RGB and thermal; "separate": the thermal channel has opacities_thermal and a transmittance chain of its own
    # (ThermalNerfactoModelConfig.density_mode's two values).  density_loss (thermal_nerfacto.py:328-344, separate mode, 0 = off) =
    # opacity_loss_mult * (mean|o_th - o.detach()| + rgb_opacity_loss_mult * mean|o - o_th.detach()|) on the sigmoids
    thermal_opacity_mode: str = "shared"
    opacity_loss_mult: float = 0.0
    rgb_opacity_loss_mult: float = 0.01
    # removal renders in eval (thermal_nerfacto.py:460-487; render.py's removal_min_density_diff): a Gaussian stays in `removal` while
    # |o - o_th| < removal_min_opacity_diff * o, in `removal_thermal` while |o_th - o| < removal_min_opacity_diff * o_th.  None = off; separate mode only
    removal_min_opacity_diff: Optional[float] = None
    # initialisation (splatfacto.py:127-131): random_init ignores the model's seed_points
    random_init: bool = False
    num_random: int = 50000
    random_scale: float = 10.0
    # refinement (splatfacto.py:108-148)
    warmup_length: int = 500
    refine_every: int = 100
    cull_alpha_thresh: float = 0.1
    cull_scale_thresh: float = 0.5
    continue_cull_post_densification: bool = True
    reset_alpha_every: int = 30
    densify_grad_thresh: float = 0.0002
    # AbsGS's statistic (gsplat's `absgrad`, splatfacto's `use_absgrad`): densify on the norm of sum over pixels |d L_p / d xys| per component
    # instead of |sum over pixels d L_p / d xys|, whose pixel terms cancel on a large Gaussian over fine structure (tn_splat_raster_backward with v_xys_abs;
    # `last_xys_absgrad`).  The absolute statistic is several times the signed one (a median 3.5 to 12.5 times on the backward test scenes), so
    # densify_grad_thresh wants raising with it: gsplat's documentation advises about 0.0008 with absgrad where 0.0002 is used without.  The
    # default above is NOT changed by the flag, and no scene has been trained here to pick a value.
    use_absgrad: bool = False
    densify_size_thresh: float = 0.01
    n_split_samples: int = 2
    cull_screen_size: float = 0.15
    split_screen_size: float = 0.05
    stop_screen_size_at: int = 4000
    stop_split_at: int = 15000
    # densification strategy (current splatfacto's `strategy`): "default" is the gradient-threshold refinement above; "mcmc" is gsplat's MCMCStrategy
    # ("3D Gaussian Splatting as Markov Chain Monte Carlo"): a budget of max_gs_num Gaussians, every refine_every steps the dead ones (visible
    # opacity <= mcmc_min_opacity) are relocated onto live ones and the population grows by mcmc_grow_factor up to the budget, every step the means
    # take noise of noise_lr x their learning rate shaped by each Gaussian's covariance, and the loss adds mcmc_opacity_reg * mean(opacity) and
    # mcmc_scale_reg * mean(exp(scales)).  No gradient statistics, no threshold, no cull, no opacity reset.  Whether it trains thermal scenes better
    # than "default" has not been established here.
    strategy: str = "default"
    max_gs_num: int = 1_000_000
    noise_lr: float = 5e5
    mcmc_opacity_reg: float = 0.01
    mcmc_scale_reg: float = 0.01
    mcmc_min_opacity: float = 0.005
    mcmc_grow_factor: float = 1.05
    # coarse-to-fine training (splatfacto.py:112-116): 1 / 2^num_downscales of the resolution at first, doubled every resolution_schedule steps
    resolution_schedule: int = 250
    num_downscales: int = 0
    # pose refinement (ThermalNerfactoModelConfig's camera_optimizer / camera_optimizer_thermal; cameras/camera_optimizers.py:39-56): "off",
    # "SO3xR3" (a row per training frame, training renders only) or "shared_SO3xR3" (one row for the whole spectrum, the rig extrinsic, eval
    # renders too).  RGB frames read camera_optimizer, thermal frames camera_optimizer_thermal; penalty_scale < 0 also means off
    camera_optimizer: CameraOptimizerConfig = field(default_factory=CameraOptimizerConfig)
    camera_optimizer_thermal: CameraOptimizerConfig = field(default_factory=CameraOptimizerConfig)
    # Mip-Splatting's 3D smoothing filter (splat_filter.py), the world-space companion of rasterize_mode "antialiased": every render reads scales
    # convolved with a per-Gaussian filter of standard deviation sqrt(filter_3d_variance) / nu_k -- nu_k the highest sampling rate (focal length in
    # pixels over depth) of any camera given to `set_filter_cameras` that sees the Gaussian beyond filter_3d_near -- and the compensated opacity;
    # the buffer is recomputed every filter_3d_every training steps and whenever the cameras or the Gaussians change.  The parameters stay raw:
    # refinement, culls, the opacity reset and the scale regulariser read them as before.  Not with strategy "mcmc", whose relocation preserves
    # the render of the raw parameters only.  Off: nothing new is called
    use_3d_filter: bool = False
    filter_3d_variance: float = 0.2
    filter_3d_near: float = 0.2
    filter_3d_every: int = 100
    # pruning by ray contribution (splat_prune.py; RadSplat prunes at steps 16000 and 24000 below 0.01): at each of prune_at_steps the refinement
    # callback, after its own work, scores every Gaussian over the cameras given to `set_prune_cameras` and removes those whose largest blending
    # weight alpha T on any training ray of either spectrum is below prune_min_contribution.  The steps lie after stop_split_at (a prune right
    # after an opacity reset would score clamped opacities, and resets end there) and are refinement steps (multiples of refine_every: the
    # callback runs on no other).  Not with strategy "mcmc", whose budget is the user's stated N.  Empty: nothing new is called
    prune_at_steps: Tuple[int, ...] = ()
    prune_min_contribution: float = 0.01
    # per-frame colour correction (current splatfacto's use_bilateral_grid / grid_shape; gsplat's bilateral grids): every training frame has a grid
    # of affine colour transforms, grid_shape = (GW, GH, L) -- indexed by pixel position and brightness -- applied to its training render only and
    # regularised by tv_loss = bilateral_grid_tv_mult * total variation (10: splatfacto's constant).  RGB frames have 3 x 4 matrices (bil_grids),
    # thermal frames a gain and an offset (bil_grids_thermal: this project's).  Every side of the grid is in 2..256.  Off: no parameter, no group
    use_bilateral_grid: bool = False
    grid_shape: Tuple[int, int, int] = (16, 16, 8)
    bilateral_grid_tv_mult: float = 10.0

    def __post_init__(self):
        steps = tuple(self.prune_at_steps) if isinstance(self.prune_at_steps, (tuple, list)) else None
        if steps is None or not all(isinstance(s, int) and not isinstance(s, bool) for s in steps) or any(b <= a for a, b in zip(steps, steps[1:])):
            raise ValueError(f"prune_at_steps = {self.prune_at_steps!r}: increasing integer steps")
        self.prune_at_steps = steps
        if not self.prune_min_contribution >= 0:
            raise ValueError(f"prune_min_contribution = {self.prune_min_contribution}: a contribution threshold cannot be negative")
        if steps and self.strategy == "mcmc":
            raise ValueError('prune_at_steps does not go with strategy "mcmc": its budget max_gs_num is the stated number of Gaussians')
        if steps and steps[0] <= self.stop_split_at:
            raise ValueError(f"prune_at_steps = {steps}: every step must lie after stop_split_at = {self.stop_split_at} (a prune right after an opacity "
                             "reset would score clamped opacities, and the resets end there)")
        if self.refine_every > 0 and any(s % self.refine_every for s in steps):
            raise ValueError(f"prune_at_steps = {steps}: the refinement callback runs every refine_every = {self.refine_every} steps, a prune on another "
                             "step would never happen")
        shape = tuple(self.grid_shape) if isinstance(self.grid_shape, (tuple, list)) else ()
        if len(shape) != 3 or not all(isinstance(v, int) and not isinstance(v, bool) and 2 <= v <= splat_calls.BILAGRID_MAX_SIDE for v in shape):
            raise ValueError(f"grid_shape = {self.grid_shape!r}: (GW, GH, L), three integers in 2..{splat_calls.BILAGRID_MAX_SIDE}")
        self.grid_shape = shape
        if not self.bilateral_grid_tv_mult >= 0:
            raise ValueError(f"bilateral_grid_tv_mult = {self.bilateral_grid_tv_mult}: a loss multiplier cannot be negative")
        for name in ("camera_optimizer", "camera_optimizer_thermal"):
            mode = getattr(self, name).mode
            if mode not in CAMERA_OPTIMIZER_MODES:
                raise ValueError(f'{name}.mode = {mode!r}: the splat path refines poses with "SO3xR3" or "shared_SO3xR3" ("off": not at all)')
        for name in ("tv_pixel_loss_mult", "cross_channel_loss_mult", "opacity_loss_mult", "rgb_opacity_loss_mult", "depth_loss_mult", "depth_tv_loss_mult"):
            if getattr(self, name) < 0:
                raise ValueError(f"{name} = {getattr(self, name)}: a loss multiplier cannot be negative")
        if self.differentiable_depth and self.rasterize_mode == "antialiased":
            raise ValueError('differentiable_depth needs rasterize_mode "classic": antialiased depth is blended with the uncompensated opacity in a chain of '
                             "its own, whose final transmittance and last contributor the training forward does not keep for a backward")
        for name in ("depth_loss_mult", "depth_tv_loss_mult"):
            if getattr(self, name) > 0 and not self.differentiable_depth:
                raise ValueError(f"{name} = {getattr(self, name)} needs differentiable_depth: with a detached depth the loss would train nothing")
        if self.thermal_opacity_mode not in ("shared", "separate"):
            raise ValueError(f'thermal_opacity_mode = {self.thermal_opacity_mode!r}: "shared" or "separate"')
        if self.strategy not in STRATEGIES:
            raise ValueError(f'strategy = {self.strategy!r}: "default" or "mcmc"')
        if not self.max_gs_num >= 1:
            raise ValueError(f"max_gs_num = {self.max_gs_num}: the budget holds at least one Gaussian")
        for name in ("noise_lr", "mcmc_opacity_reg", "mcmc_scale_reg"):
            if not getattr(self, name) >= 0:
                raise ValueError(f"{name} = {getattr(self, name)}: a number >= 0")
        if not 0 < self.mcmc_min_opacity < 1:
            raise ValueError(f"mcmc_min_opacity = {self.mcmc_min_opacity}: an opacity inside (0, 1)")
        if not self.mcmc_grow_factor >= 1:
            raise ValueError(f"mcmc_grow_factor = {self.mcmc_grow_factor}: a factor >= 1")
        if self.use_3d_filter and self.strategy == "mcmc":
            raise ValueError('use_3d_filter does not go with strategy "mcmc": the relocation\'s render-preserving opacity and scale correction is '
                             "stated on the raw parameters, not on the filtered ones the render would read")
        for name in ("filter_3d_variance", "filter_3d_near"):
            if not (getattr(self, name) >= 0 and math.isfinite(getattr(self, name))):
                raise ValueError(f"{name} = {getattr(self, name)}: a finite number >= 0")
        if isinstance(self.filter_3d_every, bool) or not isinstance(self.filter_3d_every, int) or self.filter_3d_every < 1:
            raise ValueError(f"filter_3d_every = {self.filter_3d_every!r}: a number of steps >= 1")
        if self.removal_min_opacity_diff is not None:
            if self.thermal_opacity_mode != "separate":
                raise ValueError('removal_min_opacity_diff needs thermal_opacity_mode "separate": the removal renders compare the two opacities')
            if not self.removal_min_opacity_diff >= 0:
                raise ValueError(f"removal_min_opacity_diff = {self.removal_min_opacity_diff}: a number >= 0, or None for no removal renders")


SH_C0 = 0.28209479177387814  # utils/spherical_harmonics.py


def RGB2SH(rgb: Tensor) -> Tensor:
    """utils/spherical_harmonics.py: RGB2SH"""
    return (rgb - 0.5) / SH_C0


VIEWER_BACKGROUND = (0.1490, 0.1647, 0.2157)  # eval background of "random" (splatfacto.py:680-682)


def opacity_density_loss(opacities: Tensor, opacities_thermal: Tensor, opacity_loss_mult: float, rgb_opacity_loss_mult: float) -> Tensor:
    """ThermalNeRF's density_loss (models/thermal_nerfacto.py:328-344) on the two opacity logits [N,1] of the separate mode:
    opacity_loss_mult * (mean|s(o_th) - s(o).detach()| + rgb_opacity_loss_mult * mean|s(o) - s(o_th).detach()|), s = sigmoid.  The first term pulls
    the thermal opacity towards the RGB one, the second (weaker) the RGB one towards the thermal: each term's gradient reaches only its own tensor.
    Elementwise on [N,1], plain torch."""
    o, o_th = torch.sigmoid(opacities), torch.sigmoid(opacities_thermal)
    return opacity_loss_mult * ((o_th - o.detach()).abs().mean() + rgb_opacity_loss_mult * (o - o_th.detach()).abs().mean())


def identity_bilateral_grids(num_frames: int, channels: int, grid_shape: Tuple[int, int, int], device=None) -> Tensor:
    """[F, C (C + 1), L, GH, GW] grids of the identity transform (gsplat's initialisation): the matrix's diagonal -- for one channel the gain --
    is 1, every other entry 0.  grid_shape = (GW, GH, L)."""
    GW, GH, L = grid_shape
    eye = torch.eye(channels, channels + 1).reshape(1, channels * (channels + 1), 1, 1, 1)
    grids = eye.repeat(num_frames, 1, L, GH, GW).contiguous()
    return grids if device is None else grids.to(device)


def _is_thermal_frame(batch) -> bool:
    is_th = batch["is_thermal"]
    return bool(is_th) if not hasattr(is_th, "__len__") else bool(torch.as_tensor(is_th).reshape(-1)[0])


# optimiser group -> gauss_params entry (splatfacto.py:620-628, plus the thermal SH coefficients)
GROUP_PARAMS = {"xyz": "means", "features_dc": "features_dc", "features_rest": "features_rest", "opacity": "opacities", "scaling": "scales",
                "rotation": "quats", "features_dc_thermal": "features_dc_thermal", "features_rest_thermal": "features_rest_thermal"}
# thermal_opacity_mode "separate": the thermal opacity logits come ninth, in a group of their own
GROUP_PARAMS_SEP = {**GROUP_PARAMS, "opacities_thermal": "opacities_thermal"}


def _project_and_bin(model, cam, params, H: int, W: int, deg: int, aa: int, cap: int, workspace, crop: Optional[_lib.TnSplatCrop] = None,
                     pose_rec: Optional[Tensor] = None):
    """One frame's project -> bin into `workspace(N, cap, tiles)`, a buffer for `cap` (Gaussian, tile) pairs: the caller says where it comes from.
    `crop` (the eval render's box) and `pose_rec` (pose_camera_record) go to splat_calls.project, which picks the instantiation.  A frame with more
    pairs grows `cap` once and is redone.  Leaves `last_projection` / `last_num_intersections` on the model
    and returns (projection tensors, workspace, cap, pairs).  No Gaussians: nothing to project, no workspace (None), the frame is the background."""
    i32 = torch.int32
    N, dev = params[0].shape[0], params[0].device
    tiles = ((W + BLOCK_WIDTH - 1) // BLOCK_WIDTH) * ((H + BLOCK_WIDTH - 1) // BLOCK_WIDTH)
    proj = {"xys": torch.empty((N, 2), device=dev), "depths": torch.empty((N,), device=dev), "radii": torch.empty((N,), dtype=i32, device=dev),
            "conics": torch.empty((N, 3), device=dev), "compensation": torch.empty((N,), device=dev),
            "num_tiles_hit": torch.empty((N,), dtype=i32, device=dev), "tile_box": torch.empty((N, 4), dtype=i32, device=dev)}
    ws, total = None, C.c_int64(0)
    for attempt in range(2 if N > 0 else 0):
        ws = workspace(N, cap, tiles)
        splat_calls.project(cam, params, deg, aa, proj, ws, cap, crop, pose_rec)
        if splat_calls.bin(cam, proj["depths"], N, ws, cap, total, may_grow=attempt == 0):
            break
        cap = int(total.value * 1.25) + 1024  # more (Gaussian, tile) pairs than the workspace holds: grow once and redo the frame
    model.last_projection = proj
    model.last_num_intersections = int(total.value)
    return proj, ws, cap, int(total.value)


def _outputs(rgb: Tensor, thermal: Tensor, depth: Tensor, accumulation: Tensor, bgl: List[float], accumulation_thermal: Optional[Tensor] = None) -> Dict[str, Tensor]:
    dev = rgb.device
    out = {"rgb": rgb, "thermal": thermal, "depth": depth, "accumulation": accumulation, "background": torch.tensor(bgl[:3]).to(dev),
           "background_thermal": torch.tensor(bgl[3:], device=dev)}
    if accumulation_thermal is not None:  # separate thermal opacity: the thermal chain's accumulation
        out["accumulation_thermal"] = accumulation_thermal
    return out


def _background_outputs(H: int, W: int, bgl: List[float], dev, sep: bool = False, removal: bool = False) -> Dict[str, Tensor]:
    """Nothing to render (splatfacto.py:759-764): the background, depth 10, no accumulation; removal: the removal renders are the background too."""
    out = _outputs(torch.tensor(bgl[:3]).to(dev).repeat(H, W, 1), torch.full((H, W, 1), bgl[3], device=dev), torch.full((H, W, 1), 10.0, device=dev),
                   torch.zeros((H, W, 1), device=dev), bgl, torch.zeros((H, W, 1), device=dev) if sep else None)
    if removal:
        out["removal"], out["removal_thermal"] = out["rgb"].clone(), out["thermal"].clone()
    return out


class _SplatRender(torch.autograd.Function):
    """project -> bin -> training raster; backward = raster backward -> projection backward.  Inputs after `frame` are the gauss_params in
    _PARAM_NAMES order; outputs: colour before the clamp [H,W,4] (RGB + thermal over the background), accumulation [H,W,1], depth [H,W,1]
    (not differentiable, unless frame["depth_grad"]: then a backward that receives a gradient for it passes the depth groups of the two backward entry points, and one
    that does not leaves them out).  Nine parameters (separate thermal opacity, opacities_thermal last): the thermal group of every entry point, and a fourth output,
    the thermal chain's accumulation [H,W,1].  A frame with a pose row (frame["pose_row"]) passes its optimiser's pose_adjustment [C,6] as one
    more input behind the parameters: the camera is corrected on the device (pose_camera_record), the projection and its backward read that record, and the backward
    also returns dL/d pose_adjustment [C,6], zero outside the frame's row, and leaves dL/d view' [3,4] in `last_view_grad`."""

    @staticmethod
    def forward(ctx, frame, *params):
        row = frame.get("pose_row")
        pose = None
        if row is not None:
            params, pose = params[:-1], params[-1].detach().contiguous()
        ctx.pose, ctx.rec = pose, (pose_camera_record(frame["camera"], frame["cam"], pose, row) if pose is not None else None)
        model, camera = frame["model"], frame["camera"]
        cam, N, H, W = frame["cam"], params[0].shape[0], int(camera.height), int(camera.width)
        aa, bg4, dev = frame["aa"], frame["bg4"], params[0].device
        sep = len(params) == 9
        # a workspace of this frame's own: the backward reads it after other frames may have been rendered
        proj, ws, cap, total = _project_and_bin(model, cam, params, H, W, frame["deg"], aa, max(model._train_cap, 1 << 16), model._new_workspace,
                                                pose_rec=ctx.rec)
        model._train_cap = cap
        # what after_train reads of the training frame (the reference's self.radii / self.last_size); eval renders leave these alone
        model.last_radii, model.last_size = proj["radii"], (H, W)
        ctx.frame, ctx.empty = frame, total == 0
        depth_grad = bool(frame.get("depth_grad"))
        if depth_grad:  # an output the loss never touched arrives as None in the backward: that is how it tells a depth upstream from none
            ctx.set_materialize_grads(False)
        if total == 0:  # nothing on screen: the background, and zero gradients
            rgbt = torch.tensor(list(bg4), device=dev).repeat(H, W, 1)
            alpha = torch.zeros((H, W, 1), device=dev)
            depth = torch.full((H, W, 1), 10.0, device=dev)
            if not depth_grad:
                ctx.mark_non_differentiable(depth)
            ctx.save_for_backward(*params)
            return (rgbt, alpha, depth, torch.zeros((H, W, 1), device=dev)) if sep else (rgbt, alpha, depth)
        image = lambda *c, dtype=torch.float32: torch.empty((H, W) + c, dtype=dtype, device=dev)  # noqa: E731
        rgbt, depth, alpha, final_t, last = image(4), image(1), image(1), image(), image(dtype=torch.int32)
        thermal = (image(1), image(), image(dtype=torch.int32)) if sep else ()  # the thermal chain's accumulation, final transmittance and last index
        splat_calls.raster_train(cam, N, ws, cap, bg4, aa, rgbt, depth, alpha, final_t, last, *thermal)
        if not depth_grad:
            ctx.mark_non_differentiable(depth)
        ctx.ws, ctx.cap, ctx.total = ws, cap, total
        ctx.save_for_backward(*params, proj["radii"], proj["conics"], final_t, last, *thermal[1:], *([depth] if depth_grad else []))
        return (rgbt, alpha, depth) + thermal[:1]

    @staticmethod
    def backward(ctx, v_rgbt, v_alpha, v_depth, v_alpha_th=None):
        frame = ctx.frame
        model = frame["model"]
        P = frame["num_params"]
        params, rest = ctx.saved_tensors[:P], ctx.saved_tensors[P:]
        N, dev = params[0].shape[0], params[0].device
        pose, row = ctx.pose, frame.get("pose_row")
        absgrad = bool(model.config.use_absgrad)  # v_xys_abs of the raster backward: the same gradients plus last_xys_absgrad, the densification statistic
        if ctx.empty:
            model.last_xys_grad = torch.zeros((N, 2), device=dev)
            model.last_xys_absgrad = torch.zeros((N, 2), device=dev) if absgrad else None
            return (None,) + tuple(torch.zeros_like(p) for p in params) + ((torch.zeros_like(pose),) if pose is not None else ())
        radii, conics, final_t, last = rest[:4]
        H, W = final_t.shape
        upstream = lambda v, c: torch.zeros((H, W, c), device=dev) if v is None else v.float().contiguous()  # noqa: E731
        per_gaussian = lambda *c: torch.empty((N,) + c, device=dev)  # noqa: E731
        v_rgbt, v_alpha = upstream(v_rgbt, 4), upstream(v_alpha, 1)
        v_xys, v_xys_abs = per_gaussian(2), (per_gaussian(2) if absgrad else None)
        v_conics, v_colors, v_lnop = per_gaussian(3), per_gaussian(4), per_gaussian()
        th = {}  # separate thermal opacity: the second chain's saved tensors, its upstream gradient and its opacity gradient
        if P == 9:
            th = {"final_t_th": rest[4], "last_th": rest[5], "v_alpha_th": upstream(v_alpha_th, 1), "v_lnop_th": per_gaussian()}
        dz = {}  # a depth upstream (differentiable_depth, and the loss read depth): the forward's depth image, dL / d depth, and dL / d depths [N] to fill
        if v_depth is not None and frame.get("depth_grad"):
            dz = {"aa": frame["aa"], "depth": rest[-1], "v_depth": upstream(v_depth, 1), "v_depths": per_gaussian()}
        splat_calls.raster_backward(frame["cam"], N, ctx.ws, ctx.cap, ctx.total, frame["bg4"], final_t, last, conics, v_rgbt, v_alpha, v_xys, v_conics,
                                    v_colors, v_lnop, v_xys_abs=v_xys_abs, **th, **dz)
        grads = [torch.empty_like(p) for p in params]
        # a pose row: dL/d pose [C,6], zeros but for the frame's row, which the finishing kernel adds into, and dL/d view' [3,4]
        g_pose, dview = (torch.zeros_like(pose), torch.empty((3, 4), device=dev)) if pose is not None else (None, None)
        splat_calls.project_backward(frame["cam"], params, frame["deg"], frame["aa"], radii, v_xys, v_conics, v_colors, v_lnop, grads, th.get("v_lnop_th"),
                                     ctx.rec, pose, row, g_pose, dview, v_depths=dz.get("v_depths"))
        model.last_xys_grad, model.last_xys_absgrad = v_xys, v_xys_abs
        if pose is not None:
            model.last_view_grad = dview
        return (None,) + tuple(grads) + ((g_pose,) if pose is not None else ())


class ThermalSplatfactoModel(nn.Module):
    """RGB + thermal Gaussians: eval render (`get_outputs`) and differentiable training render (`get_train_outputs`).  `gauss_params` keeps the
    reference's names (splatfacto.py:226-235).

    Initialisation (populate_modules, splatfacto.py:190-242).  With `seed_points` = (xyz [M,3], rgb [M,3] uint8, either device) and
    `random_init` False: means = xyz; scales = log(mean distance to the 3 nearest neighbours) on all three axes (knn_distances, then the
    reference's torch ops); quats = a normalised Gaussian draw of the model's seeded CPU generator (uniform on S^3, like random_quat_tensor);
    opacities = logit(0.1); features_dc = RGB2SH(rgb / 255) for sh_degree > 0, or logit(rgb / 255, eps=1e-10) for sh_degree 0 -- evaluated in
    float64 and cast to float32, a deviation from the reference, whose fp32 logit is +inf for a channel value of 255 (float64 gives +-23.03);
    random features_dc when rgb has no rows (the reference's "colors without points"); features_rest zero.  A 2-tuple carries no thermal
    values, so features_dc_thermal and features_rest_thermal start at zero: mid-grey in thermal under both colour modes (this project's rule).
    A 3-tuple (xyz, rgb, thermal [M,1] or [M] uint8: a NeRF point cloud, cloud.py) seeds features_dc_thermal by the colours' rule,
    RGB2SH(thermal / 255) or the float64 logit; features_rest_thermal stays zero.
    Fewer than 4 seed points is a ValueError (the kNN needs 3 neighbours).  Without seeds, or with `random_init`, construction is this model's
    random cube as before, with the constant log-scale log(0.01 * random_scale): the reference would give the random start kNN scales too,
    which this model deliberately does not, to keep that start unchanged."""

    def __init__(self, config: Optional[ThermalSplatfactoModelConfig] = None, num_points: Optional[int] = None, device="cuda", seed: int = 0,
                 num_train_data: int = 0, seed_points: Optional[Tuple[Tensor, ...]] = None, train_is_thermal: Optional[List[bool]] = None):
        super().__init__()
        self.config = config or ThermalSplatfactoModelConfig()
        self.num_train_data = num_train_data
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("ThermalSplatfactoModel needs a HIP device: there is no CPU fallback on this path")
        _lib.load()
        g = torch.Generator().manual_seed(seed)
        dim_sh = (self.config.sh_degree + 1) ** 2
        if seed_points is not None and not self.config.random_init:
            self.gauss_params = self._seeded_params(seed_points, g, dim_sh, dev)
        else:
            n = self.config.num_random if num_points is None else num_points
            # random_init of the reference (splatfacto.py:190-225): positions uniform in a cube, identity-ish colours, opacity logit(0.1)
            means = (torch.rand((n, 3), generator=g) - 0.5) * self.config.random_scale
            self.gauss_params = nn.ParameterDict({
                "means": nn.Parameter(means.to(dev)),
                "scales": nn.Parameter(torch.full((n, 3), math.log(0.01 * self.config.random_scale)).to(dev)),
                "quats": nn.Parameter(torch.nn.functional.normalize(torch.randn((n, 4), generator=g), dim=-1).to(dev)),
                "opacities": nn.Parameter(torch.logit(0.1 * torch.ones(n, 1)).to(dev)),
                "features_dc": nn.Parameter(torch.rand((n, 3), generator=g).to(dev)),
                "features_rest": nn.Parameter(torch.zeros((n, dim_sh - 1, 3), device=dev)),
                "features_dc_thermal": nn.Parameter(torch.rand((n, 1), generator=g).to(dev)),
                "features_rest_thermal": nn.Parameter(torch.zeros((n, dim_sh - 1, 1), device=dev)),
            })
        if self.mcmc and self.gauss_params["means"].shape[0] > self.config.max_gs_num:
            raise ValueError(f'strategy "mcmc": {self.gauss_params["means"].shape[0]} initial Gaussians are above the budget max_gs_num = {self.config.max_gs_num}')
        if self.separate:  # the thermal opacity logits start exactly as the opacities do
            self.gauss_params["opacities_thermal"] = nn.Parameter(torch.logit(0.1 * torch.ones(self.gauss_params["means"].shape[0], 1)).to(dev))
        # pose refinement: one optimiser per spectrum, both sized to all training frames; the other spectrum's rows are non-trainable
        # (`train_is_thermal`, one flag per training frame, names them; without it no row is marked and the routing by camera.is_thermal alone
        # keeps a frame off the other optimiser).  Mode "off" adds no parameter, no state-dict entry and no optimiser group.
        flags = None if train_is_thermal is None else torch.tensor([bool(t) for t in train_is_thermal], dtype=torch.bool)
        if flags is not None and flags.numel() != num_train_data:
            raise ValueError(f"train_is_thermal has {flags.numel()} flags for num_train_data = {num_train_data}")
        self.camera_optimizer = SplatCameraOptimizer(self.config.camera_optimizer, num_train_data, dev, False,
                                                     None if flags is None else flags.nonzero().reshape(-1))
        self.camera_optimizer_thermal = SplatCameraOptimizer(self.config.camera_optimizer_thermal, num_train_data, dev, True,
                                                             None if flags is None else (~flags).nonzero().reshape(-1))
        self.last_view_grad: Optional[Tensor] = None  # dL/d view' [3,4] of the last training frame that read a pose row
        # per-frame bilateral grids, identity at the start.  With `train_is_thermal` each tensor has a row per training frame of its spectrum, in
        # cam_idx order (`_bil_rows`: cam_idx -> row, a host list); without, both have num_train_data rows and the row is cam_idx.  A spectrum
        # without a training frame has no tensor.  Switch off: no parameter, no state-dict entry, no optimiser group.
        self._bil_rows: Optional[List[int]] = None
        if self.config.use_bilateral_grid:
            n_rgb = n_th = num_train_data
            if flags is not None:
                seen = [0, 0]
                self._bil_rows = []
                for t in flags.tolist():
                    self._bil_rows.append(seen[t])
                    seen[t] += 1
                n_rgb, n_th = seen
            if n_rgb > 0:
                self.bil_grids = nn.Parameter(identity_bilateral_grids(n_rgb, 3, self.config.grid_shape, dev))
            if n_th > 0:
                self.bil_grids_thermal = nn.Parameter(identity_bilateral_grids(n_th, 1, self.config.grid_shape, dev))
        # Mip-Splatting's 3D filter: a value per Gaussian (a buffer -- no parameter, in no optimiser group, and not in the state dict: it follows
        # from the means and the cameras), the device table of the cameras it is computed from, and what says that it must be computed again
        self._filter_table: Optional[Tensor] = None
        self._filter_stale = True
        self._filter_epoch = 0  # step // filter_3d_every at the last refresh
        self.filter_refreshes = 0
        if self.config.use_3d_filter:
            self.register_buffer("filter_3D", torch.zeros(self.gauss_params["means"].shape[0], device=dev), persistent=False)
        # pruning by ray contribution (splat_prune.py): the cameras it scores over, and (Gaussians before, removed) of the last prune
        self._prune_cameras: List[PinholeCamera] = []
        self.last_prune_counts: Optional[Tuple[int, int]] = None
        self.step = 0
        self._ws: Optional[Tensor] = None
        self._cap = 0
        self._train_cap = 0  # intersection capacity the training render last needed (each training frame has a workspace of its own)
        self.last_xys_grad: Optional[Tensor] = None
        self.last_xys_absgrad: Optional[Tensor] = None  # use_absgrad: sum over pixels of |the pixel's term of last_xys_grad| [N,2]; else None
        self.last_projection: Dict[str, Tensor] = {}
        self.last_num_intersections = 0
        self.last_radii: Optional[Tensor] = None  # radii [N] and (H, W) of the last TRAINING frame
        self.last_size: Optional[Tuple[int, int]] = None
        # the eval render's crop box (splatfacto.py:374-376): plain attributes, neither parameters nor in the state dict
        self.crop_box: Optional[OrientedBox] = None
        # refinement statistics (after_train); None = the next after_train is the first after a reset
        self.xys_grad_norm: Optional[Tensor] = None
        self.vis_counts: Optional[Tensor] = None
        self.max_2Dsize: Optional[Tensor] = None
        self.noise_generator = torch.Generator(device=dev)  # the split noise (splatfacto.py:541)
        self.noise_generator.manual_seed(seed)
        self.background_generator = torch.Generator().manual_seed(seed)  # background_color "random": host draws, no synchronisation

    def _seeded_params(self, seed_points: Tuple[Tensor, ...], g: torch.Generator, dim_sh: int, dev: torch.device) -> nn.ParameterDict:
        """populate_modules with seed points (splatfacto.py:190-225); the rules are in the class docstring."""
        if len(seed_points) not in (2, 3):
            raise ValueError(f"seed_points must be (xyz, rgb) or (xyz, rgb, thermal), got {len(seed_points)} entries")
        xyz, rgb = seed_points[:2]
        thermal = seed_points[2] if len(seed_points) == 3 else None
        if xyz.dim() != 2 or xyz.shape[1] != 3 or rgb.dim() != 2 or rgb.shape[1] != 3:
            raise ValueError(f"seed_points must be (xyz [M,3], rgb [M,3]), got {tuple(xyz.shape)} and {tuple(rgb.shape)}")
        n = xyz.shape[0]
        if n < 4:
            raise ValueError(f"seed_points: {n} points, the kNN scales need at least 4")
        if rgb.shape[0] not in (0, n):
            raise ValueError(f"seed_points: {rgb.shape[0]} colours for {n} points")
        if thermal is not None:
            if thermal.dim() not in (1, 2) or (thermal.dim() == 2 and thermal.shape[1] != 1):
                raise ValueError(f"seed_points: thermal must be [M,1] or [M], got {tuple(thermal.shape)}")
            if thermal.shape[0] != n:
                raise ValueError(f"seed_points: {thermal.shape[0]} thermal values for {n} points")
        means = xyz.detach().to(device=dev, dtype=torch.float32).contiguous()
        distances = knn_distances(means, 3)
        avg_dist = distances.mean(dim=-1, keepdim=True)
        scales = torch.log(avg_dist.repeat(1, 3))
        quats = torch.nn.functional.normalize(torch.randn((n, 4), generator=g), dim=-1).to(dev)
        if rgb.shape[0] > 0:
            c = rgb.detach().to(device=dev)
            if self.config.sh_degree > 0:
                dc = RGB2SH(c / 255)
            else:
                dc = torch.logit(c.double() / 255, eps=1e-10).float()
        else:
            dc = torch.rand((n, 3), generator=g).to(dev)
        if thermal is not None:
            t = thermal.detach().to(device=dev).reshape(n, 1)
            dc_thermal = RGB2SH(t / 255) if self.config.sh_degree > 0 else torch.logit(t.double() / 255, eps=1e-10).float()
        else:
            dc_thermal = torch.zeros((n, 1), device=dev)
        return nn.ParameterDict({
            "means": nn.Parameter(means),
            "scales": nn.Parameter(scales),
            "quats": nn.Parameter(quats),
            "opacities": nn.Parameter(torch.logit(0.1 * torch.ones(n, 1)).to(dev)),
            "features_dc": nn.Parameter(dc.float().contiguous()),
            "features_rest": nn.Parameter(torch.zeros((n, dim_sh - 1, 3), device=dev)),
            "features_dc_thermal": nn.Parameter(dc_thermal.float().contiguous()),
            "features_rest_thermal": nn.Parameter(torch.zeros((n, dim_sh - 1, 1), device=dev)),
        })

    @property
    def separate(self) -> bool:
        """thermal_opacity_mode == "separate": gauss_params holds opacities_thermal and the entry points take their thermal groups."""
        return self.config.thermal_opacity_mode == "separate"

    @property
    def mcmc(self) -> bool:
        """strategy == "mcmc": the refinement callback relocates and grows, one more callback adds the position noise."""
        return self.config.strategy == "mcmc"

    @property
    def param_names(self) -> Tuple[str, ...]:
        return param_names(self.config.thermal_opacity_mode)

    @property
    def group_params(self) -> Dict[str, str]:
        return GROUP_PARAMS_SEP if self.separate else GROUP_PARAMS

    # the reference's accessors
    @property
    def num_points(self) -> int:
        return self.gauss_params["means"].shape[0]

    @property
    def means(self):
        return self.gauss_params["means"]

    def load_gaussians(self, params: Dict[str, Tensor]) -> None:
        """Replace the Gaussians by `params`.  In separate mode a dict without opacities_thermal starts the thermal logits as a copy of the
        opacities; shared mode has no such entry and refuses it."""
        dev = self.means.device
        if self.separate and "opacities_thermal" not in params:
            params = {**params, "opacities_thermal": params["opacities"].clone()}
        if not self.separate and "opacities_thermal" in params:
            raise ValueError('load_gaussians: opacities_thermal belongs to thermal_opacity_mode "separate"')
        self.gauss_params = nn.ParameterDict({k: nn.Parameter(v.detach().float().contiguous().to(dev)) for k, v in params.items()})
        self._filter_stale = True

    # ------------------------------------------------------------------------------------------------ Mip-Splatting's 3D filter (splat_filter.py)
    def set_filter_cameras(self, cameras) -> None:
        """The cameras the 3D filter is computed from: the full-resolution training cameras of both spectra, uncorrected by any pose optimiser
        (ThermalFullImageDatamanager.train_cameras); None or an empty list takes them away, which switches the filter off.  The table goes to the
        device now, the buffer is recomputed before the next render."""
        cameras = list(cameras) if cameras is not None else []
        self._filter_table = filter_camera_table(cameras, self.means.device).contiguous() if cameras else None
        self._filter_stale = True

    def set_prune_cameras(self, cameras) -> None:
        """The cameras the pruning steps (config.prune_at_steps) score the Gaussians over: the full-resolution training cameras of both spectra
        (ThermalFullImageDatamanager.train_cameras), as `set_filter_cameras` takes them; None or an empty list takes them away."""
        self._prune_cameras = list(cameras) if cameras is not None else []

    def _current_filter(self, training: bool = False) -> Optional[Tensor]:
        """filter_3D [N] as every render of this moment must read it, or None when there is nothing to apply (the switch is off, or no cameras
        are set: the buffer is zero then).  Recomputed (`compute_3d_filter`: two launches, nothing read back) when the cameras were set, when the
        Gaussians were replaced or their number changed, and in training every filter_3d_every steps; a buffer whose row count is not N is never
        handed out."""
        if not self.config.use_3d_filter:
            return None
        N = self.num_points
        if self._filter_table is None:
            if self.filter_3D.shape[0] != N or self._filter_stale:
                self.filter_3D = torch.zeros(N, device=self.means.device)
                self._filter_stale = False
            return None
        epoch = self.step // self.config.filter_3d_every
        if self._filter_stale or self.filter_3D.shape[0] != N or (training and epoch != self._filter_epoch):
            with torch.no_grad():
                self.filter_3D = compute_3d_filter(self.gauss_params["means"].detach().contiguous(), self._filter_table, self.config.filter_3d_near,
                                                   self.config.filter_3d_variance)
            self._filter_stale, self._filter_epoch = False, epoch
            self.filter_refreshes += 1
        return self.filter_3D

    def _render_params(self, training: bool = False) -> List[Tensor]:
        """The gauss_params tensors in param_names order as the projection reads them: with use_3d_filter and cameras the log-scales and the
        opacity logits (both, in separate mode) are the filtered ones (`apply_3d_filter`: one launch, differentiable in the raw parameters)."""
        params = [self.gauss_params[k] for k in self.param_names]
        f = self._current_filter(training)
        if f is not None and self.num_points > 0:
            out = apply_3d_filter(params[1], params[3], f, params[8] if self.separate else None)
            params[1], params[3] = out[0], out[1]
            if self.separate:
                params[8] = out[2]
        return params

    @torch.no_grad()
    def filtered_gaussians(self) -> Dict[str, Tensor]:
        """name -> tensor, detached: the Gaussians every render shows -- gauss_params with the 3D filter fused into scales and opacities (what
        Mip-Splatting's save_fused_ply writes); the raw parameters themselves when the filter is off or has no cameras."""
        return {k: v.detach() for k, v in zip(self.param_names, self._render_params())}

    def _background4(self, training: bool) -> List[float]:
        """The frame's background, RGB + thermal (splatfacto.py:668-682): "white", "random" (training: four uniform draws of the model's own
        generator; eval: the viewer colour and background_thermal) or black."""
        cfg = self.config
        if cfg.background_color == "random":
            if training:
                return torch.rand(4, generator=self.background_generator).tolist()
            return [*VIEWER_BACKGROUND, float(cfg.background_thermal)]
        v = 1.0 if cfg.background_color == "white" else 0.0
        return [v, v, v, float(cfg.background_thermal)]

    def _new_workspace(self, n: int, cap: int, tiles: int) -> Tensor:
        return torch.empty(splat_calls.frame_workspace_bytes(n, cap, tiles), dtype=torch.uint8, device=self.means.device)

    def _workspace(self, n: int, cap: int, tiles: int) -> Tensor:
        """The eval render's workspace, kept between frames (`_ws`, for `_cap` pairs) while it is large enough."""
        need = splat_calls.frame_workspace_bytes(n, cap, tiles)
        if self._ws is None or self._ws.numel() < need or self._cap != cap:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.means.device)
            self._cap = cap
        return self._ws

    def _frame_settings(self) -> Tuple[int, int]:
        """(antialiased flag, SH degree at this step) of a frame rendered now (splatfacto.py:772; sh_degree == 0 -> -1: sigmoid of the DC
        term, :776-777)."""
        cfg = self.config
        if cfg.rasterize_mode not in ("classic", "antialiased"):
            raise ValueError(f"Unknown rasterize_mode: {cfg.rasterize_mode}")
        return int(cfg.rasterize_mode == "antialiased"), min(self.step // cfg.sh_degree_interval, cfg.sh_degree) if cfg.sh_degree > 0 else -1

    def set_crop(self, crop_box: Optional[OrientedBox]) -> None:
        """splatfacto.py:374-376: the box `get_outputs` crops to from now on; None clears it.  The box is read anew by every cropped frame (its
        world -> box matrix is inverted on the host, a few dozen float operations), so a box changed afterwards, in place or not, is seen; a
        singular R is the ValueError of that frame, raised before any launch."""
        if crop_box is not None and not isinstance(crop_box, OrientedBox):
            raise TypeError(f"set_crop: an OrientedBox or None expected, got {type(crop_box).__name__}")
        self.crop_box = crop_box

    def _crop(self) -> Optional[_lib.TnSplatCrop]:
        """The C struct of `crop_box` as it is now (also when the attribute was assigned without set_crop, as the reference's viewer does)."""
        return None if self.crop_box is None else self.crop_box.crop_struct()

    def get_outputs_for_camera(self, camera: PinholeCamera, obb_box: Optional[OrientedBox] = None) -> Dict[str, Tensor]:
        """splatfacto.py:904-915: the eval render cropped to `obb_box`; as in the reference, None clears an earlier crop."""
        self.set_crop(obb_box)
        return self.get_outputs(camera)

    @torch.no_grad()
    def get_outputs(self, camera: PinholeCamera) -> Dict[str, Tensor]:
        """splatfacto.py:659-822 (eval mode): project -> SH colours -> tile binning -> raster (colour + depth in one pass).
        Returns rgb [H,W,3], thermal [H,W,1], depth [H,W,1], accumulation [H,W,1], background [3], background_thermal [1]; in separate mode also
        accumulation_thermal [H,W,1], the thermal chain's accumulation (accumulation is the RGB chain's); with removal_min_opacity_diff set also
        removal [H,W,3] and removal_thermal [H,W,1], from one more launch over the frame's tile lists.  With `crop_box` set the projection is the
        crop instantiation: every output is that of the Gaussians strictly inside the box alone, `last_projection` holds radius 0 for the others, and
        a box that keeps nothing gives the background (splatfacto.py:690-698, 759-764)."""
        dev = self.means.device
        thr = self.config.removal_min_opacity_diff
        N, H, W = self.num_points, int(camera.height), int(camera.width)
        aa, deg = self._frame_settings()
        bgl = self._background4(training=False)
        if N == 0:  # every Gaussian culled: the background (splatfacto.py:759-764); last_projection stays what it was
            return _background_outputs(H, W, bgl, dev, self.separate, thr is not None)
        cam = camera_struct(camera)
        params = self._render_params()
        pose, row = self._pose_row(camera, training=False)  # a shared row corrects eval renders of its spectrum too; per-frame rows never do
        rec = pose_camera_record(camera, cam, pose.detach(), row) if row is not None else None
        _, ws, cap, total = _project_and_bin(self, cam, params, H, W, deg, aa, max(self._cap, 1 << 16), self._workspace, self._crop(), rec)
        if total == 0:  # nothing on screen
            return _background_outputs(H, W, bgl, dev, self.separate, thr is not None)
        rgbt = torch.empty((H, W, 4), device=dev)
        depth = torch.empty((H, W, 1), device=dev)
        alpha = torch.empty((H, W, 1), device=dev)
        alpha_th = torch.empty((H, W, 1), device=dev) if self.separate else None  # the thermal chain's accumulation
        bg4 = (C.c_float * 4)(*bgl)
        splat_calls.raster(cam, N, ws, cap, bg4, aa, rgbt, depth, alpha, alpha_th)
        out = _outputs(rgbt[..., :3], rgbt[..., 3:], depth, alpha, bgl, alpha_th)
        if thr is not None:  # the removal renders (separate mode): one more walk over the same lists
            rem = torch.empty((H, W, 4), device=dev)
            splat_calls.raster_removal(cam, N, ws, cap, bg4, thr, rem)
            out["removal"], out["removal_thermal"] = rem[..., :3], rem[..., 3:]
        return out

    def _pose_row(self, camera: PinholeCamera, training: bool) -> Tuple[Optional[Tensor], Optional[int]]:
        """(pose_adjustment, row) the frame of `camera` reads -- its spectrum's optimiser, at most one row of one tensor -- or (None, None)."""
        opt = self.camera_optimizer_thermal if camera.is_thermal else self.camera_optimizer
        row = opt.row(camera, training)
        return (opt.pose_adjustment, row) if row is not None else (None, None)

    def _bilateral_grid(self, camera: PinholeCamera) -> Tuple[Optional[Tensor], Optional[int]]:
        """(grids, row) that correct the training render of `camera` -- its spectrum's tensor and, on the host, the frame's row -- or (None, None):
        the switch is off, or the camera has no cam_idx."""
        idx = camera.cam_idx
        if not self.config.use_bilateral_grid or idx is None:
            return None, None
        grids = getattr(self, "bil_grids_thermal" if camera.is_thermal else "bil_grids", None)
        if not 0 <= int(idx) < self.num_train_data or grids is None:
            raise ValueError(f"camera.cam_idx = {idx} (is_thermal = {bool(camera.is_thermal)}): the model has no bilateral grid for that training frame")
        row = int(idx) if self._bil_rows is None else self._bil_rows[int(idx)]
        return grids, row

    def _get_downscale_factor(self) -> int:
        """splatfacto.py:639-646: the resolution schedule's factor at this step while the module is in training mode, else 1."""
        return downscale_factor(self.step, self.config.num_downscales, self.config.resolution_schedule, self.training)

    def get_train_outputs(self, camera: PinholeCamera) -> Dict[str, Tensor]:
        """The render of get_outputs as a differentiable function of every gauss_params tensor (splatfacto.py:659-822 in training: `crop_box`
        is not read, the reference crops only outside training).  rgb [H,W,3], thermal [H,W,1] and accumulation [H,W,1] carry gradients; depth [H,W,1] is
        detached, or with config.differentiable_depth carries them too (where accumulation > 0; the fill value elsewhere takes none).  With a fixed
        background the values equal get_outputs' bit for bit; background_color "random" draws this frame's RGB + thermal background from the
        model's generator (background [3], background_thermal [1]).  After backward(), `last_xys_grad` [N,2] holds dL/d xys per Gaussian
        (and, with config.use_absgrad, `last_xys_absgrad` [N,2] the sum of its per-pixel terms' absolute values).
        Under the resolution schedule the frame is that of `rescaled_camera(camera, d)` (splatfacto.py:699-700): its size is what `last_size`,
        `last_radii`, `last_xys_grad` and the refinement statistics refer to; `camera` is not modified.  With config.use_bilateral_grid and a
        camera.cam_idx the frame's bilateral grid corrects the render of the camera's spectrum after the clamp (rgb by bil_grids[row] on an RGB
        frame, thermal by bil_grids_thermal[row] on a thermal one; `bilateral_slice`): that output then also carries gradients to the grid, it is
        not clamped again, and the other spectrum's render passes through as it is.  `get_outputs` never applies a grid."""
        d = self._get_downscale_factor()
        if d > 1:
            camera = rescaled_camera(camera, d)
        aa, deg = self._frame_settings()
        bgl = self._background4(training=True)
        names = self.param_names
        frame = {"model": self, "camera": camera, "cam": camera_struct(camera), "aa": aa, "deg": deg, "bg4": (C.c_float * 4)(*bgl), "num_params": len(names)}
        if self.config.differentiable_depth:
            if aa:  # (the config refuses the combination; a rasterize_mode assigned afterwards must not reach the kernels)
                raise ValueError('differentiable_depth needs rasterize_mode "classic"')
            frame["depth_grad"] = True
        self.last_xys_grad = None
        self.last_xys_absgrad = None
        pose, row = self._pose_row(camera, training=True)
        if row is not None:  # the frame's pose row: one more differentiable input
            frame["pose_row"] = row
        rgbt, alpha, depth, *alpha_th = _SplatRender.apply(frame, *self._render_params(training=True), *([pose] if row is not None else []))
        alpha_th = alpha_th[0] if alpha_th else None  # separate mode: the thermal chain's accumulation (differentiable)
        if self.last_num_intersections == 0:  # the background as get_outputs returns it (no clamp)
            rgb, thermal = rgbt[..., :3], rgbt[..., 3:]
        else:
            rgb, thermal = torch.clamp(rgbt[..., :3], max=1.0), torch.clamp(rgbt[..., 3:], max=1.0)
        grids, row = self._bilateral_grid(camera)
        if grids is not None:  # the frame's colour correction, on its own spectrum; the result is not clamped again
            if camera.is_thermal:
                thermal = bilateral_slice(grids, row, thermal)
            else:
                rgb = bilateral_slice(grids, row, rgb)
        return _outputs(rgb, thermal, depth, alpha, bgl, alpha_th)

    # ------------------------------------------------------------------------------------------------ loss and metrics (splatfacto.py:824-934)
    def get_gt_img(self, image: Tensor) -> Tensor:
        """splatfacto.py:824-834: uint8 -> [0, 1] float, on the model's device; under the resolution schedule (d > 1) shrunk to
        (H // d, W // d) by one resize_image call, uint8 going straight into the kernel."""
        d = self._get_downscale_factor()
        if d > 1:
            image = image.to(self.means.device)
            if image.dtype != torch.uint8:
                image = image.float()
            return resize_image(image, (image.shape[0] // d, image.shape[1] // d))
        if image.dtype == torch.uint8:
            image = image.float() / 255.0
        return image.to(self.means.device)

    def composite_with_background(self, image: Tensor, background: Tensor) -> Tensor:
        """splatfacto.py:836-846: an [H,W,4] image (alpha last) over the frame's background -- background [3] for an RGB frame, [1] (the
        thermal background) for a thermal one; other images pass through."""
        if image.shape[2] == 4:
            alpha = image[..., -1].unsqueeze(-1).repeat((1, 1, 3))
            return alpha * image[..., :3] + (1 - alpha) * background
        return image

    def _frame_pred_gt(self, outputs: Dict[str, Tensor], batch, resize_pred: bool = False) -> Tuple[bool, Tensor, Tensor]:
        """(is thermal, prediction, ground truth) of the frame's spectrum: RGB [H,W,3] against image[..., :3], or thermal [H,W,1] against
        image[..., 0:1] (model.rgb_to_rgbt_image), the ground truth -- at the resolution schedule's size -- composited over the frame's
        background.  A prediction of another size (a full-size eval render scored in training mode while the schedule's factor is above 1) is a
        ValueError, or with `resize_pred` is resized to the ground truth's size (splatfacto.py:931-938)."""
        th = _is_thermal_frame(batch)
        bg = outputs["background_thermal"] if th else outputs["background"]
        gt = self.composite_with_background(self.get_gt_img(batch["image"]), bg)
        pred, gt = (outputs["thermal"], gt[..., 0:1]) if th else (outputs["rgb"], gt[..., :3])
        d = self._get_downscale_factor()
        if resize_pred and d > 1 and pred.shape[:2] != gt.shape[:2]:
            pred = resize_image(pred, gt.shape[:2])
        if pred.shape[:2] != gt.shape[:2]:
            raise ValueError(f"the prediction is {pred.shape[0]} x {pred.shape[1]}, the ground truth {gt.shape[0]} x {gt.shape[1]} at the resolution "
                             f"schedule's downscale factor {d} (step {self.step}): score training renders (get_train_outputs), or call eval() first")
        return th, pred, gt

    def get_loss_dict(self, outputs: Dict[str, Tensor], batch, metrics_dict=None) -> Dict[str, Tensor]:
        """splatfacto.py:863-903 on the frame's spectrum: main_loss = (1 - ssim_lambda) * L1 + ssim_lambda * (1 - SSIM) (one tn_image_loss call,
        times thermal_loss_mult on a thermal frame) and scale_reg (every 10th step when use_scale_regularization, else 0).  With
        tv_pixel_loss_mult / cross_channel_loss_mult above 0 also tv_pixel_loss / cross_channel_loss (the NeRF model's keys,
        models/thermal_nerfacto.py:346-354): on an RGB frame ThermalNeRF's regularisers of outputs["thermal"] against the main loss's ground truth
        (one tn_thermal_reg call), on a thermal frame 0 -- the reference keeps both to the RGB rays, and the keys depend on the config alone.
        In separate mode with opacity_loss_mult > 0 also density_loss = opacity_loss_mult * (mean|s(o_th) - s(o).detach()| + rgb_opacity_loss_mult *
        mean|s(o) - s(o_th).detach()|), s = sigmoid (plain torch on [N,1]).  Under strategy "mcmc" also mcmc_opacity_reg = mcmc_opacity_reg *
        mean(s(o)) (+ mean(s(o_th)) in separate mode) and mcmc_scale_reg = mcmc_scale_reg * mean(exp(scales)) (plain torch).  With depth_loss_mult /
        depth_tv_loss_mult above 0 also depth_loss / depth_tv_loss of outputs["depth"] over its covered pixels (one tn_depth_loss call), on RGB and thermal
        frames alike; depth_loss is 0 for a batch without `depth_image`, and the keys depend on the config alone.  With use_bilateral_grid also tv_loss
        (splatfacto's key) = bilateral_grid_tv_mult * (tv(bil_grids) + tv(bil_grids_thermal)), `bilateral_grid_tv`.  `batch`: image [H,W,3|4], is_thermal,
        optionally depth_image [H,W,1] float32 in scene units (full size: under the resolution schedule it is taken as depth_image[::d, ::d], cut to the
        frame -- depth is not interpolated)."""
        if "mask" in batch:
            raise NotImplementedError("masks are not supported by the splat loss (DESIGN.md section 7)")
        cfg = self.config
        th, pred, gt = self._frame_pred_gt(outputs, batch)
        main, _, _ = image_loss(pred, gt.float(), cfg.ssim_lambda, cfg.thermal_loss_mult if th else 1.0)
        dev = self.means.device
        if cfg.use_scale_regularization and self.step % 10 == 0:
            scale_exp = torch.exp(self.gauss_params["scales"])
            scale_reg = torch.maximum(scale_exp.amax(dim=-1) / scale_exp.amin(dim=-1), torch.tensor(cfg.max_gauss_ratio, device=dev)) - cfg.max_gauss_ratio
            scale_reg = 0.1 * scale_reg.mean()
        else:
            scale_reg = torch.tensor(0.0).to(dev)
        losses = {"main_loss": main, "scale_reg": scale_reg}
        tv_mult, cross_mult = cfg.tv_pixel_loss_mult, cfg.cross_channel_loss_mult
        if tv_mult > 0 or cross_mult > 0:
            if th:
                tv = cross = torch.tensor(0.0).to(dev)
            else:
                tv, cross = thermal_regularizers(outputs["thermal"], gt.float(), tv_mult, cross_mult)
            if tv_mult > 0:
                losses["tv_pixel_loss"] = tv
            if cross_mult > 0:
                losses["cross_channel_loss"] = cross
        if cfg.depth_loss_mult > 0 or cfg.depth_tv_loss_mult > 0:
            depth = outputs["depth"]
            sensor = batch.get("depth_image") if cfg.depth_loss_mult > 0 else None
            if sensor is not None:
                sensor = sensor.to(dev).float()
                if sensor.shape[:2] != depth.shape[:2]:  # the resolution schedule: every d-th pixel, never an interpolated depth
                    d = self._get_downscale_factor()
                    sensor = sensor[::d, ::d][:depth.shape[0], :depth.shape[1]]
                if sensor.shape != depth.shape:
                    raise ValueError(f"depth_image is {tuple(batch['depth_image'].shape)}, the depth render {tuple(depth.shape)} (downscale factor "
                                     f"{self._get_downscale_factor()})")
            d_loss, d_tv = depth_losses(depth, outputs["accumulation"], sensor, cfg.depth_loss_mult, cfg.depth_tv_loss_mult)
            if cfg.depth_loss_mult > 0:
                losses["depth_loss"] = d_loss
            if cfg.depth_tv_loss_mult > 0:
                losses["depth_tv_loss"] = d_tv
        if self.separate and cfg.opacity_loss_mult > 0:
            losses["density_loss"] = opacity_density_loss(self.gauss_params["opacities"], self.gauss_params["opacities_thermal"], cfg.opacity_loss_mult,
                                                          cfg.rgb_opacity_loss_mult)
        if self.mcmc:  # gsplat's MCMC regularisers: few and small Gaussians (elementwise on [N,1] and [N,3], plain torch)
            o_mean = torch.sigmoid(self.gauss_params["opacities"]).mean()
            if self.separate:
                o_mean = o_mean + torch.sigmoid(self.gauss_params["opacities_thermal"]).mean()
            losses["mcmc_opacity_reg"] = cfg.mcmc_opacity_reg * o_mean
            losses["mcmc_scale_reg"] = cfg.mcmc_scale_reg * torch.exp(self.gauss_params["scales"]).mean()
        if cfg.use_bilateral_grid:  # the grids' total variation, over every frame's grid of both spectra (tn_bilagrid_tv)
            tv_loss = torch.zeros((), device=dev)
            for name in ("bil_grids", "bil_grids_thermal"):
                if hasattr(self, name):
                    tv_loss = tv_loss + bilateral_grid_tv(getattr(self, name), cfg.bilateral_grid_tv_mult)
            losses["tv_loss"] = tv_loss
        self.camera_optimizer.get_loss_dict(losses)  # camera_opt_regularizer / _thermal (tn_camera_reg), only when the mode is on
        self.camera_optimizer_thermal.get_loss_dict(losses)
        return losses

    @torch.no_grad()
    def get_metrics_dict(self, outputs: Dict[str, Tensor], batch) -> Dict[str, Tensor]:
        """splatfacto.py:848-861 on the frame's spectrum: psnr (data range 1, a device scalar) and gaussian_count."""
        _, pred, gt = self._frame_pred_gt(outputs, batch)
        metrics = {"psnr": _psnr(pred, gt), "gaussian_count": self.num_points}
        self.camera_optimizer.get_metrics_dict(metrics)  # camera_opt_translation / camera_opt_rotation (+ _thermal), only when the mode is on
        self.camera_optimizer_thermal.get_metrics_dict(metrics)
        return metrics

    @torch.no_grad()
    def get_image_metrics_and_images(self, outputs: Dict[str, Tensor], batch) -> Tuple[Dict[str, float], Dict[str, Tensor]]:
        """splatfacto.py:917-934 with ThermalNerfactoModel's keys: psnr_rgb / ssim_rgb or psnr_thermal / ssim_thermal of the frame's spectrum
        (SSIM = the loss's, tn_image_loss), and the ground truth beside both renders; `removal` / `removal_thermal` join the images when the
        outputs hold them.  Scored in training mode under the resolution schedule
        (factor above 1), full-size renders are resized to the ground truth's size, as the reference does (:931-938).  LPIPS is left out, as
        elsewhere in this project."""
        th, pred, gt = self._frame_pred_gt(outputs, batch, resize_pred=True)
        key = "thermal" if th else "rgb"
        metrics = {f"psnr_{key}": float(_psnr(pred, gt)), f"ssim_{key}": float(ssim(pred, gt.float()))}
        gt3 = gt.expand(-1, -1, 3) if th else gt
        rgb, thermal = outputs["rgb"], outputs["thermal"]
        if rgb.shape[:2] != gt.shape[:2]:  # full-size renders under the schedule: shown, like the scored one, at the ground truth's size
            rgb, thermal = resize_image(rgb, gt.shape[:2]), resize_image(thermal, gt.shape[:2])
        images = {"img": torch.cat([gt3, rgb, thermal.expand(-1, -1, 3)], dim=1), "accumulation": outputs["accumulation"],
                  "depth": outputs["depth"]}
        for k in ("removal", "removal_thermal"):  # the removal renders, at the ground truth's size like rgb and thermal
            if k in outputs:
                images[k] = outputs[k] if outputs[k].shape[:2] == gt.shape[:2] else resize_image(outputs[k], gt.shape[:2])
        return metrics, images

    # ------------------------------------------------------------------------------------------------ training (splatfacto.py:258-628)
    def step_cb(self, step: int) -> None:
        self.step = step

    def get_gaussian_param_groups(self) -> Dict[str, List[nn.Parameter]]:
        """splatfacto.py:620-628: the reference's six groups plus the thermal SH coefficients (and, in separate mode, opacities_thermal)."""
        return {g: [self.gauss_params[k]] for g, k in self.group_params.items()}

    def get_param_groups(self) -> Dict[str, List[nn.Parameter]]:
        """The Gaussian groups, for each pose optimiser that is on camera_opt / camera_opt_thermal (optim.SPLAT_CAMERA_OPTIMIZERS), and with
        use_bilateral_grid bilateral_grid / bilateral_grid_thermal (optim.SPLAT_BILAGRID_OPTIMIZERS)."""
        groups = self.get_gaussian_param_groups()
        self.camera_optimizer.get_param_groups(groups)
        self.camera_optimizer_thermal.get_param_groups(groups)
        for group, name in (("bilateral_grid", "bil_grids"), ("bilateral_grid_thermal", "bil_grids_thermal")):
            if hasattr(self, name):
                groups[group] = [getattr(self, name)]
        return groups

    def get_training_callbacks(self, training_callback_attributes) -> List["TrainingCallback"]:
        """splatfacto.py:595-617.  `training_callback_attributes` carries the `Optimizers` as `.optimizers` (or is the `Optimizers`); the
        refinement callback reaches them through a closure.  Strategy "mcmc": the same three (after_train does nothing, the refinement callback
        relocates and grows) and a fourth that adds the position noise after every iteration."""
        from .model import TrainingCallback, TrainingCallbackLocation

        opts = training_callback_attributes
        if not isinstance(getattr(opts, "optimizers", None), dict):
            opts = opts.optimizers
        after = [TrainingCallbackLocation.AFTER_TRAIN_ITERATION]
        cbs = [TrainingCallback([TrainingCallbackLocation.BEFORE_TRAIN_ITERATION], self.step_cb), TrainingCallback(after, self.after_train),
               TrainingCallback(after, lambda step: self.refinement_after(opts, step), update_every_num_iters=self.config.refine_every)]
        if self.mcmc:  # the position noise: every step, after the optimiser step and after the refinement of a refine step
            cbs.append(TrainingCallback(after, lambda step: self.mcmc_noise_after(opts, step)))
        return cbs

    def load_state_dict(self, state_dict, strict: bool = True, **kwargs):
        """splatfacto.py:258-271: resize the Gaussians to the checkpoint's count, then load (and, as the reference, step = 30000: every SH degree on)."""
        self.step = 30000
        n = state_dict["gauss_params.means"].shape[0]
        dev = self.means.device
        self.gauss_params = nn.ParameterDict({k: nn.Parameter(torch.zeros((n,) + tuple(self.gauss_params[k].shape[1:]), device=dev)) for k in self.param_names})
        self.xys_grad_norm = self.vis_counts = self.max_2Dsize = None
        self._filter_stale = True
        return super().load_state_dict(state_dict, strict=strict, **kwargs)

    def _refine_struct(self) -> _lib.TnSplatRefine:
        cfg = self.config
        r = _lib.TnSplatRefine()
        r.cull_alpha_thresh, r.cull_scale_thresh = cfg.cull_alpha_thresh, cfg.cull_scale_thresh
        r.densify_grad_thresh, r.densify_size_thresh = cfg.densify_grad_thresh, cfg.densify_size_thresh
        r.cull_screen_size, r.split_screen_size = cfg.cull_screen_size, cfg.split_screen_size
        r.refine_every, r.reset_alpha_every = cfg.refine_every, cfg.reset_alpha_every
        r.stop_screen_size_at, r.stop_split_at = cfg.stop_screen_size_at, cfg.stop_split_at
        r.n_split_samples, r.continue_cull_post_densification = cfg.n_split_samples, int(cfg.continue_cull_post_densification)
        r.num_train_data = self.num_train_data
        r.max_size = max(self.last_size) if self.last_size else 1
        return r

    @torch.no_grad()
    def after_train(self, step: int) -> None:
        """splatfacto.py:346-372 on the last training frame (its radii, size and, after backward(), last_xys_grad): tn_splat_grad_stats.
        With config.use_absgrad the statistic accumulated is the norm of last_xys_absgrad instead."""
        assert step == self.step
        if self.mcmc or self.step >= self.config.stop_split_at:  # the MCMC strategy keeps no gradient statistics
            return
        xys_grad = self.last_xys_absgrad if self.config.use_absgrad else self.last_xys_grad
        if xys_grad is None or self.last_radii is None or self.last_size is None:
            raise RuntimeError("after_train needs a get_train_outputs() frame and its backward()")
        N, dev = self.num_points, self.means.device
        if self.last_radii.shape[0] != N or xys_grad.shape[0] != N:
            raise RuntimeError("after_train: the Gaussians changed since the last training frame")
        first = self.xys_grad_norm is None
        if first:
            self.xys_grad_norm = torch.empty(N, device=dev)
            self.vis_counts = torch.empty(N, device=dev)
            self.max_2Dsize = torch.empty(N, device=dev)
        splat_calls.grad_stats(xys_grad.contiguous(), self.last_radii, N, max(self.last_size), first, self.xys_grad_norm, self.vis_counts, self.max_2Dsize)

    @torch.no_grad()
    def refinement_after(self, optimizers, step: int) -> None:
        """splatfacto.py:381-498: densify (split + duplicate) and cull, or cull only after stop_split_at; then the opacity reset and a reset of
        the statistics.  `optimizers`: an `Optimizers` (or a dict group -> torch.optim optimiser, or None); every optimiser's parameter is
        replaced by the model's new one, surviving Gaussians keep their Adam moments, new ones start at zero, step counts are kept.
        Strategy "mcmc": when warmup_length < step < stop_split_at and step % refine_every == 0, relocate the dead Gaussians and grow towards
        max_gs_num (`_mcmc_refine`); nothing else.  After that, at a step of config.prune_at_steps, the Gaussians are scored by their ray
        contribution over the cameras of `set_prune_cameras` and those below config.prune_min_contribution are removed through the same
        optimisers (splat_prune.py); `last_prune_counts` = (Gaussians before, removed)."""
        assert step == self.step
        self._refinement_step(optimizers)
        if self.step in self.config.prune_at_steps:
            self._prune_step(optimizers)

    def _prune_step(self, optimizers) -> None:
        """One pruning step: score_gaussians over the prune cameras, RadSplat's threshold, prune_gaussians."""
        from . import splat_prune

        if not self._prune_cameras:
            raise RuntimeError(f"step {self.step} is in prune_at_steps but the model has no cameras to score over: call set_prune_cameras(train cameras) first")
        before = self.num_points
        scores = splat_prune.score_gaussians(self, self._prune_cameras)
        keep = splat_prune.prune_mask(scores, min_contribution=self.config.prune_min_contribution)
        self.last_prune_counts = (before, splat_prune.prune_gaussians(self, keep, optimizers))

    def _refinement_step(self, optimizers) -> None:
        """The refinement proper of `refinement_after`."""
        cfg = self.config
        if self.step <= cfg.warmup_length:
            return
        opts = getattr(optimizers, "optimizers", optimizers) or {}
        if self.mcmc:  # relocate the dead, grow to the budget: no cull, no opacity reset, no statistics
            if self.step < cfg.stop_split_at and self.step % cfg.refine_every == 0:
                self._mcmc_refine(optimizers, opts)
            return
        reset_interval = cfg.reset_alpha_every * cfg.refine_every
        densify = self.step < cfg.stop_split_at and self.step % reset_interval > self.num_train_data + cfg.refine_every
        if densify or (self.step >= cfg.stop_split_at and cfg.continue_cull_post_densification):
            if densify and self.xys_grad_norm is None:
                raise RuntimeError("refinement_after: densification needs after_train statistics")
            self._refine(optimizers, opts, densify)
        if self.step < cfg.stop_split_at and self.step % reset_interval == cfg.refine_every:
            reset_value = cfg.cull_alpha_thresh * 2.0
            for group, key in (("opacity", "opacities"), ("opacities_thermal", "opacities_thermal"))[:2 if self.separate else 1]:
                op = self.gauss_params[key]
                op.data = torch.clamp(op.data, max=torch.logit(torch.tensor(reset_value, device=op.device)).item())
                o = opts.get(group)
                if o is not None and o.state.get(op):
                    st = o.state[op]
                    st["exp_avg"] = torch.zeros_like(st["exp_avg"])
                    st["exp_avg_sq"] = torch.zeros_like(st["exp_avg_sq"])
        self.xys_grad_norm = self.vis_counts = self.max_2Dsize = None

    def _refine(self, optimizers, opts, densify: bool) -> None:
        """One tn_splat_refine_plan (one host sync: the counts) + one tn_splat_refine_apply into freshly allocated tensors."""
        gp = self.gauss_params
        N, dev = self.num_points, self.means.device
        S, K = self.config.n_split_samples, gp["features_rest"].shape[1]
        rs = self._refine_struct()
        stats = [self.xys_grad_norm, self.vis_counts, self.max_2Dsize]
        if stats[0] is None:  # cull only, straight after a reset: no screen sizes recorded
            stats = [torch.ones(N, device=dev), torch.ones(N, device=dev), torch.zeros(N, device=dev)]
        counts = (C.c_int64 * 4)()
        names = self.param_names
        ws = splat_calls.refine_plan(rs, self.step, gp["scales"], gp["opacities"], stats, N, S, counts, gp["opacities_thermal"] if self.separate else None)
        n_split, n_orig, n_child, n_dup = (int(c) for c in counts)
        # the reference's noise: randn((n_split_samples * n_split, 3)), sample-major (splatfacto.py:541)
        noise = torch.randn((S * n_split, 3), device=dev, generator=self.noise_generator) if densify else None
        self.last_refine_counts = (n_split, n_orig, n_child, n_dup)
        if n_orig == N and n_child == 0 and n_dup == 0:
            return  # nothing split, duplicated or culled: every tensor stays as it is
        M = n_orig + n_child + n_dup
        moments = self._adam_moments(opts)
        new = {k: torch.empty((M,) + tuple(gp[k].shape[1:]), device=dev) for k in names}
        new_m = {k: (torch.empty_like(new[k]), torch.empty_like(new[k])) for k in moments}
        column = lambda d, i: [d[k][i] if k in d else None for k in names]  # noqa: E731
        splat_calls.refine_apply(rs, N, K, ws, counts, noise, [gp[k].detach() for k in names], column(moments, 0), column(moments, 1),
                                 [new[k] for k in names], column(new_m, 0), column(new_m, 1))
        self._swap_params(optimizers, opts, new, new_m)

    def _swap_params(self, optimizers, opts, new: Dict[str, Tensor], new_moments: Dict[str, Tuple[Tensor, Tensor]]) -> None:
        """dup_in_optim / remove_from_optim (splatfacto.py:292-344): `new` replaces gauss_params, and every optimiser is handed its group's new
        parameter -- param_groups and `optimizers.parameters` point at it, the old parameter's state moves to it with `new_moments[k]` (exp_avg,
        exp_avg_sq) installed where given; step counts and every other state key are kept."""
        old = {k: self.gauss_params[k] for k in self.param_names}
        self.gauss_params = nn.ParameterDict({k: nn.Parameter(new[k]) for k in self.param_names})
        self._filter_stale = True  # other Gaussians: the 3D filter's buffer is recomputed before the next render
        for g, k in self.group_params.items():
            o = opts.get(g)
            if o is None:
                continue
            st = o.state.pop(old[k], None)
            p = self.gauss_params[k]
            o.param_groups[0]["params"] = [p]
            if st is not None:
                if k in new_moments:
                    st["exp_avg"], st["exp_avg_sq"] = new_moments[k]
                o.state[p] = st
            if isinstance(getattr(optimizers, "parameters", None), dict) and g in optimizers.parameters:
                optimizers.parameters[g] = [p]

    # ------------------------------------------------------------------------------------------------ MCMC strategy (gsplat's MCMCStrategy)
    def _visible_opacity(self) -> Tensor:
        """o_vis [N]: sigmoid(opacities), in separate mode the larger of the two sigmoids -- the cull's "visible in either spectrum" rule."""
        o = torch.sigmoid(self.gauss_params["opacities"].detach()).reshape(-1)
        if self.separate:
            o = torch.maximum(o, torch.sigmoid(self.gauss_params["opacities_thermal"].detach()).reshape(-1))
        return o

    def _adam_moments(self, opts) -> Dict[str, Tuple[Tensor, Tensor]]:
        """gauss_params entry -> (exp_avg, exp_avg_sq) of its optimiser, contiguous and the state's own tensors (written in place); entries
        without Adam state are left out."""
        group_of = {v: g for g, v in self.group_params.items()}
        moments = {}
        for k in self.param_names:
            o = opts.get(group_of[k])
            st = o.state.get(self.gauss_params[k]) if o is not None else None
            if st and "exp_avg" in st:
                st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].contiguous(), st["exp_avg_sq"].contiguous()
                moments[k] = (st["exp_avg"], st["exp_avg_sq"])
        return moments

    def _mcmc_grow(self, optimizers, opts, n_add: int) -> None:
        """Append n_add zero rows to every parameter and both moments, and hand the new parameters to the optimisers as `_refine` does: existing
        rows keep their values, moments and step counts."""
        grown = lambda t: torch.cat([t.detach(), torch.zeros((n_add,) + tuple(t.shape[1:]), device=t.device)], dim=0)  # noqa: E731
        self._swap_params(optimizers, opts, {k: grown(self.gauss_params[k]) for k in self.param_names},
                          {k: (grown(m), grown(v)) for k, (m, v) in self._adam_moments(opts).items()})

    def _mcmc_refine(self, optimizers, opts) -> None:
        """One MCMC refinement: relocate the dead Gaussians onto live ones, then grow towards the budget (each: one torch.multinomial draw of the
        model's noise_generator on the device and one tn_splat_mcmc_relocate call).  One host synchronisation: the number of dead Gaussians."""
        cfg = self.config
        N = self.num_points
        n_dead = n_relocated = 0
        if N > 0:
            o_vis = self._visible_opacity()
            dead = o_vis <= cfg.mcmc_min_opacity
            dst = dead.nonzero().reshape(-1)
            n_dead = int(dst.numel())
            if 0 < n_dead < N:
                alive = (~dead).nonzero().reshape(-1)
                src = alive[torch.multinomial(o_vis[alive], n_dead, replacement=True, generator=self.noise_generator)]
                self._mcmc_relocate(opts, src, dst)
                n_relocated = n_dead
        n_add = mcmc_num_added(N, cfg.max_gs_num, cfg.mcmc_grow_factor)
        if n_add > 0:
            src = torch.multinomial(self._visible_opacity(), n_add, replacement=True, generator=self.noise_generator)  # on the relocated values
            self._mcmc_grow(optimizers, opts, n_add)
            self._mcmc_relocate(opts, src, torch.arange(N, N + n_add, device=src.device))
        self.last_refine_counts = (n_dead, n_relocated, n_add)
        if n_relocated or n_add:  # what the last training frame left refers to other Gaussians now
            self.last_radii = None
            self.last_xys_grad = self.last_xys_absgrad = None
        self.xys_grad_norm = self.vis_counts = self.max_2Dsize = None

    def _mcmc_relocate(self, opts, src: Tensor, dst: Tensor) -> None:
        names = self.param_names
        moments = self._adam_moments(opts)
        mcmc_relocate([self.gauss_params[k].data for k in names], [moments[k][0] if k in moments else None for k in names],
                      [moments[k][1] if k in moments else None for k in names], src, dst, self.config.mcmc_min_opacity)

    @torch.no_grad()
    def mcmc_noise_after(self, optimizers, step: int) -> None:
        """The MCMC position noise of one iteration (while step < stop_split_at): means += Sigma (randn * g * noise_lr * lr), lr the "xyz"
        optimiser's current learning rate, randn [N,3] from the model's noise_generator, in one tn_splat_mcmc_noise call; Adam state untouched."""
        assert step == self.step
        if not self.mcmc or self.step >= self.config.stop_split_at or self.num_points == 0:
            return
        opts = getattr(optimizers, "optimizers", optimizers) or {}
        if "xyz" not in opts:
            raise RuntimeError('mcmc_noise_after: the noise is scaled by the learning rate of the "xyz" optimiser, which is missing')
        lr = float(opts["xyz"].param_groups[0]["lr"])
        gp = self.gauss_params
        z = torch.randn((self.num_points, 3), device=self.means.device, generator=self.noise_generator)
        mcmc_noise(gp["means"].data, gp["scales"].data, gp["quats"].data, gp["opacities"].data, z, self.config.noise_lr * lr,
                   gp["opacities_thermal"].data if self.separate else None)


def mcmc_num_added(n: int, max_gs_num: int, grow_factor: float) -> int:
    """How many Gaussians an MCMC refinement adds to n of them: max(0, min(max_gs_num, int(grow_factor * n)) - n)."""
    return max(0, min(int(max_gs_num), int(grow_factor * n)) - n)
