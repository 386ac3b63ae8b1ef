"""N4: forward Gaussian-splat render with an RGB + thermal colour per Gaussian ("thermal-splatfacto", BASELINE config 4).

The reference has no thermal-splatfacto method; the boundary mirrored here is stock `SplatfactoModel.get_outputs(camera)`
(nerfstudio/models/splatfacto.py:659-822) with the parameter names of its `gauss_params` (means, scales, quats, opacities, features_dc,
features_rest) plus a second set of SH coefficients with one channel (features_dc_thermal / features_rest_thermal) rendered through the
same rasteriser -- the splat analogue of thermal-nerfacto's shared density (`thermal_opacity_mode` "shared", the default).  With
`thermal_opacity_mode` "separate" -- the analogue of ThermalNerfactoModelConfig.density_mode "separate", the reference's default -- every
Gaussian also has `opacities_thermal` [N,1] (logits, started at logit(0.1) like `opacities`, its own optimiser group): RGB, accumulation and
depth composite with sigmoid(opacities), the thermal channel with sigmoid(opacities_thermal) through a transmittance chain of its own over the
same depth-sorted tile lists (its own 1e-4 stop, its background weighted by its own final transmittance; `accumulation_thermal` [H,W,1] is its
accumulation), so glass can be clear in RGB and opaque in thermal.  That mode runs the _sep family of entry points (tn_splat_project_sep ...
tn_splat_refine_apply_sep: the same kernels instantiated with the second chain); its backward is as exact and bit-reproducible, `last_xys_grad`
sums both chains; refinement culls a Gaussian for low opacity only when BOTH opacities are below `cull_alpha_thresh`, and carries, copies and
resets the thermal logits exactly as the opacities.  `opacity_loss_mult` > 0 adds the NeRF model's `density_loss`
(models/thermal_nerfacto.py:328-344) on the two opacities.  With `removal_min_opacity_diff` = thr set (separate mode only; None = off) the eval
render also returns ThermalNeRF's removal renders (models/thermal_nerfacto.py:460-487, scripts/render.py:737-765, opacities for densities):
`removal` [H,W,3], the RGB colour composited only from the Gaussians with |o - o_th| < thr * o, and `removal_thermal` [H,W,1], the thermal colour
from those with |o_th - o| < thr * o_th (o, o_th the two sigmoids; strict, so thr = 0 is the background), each with a transmittance chain, stop
and background weight of its own -- what sits behind glass or an IR-transparent cover -- from ONE more rasteriser launch
(tn_splat_raster_removal_sep) over the tile lists the frame already has; training renders never carry them.  The three gsplat calls (project_gaussians,
spherical_harmonics, rasterize_gaussians x2) run as tn_splat_project / tn_splat_bin / tn_splat_raster of libthermal_nerf_hip.so.
`get_outputs` is the eval render.  `get_train_outputs` is the same render as a differentiable function of every `gauss_params` tensor: its
backward (tn_splat_raster_backward / tn_splat_project_backward) is the exact, bit-reproducible derivative of the forward this file computes,
and it leaves dL/d xys per Gaussian in `last_xys_grad` (what splatfacto's densification reads as `self.xys.grad`, splatfacto.py:355).
Depth is returned detached.  Training follows splatfacto's refinement (splatfacto.py:346-498): `after_train` accumulates the gradient
statistics (tn_splat_grad_stats), `refinement_after` splits, duplicates and culls the Gaussians (tn_splat_refine_plan / tn_splat_refine_apply)
and carries every optimiser's parameter and Adam moments along, and resets the opacities now and then.  The objective is splatfacto's
(splatfacto.py:848-903): `get_loss_dict` takes (1 - ssim_lambda) * L1 + ssim_lambda * (1 - SSIM) of the frame's spectrum in one fused HIP call
(tn_image_loss: the loss and d loss / d prediction, no host synchronisation), with pytorch_msssim's SSIM; `background_color = "random"` draws
a random RGB + thermal background per training frame.  Construction follows splatfacto's populate_modules (splatfacto.py:190-242): from
`seed_points` (the dataparser's points3D_xyz / points3D_rgb, dataparser.py `load_3D_points`) one Gaussian per point, its log-scale the log of the
mean distance to its 3 nearest neighbours (`knn_distances`: tn_knn, an exact HIP search), or -- without seeds or with `random_init` -- the random
cube of before.  Training can run splatfacto's coarse-to-fine resolution schedule (splatfacto.py:112-116, 639-657): with `num_downscales` = n the
training render and its ground truth are at 1 / 2^n of the frame's size for the first `resolution_schedule` steps and double every
`resolution_schedule` steps after (`downscale_factor`); the camera is rescaled as a copy (`rescaled_camera`), the ground truth -- uint8 or float --
by one HIP bilinear resize with torchvision's resize(antialias=None) semantics (`resize_image`: tn_image_resize); the eval render is always
full size.  ThermalNeRF's two cross-spectrum regularisers (model_components/losses.py:602-651, used at models/thermal_nerfacto.py:346-354) are there
for RGB frames: with `tv_pixel_loss_mult` / `cross_channel_loss_mult` above 0 (both default 0: stock splatfacto has neither) `get_loss_dict` adds
`tv_pixel_loss` -- the 2 x 2-patch total variation of the thermal render at the RGB camera -- and `cross_channel_loss` -- that render's pixel
differences against those of the RGB ground truth's grey value -- over every stride-1 window of the frame, in one fused HIP call
(`thermal_regularizers`: tn_thermal_reg), so the thermal channel gets a gradient from RGB frames too.  The rasteriser is strictly pinhole; distorted frames
are resampled once into pinhole frames, as the reference's FullImageDatamanager does with OpenCV (full_images_datamanager.py:132-225, 351-386):
`undistorted_camera` is the pinhole camera of a distorted one (the largest frame of the same size that reads only inside the source),
`undistort_image` the frame it sees (tn_image_undistort, uint8 or fp32 in and out), with tn_raygen's distortion model and pixel convention, so a
dataset means the same on the NeRF path and here; splat_datamanager.ThermalFullImageDatamanager caches the undistorted frames on the device and
serves (camera, batch).  The eval render takes splatfacto's crop box (splatfacto.py:374-376, 690-698, 904-915): `OrientedBox` (R, T, S as
nerfstudio/data/scene_box.py:82-114; `from_params(pos, rpy, scale)`, `within(pts)`), `set_crop(box)` / `crop_box` and
`get_outputs_for_camera(camera, obb_box)`, the door of the viewer, ns-render and the exporter.  With a box set `get_outputs` renders only the
Gaussians whose mean is strictly inside it, bit for bit the frame of a model holding those alone -- rgb, thermal, depth, the accumulations and the
removal renders.  The reference gathers six parameter tensors through a boolean index per frame; here the box test is the first thing the
projection kernel does (tn_splat_project_crop / _crop_sep): a Gaussian outside leaves with radius 0 and no tiles, as one behind the camera, a
block of Gaussians that are all outside never reads its SH coefficients, and nothing is copied, allocated or read back.  The training render never
crops (the reference crops only outside training), and the box is neither a parameter nor in the state dict.  Camera poses can be refined as on
the NeRF path (ThermalNerfactoModelConfig's camera_optimizer / camera_optimizer_thermal, cameras/camera_optimizers.py): with
`camera_optimizer` / `camera_optimizer_thermal` in mode "SO3xR3" (a row per training frame, training renders only) or "shared_SO3xR3" (one row per
spectrum -- a mis-registered thermal rig -- eval renders too) a frame reads the row (t, w) its PinholeCamera.cam_idx / is_thermal names,
c2w' = c2w [A(p); 0 0 0 1] with A = exp_map_SO3xR3, and `get_train_outputs` is differentiable in it: the corrected camera is built on the device
(tn_splat_pose_camera), the pose instantiations of the projection kernels read it (tn_splat_project_pose / tn_splat_project_backward_pose), and
the backward reduces dL/d view' over the Gaussians without atomics, bit-reproducibly; the SH view directions take the corrected position as a
value (splatfacto.py:770).  Both modes default to "off", which changes nothing.  Densification has a second strategy,
`strategy` = "mcmc" ("3D Gaussian Splatting as Markov Chain Monte Carlo": gsplat's MCMCStrategy, current splatfacto's strategy "mcmc" with
`max_gs_num`): a fixed budget of Gaussians instead of gradient thresholds.  Every `refine_every` steps (between warmup_length and stop_split_at)
the refinement callback relocates the dead Gaussians -- visible opacity (the larger of the two sigmoids in separate mode) <= `mcmc_min_opacity` --
onto live ones drawn with probability proportional to their visible opacity (torch.multinomial of the model's noise_generator), correcting the
opacity and the scale of source and copies so that the render is preserved, then grows the population by `mcmc_grow_factor` up to `max_gs_num`
in the same way; both go through tn_splat_mcmc_relocate / _sep, in place on every parameter tensor and both Adam moments (source rows lose their
moments, as in gsplat), with the relocation values evaluated in double.  One more callback adds position noise after every step,
means += Sigma (randn * g * noise_lr * lr of the means), g = sigmoid(100 ((1 - o_vis) - 0.995)), in one tn_splat_mcmc_noise / _sep launch, and
`get_loss_dict` adds `mcmc_opacity_reg` * mean(sigmoid(opacities)) (+ the thermal mean in separate mode) and `mcmc_scale_reg` * mean(exp(scales)).
No gradient statistics, no cull, no opacity reset; `last_refine_counts` = (dead, relocated, added).  "default" (the default) takes the code path
of before, untouched.  Whether "mcmc" trains thermal scenes better is not established (profiles/splat_mcmc.md).  Masks are not built.  Parity is unpinned (gsplat is a third-party package outside the reference
tree; oracle/splat_oracle.py restates its published algorithm).  No CPU path.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib
from .config import CameraOptimizerConfig
from .ops import _stream

BLOCK_WIDTH = 16  # splatfacto.py:738
CAMERA_OPTIMIZER_MODES = ("off", "SO3xR3", "shared_SO3xR3")  # "SE3" is not built
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
    # instead of |sum over pixels d L_p / d xys|, whose pixel terms cancel on a large Gaussian over fine structure (tn_splat_raster_backward_abs;
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

    def __post_init__(self):
        for name in ("camera_optimizer", "camera_optimizer_thermal"):
            mode = getattr(self, name).mode
            if mode not in CAMERA_OPTIMIZER_MODES:
                raise ValueError(f'{name}.mode = {mode!r}: the splat path refines poses with "SO3xR3" or "shared_SO3xR3" ("off": not at all)')
        for name in ("tv_pixel_loss_mult", "cross_channel_loss_mult", "opacity_loss_mult", "rgb_opacity_loss_mult"):
            if getattr(self, name) < 0:
                raise ValueError(f"{name} = {getattr(self, name)}: a loss multiplier cannot be negative")
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
        if self.removal_min_opacity_diff is not None:
            if self.thermal_opacity_mode != "separate":
                raise ValueError('removal_min_opacity_diff needs thermal_opacity_mode "separate": the removal renders compare the two opacities')
            if not self.removal_min_opacity_diff >= 0:
                raise ValueError(f"removal_min_opacity_diff = {self.removal_min_opacity_diff}: a number >= 0, or None for no removal renders")


@dataclass
class PinholeCamera:
    """One perspective camera: what SplatfactoModel.get_outputs reads from `Cameras` (camera_to_worlds [3,4] in nerfstudio's convention --
    x right, y up, z back -- and the intrinsics)."""

    camera_to_world: Tensor
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    cam_idx: Optional[int] = None  # the frame's index among the training frames: the row of a per-frame pose optimiser (None: no row)
    is_thermal: bool = False  # the spectrum, which picks the pose optimiser (camera_optimizer / camera_optimizer_thermal)


def _rotation_rpy(roll: float, pitch: float, yaw: float) -> Tensor:
    """Rz(yaw) Ry(pitch) Rx(roll) [3,3] in float64 (radians): what viser's SO3.from_rpy_radians(roll, pitch, yaw).as_matrix() gives."""
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    rz = torch.tensor([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    ry = torch.tensor([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]], dtype=torch.float64)
    rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]], dtype=torch.float64)
    return rz @ ry @ rx


@dataclass
class OrientedBox:
    """The reference's oriented box (nerfstudio/data/scene_box.py:82-114): box coordinates -> world is p = R q + T, and the box is
    |q_i| < S_i / 2.  R [3,3] may be any invertible matrix (a rotation from `from_params`), T [3] is the centre, S [3] the full extents.

    `within(pts)`: q = inverse([R|T]) [p, 1]; inside iff -S_i/2 < q_i < S_i/2 on all three axes, strictly on both sides -- a point exactly on
    a face is outside and a non-positive S_i keeps nothing.  The 3x4 world -> box matrix is computed once per call on the host in float64 and
    rounded to fp32 (`world_to_box`; a singular R is a ValueError); q_i = ((m_i0 x + m_i1 y) + m_i2 z) + m_i3 is then evaluated in the points'
    precision, every product and sum rounded on its own.  float32 HIP tensors go through tn_splat_crop_mask, the device function the cropped
    projection itself uses; anything else runs the same rule in torch."""

    R: Tensor
    T: Tensor
    S: Tensor

    @staticmethod
    def from_params(pos: Tuple[float, float, float], rpy: Tuple[float, float, float], scale: Tuple[float, float, float]) -> "OrientedBox":
        """Centre `pos`, extents `scale`, R = Rz(yaw) Ry(pitch) Rx(roll) with rpy = (roll, pitch, yaw) in radians (scene_box.py:100-114)."""
        return OrientedBox(R=_rotation_rpy(*(float(a) for a in rpy)).float(), T=torch.tensor([float(v) for v in pos], dtype=torch.float32),
                           S=torch.tensor([float(v) for v in scale], dtype=torch.float32))

    def _world_to_box_rows(self) -> List[List[float]]:
        """inverse([R|T]) = [R^-1 | -R^-1 T], three rows of four, in float64 (Python floats: the adjugate over the determinant -- no tensor
        work, this runs once per cropped frame)."""
        R, T, S = (torch.as_tensor(v).detach() for v in (self.R, self.T, self.S))
        if R.shape != (3, 3) or T.shape != (3,) or S.shape != (3,):
            raise ValueError(f"OrientedBox: R [3,3], T [3] and S [3] expected, got {tuple(R.shape)}, {tuple(T.shape)} and {tuple(S.shape)}")
        (a, b, c), (d, e, f), (g, h, i) = R.tolist()
        t = T.tolist()
        adj = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f], [d * h - e * g, b * g - a * h, a * e - b * d]]
        det = a * adj[0][0] + b * adj[1][0] + c * adj[2][0]
        size = math.sqrt(a * a + b * b + c * c) * math.sqrt(d * d + e * e + f * f) * math.sqrt(g * g + h * h + i * i)  # |det| <= this (Hadamard)
        if not (math.isfinite(det) and math.isfinite(size)) or abs(det) <= 1e-12 * size:
            raise ValueError("OrientedBox: R is singular, the box has no world -> box transform")
        rows = [[v / det for v in row] for row in adj]
        return [row + [-(row[0] * t[0] + row[1] * t[1] + row[2] * t[2])] for row in rows]

    def world_to_box(self) -> Tensor:
        """inverse([R|T]) as [3,4] fp32 on the host, inverted in float64 and rounded once."""
        return torch.tensor(self._world_to_box_rows(), dtype=torch.float64).float()

    def crop_struct(self) -> _lib.TnSplatCrop:
        """The box as the C entry points take it: rows of `world_to_box` and S / 2."""
        rows = self._world_to_box_rows()
        c = _lib.TnSplatCrop()
        c.world_to_box[:] = [v for row in rows for v in row]  # ctypes rounds the float64 values to fp32
        c.half_extent[:] = [0.5 * v for v in torch.as_tensor(self.S).detach().float().tolist()]
        return c

    def within(self, pts: Tensor) -> Tensor:
        """bool [n] for pts [n,3]: which points are strictly inside the box."""
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"OrientedBox.within: pts must be [n,3], got {tuple(pts.shape)}")
        if pts.is_cuda and pts.dtype == torch.float32:
            p = pts.detach().contiguous()
            mask = torch.empty((p.shape[0],), dtype=torch.uint8, device=p.device)
            crop = self.crop_struct()
            _lib.check(_lib.load().tn_splat_crop_mask(C.byref(crop), _ptr(p, torch.float32, "pts"), p.shape[0], C.c_void_p(mask.data_ptr()), _stream()),
                       "tn_splat_crop_mask")
            return mask.bool()
        p = pts.detach()
        if not p.is_floating_point():
            p = p.float()
        m = self.world_to_box().to(device=p.device, dtype=p.dtype)
        h = (0.5 * torch.as_tensor(self.S).detach().to("cpu", torch.float32)).to(device=p.device, dtype=p.dtype)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        inside = torch.ones(p.shape[0], dtype=torch.bool, device=p.device)
        for i in range(3):
            q = ((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3]
            inside &= q.abs() < h[i]
        return inside


def downscale_factor(step: int, num_downscales: int, resolution_schedule: int, training: bool) -> int:
    """splatfacto.py:639-646: what the training render and its ground truth are shrunk by at `step`; 1 outside training."""
    if training:
        return 2 ** max(num_downscales - step // resolution_schedule, 0)
    return 1


def rescaled_camera(camera: PinholeCamera, d: int) -> PinholeCamera:
    """Cameras.rescale_output_resolution(1 / d) (cameras/cameras.py:986-1010) as a new camera: the intrinsics times 1 / d, the size truncated.
    The reference rescales its camera in place and back after the projection (splatfacto.py:700, 756); the caller's camera is left alone here."""
    f = 1 / d
    return dataclasses.replace(camera, fx=camera.fx * f, fy=camera.fy * f, cx=camera.cx * f, cy=camera.cy * f, width=int(camera.width / d),
                               height=int(camera.height / d))


def projection_matrix(znear: float, zfar: float, fovx: float, fovy: float) -> Tensor:
    """splatfacto.py:82-100."""
    t = znear * math.tan(0.5 * fovy)
    b = -t
    r = znear * math.tan(0.5 * fovx)
    l = -r  # noqa: E741
    n, f = znear, zfar
    return torch.tensor([[2 * n / (r - l), 0.0, (r + l) / (r - l), 0.0], [0.0, 2 * n / (t - b), (t + b) / (t - b), 0.0],
                         [0.0, 0.0, (f + n) / (f - n), -1.0 * f * n / (f - n)], [0.0, 0.0, 1.0, 0.0]], dtype=torch.float32)


def camera_struct(cam: PinholeCamera, clip_thresh: float = 0.01) -> _lib.TnSplatCamera:
    """splatfacto.py:700-720: flip y/z into gsplat's convention, invert analytically, build the full projection matrix (host side, 4x4)."""
    c2w = cam.camera_to_world.detach().float().cpu()
    R = c2w[:3, :3] @ torch.diag(torch.tensor([1.0, -1.0, -1.0]))
    T = c2w[:3, 3:4]
    R_inv = R.T
    T_inv = -R_inv @ T
    viewmat = torch.eye(4)
    viewmat[:3, :3] = R_inv
    viewmat[:3, 3:4] = T_inv
    fovx = 2 * math.atan(cam.width / (2 * cam.fx))
    fovy = 2 * math.atan(cam.height / (2 * cam.fy))
    proj = projection_matrix(0.001, 1000, fovx, fovy) @ viewmat
    s = _lib.TnSplatCamera()
    for i, v in enumerate(viewmat[:3].reshape(-1).tolist()):
        s.viewmat[i] = v
    for i, v in enumerate(proj.reshape(-1).tolist()):
        s.projmat[i] = v
    s.fx, s.fy, s.cx, s.cy = float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)
    for i, v in enumerate(c2w[:3, 3].tolist()):
        s.position[i] = v
    s.clip_thresh = clip_thresh
    s.width, s.height = int(cam.width), int(cam.height)
    return s


def _ptr(t: Optional[Tensor], dtype, name: str):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} HIP tensor (the splat path has no CPU fallback)")
    return C.c_void_p(t.data_ptr())


def _pose_row_ptr(pose: Tensor, row: int, name: str = "pose_adjustment"):
    """Device pointer of row `row` of a contiguous fp32 [C,6] tensor (a host offset: nothing is read)."""
    _ptr(pose, torch.float32, name)
    if pose.dim() != 2 or pose.shape[1] != 6 or not 0 <= row < pose.shape[0]:
        raise ValueError(f"{name} must be [C,6] with the frame's row {row} inside, got {tuple(pose.shape)}")
    return C.c_void_p(pose.data_ptr() + 24 * row)


def pose_camera_record(camera: PinholeCamera, cam: _lib.TnSplatCamera, pose: Tensor, row: int) -> Tensor:
    """The camera corrected by row `row` of `pose` [C,6] (c2w' = c2w [A(p); 0 0 0 1], camera_optimizers.py:178-186) as the device record the
    _pose entry points read (tn_splat_pose_camera: one launch, the pose is never read on the host).  [TN_SPLAT_POSE_CAMERA_FLOATS] fp32: view'
    [0:12], proj' [12:28], position' [28:31], the two intrinsic projection entries [31:33].  With a zero row it holds `cam`'s own numbers."""
    fovx, fovy = 2 * math.atan(camera.width / (2 * camera.fx)), 2 * math.atan(camera.height / (2 * camera.fy))
    P = projection_matrix(0.001, 1000, fovx, fovy)  # camera_struct's: projmat = P @ viewmat, rows 0, 1, 3 one product each
    rec = torch.empty(_lib.TN_SPLAT_POSE_CAMERA_FLOATS, device=pose.device)
    _lib.check(_lib.load().tn_splat_pose_camera(C.byref(cam), float(P[0, 0]), float(P[1, 1]), _pose_row_ptr(pose, row), _ptr(rec, torch.float32, "pose camera"),
                                                _stream()), "tn_splat_pose_camera")
    return rec


KNN_MAX_K = 8  # tn_knn's largest k


def knn_distances(points: Tensor, k: int = 3, return_index: bool = False):
    """Exact k-nearest-neighbour distances of every point to the OTHER points (k_nearest_sklearn, splatfacto.py:272-290: NearestNeighbors(k + 1)
    over the cloud, the point itself dropped) in one tn_knn call on the current stream.  points: contiguous [N,3] fp32 on the device ->
    distances [N,k] fp32, ascending (and neighbour indices [N,k] int64 with return_index).  d = sqrtf((dx*dx + dy*dy) + dz*dz) in fp32, ties go
    to the smaller index: bit-identical to a brute force with that formula, and deterministic.  Raises ValueError for non-finite points (one
    host synchronisation) and for N < k + 1."""
    if not isinstance(points, Tensor) or not points.is_cuda or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("knn_distances takes an [N,3] float32 HIP tensor (the splat path has no CPU fallback)")
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"knn_distances: k = {k}, tn_knn supports 1..{KNN_MAX_K}")
    n = points.shape[0]
    if n < k + 1:
        raise ValueError(f"knn_distances: {n} points, k = {k} needs at least k + 1")
    pts = points.contiguous()
    if not bool(torch.isfinite(pts).all()):
        raise ValueError("knn_distances: the points must be finite")
    lib = _lib.load()
    need = int(lib.tn_knn_workspace_bytes(n, k))
    if need < 0:
        raise RuntimeError(f"tn_knn_workspace_bytes({n}, {k}) failed")
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=pts.device)
    dist = torch.empty((n, k), device=pts.device)
    idx = torch.empty((n, k), dtype=torch.int32, device=pts.device) if return_index else None
    _lib.check(lib.tn_knn(_ptr(pts, torch.float32, "points"), n, k, _ptr(dist, torch.float32, "distances"), _ptr(idx, torch.int32, "indices"),
                          C.c_void_p(ws.data_ptr()), need, _stream()), "tn_knn")
    return (dist, idx.long()) if return_index else dist


SH_C0 = 0.28209479177387814  # utils/spherical_harmonics.py


def RGB2SH(rgb: Tensor) -> Tensor:
    """utils/spherical_harmonics.py: RGB2SH"""
    return (rgb - 0.5) / SH_C0


VIEWER_BACKGROUND = (0.1490, 0.1647, 0.2157)  # eval background of "random" (splatfacto.py:680-682)


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
    lib = _lib.load()
    need = int(lib.tn_image_loss_workspace_bytes(H, W, Cc))
    if need < 0:
        raise ValueError(f"tn_image_loss_workspace_bytes: bad sizes {H} x {W} x {Cc}")
    dev = pred.device
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(3, device=dev)
    grad = torch.empty((H, W, Cc), device=dev) if want_grad else None
    _lib.check(lib.tn_image_loss(C.c_void_p(pred.data_ptr()), ps, C.c_void_p(gt.data_ptr()), gs, H, W, Cc, float(ssim_lambda), float(weight),
                                 C.c_void_p(ws.data_ptr()), need, C.c_void_p(out.data_ptr()), C.c_void_p(grad.data_ptr()) if grad is not None else None,
                                 _stream()), "tn_image_loss")
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
    dtype = _lib.TN_IMAGE_U8 if image.dtype == torch.uint8 else _lib.TN_IMAGE_F32
    _lib.check(_lib.load().tn_image_resize(C.c_void_p(image.data_ptr()), dtype, ps, H, W, Cc, C.c_void_p(out.data_ptr()), h, w, _stream()),
               "tn_image_resize")
    return out


_NEWTON_ITERS = 50  # undistorted_camera: Newton steps per border pixel, and the residual (normalised coordinates) it must reach
_NEWTON_TOL = 1e-9
_SETTLE_ITERS = 100  # ... and the steps and the miss (pixels) of settling the rectangle on the new frame's own border
_SETTLE_TOL = 1e-9


def _distort(x: Tensor, y: Tensor, k: List[float]) -> Tuple[Tensor, Tensor]:
    k1, k2, k3, k4, p1, p2 = k
    r = x * x + y * y
    d = 1 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
    return d * x + 2 * p1 * x * y + p2 * (r + 2 * x * x), d * y + 2 * p2 * x * y + p1 * (r + 2 * y * y)


def _undistort_points(xd: Tensor, yd: Tensor, k: List[float]) -> Tuple[Tensor, Tensor, float]:
    """Newton from (xd, yd) on _distort(x, y) = (xd, yd), float64, _NEWTON_ITERS steps -> (x, y, the largest residual; inf when not finite)."""
    k1, k2, k3, k4, p1, p2 = k
    x, y = xd.clone(), yd.clone()
    for _ in range(_NEWTON_ITERS):
        r = x * x + y * y
        d = 1 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
        d_r = k1 + r * (2 * k2 + r * (3 * k3 + r * 4 * k4))
        ex, ey = _distort(x, y, k)
        ex, ey = ex - xd, ey - yd
        a, b = d + 2 * x * x * d_r + 2 * p1 * y + 6 * p2 * x, 2 * x * y * d_r + 2 * p1 * x + 2 * p2 * y
        c, e = 2 * x * y * d_r + 2 * p2 * y + 2 * p1 * x, d + 2 * y * y * d_r + 2 * p2 * x + 6 * p1 * y
        det = a * e - b * c
        x, y = x - (ex * e - ey * b) / det, y - (ey * a - ex * c) / det
    ex, ey = _distort(x, y, k)
    res = torch.maximum((ex - xd).abs(), (ey - yd).abs())
    return x, y, (float(res.max()) if bool(torch.isfinite(res).all()) else math.inf)


def _coefficients(distortion) -> List[float]:
    k = [float(v) for v in (distortion.detach().reshape(-1).tolist() if isinstance(distortion, Tensor) else distortion)]  # (floats keep their 64 bits)
    if len(k) != 6:
        raise ValueError(f"distortion must hold the six coefficients k1 k2 k3 k4 p1 p2, got {len(k)} values")
    if not all(math.isfinite(v) for v in k):
        raise ValueError(f"distortion coefficients {k} are not finite")
    return k


def undistorted_camera(camera: PinholeCamera, distortion) -> PinholeCamera:
    """The pinhole camera of the frame `undistort_image` makes of a frame of `camera` with `distortion` = (k1, k2, k3, k4, p1, p2), the
    dataparser's order: the part of cv2.getOptimalNewCameraMatrix(alpha=0) in the reference's _undistort_image
    (data/datamanagers/full_images_datamanager.py:351-386) -- the largest pinhole frame of the same size that sees only valid source pixels.  Size
    and pose are the camera's own; with all six coefficients zero the camera itself is returned.  Host side, float64.

    Model: tn_raygen's (and oracle undistort_opencv's): r = x^2 + y^2, d = 1 + r (k1 + r (k2 + r (k3 + r k4))), x_d = d x + 2 p1 x y +
    p2 (r + 2 x^2), y_d = d y + 2 p2 x y + p1 (r + 2 y^2), so a dataset means the same on the NeRF path and here.  That deviates from the
    reference, whose OpenCV call reads slot k4 as a rational-model coefficient; datasets written as OPENCV have k4 = 0.  Pixel centres are at
    (u + 0.5, v + 0.5), x = (u + 0.5 - cx) / fx, the ray generator's and the rasteriser's convention; OpenCV puts centres at integers and the
    reference hands its K to a half-pixel rasteriser unchanged -- one convention throughout is a deliberate deviation too.

    Rule: the centres of all 2W + 2H - 4 border pixels are mapped to undistorted normalised coordinates by Newton iteration; x0 = the largest x
    over the left column, x1 = the smallest over the right column, y0 / y1 likewise over the top / bottom row; fx' = (W - 1) / (x1 - x0),
    cx' = 0.5 - fx' x0, fy' = (H - 1) / (y1 - y0), cy' = 0.5 - fy' y0.  The new frame's rows and columns are not the undistorted positions of the
    source's border pixels, so at this point its own border pixels still read up to ~1e-3 px outside (or inside) the source frame; the rectangle is
    then settled on them: each side moves by its miss -- min of the source x over the new column 0, max over column W - 1 minus (W - 1), and
    the rows likewise, closed form -- over the focal length, until every miss is below 1e-9 px.  Every output pixel's four taps then lie inside
    the source frame up to rounding and one border pixel per side reads the source's very edge: no region-of-interest pass, no crop.

    ValueError: non-finite coefficients, a distortion Newton cannot invert on the border (residual above 1e-9 after 50 steps), an empty or
    inverted rectangle, one that does not settle."""
    k = _coefficients(distortion)
    if not any(k):
        return camera
    W, H = int(camera.width), int(camera.height)
    fx, fy, cx, cy = float(camera.fx), float(camera.fy), float(camera.cx), float(camera.cy)
    if W < 2 or H < 2:
        raise ValueError(f"undistorted_camera: a {W} x {H} frame has no inner rectangle")
    us, vs = torch.arange(W, dtype=torch.float64), torch.arange(H, dtype=torch.float64)
    xs, ys = (us + 0.5 - cx) / fx, (vs + 0.5 - cy) / fy
    left = _undistort_points(xs[0].expand(H), ys, k)
    right = _undistort_points(xs[-1].expand(H), ys, k)
    top = _undistort_points(xs, ys[0].expand(W), k)
    bottom = _undistort_points(xs, ys[-1].expand(W), k)
    worst = max(s[2] for s in (left, right, top, bottom))
    if not worst <= _NEWTON_TOL:
        raise ValueError(f"undistorted_camera: the distortion {k} cannot be inverted on the border of the {W} x {H} frame (residual {worst:.3g})")
    x0, x1, y0, y1 = float(left[0].max()), float(right[0].min()), float(top[1].max()), float(bottom[1].min())
    for _ in range(_SETTLE_ITERS):
        if not (x1 > x0 and y1 > y0):
            raise ValueError(f"undistorted_camera: the distortion {k} leaves no rectangle inside the {W} x {H} frame "
                             f"(x {x0:.4g} .. {x1:.4g}, y {y0:.4g} .. {y1:.4g})")
        nfx, nfy = (W - 1) / (x1 - x0), (H - 1) / (y1 - y0)
        ncx, ncy = 0.5 - nfx * x0, 0.5 - nfy * y0
        nx, ny = (us + 0.5 - ncx) / nfx, (vs + 0.5 - ncy) / nfy
        sx = lambda x, y: fx * _distort(x, y, k)[0] + cx - 0.5  # noqa: E731
        sy = lambda x, y: fy * _distort(x, y, k)[1] + cy - 0.5  # noqa: E731
        miss = (float(sx(nx[0].expand(H), ny).min()), float(sx(nx[-1].expand(H), ny).max()) - (W - 1),
                float(sy(nx, ny[0].expand(W)).min()), float(sy(nx, ny[-1].expand(W)).max()) - (H - 1))
        if max(abs(m) for m in miss) <= _SETTLE_TOL:
            return dataclasses.replace(camera, fx=nfx, fy=nfy, cx=ncx, cy=ncy)
        x0, x1, y0, y1 = x0 - miss[0] / fx, x1 - miss[1] / fx, y0 - miss[2] / fy, y1 - miss[3] / fy
    raise ValueError(f"undistorted_camera: the inner rectangle of the distortion {k} on the {W} x {H} frame does not settle")


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
    code = {torch.uint8: _lib.TN_IMAGE_U8, torch.float32: _lib.TN_IMAGE_F32}
    _lib.check(_lib.load().tn_image_undistort(C.c_void_p(image.data_ptr()), code[image.dtype], ps, H, W, Cc, C.c_void_p(out.data_ptr()),
                                              code[out_dtype], C.byref(p), _stream()), "tn_image_undistort")
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
    lib = _lib.load()
    need = int(lib.tn_thermal_reg_workspace_bytes(H, W))
    if need < 0:
        raise ValueError(f"tn_thermal_reg_workspace_bytes: bad sizes {H} x {W}")
    dev = pred.device
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(2, device=dev)
    grad = torch.empty((H, W, 1), device=dev) if want_grad else None
    _lib.check(lib.tn_thermal_reg(C.c_void_p(pred.data_ptr()), ps, C.c_void_p(gt.data_ptr()), gs, H, W, float(tv_mult), float(cross_mult),
                                  C.c_void_p(ws.data_ptr()), need, C.c_void_p(out.data_ptr()), C.c_void_p(grad.data_ptr()) if grad is not None else None,
                                  _stream()), "tn_thermal_reg")
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


def opacity_density_loss(opacities: Tensor, opacities_thermal: Tensor, opacity_loss_mult: float, rgb_opacity_loss_mult: float) -> Tensor:
    """ThermalNeRF's density_loss (models/thermal_nerfacto.py:328-344) on the two opacity logits [N,1] of the separate mode:
    opacity_loss_mult * (mean|s(o_th) - s(o).detach()| + rgb_opacity_loss_mult * mean|s(o) - s(o_th).detach()|), s = sigmoid.  The first term pulls
    the thermal opacity towards the RGB one, the second (weaker) the RGB one towards the thermal: each term's gradient reaches only its own tensor.
    Elementwise on [N,1], plain torch."""
    o, o_th = torch.sigmoid(opacities), torch.sigmoid(opacities_thermal)
    return opacity_loss_mult * ((o_th - o.detach()).abs().mean() + rgb_opacity_loss_mult * (o - o_th.detach()).abs().mean())


def ssim(pred: Tensor, gt: Tensor) -> Tensor:
    """pytorch_msssim's SSIM(data_range=1) of two [H,W,C] images (mean over channels), a device scalar; no gradient."""
    return image_loss(pred.detach(), gt, 1.0, 1.0)[2]


def _psnr(pred: Tensor, gt: Tensor) -> Tensor:
    """PeakSignalNoiseRatio(data_range=1.0)."""
    return -10.0 * torch.log10(torch.mean((pred - gt) ** 2))


def _is_thermal_frame(batch) -> bool:
    is_th = batch["is_thermal"]
    return bool(is_th) if not hasattr(is_th, "__len__") else bool(torch.as_tensor(is_th).reshape(-1)[0])


_PARAM_NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest", "features_dc_thermal", "features_rest_thermal")
# optimiser group -> gauss_params entry (splatfacto.py:620-628, plus the thermal SH coefficients)
GROUP_PARAMS = {"xyz": "means", "features_dc": "features_dc", "features_rest": "features_rest", "opacity": "opacities", "scaling": "scales",
                "rotation": "quats", "features_dc_thermal": "features_dc_thermal", "features_rest_thermal": "features_rest_thermal"}
# thermal_opacity_mode "separate": the thermal opacity logits come ninth, in a group of their own
_PARAM_NAMES_SEP = _PARAM_NAMES + ("opacities_thermal",)
GROUP_PARAMS_SEP = {**GROUP_PARAMS, "opacities_thermal": "opacities_thermal"}


def param_names(mode: str) -> Tuple[str, ...]:
    """The gauss_params entries of a thermal_opacity_mode, in the order the C entry points take them."""
    return _PARAM_NAMES_SEP if mode == "separate" else _PARAM_NAMES


def _param_ptrs(tensors) -> list:
    """Pointers of eight tensors laid out as the gauss_params, in _PARAM_NAMES order, as the C entry points take them: without higher-order SH
    coefficients (K == 0) the two features_rest tensors are null, and opacities [N,1] goes in flat.  Nine tensors (separate thermal opacity):
    opacities_thermal [N,1] follows, flat too, where the _sep entry points take it."""
    K = tensors[5].shape[1]
    pp = [_ptr(t, torch.float32, n) if (K or not n.startswith("features_rest")) else None for t, n in zip(tensors, _PARAM_NAMES_SEP)]
    for j in (3, 8)[:len(tensors) - 7]:
        pp[j] = _ptr(tensors[j].reshape(-1), torch.float32, _PARAM_NAMES_SEP[j])
    return pp


def _project_and_bin(model, cam, params, H: int, W: int, deg: int, aa: int, cap: int, workspace, crop: Optional[_lib.TnSplatCrop] = None,
                     pose_rec: Optional[Tensor] = None):
    """One frame's tn_splat_project -> tn_splat_bin into `workspace(N, cap, tiles)`, a buffer for `cap` (Gaussian, tile) pairs: the caller says
    where it comes from.  With `crop` the projection is tn_splat_project_crop / _crop_sep: Gaussians outside the box leave with radius 0.  With
    `pose_rec` (pose_camera_record) it is tn_splat_project_pose / _pose_sep, which reads the corrected camera from that record (and takes the box too).  A frame with more pairs grows `cap` once and is redone.  Leaves `last_projection` / `last_num_intersections` on the model
    and returns (projection tensors, workspace, cap, pairs).  No Gaussians: nothing to project, no workspace (None), the frame is the background."""
    i32 = torch.int32
    lib = _lib.load()
    N, K, dev = params[0].shape[0], params[5].shape[1], params[0].device
    tiles = ((W + BLOCK_WIDTH - 1) // BLOCK_WIDTH) * ((H + BLOCK_WIDTH - 1) // BLOCK_WIDTH)
    proj = {"xys": torch.empty((N, 2), device=dev), "depths": torch.empty((N,), device=dev), "radii": torch.empty((N,), dtype=i32, device=dev),
            "conics": torch.empty((N, 3), device=dev), "compensation": torch.empty((N,), device=dev),
            "num_tiles_hit": torch.empty((N,), dtype=i32, device=dev), "tile_box": torch.empty((N, 4), dtype=i32, device=dev)}
    ws, total = None, C.c_int64(0)
    for attempt in range(2 if N > 0 else 0):
        out_ptrs = [_ptr(t, t.dtype, k) for k, t in proj.items()]
        ws = workspace(N, cap, tiles)
        wsp = C.c_void_p(ws.data_ptr())
        if pose_rec is not None:  # a refined pose: the camera comes from the device record
            name = "tn_splat_project_pose_sep" if len(params) == 9 else "tn_splat_project_pose"
            _lib.check(getattr(lib, name)(C.byref(cam), _ptr(pose_rec, torch.float32, "pose camera"), *_param_ptrs(params), N, K, deg, aa, *out_ptrs, wsp, cap,
                                          C.byref(crop) if crop is not None else None, _stream()), name)
        elif crop is not None:  # the eval render's crop box: the same launch with the box test in front
            name = "tn_splat_project_crop_sep" if len(params) == 9 else "tn_splat_project_crop"
            _lib.check(getattr(lib, name)(C.byref(cam), *_param_ptrs(params), N, K, deg, aa, *out_ptrs, wsp, cap, C.byref(crop), _stream()), name)
        elif len(params) == 9:  # separate thermal opacity
            _lib.check(lib.tn_splat_project_sep(C.byref(cam), *_param_ptrs(params), N, K, deg, aa, *out_ptrs, wsp, cap, _stream()), "tn_splat_project_sep")
        else:
            _lib.check(lib.tn_splat_project(C.byref(cam), *_param_ptrs(params), N, K, deg, aa, *out_ptrs, wsp, cap, _stream()), "tn_splat_project")
        rc = lib.tn_splat_bin(C.byref(cam), out_ptrs[1], N, wsp, cap, C.byref(total), _stream())
        if rc == 0:
            break
        if attempt == 0 and total.value > cap:  # more (Gaussian, tile) pairs than the workspace holds: grow once and redo the frame
            cap = int(total.value * 1.25) + 1024
            continue
        _lib.check(rc, "tn_splat_bin")
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


def _project_backward_pose(model, entry, name: str, cam, rec: Tensor, pose: Tensor, row: int, params, grads, N: int, deg: int, aa: int, radii: Tensor,
                           upstream) -> Tensor:
    """The pose instantiation of the projection backward (tn_splat_project_backward_pose / _pose_sep): fills `grads` as the entry point without
    _pose does and returns dL/d pose [C,6] -- zeros but for the frame's row, which the finishing kernel adds into.  dL/d view' [3,4] is left in
    `model.last_view_grad`.  The partials' workspace is this call's own; nothing is read back."""
    f32, dev = torch.float32, pose.device
    need = int(_lib.load().tn_splat_pose_workspace_bytes(N))
    if need < 0:
        raise RuntimeError("tn_splat_pose_workspace_bytes: bad Gaussian count")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    g_pose = torch.zeros_like(pose)
    dview = torch.empty((3, 4), device=dev)
    names = ("v_xys", "v_conics", "v_colors", "v_log_opacity", "v_log_opacity_thermal")
    _lib.check(entry(C.byref(cam), _ptr(rec, f32, "pose camera"), _pose_row_ptr(pose, row), *_param_ptrs(params), N, params[5].shape[1], deg, aa,
                     _ptr(radii, torch.int32, "radii"), *(_ptr(t, f32, n) for t, n in zip(upstream, names)), *_param_ptrs(grads), C.c_void_p(ws.data_ptr()), need,
                     _pose_row_ptr(g_pose, row, "grad_pose"), _ptr(dview, f32, "dview"), _stream()), name)
    model.last_view_grad = dview
    return g_pose


class _SplatRender(torch.autograd.Function):
    """project -> bin -> training raster; backward = raster backward -> projection backward.  Inputs after `frame` are the gauss_params in
    _PARAM_NAMES order; outputs: colour before the clamp [H,W,4] (RGB + thermal over the background), accumulation [H,W,1], depth [H,W,1]
    (not differentiable).  Nine parameters (separate thermal opacity, opacities_thermal last): the _sep entry points, and a fourth output,
    the thermal chain's accumulation [H,W,1].  A frame with a pose row (frame["pose_row"]) passes its optimiser's pose_adjustment [C,6] as one
    more input behind the parameters: the camera is corrected on the device (pose_camera_record), the _pose entry points run, and the backward
    also returns dL/d pose_adjustment [C,6], zero outside the frame's row, and leaves dL/d view' [3,4] in `last_view_grad`."""

    @staticmethod
    def forward(ctx, frame, *params):
        row = frame.get("pose_row")
        pose = None
        if row is not None:
            params, pose = params[:-1], params[-1].detach().contiguous()
        ctx.pose, ctx.rec = pose, (pose_camera_record(frame["camera"], frame["cam"], pose, row) if pose is not None else None)
        model, camera = frame["model"], frame["camera"]
        f32, i32 = torch.float32, torch.int32
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
        if total == 0:  # nothing on screen: the background, and zero gradients
            rgbt = torch.tensor(list(bg4), device=dev).repeat(H, W, 1)
            alpha = torch.zeros((H, W, 1), device=dev)
            depth = torch.full((H, W, 1), 10.0, device=dev)
            ctx.mark_non_differentiable(depth)
            ctx.save_for_backward(*params)
            return (rgbt, alpha, depth, torch.zeros((H, W, 1), device=dev)) if sep else (rgbt, alpha, depth)
        rgbt = torch.empty((H, W, 4), device=dev)
        depth = torch.empty((H, W, 1), device=dev)
        alpha = torch.empty((H, W, 1), device=dev)
        final_t = torch.empty((H, W), device=dev)
        last = torch.empty((H, W), dtype=i32, device=dev)
        if sep:
            alpha_th = torch.empty((H, W, 1), device=dev)
            final_t_th = torch.empty((H, W), device=dev)
            last_th = torch.empty((H, W), dtype=i32, device=dev)
            _lib.check(_lib.load().tn_splat_raster_train_sep(C.byref(cam), N, C.c_void_p(ws.data_ptr()), cap, bg4, aa, _ptr(rgbt, f32, "rgbt"), _ptr(depth, f32, "depth"),
                                                             _ptr(alpha, f32, "alpha"), _ptr(alpha_th, f32, "alpha_thermal"), _ptr(final_t, f32, "transmittance"),
                                                             _ptr(last, i32, "last"), _ptr(final_t_th, f32, "transmittance_thermal"),
                                                             _ptr(last_th, i32, "last_thermal"), _stream()), "tn_splat_raster_train_sep")
            ctx.mark_non_differentiable(depth)
            ctx.ws, ctx.cap, ctx.total = ws, cap, total
            ctx.save_for_backward(*params, proj["radii"], proj["conics"], final_t, last, final_t_th, last_th)
            return rgbt, alpha, depth, alpha_th
        _lib.check(_lib.load().tn_splat_raster_train(C.byref(cam), N, C.c_void_p(ws.data_ptr()), cap, bg4, aa, _ptr(rgbt, f32, "rgbt"), _ptr(depth, f32, "depth"),
                                                     _ptr(alpha, f32, "alpha"), _ptr(final_t, f32, "transmittance"), _ptr(last, i32, "last"), _stream()),
                   "tn_splat_raster_train")
        ctx.mark_non_differentiable(depth)
        ctx.ws, ctx.cap, ctx.total = ws, cap, total
        ctx.save_for_backward(*params, proj["radii"], proj["conics"], final_t, last)
        return rgbt, alpha, depth

    @staticmethod
    def backward(ctx, v_rgbt, v_alpha, _v_depth, v_alpha_th=None):
        frame = ctx.frame
        model = frame["model"]
        saved = ctx.saved_tensors
        P = frame["num_params"]
        sep = P == 9
        params = saved[:P]
        means = params[0]
        N, dev = means.shape[0], means.device
        pose, row = ctx.pose, frame.get("pose_row")
        absgrad = bool(model.config.use_absgrad)  # the _abs entry points: the same gradients plus last_xys_absgrad, the densification statistic
        if ctx.empty:
            model.last_xys_grad = torch.zeros((N, 2), device=dev)
            model.last_xys_absgrad = torch.zeros((N, 2), device=dev) if absgrad else None
            return (None,) + tuple(torch.zeros_like(p) for p in params) + ((torch.zeros_like(pose),) if pose is not None else ())
        radii, conics, final_t, last = saved[P:P + 4]
        lib = _lib.load()
        f32 = torch.float32
        cam, deg, aa, bg4 = frame["cam"], frame["deg"], frame["aa"], frame["bg4"]
        H, W = final_t.shape
        v_rgbt = torch.zeros((H, W, 4), device=dev) if v_rgbt is None else v_rgbt.float().contiguous()
        v_alpha = torch.zeros((H, W, 1), device=dev) if v_alpha is None else v_alpha.float().contiguous()
        if absgrad:
            need = int((lib.tn_splat_backward_workspace_bytes_abs_sep if sep else lib.tn_splat_backward_workspace_bytes_abs)(N, ctx.cap))
        else:
            need = int((lib.tn_splat_backward_workspace_bytes_sep if sep else lib.tn_splat_backward_workspace_bytes)(N, ctx.cap))
        bws = torch.empty(need, dtype=torch.uint8, device=dev)
        v_xys = torch.empty((N, 2), device=dev)
        v_xys_abs = torch.empty((N, 2), device=dev) if absgrad else None
        model.last_xys_absgrad = v_xys_abs
        xys_ptrs = (_ptr(v_xys, f32, "v_xys"),) + ((_ptr(v_xys_abs, f32, "v_xys_abs"),) if absgrad else ())
        v_conics = torch.empty((N, 3), device=dev)
        v_colors = torch.empty((N, 4), device=dev)
        v_lnop = torch.empty((N,), device=dev)
        if sep:
            final_t_th, last_th = saved[P + 4:]
            v_alpha_th = torch.zeros((H, W, 1), device=dev) if v_alpha_th is None else v_alpha_th.float().contiguous()
            v_lnop_th = torch.empty((N,), device=dev)
            name = "tn_splat_raster_backward_abs_sep" if absgrad else "tn_splat_raster_backward_sep"
            _lib.check(getattr(lib, name)(C.byref(cam), N, C.c_void_p(ctx.ws.data_ptr()), ctx.cap, ctx.total, bg4, _ptr(final_t, f32, "transmittance"),
                                          _ptr(last, torch.int32, "last"), _ptr(final_t_th, f32, "transmittance_thermal"),
                                          _ptr(last_th, torch.int32, "last_thermal"), _ptr(conics, f32, "conics"), _ptr(v_rgbt, f32, "v_rgbt"),
                                          _ptr(v_alpha, f32, "v_alpha"), _ptr(v_alpha_th, f32, "v_alpha_thermal"), C.c_void_p(bws.data_ptr()), need,
                                          *xys_ptrs, _ptr(v_conics, f32, "v_conics"), _ptr(v_colors, f32, "v_colors"),
                                          _ptr(v_lnop, f32, "v_log_opacity"), _ptr(v_lnop_th, f32, "v_log_opacity_thermal"), _stream()), name)
            grads = [torch.empty_like(p) for p in params]
            if pose is not None:
                g_pose = _project_backward_pose(model, lib.tn_splat_project_backward_pose_sep, "tn_splat_project_backward_pose_sep", cam, ctx.rec, pose, row,
                                                params, grads, N, deg, aa, radii, (v_xys, v_conics, v_colors, v_lnop, v_lnop_th))
                model.last_xys_grad = v_xys
                return (None,) + tuple(grads) + (g_pose,)
            _lib.check(lib.tn_splat_project_backward_sep(C.byref(cam), *_param_ptrs(params), N, params[5].shape[1], deg, aa, _ptr(radii, torch.int32, "radii"),
                                                         _ptr(v_xys, f32, "v_xys"), _ptr(v_conics, f32, "v_conics"), _ptr(v_colors, f32, "v_colors"),
                                                         _ptr(v_lnop, f32, "v_log_opacity"), _ptr(v_lnop_th, f32, "v_log_opacity_thermal"), *_param_ptrs(grads),
                                                         _stream()), "tn_splat_project_backward_sep")
            model.last_xys_grad = v_xys
            return (None,) + tuple(grads)
        name = "tn_splat_raster_backward_abs" if absgrad else "tn_splat_raster_backward"
        _lib.check(getattr(lib, name)(C.byref(cam), N, C.c_void_p(ctx.ws.data_ptr()), ctx.cap, ctx.total, bg4, _ptr(final_t, f32, "transmittance"),
                                      _ptr(last, torch.int32, "last"), _ptr(conics, f32, "conics"), _ptr(v_rgbt, f32, "v_rgbt"),
                                      _ptr(v_alpha, f32, "v_alpha"), C.c_void_p(bws.data_ptr()), need, *xys_ptrs,
                                      _ptr(v_conics, f32, "v_conics"), _ptr(v_colors, f32, "v_colors"), _ptr(v_lnop, f32, "v_log_opacity"), _stream()), name)
        grads = [torch.empty_like(p) for p in params]
        if pose is not None:
            g_pose = _project_backward_pose(model, lib.tn_splat_project_backward_pose, "tn_splat_project_backward_pose", cam, ctx.rec, pose, row, params,
                                            grads, N, deg, aa, radii, (v_xys, v_conics, v_colors, v_lnop))
            model.last_xys_grad = v_xys
            return (None,) + tuple(grads) + (g_pose,)
        _lib.check(lib.tn_splat_project_backward(C.byref(cam), *_param_ptrs(params), N, params[5].shape[1], deg, aa, _ptr(radii, torch.int32, "radii"),
                                                 _ptr(v_xys, f32, "v_xys"), _ptr(v_conics, f32, "v_conics"), _ptr(v_colors, f32, "v_colors"),
                                                 _ptr(v_lnop, f32, "v_log_opacity"), *_param_ptrs(grads), _stream()), "tn_splat_project_backward")
        model.last_xys_grad = v_xys
        return (None,) + tuple(grads)


class SplatCameraOptimizer(nn.Module):
    """The reference's CameraOptimizer (cameras/camera_optimizers.py:89-213) for one spectrum of the splat model: `pose_adjustment` [C,6] (mode
    "SO3xR3", a row (t, w) per training frame) or [1,6] ("shared_SO3xR3", one row for the whole spectrum), zeros at the start; mode "off" (or
    penalty_scale < 0) holds no parameter at all.  As in ThermalNerfactoModel (models/thermal_nerfacto.py:132-144) the optimiser of each
    spectrum is sized to ALL training frames and the other spectrum's rows are non-trainable (`non_trainable_camera_indices`, the frozen mask):
    a frame reads a row only from its own spectrum's optimiser, so those rows never receive a gradient.  `row(camera, training)` is the row a
    frame reads, decided on the host from camera.cam_idx / camera.is_thermal alone: a per-frame row in training only
    (thermal_nerfacto.py:410-412), the shared row always; None renders the camera as it is."""

    def __init__(self, config: CameraOptimizerConfig, num_cameras: int, device, thermal: bool = False,
                 non_trainable_camera_indices: Optional[Tensor] = None):
        super().__init__()
        if config.mode not in CAMERA_OPTIMIZER_MODES:
            raise ValueError(f'camera optimiser mode {config.mode!r}: the splat path refines poses with "SO3xR3" or "shared_SO3xR3" ("off": not at all)')
        self.config = config
        self.mode = "off" if config.penalty_scale < 0 else config.mode
        self.thermal = bool(thermal)
        self.suffix = "_thermal" if thermal else ""
        self.group = "camera_opt" + self.suffix
        self.num_cameras = int(num_cameras)
        frozen = torch.zeros(max(self.num_cameras, 0), dtype=torch.uint8)
        if non_trainable_camera_indices is not None and self.num_cameras > 0:
            frozen[torch.as_tensor(non_trainable_camera_indices, dtype=torch.long)] = 1
        self._frozen_rows = frozenset(int(i) for i in frozen.nonzero().reshape(-1).tolist())  # the host's copy: what row() reads
        self.register_buffer("_frozen", frozen.to(device), persistent=False)
        if self.mode == "SO3xR3" and self.num_cameras < 1:
            raise ValueError('camera optimiser mode "SO3xR3" needs num_train_data: a pose row per training frame')
        if self.mode != "off":
            self.pose_adjustment = nn.Parameter(torch.zeros((1 if self.shared else self.num_cameras, 6), device=device))

    @property
    def shared(self) -> bool:
        return self.mode == "shared_SO3xR3"

    def row(self, camera: PinholeCamera, training: bool) -> Optional[int]:
        if self.mode == "off" or bool(camera.is_thermal) != self.thermal:
            return None
        if self.shared:
            return 0
        idx = camera.cam_idx
        if not training or idx is None or idx in self._frozen_rows:
            return None
        if not 0 <= int(idx) < self.num_cameras:
            raise ValueError(f"camera.cam_idx = {idx}: {self.group} has {self.num_cameras} rows")
        return int(idx)

    def get_loss_dict(self, loss_dict: dict) -> None:
        if self.mode != "off":
            from .autograd_ops import CameraRegularizer

            loss_dict[f"camera_opt_regularizer{self.suffix}"] = CameraRegularizer.apply(
                self.pose_adjustment, self.config.trans_l2_penalty, self.config.rot_l2_penalty, self.config.penalty_scale)

    def get_metrics_dict(self, metrics_dict: dict) -> None:
        if self.mode != "off":
            pa = self.pose_adjustment.detach()
            metrics_dict[f"camera_opt_translation{self.suffix}"] = pa[:, :3].norm()
            metrics_dict[f"camera_opt_rotation{self.suffix}"] = pa[:, 3:].norm()

    def get_param_groups(self, param_groups: dict) -> None:
        if self.mode != "off":
            param_groups[self.group] = [self.pose_adjustment]


class ThermalSplatfactoModel(nn.Module):
    """RGB + thermal Gaussians: eval render (`get_outputs`) and differentiable training render (`get_train_outputs`).  `gauss_params` keeps the
    reference's names (splatfacto.py:226-235).

    Initialisation (populate_modules, splatfacto.py:190-242).  With `seed_points` = (xyz [M,3], rgb [M,3] uint8, either device) and
    `random_init` False: means = xyz; scales = log(mean distance to the 3 nearest neighbours) on all three axes (knn_distances, then the
    reference's torch ops); quats = a normalised Gaussian draw of the model's seeded CPU generator (uniform on S^3, like random_quat_tensor);
    opacities = logit(0.1); features_dc = RGB2SH(rgb / 255) for sh_degree > 0, or logit(rgb / 255, eps=1e-10) for sh_degree 0 -- evaluated in
    float64 and cast to float32, a deviation from the reference, whose fp32 logit is +inf for a channel value of 255 (float64 gives +-23.03);
    random features_dc when rgb has no rows (the reference's "colors without points"); features_rest zero.  The cloud carries no thermal
    values, so features_dc_thermal and features_rest_thermal start at zero: mid-grey in thermal under both colour modes (this project's rule).
    Fewer than 4 seed points is a ValueError (the kNN needs 3 neighbours).  Without seeds, or with `random_init`, construction is this model's
    random cube as before, with the constant log-scale log(0.01 * random_scale): the reference would give the random start kNN scales too,
    which this model deliberately does not, to keep that start unchanged."""

    def __init__(self, config: Optional[ThermalSplatfactoModelConfig] = None, num_points: Optional[int] = None, device="cuda", seed: int = 0,
                 num_train_data: int = 0, seed_points: Optional[Tuple[Tensor, Tensor]] = None, train_is_thermal: Optional[List[bool]] = None):
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

    def _seeded_params(self, seed_points: Tuple[Tensor, Tensor], g: torch.Generator, dim_sh: int, dev: torch.device) -> nn.ParameterDict:
        """populate_modules with seed points (splatfacto.py:190-225); the rules are in the class docstring."""
        xyz, rgb = seed_points
        if xyz.dim() != 2 or xyz.shape[1] != 3 or rgb.dim() != 2 or rgb.shape[1] != 3:
            raise ValueError(f"seed_points must be (xyz [M,3], rgb [M,3]), got {tuple(xyz.shape)} and {tuple(rgb.shape)}")
        n = xyz.shape[0]
        if n < 4:
            raise ValueError(f"seed_points: {n} points, the kNN scales need at least 4")
        if rgb.shape[0] not in (0, n):
            raise ValueError(f"seed_points: {rgb.shape[0]} colours for {n} points")
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
        return nn.ParameterDict({
            "means": nn.Parameter(means),
            "scales": nn.Parameter(scales),
            "quats": nn.Parameter(quats),
            "opacities": nn.Parameter(torch.logit(0.1 * torch.ones(n, 1)).to(dev)),
            "features_dc": nn.Parameter(dc.float().contiguous()),
            "features_rest": nn.Parameter(torch.zeros((n, dim_sh - 1, 3), device=dev)),
            "features_dc_thermal": nn.Parameter(torch.zeros((n, 1), device=dev)),
            "features_rest_thermal": nn.Parameter(torch.zeros((n, dim_sh - 1, 1), device=dev)),
        })

    @property
    def separate(self) -> bool:
        """thermal_opacity_mode == "separate": gauss_params holds opacities_thermal and the _sep entry points run."""
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

    def _workspace_bytes(self, n: int, cap: int, tiles: int) -> int:
        need = int(_lib.load().tn_splat_workspace_bytes(n, cap, tiles))
        if need < 0:
            raise RuntimeError("tn_splat_workspace_bytes: bad sizes")
        return need

    def _new_workspace(self, n: int, cap: int, tiles: int) -> Tensor:
        return torch.empty(self._workspace_bytes(n, cap, tiles), dtype=torch.uint8, device=self.means.device)

    def _workspace(self, n: int, cap: int, tiles: int) -> Tensor:
        """The eval render's workspace, kept between frames (`_ws`, for `_cap` pairs) while it is large enough."""
        need = self._workspace_bytes(n, cap, tiles)
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
        params = [self.gauss_params[k] for k in self.param_names]
        pose, row = self._pose_row(camera, training=False)  # a shared row corrects eval renders of its spectrum too; per-frame rows never do
        rec = pose_camera_record(camera, cam, pose.detach(), row) if row is not None else None
        _, ws, cap, total = _project_and_bin(self, cam, params, H, W, deg, aa, max(self._cap, 1 << 16), self._workspace, self._crop(), rec)
        if total == 0:  # nothing on screen
            return _background_outputs(H, W, bgl, dev, self.separate, thr is not None)
        f32 = torch.float32
        rgbt = torch.empty((H, W, 4), device=dev)
        depth = torch.empty((H, W, 1), device=dev)
        alpha = torch.empty((H, W, 1), device=dev)
        if self.separate:
            alpha_th = torch.empty((H, W, 1), device=dev)
            _lib.check(_lib.load().tn_splat_raster_sep(C.byref(cam), N, C.c_void_p(ws.data_ptr()), cap, (C.c_float * 4)(*bgl), aa, _ptr(rgbt, f32, "rgbt"),
                                                       _ptr(depth, f32, "depth"), _ptr(alpha, f32, "alpha"), _ptr(alpha_th, f32, "alpha_thermal"), _stream()),
                       "tn_splat_raster_sep")
            out = _outputs(rgbt[..., :3], rgbt[..., 3:], depth, alpha, bgl, alpha_th)
            if thr is not None:  # the removal renders: one more walk over the same lists
                rem = torch.empty((H, W, 4), device=dev)
                _lib.check(_lib.load().tn_splat_raster_removal_sep(C.byref(cam), N, C.c_void_p(ws.data_ptr()), cap, (C.c_float * 4)(*bgl), float(thr),
                                                                   _ptr(rem, f32, "removal"), _stream()), "tn_splat_raster_removal_sep")
                out["removal"], out["removal_thermal"] = rem[..., :3], rem[..., 3:]
            return out
        _lib.check(_lib.load().tn_splat_raster(C.byref(cam), N, C.c_void_p(ws.data_ptr()), cap, (C.c_float * 4)(*bgl), aa, _ptr(rgbt, f32, "rgbt"),
                                               _ptr(depth, f32, "depth"), _ptr(alpha, f32, "alpha"), _stream()), "tn_splat_raster")
        return _outputs(rgbt[..., :3], rgbt[..., 3:], depth, alpha, bgl)

    def _pose_row(self, camera: PinholeCamera, training: bool) -> Tuple[Optional[Tensor], Optional[int]]:
        """(pose_adjustment, row) the frame of `camera` reads -- its spectrum's optimiser, at most one row of one tensor -- or (None, None)."""
        opt = self.camera_optimizer_thermal if camera.is_thermal else self.camera_optimizer
        row = opt.row(camera, training)
        return (opt.pose_adjustment, row) if row is not None else (None, None)

    def _get_downscale_factor(self) -> int:
        """splatfacto.py:639-646: the resolution schedule's factor at this step while the module is in training mode, else 1."""
        return downscale_factor(self.step, self.config.num_downscales, self.config.resolution_schedule, self.training)

    def get_train_outputs(self, camera: PinholeCamera) -> Dict[str, Tensor]:
        """The render of get_outputs as a differentiable function of every gauss_params tensor (splatfacto.py:659-822 in training: `crop_box`
        is not read, the reference crops only outside training).  rgb [H,W,3], thermal [H,W,1] and accumulation [H,W,1] carry gradients; depth [H,W,1] is detached.  With a fixed
        background the values equal get_outputs' bit for bit; background_color "random" draws this frame's RGB + thermal background from the
        model's generator (background [3], background_thermal [1]).  After backward(), `last_xys_grad` [N,2] holds dL/d xys per Gaussian
        (and, with config.use_absgrad, `last_xys_absgrad` [N,2] the sum of its per-pixel terms' absolute values).
        Under the resolution schedule the frame is that of `rescaled_camera(camera, d)` (splatfacto.py:699-700): its size is what `last_size`,
        `last_radii`, `last_xys_grad` and the refinement statistics refer to; `camera` is not modified."""
        d = self._get_downscale_factor()
        if d > 1:
            camera = rescaled_camera(camera, d)
        aa, deg = self._frame_settings()
        bgl = self._background4(training=True)
        names = self.param_names
        frame = {"model": self, "camera": camera, "cam": camera_struct(camera), "aa": aa, "deg": deg, "bg4": (C.c_float * 4)(*bgl), "num_params": len(names)}
        self.last_xys_grad = None
        self.last_xys_absgrad = None
        pose, row = self._pose_row(camera, training=True)
        if row is not None:  # the frame's pose row: one more differentiable input
            frame["pose_row"] = row
            rgbt, alpha, depth, *alpha_th = _SplatRender.apply(frame, *(self.gauss_params[k] for k in names), pose)
        else:
            rgbt, alpha, depth, *alpha_th = _SplatRender.apply(frame, *(self.gauss_params[k] for k in names))
        alpha_th = alpha_th[0] if alpha_th else None  # separate mode: the thermal chain's accumulation (differentiable)
        if self.last_num_intersections == 0:  # the background as get_outputs returns it (no clamp)
            return _outputs(rgbt[..., :3], rgbt[..., 3:], depth, alpha, bgl, alpha_th)
        return _outputs(torch.clamp(rgbt[..., :3], max=1.0), torch.clamp(rgbt[..., 3:], max=1.0), depth, alpha, bgl, alpha_th)

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
        mean(s(o)) (+ mean(s(o_th)) in separate mode) and mcmc_scale_reg = mcmc_scale_reg * mean(exp(scales)) (plain torch).  `batch`: image [H,W,3|4],
        is_thermal."""
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
        if self.separate and cfg.opacity_loss_mult > 0:
            losses["density_loss"] = opacity_density_loss(self.gauss_params["opacities"], self.gauss_params["opacities_thermal"], cfg.opacity_loss_mult,
                                                          cfg.rgb_opacity_loss_mult)
        if self.mcmc:  # gsplat's MCMC regularisers: few and small Gaussians (elementwise on [N,1] and [N,3], plain torch)
            o_mean = torch.sigmoid(self.gauss_params["opacities"]).mean()
            if self.separate:
                o_mean = o_mean + torch.sigmoid(self.gauss_params["opacities_thermal"]).mean()
            losses["mcmc_opacity_reg"] = cfg.mcmc_opacity_reg * o_mean
            losses["mcmc_scale_reg"] = cfg.mcmc_scale_reg * torch.exp(self.gauss_params["scales"]).mean()
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
        """The Gaussian groups and, for each pose optimiser that is on, camera_opt / camera_opt_thermal (optim.SPLAT_CAMERA_OPTIMIZERS)."""
        groups = self.get_gaussian_param_groups()
        self.camera_optimizer.get_param_groups(groups)
        self.camera_optimizer_thermal.get_param_groups(groups)
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
        f32 = torch.float32
        _lib.check(_lib.load().tn_splat_grad_stats(_ptr(xys_grad.contiguous(), f32, "xys_grad"), _ptr(self.last_radii, torch.int32, "radii"), N,
                                                   max(self.last_size), int(first), _ptr(self.xys_grad_norm, f32, "grad_norm_sum"),
                                                   _ptr(self.vis_counts, f32, "vis_counts"), _ptr(self.max_2Dsize, f32, "max_2d_size"), _stream()),
                   "tn_splat_grad_stats")

    @torch.no_grad()
    def refinement_after(self, optimizers, step: int) -> None:
        """splatfacto.py:381-498: densify (split + duplicate) and cull, or cull only after stop_split_at; then the opacity reset and a reset of
        the statistics.  `optimizers`: an `Optimizers` (or a dict group -> torch.optim optimiser, or None); every optimiser's parameter is
        replaced by the model's new one, surviving Gaussians keep their Adam moments, new ones start at zero, step counts are kept.
        Strategy "mcmc": when warmup_length < step < stop_split_at and step % refine_every == 0, relocate the dead Gaussians and grow towards
        max_gs_num (`_mcmc_refine`); nothing else."""
        assert step == self.step
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
        lib = _lib.load()
        gp = self.gauss_params
        N, dev, f32 = self.num_points, self.means.device, torch.float32
        S, K = self.config.n_split_samples, gp["features_rest"].shape[1]
        rs = self._refine_struct()
        need = int(lib.tn_splat_refine_workspace_bytes(N, S))
        if need < 0:
            raise RuntimeError("tn_splat_refine_workspace_bytes: bad sizes")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        stats = [self.xys_grad_norm, self.vis_counts, self.max_2Dsize]
        if stats[0] is None:  # cull only, straight after a reset: no screen sizes recorded
            stats = [torch.ones(N, device=dev), torch.ones(N, device=dev), torch.zeros(N, device=dev)]
        counts = (C.c_int64 * 4)()
        names, sep = self.param_names, self.separate
        op_ptrs = [_ptr(gp[k].reshape(-1), f32, k) for k in (("opacities", "opacities_thermal") if sep else ("opacities",))]
        plan, plan_name = (lib.tn_splat_refine_plan_sep, "tn_splat_refine_plan_sep") if sep else (lib.tn_splat_refine_plan, "tn_splat_refine_plan")
        _lib.check(plan(C.byref(rs), int(self.step), _ptr(gp["scales"], f32, "scales"), *op_ptrs, _ptr(stats[0], f32, "grad_norm_sum"),
                        _ptr(stats[1], f32, "vis_counts"), _ptr(stats[2], f32, "max_2d_size"), N, C.c_void_p(ws.data_ptr()), need, counts, _stream()), plan_name)
        n_split, n_orig, n_child, n_dup = (int(c) for c in counts)
        # the reference's noise: randn((n_split_samples * n_split, 3)), sample-major (splatfacto.py:541)
        noise = torch.randn((S * n_split, 3), device=dev, generator=self.noise_generator) if densify else None
        self.last_refine_counts = (n_split, n_orig, n_child, n_dup)
        if n_orig == N and n_child == 0 and n_dup == 0:
            return  # nothing split, duplicated or culled: every tensor stays as it is
        M = n_orig + n_child + n_dup
        old = {k: gp[k] for k in names}
        group_of = {v: g for g, v in self.group_params.items()}
        moments = {}
        for k in names:
            o = opts.get(group_of[k])
            st = o.state.get(old[k]) if o is not None else None
            if st and "exp_avg" in st:
                moments[k] = (st["exp_avg"].contiguous(), st["exp_avg_sq"].contiguous())
        new = {k: torch.empty((M,) + tuple(old[k].shape[1:]), device=dev) for k in names}
        new_m = {k: (torch.empty_like(new[k]), torch.empty_like(new[k])) for k in moments}
        arr = lambda ts: (C.c_void_p * len(names))(*[t.data_ptr() if t is not None and t.numel() else None for t in ts])  # noqa: E731
        apply, apply_name = (lib.tn_splat_refine_apply_sep, "tn_splat_refine_apply_sep") if sep else (lib.tn_splat_refine_apply, "tn_splat_refine_apply")
        _lib.check(apply(C.byref(rs), N, K, C.c_void_p(ws.data_ptr()), need, counts,
                                             _ptr(noise, f32, "noise") if noise is not None and noise.numel() else None,
                                             arr([old[k].detach() for k in names]), arr([moments[k][0] if k in moments else None for k in names]),
                                             arr([moments[k][1] if k in moments else None for k in names]), arr([new[k] for k in names]),
                                             arr([new_m[k][0] if k in new_m else None for k in names]),
                                             arr([new_m[k][1] if k in new_m else None for k in names]), _stream()), apply_name)
        self.gauss_params = nn.ParameterDict({k: nn.Parameter(new[k]) for k in names})
        for k in names:  # dup_in_optim / remove_from_optim (splatfacto.py:292-344)
            g = group_of[k]
            o = opts.get(g)
            if o is None:
                continue
            st = o.state.pop(old[k], None)
            p = self.gauss_params[k]
            o.param_groups[0]["params"] = [p]
            if st is not None:
                if k in new_m:
                    st["exp_avg"], st["exp_avg_sq"] = new_m[k]
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
        names = self.param_names
        old = {k: self.gauss_params[k] for k in names}
        moments = self._adam_moments(opts)
        grown = lambda t: torch.cat([t.detach(), torch.zeros((n_add,) + tuple(t.shape[1:]), device=t.device)], dim=0)  # noqa: E731
        self.gauss_params = nn.ParameterDict({k: nn.Parameter(grown(old[k])) for k in names})
        group_of = {v: g for g, v in self.group_params.items()}
        for k in names:
            g = group_of[k]
            o = opts.get(g)
            if o is None:
                continue
            st = o.state.pop(old[k], None)
            p = self.gauss_params[k]
            o.param_groups[0]["params"] = [p]
            if st is not None:
                if k in moments:
                    st["exp_avg"], st["exp_avg_sq"] = grown(moments[k][0]), grown(moments[k][1])
                o.state[p] = st
            if isinstance(getattr(optimizers, "parameters", None), dict) and g in optimizers.parameters:
                optimizers.parameters[g] = [p]

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


def mcmc_relocate(params: List[Tensor], exp_avg: List[Optional[Tensor]], exp_avg_sq: List[Optional[Tensor]], src_idx: Tensor, dst_idx: Tensor,
                  min_opacity: float) -> None:
    """tn_splat_mcmc_relocate / _sep in place on the current stream, without a host synchronisation.  params: the 8 (9: separate thermal opacity)
    gauss_params tensors in param_names order, contiguous fp32 on the device, all with the same number of rows; exp_avg / exp_avg_sq: per tensor
    its Adam moments or None (both); src_idx / dst_idx: int64 [M] on the device.  Row dst_idx[j] becomes a copy of row src_idx[j] with gsplat's
    relocation opacity and scale (ratio = 1 + how often the source was drawn, capped at 51; evaluated in double), every drawn source takes that
    opacity and scale once and loses its moments; destination moments and every row not named stay.  No destination may be a source or repeat."""
    if len(params) not in (8, 9):
        raise ValueError(f"mcmc_relocate takes the 8 or 9 gauss_params tensors, got {len(params)}")
    if len(exp_avg) != len(params) or len(exp_avg_sq) != len(params):
        raise ValueError("mcmc_relocate: one exp_avg and one exp_avg_sq entry (a tensor or None) per parameter")
    rows, K = params[0].shape[0], params[5].shape[1]
    for t, m1, m2, n in zip(params, exp_avg, exp_avg_sq, _PARAM_NAMES_SEP):
        if t.shape[0] != rows:
            raise ValueError(f"mcmc_relocate: {n} has {t.shape[0]} rows, means {rows}")
        if (m1 is None) != (m2 is None) or (m1 is not None and (m1.shape != t.shape or m2.shape != t.shape)):
            raise ValueError(f"mcmc_relocate: the moments of {n} must both be None or both have its shape")
    if src_idx.shape != dst_idx.shape or src_idx.dim() != 1:
        raise ValueError(f"mcmc_relocate: src_idx and dst_idx must be [M], got {tuple(src_idx.shape)} and {tuple(dst_idx.shape)}")
    M = src_idx.shape[0]
    if M == 0:
        return
    lib = _lib.load()
    pp = _param_ptrs(params)  # checks device, dtype and contiguity; the two features_rest entries are null without higher-order coefficients

    def arr(ts, what):  # a HOST array of device pointers; an entry is null where the tensor is None or the parameter itself is
        return (C.c_void_p * len(params))(*[_ptr(t, torch.float32, what).value if t is not None and p is not None else None for t, p in zip(ts, pp)])

    need = int(lib.tn_splat_mcmc_workspace_bytes(rows, M))
    if need < 0:
        raise RuntimeError("tn_splat_mcmc_workspace_bytes: bad sizes")
    ws = torch.empty(need, dtype=torch.uint8, device=params[0].device)
    name = "tn_splat_mcmc_relocate_sep" if len(params) == 9 else "tn_splat_mcmc_relocate"
    _lib.check(getattr(lib, name)(rows, K, _ptr(src_idx, torch.int64, "src_idx"), _ptr(dst_idx, torch.int64, "dst_idx"), M, float(min_opacity),
                                  arr(params, "params"), arr(exp_avg, "exp_avg"), arr(exp_avg_sq, "exp_avg_sq"), C.c_void_p(ws.data_ptr()), need,
                                  _stream()), name)


def mcmc_noise(means: Tensor, scales: Tensor, quats: Tensor, opacities: Tensor, randn: Tensor, scaler: float,
               opacities_thermal: Optional[Tensor] = None) -> None:
    """tn_splat_mcmc_noise / _sep: means [N,3] += Sigma (randn * g * scaler) in place, one launch on the current stream, fp32.  Sigma =
    R diag(exp(scales)^2) R^T with R the rotation of quats / |quats|; g = 1 / (1 + exp(-100 ((1 - o_vis) - 0.995))), o_vis = sigmoid(opacities)
    or, with opacities_thermal, the larger of the two sigmoids: a Gaussian anyone can see stays where it is.  Contiguous fp32 device tensors."""
    N = means.shape[0]
    if means.shape != (N, 3) or scales.shape != (N, 3) or quats.shape != (N, 4) or randn.shape != (N, 3) or opacities.numel() != N or \
            (opacities_thermal is not None and opacities_thermal.numel() != N):
        raise ValueError("mcmc_noise: means, scales, randn [N,3], quats [N,4], opacities [N,1] of one N expected")
    f32 = torch.float32
    args = [_ptr(means, f32, "means"), _ptr(scales, f32, "scales"), _ptr(quats, f32, "quats"), _ptr(opacities.reshape(-1), f32, "opacities")]
    if opacities_thermal is not None:
        args.append(_ptr(opacities_thermal.reshape(-1), f32, "opacities_thermal"))
    name = "tn_splat_mcmc_noise_sep" if opacities_thermal is not None else "tn_splat_mcmc_noise"
    _lib.check(getattr(_lib.load(), name)(*args, _ptr(randn, f32, "randn"), N, float(scaler), _stream()), name)
