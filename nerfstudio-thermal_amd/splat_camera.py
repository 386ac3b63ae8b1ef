"""The cameras of the splat path (splat.py): the pinhole camera and its C struct, the crop box and the pose optimiser.  Training can run splatfacto's
coarse-to-fine resolution schedule (splatfacto.py:112-116, 639-657): with `num_downscales` = n the training render and its ground truth are at 1 / 2^n
of the frame's size for the first `resolution_schedule` steps and double every `resolution_schedule` steps after (`downscale_factor`); the camera is
rescaled as a copy (`rescaled_camera`).  The rasteriser is strictly pinhole; distorted frames are resampled once into pinhole frames, as the
reference's FullImageDatamanager does with OpenCV (full_images_datamanager.py:132-225, 351-386): `undistorted_camera` is the pinhole camera of a
distorted one (the largest frame of the same size that reads only inside the source), with tn_raygen's distortion model and pixel convention, so a
dataset means the same on the NeRF path and here.  The eval render takes splatfacto's crop box (splatfacto.py:374-376, 690-698, 904-915):
`OrientedBox` (R, T, S as nerfstudio/data/scene_box.py:82-114; `from_params(pos, rpy, scale)`, `within(pts)`).  Camera poses can be refined as on the
NeRF path (ThermalNerfactoModelConfig's camera_optimizer / camera_optimizer_thermal, cameras/camera_optimizers.py): with `camera_optimizer` /
`camera_optimizer_thermal` in mode "SO3xR3" (a row per training frame, training renders only) or "shared_SO3xR3" (one row per spectrum -- a
mis-registered thermal rig -- eval renders too) a frame reads the row (t, w) its PinholeCamera.cam_idx / is_thermal names, c2w' = c2w [A(p); 0 0 0 1]
with A = exp_map_SO3xR3; the corrected camera is built on the device (`pose_camera_record`: tn_splat_pose_camera).  Both modes default to "off", which
changes nothing.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib, splat_calls
from .config import CameraOptimizerConfig

CAMERA_OPTIMIZER_MODES = ("off", "SO3xR3", "shared_SO3xR3")  # "SE3" is not built


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
            splat_calls.crop_mask(self.crop_struct(), p, mask)
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


def pose_camera_record(camera: PinholeCamera, cam: _lib.TnSplatCamera, pose: Tensor, row: int) -> Tensor:
    """The camera corrected by row `row` of `pose` [C,6] (c2w' = c2w [A(p); 0 0 0 1], camera_optimizers.py:178-186) as the device record the
    projection and its backward read (tn_splat_pose_camera: one launch, the pose is never read on the host).  [TN_SPLAT_POSE_CAMERA_FLOATS] fp32: view'
    [0:12], proj' [12:28], position' [28:31], the two intrinsic projection entries [31:33].  With a zero row it holds `cam`'s own numbers."""
    fovx, fovy = 2 * math.atan(camera.width / (2 * camera.fx)), 2 * math.atan(camera.height / (2 * camera.fy))
    P = projection_matrix(0.001, 1000, fovx, fovy)  # camera_struct's: projmat = P @ viewmat, rows 0, 1, 3 one product each
    rec = torch.empty(_lib.TN_SPLAT_POSE_CAMERA_FLOATS, device=pose.device)
    splat_calls.pose_camera(cam, P[0, 0], P[1, 1], pose, row, rec)
    return rec


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
