"""Frames for people: colour maps, camera paths and the frame renderer -- the counterpart of nerfstudio/utils/colormaps.py,
nerfstudio/cameras/camera_paths.py and _render_trajectory_video / the Render* commands of nerfstudio/scripts/render.py (ns-render), for both models.

Colour maps run on the device (csrc/tn_render.hip states the rule once; tests/render_functional.py restates it in torch): `tn_frame_minmax` reads a
panel's finite min and max into two device floats -- only for panels that need them, and nothing is read back --, `tn_frame_compose` writes the whole
side-by-side uint8 frame [H, k W, 3] in one launch, `tn_frame_colors` gives one panel's float colours for a viewer.  The 256 x 3 tables are
matplotlib's, committed as data (colormap_luts.json, scripts/make_colormap_luts.py), so rendering needs no matplotlib.  Camera paths are host work in
float64: they are tens of poses.  Only PNG sequences are written (texture.png_bytes: zlib and struct): there is no video encoder here.  The raw calls
are `minmax_call`, `compose_call` and `colors_call`, the only places that know the argument order of their entry points.  Everything runs on torch's
current stream; there is no CPU fallback.

Differences from the reference, all deliberate: min and max are over a frame's FINITE values ((0, 0) where it has none; torch.min would turn one NaN
into a black frame; all-finite frames agree); `pca` is not built; path cameras are perspective only; nearest-training-camera panels and the crop's
background-colour override are not built; the NeRF model's render is not cropped (its NotImplementedError is passed on).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import math
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .mesh import _is_splat
from .ops import _stream
from .splat_camera import OrientedBox, PinholeCamera, rescaled_camera
from .texture import png_bytes

F32 = torch.float32
COLORMAPS = ("default", "turbo", "viridis", "magma", "inferno", "cividis", "gray", "pca")
LUT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "colormap_luts.json")
_EPS = float(np.finfo(float).eps) * 4.0  # camera_utils._EPS


@dataclass(frozen=True)
class ColormapOptions:
    """colormaps.py:30-43, field for field."""

    colormap: str = "default"
    normalize: bool = False
    colormap_min: float = 0
    colormap_max: float = 1
    invert: bool = False


# ---------------------------------------------------------------------------------------------------- tables
_LUTS: Dict[str, Any] = {}


def colormap_tables() -> Tuple[Tuple[str, ...], np.ndarray]:
    """(names, float32 [6, 256, 3]) of the committed table file."""
    if "host" not in _LUTS:
        with open(LUT_PATH, encoding="utf-8") as f:
            g = json.load(f)  # (decimals that read back to the float32 they were written from)
        _LUTS["host"] = (tuple(str(n) for n in g["names"]), np.ascontiguousarray(np.array(g["luts"], dtype=np.float64).astype(np.float32)))
    return _LUTS["host"]


def _check_colormap(name: str) -> str:
    if name == "pca":
        raise NotImplementedError('colormap "pca" (apply_pca_colormap: feature images) is not built')
    if name not in COLORMAPS:
        raise ValueError(f"colormap {name!r}: one of {COLORMAPS}")
    return "turbo" if name == "default" else name


def _table(name: str, device) -> Optional[Tensor]:
    """The device copy of a colour map's table [256,3], None for "gray" (the value is repeated, as the reference does)."""
    name = _check_colormap(name)
    if name == "gray":
        return None
    key = str(torch.device(device))
    if key not in _LUTS:
        names, luts = colormap_tables()
        _LUTS[key] = (names, torch.from_numpy(luts).to(device).contiguous())
    names, luts = _LUTS[key]
    return luts[names.index(name)]


# ---------------------------------------------------------------------------------------------------- the raw calls
def _f32_dev(t: Tensor, what: str, shape=None) -> Tensor:
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise ValueError(f"{what}: a HIP tensor expected (there is no CPU fallback)")
    if t.dtype != F32:
        raise ValueError(f"{what}: float32 expected, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: shape {tuple(shape)} expected, got {tuple(t.shape)}")
    return t if t.is_contiguous() else t.contiguous()


def minmax_call(src: Tensor, out2: Tensor, workspace: Tensor) -> None:
    """tn_frame_minmax of the contiguous fp32 `src` into out2 (device fp32 [2]); workspace: uint8 [TN_FRAME_MINMAX_WORKSPACE_BYTES]"""
    rc = _lib.load().tn_frame_minmax(C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(out2.data_ptr()), C.c_void_p(workspace.data_ptr()),
                                     workspace.numel() * workspace.element_size(), _stream())
    _lib.check(rc, "tn_frame_minmax")


def compose_call(records: Sequence[_lib.TnFramePanel], H: int, W: int, out: Tensor) -> None:
    """tn_frame_compose of the panel records into out uint8 [H, len(records) W, 3] (contiguous)"""
    k = len(records)
    if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (H, k * W, 3):
        raise ValueError(f"compose: a contiguous uint8 HIP frame [{H}, {k * W}, 3] expected, got {out.dtype} {tuple(out.shape)}")
    arr = (_lib.TnFramePanel * max(k, 1))(*records)
    rc = _lib.load().tn_frame_compose(arr, k, int(H), int(W), C.c_void_p(out.data_ptr()), _stream())
    _lib.check(rc, "tn_frame_compose")


def colors_call(record: _lib.TnFramePanel, H: int, W: int, out: Tensor) -> None:
    """tn_frame_colors of one panel record into out fp32 [H,W,3]"""
    rc = _lib.load().tn_frame_colors(C.byref(record), int(H), int(W), C.c_void_p(_f32_dev(out, "colours", (H, W, 3)).data_ptr()), _stream())
    _lib.check(rc, "tn_frame_colors")


class _Scratch:
    """The min / max pairs and the workspace of one frame's panels (one allocation; the launches are ordered by the stream)."""

    def __init__(self, device, panels: int):
        self.buf = torch.empty(_lib.TN_FRAME_MINMAX_WORKSPACE_BYTES // 4 + 2 * panels, dtype=F32, device=device)
        self.used = 0

    def minmax(self, src: Tensor) -> Tensor:
        words = _lib.TN_FRAME_MINMAX_WORKSPACE_BYTES // 4
        out2 = self.buf[words + 2 * self.used:words + 2 * self.used + 2]
        self.used += 1
        minmax_call(src, out2, self.buf[:words])
        return out2


def _panel(image: Tensor, options: ColormapOptions, scratch: _Scratch, depth: bool = False, accumulation: Optional[Tensor] = None,
           near_plane: Optional[float] = None, far_plane: Optional[float] = None, keep: Optional[list] = None) -> Tuple[_lib.TnFramePanel, int, int]:
    """The record of one panel [H,W,1] or [H,W,3] (tensors it points to are appended to `keep`), and H, W.  tn_frame_minmax is launched here, and only
    where the panel needs it: normalize, or a depth panel without both planes."""
    if image.dim() != 3 or image.shape[2] not in (1, 3):
        raise NotImplementedError(f"a float image [H,W,1] or [H,W,3] expected, got {tuple(image.shape)} (boolean and feature images are not built)")
    H, W, ch = (int(v) for v in image.shape)
    image = _f32_dev(image, "panel")
    keep = keep if keep is not None else []
    keep.append(image)
    rec = _lib.TnFramePanel()
    rec.src, rec.channels = image.data_ptr(), ch
    rec.colormap_min, rec.colormap_max = float(options.colormap_min), float(options.colormap_max)
    if ch == 3:
        return rec, H, W
    table = _table(options.colormap, image.device)
    flags = (_lib.TN_FRAME_NORMALIZE if options.normalize else 0) | (_lib.TN_FRAME_INVERT if options.invert else 0)
    if depth:
        flags |= _lib.TN_FRAME_DEPTH
        if near_plane:  # the reference's `near_plane or min`: None and 0.0 both mean "not given"
            flags |= _lib.TN_FRAME_NEAR
            rec.near_plane = float(near_plane)
        if far_plane:
            flags |= _lib.TN_FRAME_FAR
            rec.far_plane = float(far_plane)
        if accumulation is not None:
            accumulation = _f32_dev(accumulation, "accumulation").reshape(-1)
            if accumulation.numel() != H * W:
                raise ValueError(f"accumulation of {accumulation.numel()} values for a depth panel of {H} x {W}")
            keep.append(accumulation)
            rec.accumulation = accumulation.data_ptr()
    if options.normalize or (depth and not (near_plane and far_plane)):
        out2 = scratch.minmax(image)
        keep.append(out2)
        rec.minmax = out2.data_ptr()
    if table is not None:
        keep.append(table)
        rec.table = table.data_ptr()
    rec.flags = flags
    return rec, H, W


def _colors(image: Tensor, options: ColormapOptions, **kw) -> Tensor:
    keep: list = []
    rec, H, W = _panel(image, options, _Scratch(image.device, 1), keep=keep, **kw)
    out = torch.empty((H, W, 3), dtype=F32, device=image.device)
    colors_call(rec, H, W, out)
    return out


# ---------------------------------------------------------------------------------------------------- colour maps
def apply_colormap(image: Tensor, colormap_options: ColormapOptions = ColormapOptions()) -> Tensor:
    """colormaps.py:46-90 for float images on the device -> fp32 [H,W,3].  Three channels are returned as they are.  One channel: with `normalize`
    (v - min) / (max(v - min) + 1e-9); v (colormap_max - colormap_min) + colormap_min; clip to [0, 1]; with `invert` 1 - v; NaN -> 0; "gray" repeats
    the value, any other map is row trunc(255 v) of its table.  min and max are over the finite values ((0, 0) where there are none)."""
    if image.dim() == 3 and image.shape[2] == 3:
        _check_colormap(colormap_options.colormap)
        return image
    return _colors(image, colormap_options)


def apply_float_colormap(image: Tensor, colormap: str = "viridis") -> Tensor:
    """colormaps.py:93-114: NaN -> 0, then "gray" repeats the value and any other map is row trunc(255 v) of its table.  Values outside [0, 1], which
    the reference refuses with an assertion, are clipped."""
    return _colors(image, ColormapOptions(colormap=colormap))


def apply_depth_colormap(depth: Tensor, accumulation: Optional[Tensor] = None, near_plane: Optional[float] = None, far_plane: Optional[float] = None,
                         colormap_options: ColormapOptions = ColormapOptions()) -> Tensor:
    """colormaps.py:117-149 -> fp32 [H,W,3]: (d - near) / (far - near + 1e-10), clipped to [0, 1], through `apply_colormap`, then
    colour * accumulation + (1 - accumulation).  near = near_plane or min(depth), far = far_plane or max(depth): as the reference's `or` has it, a
    plane of exactly 0.0 counts as "not given" and the frame's finite min / max stands in."""
    return _colors(depth, colormap_options, depth=True, accumulation=accumulation, near_plane=near_plane, far_plane=far_plane)


def compose_frame(outputs: Dict[str, Tensor], names: Sequence[str], colormap_options: ColormapOptions = ColormapOptions(),
                  depth_near_plane: Optional[float] = None, depth_far_plane: Optional[float] = None, out: Optional[Tensor] = None) -> Tensor:
    """The side-by-side frame of render.py:200-259 -> uint8 [H, k W, 3] on the device, in one launch (plus tn_frame_minmax for the panels that need
    a min / max): an output whose name contains "depth" goes through the depth rule and is blended over `accumulation_thermal` when its name contains
    "thermal" and the model gives one, else over `accumulation`; other one-channel outputs go through `apply_colormap`; three-channel outputs pass.
    Bytes are trunc(clip(c, 0, 1) 255 + 0.5), the rule of mediapy's write_image for float images -- mediapy is not installed where this was written,
    so the bytes are NOT pinned against it.  Up to 8 panels of one size.  A name the model did not give is a KeyError that lists its keys."""
    names = list(names)
    if not 1 <= len(names) <= _lib.TN_FRAME_MAX_PANELS:
        raise ValueError(f"compose_frame: {len(names)} panels (1..{_lib.TN_FRAME_MAX_PANELS})")
    images = [k for k, v in outputs.items() if isinstance(v, Tensor) and v.dim() == 3]
    for name in names:
        if name not in images:
            raise KeyError(f"compose_frame: no output {name!r}; the model gave {sorted(images)}")
    _check_colormap(colormap_options.colormap)
    dev = outputs[names[0]].device
    scratch, keep, records, size = _Scratch(dev, len(names)), [], [], None
    for name in names:
        image = outputs[name]
        depth = "depth" in name and image.shape[2] == 1
        acc = None
        if depth:
            acc = outputs.get("accumulation_thermal") if "thermal" in name else None
            acc = acc if acc is not None else outputs.get("accumulation")
        rec, H, W = _panel(image, colormap_options, scratch, depth=depth, accumulation=acc, near_plane=depth_near_plane, far_plane=depth_far_plane,
                           keep=keep)
        if size is not None and size != (H, W):
            raise ValueError(f"compose_frame: panel {name!r} is {H} x {W}, the panels before it {size[0]} x {size[1]}")
        size = (H, W)
        records.append(rec)
    H, W = size
    if out is None:
        out = torch.empty((H, len(names) * W, 3), dtype=torch.uint8, device=dev)
    compose_call(records, H, W, out)
    return out


# ---------------------------------------------------------------------------------------------------- camera paths (host, float64)
def _pose64(camera: PinholeCamera) -> np.ndarray:
    return camera.camera_to_world.detach().to("cpu", torch.float64).numpy().reshape(3, 4)


def _camera(pose: np.ndarray, fx: float, fy: float, cx: float, cy: float, width: int, height: int) -> PinholeCamera:
    return PinholeCamera(torch.from_numpy(np.ascontiguousarray(pose[:3, :4], dtype=np.float64)), float(fx), float(fy), float(cx), float(cy), int(width),
                         int(height))


def _quaternion_from_matrix(M: np.ndarray) -> np.ndarray:
    """camera_utils.py:50-102 (isprecise False): the eigenvector of the largest eigenvalue of the symmetric matrix K, w first, w >= 0."""
    (m00, m01, m02), (m10, m11, m12), (m20, m21, m22) = M[:3, :3].tolist()
    K = np.array([[m00 - m11 - m22, 0.0, 0.0, 0.0], [m01 + m10, m11 - m00 - m22, 0.0, 0.0], [m02 + m20, m12 + m21, m22 - m00 - m11, 0.0],
                  [m21 - m12, m02 - m20, m10 - m01, m00 + m11 + m22]])
    K /= 3.0
    w, V = np.linalg.eigh(K)
    q = V[np.array([3, 0, 1, 2]), np.argmax(w)]
    return -q if q[0] < 0.0 else q


def _unit(q: np.ndarray) -> np.ndarray:
    q = np.array(q, dtype=np.float64, copy=True)
    return q / math.sqrt(np.dot(q, q))


def _quaternion_slerp(quat0: np.ndarray, quat1: np.ndarray, fraction: float) -> np.ndarray:
    """camera_utils.py:105-138 (spin 0, shortest path)."""
    q0, q1 = _unit(quat0), _unit(quat1)
    if fraction == 0.0:
        return q0
    if fraction == 1.0:
        return q1
    d = np.dot(q0, q1)
    if abs(abs(d) - 1.0) < _EPS:
        return q0
    if d < 0.0:
        d, q1 = -d, -q1
    angle = math.acos(d)
    if abs(angle) < _EPS:
        return q0
    isin = 1.0 / math.sin(angle)
    return q0 * (math.sin((1.0 - fraction) * angle) * isin) + q1 * (math.sin(fraction * angle) * isin)


def _quaternion_matrix(quaternion: np.ndarray) -> np.ndarray:
    """camera_utils.py:141-160, the rotation block."""
    q = np.array(quaternion, dtype=np.float64, copy=True)
    n = np.dot(q, q)
    if n < _EPS:
        return np.identity(3)
    q *= math.sqrt(2.0 / n)
    q = np.outer(q, q)
    return np.array([[1.0 - q[2, 2] - q[3, 3], q[1, 2] - q[3, 0], q[1, 3] + q[2, 0]], [q[1, 2] + q[3, 0], 1.0 - q[1, 1] - q[3, 3], q[2, 3] - q[1, 0]],
                     [q[1, 3] - q[2, 0], q[2, 3] + q[1, 0], 1.0 - q[1, 1] - q[2, 2]]])


def ordered_poses(poses: np.ndarray, Ks: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """camera_utils.py:209-242: the reference's greedy ordering -- start at pose 0, go on to the nearest remaining position (the first of equals)."""
    order, rest = [0], list(range(1, len(poses)))
    while rest:
        last = poses[order[-1]][:, 3]
        dist = [math.sqrt(float(np.sum((last - poses[i][:, 3]) ** 2))) for i in rest]
        order.append(rest.pop(int(np.argmin(dist))))
    return poses[order], Ks[order]


def interpolated_poses_many(poses: np.ndarray, Ks: np.ndarray, steps_per_transition: int = 10, order_poses: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """camera_utils.py:163-278 in float64 (the reference rounds its result to float32): poses [n,3,4] and Ks [n,3,3] -> (n - 1) steps poses and Ks; per
    transition t = linspace(0, 1, steps), quaternion slerp of the rotations, (1 - t) a + t b of the translations, a (1 - t) + b t of the Ks.  The end
    of one transition and the start of the next are both kept, as in the reference."""
    poses, Ks = np.asarray(poses, dtype=np.float64), np.asarray(Ks, dtype=np.float64)
    if poses.ndim != 3 or poses.shape[1:] != (3, 4) or Ks.shape != (poses.shape[0], 3, 3) or poses.shape[0] < 2 or steps_per_transition < 1:
        raise ValueError(f"interpolated_poses_many: at least 2 poses [n,3,4] with Ks [n,3,3] and at least 1 step, got {poses.shape}, {Ks.shape}, "
                         f"{steps_per_transition}")
    if order_poses:
        poses, Ks = ordered_poses(poses, Ks)
    traj, k_interp = [], []
    for a in range(poses.shape[0] - 1):
        pa, pb = poses[a], poses[a + 1]
        qa, qb = _quaternion_from_matrix(pa), _quaternion_from_matrix(pb)
        for t in np.linspace(0, 1, steps_per_transition):
            pose = np.empty((3, 4))
            pose[:, :3] = _quaternion_matrix(_quaternion_slerp(qa, qb, t))
            pose[:, 3] = (1 - t) * pa[:3, 3] + t * pb[:3, 3]
            traj.append(pose)
            k_interp.append(Ks[a] * (1.0 - t) + Ks[a + 1] * t)
    return np.stack(traj), np.stack(k_interp)


def _intrinsics(camera: PinholeCamera) -> np.ndarray:
    return np.array([[camera.fx, 0.0, camera.cx], [0.0, camera.fy, camera.cy], [0.0, 0.0, 1.0]], dtype=np.float64)


def interpolated_path(cameras: Sequence[PinholeCamera], steps: int, order_poses: bool = False) -> List[PinholeCamera]:
    """camera_paths.py:30-52 (get_interpolated_camera_path): `steps` cameras per transition between consecutive cameras; fx and fy interpolated, cx, cy
    and the size those of the first camera of the (ordered) path, as the reference takes them."""
    cameras = list(cameras)
    poses, Ks = interpolated_poses_many(np.stack([_pose64(c) for c in cameras]), np.stack([_intrinsics(c) for c in cameras]), steps, order_poses)
    return [_camera(p, K[0, 0], K[1, 1], Ks[0, 0, 2], Ks[0, 1, 2], cameras[0].width, cameras[0].height) for p, K in zip(poses, Ks)]


def _linspace(start: float, end: float, steps: int) -> List[float]:
    """torch.linspace's values: from the start in the first half, from the end in the second."""
    if steps == 1:
        return [start]
    step = (end - start) / (steps - 1)
    return [start + step * i if i < steps // 2 else end - step * (steps - 1 - i) for i in range(steps)]


def _normalize(v: np.ndarray) -> np.ndarray:
    return v / math.sqrt(float(np.sum(v * v)))


def _viewmatrix(lookat: np.ndarray, up: np.ndarray, pos: np.ndarray) -> np.ndarray:
    """camera_utils.py:301-317 -> [3,4]"""
    vec2 = _normalize(lookat)
    vec0 = _normalize(np.cross(_normalize(up), vec2))
    vec1 = _normalize(np.cross(vec2, vec0))
    return np.stack([vec0, vec1, vec2, pos], 1)


def _to4x4(m: np.ndarray) -> np.ndarray:
    return np.concatenate([m, np.array([[0.0, 0.0, 0.0, 1.0]])], 0)


def spiral_path(camera: PinholeCamera, steps: int = 30, radius: Optional[float] = None, radiuses: Optional[Tuple[float, float, float]] = None,
                rots: int = 2, zrate: float = 0.5) -> List[PinholeCamera]:
    """camera_paths.py:55-120 (get_spiral_path): `steps` cameras on a spiral around `camera`, in its own frame: at theta in
    linspace(0, 2 pi rots, steps + 1)[:-1] the centre (cos theta, -sin theta, -sin(theta zrate)) * radii, looking along centre - (0, 0, -min(fx, fy)),
    up = the camera's z axis.  Exactly one of radius / radiuses."""
    if (radius is None) == (radiuses is None):
        raise ValueError("spiral_path: exactly one of radius or radiuses must be given")
    rad = np.array([radius] * 3 if radius is not None else list(radiuses), dtype=np.float64)
    if rad.shape != (3,) or steps < 1:
        raise ValueError(f"spiral_path: three radii and at least 1 step, got {rad.shape[0]} and {steps}")
    c2w = _pose64(camera)
    up = c2w[:3, 2]
    target = np.array([0.0, 0.0, -min(float(camera.fx), float(camera.fy))])
    global_h = _to4x4(c2w)
    out = []
    for theta in _linspace(0.0, 2.0 * math.pi * rots, steps + 1)[:-1]:
        center = np.array([math.cos(theta), -math.sin(theta), -math.sin(theta * zrate)]) * rad
        local_h = _to4x4(_viewmatrix(center - target, up, center))
        out.append(dataclasses.replace(camera, camera_to_world=torch.from_numpy(np.matmul(global_h, local_h)[:3, :4].copy())))
    return out


def three_js_focal_length(fov: float, image_height: float) -> float:
    """viewer_legacy/server/utils.py:52-64: (height / 2) / tan(fov (pi / 180) / 2), fov in degrees."""
    return (image_height / 2.0) / math.tan(fov * (math.pi / 180.0) / 2.0)


def path_from_json(camera_path: Dict[str, Any]) -> List[PinholeCamera]:
    """camera_paths.py:123-189 (get_path_from_json) for perspective paths: per entry of camera_path["camera_path"] the row-major 4x4
    `camera_to_world` and fx = fy = the three.js focal length of its `fov` at `render_height`; cx, cy = half the render size.  Any `camera_type`
    the reference maps to another camera model (fisheye, equirectangular, omnidirectional, vr180) raises NotImplementedError."""
    kind = camera_path.get("camera_type", "perspective")
    if str(kind).lower() in ("fisheye", "equirectangular", "omnidirectional", "vr180"):
        raise NotImplementedError(f"camera_type {kind!r}: path cameras are perspective only")
    height, width = camera_path["render_height"], camera_path["render_width"]
    out = []
    for entry in camera_path["camera_path"]:
        c2w = np.array(entry["camera_to_world"], dtype=np.float64).reshape(4, 4)[:3]
        focal = three_js_focal_length(entry["fov"], height)
        out.append(_camera(c2w, focal, focal, width / 2, height / 2, width, height))
    return out


def crop_from_json(camera_json: Dict[str, Any]) -> Optional[Tuple[OrientedBox, Tensor]]:
    """render.py:385-405 (get_crop_from_json) -> (OrientedBox.from_params(crop_center, crop_rot or zeros, crop_scale), background fp32 [3] =
    crop_bg_color / 255), or None without a crop."""
    crop = camera_json.get("crop")
    if crop is None:
        return None
    bg, center, scale = crop["crop_bg_color"], crop["crop_center"], crop["crop_scale"]
    rot = tuple(crop["crop_rot"]) if "crop_rot" in crop else (0.0, 0.0, 0.0)
    if len(center) != 3 or len(scale) != 3 or len(rot) != 3:
        raise ValueError("crop_from_json: crop_center, crop_scale and crop_rot take three numbers each")
    return OrientedBox.from_params(center, rot, scale), torch.Tensor([bg["r"] / 255.0, bg["g"] / 255.0, bg["b"] / 255.0])


# ---------------------------------------------------------------------------------------------------- the renderer
@dataclass
class _NerfCamera:
    """What ThermalNerfactoModel.get_outputs_for_camera reads of a `Cameras` object, for one PinholeCamera."""

    camera_to_worlds: Tensor
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    camera_index: int = 0


def thermal_output_name(model) -> str:
    """The model's own name for its thermal image: `thermal` (thermal splats), `rgb_thermal` (thermal-nerfacto)."""
    return "thermal" if _is_splat(model) else "rgb_thermal"


def model_outputs(model, camera: PinholeCamera, obb_box: Optional[OrientedBox] = None) -> Dict[str, Tensor]:
    """One eval frame of either model.  The splat model takes the camera and the crop as they are; the NeRF model gets the Cameras-like view of the
    camera, and its NotImplementedError for a crop is the caller's."""
    with torch.no_grad():
        if _is_splat(model):
            return model.get_outputs_for_camera(camera, obb_box=obb_box)
        view = _NerfCamera(camera.camera_to_world.detach().to(dtype=F32), camera.fx, camera.fy, camera.cx, camera.cy, camera.width, camera.height,
                           0 if camera.cam_idx is None else int(camera.cam_idx))
        return model.get_outputs_for_camera(view, obb_box=obb_box)


def _crop_box(crop) -> Optional[OrientedBox]:
    if crop is None or isinstance(crop, OrientedBox):
        return crop
    if isinstance(crop, tuple) and len(crop) == 2 and isinstance(crop[0], OrientedBox):  # what crop_from_json returns
        return crop[0]
    raise TypeError(f"crop: an OrientedBox, crop_from_json's (box, background) or None expected, got {type(crop).__name__}")


def _write_png(path: str, frame: np.ndarray) -> None:
    with open(path, "wb") as f:
        f.write(png_bytes(frame))


def render_trajectory(model, cameras: Sequence[PinholeCamera], output_dir: str, rendered_output_names: Optional[Sequence[str]] = None, crop=None,
                      colormap_options: ColormapOptions = ColormapOptions(), depth_near_plane: Optional[float] = None,
                      depth_far_plane: Optional[float] = None, rendered_resolution_scaling_factor: float = 1.0, pinned_buffers: int = 2) -> List[str]:
    """_render_trajectory_video (render.py:96-278) with output_format "images": one PNG `00000.png`, ... per camera in output_dir, each the
    side-by-side `compose_frame` of rendered_output_names (default: rgb, the model's thermal image, depth).  `crop` (an OrientedBox, or what
    crop_from_json returns) goes to the model as obb_box; the box's background colour is not applied.  rendered_resolution_scaling_factor rescales every
    camera (`rescaled_camera`).  A frame leaves the device in ONE copy, into one of `pinned_buffers` pinned host buffers: with two, frame i is
    PNG-encoded on the host while frame i + 1 renders (measured: 7 % off a thermal-nerfacto loop, nothing off a splat loop, whose render is
    1 % of the encode: profiles/render.md).  -> the paths."""
    names = list(rendered_output_names) if rendered_output_names is not None else ["rgb", thermal_output_name(model), "depth"]
    if pinned_buffers not in (1, 2):
        raise ValueError(f"render_trajectory: pinned_buffers = {pinned_buffers} (1 or 2)")
    if not rendered_resolution_scaling_factor > 0:
        raise ValueError(f"render_trajectory: rendered_resolution_scaling_factor = {rendered_resolution_scaling_factor}")
    box = _crop_box(crop)
    os.makedirs(output_dir, exist_ok=True)
    was_training = model.training
    model.eval()
    buffers: List[Optional[Tensor]] = [None] * pinned_buffers
    events = [torch.cuda.Event() for _ in range(pinned_buffers)]
    paths: List[str] = []
    pending: Optional[Tuple[int, str]] = None

    def finish(job: Tuple[int, str]) -> None:
        events[job[0]].synchronize()
        _write_png(job[1], buffers[job[0]].numpy())

    try:
        for i, camera in enumerate(cameras):
            if rendered_resolution_scaling_factor != 1.0:
                camera = rescaled_camera(camera, 1.0 / rendered_resolution_scaling_factor)
            frame = compose_frame(model_outputs(model, camera, box), names, colormap_options, depth_near_plane, depth_far_plane)
            b = i % pinned_buffers
            if buffers[b] is None or buffers[b].shape != frame.shape:
                buffers[b] = torch.empty(tuple(frame.shape), dtype=torch.uint8, pin_memory=True)
            buffers[b].copy_(frame, non_blocking=True)
            events[b].record()
            paths.append(os.path.join(output_dir, f"{i:05d}.png"))
            if pending is not None:  # (with one buffer nothing is ever pending: the frame is written before the next one is rendered)
                finish(pending)
                pending = None
            if pinned_buffers == 1:
                finish((b, paths[-1]))
            else:
                pending = (b, paths[-1])
        if pending is not None:
            finish(pending)
    finally:
        model.train(was_training)
    return paths


def render_dataset(model, cameras_and_batches, output_dir: str, names: Optional[Sequence[str]] = None,
                   colormap_options: ColormapOptions = ColormapOptions(), depth_near_plane: Optional[float] = None,
                   depth_far_plane: Optional[float] = None) -> List[str]:
    """DatasetRender (render.py:723-908) for (camera, batch) pairs: per frame i and output name one PNG output_dir/<name>/<i:05d>.png (the
    one-panel `compose_frame`); for `rgb` on a colour frame and the model's thermal image on a thermal frame also the ground truth
    batch["image"], as output_dir/gt-<name>/<i:05d>.png -- the thermal ground truth (its first channel) through the same colour map as the prediction.
    Raw (.npy.gz) outputs are not built.  -> the paths."""
    thermal = thermal_output_name(model)
    names = list(names) if names is not None else ["rgb", thermal, "depth"]
    was_training = model.training
    model.eval()
    paths: List[str] = []

    def write(name: str, i: int, frame: Tensor) -> None:
        os.makedirs(os.path.join(output_dir, name), exist_ok=True)
        paths.append(os.path.join(output_dir, name, f"{i:05d}.png"))
        _write_png(paths[-1], frame.cpu().numpy())

    try:
        for i, (camera, batch) in enumerate(cameras_and_batches):
            outputs = model_outputs(model, camera)
            dev = outputs["rgb"].device
            is_thermal = bool(torch.as_tensor(batch.get("is_thermal", camera.is_thermal)).reshape(-1)[0])
            for name in names:
                write(name, i, compose_frame(outputs, [name], colormap_options, depth_near_plane, depth_far_plane))
                if name not in ("rgb", thermal) or (name == thermal) != is_thermal or "image" not in batch:
                    continue
                gt = batch["image"]
                gt = gt.to(dev).float() / 255.0 if gt.dtype == torch.uint8 else gt.to(dev, F32)
                gt = gt[..., :1] if is_thermal else gt[..., :3]
                write(f"gt-{name}", i, compose_frame({"gt": gt.contiguous()}, ["gt"], colormap_options))
    finally:
        model.train(was_training)
    return paths
