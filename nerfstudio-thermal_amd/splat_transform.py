"""Rigid moves of thermal splats: a similarity x' = s R x + t (s > 0, R a proper rotation) applied to every Gaussian, so that the moved model seen
from the moved camera renders the same frame.  This is what puts a splat file into the dataset's own frame, where the point-cloud and mesh exports
(cloud.to_dataset_frame, mesh.mesh_to_dataset_frame), a `ply_file_path` entry and third-party tools expect the geometry, and what brings a file
trained elsewhere on the same dataset into a model's frame.

  means' = s R x + t | log scales' = scales + log s | quats' = q_R (x) q | the SH coefficients of degree 1 to 3 of both spectra, band by band,
  c'_l = M_l c_l per channel with the real-SH rotation matrices M_1 [3,3], M_2 [5,5], M_3 [7,7] of R; opacities and the DC terms do not move.

The Gaussians are moved on the device by tn_transform_splat (csrc/tn_splat_transform.hip; `splat_calls.transform_call` knows its argument order):
one launch, every value evaluated in double and rounded once, the same bits every run; there is no CPU fallback.  The host side -- `Similarity`,
`dataset_frame`, `sh_rotation_matrices`, `rotation_quaternion` -- is float64 torch on the CPU.

The band matrices are derived numerically, once per call: the 16 basis functions of tn_splat_project's sh_eval (gsplat's constants, order and signs,
restated here in float64 as `sh_basis`) are evaluated at 64 fixed, well-spread unit directions and at their images under R, and Y_l(R d) = M_l Y_l(d)
is solved per band by least squares.  No Wigner recursion, no dependency; the error is float64 round-off (1e-15).
"""
from __future__ import annotations

import dataclasses
import functools
import math
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _lib, splat_calls
from .splat_camera import OrientedBox, PinholeCamera

F64 = torch.float64
SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)
BANDS = ((1, 4), (4, 9), (9, 16))  # the coefficients of degree 1, 2, 3 among the 16
MOVED = ("means", "scales", "quats", "features_rest", "features_rest_thermal")  # the gauss_params a similarity changes
NUM_DIRECTIONS = 64


# ---------------------------------------------------------------------------------------------------- spherical harmonics and rotations (host)
def sh_basis(dirs: Tensor) -> Tensor:
    """The 16 real SH basis functions of degree 0 to 3 at unit directions [M,3] -> [M,16] float64, constants included, in the order and with the
    signs of sh_eval (csrc/tn_splat.hip): colour = sum_k basis[k] coeffs[k]."""
    d = dirs.to(F64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return torch.stack([
        torch.full_like(x, SH_C0),
        -SH_C1 * y, SH_C1 * z, -SH_C1 * x,
        SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy),
        SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4.0 * zz - xx - yy), SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy),
        SH_C3[4] * x * (4.0 * zz - xx - yy), SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3.0 * yy)], -1)


def _directions(n: int = NUM_DIRECTIONS) -> Tensor:
    """n unit directions spread evenly over the sphere (a Fibonacci spiral), float64: fixed, so the matrices of an R are the same every call."""
    i = torch.arange(n, dtype=F64)
    z = 1.0 - (2.0 * i + 1.0) / n
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    r = torch.sqrt(1.0 - z * z)
    return torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], -1)


def _rotation(R) -> Tensor:
    R = torch.as_tensor(R).detach().to("cpu", F64)
    if R.shape != (3, 3):
        raise ValueError(f"a rotation must be [3,3], got {tuple(R.shape)}")
    if float((R @ R.T - torch.eye(3, dtype=F64)).abs().max()) > 1e-9 or float(torch.linalg.det(R)) <= 0:
        raise ValueError("R is not a proper rotation (R R^T = I to 1e-9 and det R = +1); Similarity.from_matrix takes the nearest one")
    return R


def sh_rotation_matrices(R) -> Tuple[Tensor, Tensor, Tensor]:
    """(M1 [3,3], M2 [5,5], M3 [7,7]) float64 with Y_l(R d) = M_l Y_l(d) for the basis of `sh_basis`: a Gaussian whose band-l coefficients of a
    channel are c_l shows, after the scene is rotated by R, the colours of c'_l = M_l c_l.  Least squares over NUM_DIRECTIONS fixed directions.
    The matrices of an R are computed once per process and kept (a least-squares solver may differ in the last bit from call to call), so two
    moves by the same R use the same 83 numbers."""
    return tuple(M.clone() for M in _band_matrices(tuple(_rotation(R).reshape(-1).tolist())))


@functools.lru_cache(maxsize=64)
def _band_matrices(entries: Tuple[float, ...]) -> Tuple[Tensor, Tensor, Tensor]:
    R = torch.tensor(entries, dtype=F64).reshape(3, 3)
    D = _directions()
    B0, B1 = sh_basis(D), sh_basis(D @ R.T)
    # B1 = B0 M^T on every direction
    return tuple(torch.linalg.lstsq(B0[:, a:b], B1[:, a:b]).solution.T.contiguous() for a, b in BANDS)


def rotation_quaternion(R) -> Tensor:
    """The unit quaternion (w, x, y, z) of R with w >= 0, float64, by Shepperd's method: the largest of the trace and the three diagonal entries
    picks the component that is computed from a square root, the others follow by division -- no cancellation near rotations by pi."""
    m = _rotation(R).tolist()
    tr = m[0][0] + m[1][1] + m[2][2]
    pick = max(range(4), key=lambda i: tr if i == 0 else m[i - 1][i - 1])
    if pick == 0:
        w = 0.5 * math.sqrt(1.0 + tr)
        q = [w, (m[2][1] - m[1][2]) / (4 * w), (m[0][2] - m[2][0]) / (4 * w), (m[1][0] - m[0][1]) / (4 * w)]
    else:
        i = pick - 1
        j, k = (i + 1) % 3, (i + 2) % 3
        v = 0.5 * math.sqrt(1.0 + m[i][i] - m[j][j] - m[k][k])
        q = [0.0, 0.0, 0.0, 0.0]
        q[0] = (m[k][j] - m[j][k]) / (4 * v)
        q[1 + i] = v
        q[1 + j] = (m[j][i] + m[i][j]) / (4 * v)
        q[1 + k] = (m[k][i] + m[i][k]) / (4 * v)
    t = torch.tensor(q, dtype=F64)
    t = t / t.norm()
    return -t if float(t[0]) < 0 else t


# ---------------------------------------------------------------------------------------------------- the similarity
@dataclasses.dataclass(frozen=True, eq=False)
class Similarity:
    """x' = scale * R x + t, float64 on the host; scale > 0 and R a proper rotation (reflections and non-uniform scales are not represented: they
    have no quaternion, and a reflection is not a rotation of the SH bands)."""

    scale: float
    R: Tensor
    t: Tensor

    def __post_init__(self):
        s = float(self.scale)
        if not (math.isfinite(s) and s > 0):
            raise ValueError(f"Similarity: scale must be positive and finite, got {self.scale}")
        t = torch.as_tensor(self.t).detach().to("cpu", F64).reshape(-1)
        if t.shape != (3,) or not bool(torch.isfinite(t).all()):
            raise ValueError("Similarity: t must be three finite numbers")
        object.__setattr__(self, "scale", s)
        object.__setattr__(self, "R", _rotation(self.R).clone())
        object.__setattr__(self, "t", t.clone())

    @staticmethod
    def identity() -> "Similarity":
        return Similarity(1.0, torch.eye(3, dtype=F64), torch.zeros(3, dtype=F64))

    @staticmethod
    def from_matrix(T) -> "Similarity":
        """From a [3,4] or [4,4] matrix [A | t] whose linear part is s R.  s = det(A)^(1/3); ValueError when det <= 0 (a reflection) or when
        max-row-sum |A^T A / s^2 - I| > 1e-6 (a shear or a non-uniform scale).  R is the rotation nearest to A / s (its polar factor), so `matrix()`
        gives the input back to that tolerance."""
        T = torch.as_tensor(T).detach().to("cpu", F64)
        if tuple(T.shape) not in ((3, 4), (4, 4)):
            raise ValueError(f"Similarity.from_matrix: a [3,4] or [4,4] matrix expected, got {tuple(T.shape)}")
        if T.shape[0] == 4 and float((T[3] - torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=F64)).abs().max()) > 1e-12:
            raise ValueError("Similarity.from_matrix: the last row of a [4,4] matrix must be 0 0 0 1")
        A, t = T[:3, :3], T[:3, 3]
        det = float(torch.linalg.det(A))
        if not math.isfinite(det) or det <= 0:
            raise ValueError(f"Similarity.from_matrix: det = {det:.3g}: reflections (and singular matrices) are not represented")
        s = det ** (1.0 / 3.0)
        off = float((A.T @ A / (s * s) - torch.eye(3, dtype=F64)).abs().sum(-1).max())
        if not off <= 1e-6:
            raise ValueError(f"Similarity.from_matrix: the linear part is not scale * rotation (|A^T A / s^2 - I| = {off:.3g}): shears and "
                             "non-uniform scales are not represented")
        U, _, Vh = torch.linalg.svd(A / s)
        return Similarity(s, U @ Vh, t)

    @property
    def is_identity(self) -> bool:
        return self.scale == 1.0 and bool((self.R == torch.eye(3, dtype=F64)).all()) and not bool(self.t.any())

    def matrix(self) -> Tensor:
        """[3,4] float64: [scale R | t]."""
        return torch.cat([self.scale * self.R, self.t[:, None]], 1)

    def inverse(self) -> "Similarity":
        return Similarity(1.0 / self.scale, self.R.T, -(self.R.T @ self.t) / self.scale)

    def compose(self, other: "Similarity") -> "Similarity":
        """self after other: x -> self(other(x))."""
        return Similarity(self.scale * other.scale, self.R @ other.R, self.scale * (self.R @ other.t) + self.t)

    def apply_points(self, xyz: Tensor) -> Tensor:
        """[n,3] points -> their images, on the tensor's device and in its dtype: evaluated in float64 as tn_transform_splat evaluates the means,
        ((A_i0 x + A_i1 y) + A_i2 z) + t_i with A = scale R, and rounded once."""
        if xyz.dim() != 2 or xyz.shape[1] != 3:
            raise ValueError(f"apply_points: [n,3] points expected, got {tuple(xyz.shape)}")
        A, t = (self.scale * self.R).tolist(), self.t.tolist()
        p = xyz.detach().to(F64)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        out = torch.stack([((A[i][0] * x + A[i][1] * y) + A[i][2] * z) + t[i] for i in range(3)], -1)
        return out.to(xyz.dtype if xyz.is_floating_point() else torch.float32)

    def apply_camera(self, camera: PinholeCamera) -> PinholeCamera:
        """The camera that sees the moved scene as `camera` sees the original: rotation R c2w_R, position scale R c2w_t + t (float64, rounded once to
        the pose's dtype); intrinsics, size, cam_idx and is_thermal are kept."""
        c2w = camera.camera_to_world
        c = c2w.detach().to("cpu", F64)
        new = torch.cat([self.R @ c[:3, :3], (self.scale * (self.R @ c[:3, 3]) + self.t)[:, None]], 1)
        if c.shape[0] == 4:
            new = torch.cat([new, c[3:]], 0)
        return dataclasses.replace(camera, camera_to_world=new.to(device=c2w.device, dtype=c2w.dtype))

    def apply_box(self, box: OrientedBox) -> OrientedBox:
        """The box that holds the images of the points `box` holds: R' = R R_box, T' = scale R T + t, S' = scale S.  A point within rounding of a
        face may fall on the other side of the moved face."""
        bR, bT, bS = (torch.as_tensor(v).detach() for v in (box.R, box.T, box.S))
        R, T, S = bR.to("cpu", F64), bT.to("cpu", F64), bS.to("cpu", F64)
        return OrientedBox(R=(self.R @ R).to(bR.dtype), T=(self.scale * (self.R @ T) + self.t).to(bT.dtype), S=(self.scale * S).to(bS.dtype))


def dataset_frame(dataparser_outputs, applied_transform=None) -> Similarity:
    """The map from the model's frame to the dataset's own frame (the reference's save_world_frame), the same map as cloud.to_dataset_frame: the
    inverse of what the dataparser applies (`dataparser_transform` [3,4], then `dataparser_scale`).  `applied_transform` [3,4] is the transforms.json
    entry of that name, if the dataset has one; it is taken out exactly as cloud.to_dataset_frame takes it out.  `dataset_frame(...).inverse()`
    brings dataset-frame geometry (a splat file, the points of a `ply_file_path`) into the model's frame.  ValueError when the dataparser's
    transform is not a rotation and a translation (times a uniform scale)."""
    last = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=F64)
    T = torch.as_tensor(dataparser_outputs.dataparser_transform).detach().to("cpu", F64)
    T4 = torch.cat([T[:3, :4], last], 0)
    if applied_transform is not None:
        A = torch.as_tensor(applied_transform).detach().to("cpu", F64)
        T4 = T4 @ torch.linalg.inv(torch.cat([A[:3, :4], last], 0))
    inv = torch.linalg.inv(T4)[:3]
    return Similarity.from_matrix(torch.cat([inv[:, :3] / float(dataparser_outputs.dataparser_scale), inv[:, 3:]], 1))


# ---------------------------------------------------------------------------------------------------- the Gaussians (device)
def transform_struct(T: Similarity) -> _lib.TnSplatTransform:
    """`T` as tn_transform_splat takes it: A = scale R, t, log scale, the quaternion of R and its three SH band matrices, doubles."""
    s = _lib.TnSplatTransform()
    s.A[:] = (T.scale * T.R).reshape(-1).tolist()
    s.t[:] = T.t.tolist()
    s.log_scale = math.log(T.scale)
    s.q[:] = rotation_quaternion(T.R).tolist()
    for name, M in zip(("sh1", "sh2", "sh3"), sh_rotation_matrices(T.R)):
        getattr(s, name)[:] = M.reshape(-1).tolist()
    return s


def transform_gaussians(params: Dict[str, Tensor], T: Similarity, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """`params` (gauss_params tensors on the device: at least means, scales [N,3], quats [N,4], features_rest [N,R,3], features_rest_thermal
    [N,R,1], contiguous float32, R in 0, 3, 8, 15) moved by `T`: a dict with new tensors for those five and every other entry (features_dc,
    features_dc_thermal, opacities, opacities_thermal) as the same tensor object.  `out` names the five destinations; `out=params` moves in place
    (each destination must be its own source or overlap no tensor of the call).  `T.is_identity` returns the inputs without a launch.  One launch on
    the current stream, no host synchronisation."""
    missing = [k for k in MOVED if k not in params]
    if missing:
        raise ValueError(f"transform_gaussians: params lack {missing}")
    if T.is_identity:
        return dict(params)
    src = [params[k].detach() for k in MOVED]
    if out is None:
        src = [t.contiguous() for t in src]
        dst = [torch.empty_like(t) for t in src]
    else:
        dst = [out[k].detach() for k in MOVED]
    if src[0].shape[0] > 0:
        splat_calls.transform_call(transform_struct(T), *src, *dst)
    return {**params, **dict(zip(MOVED, dst if out is None else [out[k] for k in MOVED]))}


def transform_model(model, T: Similarity) -> None:
    """Move a ThermalSplatfactoModel by `T` in place: its Gaussians (transform_gaussians, then model.load_gaussians) and its crop box
    (`T.apply_box`); cameras are the caller's to move (`T.apply_camera`).  For trained or loaded models: load_gaussians makes new parameters, so
    optimiser moments are not carried along (an optimiser built on the old parameters goes stale and must be rebuilt -- the model holds no reference
    to its optimisers, so this cannot be detected here), and pose-optimiser rows and refinement statistics are left as they are."""
    if T.is_identity:
        return
    with torch.no_grad():
        model.load_gaussians(transform_gaussians({k: model.gauss_params[k].detach() for k in model.param_names}, T))
    if model.crop_box is not None:
        model.crop_box = T.apply_box(model.crop_box)
