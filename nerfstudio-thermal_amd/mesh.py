"""An RGB+thermal triangle mesh from a trained model, on the device: the counterpart of `ns-export tsdf` (nerfstudio/exporter/tsdf_utils.py:
TSDF.from_aabb, integrate_tsdf, get_mesh, export_tsdf_mesh).

Every training camera is rendered (depth, accumulation, RGB and thermal), the frames are fused into a truncated signed distance volume that carries
a colour and a temperature per voxel (tn_tsdf_integrate: one launch per batch of frames, a thread per voxel, no [B,*,N] temporaries), and the zero
level of the volume is extracted as an indexed mesh with a normal, a colour and a temperature per vertex (tn_mesh_count / tn_mesh_emit: marching
tetrahedra on the Freudenthal split of each cell, ordered by prefix sums).  The reference extracts with skimage's marching cubes and writes with
pymeshlab; neither is used here, and the triangulation is not theirs.

Two deliberate additions to the reference's fusion: `depth_kind` ("ray": Euclidean distances, the reference's rule and a NeRF's depth; "z": camera z,
a rasteriser's depth) and voxels behind a camera (camera z <= 0) are skipped, where the reference divides by that z and mirrors them into the image.

Where the reference then decimates the mesh to a face budget with pymeshlab's edge collapse, `simplify_mesh` / `simplify_to_target` cluster the
vertices on a regular grid (tn_mesh_simplify_count / _plan / _emit: sorts and prefix sums, a quadric solve per cluster); `export_tsdf_mesh` runs it
when given target_num_faces.

The raw calls are `integrate_call`, `mesh_count_call`, `mesh_emit_call`, `simplify_count_call`, `simplify_plan_call` and `simplify_emit_call`, the only
places that know the argument order of their entry points (include/thermal_nerf_hip.h).  Everything runs on torch's current stream; there is no CPU
fallback.
"""
from __future__ import annotations

import ctypes as C
import types
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .cloud import _contig, _dev, to_dataset_frame, to_uint8
from .ops import _stream
from .splat_camera import PinholeCamera, rescaled_camera

F32 = torch.float32
DEPTH_KINDS = ("z", "ray")  # the entry point's ray_depth flag


@dataclass
class Mesh:
    """vertices [V,3] in world units, faces [F,3] int32 (wound so that the normal points out of the surface), normals [V,3] (unit length, or zero
    where the volume is flat), colors [V,3] and thermal [V,1] in 0..1; fp32 on the device.  colors and thermal are views of `rgbt` [V,4]."""

    vertices: Tensor
    faces: Tensor
    normals: Tensor
    rgbt: Tensor

    @property
    def colors(self) -> Tensor:
        return self.rgbt[:, :3]

    @property
    def thermal(self) -> Tensor:
        return self.rgbt[:, 3:]


# ---------------------------------------------------------------------------------------------------- the raw calls
def camera_records(cameras: Sequence[PinholeCamera], device) -> Tensor:
    """[B,16] fp32 on the device: the rows of the 3x4 world -> camera matrix of each camera (nerfstudio's convention, as camera_to_world has it),
    then fx fy cx cy.  The inverse is the analytic one of a rigid pose, [R^T | -R^T t], evaluated on the host in float64 and rounded once."""
    rec = torch.empty((len(cameras), 16), dtype=torch.float64)
    for b, cam in enumerate(cameras):
        c2w = torch.as_tensor(cam.camera_to_world).detach().to("cpu", torch.float64)[:3, :4]
        Rt = c2w[:, :3].T
        rec[b, :12] = torch.cat([Rt, -Rt @ c2w[:, 3:4]], dim=1).reshape(-1)
        rec[b, 12:] = torch.tensor([float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy)], dtype=torch.float64)
    return rec.float().to(device)


def integrate_call(values: Tensor, weights: Tensor, rgbt: Tensor, origin: Sequence[float], voxel_size: Sequence[float], truncation: float,
                   max_weight: float, depth: Tensor, frame_rgbt: Tensor, accumulation: Optional[Tensor], min_accumulation: float, records: Tensor,
                   ray_depth: bool) -> None:
    """tn_tsdf_integrate of depth [B,H,W], frame_rgbt [B,H,W,4], accumulation [B,H,W] or None and records [B,16] into the volume, in place."""
    X, Y, Z = values.shape
    B, H, W = depth.shape
    rc = _lib.load().tn_tsdf_integrate(
        _contig(values, "values", (X, Y, Z)), _contig(weights, "weights", (X, Y, Z)), _contig(rgbt, "volume rgbt", (X, Y, Z, 4)), X, Y, Z,
        *(float(v) for v in origin), *(float(v) for v in voxel_size), float(truncation), float(max_weight), _contig(depth, "depth", (B, H, W)),
        _contig(frame_rgbt, "rgbt", (B, H, W, 4)), None if accumulation is None else _contig(accumulation, "accumulation", (B, H, W)),
        float(min_accumulation), _contig(records, "camera records", (B, 16)), B, H, W, int(bool(ray_depth)), _stream())
    _lib.check(rc, "tn_tsdf_integrate")


def mesh_workspace(dims: Tuple[int, int, int], device) -> Tensor:
    need = int(_lib.load().tn_mesh_workspace_bytes(*dims))
    if need < 0:
        raise ValueError(f"tn_mesh_workspace_bytes{tuple(dims)}: sizes the library refuses")
    return torch.empty(max(need, 1), dtype=torch.uint8, device=device)


def mesh_count_call(values: Tensor, weights: Tensor, observed_only: bool, totals: Tensor, workspace: Tensor) -> None:
    """tn_mesh_count: the numbers of vertices and faces into `totals` (device int64 [2]); `workspace` (mesh_workspace) then holds what
    mesh_emit_call needs."""
    X, Y, Z = values.shape
    rc = _lib.load().tn_mesh_count(_contig(values, "values", (X, Y, Z)), _contig(weights, "weights", (X, Y, Z)), X, Y, Z, int(bool(observed_only)),
                                   _contig(totals, "totals", (2,), torch.int64), C.c_void_p(workspace.data_ptr()), workspace.numel(), _stream())
    _lib.check(rc, "tn_mesh_count")


def mesh_emit_call(values: Tensor, weights: Tensor, rgbt: Tensor, observed_only: bool, origin: Sequence[float], voxel_size: Sequence[float],
                   vertices: Tensor, normals: Tensor, out_rgbt: Tensor, faces: Tensor, workspace: Tensor) -> None:
    """tn_mesh_emit after mesh_count_call on the same volume and workspace: vertices / normals [V,3], out_rgbt [V,4], faces [F,3] int32."""
    X, Y, Z = values.shape
    V, Fn = vertices.shape[0], faces.shape[0]
    rc = _lib.load().tn_mesh_emit(
        _contig(values, "values", (X, Y, Z)), _contig(weights, "weights", (X, Y, Z)), _contig(rgbt, "volume rgbt", (X, Y, Z, 4)), X, Y, Z,
        int(bool(observed_only)), *(float(v) for v in origin), *(float(v) for v in voxel_size), _contig(vertices, "vertices", (V, 3)),
        _contig(normals, "normals", (V, 3)), _contig(out_rgbt, "vertex rgbt", (V, 4)), V, _contig(faces, "faces", (Fn, 3), torch.int32), Fn,
        C.c_void_p(workspace.data_ptr()), workspace.numel(), _stream())
    _lib.check(rc, "tn_mesh_emit")


def simplify_workspace(num_vertices: int, num_faces: int, device) -> Tensor:
    need = int(_lib.load().tn_mesh_simplify_workspace_bytes(int(num_vertices), int(num_faces)))
    if need < 0:
        raise ValueError(f"tn_mesh_simplify_workspace_bytes({num_vertices}, {num_faces}): sizes the library refuses")
    return torch.empty(max(need, 1), dtype=torch.uint8, device=device)


def _simplify_mesh_args(vertices: Tensor, faces: Tensor):
    V, Fn = vertices.shape[0], faces.shape[0]
    return _contig(vertices, "vertices", (V, 3)), V, _contig(faces, "faces", (Fn, 3), torch.int32), Fn


def _simplify_grid_args(origin: Sequence[float], cell: Sequence[float], dims: Sequence[int]):
    return [float(v) for v in origin] + [float(v) for v in cell] + [int(v) for v in dims]


def simplify_count_call(vertices: Tensor, faces: Tensor, origin: Sequence[float], cell: Sequence[float], dims: Sequence[int], count: Tensor,
                        workspace: Tensor) -> None:
    """tn_mesh_simplify_count: into `count` (device int64 [1]) the number of faces whose corners fall into three different cells of the grid."""
    rc = _lib.load().tn_mesh_simplify_count(*_simplify_mesh_args(vertices, faces), *_simplify_grid_args(origin, cell, dims),
                                            _contig(count, "count", (1,), torch.int64), C.c_void_p(workspace.data_ptr()), workspace.numel(), _stream())
    _lib.check(rc, "tn_mesh_simplify_count")


def simplify_plan_call(vertices: Tensor, faces: Tensor, origin: Sequence[float], cell: Sequence[float], dims: Sequence[int], totals: Tensor,
                       workspace: Tensor) -> None:
    """tn_mesh_simplify_plan: the numbers of vertices and faces of the simplified mesh into `totals` (device int64 [2]); `workspace`
    (simplify_workspace) then holds what simplify_emit_call needs."""
    rc = _lib.load().tn_mesh_simplify_plan(*_simplify_mesh_args(vertices, faces), *_simplify_grid_args(origin, cell, dims),
                                           _contig(totals, "totals", (2,), torch.int64), C.c_void_p(workspace.data_ptr()), workspace.numel(), _stream())
    _lib.check(rc, "tn_mesh_simplify_plan")


def simplify_emit_call(vertices: Tensor, normals: Tensor, rgbt: Tensor, faces: Tensor, origin: Sequence[float], cell: Sequence[float],
                       dims: Sequence[int], regularization: float, out_vertices: Tensor, out_normals: Tensor, out_rgbt: Tensor, out_faces: Tensor,
                       workspace: Tensor) -> None:
    """tn_mesh_simplify_emit after simplify_plan_call on the same mesh, grid and workspace: out_vertices / out_normals [Vo,3], out_rgbt [Vo,4],
    out_faces [Fo,3] int32."""
    V, Fn, Vo, Fo = vertices.shape[0], faces.shape[0], out_vertices.shape[0], out_faces.shape[0]
    rc = _lib.load().tn_mesh_simplify_emit(
        _contig(vertices, "vertices", (V, 3)), _contig(normals, "normals", (V, 3)), _contig(rgbt, "vertex rgbt", (V, 4)), V,
        _contig(faces, "faces", (Fn, 3), torch.int32), Fn, *_simplify_grid_args(origin, cell, dims), float(regularization),
        _contig(out_vertices, "simplified vertices", (Vo, 3)), _contig(out_normals, "simplified normals", (Vo, 3)),
        _contig(out_rgbt, "simplified rgbt", (Vo, 4)), Vo, _contig(out_faces, "simplified faces", (Fo, 3), torch.int32), Fo,
        C.c_void_p(workspace.data_ptr()), workspace.numel(), _stream())
    _lib.check(rc, "tn_mesh_simplify_emit")


# ---------------------------------------------------------------------------------------------------- simplification
MAX_CELLS = 2 ** 31  # a grid holds fewer cells than this (the keys are 31 bits)


def _triple(v, name: str) -> np.ndarray:
    """A number or three -> fp32 [3], as the entry points take them."""
    a = np.asarray(v.detach().cpu().numpy() if isinstance(v, Tensor) else v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3 or not np.isfinite(a).all():
        raise ValueError(f"{name} = {v!r}: one finite number or three")
    return a.astype(np.float32)


def vertex_extent(vertices: Tensor) -> np.ndarray:
    """[2,3] fp32 on the host: the smallest and largest coordinate per axis (zeros for no vertices).  One read-back."""
    if vertices.shape[0] == 0:
        return np.zeros((2, 3), dtype=np.float32)
    return torch.stack([vertices.amin(dim=0), vertices.amax(dim=0)]).cpu().numpy()


def simplify_grid(extent: np.ndarray, cell: np.ndarray, origin: Optional[np.ndarray] = None) -> Tuple[np.ndarray, Tuple[int, int, int]]:
    """The cell grid over `extent` (vertex_extent): origin (fp32 [3]; without one the smallest coordinates minus half a cell, in fp32) and dims, one
    more than the cell index of the largest coordinates -- the entry points' own fp32 expression floor((v - origin) / cell), so no vertex is clamped
    from above.  A dims product of MAX_CELLS or more is for the caller to refuse."""
    if origin is None:
        origin = extent[0] - cell * np.float32(0.5)
    with np.errstate(over="ignore", invalid="ignore"):
        top = np.floor((extent[1] - origin) / cell).astype(np.float64)
    top = np.where(top > 0, np.minimum(top, float(MAX_CELLS)), 0.0)  # (a NaN goes to 0, as in the kernel)
    return origin, tuple(int(t) + 1 for t in top)


def simplify_mesh(mesh: Mesh, cell, origin=None, dims: Optional[Sequence[int]] = None, regularization: float = 1e-3,
                  workspace: Optional[Tensor] = None) -> Mesh:
    """`mesh` with the vertices of every cell of a regular grid merged into one (vertex clustering; tn_mesh_simplify_plan / tn_mesh_simplify_emit,
    whose source states the algorithm): the new vertex minimises the summed squared distances to the planes of the cluster's faces, weighted by their
    squared areas and regularised towards the cluster's mean (`regularization` times the quadric's trace); it is the mean where that point leaves the
    cell.  RGB+T is the cluster's mean, the normal its normalised normal sum.  Faces that collapse are dropped, of those that name the same three
    clusters the first stays; vertices no face names are dropped.  `cell` is a size or three, in the mesh's units; without `origin` the grid starts
    half a cell below the smallest coordinates, without `dims` it reaches the largest.  Not an edge collapse, and no manifold guarantee: clustering
    cannot give one.  Two read-backs (the extent, when the grid is not given in full; the two sizes)."""
    dev = mesh.vertices.device
    V, Fn = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    cell3 = _triple(cell, "cell")
    if not (cell3 > 0).all():
        raise ValueError(f"simplify_mesh: cell = {cell!r} must be positive")
    origin3 = None if origin is None else _triple(origin, "origin")
    if origin3 is None or dims is None:
        origin3, grid_dims = simplify_grid(vertex_extent(mesh.vertices), cell3, origin3)
        dims = grid_dims if dims is None else dims
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] >= MAX_CELLS:
        raise ValueError(f"simplify_mesh: a grid of {dims} cells (three sizes >= 1, below 2^31 cells in all): the cell is too small for the mesh")
    ws = simplify_workspace(V, Fn, dev) if workspace is None else workspace
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    simplify_plan_call(mesh.vertices, mesh.faces, origin3, cell3, dims, totals, ws)
    Vo, Fo = (int(v) for v in totals.tolist())
    out = Mesh(torch.empty((Vo, 3), dtype=F32, device=dev), torch.empty((Fo, 3), dtype=torch.int32, device=dev),
               torch.empty((Vo, 3), dtype=F32, device=dev), torch.empty((Vo, 4), dtype=F32, device=dev))
    simplify_emit_call(mesh.vertices, mesh.normals, mesh.rgbt, mesh.faces, origin3, cell3, dims, regularization, out.vertices, out.normals, out.rgbt,
                       out.faces, ws)
    return out


SEARCH_START, SEARCH_BISECTIONS, SEARCH_MAX_DOUBLINGS = 0.25, 12, 64


def search_cell(scale: float, unit: np.ndarray) -> np.ndarray:
    """cell = scale * unit in float64, rounded to fp32 once"""
    return (np.float64(scale) * unit.astype(np.float64)).astype(np.float32)


def simplify_to_target(mesh: Mesh, target_num_faces: int, unit, origin=None, regularization: float = 1e-3) -> Tuple[Mesh, Optional[Tuple[float, ...]]]:
    """`mesh` simplified to at most `target_num_faces` faces -> (Mesh, the cell used, three floats; None where the mesh is returned as it is because it
    has no more faces than that).  The cell is s * `unit` (the voxel size of the volume the mesh came from; a number or three).  tn_mesh_simplify_count
    gives, per cell size, the faces whose corners lie in three different cells -- an upper bound of the simplified mesh's faces: s starts at 1/4 and
    doubles until that count is within the target (a grid of 2^31 cells or more counts as over it), then 12 bisections on the geometric mean of the
    bracket (s / 2, s) narrow it, and the mesh is simplified at the bracket's upper end, so its face count is within the target by construction.
    One read-back per step; the same mesh gives the same cell."""
    target = int(target_num_faces)
    if target < 0:
        raise ValueError(f"simplify_to_target: target_num_faces = {target_num_faces}")
    V, Fn = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    if Fn <= target:
        return mesh, None
    dev = mesh.vertices.device
    unit3 = _triple(unit, "unit")
    if not (unit3 > 0).all():
        raise ValueError(f"simplify_to_target: unit = {unit!r} must be positive")
    origin3 = None if origin is None else _triple(origin, "origin")
    extent = vertex_extent(mesh.vertices)
    ws = simplify_workspace(V, Fn, dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def within(scale: float) -> bool:
        cell = search_cell(scale, unit3)
        o, dims = simplify_grid(extent, cell, origin3)
        if not (cell > 0).all() or dims[0] * dims[1] * dims[2] >= MAX_CELLS:
            return False
        simplify_count_call(mesh.vertices, mesh.faces, o, cell, dims, count, ws)
        return int(count.item()) <= target

    hi = SEARCH_START
    for _ in range(SEARCH_MAX_DOUBLINGS):
        if within(hi):
            break
        hi *= 2.0
    else:
        raise ValueError(f"simplify_to_target: no cell up to {hi} units brings the mesh to {target} faces")
    lo = hi / 2.0
    for _ in range(SEARCH_BISECTIONS):
        mid = float(np.sqrt(np.float64(lo) * np.float64(hi)))
        if within(mid):
            hi = mid
        else:
            lo = mid
    cell = search_cell(hi, unit3)
    o, dims = simplify_grid(extent, cell, origin3)
    return simplify_mesh(mesh, cell, origin=o, dims=dims, regularization=regularization, workspace=ws), tuple(float(c) for c in cell)


# ---------------------------------------------------------------------------------------------------- the volume
class TSDFVolume:
    """The reference's TSDF (tsdf_utils.py:41-275) with a fourth, thermal channel: `values` [X,Y,Z] start at -1, `weights` [X,Y,Z] at 0, `rgbt`
    [X,Y,Z,4] at 0 (`colors` and `thermal` are views of it), fp32 on the device, z fastest.  Voxel (i, j, k) sits at origin + (i, j, k) * voxel_size
    and voxel_size = (aabb[1] - aabb[0]) / volume_dims, both rounded to fp32 as the reference's tensors are.  truncation = voxel_size[0] *
    truncation_margin, as the reference has it."""

    def __init__(self, origin: Tensor, voxel_size: Tensor, volume_dims: Sequence[int], truncation_margin: float = 5.0, max_weight: float = 1.0,
                 device="cuda"):
        dims = tuple(int(v) for v in volume_dims)
        if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] >= 2 ** 31:
            raise ValueError(f"TSDFVolume: volume_dims = {dims} (three sizes >= 1, below 2^31 voxels in all)")
        if not (float(truncation_margin) > 0 and float(max_weight) > 0):
            raise ValueError(f"TSDFVolume: truncation_margin = {truncation_margin} and max_weight = {max_weight} must be positive")
        self.origin = torch.as_tensor(origin).detach().to("cpu", F32).reshape(3)
        self.voxel_size = torch.as_tensor(voxel_size).detach().to("cpu", F32).reshape(3)
        if not bool((self.voxel_size > 0).all()):
            raise ValueError(f"TSDFVolume: voxel_size = {self.voxel_size.tolist()} must be positive")
        self.dims, self.truncation_margin, self.max_weight = dims, float(truncation_margin), float(max_weight)
        self.values = torch.full(dims, -1.0, dtype=F32, device=device)
        self.weights = torch.zeros(dims, dtype=F32, device=device)
        self.rgbt = torch.zeros(dims + (4,), dtype=F32, device=device)

    @staticmethod
    def from_aabb(aabb, volume_dims: Sequence[int], truncation_margin: float = 5.0, max_weight: float = 1.0, device="cuda") -> "TSDFVolume":
        """TSDF.from_aabb (tsdf_utils.py:88-114): aabb [[xmin, ymin, zmin], [xmax, ymax, zmax]]; max_weight 1 is the reference (the weight is
        clamped to 1: a running half-and-half average that depends on the frame order), a large max_weight the usual running mean."""
        aabb = torch.as_tensor(aabb).detach().to("cpu", F32).reshape(2, 3)
        dims = torch.tensor([int(v) for v in volume_dims])
        return TSDFVolume(aabb[0], (aabb[1] - aabb[0]) / dims, volume_dims, truncation_margin, max_weight, device)

    @property
    def device(self):
        return self.values.device

    @property
    def colors(self) -> Tensor:
        return self.rgbt[..., :3]

    @property
    def thermal(self) -> Tensor:
        return self.rgbt[..., 3:]

    @property
    def truncation(self) -> float:
        return float(self.voxel_size[0]) * self.truncation_margin

    def integrate(self, cameras: Sequence[PinholeCamera], depth: Tensor, rgbt: Tensor, accumulation: Optional[Tensor] = None,
                  min_accumulation: float = 0.5, depth_kind: str = "ray") -> None:
        """integrate_tsdf (tsdf_utils.py:173-275) of B frames in the order given, one launch: depth [B,H,W] or [B,H,W,1], rgbt [B,H,W,4]
        channel-last (RGB + thermal, as the renders produce it), accumulation [B,H,W] or [B,H,W,1] or None.  Per frame a voxel takes the nearest
        pixel of its projection (grid_sample's nearest, align_corners False, zero padding); with dist = sampled depth - voxel depth it is updated
        where voxel depth > 0, sampled depth > 0 and dist > -truncation: value = (value w + clamp(dist / truncation, -1, 1)) / (w + 1), the same
        for the four channels, w = min(w + 1, max_weight).  A pixel with accumulation < min_accumulation counts as depth 0, no observation (a splat
        depth image fills uncovered pixels with the image's maximum).  depth_kind "ray" compares distances from the camera centre (the reference;
        a NeRF's depth), "z" camera z (the splat rasteriser's depth).  A voxel behind the camera (z <= 0) is skipped.  Voxels no frame observes
        keep their bits, so any split of the frames into calls gives the same volume."""
        if depth_kind not in DEPTH_KINDS:
            raise ValueError(f"integrate: depth_kind = {depth_kind!r}, one of {DEPTH_KINDS}")
        B = len(cameras)
        _dev(depth, "depth"), _dev(rgbt, "rgbt")
        if depth.dim() == 4 and depth.shape[-1] == 1:
            depth = depth[..., 0]
        if depth.dim() != 3 or depth.shape[0] != B:
            raise ValueError(f"integrate: depth must be [{B},H,W], got {tuple(depth.shape)}")
        H, W = int(depth.shape[1]), int(depth.shape[2])
        if tuple(rgbt.shape) != (B, H, W, 4):
            raise ValueError(f"integrate: rgbt must be [{B},{H},{W},4], got {tuple(rgbt.shape)}")
        if accumulation is not None:
            _dev(accumulation, "accumulation")
            if accumulation.dim() == 4 and accumulation.shape[-1] == 1:
                accumulation = accumulation[..., 0]
            if tuple(accumulation.shape) != (B, H, W):
                raise ValueError(f"integrate: accumulation must be [{B},{H},{W}], got {tuple(accumulation.shape)}")
            accumulation = accumulation.contiguous()
        if B == 0:
            return
        integrate_call(self.values, self.weights, self.rgbt, self.origin.tolist(), self.voxel_size.tolist(), self.truncation, self.max_weight,
                       depth.contiguous(), rgbt.contiguous(), accumulation, min_accumulation, camera_records(cameras, self.device), depth_kind == "ray")

    def get_mesh(self, observed_only: bool = False) -> Mesh:
        """The zero level of clamp(values, -1, 1) as an indexed mesh (values < 0 are inside; normals and winding point to the positive side).  A
        vertex sits on a lattice edge at the linear zero, its normal is the interpolated, normalised gradient of the clamped values, its colour and
        temperature those of the nearer end of its edge (of the other where that end was never observed).  observed_only False is the reference:
        the whole volume, the unobserved -1 fill included, which closes observed free space with a shell; True drops every cell with an unobserved
        corner.  One host synchronisation, for the two sizes."""
        dev = self.device
        ws = mesh_workspace(self.dims, dev)
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        mesh_count_call(self.values, self.weights, observed_only, totals, ws)
        V, Fn = (int(v) for v in totals.tolist())
        if V >= 2 ** 31:
            raise ValueError(f"get_mesh: {V} vertices do not fit the faces' int32 indices")
        mesh = Mesh(torch.empty((V, 3), dtype=F32, device=dev), torch.empty((Fn, 3), dtype=torch.int32, device=dev),
                    torch.empty((V, 3), dtype=F32, device=dev), torch.empty((V, 4), dtype=F32, device=dev))
        mesh_emit_call(self.values, self.weights, self.rgbt, observed_only, self.origin.tolist(), self.voxel_size.tolist(), mesh.vertices,
                       mesh.normals, mesh.rgbt, mesh.faces, ws)
        return mesh


# ---------------------------------------------------------------------------------------------------- the export
def _is_splat(model) -> bool:
    return hasattr(model, "gauss_params")


def render_frame(model, camera: PinholeCamera) -> Tuple[Tensor, Tensor, Tensor, str]:
    """One eval render of `camera` through the model's get_outputs_for_camera -> (depth [H,W], accumulation [H,W], rgbt [H,W,4], depth kind).
    Thermal splats: rgb + `thermal`, z depth (the model's crop box is handed back to the call, so it stays what it was).  Thermal-nerfacto:
    rgb + `rgb_thermal`, ray depth; depth and accumulation are the RGB branch's in both density modes, as in the point-cloud export."""
    if _is_splat(model):
        out = model.get_outputs_for_camera(camera, obb_box=model.crop_box)
        thermal, kind = out["thermal"], "z"
    else:
        cam = types.SimpleNamespace(camera_to_worlds=torch.as_tensor(camera.camera_to_world)[:3, :4], fx=camera.fx, fy=camera.fy, cx=camera.cx,
                                    cy=camera.cy, width=camera.width, height=camera.height,
                                    camera_index=0 if camera.cam_idx is None else int(camera.cam_idx))
        out = model.get_outputs_for_camera(cam)
        thermal, kind = out["rgb_thermal"], "ray"
    H, W = int(camera.height), int(camera.width)
    rgb = out["rgb"]
    if (rgb.stride() == (4 * W, 4, 1) and thermal.stride() == (4 * W, 4, 1) and thermal.data_ptr() == rgb.data_ptr() + 3 * rgb.element_size()
            and rgb.untyped_storage().data_ptr() == thermal.untyped_storage().data_ptr()):
        rgbt = rgb.as_strided((H, W, 4), (4 * W, 4, 1))  # the rasteriser's own [H,W,4] buffer
    else:
        rgbt = torch.cat([rgb.reshape(H, W, 3), thermal.reshape(H, W, 1)], dim=-1)
    return out["depth"].reshape(H, W).float(), out["accumulation"].reshape(H, W).float(), rgbt.float(), kind


def export_tsdf_mesh(model, cameras: Sequence[PinholeCamera], resolution: Union[int, Sequence[int]] = 256, downscale_factor: int = 2,
                     batch_size: int = 10, use_bounding_box: bool = True, bounding_box_min: Sequence[float] = (-1.0, -1.0, -1.0),
                     bounding_box_max: Sequence[float] = (1.0, 1.0, 1.0), scene_box=None, truncation_margin: float = 5.0, max_weight: float = 1.0,
                     min_accumulation: float = 0.5, observed_only: bool = False, return_volume: bool = False,
                     target_num_faces: Optional[int] = None):
    """export_tsdf_mesh (tsdf_utils.py:278-361) for a ThermalSplatfactoModel or a ThermalNerfactoModel: `cameras` (PinholeCamera, undistorted; the
    reference takes the training cameras with distortion off) are rendered at 1 / downscale_factor (rescaled_camera) in eval mode under no_grad (the
    model's mode is restored), fused in their order -- up to batch_size frames of one size per launch, and the batching does not change a bit of the
    result -- into a volume of `resolution` voxels (an int or a triple) over the bounding box -- or, with use_bounding_box False, over `scene_box` ([2,3], the dataparser's scene_box_aabb) -- and meshed.
    With target_num_faces the mesh is then simplified to at most that many faces (simplify_to_target with the voxel size as the unit and the grid
    origin half a voxel below the volume's, so that the cells are centred on lattice points: marching-tetrahedra vertices lie on lattice planes in
    two coordinates, and a cell border there would split them by rounding alone); the reference's export decimates to 50 000 faces by default, with
    pymeshlab's edge collapse, which this is not.  None, the default, leaves the mesh as extracted.
    -> Mesh, or (Mesh, TSDFVolume) with return_volume."""
    if isinstance(resolution, int):
        dims: List[int] = [resolution] * 3
    elif isinstance(resolution, (list, tuple)) and len(resolution) == 3:
        dims = [int(v) for v in resolution]
    else:
        raise ValueError("Resolution must be an int or a list.")
    if use_bounding_box:
        aabb = torch.tensor([list(bounding_box_min), list(bounding_box_max)], dtype=F32)
    elif scene_box is None:
        raise ValueError("export_tsdf_mesh: use_bounding_box False needs the scene box")
    else:
        aabb = torch.as_tensor(getattr(scene_box, "aabb", scene_box)).detach().to("cpu", F32)
    if len(cameras) == 0 or batch_size < 1 or downscale_factor < 1:
        raise ValueError(f"export_tsdf_mesh: {len(cameras)} cameras, batch_size = {batch_size}, downscale_factor = {downscale_factor}")
    dev = model.means.device if _is_splat(model) else model.device
    volume = TSDFVolume.from_aabb(aabb, dims, truncation_margin, max_weight, dev)
    cams = [rescaled_camera(c, downscale_factor) if downscale_factor != 1 else c for c in cameras]
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            b0 = 0
            while b0 < len(cams):  # a launch takes up to batch_size consecutive cameras of one image size (RGB and thermal frames may differ)
                size = (int(cams[b0].height), int(cams[b0].width))
                b1 = b0 + 1
                while b1 < min(len(cams), b0 + batch_size) and (int(cams[b1].height), int(cams[b1].width)) == size:
                    b1 += 1
                frames = [render_frame(model, c) for c in cams[b0:b1]]
                volume.integrate(cams[b0:b1], torch.stack([f[0] for f in frames]), torch.stack([f[2] for f in frames]),
                                 torch.stack([f[1] for f in frames]), min_accumulation, frames[0][3])
                b0 = b1
    finally:
        model.train(was_training)
    mesh = volume.get_mesh(observed_only)
    if target_num_faces is not None:
        mesh, _ = simplify_to_target(mesh, target_num_faces, volume.voxel_size, origin=lattice_centred_origin(volume))
    return (mesh, volume) if return_volume else mesh


def lattice_centred_origin(volume: TSDFVolume) -> np.ndarray:
    """The origin of a simplification grid whose cells of one voxel are centred on the volume's lattice points: origin - voxel_size / 2, in fp32."""
    return (volume.origin - volume.voxel_size * 0.5).numpy()


# ---------------------------------------------------------------------------------------------------- frames and files
def mesh_to_dataset_frame(mesh: Mesh, dataparser_outputs, applied_transform=None) -> Mesh:
    """`mesh` in the dataset's own frame: the vertices through cloud.to_dataset_frame, the normals through the rotation of the same transform
    (float64, renormalised, zero normals stay zero); a transform that mirrors also swaps the winding, so normals and faces go on agreeing."""
    verts = to_dataset_frame(mesh.vertices, dataparser_outputs, applied_transform)
    zero = torch.zeros((1, 3), dtype=F32, device=mesh.vertices.device)
    basis = torch.cat([zero, torch.eye(3, dtype=F32, device=mesh.vertices.device)])
    moved = to_dataset_frame(basis, dataparser_outputs, applied_transform).double()
    lin = (moved[1:] - moved[:1]).T  # columns: the images of the axes (rotation times 1 / scale)
    n = mesh.normals.double() @ lin.T
    length = n.norm(dim=-1, keepdim=True)
    n = torch.where(length > 0, n / length.clamp_min(1e-300), torch.zeros_like(n)).float()
    faces = mesh.faces[:, [0, 2, 1]].contiguous() if float(torch.linalg.det(lin)) < 0 else mesh.faces
    return Mesh(verts, faces, n, mesh.rgbt)


def write_mesh_ply(path: str, mesh: Mesh, binary: bool = True, dataparser_outputs=None, applied_transform=None) -> str:
    """`mesh` as a PLY: vertex properties float x y z nx ny nz, uchar red green blue and thermal (the bytes cloud.write_cloud_ply writes,
    rint(255 clamp(v, 0, 1))), then `element face` with `property list uchar int vertex_indices`; binary little-endian or ascii.  With
    dataparser_outputs the mesh is written in the dataset's frame (mesh_to_dataset_frame).  dataparser.read_ply_thermal reads the vertices back."""
    if dataparser_outputs is not None:
        mesh = mesh_to_dataset_frame(mesh, dataparser_outputs, applied_transform)
    V, Fn = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    vert = np.empty(V, dtype=[(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz")] + [(n, "u1") for n in ("red", "green", "blue", "thermal")])
    xyz, nrm = mesh.vertices.detach().float().cpu().numpy(), mesh.normals.detach().float().cpu().numpy()
    u8 = to_uint8(mesh.rgbt)
    for i, (a, b) in enumerate((("x", "nx"), ("y", "ny"), ("z", "nz"))):
        vert[a], vert[b] = xyz[:, i], nrm[:, i]
    for i, n in enumerate(("red", "green", "blue", "thermal")):
        vert[n] = u8[:, i]
    face = np.empty(Fn, dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"], face["v"] = 3, mesh.faces.detach().cpu().numpy().astype(np.int32)
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", f"element vertex {V}"]
    head += [f"property float {n}" for n in ("x", "y", "z", "nx", "ny", "nz")] + [f"property uchar {n}" for n in ("red", "green", "blue", "thermal")]
    head += [f"element face {Fn}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            f.write(vert.tobytes())
            f.write(face.tobytes())
        else:
            for r in vert:
                f.write((" ".join([repr(float(r[n])) for n in ("x", "y", "z", "nx", "ny", "nz")] +
                                  [str(int(r[n])) for n in ("red", "green", "blue", "thermal")]) + "\n").encode("ascii"))
            for r in face["v"]:
                f.write(f"3 {int(r[0])} {int(r[1])} {int(r[2])}\n".encode("ascii"))
    return path


def read_mesh_ply_faces(path: str) -> np.ndarray:
    """The triangles of a PLY written by write_mesh_ply -> [F,3] int32 (the vertices: dataparser.read_ply_thermal)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header")
    body = data.index(b"\n", end) + 1
    head = data[:end].decode("ascii").splitlines()
    binary = any(ln.startswith("format binary_little_endian") for ln in head)
    V = next(int(ln.split()[2]) for ln in head if ln.startswith("element vertex"))
    Fn = next(int(ln.split()[2]) for ln in head if ln.startswith("element face"))
    if binary:
        off = body + V * (6 * 4 + 4)
        rec = np.frombuffer(data, dtype=[("n", "u1"), ("v", "<i4", (3,))], count=Fn, offset=off)
        if Fn and not bool((rec["n"] == 3).all()):
            raise ValueError(f"{path}: faces that are not triangles")
        return rec["v"].astype(np.int32).reshape(Fn, 3)
    lines = data[body:].decode("ascii").splitlines()[V:V + Fn]
    rows = np.array([[int(t) for t in ln.split()] for ln in lines], dtype=np.int64).reshape(Fn, 4)
    if Fn and not bool((rows[:, 0] == 3).all()):
        raise ValueError(f"{path}: faces that are not triangles")
    return rows[:, 1:].astype(np.int32)
