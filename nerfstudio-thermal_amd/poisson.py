"""A Poisson surface mesh from an oriented RGB+thermal point cloud, on the device: the counterpart of `ns-export poisson`
(nerfstudio/scripts/exporter.py ExportPoissonMesh: generate_point_cloud with normals, Open3D's create_from_point_cloud_poisson(depth=9), vertices
below the 0.1 quantile of the density removed).

The cloud's normals, weighted by the inverse of the local sampling density (Kazhdan, Bolitho and Hoppe 2006), are splatted onto a regular lattice
(tn_poisson_bin / tn_poisson_splat: a gather over a sorted plan, no atomics), the Poisson equation -laplace(chi) = -div V is solved on that lattice by
conjugate gradients (tn_poisson_divergence, tn_poisson_solve; Dirichlet boundary), the level is the weighted mean of chi at the points
(tn_poisson_sample), and the extractor of the TSDF export (mesh.TSDFVolume.get_mesh: tn_mesh_count / tn_mesh_emit) meshes it with a colour and a
temperature per vertex; `project_vertices` then moves the vertices onto the zero level of the volume's trilinear interpolant.  This is a DENSE-grid solve, not Kazhdan's adaptive octree: Open3D is not used, its depth-9 octree corresponds to a 512^3
lattice here, and the triangulation is marching tetrahedra, not Open3D's.  `screening` adds a lumped diagonal term, which is not PoissonRecon's
point-interpolation constraint.

The raw calls are `bin_call`, `splat_call`, `sample_call`, `divergence_call`, `apply_call` and `solve_call`, the only places that know the argument
order of their entry points (include/thermal_nerf_hip.h, which states every rule; tests/poisson_functional.py restates them).  Everything runs on
torch's current stream; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .cloud import PointCloud, _contig, _dev, generate_point_cloud
from .mesh import Mesh, TSDFVolume, lattice_centred_origin, simplify_to_target
from .ops import _stream
from .splat_camera import OrientedBox

F32, F64 = torch.float32, torch.float64
SOLVE_BLOCK, SOLVE_MAX_BLOCKS = 256, 1024  # csrc/tn_poisson.hip: POISSON_BLOCK, POISSON_MAX_BLOCKS (a dot product is one partial per block)
DENSITY_FLOOR = 0.125  # the least density a kept point can see: its own trilinear weights, squared and summed, are at least 1/8


@dataclass(frozen=True)
class Grid:
    """dims (X, Y, Z) lattice points, origin and voxel as fp32 [3]: lattice point (i, j, k) sits at origin + (i, j, k) * voxel."""

    dims: Tuple[int, int, int]
    origin: np.ndarray
    voxel: np.ndarray

    @staticmethod
    def over_box(box, dims: Union[int, Sequence[int]]) -> "Grid":
        """The lattice whose first and last points lie on the faces of `box` ((min xyz), (max xyz)): voxel = (max - min) / (dims - 1), in float64,
        rounded once."""
        d = (int(dims),) * 3 if isinstance(dims, (int, np.integer)) else tuple(int(v) for v in dims)
        b = np.asarray(box, dtype=np.float64).reshape(2, 3)
        if len(d) != 3 or min(d) < 2 or d[0] * d[1] * d[2] >= 2 ** 31:
            raise ValueError(f"a lattice of {d} points: three sizes >= 2, below 2^31 points in all")
        if not (np.isfinite(b).all() and (b[1] > b[0]).all()):
            raise ValueError(f"box = {box!r}: two finite corners, the second above the first on every axis")
        return Grid(d, b[0].astype(np.float32), ((b[1] - b[0]) / (np.asarray(d, dtype=np.float64) - 1.0)).astype(np.float32))

    def args(self):
        return [int(v) for v in self.dims] + [float(v) for v in self.origin] + [float(v) for v in self.voxel]

    def size_args(self):
        return [int(v) for v in self.dims] + [float(v) for v in self.voxel]


# ---------------------------------------------------------------------------------------------------- the raw calls
def _ptr(t: Optional[Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def plan_workspace(n: int, grid: Grid, device) -> Tensor:
    need = int(_lib.load().tn_poisson_workspace_bytes(int(n), *grid.dims))
    if need < 0:
        raise ValueError(f"tn_poisson_workspace_bytes({n}, {grid.dims}): sizes the library refuses")
    return torch.empty(max(need, 1), dtype=torch.uint8, device=device)


def bin_call(points: Tensor, grid: Grid, workspace: Tensor) -> None:
    """tn_poisson_bin: the plan of points [n,3] on `grid` into `workspace` (plan_workspace)."""
    n = int(points.shape[0])
    rc = _lib.load().tn_poisson_bin(_contig(points, "points", (n, 3)), n, *grid.args(), C.c_void_p(workspace.data_ptr()), workspace.numel(), _stream())
    _lib.check(rc, "tn_poisson_bin")


def splat_call(points: Tensor, values: Optional[Tensor], weights: Optional[Tensor], normalize: bool, grid: Grid, out: Tensor, workspace: Tensor) -> None:
    """tn_poisson_splat after bin_call on the same points, grid and workspace: values [n,C] or None (ones), weights [n] or None -> out [X,Y,Z,C]
    ([X,Y,Z] for C = 1 is accepted)."""
    n = int(points.shape[0])
    ch = 1 if values is None else int(values.shape[1])
    if tuple(out.shape) != (*grid.dims, ch) and not (ch == 1 and tuple(out.shape) == tuple(grid.dims)):
        raise ValueError(f"out must be {(*grid.dims, ch)}, got {tuple(out.shape)}")
    rc = _lib.load().tn_poisson_splat(
        _contig(points, "points", (n, 3)), n, None if values is None else _contig(values, "values", (n, ch)), ch,
        None if weights is None else _contig(weights, "weights", (n,)), int(bool(normalize)), *grid.args(), _contig(out, "out", tuple(out.shape)),
        C.c_void_p(workspace.data_ptr()), workspace.numel(), _stream())
    _lib.check(rc, "tn_poisson_splat")


def sample_call(points: Tensor, volume: Tensor, grid: Grid, out: Tensor) -> None:
    """tn_poisson_sample: volume [X,Y,Z] at points [n,3] -> out [n] float64."""
    n = int(points.shape[0])
    rc = _lib.load().tn_poisson_sample(_contig(points, "points", (n, 3)), n, _contig(volume, "volume", grid.dims), *grid.args(),
                                       _contig(out, "out", (n,), F64), _stream())
    _lib.check(rc, "tn_poisson_sample")


def divergence_call(field: Tensor, grid: Grid, out: Tensor) -> None:
    """tn_poisson_divergence: field [X,Y,Z,3] -> out [X,Y,Z] = -div field."""
    rc = _lib.load().tn_poisson_divergence(_contig(field, "field", (*grid.dims, 3)), *grid.size_args(), _contig(out, "out", grid.dims), _stream())
    _lib.check(rc, "tn_poisson_divergence")


def apply_call(x: Tensor, screening: Optional[Tensor], grid: Grid, out: Tensor) -> None:
    """tn_poisson_apply: out = A x, all [X,Y,Z]; screening [X,Y,Z] or None."""
    rc = _lib.load().tn_poisson_apply(_contig(x, "x", grid.dims), None if screening is None else _contig(screening, "screening", grid.dims),
                                      *grid.size_args(), _contig(out, "out", grid.dims), _stream())
    _lib.check(rc, "tn_poisson_apply")


def solve_workspace(grid: Grid, device) -> Tensor:
    need = int(_lib.load().tn_poisson_solve_workspace_bytes(*grid.dims))
    if need < 0:
        raise ValueError(f"tn_poisson_solve_workspace_bytes{grid.dims}: sizes the library refuses")
    return torch.empty(max(need, 1), dtype=torch.uint8, device=device)


def solve_call(b: Tensor, screening: Optional[Tensor], x: Tensor, grid: Grid, tol: float, max_iterations: int, check_every: int,
               workspace: Tensor) -> Tuple[int, float, float]:
    """tn_poisson_solve: conjugate gradients on A x = b from the guess in x, in place -> (iterations run, r.r, b.b).  Synchronises the stream every
    `check_every` iterations and at the end."""
    record = (C.c_double * 3)()
    rc = _lib.load().tn_poisson_solve(_contig(b, "b", grid.dims), None if screening is None else _contig(screening, "screening", grid.dims),
                                      _contig(x, "x", grid.dims), *grid.size_args(), float(tol), int(max_iterations), int(check_every), record,
                                      C.c_void_p(workspace.data_ptr()), workspace.numel(), _stream())
    _lib.check(rc, "tn_poisson_solve")
    return int(record[0]), float(record[1]), float(record[2])


# ---------------------------------------------------------------------------------------------------- the steps
def splat(points: Tensor, grid: Grid, workspace: Tensor, values: Optional[Tensor] = None, weights: Optional[Tensor] = None,
          normalize: bool = False) -> Tensor:
    """splat_call into a new [X,Y,Z,C] volume ([X,Y,Z] without values)."""
    shape = grid.dims if values is None else (*grid.dims, int(values.shape[1]))
    out = torch.empty(shape, dtype=F32, device=points.device)
    splat_call(points, values, weights, normalize, grid, out, workspace)
    return out


def sample(points: Tensor, volume: Tensor, grid: Grid) -> Tensor:
    out = torch.empty(points.shape[0], dtype=F64, device=points.device)
    sample_call(points, volume, grid, out)
    return out


def kept_mask(points: Tensor, grid: Grid) -> Tensor:
    """The points tn_poisson_bin keeps: finite, and floor((p - origin) / voxel) in 0..dim - 2 on every axis (float64, as the kernel has it)."""
    o = torch.as_tensor(grid.origin, device=points.device).double()
    h = torch.as_tensor(grid.voxel, device=points.device).double()
    t = (points.double() - o) / h
    c = torch.floor(t)
    top = torch.tensor([d - 2 for d in grid.dims], dtype=F64, device=points.device)
    return torch.isfinite(t).all(dim=1) & (c >= 0).all(dim=1) & (c <= top).all(dim=1)


def level_volume(phi: Tensor, phi_at_points: Tensor, weights: Tensor, kept: Tensor) -> Tuple[Tensor, float]:
    """values = (phi - iso) / max |phi - iso| in fp32 (so the extractor's clamp to [-1, 1] never bites) and iso = sum w phi(p) / sum w in float64 over
    the kept points with a finite weight and value."""
    w = weights.double()
    ok = kept & torch.isfinite(w) & torch.isfinite(phi_at_points)
    w = torch.where(ok, w, torch.zeros_like(w))
    total = w.sum()
    iso = float((w * torch.where(ok, phi_at_points, torch.zeros_like(phi_at_points))).sum() / total) if float(total) > 0 else 0.0
    d = phi.double() - iso
    top = float(d.abs().max())
    return (d / top if top > 0 else d).float(), iso


PROJECT_OFFSET, PROJECT_MAX_STEP = 0.25, 0.5  # voxels: the half-width of the gradient's central difference, the cap of one Newton step


def project_vertices(vertices: Tensor, values: Tensor, grid: Grid, iterations: int = 2) -> Tensor:
    """vertices [V,3] moved onto the zero level of the trilinear interpolant of `values` -> [V,3] fp32.  The extractor puts a vertex at the LINEAR
    zero between the two ends of its lattice edge; across the surface the Poisson solution is an S-curve some two voxels wide, and over a face or
    body diagonal (1.4 and 1.7 voxels) that chord misses the level set of the volume itself by up to 0.3 voxel.  Each iteration is one Newton step
    in float64, v -= f g / |g|^2 with f = the interpolant at v (tn_poisson_sample) and g its central difference over +-0.25 voxel per axis (six
    more samples), capped at half a voxel and skipped where g vanishes or anything is not finite; the result is rounded to fp32 after every step.
    The faces are untouched, so a closed mesh stays closed."""
    if int(iterations) < 0:
        raise ValueError(f"project_vertices: iterations = {iterations}")
    v = vertices.float()
    if v.shape[0] == 0:
        return v
    h = torch.as_tensor(grid.voxel, device=v.device).double()
    eye = torch.eye(3, dtype=F64, device=v.device)
    for _ in range(int(iterations)):
        p = v.double()
        f = sample(v, values, grid)
        g = torch.stack([(sample((p + eye[a] * (PROJECT_OFFSET * h[a])).float(), values, grid)
                          - sample((p - eye[a] * (PROJECT_OFFSET * h[a])).float(), values, grid)) / (2.0 * PROJECT_OFFSET * h[a]) for a in range(3)], dim=1)
        gg = (g * g).sum(dim=1, keepdim=True)
        step = -f[:, None] * g / torch.where(gg > 0, gg, torch.ones_like(gg))
        length = (step / h).norm(dim=1, keepdim=True)
        step = step * torch.clamp(PROJECT_MAX_STEP / torch.where(length > 0, length, torch.ones_like(length)), max=1.0)
        ok = (gg > 0) & torch.isfinite(step).all(dim=1, keepdim=True)
        v = (p + torch.where(ok, step, torch.zeros_like(step))).float()
    return v


def quantile_threshold(values: Tensor, q: float) -> float:
    """numpy's default (linear) quantile of a 1-D tensor in float64: s[lo] + (s[hi] - s[lo]) (pos - lo), pos = q (n - 1), over the sorted values."""
    s = torch.sort(values.double().reshape(-1)).values
    pos = float(q) * (s.numel() - 1)
    lo, hi = int(np.floor(pos)), int(np.ceil(pos))
    return float(s[lo]) + (float(s[hi]) - float(s[lo])) * (pos - lo)


def trim_mesh(mesh: Mesh, densities: Tensor, trim_quantile: float) -> Mesh:
    """The reference's `densities < quantile(densities, q)` rule: vertices whose density is below the quantile go, faces that name one go with them,
    the survivors keep their order and are renumbered (one cumsum, a few gathers).  trim_quantile 0, or no vertices: the mesh as it is."""
    V = int(mesh.vertices.shape[0])
    if not 0.0 <= float(trim_quantile) <= 1.0:
        raise ValueError(f"trim_quantile = {trim_quantile}: 0..1")
    if tuple(densities.shape) != (V,):
        raise ValueError(f"densities must be [{V}], got {tuple(densities.shape)}")
    if float(trim_quantile) == 0.0 or V == 0:
        return mesh
    keep = ~(densities.double() < quantile_threshold(densities, trim_quantile))
    newid = torch.cumsum(keep.to(torch.int64), 0) - 1
    faces = mesh.faces.long()
    faces = faces[keep[faces].all(dim=1)]
    return Mesh(mesh.vertices[keep], newid[faces].to(torch.int32), mesh.normals[keep], mesh.rgbt[keep])


# ---------------------------------------------------------------------------------------------------- the pipeline
def poisson_reconstruct(cloud: PointCloud, resolution: Union[int, Sequence[int]] = 256, box=((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)),
                        density_normalize: bool = True, density_downscale: int = 4, screening: float = 0.0, tol: float = 1e-3,
                        max_iterations: Optional[int] = None, check_every: int = 25, trim_quantile: float = 0.1, return_volume: bool = False,
                        project_iterations: int = 2):
    """`cloud` (with normals that point out of the surface: cloud.estimate_normals, or a PLY read with dataparser.read_ply_normals) -> Mesh.

    A lattice of `resolution` points per axis (an int or three) spans `box`.  With density_normalize the cloud's density is splatted on a lattice of
    resolution // density_downscale points (PoissonRecon estimates it two octree levels below the solve: the default 4), sampled at the points, and
    every point weighs 1 / max(density, 1/8).  V = the splat of w n; b = -div V; A chi = b is solved by conjugate gradients from zero until
    |r| <= tol |b| or for max_iterations (None: 4 x the largest dimension; CG on this operator needs O(largest dimension) iterations), with one
    read-back per check_every iterations; hitting the cap is a warning that names the residual, and the result is still returned.  `screening` > 0
    adds the diagonal screening * (fine density) / mean(voxel^2) -- a lumped term, not PoissonRecon's point interpolation.  The level is
    iso = sum w chi(p) / sum w, the meshed volume (chi - iso) / max |chi - iso| (negative inside), its weights (fine density > 0), its RGB+T the
    normalised splat of the cloud's; mesh.TSDFVolume.get_mesh extracts the closed surface, and project_vertices then moves every vertex from the
    chord's zero on its lattice edge onto the zero level of the volume's trilinear interpolant (project_iterations Newton steps; 0: the vertices
    as extracted).  trim_quantile q > 0 then removes the vertices whose
    coarse density lies below the q quantile of the vertices' densities (the reference trims at 0.1), which opens the mesh where the cloud has no
    points.  -> Mesh, or (Mesh, TSDFVolume) with return_volume; the volume carries `solve_record` (iterations, r.r, b.b), `iso` and
    `density_grid` / `density` (the coarse lattice and its density)."""
    if cloud.normals is None:
        raise ValueError("poisson_reconstruct: the cloud has no normals (cloud.estimate_normals, or generate_point_cloud(estimate_normals=True))")
    n = len(cloud)
    for name, t, w in (("xyz", cloud.xyz, 3), ("normals", cloud.normals, 3), ("rgb", cloud.rgb, 3), ("thermal", cloud.thermal, 1)):
        _dev(t, f"cloud {name}")
        if tuple(t.shape) != (n, w):
            raise ValueError(f"cloud {name} must be [{n},{w}], got {tuple(t.shape)}")
    grid = Grid.over_box(box, resolution)
    if int(density_downscale) < 1 or int(check_every) < 1 or not float(tol) >= 0 or not float(screening) >= 0:
        raise ValueError(f"poisson_reconstruct: density_downscale = {density_downscale}, check_every = {check_every} (>= 1), tol = {tol}, "
                         f"screening = {screening} (>= 0)")
    if max_iterations is None:
        max_iterations = 4 * max(grid.dims)
    if int(max_iterations) < 0 or int(project_iterations) < 0 or not 0.0 <= float(trim_quantile) <= 1.0 or n >= 2 ** 31:
        raise ValueError(f"poisson_reconstruct: max_iterations = {max_iterations} (>= 0), trim_quantile = {trim_quantile} (0..1), {n} points (< 2^31)")
    coarse = Grid.over_box(box, tuple(max(d // int(density_downscale), 2) for d in grid.dims))
    dev = cloud.xyz.device
    xyz, normals = cloud.xyz.contiguous(), cloud.normals.contiguous()
    rgbt = torch.cat([cloud.rgb, cloud.thermal], dim=1).contiguous()

    ws_c = plan_workspace(n, coarse, dev)
    bin_call(xyz, coarse, ws_c)
    density_c = splat(xyz, coarse, ws_c)
    del ws_c
    ws = plan_workspace(n, grid, dev)
    bin_call(xyz, grid, ws)
    density = splat(xyz, grid, ws)
    if density_normalize:
        weights = (1.0 / sample(xyz, density_c, coarse).clamp_min(DENSITY_FLOOR)).float()
    else:
        weights = torch.ones(n, dtype=F32, device=dev)
    field = splat(xyz, grid, ws, normals, weights)
    b = torch.empty(grid.dims, dtype=F32, device=dev)
    divergence_call(field, grid, b)
    del field
    s = None
    if float(screening) > 0:
        s = (density.double() * (float(screening) / float(np.mean(grid.voxel.astype(np.float64) ** 2)))).float()
    chi = torch.zeros(grid.dims, dtype=F32, device=dev)
    iterations, rr, bb = solve_call(b, s, chi, grid, tol, int(max_iterations), int(check_every), solve_workspace(grid, dev))
    if rr > float(tol) ** 2 * bb:
        warnings.warn(f"poisson_reconstruct: conjugate gradients stopped at the cap of {iterations} iterations with |r| / |b| = "
                      f"{float(np.sqrt(rr / bb)) if bb > 0 else float('nan'):.3e} (tol = {tol}); the surface is extracted from that solution")
    values, iso = level_volume(chi, sample(xyz, chi, grid), weights, kept_mask(xyz, grid))
    volume = TSDFVolume(torch.from_numpy(grid.origin), torch.from_numpy(grid.voxel), (2, 2, 2), device=dev)  # (the buffers are replaced below)
    volume.dims, volume.values, volume.weights = grid.dims, values, (density > 0).float()
    volume.rgbt = splat(xyz, grid, ws, rgbt, None, normalize=True)
    volume.solve_record, volume.iso, volume.density_grid, volume.density = (iterations, rr, bb), iso, coarse, density_c
    mesh = volume.get_mesh()
    if int(project_iterations) > 0:
        mesh = Mesh(project_vertices(mesh.vertices, values, grid, project_iterations), mesh.faces, mesh.normals, mesh.rgbt)
    if float(trim_quantile) > 0 and int(mesh.vertices.shape[0]) > 0:
        mesh = trim_mesh(mesh, sample(mesh.vertices, density_c, coarse), trim_quantile)
    return (mesh, volume) if return_volume else mesh


def export_poisson_mesh(model, next_rays: Callable[[], object], num_points: int = 1_000_000, resolution: Union[int, Sequence[int]] = 256,
                        bounding_box_min: Sequence[float] = (-1.0, -1.0, -1.0), bounding_box_max: Sequence[float] = (1.0, 1.0, 1.0),
                        remove_outliers: bool = True, std_ratio: float = 10.0, normals_knn: int = 30, density_normalize: bool = True,
                        density_downscale: int = 4, screening: float = 0.0, tol: float = 1e-3, max_iterations: Optional[int] = None,
                        check_every: int = 25, trim_quantile: float = 0.1, target_num_faces: Optional[int] = None, return_volume: bool = False,
                        return_cloud: bool = False):
    """ExportPoissonMesh for a ThermalNerfactoModel: generate_point_cloud(..., estimate_normals=True) inside the bounding box (`next_rays` hands out
    RayBundles, as in cloud.generate_point_cloud; the model's mode is restored), poisson_reconstruct over the same box, and with target_num_faces
    mesh.simplify_to_target with the voxel size as the unit and the grid centred on the lattice points, as in the TSDF export (the reference
    decimates to 50 000 faces by default, with pymeshlab's edge collapse, which this is not).  -> Mesh, then the TSDFVolume with return_volume,
    then the PointCloud with return_cloud."""
    lo, hi = np.asarray(bounding_box_min, dtype=np.float64), np.asarray(bounding_box_max, dtype=np.float64)
    box = OrientedBox.from_params(tuple((lo + hi) / 2), (0.0, 0.0, 0.0), tuple(hi - lo))
    cloud = generate_point_cloud(model, next_rays, num_points=num_points, remove_outliers=remove_outliers, std_ratio=std_ratio, box=box,
                                 estimate_normals=True, reorient_normals=True, normals_knn=normals_knn)
    mesh, volume = poisson_reconstruct(cloud, resolution, (tuple(lo), tuple(hi)), density_normalize, density_downscale, screening, tol, max_iterations,
                                       check_every, trim_quantile, return_volume=True)
    if target_num_faces is not None:
        mesh, _ = simplify_to_target(mesh, target_num_faces, volume.voxel_size, origin=lattice_centred_origin(volume))
    out = (mesh,) + ((volume,) if return_volume else ()) + ((cloud,) if return_cloud else ())
    return out[0] if len(out) == 1 else out
