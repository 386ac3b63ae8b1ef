"""An RGB+thermal point cloud from a trained thermal-nerfacto model, on the device: the counterpart of `ns-export pointcloud`
(nerfstudio/scripts/exporter.py:90-186; nerfstudio/exporter/exporter_utils.py:83-260, generate_point_cloud).

Training rays are rendered in eval mode, back-projected by their depth, kept where they are opaque and inside a box (tn_cloud_append: a stable
compaction, the points of a batch stay in ray order), and cleaned by Open3D's statistical outlier rule (tn_cloud_remove_outliers: a wide exact
neighbour search on tn_knn's tree).  Every point carries the colour AND the thermal value the model rendered for its ray, so a cloud written
with `write_cloud_ply` and named as a dataset's `ply_file_path` seeds thermal splats with a temperature per Gaussian (dataparser.load_3D_points
-> ThermalFullImageDatamanager.seed_points -> ThermalSplatfactoModel(seed_points=(xyz, rgb, thermal))).

With `estimate_normals` the cloud also carries an oriented unit normal per point, the reference's default export (normal_method="open3d",
reorient_normals=True): the direction of every kept ray travels beside its point through both compactions (tn_cloud_append_view,
tn_cloud_remove_outliers_view), and tn_cloud_estimate_normals ends the same wide neighbour search in the covariance of the `knn` nearest points and
its smallest eigenvector, flipped against the ray.  `write_cloud_ply` then writes float nx ny nz after x y z.  Normals rendered by the model
(`predict_normals`) are not supported; a mesh with normals, colours and temperatures per vertex is mesh.py's (the counterpart of `ns-export tsdf`).

The raw calls of the entry points are `append_call`, `remove_outliers_call` and `estimate_normals_call`, the only places that know their argument
order (include/thermal_nerf_hip.h).  Everything runs on torch's current stream; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .ops import _stream
from .splat_camera import OrientedBox

F32 = torch.float32
Box = Union[OrientedBox, _lib.TnSplatCrop, None]


@dataclass
class PointCloud:
    """xyz [M,3], rgb [M,3] in 0..1 and thermal [M,1] in 0..1, float32 on the device; optionally view [M,3], the direction of the ray that
    produced each point (as rendered, not renormalised), and normals [M,3], unit vectors (estimate_normals)."""

    xyz: Tensor
    rgb: Tensor
    thermal: Tensor
    view: Optional[Tensor] = None
    normals: Optional[Tensor] = None

    def __len__(self) -> int:
        return int(self.xyz.shape[0])

    def __getitem__(self, rows) -> "PointCloud":
        return PointCloud(self.xyz[rows], self.rgb[rows], self.thermal[rows], None if self.view is None else self.view[rows],
                          None if self.normals is None else self.normals[rows])

    @staticmethod
    def empty(num_points: int, device="cuda", with_view: bool = False) -> "PointCloud":
        """Buffers of exactly `num_points` rows for `append_points` (uninitialised: the counter says how many rows are points); with_view adds
        the buffer of the view directions."""
        return PointCloud(torch.empty((num_points, 3), device=device), torch.empty((num_points, 3), device=device),
                          torch.empty((num_points, 1), device=device), torch.empty((num_points, 3), device=device) if with_view else None)


def default_box() -> OrientedBox:
    """The reference's default bounding box, (-1,-1,-1)..(1,1,1), as an oriented box."""
    return OrientedBox.from_params((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (2.0, 2.0, 2.0))


# ---------------------------------------------------------------------------------------------------- the raw calls
def _dev(t: Tensor, name: str, dtype=F32) -> Tensor:
    if not isinstance(t, Tensor) or not t.is_cuda or t.dtype != dtype:
        raise ValueError(f"{name} must be a {dtype} HIP tensor (the point-cloud path has no CPU fallback)")
    return t


def _contig(t: Tensor, name: str, shape, dtype=F32):
    _dev(t, name, dtype)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous {tuple(shape)}, got {tuple(t.shape)}")
    return C.c_void_p(t.data_ptr())


def _rows(t: Tensor, name: str, rows: int, width: int):
    """(pointer, element stride per row) of a [rows, width] fp32 device tensor read in place: its channels must be adjacent, its rows any constant
    stride apart (a view of the shared-density render's [R,4] rgbt buffer); anything else is copied."""
    _dev(t, name)
    if t.dim() == 1 and width == 1:
        t = t[:, None]
    if t.dim() != 2 or t.shape[0] != rows or t.shape[1] != width:
        raise ValueError(f"{name} must be [{rows},{width}], got {tuple(t.shape)}")
    if rows > 1 and ((width > 1 and t.stride(1) != 1) or t.stride(0) < width):
        t = t.contiguous()
    return t, C.c_void_p(t.data_ptr()), (int(t.stride(0)) if rows > 1 else width)


def _crop(box: Box) -> Optional[_lib.TnSplatCrop]:
    if box is None or isinstance(box, _lib.TnSplatCrop):
        return box
    if isinstance(box, OrientedBox):
        return box.crop_struct()
    raise ValueError(f"box must be an OrientedBox, a TnSplatCrop or None, got {type(box).__name__}")


def _workspace(size_fn: str, *sizes, device) -> Tensor:
    need = int(getattr(_lib.load(), size_fn)(*sizes))
    if need < 0:
        raise ValueError(f"{size_fn}{sizes}: sizes the library refuses")
    return torch.empty(max(need, 1), dtype=torch.uint8, device=device)


def append_call(origins, directions, depth, accumulation, rgb, thermal, alpha_thresh: float, box: Optional[_lib.TnSplatCrop], out: PointCloud,
                count: Tensor) -> None:
    """tn_cloud_append of R rays into the rows of `out` from `count` (device int64 [1]) on; rgb [R,3] and thermal [R,1] may be strided views.
    When `out` has a view buffer the call is tn_cloud_append_view and the kept rays' directions go there."""
    R, cap = origins.shape[0], out.xyz.shape[0]
    rgb, p_rgb, s_rgb = _rows(rgb, "rgb", R, 3)  # (a copy _rows had to make is held here until the call is enqueued)
    thermal, p_th, s_th = _rows(thermal, "rgb_thermal", R, 1)
    ws = _workspace("tn_cloud_append_workspace_bytes", R, device=origins.device)
    name = "tn_cloud_append" if out.view is None else "tn_cloud_append_view"
    view = () if out.view is None else (_contig(out.view, "cloud view", (cap, 3)),)
    rc = getattr(_lib.load(), name)(_contig(origins, "origins", (R, 3)), _contig(directions, "directions", (R, 3)), _contig(depth, "depth", (R,)),
                                    _contig(accumulation, "accumulation", (R,)), p_rgb, s_rgb, p_th, s_th, R, float(alpha_thresh),
                                    C.byref(box) if box is not None else None, _contig(out.xyz, "cloud xyz", (cap, 3)),
                                    _contig(out.rgb, "cloud rgb", (cap, 3)), _contig(out.thermal, "cloud thermal", (cap, 1)), *view, cap,
                                    _contig(count, "count", (1,), torch.int64), C.c_void_p(ws.data_ptr()), ws.numel(), _stream())
    _lib.check(rc, name)


def remove_outliers_call(cloud: PointCloud, nb_neighbors: int, std_ratio: float, out: PointCloud, count: Tensor, stats: Tensor,
                         mean: Optional[Tensor] = None, keep: Optional[Tensor] = None) -> None:
    """tn_cloud_remove_outliers of `cloud` into `out` (room for as many rows), the kept number into `count` (int64 [1]), [m, s, thr] into `stats`
    (float64 [3]) and, when given, every neighbour mean into `mean` (float64 [n]) and the mask into `keep` (uint8 [n]).  When both clouds have
    a view buffer the call is tn_cloud_remove_outliers_view and the view directions are compacted with the points."""
    n = len(cloud)
    ws = _workspace("tn_cloud_remove_outliers_workspace_bytes", n, nb_neighbors, device=cloud.xyz.device)
    with_view = cloud.view is not None and out.view is not None
    name = "tn_cloud_remove_outliers_view" if with_view else "tn_cloud_remove_outliers"
    view = (_contig(cloud.view, "cloud view", (n, 3)),) if with_view else ()
    out_view = (_contig(out.view, "out view", (n, 3)),) if with_view else ()
    rc = getattr(_lib.load(), name)(
        _contig(cloud.xyz, "cloud xyz", (n, 3)), _contig(cloud.rgb, "cloud rgb", (n, 3)), _contig(cloud.thermal, "cloud thermal", (n, 1)), *view, n,
        int(nb_neighbors), float(std_ratio), _contig(out.xyz, "out xyz", (n, 3)), _contig(out.rgb, "out rgb", (n, 3)),
        _contig(out.thermal, "out thermal", (n, 1)), *out_view, _contig(count, "count", (1,), torch.int64),
        _contig(stats, "stats", (3,), torch.float64), None if mean is None else _contig(mean, "mean", (n,), torch.float64),
        None if keep is None else _contig(keep, "keep", (n,), torch.uint8), C.c_void_p(ws.data_ptr()), ws.numel(), _stream())
    _lib.check(rc, name)


def estimate_normals_call(xyz: Tensor, knn: int, view: Optional[Tensor], normals: Tensor) -> None:
    """tn_cloud_estimate_normals of xyz [n,3] into normals [n,3]: the kNN PCA over `knn` points (the point itself counted), oriented against
    view [n,3] when given, by the sign rule of the header otherwise."""
    n = int(xyz.shape[0])
    ws = _workspace("tn_cloud_normals_workspace_bytes", n, int(knn), device=xyz.device)
    rc = _lib.load().tn_cloud_estimate_normals(_contig(xyz, "cloud xyz", (n, 3)), n, int(knn), None if view is None else _contig(view, "cloud view", (n, 3)),
                                               _contig(normals, "normals", (n, 3)), C.c_void_p(ws.data_ptr()), ws.numel(), _stream())
    _lib.check(rc, "tn_cloud_estimate_normals")


# ---------------------------------------------------------------------------------------------------- the two steps
def append_points(outputs: Dict[str, Tensor], ray_bundle, cloud_buffers: PointCloud, count: Tensor, box: Box, alpha_thresh: float = 0.5) -> None:
    """One rendered batch into the cloud: `outputs` is the model's eval render of `ray_bundle` (rgb, rgb_thermal, and depth / accumulation of the
    RGB branch, which is where the reference takes them from in both density modes).  Ray r is kept iff accumulation > alpha_thresh (strict),
    origin + direction * depth is finite, and the point is strictly inside `box` (None: no box).  Kept rays are appended in ray order at the row
    `count` (device int64 [1]) names; rows beyond the buffers are dropped and the counter stops at their size.  No host synchronisation."""
    o = _dev(ray_bundle.origins, "origins").reshape(-1, 3).contiguous()
    d = _dev(ray_bundle.directions, "directions").reshape(-1, 3).contiguous()
    R = o.shape[0]
    flat = lambda k: _dev(outputs[k], k).reshape(R).contiguous()  # noqa: E731
    rgb, th = _dev(outputs["rgb"], "rgb"), _dev(outputs["rgb_thermal"], "rgb_thermal")
    append_call(o, d, flat("depth"), flat("accumulation"), rgb.reshape(R, 3) if rgb.dim() != 2 else rgb, th.reshape(R, 1) if th.dim() != 2 else th,
                alpha_thresh, _crop(box), cloud_buffers, count)


def remove_outliers(cloud: PointCloud, nb_neighbors: int = 20, std_ratio: float = 10.0, details: Optional[dict] = None) -> PointCloud:
    """Open3D's remove_statistical_outlier(nb_neighbors, std_ratio) on the device.  mean_i = the sum of the distances to the nb_neighbors - 1
    nearest other points over nb_neighbors; over the points with mean_i > 0, m and s are their mean and sample standard deviation; point i stays
    iff 0 < mean_i < m + std_ratio * s.  The kept points come back in their original order (one host synchronisation, for their number).
    A cloud of fewer than nb_neighbors points is returned unchanged, with a warning.  `details`, when a dict, receives "stats" (float64
    [m, s, thr]), "mean" (float64 [n]) and "keep" (bool [n]).  A cloud with view directions keeps them beside its points; normals are not carried
    (they are estimated after this step, as in the reference)."""
    for name, t, w in (("xyz", cloud.xyz, 3), ("rgb", cloud.rgb, 3), ("thermal", cloud.thermal, 1)):
        _dev(t, f"cloud {name}")
        if t.dim() != 2 or t.shape != (len(cloud), w):
            raise ValueError(f"cloud {name} must be [{len(cloud)},{w}], got {tuple(t.shape)}")
    if not 2 <= int(nb_neighbors) <= 32:
        raise ValueError(f"remove_outliers: nb_neighbors = {nb_neighbors}, tn_cloud_remove_outliers supports 2..32")
    n = len(cloud)
    if n < nb_neighbors:
        print(f"Warning: remove_outliers needs at least nb_neighbors = {nb_neighbors} points, the cloud has {n}: it is returned unchanged.")
        return cloud
    dev = cloud.xyz.device
    if cloud.view is not None and (_dev(cloud.view, "cloud view").dim() != 2 or cloud.view.shape != (n, 3)):
        raise ValueError(f"cloud view must be [{n},3], got {tuple(cloud.view.shape)}")
    src = PointCloud(cloud.xyz.contiguous(), cloud.rgb.contiguous(), cloud.thermal.contiguous(), None if cloud.view is None else cloud.view.contiguous())
    out = PointCloud.empty(n, dev, with_view=cloud.view is not None)
    count, stats = torch.zeros(1, dtype=torch.int64, device=dev), torch.empty(3, dtype=torch.float64, device=dev)
    mean = torch.empty(n, dtype=torch.float64, device=dev) if details is not None else None
    keep = torch.empty(n, dtype=torch.uint8, device=dev) if details is not None else None
    remove_outliers_call(src, nb_neighbors, std_ratio, out, count, stats, mean, keep)
    if details is not None:
        details.update(stats=stats, mean=mean, keep=keep.bool())
    return out[: int(count.item())]


def estimate_normals(cloud: PointCloud, knn: int = 30, reorient: bool = True) -> PointCloud:
    """Open3D's estimate_normals(KDTreeSearchParamKNN(knn)) and the reference's reorient_normals on the device: the unit eigenvector of the
    smallest eigenvalue of the covariance of each point's `knn` nearest points (the point itself counted; include/thermal_nerf_hip.h states the
    rule).  reorient flips every normal against the point's view direction (v . n <= 0 afterwards) and needs `cloud.view`; without it the first
    non-zero of (nz, ny, nx) is positive.  The same cloud comes back with `normals` [M,3] float32 set.  An empty cloud gets empty normals; one
    of fewer than `knn` points is a ValueError."""
    n = len(cloud)
    if reorient and cloud.view is None:
        raise ValueError("estimate_normals: reorient=True needs the cloud's view directions (PointCloud.view)")
    if not 3 <= int(knn) <= 32:
        raise ValueError(f"estimate_normals: knn = {knn}, tn_cloud_estimate_normals supports 3..32")
    _dev(cloud.xyz, "cloud xyz")
    if cloud.xyz.dim() != 2 or cloud.xyz.shape[1] != 3:
        raise ValueError(f"cloud xyz must be [{n},3], got {tuple(cloud.xyz.shape)}")
    view = None
    if reorient:
        if _dev(cloud.view, "cloud view").dim() != 2 or cloud.view.shape != (n, 3):
            raise ValueError(f"cloud view must be [{n},3], got {tuple(cloud.view.shape)}")
        view = cloud.view.contiguous()
    if 0 < n < int(knn):
        raise ValueError(f"estimate_normals: knn = {knn} needs at least as many points, the cloud has {n}")
    normals = torch.empty((n, 3), dtype=F32, device=cloud.xyz.device)
    estimate_normals_call(cloud.xyz.contiguous(), knn, view, normals)
    cloud.normals = normals
    return cloud


_remove_outliers = remove_outliers  # generate_point_cloud has a flag of the same name, as the reference's has
_estimate_normals = estimate_normals


# ---------------------------------------------------------------------------------------------------- the export
def generate_point_cloud(model, next_rays: Callable[[], object], num_points: int = 1_000_000, remove_outliers: bool = True, std_ratio: float = 10.0,
                         nb_neighbors: int = 20, box: Optional[OrientedBox] = None, use_bounding_box: bool = True,
                         max_batches: Optional[int] = None, alpha_thresh: float = 0.5, estimate_normals: bool = False, reorient_normals: bool = True,
                         normals_knn: int = 30) -> PointCloud:
    """exporter_utils.py:83-260 for a ThermalNerfactoModel: gather_points, then the outliers go, then -- estimate_normals, the reference's
    normal_method="open3d" -- a normal per point from its `normals_knn` nearest points, flipped against the ray when reorient_normals.  With
    estimate_normals off no view buffer exists and the launches are the ones that ran before the switch existed."""
    buffers = gather_points(model, next_rays, num_points, box, use_bounding_box, max_batches, alpha_thresh, with_view=estimate_normals)
    if remove_outliers:
        buffers = _remove_outliers(buffers, nb_neighbors, std_ratio)
    return _estimate_normals(buffers, normals_knn, reorient_normals) if estimate_normals else buffers


def gather_points(model, next_rays: Callable[[], object], num_points: int = 1_000_000, box: Optional[OrientedBox] = None, use_bounding_box: bool = True,
                  max_batches: Optional[int] = None, alpha_thresh: float = 0.5, with_view: bool = False) -> PointCloud:
    """The render-and-append loop of generate_point_cloud: `next_rays()` hands out RayBundles (the default caller passes
    `lambda: datamanager.next_train(0)[0]` of HipDataManager), each is rendered in eval mode under no_grad (the model's mode is restored) and
    appended until the buffers of exactly `num_points` rows are full.  `box` defaults to the reference's
    (-1,-1,-1)..(1,1,1); use_bounding_box False keeps every opaque finite point.  The device counter is read back every eighth batch only.  Where
    the reference would loop forever -- nothing opaque inside the box -- the loop ends after `max_batches` (default: 64 x the batches num_points
    needs when every ray is kept) with a RuntimeError that names the keep rate.  The cloud has exactly num_points points.  with_view carries the
    kept rays' directions beside the points (`view`)."""
    if num_points < 1:
        raise ValueError(f"generate_point_cloud: num_points = {num_points}")
    crop = _crop((box if box is not None else default_box()) if use_bounding_box else None)
    dev = model.device
    buffers = PointCloud.empty(num_points, dev, with_view=with_view)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    was_training = model.training
    model.eval()
    batches = rays = have = 0
    try:
        with torch.no_grad():
            while have < num_points:
                bundle = next_rays()
                if max_batches is None:
                    max_batches = 64 * math.ceil(num_points / max(len(bundle), 1))
                outputs = model(bundle)
                append_points(outputs, bundle, buffers, count, crop, alpha_thresh)
                batches, rays = batches + 1, rays + len(bundle)
                if batches % 8 == 0 or batches >= max_batches:
                    have = int(count.item())
                    if have < num_points and batches >= max_batches:
                        raise RuntimeError(f"generate_point_cloud: {have} of {num_points} points after {batches} batches ({rays} rays): "
                                           f"{have / max(rays, 1):.3%} of the rays are opaque (accumulation > {alpha_thresh}) and inside the box")
    finally:
        model.train(was_training)
    return buffers


# ---------------------------------------------------------------------------------------------------- frames and files
def to_dataset_frame(cloud_xyz: Tensor, dataparser_outputs, applied_transform=None) -> Tensor:
    """The inverse of what dataparser.load_3D_points applies (`transform`, then `scale`): points in the model's frame -> the dataset's own frame
    (the reference's save_world_frame), so that a cloud written as the dataset's `ply_file_path` loads back where it was.  Evaluated in float64
    from dataparser_outputs.dataparser_transform [3,4] and .dataparser_scale, rounded once to float32.  `applied_transform` [3,4] is the
    transforms.json entry of that name, if the dataset has one: load_3D_points leaves it out of its transform, so it is taken out here."""
    T = torch.as_tensor(dataparser_outputs.dataparser_transform).detach().to("cpu", torch.float64)
    T4 = torch.cat([T[:3, :4], torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)], 0)
    if applied_transform is not None:
        A = torch.as_tensor(applied_transform).detach().to("cpu", torch.float64)
        T4 = T4 @ torch.linalg.inv(torch.cat([A[:3, :4], torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)], 0))
    inv = torch.linalg.inv(T4)[:3].to(cloud_xyz.device)
    p = cloud_xyz.detach().double() / float(dataparser_outputs.dataparser_scale)
    return (p @ inv[:, :3].T + inv[:, 3]).float()


def normals_to_dataset_frame(normals: Tensor, dataparser_outputs, applied_transform=None) -> Tensor:
    """Normals in the model's frame -> the dataset's own frame: the linear part of to_dataset_frame's map, with no scale and no translation (the
    rotation mesh.mesh_to_dataset_frame applies to a mesh's normals), evaluated in float64 and rounded once to float32.  load_3D_points turns
    them back (points3D_normals = n @ transform[:, :3].T)."""
    T = torch.as_tensor(dataparser_outputs.dataparser_transform).detach().to("cpu", torch.float64)
    T4 = torch.cat([T[:3, :4], torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)], 0)
    if applied_transform is not None:
        A = torch.as_tensor(applied_transform).detach().to("cpu", torch.float64)
        T4 = T4 @ torch.linalg.inv(torch.cat([A[:3, :4], torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)], 0))
    lin = torch.linalg.inv(T4)[:3, :3].to(normals.device)
    return (normals.detach().double() @ lin.T).float()


def to_uint8(values: Tensor) -> np.ndarray:
    """0..1 floats -> the PLY's bytes, rint(255 * clamp(v, 0, 1)), on the host."""
    return torch.clamp(values.detach() * 255.0, 0.0, 255.0).round().to(torch.uint8).cpu().numpy()


def write_cloud_ply(path: str, cloud: PointCloud, xyz: Optional[Tensor] = None, binary: bool = True, normals: Optional[Tensor] = None) -> str:
    """`cloud` as a PLY with uchar red green blue and thermal (dataparser.write_ply); `xyz` replaces the cloud's positions (to_dataset_frame) and
    `normals` its normals (normals_to_dataset_frame).  A cloud with normals gets float nx ny nz after x y z; one without is written as before."""
    from .dataparser import write_ply

    pts = cloud.xyz if xyz is None else xyz
    nrm = cloud.normals if normals is None else normals
    return write_ply(path, pts.detach().float().cpu().numpy(), to_uint8(cloud.rgb), binary=binary, thermal=to_uint8(cloud.thermal),
                     normals=None if nrm is None else nrm.detach().float().cpu().numpy())
