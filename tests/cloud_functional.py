"""Restatement of the point-cloud export's two entry points (include/thermal_nerf_hip.h: tn_cloud_append, tn_cloud_remove_outliers) in plain torch
and numpy on the host.

append_ref    the keep rule and the points in IEEE float32, operation by operation in the kernel's order: every step is evaluated in float64 and
              rounded to float32 by its own cast (a float64 sum or product of two float32 values rounded to float32 is the correctly rounded float32
              result -- knn_functional.py says why), so points and masks are bit-comparable with the device's.
crop_inside   the crop box's test as the header states it: q_i = ((m_i0 x + m_i1 y) + m_i2 z) + m_i3 in float32, |q_i| < h_i strictly.
neighbor_means / outliers_ref   Open3D's remove_statistical_outlier as the issue states it: brute-force float32 distances by tn_knn's formula and tie
              rule (knn_functional.knn_brute), their ascending sum in float64 over nb_neighbors, the statistics in float64 (numpy's sums)."""
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from knn_functional import knn_brute


def _rnd(t: Tensor) -> Tensor:
    return t.to(torch.float32).to(torch.float64)


def crop_arrays(crop) -> Tuple[Tensor, Tensor]:
    """A TnSplatCrop's float32 values: world_to_box [3,4] and half_extent [3]."""
    return torch.tensor(list(crop.world_to_box), dtype=torch.float32).reshape(3, 4), torch.tensor(list(crop.half_extent), dtype=torch.float32)


def crop_inside(m: Tensor, h: Tensor, p: Tensor) -> Tensor:
    """bool [n]: p [n,3] float32 strictly inside the box (a NaN compares false and keeps nothing)."""
    m, h, p = m.double(), h.double(), p.to(torch.float32).double()
    inside = torch.ones(p.shape[0], dtype=torch.bool)
    for i in range(3):
        q = _rnd(_rnd(_rnd(_rnd(m[i, 0] * p[:, 0]) + _rnd(m[i, 1] * p[:, 1])) + _rnd(m[i, 2] * p[:, 2])) + m[i, 3])
        inside &= q.abs() < h[i]
    return inside


def append_ref(origins: Tensor, directions: Tensor, depth: Tensor, accumulation: Tensor, rgb: Tensor, thermal: Tensor, alpha_thresh: float,
               crop=None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (xyz [K,3], rgb [K,3], thermal [K,1], keep [R] bool) of the kept rays, in ray order; inputs are CPU float32."""
    o, d, t = origins.double(), directions.double(), depth.reshape(-1, 1).double()
    p = _rnd(o + _rnd(d * t)).float()
    keep = accumulation.reshape(-1) > torch.tensor(alpha_thresh, dtype=torch.float32)
    keep &= torch.isfinite(p).all(1)
    if crop is not None:
        keep &= crop_inside(*crop_arrays(crop), p)
    return p[keep], rgb.reshape(-1, 3)[keep], thermal.reshape(-1, 1)[keep], keep


def neighbor_means(points: Tensor, nb_neighbors: int) -> np.ndarray:
    """float64 [n]: (sum of the nb_neighbors - 1 nearest other points' float32 distances, ascending, in float64) / nb_neighbors."""
    dist, _ = knn_brute(points, nb_neighbors - 1)
    total = torch.zeros(dist.shape[0], dtype=torch.float64)
    for m in range(dist.shape[1]):
        total = total + dist[:, m].double()
    return (total / float(nb_neighbors)).numpy()


def outliers_ref(points: Tensor, nb_neighbors: int, std_ratio: float, mean: Optional[np.ndarray] = None):
    """-> (mean [n] float64, (m, s, thr), keep [n] bool)."""
    mean = neighbor_means(points, nb_neighbors) if mean is None else mean
    pos = mean[mean > 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        m = pos.sum() / np.float64(pos.shape[0])
        s = np.sqrt(((pos - m) ** 2).sum() / np.float64(pos.shape[0] - 1))
    thr = m + np.float64(std_ratio) * s
    return mean, (float(m), float(s), float(thr)), (mean > 0) & (mean < thr)
