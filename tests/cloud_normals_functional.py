"""Restatement of tn_cloud_estimate_normals (include/thermal_nerf_hip.h) in float64 torch on the host.

Neighbour sets come from knn_functional.knn_brute(points, knn - 1): float32 distances by tn_knn's formula and tie rule, so membership and order
are the device's, bit for bit.  Everything after that is float64: c_j = p_j - p_i (exact), S1 = sum c_j and S2 = sum c_j c_j^T over the
neighbourhood in its order (the point itself, first, adds zeros), C = S2 / knn - (S1 / knn)(S1 / knn)^T, torch.linalg.eigh, the eigenvector of
the smallest eigenvalue, normalised; (0, 0, 1) where C is exactly zero; then the sign: against the view direction when there is one (flip when
v . n > 0), the first non-zero of (nz, ny, nx) positive otherwise."""
from typing import NamedTuple, Optional

import torch
from torch import Tensor

from knn_functional import knn_brute


class Normals(NamedTuple):
    normals: Tensor  # [n,3] float64, unit, oriented
    gap: Tensor      # [n] (lambda_1 - lambda_0) / lambda_2 of C (0 where C is zero): below ~1e-3 the vector is not a function of the data at fp32 resolution
    vdot: Tensor     # [n] v . n of the oriented normal (<= 0), or zeros without view directions
    zero: Tensor     # [n] bool: C exactly zero, the fallback (0, 0, 1) was used


def covariance(points: Tensor, knn: int) -> Tensor:
    """[n,3,3] float64: C of every point's knn-neighbourhood, summed in the neighbourhood's order."""
    p = points.to(torch.float32).double().cpu()
    _, idx = knn_brute(points, knn - 1)
    s1 = torch.zeros(p.shape[0], 3, dtype=torch.float64)
    s2 = torch.zeros(p.shape[0], 3, 3, dtype=torch.float64)
    for m in range(knn - 1):
        c = p[idx[:, m]] - p
        s1 = s1 + c
        s2 = s2 + c[:, :, None] * c[:, None, :]
    mean = s1 / float(knn)
    return s2 / float(knn) - mean[:, :, None] * mean[:, None, :]


def estimate_normals_ref(points: Tensor, knn: int, view: Optional[Tensor] = None) -> Normals:
    C = covariance(points, knn)
    zero = (C == 0).reshape(-1, 9).all(1)
    lam, vec = torch.linalg.eigh(C)  # ascending eigenvalues, eigenvectors in columns
    n = vec[:, :, 0]
    n = n / n.norm(dim=1, keepdim=True)
    n[zero] = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    gap = torch.where(zero, torch.zeros_like(lam[:, 0]), (lam[:, 1] - lam[:, 0]) / lam[:, 2].clamp_min(1e-300))
    if view is not None:
        v = view.to(torch.float32).double().cpu()
        flip = (v * n).sum(1) > 0
    else:
        z, y, x = n[:, 2], n[:, 1], n[:, 0]
        flip = torch.where(z != 0, z < 0, torch.where(y != 0, y < 0, x < 0))
    n = torch.where(flip[:, None], -n, n)
    vdot = (view.to(torch.float32).double().cpu() * n).sum(1) if view is not None else torch.zeros_like(gap)
    return Normals(n, gap, vdot, zero)
