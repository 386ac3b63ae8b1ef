"""Brute-force restatement of tn_knn (and of splatfacto's k_nearest_sklearn, nerfstudio/models/splatfacto.py:272-290): for every query row i
the k smallest (d2, j) over the points j != i, ascending, ties on d2 to the smaller index; d2 = (dx*dx + dy*dy) + dz*dz with dx = xi - xj, one
rounded operation per step, distance = sqrt(d2) (numpy, on the host).  Chunked over query rows.

In float32 every step is evaluated in float64 and rounded to float32 by its own cast.  A float64 sum, difference or product of float32
values rounded to float32 is the correctly rounded float32 result (53 >= 2 * 24 + 2 bits: double rounding is innocuous), so the restatement
is IEEE float32 arithmetic on either device, whatever a device's elementwise kernels contract or fuse."""
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor


def knn_brute(points: Tensor, k: int, rows: Optional[Tensor] = None, dtype=torch.float32, max_elems: int = 1 << 24) -> Tuple[Tensor, Tensor]:
    """points [N,3] (any device) -> (distances [R,k] in `dtype`, indices [R,k] int64) for the query rows `rows` (default: all N)."""
    p = points.to(dtype).to(torch.float64)  # the points' values, exactly
    n = p.shape[0]

    def rnd(t: Tensor) -> Tensor:  # one rounding to `dtype`, back in float64 for the next step
        return t.to(dtype).to(torch.float64)

    assert n >= k + 1
    rows = torch.arange(n, device=p.device) if rows is None else rows.to(p.device).long()
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    cols = torch.arange(n, device=p.device)
    chunk = max(1, max_elems // n)
    out_d, out_i = [], []
    for b in range(0, rows.shape[0], chunk):
        r = rows[b:b + chunk]
        dx = rnd(x[r, None] - x[None, :])
        dy = rnd(y[r, None] - y[None, :])
        dz = rnd(z[r, None] - z[None, :])
        sx = rnd(dx * dx)
        sy = rnd(dy * dy)
        sz = rnd(dz * dz)
        d2 = rnd(sx + sy)
        d2 = rnd(d2 + sz).to(dtype)
        d2[cols[None, :] == r[:, None]] = float("inf")  # j != i (finite clouds: the point itself is never among the k)
        # the k smallest with the tie rule: everything below the k-th value, then the lowest indices among the entries equal to it
        kth = torch.kthvalue(d2, k, dim=1, keepdim=True).values
        below = d2 < kth
        need = k - below.sum(1, keepdim=True)
        equal = d2 == kth
        take = below | (equal & (torch.cumsum(equal.int(), 1) <= need))
        idx = take.nonzero()[:, 1].reshape(r.shape[0], k)  # row-major: ascending index within each row
        dd = torch.gather(d2, 1, idx)
        dd, order = torch.sort(dd, dim=1, stable=True)  # stable: equal d2 keep ascending index
        # numpy's float64 sqrt rounded to `dtype`: correctly rounded (torch's vectorised host sqrt is not, on every CPU)
        out_d.append(torch.from_numpy(np.sqrt(dd.cpu().numpy().astype(np.float64))).to(dtype))
        out_i.append(torch.gather(idx, 1, order))
    return torch.cat(out_d), torch.cat(out_i).cpu()


def cloud(kind: str, n: int, seed: int = 0) -> Tensor:
    """[n,3] float32 test clouds (CPU): uniform, plane, line, identical, lattice (mass ties), duplicates (heavy), clusters (spread 1e-4 next
    to spread 1e2), surface (points on a few planes with dense clusters, like an SfM cloud)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(s, generator=g)  # noqa: E731
    if kind == "uniform":
        return u(n, 3) * 2 - 1
    if kind == "plane":
        p = u(n, 3) * 2 - 1
        p[:, 2] = 0.25
        return p
    if kind == "line":
        t = u(n, 1)
        return (torch.tensor([[0.3, -1.0, 2.0]]) + t * torch.tensor([[1.0, 2.0, -0.5]])).float()
    if kind == "identical":
        return torch.tensor([[0.1, -0.2, 0.3]]).repeat(n, 1)
    if kind == "lattice":
        s = max(2, round(n ** (1 / 3)) + 1)
        ijk = torch.stack(torch.meshgrid(*(torch.arange(s),) * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
        return ijk.float() * 0.5 - 1.0
    if kind == "duplicates":
        base = u(max(1, n // 8), 3)
        return base[torch.randint(0, base.shape[0], (n,), generator=g)].contiguous()
    if kind == "clusters":
        c = n // 2
        tight = torch.tensor([[1.0, 2.0, 3.0]]) + (u(c, 3) - 0.5) * 1e-4
        wide = (u(n - c, 3) - 0.5) * 1e2
        return torch.cat([tight, wide])[torch.randperm(n, generator=g)].contiguous()
    if kind == "surface":
        planes = torch.randint(0, 3, (n,), generator=g)
        p = u(n, 3) * 4 - 2
        p[torch.arange(n), planes] = planes.float() - 1.0
        hot = torch.rand(n, generator=g) < 0.3  # 30 % of the points in 64 tight clusters
        centres = p[torch.randint(0, n, (64,), generator=g)]
        p[hot] = centres[torch.randint(0, 64, (int(hot.sum()),), generator=g)] + (u(int(hot.sum()), 3) - 0.5) * 1e-3
        return p.contiguous()
    raise KeyError(kind)
