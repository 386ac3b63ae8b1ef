"""The float64 restatement of the dense-grid Poisson reconstruction (include/thermal_nerf_hip.h, "Poisson surface reconstruction"; rules 1-7 of
nerfstudio_thermal_amd/poisson.py's pipeline), in torch on the host.  Nothing here imports the package: a grid is any object with `dims` (X, Y, Z),
`origin` and `voxel` (fp32 [3]).

Every function that stands for an fp32 output returns the float64 value AND the sum of the absolute values of the terms that make it up, which is
what the device tests scale their rounding bounds by."""
from collections import namedtuple

import numpy as np
import torch

F64 = torch.float64
Grid = namedtuple("Grid", "dims origin voxel")


def grid_over_box(box, dims):
    """first and last lattice point on the faces of the box: voxel = (max - min) / (dims - 1) in float64, rounded once to fp32"""
    d = (int(dims),) * 3 if isinstance(dims, int) else tuple(int(v) for v in dims)
    b = np.asarray(box, dtype=np.float64).reshape(2, 3)
    return Grid(d, b[0].astype(np.float32), ((b[1] - b[0]) / (np.asarray(d, dtype=np.float64) - 1.0)).astype(np.float32))


def _oh(grid):
    return torch.from_numpy(np.asarray(grid.origin, dtype=np.float32)).double(), torch.from_numpy(np.asarray(grid.voxel, dtype=np.float32)).double()


def r32(t):
    """round to fp32, keep float64 storage"""
    return t.float().double()


# ---------------------------------------------------------------------------------------------------- 1. binning
def bin_ref(points, grid):
    """-> kept [n] bool, c [n,3] int64 (0 where not kept), t [n,3] float64.  t = (p - origin) / voxel in double from the fp32 inputs, c = floor(t);
    kept iff t is finite and every c lies in 0..dim - 2."""
    o, h = _oh(grid)
    t = (points.float().double() - o) / h
    c = torch.floor(t)
    top = torch.tensor([d - 2 for d in grid.dims], dtype=F64)
    kept = torch.isfinite(t).all(1) & (c >= 0).all(1) & (c <= top).all(1)
    return kept, torch.where(kept[:, None], c, torch.zeros_like(c)).long(), t


# ---------------------------------------------------------------------------------------------------- 2. splat
def splat_ref(points, grid, values=None, weights=None, normalize=False):
    """out[q] = sum_p (w_p tri_p(q)) value_p -> (out [X,Y,Z,C] float64, the sum of |terms| [X,Y,Z,C], den [X,Y,Z] = sum_p w_p tri_p(q)).  A point
    is skipped when it is not kept, or its weight or one of its values is not finite.  normalize: out / den where den > 0, else 0 (the |terms| are
    then those of the numerator over den)."""
    X, Y, Z = grid.dims
    n = points.shape[0]
    kept, c, t = bin_ref(points, grid)
    v = torch.ones((n, 1), dtype=F64) if values is None else values.float().double()
    w = torch.ones(n, dtype=F64) if weights is None else weights.float().double()
    kept = kept & torch.isfinite(w) & torch.isfinite(v).all(1)
    C = v.shape[1]
    out, mag, den = torch.zeros((X * Y * Z, C), dtype=F64), torch.zeros((X * Y * Z, C), dtype=F64), torch.zeros(X * Y * Z, dtype=F64)
    idx = kept.nonzero()[:, 0]
    c, v, w = c[idx], v[idx], w[idx]
    f = t[idx] - torch.floor(t[idx])
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                wx = f[:, 0] if dx else 1.0 - f[:, 0]
                wy = f[:, 1] if dy else 1.0 - f[:, 1]
                wz = f[:, 2] if dz else 1.0 - f[:, 2]
                wt = w * ((wx * wy) * wz)
                q = ((c[:, 0] + dx) * Y + (c[:, 1] + dy)) * Z + (c[:, 2] + dz)
                out.index_add_(0, q, wt[:, None] * v)
                mag.index_add_(0, q, (wt[:, None] * v).abs())
                den.index_add_(0, q, wt)
    if normalize:
        pos = (den > 0)[:, None]
        safe = torch.where(den > 0, den, torch.ones_like(den))[:, None]
        out, mag = torch.where(pos, out / safe, torch.zeros_like(out)), torch.where(pos, mag / safe.abs(), torch.zeros_like(mag))
    return out.reshape(X, Y, Z, C), mag.reshape(X, Y, Z, C), den.reshape(X, Y, Z)


# ---------------------------------------------------------------------------------------------------- 3. sample
def sample_ref(points, volume, grid):
    """Trilinear interpolation in double, the eight corners in lexicographic order of the offset -> (out [n], the sum of |terms| [n]); the cell is
    clamped into the grid (a point outside extrapolates its border cell); a non-finite point gives NaN."""
    X, Y, Z = grid.dims
    o, h = _oh(grid)
    t = (points.float().double() - o) / h
    bad = ~torch.isfinite(t).all(1)
    t = torch.where(bad[:, None], torch.zeros_like(t), t)
    top = torch.tensor([d - 2 for d in grid.dims], dtype=F64)
    c = torch.minimum(torch.maximum(torch.floor(t), torch.zeros(3, dtype=F64)), top)
    f = t - c
    c = c.long()
    vol = volume.double().reshape(-1)
    out, mag = torch.zeros(points.shape[0], dtype=F64), torch.zeros(points.shape[0], dtype=F64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                wx = f[:, 0] if dx else 1.0 - f[:, 0]
                wy = f[:, 1] if dy else 1.0 - f[:, 1]
                wz = f[:, 2] if dz else 1.0 - f[:, 2]
                term = ((wx * wy) * wz) * vol[((c[:, 0] + dx) * Y + (c[:, 1] + dy)) * Z + (c[:, 2] + dz)]
                out = out + term
                mag = mag + term.abs()
    nan = torch.full_like(out, float("nan"))
    return torch.where(bad, nan, out), torch.where(bad, nan, mag)


# ---------------------------------------------------------------------------------------------------- 4. right-hand side
def _shift(x, axis, step):
    """x(q + step e_axis), 0 outside the grid"""
    out = torch.zeros_like(x)
    n = x.shape[axis]
    src = [slice(None)] * x.dim()
    dst = [slice(None)] * x.dim()
    if step > 0:
        src[axis], dst[axis] = slice(1, n), slice(0, n - 1)
    else:
        src[axis], dst[axis] = slice(0, n - 1), slice(1, n)
    out[tuple(dst)] = x[tuple(src)]
    return out


def divergence_ref(V, grid):
    """b = -div V by central differences over 2 voxel_a, V = 0 outside -> (b [X,Y,Z], the sum of |terms|)"""
    _, h = _oh(grid)
    V = V.double()
    d, mag = [], torch.zeros(grid.dims, dtype=F64)
    for a in range(3):
        plus, minus = _shift(V[..., a], a, +1), _shift(V[..., a], a, -1)
        d.append((plus - minus) / (2.0 * h[a]))
        mag = mag + (plus.abs() + minus.abs()) / (2.0 * h[a])
    return -((d[0] + d[1]) + d[2]), mag


# ---------------------------------------------------------------------------------------------------- 5. operator
def apply_ref(x, grid, screening=None):
    """A x = sum_axes ((2 x - x_minus) - x_plus) / voxel_a^2 + s x, x = 0 outside (Dirichlet) -> (A x [X,Y,Z], the sum of |terms|)"""
    _, h = _oh(grid)
    x = x.double()
    parts, mag = [], torch.zeros(grid.dims, dtype=F64)
    for a in range(3):
        minus, plus = _shift(x, a, -1), _shift(x, a, +1)
        parts.append(((2.0 * x - minus) - plus) / (h[a] * h[a]))
        mag = mag + (2.0 * x.abs() + minus.abs() + plus.abs()) / (h[a] * h[a])
    out = (parts[0] + parts[1]) + parts[2]
    if screening is not None:
        out = out + screening.double() * x
        mag = mag + (screening.double() * x).abs()
    return out, mag


# ---------------------------------------------------------------------------------------------------- 6. solve
def cg_ref(b, grid, screening=None, x0=None, tol=1e-3, max_iterations=100, fp32_storage=False):
    """Conjugate gradients on A x = b from x0 (zero) -> (x, iterations, r.r, b.b).  fp32_storage: x, r, p and A p are rounded to fp32 after every
    update (the device's storage), the dot products stay in double; without it everything is float64.  Stops after the first iteration with
    r.r <= tol^2 b.b (before the first if the guess satisfies it) or after max_iterations."""
    rnd = r32 if fp32_storage else (lambda t: t)
    b = b.double()
    x = torch.zeros(grid.dims, dtype=F64) if x0 is None else x0.double().clone()
    r = rnd(b - rnd(apply_ref(x, grid, screening)[0]))
    p = r.clone()
    rr, bb = float((r * r).sum()), float((b * b).sum())
    it = 0
    while it < max_iterations and not rr <= tol * tol * bb:
        Ap = rnd(apply_ref(p, grid, screening)[0])
        pAp = float((p * Ap).sum())
        alpha = rr / pAp if pAp > 0 else 0.0
        x = rnd(x + alpha * p)
        r = rnd(r - alpha * Ap)
        rr_new = float((r * r).sum())
        beta = rr_new / rr if rr > 0 else 0.0
        p = rnd(r + beta * p)
        rr, it = rr_new, it + 1
    return x, it, rr, bb


# ---------------------------------------------------------------------------------------------------- 7. level, volume, trim
def level_ref(phi, phi_at_points, weights, kept):
    """iso = sum w phi(p) / sum w over the kept points with a finite weight and value, in double; values = (phi - iso) / max |phi - iso| -> fp32"""
    w = weights.double()
    ok = kept & torch.isfinite(w) & torch.isfinite(phi_at_points)
    iso = float((w[ok] * phi_at_points[ok]).sum() / w[ok].sum()) if bool(ok.any()) else 0.0
    d = phi.double() - iso
    top = float(d.abs().max())
    return (d / top if top > 0 else d).float(), iso


def quantile_ref(values, q):
    """the linear quantile: s[lo] + (s[hi] - s[lo]) (pos - lo), pos = q (n - 1), over the sorted values, in float64"""
    s = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    pos = float(q) * (s.size - 1)
    lo, hi = int(np.floor(pos)), int(np.ceil(pos))
    return float(s[lo]) + (float(s[hi]) - float(s[lo])) * (pos - lo)


def trim_ref(num_vertices, faces, densities, q):
    """-> (keep [V] bool, the surviving faces renumbered [F',3] int64): a vertex goes iff its density < the q quantile of all of them, a face goes
    iff it names such a vertex; survivors keep their order.  q == 0 keeps everything."""
    d = np.asarray(densities, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if q == 0 or num_vertices == 0:
        return np.ones(num_vertices, dtype=bool), faces
    keep = ~(d < quantile_ref(d, q))
    newid = np.full(num_vertices, -1, dtype=np.int64)
    newid[keep] = np.arange(int(keep.sum()))
    return keep, np.array([[newid[v] for v in f] for f in faces if keep[f].all()], dtype=np.int64).reshape(-1, 3)


DENSITY_FLOOR = 0.125


def reconstruct_ref(points, normals, resolution, box, density_normalize=True, density_downscale=4, screening=0.0, tol=1e-3, max_iterations=None,
                    fp32_storage=False):
    """The pipeline up to the meshed volume -> dict(grid, coarse, density_coarse, density, weights, b, phi, iterations, rr, bb, iso, values).
    fp32_storage rounds every stored array (densities, weights, V, b, the CG vectors) to fp32 as the device stores them; without it only the
    inputs and `values` are fp32."""
    rnd = r32 if fp32_storage else (lambda t: t)
    grid = grid_over_box(box, resolution)
    coarse = grid_over_box(box, tuple(max(d // density_downscale, 2) for d in grid.dims))
    density_c = rnd(splat_ref(points, coarse)[0][..., 0])
    density = rnd(splat_ref(points, grid)[0][..., 0])
    n = points.shape[0]
    w = rnd(1.0 / sample_ref(points, density_c, coarse)[0].clamp_min(DENSITY_FLOOR)) if density_normalize else torch.ones(n, dtype=F64)
    V = rnd(splat_ref(points, grid, normals, w)[0])
    b = rnd(divergence_ref(V, grid)[0])
    s = rnd(density * (float(screening) / float(np.mean(np.asarray(grid.voxel, dtype=np.float64) ** 2)))) if screening > 0 else None
    if max_iterations is None:
        max_iterations = 4 * max(grid.dims)
    phi, it, rr, bb = cg_ref(b, grid, s, None, tol, max_iterations, fp32_storage)
    values, iso = level_ref(phi, sample_ref(points, phi, grid)[0], w, bin_ref(points, grid)[0])
    return dict(grid=grid, coarse=coarse, density_coarse=density_c, density=density, weights=w, b=b, phi=phi, iterations=it, rr=rr, bb=bb, iso=iso,
                values=values)


PROJECT_OFFSET, PROJECT_MAX_STEP = 0.25, 0.5


def project_ref(vertices, values, grid, iterations=2):
    """Newton steps onto the zero level of the trilinear interpolant of `values`, in float64, rounded to fp32 after every step: v -= f g / |g|^2, f the
    interpolant at v, g its central difference over +-0.25 voxel per axis (the offset points rounded to fp32, as they are sampled), the step capped
    at half a voxel and skipped where g is zero or anything is not finite -> [V,3] fp32"""
    _, h = _oh(grid)
    v = vertices.float()
    eye = torch.eye(3, dtype=F64)
    for _ in range(iterations):
        p = v.double()
        f = sample_ref(v, values, grid)[0]
        g = torch.stack([(sample_ref((p + eye[a] * (PROJECT_OFFSET * h[a])).float(), values, grid)[0]
                          - sample_ref((p - eye[a] * (PROJECT_OFFSET * h[a])).float(), values, grid)[0]) / (2.0 * PROJECT_OFFSET * h[a]) for a in range(3)], 1)
        gg = (g * g).sum(1, keepdim=True)
        step = -f[:, None] * g / torch.where(gg > 0, gg, torch.ones_like(gg))
        length = (step / h).norm(dim=1, keepdim=True)
        step = step * torch.clamp(PROJECT_MAX_STEP / torch.where(length > 0, length, torch.ones_like(length)), max=1.0)
        ok = (gg > 0) & torch.isfinite(step).all(1, keepdim=True)
        v = (p + torch.where(ok, step, torch.zeros_like(step))).float()
    return v


def sphere_cloud(n=8000, radius=0.5, seed=0):
    """n points on the sphere of `radius` about the origin with their exact outward normals, fp32, from a seeded generator"""
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn((n, 3), generator=g, dtype=F64), dim=1)
    return (radius * d).float(), d.float()


def edge_crossings(values, grid, diagonals=False):
    """the linear zeros of `values` along the lattice edges whose ends differ in sign (negative: < 0) -> points [m,3] float64; the three axis
    edges per lattice point, with `diagonals` also the face and body diagonals of the extractor's tetrahedra (+xy +yz +xz +xyz)"""
    o, h = _oh(grid)
    v = values.double()
    X, Y, Z = grid.dims
    ijk = torch.stack(torch.meshgrid(torch.arange(X), torch.arange(Y), torch.arange(Z), indexing="ij"), -1).double()
    kinds = [(1, 0, 0), (0, 1, 0), (0, 0, 1)] + ([(1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)] if diagonals else [])
    out = []
    for e in kinds:
        lo = tuple(slice(0, d - k) for d, k in zip(grid.dims, e))
        hi = tuple(slice(k, d) for d, k in zip(grid.dims, e))
        va, vb = v[lo], v[hi]
        cross = (va < 0) != (vb < 0)
        t = va[cross] / (va[cross] - vb[cross])
        out.append(o + (ijk[lo][cross] + t[:, None] * torch.tensor(e, dtype=F64)) * h)
    return torch.cat(out)
