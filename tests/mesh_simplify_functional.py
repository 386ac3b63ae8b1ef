"""Restatement of the mesh simplification (include/thermal_nerf_hip.h: tn_mesh_simplify_count, tn_mesh_simplify_plan, tn_mesh_simplify_emit; the
algorithm is stated in the header comment of csrc/tn_mesh_simplify.hip) in numpy, and of the face-budget search of mesh.simplify_to_target.

The cell keys are evaluated in float32 with the kernel's own expression, so cluster membership is exact; everything else is float64 with the kernel's
operation order (np.add.at adds its records one by one, in the order given: ascending vertex index for the means, ascending face index for the
quadrics).  Positions, normals and RGB+T are returned in float64, before the one rounding to float32 the kernel applies."""
import numpy as np

F32, F64 = np.float32, np.float64
MAX_CELLS = 2 ** 31
CELL_REACH = 0.500001  # a solved vertex may lie this many cells from its cell's centre: the closed cell and a margin of 1e-6 cell (tn_mesh_simplify.hip)


def _np(a, dtype):
    return np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=dtype)


def _grid(origin, cell, dims):
    o, c = _np(origin, F32).reshape(3), _np(cell, F32).reshape(3)
    d = tuple(int(v) for v in dims)
    assert len(d) == 3 and min(d) >= 1 and d[0] * d[1] * d[2] < MAX_CELLS and bool((c > 0).all())
    return o, c, d


def cell_keys(vertices, origin, cell, dims):
    """-> (key [V] int64, cell index [V,3] int64): floor((v - origin) / cell) in float32, clamped to [0, dims - 1], a NaN to 0."""
    o, c, d = _grid(origin, cell, dims)
    v = _np(vertices, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        t = np.floor((v - o) / c).astype(F64)
    idx = np.where(t > 0, np.minimum(t, np.array(d, dtype=F64) - 1), 0.0).astype(np.int64)
    return (idx[:, 0] * d[1] + idx[:, 1]) * d[2] + idx[:, 2], idx


def _valid_faces(faces, V):
    f = _np(faces, np.int64).reshape(-1, 3)
    return f, ((f >= 0) & (f < V)).all(axis=1)


def count_ref(vertices, faces, origin, cell, dims):
    """tn_mesh_simplify_count: the faces whose three corners have three different keys."""
    key, _ = cell_keys(vertices, origin, cell, dims)
    f, ok = _valid_faces(faces, key.shape[0])
    k = key[f[ok]]
    return int(((k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])).sum())


def solve_ldlt(m00, m01, m02, m11, m12, m22, r0, r1, r2):
    """(A + eps I) x = r by LDL^T, the kernel's operations in the kernel's order."""
    l10, l20 = m01 / m00, m02 / m00
    d1 = m11 - l10 * m01
    t = m12 - l20 * m01
    l21 = t / d1
    d2 = (m22 - l20 * m02) - l21 * t
    y1 = r1 - l10 * r0
    y2 = (r2 - l20 * r0) - l21 * y1
    x2 = y2 / d2
    x1 = y1 / d1 - l21 * x2
    x0 = (r0 / m00 - l10 * x1) - l20 * x2
    return np.stack([x0, x1, x2], axis=-1)


def simplify_ref(vertices, faces, normals, rgbt, origin, cell, dims, regularization=1e-3, details=None):
    """tn_mesh_simplify_plan + tn_mesh_simplify_emit.  -> dict: vertices [Vo,3], normals [Vo,3], rgbt [Vo,4] float64 (not yet rounded), faces [Fo,3]
    int32.  `details`, when a dict, receives, per EMITTED vertex: "near" (the solved point lies within 1e-9 cell of the reach the rule allows it, CELL_REACH:
    the outside-the-cell decision may go either way), "solved" (the quadric's point was taken, not the mean), "mean" [Vo,3] (the cluster's mean vertex),
    "centre" and "cell" (of its cell), "members" (its input vertices); and "clusters" (their number, unreferenced ones included), "cluster_of" [V]
    (the output vertex of every input vertex, -1 where its cluster is not emitted), "kept" (the input indices of the surviving faces), "count"."""
    o, c, d = _grid(origin, cell, dims)
    o64, c64 = o.astype(F64), c.astype(F64)
    reg = F64(F32(regularization))
    v32 = _np(vertices, F32).reshape(-1, 3)
    v64, n64, a64 = v32.astype(F64), _np(normals, F32).reshape(-1, 3).astype(F64), _np(rgbt, F32).reshape(-1, 4).astype(F64)
    V = v64.shape[0]
    f, ok = _valid_faces(faces, V)
    key, idx = cell_keys(v32, o, c, d)
    uniq, first, cluster_of = np.unique(key, return_index=True, return_inverse=True)  # clusters in ascending key order
    cluster_of = cluster_of.reshape(-1)
    C = uniq.shape[0]
    centre = o64 + (idx[first].astype(F64) + 0.5) * c64
    # the vertex segments, in ascending vertex index
    members = np.bincount(cluster_of, minlength=C).astype(F64)
    msum, nsum, asum = np.zeros((C, 3)), np.zeros((C, 3)), np.zeros((C, 4))
    np.add.at(msum, cluster_of, v64 - centre[cluster_of])
    np.add.at(nsum, cluster_of, n64)
    np.add.at(asum, cluster_of, a64)
    with np.errstate(all="ignore"):
        mean = msum / members[:, None]
        # the quadrics: corner records in (face, corner) order
        fv = f[ok]
        p0 = v64[fv[:, 0]]
        e1, e2 = v64[fv[:, 1]] - p0, v64[fv[:, 2]] - p0
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=-1)
        cl = cluster_of[fv] if V else np.zeros((0, 3), dtype=np.int64)
        rec_cluster, rec_face = cl.reshape(-1), np.repeat(np.arange(fv.shape[0]), 3)
        q = p0[rec_face] - centre[rec_cluster]
        rn = n[rec_face]
        dist = (rn[:, 0] * q[:, 0] + rn[:, 1] * q[:, 1]) + rn[:, 2] * q[:, 2]
        A, b = np.zeros((C, 6)), np.zeros((C, 3))
        np.add.at(A, rec_cluster, np.stack([rn[:, 0] * rn[:, 0], rn[:, 0] * rn[:, 1], rn[:, 0] * rn[:, 2], rn[:, 1] * rn[:, 1], rn[:, 1] * rn[:, 2],
                                            rn[:, 2] * rn[:, 2]], axis=-1))
        np.add.at(b, rec_cluster, dist[:, None] * rn)
        trace = (A[:, 0] + A[:, 3]) + A[:, 5]
        eps = reg * trace
        x = solve_ldlt(A[:, 0] + eps, A[:, 1], A[:, 2], A[:, 3] + eps, A[:, 4], A[:, 5] + eps, b[:, 0] + eps * mean[:, 0], b[:, 1] + eps * mean[:, 1],
                       b[:, 2] + eps * mean[:, 2])
        reach = CELL_REACH * c64
        solved = (trace != 0.0) & (np.abs(x) <= reach).all(axis=1)
        near = (trace != 0.0) & (np.abs(np.abs(x) - reach) < 1e-9 * c64).any(axis=1)
        position = centre + np.where(solved[:, None], x, mean)
        length = np.sqrt((nsum[:, 0] * nsum[:, 0] + nsum[:, 1] * nsum[:, 1]) + nsum[:, 2] * nsum[:, 2])
        normal = np.where((length > 0)[:, None], nsum / length[:, None], 0.0)
        colour = asum / members[:, None]
    # the faces
    tri = np.sort(cl, axis=1)
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2])
    is_first = np.zeros(tri.shape[0], dtype=bool)
    if tri.shape[0]:
        is_first[np.unique(tri, axis=0, return_index=True)[1]] = True  # the first face of every triple, in input order
    keep = distinct & is_first
    used = np.zeros(C, dtype=bool)
    used[cl[keep].reshape(-1)] = True
    newid = np.cumsum(used) - 1
    out_faces = newid[cl[keep]].astype(np.int32).reshape(-1, 3)
    if details is not None:
        order = np.argsort(cluster_of, kind="stable")
        starts = np.concatenate([[0], np.cumsum(members.astype(np.int64))])
        details.update(near=near[used], solved=solved[used], mean=(centre + mean)[used], centre=centre[used], cell=idx[first][used],
                       members=[order[starts[k]:starts[k + 1]] for k in np.nonzero(used)[0]], clusters=C,
                       cluster_of=np.where(used[cluster_of], newid[cluster_of], -1) if V else np.zeros(0, dtype=np.int64),
                       kept=np.nonzero(ok)[0][keep], count=int(distinct.sum()))
    return {"vertices": position[used], "normals": normal[used], "rgbt": colour[used], "faces": out_faces}


# ---------------------------------------------------------------------------------------------------- the grid and the search
def extent_of(vertices):
    v = _np(vertices, F32).reshape(-1, 3)
    return np.stack([v.min(axis=0), v.max(axis=0)]) if v.shape[0] else np.zeros((2, 3), dtype=F32)


def grid_ref(extent, cell, origin=None):
    """mesh.simplify_grid: origin (the smallest coordinates minus half a cell, in float32, unless given) and dims (the largest coordinates' cell + 1)."""
    cell = _np(cell, F32).reshape(3)
    origin = extent[0] - cell * F32(0.5) if origin is None else _np(origin, F32).reshape(3)
    with np.errstate(all="ignore"):
        top = np.floor((extent[1] - origin) / cell).astype(F64)
    top = np.where(top > 0, np.minimum(top, float(MAX_CELLS)), 0.0)
    return origin, tuple(int(t) + 1 for t in top)


def search_ref(vertices, faces, target, unit, origin=None, start=0.25, bisections=12):
    """mesh.simplify_to_target's search -> (scale s, cell = s * unit in float32, origin, dims), or None where the mesh is within the target already:
    s doubles from 1/4 until count_ref is within the target, then 12 bisections on the geometric mean; the upper end of the bracket is used."""
    f = _np(faces, np.int64).reshape(-1, 3)
    if f.shape[0] <= target:
        return None
    unit = np.broadcast_to(_np(unit, F32).reshape(-1), (3,)).astype(F64)
    extent = extent_of(vertices)

    def grid(scale):
        cell = (F64(scale) * unit).astype(F32)
        return (cell,) + grid_ref(extent, cell, origin)

    def within(scale):
        cell, o, dims = grid(scale)
        if dims[0] * dims[1] * dims[2] >= MAX_CELLS:
            return False
        return count_ref(vertices, f, o, cell, dims) <= target

    hi = start
    while not within(hi):
        hi *= 2.0
    lo = hi / 2.0
    for _ in range(bisections):
        mid = float(np.sqrt(F64(lo) * F64(hi)))
        if within(mid):
            hi = mid
        else:
            lo = mid
    return (hi,) + grid(hi)


def ulp32(x):
    """The spacing of float32 at |x| (of the smallest normal below it)."""
    return np.spacing(np.maximum(np.abs(np.asarray(x, dtype=F64)), np.finfo(F32).tiny).astype(F32)).astype(F64)
