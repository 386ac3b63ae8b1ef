"""Restatement of the TSDF mesh export's entry points (include/thermal_nerf_hip.h: tn_tsdf_integrate, tn_mesh_count, tn_mesh_emit) in plain torch, and
the small analytic scene their tests share.

`integrate_ref` takes a dtype: in float64 it is the yardstick, in float32 it gives the floor of the convention (the kernel may miss float64 by
8 x what the float32 restatement misses it by).  `extract_ref` runs in float32 with the kernel's operation order, one torch operation per rounding,
so the kernel can be compared bit for bit.

Sign convention, made explicit: values < 0 are INSIDE the surface (the reference fuses sampled depth - voxel depth, positive in front of a surface),
the triangles' normals and the vertex normals point to the positive side.  A solid therefore stores a negative distance inside it; a cavity -- free
space enclosed by matter -- stores the negated field, and its mesh faces the enclosed free space."""
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64

# ---------------------------------------------------------------------------------------------------- the split
# corners of a cell: dx + 2 dy + 4 dz; tetrahedra (0, a, a + b, 7) for the six orders of the axes, lexicographic; odd orders are negatively oriented
TET_CORNER = torch.tensor([[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]])
TET_ODD = torch.tensor([0, 1, 1, 0, 0, 1], dtype=torch.bool)
KIND_MASK = (1, 2, 4, 3, 6, 5, 7)  # +x +y +z +xy +yz +xz +xyz as corner numbers
MASK_KIND = torch.tensor([0, 0, 1, 3, 2, 5, 4, 6])
TET_EDGE = torch.tensor([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]])
# the sign cases of a positively oriented tetrahedron (bit n: v_n < 0): triangles as edges of TET_EDGE, normals towards the positive values
CASE_TRIS = torch.tensor([0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0])
CASE_EDGE = torch.tensor([[0, 0, 0, 0, 0, 0], [0, 1, 2, 0, 0, 0], [0, 4, 3, 0, 0, 0], [4, 3, 1, 4, 1, 2], [1, 3, 5, 0, 0, 0], [3, 5, 2, 3, 2, 0],
                          [5, 1, 0, 5, 0, 4], [2, 4, 5, 0, 0, 0], [2, 5, 4, 0, 0, 0], [5, 4, 0, 5, 0, 1], [2, 5, 3, 2, 3, 0], [1, 5, 3, 0, 0, 0],
                          [4, 2, 1, 4, 1, 3], [0, 3, 4, 0, 0, 0], [0, 2, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0]])


def _off(mask):
    return mask & 1, (mask >> 1) & 1, mask >> 2


# ---------------------------------------------------------------------------------------------------- integration
def camera_records(c2w, intrinsics):
    """c2w [B,3,4] and (fx, fy, cx, cy) [B,4] -> the [B,16] fp32 records: world -> camera by the analytic inverse in float64, rounded once."""
    c2w = torch.as_tensor(c2w, dtype=F64)
    Rt = c2w[:, :3, :3].transpose(1, 2)
    w2c = torch.cat([Rt, -Rt @ c2w[:, :3, 3:4]], dim=2)
    return torch.cat([w2c.reshape(-1, 12), torch.as_tensor(intrinsics, dtype=F64)], dim=1).float()


def integrate_ref(values, weights, rgbt, origin, voxel_size, truncation, max_weight, records, depth, frame_rgbt, accumulation=None,
                  min_accumulation=0.5, depth_kind="ray", dtype=F64, details=None):
    """tn_tsdf_integrate on fp32 inputs, evaluated in `dtype`.  -> (values, weights, rgbt) in `dtype`, the inputs are left alone.  `details`, when a
    dict, receives "near" (bool [X,Y,Z]: for some frame the voxel's pixel coordinate lies within 1e-4 pixel of a rounding boundary of a pixel
    in or next to the image, or its dist + truncation within 1e-4 truncation of 0) and "touched" (bool: some frame updated the voxel)."""
    dev = values.device  # (the inputs may sit on a device: scripts/time_tsdf_mesh.py times this path there as the torch baseline)
    t = lambda a: torch.as_tensor(a, dtype=F32).to(dev, dtype)  # noqa: E731  (every scalar reaches the kernel as an fp32)
    X, Y, Z = values.shape
    val, w, c = values.to(dtype).clone(), weights.to(dtype).clone(), rgbt.to(dtype).clone()
    o, s, trunc, maxw, mina = t(origin), t(voxel_size), t(truncation), t(max_weight), t(min_accumulation)
    i, j, k = torch.meshgrid(torch.arange(X, device=dev), torch.arange(Y, device=dev), torch.arange(Z, device=dev), indexing="ij")
    px, py, pz = o[0] + i.to(dtype) * s[0], o[1] + j.to(dtype) * s[1], o[2] + k.to(dtype) * s[2]
    B, H, W = depth.shape
    near = torch.zeros((X, Y, Z), dtype=torch.bool, device=dev)
    touched = torch.zeros((X, Y, Z), dtype=torch.bool, device=dev)
    for b in range(B):
        m = records[b].to(dtype)
        x = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3]
        y = -(((m[4] * px + m[5] * py) + m[6] * pz) + m[7])
        z = -(((m[8] * px + m[9] * py) + m[10] * pz) + m[11])
        front = z > 0
        zs = torch.where(front, z, torch.ones_like(z))
        vd = torch.sqrt((x * x + y * y) + z * z) if depth_kind == "ray" else z
        ru, rv = (m[12] * (x / zs) + m[14]) - 0.5, (m[13] * (y / zs) + m[15]) - 0.5
        fu, fv = torch.round(ru), torch.round(rv)  # half to even
        inb = front & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        iu, iv = fu.clamp(0, W - 1).long(), fv.clamp(0, H - 1).long()
        d = torch.where(inb, depth[b].to(dtype)[iv, iu], torch.zeros_like(z))
        if accumulation is not None:
            d = torch.where(accumulation[b].to(dtype)[iv, iu] < mina, torch.zeros_like(d), d)
        dist = d - vd
        valid = inb & (vd > 0) & (d > 0) & (dist > -trunc)
        tsdf = torch.clamp(dist / trunc, -1.0, 1.0)
        tw = w + 1.0
        val = torch.where(valid, (val * w + tsdf) / tw, val)
        c = torch.where(valid[..., None], (c * w[..., None] + frame_rgbt[b].to(dtype)[iv, iu]) / tw[..., None], c)
        w = torch.where(valid, torch.minimum(tw, maxw), w)
        touched |= valid
        if details is not None:
            by_image = front & (fu >= -1) & (fu <= W) & (fv >= -1) & (fv <= H)
            edge = lambda r: ((r - torch.floor(r)) - 0.5).abs() < 1e-4  # noqa: E731
            near |= by_image & (edge(ru) | edge(rv))
            near |= inb & (d > 0) & ((dist + trunc).abs() < 1e-4 * trunc)
    if details is not None:
        details.update(near=near, touched=touched)
    return val, w, c


# ---------------------------------------------------------------------------------------------------- extraction
def _gradient(v, voxel_size):
    """[X,Y,Z,3] fp32: central differences of v, one-sided at the border, 0 along an axis of one point; over the voxel size."""
    g = []
    for axis in range(3):
        n = v.shape[axis]
        d = torch.zeros_like(v)
        if n > 1:
            mv = v.movedim(axis, 0)
            dm = d.movedim(axis, 0)
            dm[0] = mv[1] - mv[0]
            dm[n - 1] = mv[n - 1] - mv[n - 2]
            if n > 2:
                dm[1:n - 1] = (mv[2:] - mv[:n - 2]) * 0.5
        g.append(d / voxel_size[axis])
    return torch.stack(g, dim=-1)


def _sqrt32(x):
    """The correctly rounded fp32 square root, which is what sqrtf gives on the device: numpy's float64 sqrt rounded once more (torch's vectorised
    host sqrt is not correctly rounded on every CPU).  A tensor on a device takes torch's sqrt there."""
    if x.is_cuda:
        return torch.sqrt(x)
    return torch.from_numpy(np.sqrt(x.numpy().astype(np.float64)).astype(np.float32))


def cell_mask(weights, observed_only):
    """bool [X-1,Y-1,Z-1]: the cells that emit triangles."""
    X, Y, Z = weights.shape
    ok = torch.ones((X - 1, Y - 1, Z - 1), dtype=torch.bool, device=weights.device)
    if observed_only:
        for c in range(8):
            dx, dy, dz = _off(c)
            ok &= weights[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz] > 0
    return ok


def extract_ref(values, weights, rgbt, origin, voxel_size, observed_only=False):
    """tn_mesh_count + tn_mesh_emit in torch, on the device the volume is on.  -> dict: vertices [V,3], normals [V,3], rgbt [V,4] fp32, faces [F,3] int32, and for the tests
    `edge_point` [V,3] int64 (the lattice point of each vertex), `edge_kind` [V], `t` [V], `cases` (the set of sign cases met, 0..15)."""
    dev = values.device
    values, weights, rgbt = values.to(F32), weights.to(F32), rgbt.to(F32)
    origin, voxel_size = torch.as_tensor(origin, dtype=F32).to(dev), torch.as_tensor(voxel_size, dtype=F32).to(dev)
    tet_corner, mask_kind, tet_edge, case_tris, case_edge = (a.to(dev) for a in (TET_CORNER, MASK_KIND, TET_EDGE, CASE_TRIS, CASE_EDGE))
    zero = torch.zeros(1, device=dev)
    X, Y, Z = values.shape
    if min(X, Y, Z) < 2:
        return {"vertices": torch.zeros((0, 3)), "normals": torch.zeros((0, 3)), "rgbt": torch.zeros((0, 4)), "faces": torch.zeros((0, 3), dtype=torch.int32),
                "edge_point": torch.zeros((0, 3), dtype=torch.int64), "edge_kind": torch.zeros(0, dtype=torch.int64), "t": torch.zeros(0), "cases": set()}
    v = values.clamp(-1.0, 1.0)
    inside = v < 0
    cells = cell_mask(weights, observed_only)
    pad = torch.zeros((X + 1, Y + 1, Z + 1), dtype=torch.bool, device=dev)  # pad[i + 1, j + 1, k + 1] = cell (i, j, k); cells outside the volume are False
    pad[1:X, 1:Y, 1:Z] = cells
    flags = torch.zeros((X, Y, Z, 7), dtype=torch.bool, device=dev)
    for q, m in enumerate(KIND_MASK):
        dx, dy, dz = _off(m)
        cross = inside[:X - dx, :Y - dy, :Z - dz] != inside[dx:, dy:, dz:]
        used = torch.zeros_like(cross)
        for a in range(2 - dx):  # the cells around the edge: one step back along every axis the edge does not run along
            for b in range(2 - dy):
                for c in range(2 - dz):
                    used |= pad[1 - a:1 - a + X - dx, 1 - b:1 - b + Y - dy, 1 - c:1 - c + Z - dz]
        flags[:X - dx, :Y - dy, :Z - dz, q] = cross & used
    flat = flags.reshape(-1, 7)
    vid = (torch.cumsum(flat.reshape(-1).long(), 0) - 1).reshape(-1, 7)  # exclusive prefix sum of the flags at the flagged edges
    pq = torch.nonzero(flat)  # (lattice point, kind) in that order
    p, q = pq[:, 0], pq[:, 1]
    k, j, i = p % Z, (p // Z) % Y, p // (Y * Z)
    m = torch.tensor(KIND_MASK, device=dev)[q]
    e = torch.stack([m & 1, (m >> 1) & 1, m >> 2], dim=-1)
    i1, j1, k1 = i + e[:, 0], j + e[:, 1], k + e[:, 2]
    a, b = v[i, j, k], v[i1, j1, k1]
    t = a / (a - b)
    ijk = torch.stack([i, j, k], dim=-1)
    vertices = origin + (ijk.float() + torch.where(e.bool(), t[:, None], zero)) * voxel_size
    g = _gradient(v, voxel_size)
    g0, g1 = g[i, j, k], g[i1, j1, k1]
    gi = g0 + t[:, None] * (g1 - g0)
    length = _sqrt32((gi[:, 0] * gi[:, 0] + gi[:, 1] * gi[:, 1]) + gi[:, 2] * gi[:, 2])[:, None]
    normals = torch.where(length > 0, gi / length, zero)
    p1 = (i1 * Y + j1) * Z + k1
    src = torch.where(t <= 0.5, p, p1)
    wflat = weights.reshape(-1)
    src = torch.where(wflat[src] > 0, src, p + p1 - src)
    out_rgbt = rgbt.reshape(-1, 4)[src]
    # faces: (cell, tetrahedron, triangle) order
    cidx = torch.nonzero(cells)  # row-major = the lattice order of the cells' lowest corners
    ci, cj, ck = cidx[:, 0], cidx[:, 1], cidx[:, 2]
    cube = torch.stack([inside[ci + dx, cj + dy, ck + dz] for dx, dy, dz in (_off(c) for c in range(8))], dim=-1).long()  # [C,8]
    case = sum(cube[:, tet_corner[:, n]] << n for n in range(4))  # [C,6]
    lo_of, hi_of = tet_corner[:, tet_edge[:, 0]], tet_corner[:, tet_edge[:, 1]]  # [6 tetrahedra, 6 edges]: the two corners of an edge, as cell corners
    tris, keeps = [], []
    for n in range(6):  # tetrahedron by tetrahedron: plain table look-ups
        edges = case_edge[case[:, n]].reshape(-1, 2, 3)  # [C,2,3] edge numbers of the (at most two) triangles
        lo, hi = lo_of[n][edges], hi_of[n][edges]
        owner = ((ci[:, None, None] + (lo & 1)) * Y + (cj[:, None, None] + ((lo >> 1) & 1))) * Z + (ck[:, None, None] + (lo >> 2))
        tri = vid[owner, mask_kind[hi ^ lo]]
        tris.append(tri[..., [0, 2, 1]] if bool(TET_ODD[n]) else tri)
        keeps.append(torch.arange(2, device=dev)[None, :] < case_tris[case[:, n]][:, None])
    tri, keep = torch.stack(tris, dim=1), torch.stack(keeps, dim=1)  # [C,6,2,3], [C,6,2]
    faces = tri[keep].to(torch.int32)
    return {"vertices": vertices, "normals": normals, "rgbt": out_rgbt, "faces": faces, "edge_point": ijk, "edge_kind": q, "t": t,
            "cases": set(torch.unique(case).tolist())}


# ---------------------------------------------------------------------------------------------------- the scene
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """camera_to_world [3,4] float64 in nerfstudio's convention (x right, y up, z back) of a camera at `eye` that looks at `target`."""
    eye, target, up = (torch.tensor(v, dtype=F64) for v in (eye, target, up))
    back = torch.nn.functional.normalize(eye - target, dim=0)
    right = torch.nn.functional.normalize(torch.linalg.cross(up, back), dim=0)
    return torch.stack([right, torch.linalg.cross(back, right), back, eye], dim=1)


def scene_cameras(B, H=48, W=64, radius=2.6, seed=0):
    """B look-at cameras on a tilted ring outside the unit box, none aligned with an axis, each with its own focal lengths (60..69, 58..64 at 64 x 48,
    scaled with the image) and a principal point half a pixel off centre.  -> c2w [B,3,4] float64, intrinsics [B,4] float64."""
    g = np.random.default_rng(seed)
    c2w, intr = [], []
    for b in range(B):
        az = 0.37 + 2 * math.pi * b / B + 0.11 * g.uniform(-1, 1)
        el = 0.23 + 0.5 * math.sin(1.7 * b + 0.4)
        r = radius * (1 + 0.08 * g.uniform(-1, 1))
        eye = (r * math.cos(el) * math.cos(az), r * math.cos(el) * math.sin(az), r * math.sin(el))
        c2w.append(look_at(eye, (0.03 * math.sin(b), 0.02 * math.cos(2 * b), 0.01 * b / B)))
        intr.append([(60.0 + 9.0 * g.uniform()) * W / 64, (58.0 + 6.0 * g.uniform()) * H / 48, W / 2 + 0.5, H / 2 - 0.5])
    return torch.stack(c2w), torch.tensor(intr, dtype=F64)


def sphere_frames(c2w, intrinsics, H, W, radius=0.6, seed=0, depth_kind="ray"):
    """Analytic depth of a sphere of `radius` at the origin for every pixel centre (0 where the ray misses), random RGB+T and an accumulation
    that is 1 on the sphere and 0 off it.  -> depth [B,H,W], rgbt [B,H,W,4], accumulation [B,H,W], fp32."""
    B = c2w.shape[0]
    g = torch.Generator().manual_seed(seed)
    v, u = torch.meshgrid(torch.arange(H, dtype=F64) + 0.5, torch.arange(W, dtype=F64) + 0.5, indexing="ij")
    depth = torch.zeros((B, H, W), dtype=F64)
    for b in range(B):
        fx, fy, cx, cy = intrinsics[b].tolist()
        d_cam = torch.stack([(u - cx) / fx, -(v - cy) / fy, -torch.ones_like(u)], dim=-1)  # z = -1 plane: |z| of a point = its ray parameter
        d = d_cam @ c2w[b, :, :3].T
        o = c2w[b, :, 3]
        qa, qb, qc = (d * d).sum(-1), 2 * (d @ o), (o * o).sum() - radius * radius
        disc = qb * qb - 4 * qa * qc
        s = (-qb - torch.sqrt(disc.clamp_min(0))) / (2 * qa)
        hit = (disc > 0) & (s > 0)
        depth[b] = torch.where(hit, s * (torch.sqrt(qa) if depth_kind == "ray" else 1.0), torch.zeros_like(s))
    return depth.float(), torch.rand((B, H, W, 4), generator=g), (depth > 0).float()


def fresh_volume(dims):
    return torch.full(dims, -1.0), torch.zeros(dims), torch.zeros(tuple(dims) + (4,))


def box_grid(dims, lo=(-1.0, -0.9, -0.8), hi=(1.0, 0.9, 0.8)):
    """origin and voxel size (fp32) of a volume of `dims` voxels over lo..hi, as TSDF.from_aabb computes them."""
    lo, hi = torch.tensor(lo, dtype=F32), torch.tensor(hi, dtype=F32)
    return lo, (hi - lo) / torch.tensor(dims)
