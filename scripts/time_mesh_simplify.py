"""The mesh simplification at export sizes (profiles/mesh_simplify.md): the meshes of scripts/time_tsdf_mesh.py -- the analytic sphere scene fused into a
128^3 and a 256^3 volume and extracted -- through `simplify_mesh` at a cell of 2 voxels (tn_mesh_simplify_plan + tn_mesh_simplify_emit) and through
`simplify_to_target` at 50 000 faces (the reference's default budget; about 20 calls of tn_mesh_simplify_count, a read-back each, then one
simplification), against the same clustering written in plain torch on the same device (`torch_simplify` below: unique / index_add_ /
linalg.solve in float64; not the code under test, and its sums are atomic, so its last bits vary from run to run).

    python scripts/time_mesh_simplify.py [--sizes 128 256] [--cell 2] [--target 50000] [--repeats 20] [--warmup 3] [--torch-repeats 5] [--no-torch]

Times are HIP events around one call after warm-up, the median of --repeats (the spread is reported too); both calls include their read-backs and
the allocation of their outputs and workspace.  Peak temporary memory is torch's allocator high-water mark above the inputs: the workspace and the
outputs for the HIP path.  One JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
import tsdf_functional as tf  # noqa: E402
from nerfstudio_thermal_amd import mesh  # noqa: E402
from nerfstudio_thermal_amd.splat_camera import PinholeCamera  # noqa: E402
from time_tsdf_mesh import timed  # noqa: E402

F64 = torch.float64


def torch_simplify(m, origin, cell, dims, regularization=1e-3):
    """The clustering of tn_mesh_simplify_plan / _emit in plain torch on the mesh's device -> Mesh."""
    dev = m.vertices.device
    o, c = torch.as_tensor(origin, dtype=torch.float32, device=dev), torch.as_tensor(cell, dtype=torch.float32, device=dev)
    d = torch.tensor(dims, device=dev)
    idx = torch.minimum(torch.floor((m.vertices - o) / c).clamp_min(0).long(), d - 1)
    key = (idx[:, 0] * d[1] + idx[:, 1]) * d[2] + idx[:, 2]
    uniq, cluster_of = torch.unique(key, return_inverse=True)
    C = uniq.numel()
    ci = torch.stack([uniq // (d[1] * d[2]), (uniq // d[2]) % d[1], uniq % d[2]], dim=-1)
    centre = o.double() + (ci.double() + 0.5) * c.double()
    v = m.vertices.double()
    members = torch.zeros(C, dtype=F64, device=dev).index_add_(0, cluster_of, torch.ones(v.shape[0], dtype=F64, device=dev))
    mean = torch.zeros((C, 3), dtype=F64, device=dev).index_add_(0, cluster_of, v - centre[cluster_of]) / members[:, None]
    nsum = torch.zeros((C, 3), dtype=F64, device=dev).index_add_(0, cluster_of, m.normals.double())
    colour = torch.zeros((C, 4), dtype=F64, device=dev).index_add_(0, cluster_of, m.rgbt.double()) / members[:, None]
    f = m.faces.long()
    cl = cluster_of[f]
    p0 = v[f[:, 0]]
    n = torch.linalg.cross(v[f[:, 1]] - p0, v[f[:, 2]] - p0)
    rec = cl.reshape(-1)
    rn = n.repeat_interleave(3, dim=0)
    dist = (rn * (p0.repeat_interleave(3, dim=0) - centre[rec])).sum(-1)
    A = torch.zeros((C, 3, 3), dtype=F64, device=dev).index_add_(0, rec, rn[:, :, None] * rn[:, None, :])
    b = torch.zeros((C, 3), dtype=F64, device=dev).index_add_(0, rec, dist[:, None] * rn)
    trace = A.diagonal(dim1=1, dim2=2).sum(-1)
    eye = torch.eye(3, dtype=F64, device=dev)
    eps = float(regularization) * trace
    has = trace > 0
    x = torch.linalg.solve(torch.where(has[:, None, None], A + eps[:, None, None] * eye, eye), b + eps[:, None] * mean)
    take = has & (x.abs() <= 0.5 * c.double()).all(dim=-1)
    position = centre + torch.where(take[:, None], x, mean)
    length = nsum.norm(dim=-1, keepdim=True)
    normal = torch.where(length > 0, nsum / length.clamp_min(1e-300), torch.zeros_like(nsum))
    tri = cl.sort(dim=1).values
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2])
    packed = (tri[:, 0] * C + tri[:, 1]) * C + tri[:, 2]  # C below 2^21
    _, inverse = torch.unique(packed, return_inverse=True)
    number = torch.arange(f.shape[0], device=dev)
    first = torch.full((int(inverse.max()) + 1 if f.shape[0] else 0,), f.shape[0], device=dev).scatter_reduce_(0, inverse, number, "amin")
    keep = distinct & (first[inverse] == number)
    used = torch.zeros(C, dtype=torch.bool, device=dev)
    used[cl[keep].reshape(-1)] = True
    newid = torch.cumsum(used.long(), 0) - 1
    return mesh.Mesh(position[used].float(), newid[cl[keep]].int(), normal[used].float(), colour[used].float())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--cell", type=float, default=2.0, help="the cell of the simplify_mesh timing, in voxels")
    ap.add_argument("--target", type=int, default=50000, help="the face budget of the simplify_to_target timing")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the HIP path only")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "time_mesh_simplify.py needs a GPU"
    dev = torch.device("cuda", 0)
    B, H, W = args.frames, args.height, args.width
    c2w, intr = tf.scene_cameras(B, H, W, seed=0)
    c2w, intr = c2w.float(), intr.float()
    depth, rgbt, acc = (t.to(dev) for t in tf.sphere_frames(c2w.double(), intr.double(), H, W, seed=0))
    cams = [PinholeCamera(c2w[b], *(float(v) for v in intr[b]), W, H) for b in range(B)]
    results = []
    for n in args.sizes:
        vol = mesh.TSDFVolume.from_aabb([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], (n, n, n), device=dev)
        vol.integrate(cams, depth, rgbt, acc)
        m = vol.get_mesh()
        origin = mesh.lattice_centred_origin(vol)
        cell = mesh.search_cell(args.cell, vol.voxel_size.numpy())
        _, dims = mesh.simplify_grid(mesh.vertex_extent(m.vertices), cell, origin)
        V, Fn = int(m.vertices.shape[0]), int(m.faces.shape[0])
        r = {"volume": n, "vertices": V, "faces": Fn, "workspace_bytes": int(mesh.simplify_workspace(V, Fn, dev).numel()), "cell_voxels": args.cell,
             "grid": list(dims)}
        out = mesh.simplify_mesh(m, cell, origin=origin, dims=dims)
        hip = timed(lambda: mesh.simplify_mesh(m, cell, origin=origin, dims=dims), args.repeats, args.warmup)
        r.update({"simplify_vertices": int(out.vertices.shape[0]), "simplify_faces": int(out.faces.shape[0]), "simplify_hip_ms": hip[0],
                  "simplify_hip_ms_min_max": [hip[1], hip[2]], "simplify_hip_peak_temporary_bytes": hip[3]})
        small, chosen = mesh.simplify_to_target(m, args.target, vol.voxel_size, origin=origin)
        tgt = timed(lambda: mesh.simplify_to_target(m, args.target, vol.voxel_size, origin=origin), args.repeats, args.warmup)
        r.update({"target": args.target, "target_vertices": int(small.vertices.shape[0]), "target_faces": int(small.faces.shape[0]),
                  "target_cell_voxels": None if chosen is None else chosen[0] / float(vol.voxel_size[0]), "target_hip_ms": tgt[0],
                  "target_hip_ms_min_max": [tgt[1], tgt[2]], "target_hip_peak_temporary_bytes": tgt[3]})
        if not args.no_torch:
            try:
                tor = timed(lambda: torch_simplify(m, origin, cell, dims), args.torch_repeats, 1)
                want = torch_simplify(m, origin, cell, dims)
                same = tuple(want.faces.shape) == tuple(out.faces.shape) and bool(torch.equal(want.faces, out.faces))
                r.update({"simplify_torch_ms": tor[0], "simplify_torch_ms_min_max": [tor[1], tor[2]], "simplify_torch_peak_temporary_bytes": tor[3],
                          "simplify_speedup": tor[0] / hip[0], "simplify_faces_equal": same,
                          "simplify_max_position_difference": float((want.vertices - out.vertices).abs().max()) if same else None})
                del want
            except torch.cuda.OutOfMemoryError:
                r["simplify_torch_ms"] = "out of memory"
        results.append(r)
        del vol, m, out, small
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
