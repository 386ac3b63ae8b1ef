"""The TSDF mesh export without a GPU: the float64 restatement of the fusion (tsdf_functional.integrate_ref) against the live reference where its
tree is present and against the reference's recorded volumes (tests/golden/tsdf_reference.npz, scripts/make_golden_tsdf.py); the float32 restatement
of the extraction (tsdf_functional.extract_ref, what the kernels are compared with bit for bit on the GPU) on exact distance samples of a sphere --
topology, orientation, and geometric errors within bounds derived from the tetrahedra's size and the sphere's curvature --; its edge cases; the PLY
writer's round trip; and the host-side argument checks of the three entry points."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import tsdf_functional as tf
from nerfstudio_thermal_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tsdf_reference.npz")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

F32, F64 = torch.float32, torch.float64
AABB = ((-1.0, -0.9, -0.8), (1.0, 0.9, 0.8))
MAX_EXCLUDED = 0.01  # share of the voxels the discontinuities may take out of a comparison


# ---------------------------------------------------------------------------------------------------- 1. the fusion
def _scene(dims=(24, 20, 16), B=4, H=48, W=64, seed=0, depth_kind="ray"):
    aabb = torch.tensor(AABB, dtype=F32)
    origin, voxel = tf.box_grid(dims, *AABB)
    c2w, intr = tf.scene_cameras(B, H, W, seed=seed)
    c2w, intr = c2w.float(), intr.float()  # what the reference and the records are both built from
    depth, rgbt, acc = tf.sphere_frames(c2w.double(), intr.double(), H, W, seed=seed, depth_kind=depth_kind)
    return {"dims": dims, "aabb": aabb, "origin": origin, "voxel": voxel, "c2w": c2w, "intr": intr, "depth": depth, "rgbt": rgbt, "acc": acc,
            "records": tf.camera_records(c2w, intr), "truncation": float(voxel[0]) * 5.0}


def _fuse(s, dtype, details=None, max_weight=1.0, **kw):
    return tf.integrate_ref(*tf.fresh_volume(s["dims"]), s["origin"], s["voxel"], s["truncation"], max_weight, s["records"], s["depth"], s["rgbt"],
                            dtype=dtype, details=details, **kw)


def _floor_and_mask(s, **kw):
    """The float64 restatement, the voxels compared (not near a discontinuity) and the float32 restatement's largest errors on them."""
    details = {}
    want = _fuse(s, F64, details, **kw)
    keep = ~details["near"]
    excluded = 1.0 - float(keep.float().mean())
    assert excluded <= MAX_EXCLUDED, excluded
    got = _fuse(s, F32, **kw)
    assert torch.equal(got[1].double()[keep], want[1][keep])  # the float32 restatement takes the same decisions there
    floor = [float((g.double() - w)[keep].abs().max()) for g, w in zip(got, want)]
    return want, keep, floor, excluded


def _reference_volumes(s):
    """The reference's own TSDF over the scene, float32 (tsdf_utils.py, imported unchanged)."""
    ref_import.install_extended_stubs()
    for name in ("pymeshlab", "skimage", "skimage.measure"):
        if name not in sys.modules:
            ref_import._perm_mod(name)
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    from nerfstudio.exporter.tsdf_utils import TSDF

    tsdf = TSDF.from_aabb(s["aabb"], volume_dims=torch.tensor(s["dims"]))
    B = s["c2w"].shape[0]
    c2w = torch.cat([s["c2w"], torch.tensor([[[0.0, 0.0, 0.0, 1.0]]]).expand(B, 1, 4)], dim=1)
    K = torch.zeros((B, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = s["intr"][:, 0], s["intr"][:, 1], s["intr"][:, 2], s["intr"][:, 3], 1.0
    tsdf.integrate_tsdf(c2w, K, s["depth"][:, None], color_images=s["rgbt"][..., :3].permute(0, 3, 1, 2).contiguous())
    return tsdf


@pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not present")
def test_restatement_matches_the_live_reference():
    """The reference in float32 against the float64 restatement: the weights exactly, values and colours within 8 x the float32 restatement's own
    error (the project's convention), outside the voxels that sit on a discontinuity.  Measured here: values 1.3e-6 (floor 7.4e-7), colours 4.5e-8
    (floor 5.2e-8), no decision flipped, 0.12 % of the voxels left out."""
    s = _scene()
    want, keep, floor, _ = _floor_and_mask(s)
    ref = _reference_volumes(s)
    assert torch.equal(ref.voxel_size, s["voxel"]) and abs(ref.truncation - s["truncation"]) == 0.0
    assert torch.equal(ref.weights.double()[keep], want[1][keep])
    assert 0.05 < float(want[1].mean()) < 0.95  # both decisions occur
    err_v = float((ref.values.double() - want[0])[keep].abs().max())
    err_c = float((ref.colors.double() - want[2][..., :3])[keep].abs().max())
    print(f"reference vs float64 restatement: values {err_v:.3g} (floor {floor[0]:.3g}), colours {err_c:.3g} (floor {floor[2]:.3g})")
    assert err_v <= 8 * floor[0] and err_c <= 8 * floor[2]


def _golden():
    z = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(z[k])  # noqa: E731
    dims = tuple(int(v) for v in z["dims"])
    s = {"dims": dims, "origin": t("origin"), "voxel": t("voxel"), "c2w": t("c2w"), "intr": t("intr"), "depth": t("depth"), "rgbt": t("rgbt"),
         "truncation": float(z["truncation"])}
    s["records"] = tf.camera_records(s["c2w"], s["intr"])
    return s, (t("values"), t("weights"), t("colors"))


def test_restatement_reproduces_the_references_recorded_volumes():
    s, (values, weights, colors) = _golden()
    assert values.dtype == F32 and tuple(values.shape) == s["dims"] and colors.shape[-1] == 3 and s["rgbt"].shape[-1] == 4
    want, keep, floor, excluded = _floor_and_mask(s)
    assert torch.equal(weights.double()[keep], want[1][keep])
    assert 0.05 < float(weights.mean()) < 0.95
    err_v = float((values.double() - want[0])[keep].abs().max())
    err_c = float((colors.double() - want[2][..., :3])[keep].abs().max())
    print(f"golden vs float64 restatement: values {err_v:.3g} (floor {floor[0]:.3g}), colours {err_c:.3g} (floor {floor[2]:.3g}), excluded {excluded:.3%}")
    assert err_v <= 8 * floor[0] and err_c <= 8 * floor[2]


def test_restatement_batches_are_bit_equal_and_untouched_voxels_keep_their_bits():
    s = _scene(dims=(13, 11, 9), B=5, H=29, W=37, seed=3)
    guard = (torch.full(s["dims"], -7.25), torch.full(s["dims"], 0.0), torch.full(tuple(s["dims"]) + (4,), 3.5))
    details = {}
    run = lambda vol, sl, d=None: tf.integrate_ref(*vol, s["origin"], s["voxel"], s["truncation"], 4.0, s["records"][sl], s["depth"][sl],  # noqa: E731
                                                   s["rgbt"][sl], dtype=F32, details=d)
    whole = run(guard, slice(0, 5), details)
    parts = guard
    for b0 in (0, 3):
        parts = run(parts, slice(b0, b0 + 3))
    assert all(torch.equal(a, b) for a, b in zip(whole, parts))
    un = ~details["touched"]
    assert 0 < int(un.sum()) < un.numel()
    assert bool((whole[0][un] == -7.25).all()) and bool((whole[2][un] == 3.5).all())


# ---------------------------------------------------------------------------------------------------- 2. the extraction
def _sphere_volume(dims=(33, 31, 29), h=0.0625, radius=0.6, cavity=False):
    """Exact samples of the distance to a sphere, scaled by 1 / truncation and clamped as the volume stores them: negative inside a solid, and
    the negated field for a cavity.  The lattice is shifted off the sphere's centre so that no value is exactly 0."""
    origin = torch.tensor([-h * (d - 1) / 2 for d in dims], dtype=F64) + torch.tensor([0.013, -0.007, 0.021], dtype=F64)
    voxel = torch.full((3,), h, dtype=F64)
    i, j, k = torch.meshgrid(*(torch.arange(d, dtype=F64) for d in dims), indexing="ij")
    p = torch.stack([origin[0] + i * h, origin[1] + j * h, origin[2] + k * h], dim=-1)
    sdf = (p.norm(dim=-1) - radius) / (5 * h)
    values = (-sdf if cavity else sdf).clamp(-1, 1).float()
    g = torch.Generator().manual_seed(5)
    return values, torch.ones(dims), torch.rand(tuple(dims) + (4,), generator=g), origin.float(), voxel.float()


def _mesh_topology(faces):
    """(vertices used, undirected edges, faces, whether every undirected edge has exactly two faces that run it in opposite directions)"""
    f = faces.long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    directed = e[:, 0] * n + e[:, 1]
    undirected = torch.minimum(e[:, 0], e[:, 1]) * n + torch.maximum(e[:, 0], e[:, 1])
    _, counts = torch.unique(undirected, return_counts=True)
    manifold = bool((counts == 2).all()) and torch.unique(directed).numel() == directed.numel()  # each direction once: the two faces oppose
    return torch.unique(f).numel(), counts.numel(), f.shape[0], manifold


def _signed_volume(vertices, faces):
    a, b, c = (vertices.double()[faces.long()[:, n]] for n in range(3))
    return float((a * torch.linalg.cross(b, c)).sum() / 6.0)


@pytest.mark.parametrize("cavity", [False, True])
def test_sphere_mesh_is_a_closed_oriented_surface_within_the_derived_bounds(cavity):
    h, r = 0.0625, 0.6
    values, weights, rgbt, origin, voxel = _sphere_volume(h=h, radius=r, cavity=cavity)
    m = tf.extract_ref(values, weights, rgbt, origin, voxel)
    V, Fn = m["vertices"].shape[0], m["faces"].shape[0]
    used, E, _, manifold = _mesh_topology(m["faces"])
    assert manifold and used == V  # every edge shared by exactly two triangles, consistently oriented; no vertex left over
    assert V - E + Fn == 2
    # every vertex lies on its lattice edge at the linear zero of the two samples
    e = torch.tensor([tf._off(k) for k in tf.KIND_MASK])[m["edge_kind"]]
    i0, i1 = m["edge_point"], m["edge_point"] + e
    a, b = values[i0[:, 0], i0[:, 1], i0[:, 2]].double(), values[i1[:, 0], i1[:, 1], i1[:, 2]].double()
    t = m["t"].double()
    assert bool(((t >= 0) & (t <= 1)).all()) and bool(((a < 0) != (b < 0)).all())
    assert float((a + t * (b - a)).abs().max()) <= 4 * 2.0 ** -24  # |a|, |b| <= 1: a few roundings of t
    on_edge = origin.double() + (i0.double() + t[:, None] * e.double()) * voxel.double()
    assert float((m["vertices"].double() - on_edge).abs().max()) <= 4 * 2.0 ** -24 * 1.2  # coordinates below 1.2
    # Geometry.  The tetrahedra that cross the surface have edges of at most L = sqrt(3) h and lie outside the radius r - L, where the distance
    # field's Hessian is bounded by kappa = 1 / (r - L); they stay inside the unclamped band (L < 5 h).  Along an edge the linear interpolant of
    # the samples misses the field by at most kappa L^2 / 8, so a vertex misses the sphere by that; inside a tetrahedron the interpolant misses
    # it by at most kappa L^2 / 2, so the whole mesh lies between the spheres r -+ delta and its volume between theirs.
    L = math.sqrt(3.0) * h
    kappa = 1.0 / (r - L)
    radius = m["vertices"].double().norm(dim=-1)
    eps = 1e-6
    assert float((radius - r).abs().max()) <= kappa * L * L / 8 + eps
    delta = kappa * L * L / 2
    vol = _signed_volume(m["vertices"], m["faces"])
    sign = -1.0 if cavity else 1.0  # a cavity's mesh faces the enclosed free space: its signed volume is negative
    assert sign * vol > 0
    assert 4 / 3 * math.pi * (r - delta) ** 3 - eps <= sign * vol <= 4 / 3 * math.pi * (r + delta) ** 3 + eps
    # every triangle's own normal points the same way as its vertices' normals: outwards for the solid, inwards for the cavity
    f = m["faces"].long()
    pa, pb, pc = (m["vertices"].double()[f[:, n]] for n in range(3))
    tri_n = torch.linalg.cross(pb - pa, pc - pa)
    centre = (pa + pb + pc) / 3
    assert bool((sign * (tri_n * centre).sum(-1) > 0).all())
    # Normals.  The third derivative of the distance field, applied to three unit vectors u, v, w at distance rho from the centre with n the radial
    # direction, is (3 (n.u)(n.v)(n.w) - (u.v)(n.w) - (u.w)(n.v) - (v.w)(n.u)) / rho^2: at most M3 = 6 / rho^2.  A central difference along an axis
    # misses that component of the gradient by at most h^2 M3 / 6; interpolating a component of the gradient linearly along an edge of length
    # L misses it by at most L^2 M3 / 8; the stencils reach (1 + sqrt 3) h from the vertex, where rho >= r - delta - (1 + sqrt 3) h (inside the
    # unclamped band: 2.8 h < 5 h).  So g misses the unit radial vector by at most sqrt(3) (h^2 / 6 + L^2 / 8) M3, and the angle between the
    # normalised g and the radial direction is at most asin of that.
    reach = (1 + math.sqrt(3.0)) * h
    miss = math.sqrt(3.0) * (h * h / 6 + L * L / 8) * 6 / (r - delta - reach) ** 2
    assert miss < 1
    assert float((m["normals"].norm(dim=-1) - 1).abs().max()) <= 1e-6
    cos = sign * (m["normals"].double() * m["vertices"].double() / radius[:, None]).sum(-1)
    print(f"cavity {cavity}: V {V} F {Fn}, radius error {float((radius - r).abs().max()):.3g} (bound {kappa * L * L / 8:.3g}), volume {sign * vol:.4f} "
          f"(sphere {4 / 3 * math.pi * r ** 3:.4f}), largest normal angle {math.degrees(math.acos(float(cos.min()))):.2f} deg "
          f"(bound {math.degrees(math.asin(miss)):.1f})")
    assert float(cos.min()) >= math.cos(math.asin(miss))
    # attributes: the nearer end of the edge
    near = torch.where((t <= 0.5)[:, None], i0, i1)
    assert torch.equal(m["rgbt"], rgbt[near[:, 0], near[:, 1], near[:, 2]])


def test_uniform_volumes_thin_volumes_and_exact_zeros():
    origin, voxel = torch.zeros(3), torch.full((3,), 0.25)
    for fill in (-1.0, 1.0, -0.3, 0.0):  # all inside, all outside (0 counts as outside): no surface
        m = tf.extract_ref(torch.full((5, 4, 3), fill), torch.ones(5, 4, 3), torch.zeros(5, 4, 3, 4), origin, voxel)
        assert m["vertices"].shape[0] == 0 and m["faces"].shape[0] == 0
    g = torch.Generator().manual_seed(1)
    for dims in ((1, 6, 5), (6, 1, 5), (6, 5, 1), (1, 1, 1)):  # a dimension of 1: no cells, so nothing, whatever the signs
        m = tf.extract_ref(torch.rand(dims, generator=g) - 0.5, torch.ones(dims), torch.zeros(tuple(dims) + (4,)), origin, voxel)
        assert m["vertices"].shape[0] == 0 and m["faces"].shape[0] == 0
    # a plane through lattice points: values exactly 0 on the layer i = 3 (outside), negative before it.  Every crossing edge ends on the layer with
    # t = 1, the vertices coincide there, and the triangles that are not degenerate tile the layer once, facing +x.
    X, Y, Z = 6, 5, 4
    values = ((torch.arange(X, dtype=F32) - 3.0) * 0.25)[:, None, None].expand(X, Y, Z).contiguous()
    m = tf.extract_ref(values, torch.ones(X, Y, Z), torch.zeros(X, Y, Z, 4), origin, voxel)
    assert m["vertices"].shape[0] > 0 and bool(torch.isfinite(m["vertices"]).all()) and bool(torch.isfinite(m["normals"]).all())
    assert bool((m["t"] == 1.0).all()) and bool((m["vertices"][:, 0] == 0.75).all())
    f = m["faces"].long()
    assert int(f.min()) >= 0 and int(f.max()) < m["vertices"].shape[0]
    pa, pb, pc = (m["vertices"].double()[f[:, n]] for n in range(3))
    n = torch.linalg.cross(pb - pa, pc - pa)
    assert bool((n[:, 0] >= 0).all()) and bool((n[:, 1:] == 0).all())
    assert abs(float(n[:, 0].sum()) / 2 - (Y - 1) * (Z - 1) * 0.25 ** 2) < 1e-12
    assert torch.equal(m["normals"], torch.tensor([1.0, 0.0, 0.0]).expand_as(m["normals"]))


def test_observed_only_drops_exactly_the_cells_with_an_unobserved_corner():
    values, _, rgbt, origin, voxel = _sphere_volume(dims=(17, 16, 15), h=0.125)
    g = torch.Generator().manual_seed(2)
    weights = (torch.rand(values.shape, generator=g) > 0.04).float()  # a few unobserved voxels, some of them next to the surface
    full = tf.extract_ref(values, weights, rgbt, origin, voxel, observed_only=False)
    obs = tf.extract_ref(values, weights, rgbt, origin, voxel, observed_only=True)
    cells = tf.cell_mask(weights, True)
    assert 0 < int(cells.sum()) < cells.numel()
    # the triangles of the full mesh, as coordinates, cell by cell: those of the kept cells are the observed-only mesh, in the same order
    tri_full = full["vertices"][full["faces"].long()]  # [F,3,3]
    low = tri_full.double().min(dim=1).values  # the lowest corner of a triangle's bounding box names its cell
    cell = torch.floor((low - origin.double()) / voxel.double() + 1e-9).long()
    cell = torch.minimum(cell, torch.tensor(values.shape) - 2)
    kept = cells[cell[:, 0], cell[:, 1], cell[:, 2]]
    assert 0 < int(kept.sum()) < kept.numel()
    tri_obs = obs["vertices"][obs["faces"].long()]
    assert torch.equal(tri_obs, tri_full[kept])
    assert torch.unique(obs["faces"]).numel() == obs["vertices"].shape[0]  # no vertex without a triangle
    # a vertex takes its attributes from the nearer end of its edge, and from the other where that one was never observed
    e = torch.tensor([tf._off(k) for k in tf.KIND_MASK])[full["edge_kind"]]
    first = (full["t"] <= 0.5)[:, None]
    near, far = torch.where(first, full["edge_point"], full["edge_point"] + e), torch.where(first, full["edge_point"] + e, full["edge_point"])
    at = lambda a, i: a[i[:, 0], i[:, 1], i[:, 2]]  # noqa: E731
    swapped = at(weights, near) == 0
    assert 0 < int(swapped.sum()) < swapped.numel()
    assert torch.equal(full["rgbt"], torch.where(swapped[:, None], at(rgbt, far), at(rgbt, near)))


def test_random_signs_meet_every_case_and_every_edge_kind():
    g = torch.Generator().manual_seed(7)
    values = torch.rand((6, 5, 7), generator=g) * 2 - 1
    m = tf.extract_ref(values, torch.ones(6, 5, 7), torch.zeros(6, 5, 7, 4), torch.zeros(3), torch.ones(3))
    assert m["cases"] == set(range(16)) and set(m["edge_kind"].tolist()) == set(range(7))
    f = m["faces"].long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    assert torch.unique(e[:, 0] * (int(f.max()) + 1) + e[:, 1]).numel() == e.shape[0]  # no directed edge twice: neighbours agree on orientation


# ---------------------------------------------------------------------------------------------------- 3. files
def _cpu_mesh():
    from nerfstudio_thermal_amd.mesh import Mesh

    values, weights, rgbt, origin, voxel = _sphere_volume(dims=(12, 11, 10), h=0.2)
    m = tf.extract_ref(values, weights, rgbt, origin, voxel)
    return Mesh(m["vertices"], m["faces"], m["normals"], m["rgbt"])


@pytest.mark.parametrize("binary", [True, False])
def test_mesh_ply_round_trip(tmp_path, binary):
    from nerfstudio_thermal_amd import mesh as tm
    from nerfstudio_thermal_amd.cloud import to_uint8
    from nerfstudio_thermal_amd.dataparser import load_3D_points, read_ply_thermal

    m = _cpu_mesh()
    path = tm.write_mesh_ply(str(tmp_path / "mesh.ply"), m, binary=binary)
    head = open(path, "rb").read(600).split(b"end_header")[0].decode("ascii").splitlines()
    assert head[1] == f"format {'binary_little_endian' if binary else 'ascii'} 1.0"
    assert head[3:13] == [f"property float {n}" for n in ("x", "y", "z", "nx", "ny", "nz")] + [f"property uchar {n}" for n in ("red", "green", "blue", "thermal")]
    assert head[13:15] == [f"element face {m.faces.shape[0]}", "property list uchar int vertex_indices"]
    xyz, rgb, thermal = read_ply_thermal(path)
    assert np.array_equal(xyz, m.vertices.numpy()) and np.array_equal(rgb, to_uint8(m.colors)) and np.array_equal(thermal, to_uint8(m.thermal))
    assert np.array_equal(tm.read_mesh_ply_faces(path), m.faces.numpy())
    # in the dataset's frame: load_3D_points brings the vertices back to where the model has them
    T = torch.tensor([[0.0, -1.0, 0.0, 0.3], [1.0, 0.0, 0.0, -0.2], [0.0, 0.0, 1.0, 0.1]])
    outputs = types.SimpleNamespace(dataparser_transform=T, dataparser_scale=0.5)
    path = tm.write_mesh_ply(str(tmp_path / "mesh_dataset.ply"), m, binary=binary, dataparser_outputs=outputs)
    back = load_3D_points(path, T, 0.5)
    assert float((back["points3D_xyz"] - m.vertices).abs().max()) <= 1e-5
    moved = tm.mesh_to_dataset_frame(m, outputs)
    assert float((moved.normals @ T[:, :3].T - m.normals).abs().max()) <= 1e-5  # the normals rotate with the vertices
    assert torch.equal(moved.faces, m.faces)  # a rotation keeps the winding
    mirror = types.SimpleNamespace(dataparser_transform=torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0]]), dataparser_scale=1.0)
    assert torch.equal(tm.mesh_to_dataset_frame(m, mirror).faces, m.faces[:, [0, 2, 1]])  # a mirror swaps it


# ---------------------------------------------------------------------------------------------------- 4. the entry points' argument checks
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_entry_points_validate_on_the_host(lib):
    fake = C.c_void_p(256 * 4096)  # a 256-byte aligned, non-NULL address that is never dereferenced
    odd = C.c_void_p(256 * 4096 + 4)
    need = lib.tn_mesh_workspace_bytes(23, 19, 17)
    assert need >= 23 * 19 * 17 * 5
    for bad in ((0, 4, 4), (4, -1, 4), (2048, 2048, 512)):
        assert lib.tn_mesh_workspace_bytes(*bad) == -1, bad

    def integrate(**kw):
        a = dict(values=fake, weights=fake, rgbt=fake, X=4, Y=4, Z=4, o=(0.0, 0.0, 0.0), s=(0.1, 0.1, 0.1), trunc=0.5, maxw=1.0, depth=fake,
                 frgbt=fake, acc=None, mina=0.5, cams=fake, B=2, H=8, W=8, ray=1)
        a.update(kw)
        return lib.tn_tsdf_integrate(a["values"], a["weights"], a["rgbt"], a["X"], a["Y"], a["Z"], *a["o"], *a["s"], a["trunc"], a["maxw"], a["depth"],
                                     a["frgbt"], a["acc"], a["mina"], a["cams"], a["B"], a["H"], a["W"], a["ray"], None)

    for kw, msg in ((dict(X=0), b"voxels"), (dict(X=2048, Y=2048, Z=512), b"voxels"), (dict(B=-1), b"frames"), (dict(H=0), b"frames"),
                    (dict(W=40000), b"frames"), (dict(s=(0.1, 0.0, 0.1)), b"voxel size"), (dict(o=(float("nan"), 0.0, 0.0)), b"origin"),
                    (dict(trunc=0.0), b"truncation"), (dict(maxw=0.0), b"max_weight"), (dict(ray=2), b"ray_depth"), (dict(values=None), b"null pointer"),
                    (dict(cams=None), b"null pointer"), (dict(depth=None), b"null pointer"), (dict(frgbt=odd), b"16-byte"), (dict(rgbt=odd), b"16-byte")):
        assert integrate(**kw) == -22, kw
        assert msg in lib.tn_last_error(), (kw, lib.tn_last_error())
    assert integrate(B=0, values=None, depth=None, cams=None) == 0  # no frames: nothing to do

    def count(**kw):
        a = dict(values=fake, weights=fake, X=23, Y=19, Z=17, obs=0, totals=fake, ws=fake, bytes=need)
        a.update(kw)
        return lib.tn_mesh_count(a["values"], a["weights"], a["X"], a["Y"], a["Z"], a["obs"], a["totals"], a["ws"], a["bytes"], None)

    for kw, msg in ((dict(Z=0), b"points"), (dict(values=None), b"null pointer"), (dict(weights=None), b"null pointer"), (dict(totals=None), b"null pointer"),
                    (dict(ws=None), b"null pointer"), (dict(bytes=need - 1), b"workspace of")):
        assert count(**kw) == -22, kw
        assert msg in lib.tn_last_error(), (kw, lib.tn_last_error())

    def emit(**kw):
        a = dict(values=fake, weights=fake, rgbt=fake, X=23, Y=19, Z=17, obs=0, o=(0.0, 0.0, 0.0), s=(0.1, 0.1, 0.1), vertices=fake, normals=fake,
                 out=fake, V=10, faces=fake, F=10, ws=fake, bytes=need)
        a.update(kw)
        return lib.tn_mesh_emit(a["values"], a["weights"], a["rgbt"], a["X"], a["Y"], a["Z"], a["obs"], *a["o"], *a["s"], a["vertices"], a["normals"],
                                a["out"], a["V"], a["faces"], a["F"], a["ws"], a["bytes"], None)

    for kw, msg in ((dict(Y=0), b"points"), (dict(V=-1), b"vertices"), (dict(V=2 ** 31), b"vertices"), (dict(F=-1), b"faces"), (dict(s=(0.1, 0.1, -1.0)), b"voxel size"),
                    (dict(rgbt=None), b"null pointer"), (dict(vertices=None), b"null pointer"), (dict(faces=None), b"null pointer"),
                    (dict(out=odd), b"16-byte"), (dict(bytes=need - 1), b"workspace of")):
        assert emit(**kw) == -22, kw
        assert msg in lib.tn_last_error(), (kw, lib.tn_last_error())
    assert emit(V=0, F=0, vertices=None, normals=None, out=None, faces=None) == 0  # an empty mesh: nothing to write


def test_volume_and_export_refuse_host_tensors_and_bad_arguments():
    from nerfstudio_thermal_amd import mesh as tm
    from nerfstudio_thermal_amd.splat_camera import PinholeCamera

    with pytest.raises(ValueError, match="volume_dims"):
        tm.TSDFVolume.from_aabb([[-1, -1, -1], [1, 1, 1]], (4, 0, 4), device="cpu")
    with pytest.raises(ValueError, match="positive"):
        tm.TSDFVolume.from_aabb([[-1, -1, -1], [1, 1, 1]], (4, 4, 4), truncation_margin=0.0, device="cpu")
    vol = tm.TSDFVolume.from_aabb([[-1.0, -0.9, -0.8], [1.0, 0.9, 0.8]], (24, 20, 16), device="cpu")
    origin, voxel = tf.box_grid((24, 20, 16))
    assert torch.equal(vol.voxel_size, voxel) and torch.equal(vol.origin, origin) and vol.truncation == float(voxel[0]) * 5.0
    assert vol.colors.shape == (24, 20, 16, 3) and vol.thermal.shape == (24, 20, 16, 1) and vol.colors.data_ptr() == vol.rgbt.data_ptr()
    assert float(vol.values.max()) == -1.0 and not bool(vol.weights.any())
    cam = PinholeCamera(tf.look_at((2.0, 1.0, 0.5)).float(), 60.0, 58.0, 32.5, 23.5, 64, 48)
    rec = tm.camera_records([cam], "cpu")
    assert torch.equal(rec, tf.camera_records(cam.camera_to_world[None], torch.tensor([[60.0, 58.0, 32.5, 23.5]])))
    with pytest.raises(ValueError, match="depth_kind"):
        vol.integrate([cam], torch.zeros(1, 48, 64), torch.zeros(1, 48, 64, 4), depth_kind="disparity")
    with pytest.raises(ValueError, match="no CPU fallback"):
        vol.integrate([cam], torch.zeros(1, 48, 64), torch.zeros(1, 48, 64, 4))
    with pytest.raises(ValueError, match="no CPU fallback"):
        vol.get_mesh()
    with pytest.raises(ValueError, match="Resolution must be"):
        tm.export_tsdf_mesh(None, [cam], resolution="256")
    with pytest.raises(ValueError, match="scene box"):
        tm.export_tsdf_mesh(None, [cam], use_bounding_box=False)
