"""The mesh simplification without a GPU: the float64 restatement (mesh_simplify_functional.py, what the kernels are compared with on the GPU) against
geometry on the sphere mesh of test_tsdf_mesh_cpu.py -- topology, the quadric placement against the plain mean, the invariants of the clustering, the
face-budget search -- and on hand meshes; the host-side argument checks of the entry points; the script's new options; the PLY round trip."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import mesh_simplify_functional as sf
import tsdf_functional as tf
from nerfstudio_thermal_amd import _lib
from test_tsdf_mesh_cpu import _mesh_topology, _sphere_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, R = 0.0625, 0.6
GRID_OFFSET = 0.37  # the cell borders lie this share of a cell above the lattice planes: off the planes the marching-tetrahedra vertices sit on

_SPHERE = {}


def _sphere():
    """The sphere mesh of test_tsdf_mesh_cpu.py (exact distances, 33 x 31 x 29, h = 0.0625, r = 0.6: 5186 vertices, 10368 faces), built once."""
    if not _SPHERE:
        values, weights, rgbt, origin, voxel = _sphere_volume(h=H, radius=R)
        m = tf.extract_ref(values, weights, rgbt, origin, voxel)
        _SPHERE.update(mesh={k: m[k].numpy() for k in ("vertices", "faces", "normals", "rgbt")}, origin=origin.numpy(), voxel=voxel.numpy())
        assert m["vertices"].shape[0] == 5186 and m["faces"].shape[0] == 10368
    return _SPHERE


def _simplified(scale):
    """The sphere at a cell of `scale` voxels on the offset grid -> (input mesh, output, details, origin, cell, dims), computed once per scale."""
    s = _sphere()
    if scale not in s:
        cell = np.full(3, scale * H, dtype=np.float32)
        origin = s["origin"] - np.float32(1.0 - GRID_OFFSET) * cell
        _, dims = sf.grid_ref(sf.extent_of(s["mesh"]["vertices"]), cell, origin)
        details = {}
        m = s["mesh"]
        out = sf.simplify_ref(m["vertices"], m["faces"], m["normals"], m["rgbt"], origin, cell, dims, details=details)
        s[scale] = (m, out, details, origin, cell, dims)
    return s[scale]


def _edge_share(faces):
    """the share of the undirected edges that lie in exactly two faces"""
    f = torch.from_numpy(faces).long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1
    _, counts = torch.unique(torch.minimum(e[:, 0], e[:, 1]) * n + torch.maximum(e[:, 0], e[:, 1]), return_counts=True)
    return float((counts == 2).float().mean())


# ---------------------------------------------------------------------------------------------------- 1. the sphere
def test_sphere_at_one_voxel_is_a_closed_oriented_manifold():
    m, out, details, *_ = _simplified(1.0)
    V, Fn = out["vertices"].shape[0], out["faces"].shape[0]
    used, E, _, manifold = _mesh_topology(torch.from_numpy(out["faces"]))
    print(f"cell 1 voxel: {m['faces'].shape[0]} -> {Fn} faces, {m['vertices'].shape[0]} -> {V} vertices, chi {V - E + Fn}")
    assert manifold and used == V and V - E + Fn == 2
    assert Fn < 0.3 * m["faces"].shape[0]  # the prototype: 73 % of the faces go
    # and it is still the sphere, facing outwards
    a, b, c = (out["vertices"][out["faces"][:, k]] for k in range(3))
    assert bool(((np.cross(b - a, c - a) * (a + b + c)).sum(-1) > 0).all())
    assert bool(((out["normals"] * out["vertices"]).sum(-1) > 0).all())
    assert float(np.abs(np.linalg.norm(out["normals"], axis=1) - 1).max()) <= 1e-12


@pytest.mark.parametrize("scale", [1.0, 2.0, 3.5])
def test_quadric_placement_is_no_worse_than_the_mean_and_the_invariants_hold(scale):
    m, out, details, origin, cell, dims = _simplified(scale)
    V, Fn = out["vertices"].shape[0], out["faces"].shape[0]
    radius_q = float(np.abs(np.linalg.norm(out["vertices"], axis=1) - R).max())
    radius_m = float(np.abs(np.linalg.norm(details["mean"], axis=1) - R).max())
    used, E, _, _ = _mesh_topology(torch.from_numpy(out["faces"]))
    print(f"cell {scale} voxels: faces {Fn}, vertices {V}, chi {used - E + Fn}, edges in two faces {_edge_share(out['faces']):.1%}, largest radius error "
          f"quadric {radius_q:.4f} / mean {radius_m:.4f}, quadric point taken {float(details['solved'].mean()):.1%}, near the decision "
          f"{int(details['near'].sum())}, count {details['count']}")
    assert radius_q <= radius_m
    assert used - E + Fn == 2
    assert details["count"] >= Fn and details["count"] == sf.count_ref(m["vertices"], m["faces"], origin, cell, dims)
    # every emitted vertex lies in its own closed cell: to the rule's margin of 1e-6 cell for a solved point, and for a mean to the rounding of the
    # float32 key expression, a few ulps of the coordinates, which are below 2
    assert float((np.abs(out["vertices"] - details["centre"]) - 0.5 * cell.astype(np.float64)).max()) <= 1e-6 * float(cell.max()) + 4 * 2.0 ** -23
    key, _ = sf.cell_keys(out["vertices"].astype(np.float32), origin, cell, dims)
    own = (details["cell"][:, 0] * dims[1] + details["cell"][:, 1]) * dims[2] + details["cell"][:, 2]
    assert float((key == own).mean()) >= 0.99 and bool((np.diff(own) > 0).all())  # (a point on a border may round across it); key order
    # RGB+T within the range of the cluster's inputs
    for row, members in enumerate(details["members"]):
        src = m["rgbt"][members].astype(np.float64)
        assert bool((out["rgbt"][row] >= src.min(axis=0) - 1e-15).all()) and bool((out["rgbt"][row] <= src.max(axis=0) + 1e-15).all())
    f = out["faces"]
    assert bool((f[:, 0] != f[:, 1]).all()) and bool((f[:, 1] != f[:, 2]).all()) and bool((f[:, 0] != f[:, 2]).all())  # no repeated index
    assert np.unique(np.sort(f, axis=1), axis=0).shape[0] == Fn  # no two faces share a vertex set
    assert np.unique(f).shape[0] == V and int(f.min()) == 0 and int(f.max()) == V - 1  # every vertex is referenced
    assert bool((np.diff(details["kept"]) > 0).all()) and details["kept"].shape[0] == Fn  # input order
    # a surviving face is its input face with the indices remapped, corner by corner
    assert np.array_equal(details["cluster_of"][m["faces"][details["kept"]]], f)


@pytest.mark.parametrize("target,prototype", [(500, 496), (2000, 1965), (5000, 4960)])
def test_search_stays_within_the_target(target, prototype):
    s = _sphere()
    m = s["mesh"]
    origin = s["origin"] - np.float32(0.5) * s["voxel"]  # cells centred on lattice points, as export_tsdf_mesh places them
    scale, cell, o, dims = sf.search_ref(m["vertices"], m["faces"], target, s["voxel"], origin=origin)
    out = sf.simplify_ref(m["vertices"], m["faces"], m["normals"], m["rgbt"], o, cell, dims)
    count = sf.count_ref(m["vertices"], m["faces"], o, cell, dims)
    print(f"target {target}: s = {scale:.4f} voxels, count {count}, faces {out['faces'].shape[0]} (the prototype: {prototype})")
    assert out["faces"].shape[0] <= count <= target
    assert out["faces"].shape[0] >= 0.9 * target  # the bisection ends close under the budget
    assert 0.25 <= scale <= 4.0 and np.array_equal(cell, (np.float64(scale) * s["voxel"].astype(np.float64)).astype(np.float32))
    again = sf.search_ref(m["vertices"], m["faces"], target, s["voxel"], origin=origin)
    assert again[0] == scale and again[3] == dims  # deterministic


def test_search_leaves_a_mesh_within_the_target_alone():
    m = _sphere()["mesh"]
    assert sf.search_ref(m["vertices"], m["faces"], 20000, _sphere()["voxel"]) is None
    assert sf.search_ref(m["vertices"], m["faces"], 10368, _sphere()["voxel"]) is None
    assert sf.search_ref(m["vertices"], m["faces"], 10367, _sphere()["voxel"]) is not None


# ---------------------------------------------------------------------------------------------------- 2. hand meshes
OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32) * np.float32(0.7)
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)


def _attributes(V, seed=0):
    g = np.random.default_rng(seed)
    n = g.normal(size=(V, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32), g.uniform(size=(V, 4)).astype(np.float32)


def test_octahedron_with_a_cell_per_vertex_comes_back():
    normals, rgbt = _attributes(6)
    origin, cell, dims = np.full(3, -1.05, dtype=np.float32), np.full(3, 0.7, dtype=np.float32), (3, 3, 3)
    key, _ = sf.cell_keys(OCTA_V, origin, cell, dims)
    assert np.unique(key).shape[0] == 6
    details = {}
    out = sf.simplify_ref(OCTA_V, OCTA_F, normals, rgbt, origin, cell, dims, details=details)
    order = np.argsort(key)  # output vertex k is input vertex order[k]
    assert np.array_equal(order[out["faces"]], OCTA_F)
    # the planes of a vertex's four faces meet in the vertex: the quadric puts it back, to the rounding of the solve
    assert bool(details["solved"].all())
    # (one float32 ulp at the vertex's size, 0.7: its zero coordinates come back as the solve's rounding of a cell, some 1e-17, not as zeros)
    assert bool((np.abs(out["vertices"] - OCTA_V[order]) <= sf.ulp32(np.abs(OCTA_V[order]).max(axis=1, keepdims=True))).all())
    assert np.array_equal(out["rgbt"], rgbt[order].astype(np.float64))
    assert float(np.abs(out["normals"] - normals[order]).max()) <= 1e-7


def test_a_mesh_inside_one_cell_and_empty_meshes_give_nothing():
    normals, rgbt = _attributes(6)
    grid = (np.full(3, -1.0, dtype=np.float32), np.full(3, 2.0, dtype=np.float32), (1, 1, 1))
    details = {}
    out = sf.simplify_ref(OCTA_V, OCTA_F, normals, rgbt, *grid, details=details)
    assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3) and out["rgbt"].shape == (0, 4) and details["clusters"] == 1
    assert sf.count_ref(OCTA_V, OCTA_F, *grid) == 0
    none = np.zeros((0, 3), dtype=np.int32)
    out = sf.simplify_ref(OCTA_V, none, normals, rgbt, np.full(3, -1.05, dtype=np.float32), np.full(3, 0.7, dtype=np.float32), (3, 3, 3))  # F = 0
    assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3)
    out = sf.simplify_ref(np.zeros((0, 3), np.float32), none, np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32), *grid)  # V = 0
    assert out["vertices"].shape == (0, 3) and out["faces"].shape == (0, 3)
    assert sf.count_ref(np.zeros((0, 3), np.float32), none, *grid) == 0


def test_repeated_indices_and_duplicated_faces_keep_the_expected_survivors():
    # eight vertices: 0/1 share a cell, the others have a cell each (cells of 1 along x)
    x = np.array([0.2, 0.7, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5], dtype=np.float32)
    vertices = np.stack([x, np.array([0.1, 0.2, 0.9, 0.1, 0.8, 0.3, 0.6, 0.2], dtype=np.float32), np.array([0.3, 0.1, 0.2, 0.7, 0.5, 0.9, 0.4, 0.6], dtype=np.float32)], axis=1)
    faces = np.array([[2, 3, 4],   # 0: survives
                      [0, 1, 2],   # 1: two corners in one cluster
                      [3, 4, 2],   # 2: a rotation of 0
                      [4, 3, 2],   # 3: a reflection of 0
                      [3, 3, 5],   # 4: a repeated index
                      [1, 2, 3],   # 5: survives, as clusters (0, 1, 2)
                      [0, 3, 2],   # 6: the same clusters as 5, reflected, through the other vertex of cluster 0
                      [5, 6, 7],   # 7: survives
                      [7, 6, 5],   # 8: a reflection of 7
                      [4, 5, 9]],  # 9: an index out of range
                     dtype=np.int32)
    normals, rgbt = _attributes(8, seed=1)
    details = {}
    out = sf.simplify_ref(vertices, faces, normals, rgbt, np.zeros(3, np.float32), np.ones(3, np.float32), (7, 1, 1), details=details)
    assert details["clusters"] == 7 and details["kept"].tolist() == [0, 5, 7] and details["count"] == 7
    assert out["faces"].tolist() == [[1, 2, 3], [0, 1, 2], [4, 5, 6]]  # all seven clusters are referenced: cluster k is vertex k
    assert out["vertices"].shape[0] == 7
    assert sf.count_ref(vertices, faces, np.zeros(3, np.float32), np.ones(3, np.float32), (7, 1, 1)) == 7
    assert np.allclose(out["rgbt"][0], rgbt[:2].astype(np.float64).mean(axis=0), rtol=0, atol=1e-16)  # the merged vertex: the mean of its two


def test_a_shell_on_the_cell_borders_is_not_decided_by_the_last_bit():
    """A volume's shell between observed free space (+1) and the unobserved fill (-1) crosses every lattice edge at t = 0.5: on the borders of the
    lattice-centred grid export_tsdf_mesh uses.  The solved points lie on those borders too; the rule's margin keeps them, and none is near its decision."""
    X, Y, Z = 7, 6, 5
    values = torch.where(torch.arange(X) <= 2, 1.0, -1.0)[:, None, None].expand(X, Y, Z).contiguous()
    origin, voxel = torch.tensor([-0.25, 0.125, 0.25]), torch.tensor([0.125, 0.25, 0.5])  # exact in float32: the vertices sit at x = 0.0625 exactly
    m = tf.extract_ref(values, torch.ones(X, Y, Z), torch.rand((X, Y, Z, 4), generator=torch.Generator().manual_seed(3)), origin, voxel)
    assert m["vertices"].shape[0] > 0 and bool((m["t"] == 0.5).all()) and bool((m["vertices"][:, 0] == 0.0625).all())
    cell = voxel.numpy()
    grid_origin = (origin - voxel * 0.5).numpy()
    _, dims = sf.grid_ref(sf.extent_of(m["vertices"]), cell, grid_origin)
    details = {}
    out = sf.simplify_ref(m["vertices"], m["faces"], m["normals"], m["rgbt"], grid_origin, cell, dims, details=details)
    assert out["faces"].shape[0] > 0 and not bool(details["near"].any()) and bool(details["solved"].all())
    assert float(np.abs(out["vertices"][:, 0] - 0.0625).max()) <= 1e-15  # on the plane


def test_keys_clamp_to_the_grid_and_take_a_nan_to_zero():
    v = np.array([[-5.0, 0.5, 0.5], [0.5, 99.0, 0.5], [2.999999, 1.0, np.nan], [3.0, 0.0, 1e30]], dtype=np.float32)
    key, idx = sf.cell_keys(v, np.zeros(3, np.float32), np.ones(3, np.float32), (3, 2, 4))
    assert idx.tolist() == [[0, 0, 0], [0, 1, 0], [2, 1, 0], [2, 0, 3]] and key.tolist() == [0, 4, 20, 19]


# ---------------------------------------------------------------------------------------------------- 3. the entry points' argument checks
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_entry_points_validate_on_the_host(lib):
    fake = C.c_void_p(256 * 4096)  # a 256-byte aligned, non-NULL address that is never dereferenced
    odd = C.c_void_p(256 * 4096 + 4)
    V, Fn = 1000, 2000
    need = lib.tn_mesh_simplify_workspace_bytes(V, Fn)
    assert need >= 32 * V + 76 * Fn
    assert lib.tn_mesh_simplify_workspace_bytes(0, 0) > 0
    for bad in ((-1, 10), (10, -1), (2 ** 31, 10), (10, 2 ** 31), (10, (2 ** 31 - 1) // 3 + 1)):
        assert lib.tn_mesh_simplify_workspace_bytes(*bad) == -1, bad

    def grid_args(a):
        return [a["vertices"], a["V"], a["faces"], a["F"], *a["o"], *a["c"], *a["dims"]]

    base = dict(vertices=fake, V=V, faces=fake, F=Fn, o=(0.0, 0.0, 0.0), c=(0.1, 0.1, 0.1), dims=(17, 13, 11), out=fake, ws=fake, bytes=need)
    common = ((dict(V=-1), b"vertices"), (dict(V=2 ** 31), b"vertices"), (dict(F=2 ** 31), b"faces"), (dict(dims=(0, 4, 4)), b"cells"),
              (dict(dims=(2048, 2048, 512)), b"cells"), (dict(c=(0.1, 0.0, 0.1)), b"cell size"), (dict(c=(0.1, 0.1, -1.0)), b"cell size"),
              (dict(c=(float("inf"), 0.1, 0.1)), b"cell size"), (dict(o=(float("nan"), 0.0, 0.0)), b"origin"), (dict(vertices=None), b"null pointer"),
              (dict(faces=None), b"null pointer"), (dict(ws=None), b"null pointer"), (dict(ws=odd), b"misaligned"), (dict(out=None), b"null"),
              (dict(bytes=need - 1), b"workspace of"))

    def count(**kw):
        a = dict(base, **kw)
        return lib.tn_mesh_simplify_count(*grid_args(a), a["out"], a["ws"], a["bytes"], None)

    def plan(**kw):
        a = dict(base, **kw)
        return lib.tn_mesh_simplify_plan(*grid_args(a), a["out"], a["ws"], a["bytes"], None)

    for call in (count, plan):
        for kw, msg in common:
            assert call(**kw) == -22, kw
            assert msg in lib.tn_last_error(), (kw, lib.tn_last_error())

    def emit(**kw):
        a = dict(base, normals=fake, rgbt=fake, reg=1e-3, ov=fake, on=fake, oc=fake, Vo=10, of=fake, Fo=10)
        a.update(kw)
        return lib.tn_mesh_simplify_emit(a["vertices"], a["normals"], a["rgbt"], a["V"], a["faces"], a["F"], *a["o"], *a["c"], *a["dims"], a["reg"], a["ov"],
                                         a["on"], a["oc"], a["Vo"], a["of"], a["Fo"], a["ws"], a["bytes"], None)

    for kw, msg in tuple(c for c in common if "out" not in c[0]) + (
            (dict(reg=-1.0), b"regularization"), (dict(reg=float("nan")), b"regularization"), (dict(Vo=-1), b"vertices"), (dict(Vo=V + 1), b"vertices"),
            (dict(Fo=Fn + 1), b"faces"), (dict(normals=None), b"null pointer"), (dict(rgbt=None), b"null pointer"), (dict(ov=None), b"null pointer"),
            (dict(oc=None), b"null pointer"), (dict(of=None), b"null pointer"), (dict(rgbt=odd), b"16-byte"), (dict(oc=odd), b"16-byte")):
        assert emit(**kw) == -22, kw
        assert msg in lib.tn_last_error(), (kw, lib.tn_last_error())
    assert emit(Vo=0, Fo=0, ov=None, on=None, oc=None, of=None) == 0  # an empty result: nothing to write


def test_python_layer_refuses_host_tensors_and_bad_arguments():
    from nerfstudio_thermal_amd import mesh as tm

    m = tm.Mesh(torch.from_numpy(OCTA_V), torch.from_numpy(OCTA_F), torch.zeros(6, 3), torch.zeros(6, 4))
    with pytest.raises(ValueError, match="no CPU fallback"):
        tm.simplify_mesh(m, 0.7)
    with pytest.raises(ValueError, match="no CPU fallback"):
        tm.simplify_to_target(m, 4, 0.1)
    with pytest.raises(ValueError, match="positive"):
        tm.simplify_mesh(m, 0.0)
    with pytest.raises(ValueError, match="positive"):
        tm.simplify_to_target(m, 4, (0.1, -0.1, 0.1))
    with pytest.raises(ValueError, match="target_num_faces"):
        tm.simplify_to_target(m, -1, 0.1)
    with pytest.raises(ValueError, match="too small for the mesh"):
        tm.simplify_mesh(m, 1e-4, origin=(-1.0, -1.0, -1.0))
    same, cell = tm.simplify_to_target(m, 8, 0.1)  # within the target: handed back as it is, before anything touches the device
    assert same is m and cell is None
    # the grid of the Python layer is the restatement's
    for cell in (0.7, (0.3, 0.11, 0.25)):
        c = tm._triple(cell, "cell")
        o, dims = tm.simplify_grid(tm.vertex_extent(m.vertices), c)
        ro, rdims = sf.grid_ref(sf.extent_of(OCTA_V), c)
        assert np.array_equal(o, ro) and dims == rdims
        key, idx = sf.cell_keys(OCTA_V, o, c, dims)
        assert idx.max(axis=0).tolist() == [d - 1 for d in dims] and idx.min() == 0
    assert np.array_equal(tm.search_cell(1.1894083760644074, np.full(3, 0.0625, np.float32)),
                          (np.float64(1.1894083760644074) * np.full(3, 0.0625)).astype(np.float32))
    vol = tm.TSDFVolume.from_aabb([[-1.0, -0.9, -0.8], [1.0, 0.9, 0.8]], (24, 20, 16), device="cpu")
    assert np.array_equal(tm.lattice_centred_origin(vol), (vol.origin - vol.voxel_size / 2).numpy())


# ---------------------------------------------------------------------------------------------------- 4. the script and the file
def test_script_accepts_the_new_options():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import export_tsdf_mesh as script

    args = script.parse_args([])
    assert args.target_num_faces is None and args.simplify_cell is None  # the defaults change nothing
    args = script.parse_args(["--model", "splat", "--target-num-faces", "50000"])
    assert args.target_num_faces == 50000 and args.simplify_cell is None
    assert script.parse_args(["--simplify-cell", "2.5"]).simplify_cell == 2.5
    for bad in (["--target-num-faces", "-1"], ["--simplify-cell", "0"], ["--target-num-faces", "10", "--simplify-cell", "2"]):
        with pytest.raises(SystemExit):
            script.parse_args(bad)
    assert "50 000" in script.__doc__


@pytest.mark.parametrize("binary", [True, False])
def test_simplified_mesh_round_trips_through_the_ply(tmp_path, binary):
    from nerfstudio_thermal_amd import mesh as tm
    from nerfstudio_thermal_amd.cloud import to_uint8
    from nerfstudio_thermal_amd.dataparser import read_ply_thermal

    _, out, *_ = _simplified(2.0)
    m = tm.Mesh(torch.from_numpy(out["vertices"].astype(np.float32)), torch.from_numpy(out["faces"]), torch.from_numpy(out["normals"].astype(np.float32)),
                torch.from_numpy(out["rgbt"].astype(np.float32)))
    path = tm.write_mesh_ply(str(tmp_path / "simplified.ply"), m, binary=binary)
    xyz, rgb, thermal = read_ply_thermal(path)
    assert np.array_equal(xyz, m.vertices.numpy()) and np.array_equal(rgb, to_uint8(m.colors)) and np.array_equal(thermal, to_uint8(m.thermal))
    assert np.array_equal(tm.read_mesh_ply_faces(path), m.faces.numpy())
