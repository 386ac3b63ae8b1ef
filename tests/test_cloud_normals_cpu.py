"""The normals of the exported point cloud without a GPU: the host-side argument checks of tn_cloud_estimate_normals, tn_cloud_append_view and
tn_cloud_remove_outliers_view, header and binding, nx ny nz through the PLY writer and readers, the dataparser's points3D_normals,
cloud.normals_to_dataset_frame against load_3D_points, the float64 restatement (cloud_normals_functional.py) on shapes whose normals are known,
the wrappers' refusals and the export script's --help."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_normals_functional as nf
import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib
from nerfstudio_thermal_amd.dataparser import (ThermalNerfDataParserConfig, load_3D_points, read_ply, read_ply_normals, read_ply_thermal,
                                               write_ply)

from test_splat_seed_cpu import _scene

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


# ---- validation happens on the host before the first launch: the pointers only have to be non-null
def test_estimate_normals_arguments_are_refused_before_any_launch(lib):
    fake, n, knn = C.c_void_p(256 * 4096), 1000, 30
    need = lib.tn_cloud_normals_workspace_bytes(n, knn)
    assert need > 0
    for bad in ((n, 2), (n, 33), (29, 30), (2**31, 30), (-1, 30)):
        assert lib.tn_cloud_normals_workspace_bytes(*bad) == -1, bad
    assert lib.tn_cloud_normals_workspace_bytes(3, 3) > 0 and lib.tn_cloud_normals_workspace_bytes(32, 32) > 0
    assert lib.tn_cloud_normals_workspace_bytes(0, 30) == 0

    def call(**kw):
        a = dict(xyz=fake, n=n, knn=knn, view=fake, out=fake, ws=fake, ws_bytes=need)
        a.update(kw)
        return lib.tn_cloud_estimate_normals(a["xyz"], a["n"], a["knn"], a["view"], a["out"], a["ws"], a["ws_bytes"], None)

    for name in ("xyz", "out", "ws"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null pointer" in lib.tn_last_error()
        assert call(view=None, **{name: None}) == EINVAL, name  # view may be null; the others still may not
    for bad_knn in (2, 33, 0, -5):
        assert call(knn=bad_knn) == EINVAL and b"knn" in lib.tn_last_error()
    assert call(n=29) == EINVAL and b"needs at least" in lib.tn_last_error()  # n < knn
    assert call(n=2**31) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and b"workspace of" in lib.tn_last_error()
    assert call(view=None, ws_bytes=need - 1) == EINVAL and b"workspace of" in lib.tn_last_error()
    # n == 0 is TN_OK and touches nothing, whatever else is passed
    assert lib.tn_cloud_estimate_normals(None, 0, 30, None, None, None, 0, None) == 0
    # tn_knn itself keeps refusing k = 9: the wide search belongs to the cloud's two users
    assert lib.tn_knn_workspace_bytes(100, 9) == -1


def test_cloud_append_view_arguments_are_refused_before_any_launch(lib):
    fake, R, cap = C.c_void_p(256 * 4096), 1000, 500
    need = lib.tn_cloud_append_workspace_bytes(R)

    def call(**kw):
        a = dict(origins=fake, directions=fake, depth=fake, accumulation=fake, rgb=fake, rgb_stride=4, thermal=fake, thermal_stride=4, R=R, alpha=0.5,
                 box=None, xyz=fake, out_rgb=fake, out_thermal=fake, out_view=fake, cap=cap, count=fake, ws=fake, ws_bytes=need)
        a.update(kw)
        return lib.tn_cloud_append_view(a["origins"], a["directions"], a["depth"], a["accumulation"], a["rgb"], a["rgb_stride"], a["thermal"],
                                        a["thermal_stride"], a["R"], a["alpha"], a["box"], a["xyz"], a["out_rgb"], a["out_thermal"], a["out_view"],
                                        a["cap"], a["count"], a["ws"], a["ws_bytes"], None)

    for name in ("origins", "directions", "depth", "accumulation", "rgb", "thermal", "xyz", "out_rgb", "out_thermal", "out_view", "count", "ws"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null pointer" in lib.tn_last_error()
    assert call(xyz=None, out_rgb=None, out_thermal=None, out_view=None, cap=0, ws_bytes=need - 1) == EINVAL and b"workspace of" in lib.tn_last_error()
    assert call(R=-1) == EINVAL and call(R=2**31) == EINVAL and call(cap=-1) == EINVAL
    assert call(rgb_stride=2) == EINVAL and call(thermal_stride=0) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and b"workspace of" in lib.tn_last_error()
    assert lib.tn_cloud_append_view(None, None, None, None, None, 3, None, 1, 0, 0.5, None, None, None, None, None, 0, None, None, 0, None) == 0


def test_cloud_remove_outliers_view_arguments_are_refused_before_any_launch(lib):
    fake, n, nb = C.c_void_p(256 * 4096), 1000, 20
    need = lib.tn_cloud_remove_outliers_workspace_bytes(n, nb)

    def call(**kw):
        a = dict(xyz=fake, rgb=fake, thermal=fake, view=fake, n=n, nb=nb, ratio=10.0, out_xyz=fake, out_rgb=fake, out_thermal=fake, out_view=fake,
                 count=fake, stats=fake, mean=None, keep=None, ws=fake, ws_bytes=need)
        a.update(kw)
        return lib.tn_cloud_remove_outliers_view(a["xyz"], a["rgb"], a["thermal"], a["view"], a["n"], a["nb"], a["ratio"], a["out_xyz"], a["out_rgb"],
                                                 a["out_thermal"], a["out_view"], a["count"], a["stats"], a["mean"], a["keep"], a["ws"], a["ws_bytes"],
                                                 None)

    for name in ("xyz", "rgb", "thermal", "view", "out_xyz", "out_rgb", "out_thermal", "out_view", "count", "stats", "ws"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null pointer" in lib.tn_last_error()
    for bad_nb in (1, 33):
        assert call(nb=bad_nb) == EINVAL and b"nb_neighbors" in lib.tn_last_error()
    assert call(n=19) == EINVAL and call(n=2**31) == EINVAL and call(n=-1) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and b"workspace of" in lib.tn_last_error()


def test_header_and_binding_agree_and_the_abi_version_stays(lib):
    hdr = open(os.path.join(ROOT, "include", "thermal_nerf_hip.h"), encoding="utf-8").read()
    assert _lib.ABI_VERSION == 314 and lib.tn_version() == 314
    new = ("tn_cloud_normals_workspace_bytes", "tn_cloud_estimate_normals", "tn_cloud_append_view", "tn_cloud_remove_outliers_view")
    for name in new:
        decl = re.search(r"TN_API\s+\w+\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert decl is not None, name
        res, argtypes = _lib.SIGNATURES[name]
        assert len(decl.group(1).split(",")) == len(argtypes), name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res
    # each _view entry point is its plain form plus the new pointers, at the places the header names
    a, av = _lib.SIGNATURES["tn_cloud_append"][1], _lib.SIGNATURES["tn_cloud_append_view"][1]
    assert av[:14] == a[:14] and av[14] is C.c_void_p and av[15:] == a[14:]
    r, rv = _lib.SIGNATURES["tn_cloud_remove_outliers"][1], _lib.SIGNATURES["tn_cloud_remove_outliers_view"][1]
    assert rv[:3] == r[:3] and rv[3] is C.c_void_p and rv[4:10] == r[3:9] and rv[10] is C.c_void_p and rv[11:] == r[9:]
    assert _lib.SIGNATURES["tn_cloud_estimate_normals"][1] == [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]


# ---- nx ny nz through the PLY
def _cloud(n=57, seed=5):
    g = np.random.default_rng(seed)
    nrm = g.standard_normal((n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    return (g.standard_normal((n, 3)).astype(np.float32), g.integers(0, 256, (n, 3)).astype(np.uint8), g.integers(0, 256, (n, 1)).astype(np.uint8), nrm)


@pytest.mark.parametrize("binary", [True, False])
def test_ply_round_trip_with_normals(tmp_path, binary):
    xyz, rgb, th, nrm = _cloud()
    path = write_ply(str(tmp_path / "c.ply"), xyz, rgb, binary=binary, thermal=th, normals=nrm)
    head = open(path, "rb").read().split(b"end_header")[0].decode()
    props = [ln.split() for ln in head.splitlines() if ln.startswith("property")]
    assert [p[2] for p in props] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "thermal"]
    assert [p[1] for p in props] == ["float"] * 6 + ["uchar"] * 4
    got = read_ply_normals(path)
    assert got.dtype == np.float32 and got.shape == (57, 3) and np.array_equal(got, nrm)
    x, c, t = read_ply_thermal(path)  # the readers keep their tuples, and what they read
    assert np.array_equal(x, xyz) and np.array_equal(c, rgb) and np.array_equal(t, th)
    two = read_ply(path)
    assert isinstance(two, tuple) and len(two) == 2 and np.array_equal(two[0], xyz) and np.array_equal(two[1], rgb)
    # float64 normals are written as float; normals without colours work; a wrong shape or type is refused
    assert open(write_ply(str(tmp_path / "d.ply"), xyz, rgb, binary=binary, thermal=th, normals=nrm.astype(np.float64)), "rb").read() == open(path, "rb").read()
    bare = write_ply(str(tmp_path / "e.ply"), xyz, binary=binary, normals=nrm)
    assert np.array_equal(read_ply_normals(bare), nrm) and read_ply(bare)[1].shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "f.ply"), xyz, rgb, normals=nrm[:-1])
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "f.ply"), xyz, rgb, normals=(nrm * 127).astype(np.int8))


def test_ply_without_normals_reads_none_and_a_partial_set_counts_as_none(tmp_path):
    xyz, rgb, th, _ = _cloud()
    assert read_ply_normals(write_ply(str(tmp_path / "a.ply"), xyz, rgb, thermal=th)) is None
    body = "".join(f"{p[0]} {p[1]} {p[2]} 0.0 1.0\n" for p in xyz[:3].tolist())
    (tmp_path / "p.ply").write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                                    "property float nx\nproperty float ny\nend_header\n" + body)
    assert read_ply_normals(str(tmp_path / "p.ply")) is None


def test_write_ply_with_normals_none_is_byte_identical_to_the_parents(tmp_path, golden_dir):
    """tests/golden/cloud_parent_*.ply: write_ply's files from before the thermal and the normal properties existed (test_cloud_cpu.py's arrays)."""
    g = np.random.default_rng(11)
    xyz, rgb = g.standard_normal((24, 3)).astype(np.float32), g.integers(0, 256, (24, 3)).astype(np.uint8)
    for name, args, kw in (("binary", (xyz, rgb), {"binary": True}), ("ascii", (xyz, rgb), {"binary": False}),
                           ("xyz_only", (xyz.astype(np.float64), None), {"binary": True})):
        want = open(os.path.join(golden_dir, f"cloud_parent_{name}.ply"), "rb").read()
        assert open(write_ply(str(tmp_path / f"{name}.ply"), *args, normals=None, **kw), "rb").read() == want, name
        assert open(write_ply(str(tmp_path / f"{name}_none.ply"), *args, thermal=None, normals=None, **kw), "rb").read() == want, name


# ---- the dataparser and the frames
def test_load_3D_points_adds_the_normals_key_only_for_files_that_have_it(tmp_path):
    d, xyz, rgb = _scene(tmp_path)
    cfg = lambda: ThermalNerfDataParserConfig(data=d, downscale_factor=1, load_3D_points=True)  # noqa: E731
    plain = cfg().setup().get_dataparser_outputs("train")
    assert set(plain.metadata.keys()) == {"is_thermal", "points3D_xyz", "points3D_rgb"}
    g = np.random.default_rng(3)
    nrm = g.standard_normal((xyz.shape[0], 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    write_ply(os.path.join(d, "points.ply"), xyz, rgb, normals=nrm)
    out = cfg().setup().get_dataparser_outputs("train")
    assert set(out.metadata.keys()) == {"is_thermal", "points3D_xyz", "points3D_rgb", "points3D_normals"}
    got = out.metadata["points3D_normals"]
    assert got.dtype == torch.float32 and tuple(got.shape) == (xyz.shape[0], 3)
    assert torch.equal(out.metadata["points3D_xyz"], plain.metadata["points3D_xyz"]) and torch.equal(out.metadata["points3D_rgb"], plain.metadata["points3D_rgb"])
    # rotated, neither scaled nor translated: the float64 product with the linear part of the dataparser's transform, and still of unit length
    T = out.dataparser_transform.double()
    want = torch.from_numpy(nrm).double() @ T[:3, :3].T
    assert float((got.double() - want).abs().max()) <= 8 * 2.0**-24
    assert float((got.double().norm(dim=1) - 1).abs().max()) <= 8 * 2.0**-24
    assert float((T[:3, :3] - torch.eye(3, dtype=torch.float64)).abs().max()) > 1e-3  # the scene's rotation is not the identity (a tilt of 0.2 degrees)
    assert float((got - torch.from_numpy(nrm)).abs().max()) > 1e-3


@pytest.mark.parametrize("extra", [{}, {"applied_transform": [[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, -1, 0]], "applied_scale": 0.5}])
def test_normals_to_dataset_frame_then_load_3D_points_returns_the_normals(tmp_path, extra):
    """Normals in the model's frame, taken to the dataset's frame (float64, rounded once), written beside the points and loaded back by
    load_3D_points (float32: n @ R^T) are the normals again.  The float64 restatement of that round trip is the identity, so the normals
    themselves are the reference.  Error budget per component in units of u = 2^-24, all terms of magnitude at most 1: one rounding of the stored
    value, three products and two sums -- under 8 u, the factor test_cloud_cpu.py's round trip of the points uses."""
    from nerfstudio_thermal_amd import cloud
    from nerfstudio_thermal_amd.dataparser import auto_orient_and_center_poses

    d, _, rgb = _scene(tmp_path, extra)
    o = ThermalNerfDataParserConfig(data=d, downscale_factor=1, load_3D_points=True, scale_factor=1.5).setup().get_dataparser_outputs("train")
    g = torch.Generator().manual_seed(4)
    nrm = torch.nn.functional.normalize(torch.randn((500, 3), generator=g, dtype=torch.float64), dim=-1).float()
    pts = (torch.rand((500, 3), generator=g) * 2 - 1).float()
    q = cloud.normals_to_dataset_frame(nrm, o, extra.get("applied_transform"))
    assert q.dtype == torch.float32 and tuple(q.shape) == (500, 3)
    assert float((q.double().norm(dim=1) - 1).abs().max()) <= 4 * 2.0**-24  # no scale: 1.5 would show here
    write_ply(os.path.join(d, "points.ply"), cloud.to_dataset_frame(pts, o, extra.get("applied_transform")).numpy(), rgb[:500] if rgb.shape[0] >= 500 else None,
              normals=q.numpy())
    meta = json.load(open(os.path.join(d, "transforms.json")))
    poses = torch.from_numpy(np.array([f["transform_matrix"] for f in meta["frames"]]).astype(np.float32))
    _, transform = auto_orient_and_center_poses(poses)
    back = load_3D_points(os.path.join(d, "points.ply"), transform, o.dataparser_scale)["points3D_normals"]
    again = ThermalNerfDataParserConfig(data=d, downscale_factor=1, load_3D_points=True, scale_factor=1.5).setup().get_dataparser_outputs("train")
    assert torch.equal(again.metadata["points3D_normals"], back)  # the dataparser applies exactly this
    err = float((back.double() - nrm.double()).abs().max())
    print(f"normals_to_dataset_frame -> load_3D_points: max error {err:.3e}, bound {8 * 2.0**-24:.3e}")
    assert err <= 8 * 2.0**-24
    assert float((q - nrm).abs().max()) > 1e-3  # without the inverse the normals would turn (the scene's own rotation is a tilt of 0.2 degrees)


# ---- the restatement on shapes whose normals are known
def test_restatement_on_an_exact_plane_and_a_noiseless_sphere():
    g = np.random.default_rng(0)
    plane = np.concatenate([np.round(g.uniform(-1, 1, (400, 2)) * 1024) / 1024, np.full((400, 1), 0.25)], 1)  # dyadic: exact in float32
    r = nf.estimate_normals_ref(torch.from_numpy(plane).float(), 30)
    assert float((r.normals - torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)).abs().max()) <= 1e-12  # +z by the sign rule
    view = torch.tensor([[0.3, -0.2, 1.0]]).repeat(400, 1)
    r = nf.estimate_normals_ref(torch.from_numpy(plane).float(), 30, view)
    assert float((r.normals - torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)).abs().max()) <= 1e-12 and bool((r.vdot < 0).all())
    # a sphere of radius 1: 4000 points, knn 30 -> a neighbourhood of radius h with pi h^2 ~ 30 / 4000 * 4 pi, h^2 = 0.03, h = 0.17.  Over a cap
    # z = -(x^2 + y^2) / 2 the fitted plane tilts by cov(x, z) / var(x), half the sample's third moment over its second: zero for an even
    # sample, about h / 4 times its skewness otherwise.  So the typical normal is within h^2 of radial and every one within h / 2.
    d = g.standard_normal((4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sphere = torch.from_numpy(d).float()
    r = nf.estimate_normals_ref(sphere, 30, view=sphere)  # rays leaving the centre: the normals point inwards
    r_in = nf.estimate_normals_ref(sphere, 30, view=-sphere)  # rays from outside: the normals point outwards
    radial = sphere.double() / sphere.double().norm(dim=1, keepdim=True)
    dev = (r_in.normals - radial).norm(dim=1)
    print(f"sphere: deviation from radial median {float(dev.median()):.4f}, max {float(dev.max()):.4f} (h^2 = 0.03, h / 2 = 0.087)")
    assert float(dev.median()) <= 0.03 and float(dev.max()) <= 0.087 and torch.equal(r.normals, -r_in.normals)
    assert bool((r_in.gap > 0.1).all()) and not bool(r_in.zero.any())
    same = nf.estimate_normals_ref(torch.tensor([[0.1, -0.2, 0.3]]).repeat(40, 1), 30)
    assert bool(same.zero.all()) and bool((same.normals == torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)).all()) and bool((same.gap == 0).all())


# ---- wrappers and script
def test_wrappers_refuse_host_tensors_and_reorient_needs_view():
    from nerfstudio_thermal_amd import cloud

    pc = cloud.PointCloud(torch.zeros(40, 3), torch.zeros(40, 3), torch.zeros(40, 1))  # the three-argument constructor keeps working
    assert pc.view is None and pc.normals is None and pc[:7].view is None and len(pc[:7]) == 7
    with pytest.raises(ValueError, match="needs the cloud's view directions"):
        cloud.estimate_normals(pc)
    with pytest.raises(ValueError, match="no CPU fallback"):
        cloud.estimate_normals(pc, reorient=False)
    with pytest.raises(ValueError, match="3..32"):
        cloud.estimate_normals(pc, knn=33, reorient=False)
    full = cloud.PointCloud(torch.zeros(40, 3), torch.zeros(40, 3), torch.zeros(40, 1), torch.ones(40, 3), torch.ones(40, 3) * 2)
    part = full[3:9]
    assert torch.equal(part.view, torch.ones(6, 3)) and torch.equal(part.normals, torch.ones(6, 3) * 2)  # __getitem__ carries both
    with pytest.raises(ValueError, match="no CPU fallback"):
        cloud.estimate_normals(full)
    with pytest.raises(ValueError, match="no CPU fallback"):
        cloud.remove_outliers(full)
    e = cloud.PointCloud.empty(5, "cpu", with_view=True)
    assert tuple(e.view.shape) == (5, 3) and e.normals is None and cloud.PointCloud.empty(5, "cpu").view is None


def test_export_script_help_names_the_normal_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "export_point_cloud.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--normal-method" in r.stdout and "--normals-knn" in r.stdout and "--no-reorient-normals" in r.stdout
