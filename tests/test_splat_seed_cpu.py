"""Seeding thermal splats without a GPU: the kNN restatement (knn_functional.py) against scikit-learn, the PLY reader / writer, the dataparser's
load_3D_points, and the host-side argument checks of tn_knn."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib
from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig, read_ply, write_ply

import knn_functional as kf

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


# ---- the restatement against scikit-learn (k_nearest_sklearn, splatfacto.py:272-290)
@pytest.mark.parametrize("kind", ["uniform", "plane", "duplicates", "lattice", "clusters", "surface"])
def test_restatement_matches_sklearn(kind):
    sk = pytest.importorskip("sklearn.neighbors")
    p = kf.cloud(kind, 1500, seed=4)
    k = 3
    d32, i32 = kf.knn_brute(p, k)
    d64, i64 = kf.knn_brute(p, k, dtype=torch.float64)
    dist, idx = sk.NearestNeighbors(n_neighbors=k + 1, algorithm="auto", metric="euclidean").fit(p.numpy()).kneighbors(p.numpy())
    ref = dist[:, 1:]  # the reference drops column 0, the point itself
    # sorted distances agree within a few fp32 ulps (sklearn computes in float64 from the float32 coordinates)
    tol = 4 * np.spacing(ref.astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(d32.numpy().astype(np.float64) - ref) <= tol)
    assert np.abs(d64.numpy() - ref).max() <= 1e-9 * max(1.0, float(ref.max()))
    # drop-self: column 0 of sklearn is the point or one of its duplicates at distance 0; no row of the restatement names itself
    assert np.all(dist[:, 0] == 0.0)
    rows = torch.arange(p.shape[0])[:, None]
    assert not bool((i32 == rows).any()) and not bool((i64 == rows).any())
    if kind == "duplicates":  # a duplicate of the point is a neighbour at distance 0
        assert int((d32[:, 0] == 0).sum()) > p.shape[0] // 2


def test_restatement_tie_rule_and_drop_self():
    p = torch.tensor([[0.0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 0], [5, 5, 5]])
    d, i = kf.knn_brute(p, 3)
    # point 0: its duplicate 4 first (distance 0), then the three unit neighbours 1, 2, 3 tie: the smaller indices win
    assert i[0].tolist() == [4, 1, 2] and d[0].tolist() == [0.0, 1.0, 1.0]
    assert i[4].tolist() == [0, 1, 2]
    d1, i1 = kf.knn_brute(p, 1)
    assert torch.equal(d1, d[:, :1]) and torch.equal(i1, i[:, :1])
    rows = torch.tensor([5, 0])
    dr, ir = kf.knn_brute(p, 3, rows=rows)
    assert torch.equal(dr, d[rows]) and torch.equal(ir, i[rows])


# ---- PLY
def _header(fmt, props, count, extra=""):
    return ("ply\nformat %s 1.0\ncomment made by a test\nelement vertex %d\n" % (fmt, count) + "".join(f"property {t} {n}\n" for t, n in props)
            + extra + "end_header\n").encode()


@pytest.mark.parametrize("binary", [True, False])
def test_ply_round_trip_uchar_colours_all_values(tmp_path, binary):
    n = 256
    xyz = np.random.default_rng(0).standard_normal((n, 3)).astype(np.float32)
    rgb = np.stack([np.arange(256), np.arange(256)[::-1], (np.arange(256) * 7) % 256], 1).astype(np.uint8)
    path = write_ply(str(tmp_path / "c.ply"), xyz, rgb, binary=binary)
    x, c = read_ply(path)
    assert x.dtype == np.float32 and c.dtype == np.uint8
    assert np.array_equal(x, xyz) and np.array_equal(c, rgb)


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("cdtype", [np.float32, np.float64])
def test_ply_float_colours_and_double_xyz(tmp_path, binary, cdtype):
    g = np.random.default_rng(1)
    xyz = g.standard_normal((100, 3))  # float64 -> double properties
    rgb = g.uniform(0, 1, (100, 3)).astype(cdtype)
    rgb[0] = [0.0, 1.0, 0.5]
    x, c = read_ply(write_ply(str(tmp_path / "f.ply"), xyz, rgb, binary=binary))
    assert np.array_equal(x, xyz.astype(np.float32))  # open3d reads doubles, nerfstudio casts to float32
    assert np.array_equal(c, (rgb.astype(np.float64) * 255).astype(np.uint8))
    assert c[0].tolist() == [0, 255, 127]


@pytest.mark.parametrize("binary", [True, False])
def test_ply_without_colours(tmp_path, binary):
    xyz = np.arange(30, dtype=np.float32).reshape(10, 3)
    x, c = read_ply(write_ply(str(tmp_path / "n.ply"), xyz, binary=binary))
    assert np.array_equal(x, xyz) and c.shape == (0, 3) and c.dtype == np.uint8


def test_ply_extra_properties_and_trailing_faces_are_ignored(tmp_path):
    props = [("float", "x"), ("float", "nx"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue"),
             ("uchar", "alpha"), ("double", "quality")]
    faces = "element face 2\nproperty list uchar int vertex_indices\n"
    rows = [(1.5, 9.0, -2.0, 0.25, 10, 20, 30, 255, 0.5), (3.0, 8.0, 4.0, -1.0, 40, 50, 60, 128, 1.5), (0.0, 7.0, 0.0, 0.0, 70, 80, 90, 0, 2.5)]
    # binary: vertices, then two faces (lists)
    rec = np.array(rows, dtype=[("x", "<f4"), ("nx", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                                ("alpha", "u1"), ("quality", "<f8")])
    face = np.array([3], np.uint8).tobytes() + np.array([0, 1, 2], "<i4").tobytes()
    b = tmp_path / "b.ply"
    b.write_bytes(_header("binary_little_endian", props, 3, faces) + rec.tobytes() + face * 2)
    a = tmp_path / "a.ply"
    a.write_bytes(_header("ascii", props, 3, faces) + "".join(" ".join(str(v) for v in r) + "\n" for r in rows).encode() + b"3 0 1 2\n3 0 1 2\n")
    for p in (a, b):
        x, c = read_ply(str(p))
        assert np.array_equal(x, np.array([[1.5, -2.0, 0.25], [3.0, 4.0, -1.0], [0.0, 0.0, 0.0]], np.float32))
        assert c.tolist() == [[10, 20, 30], [40, 50, 60], [70, 80, 90]]


def test_ply_fixed_element_before_the_vertices_is_skipped(tmp_path):
    head = b"ply\nformat binary_little_endian 1.0\nelement camera 2\nproperty float f\nproperty uchar u\nelement vertex 2\nproperty float x\n"
    head += b"property float y\nproperty float z\nend_header\n"
    cam = np.array([(1.0, 2), (3.0, 4)], dtype=[("f", "<f4"), ("u", "u1")]).tobytes()
    p = tmp_path / "s.ply"
    p.write_bytes(head + cam + np.arange(6, dtype="<f4").tobytes())
    x, c = read_ply(str(p))
    assert x.tolist() == [[0, 1, 2], [3, 4, 5]] and c.shape == (0, 3)


def test_malformed_ply_raises(tmp_path):
    good = write_ply(str(tmp_path / "g.ply"), np.zeros((4, 3), np.float32), np.zeros((4, 3), np.uint8))
    data = open(good, "rb").read()
    cases = {
        "big_endian": data.replace(b"binary_little_endian", b"binary_big_endian"),
        "no_z": _header("ascii", [("float", "x"), ("float", "y")], 1) + b"1 2\n",
        "list_before": b"ply\nformat ascii 1.0\nelement face 1\nproperty list uchar int vertex_indices\nelement vertex 1\nproperty float x\n"
                       b"property float y\nproperty float z\nend_header\n3 0 0 0\n1 2 3\n",
        "truncated_binary": data[:-5],
        "truncated_ascii": _header("ascii", [("float", "x"), ("float", "y"), ("float", "z")], 3) + b"1 2 3\n4 5 6\n",
        "not_ply": b"obj\n",
    }
    for name, raw in cases.items():
        p = tmp_path / f"{name}.ply"
        p.write_bytes(raw)
        with pytest.raises(ValueError):
            read_ply(str(p))
    with pytest.raises(ValueError, match="big-endian"):
        read_ply(str(tmp_path / "big_endian.ply"))


# ---- the dataparser's load_3D_points (nerfstudio_dataparser.py:352-466)
def _scene(tmp_path, extra=None, ply=True):
    d = tmp_path / "scene"
    d.mkdir(exist_ok=True)
    g = np.random.default_rng(3)
    frames = []
    for i in range(6):
        ang = 2 * np.pi * i / 6
        pos = np.array([2.0 * np.cos(ang) + 0.3, 2.0 * np.sin(ang) - 0.2, 0.7])
        fwd = -pos / np.linalg.norm(pos)
        right = np.cross(fwd, [0, 0, 1.0])
        right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, -fwd, pos
        frames.append({"file_path": f"images/frame_{i + 1:05d}.png", "transform_matrix": m.tolist(), "is_thermal": 0})
    meta = {"fl_x": 100.0, "fl_y": 100.0, "cx": 32.0, "cy": 24.0, "w": 64, "h": 48, "frames": frames}
    xyz = g.standard_normal((500, 3)).astype(np.float32)
    rgb = g.integers(0, 256, (500, 3)).astype(np.uint8)
    if ply:
        write_ply(str(d / "points.ply"), xyz, rgb)
        meta["ply_file_path"] = "points.ply"
    meta.update(extra or {})
    (d / "transforms.json").write_text(json.dumps(meta))
    return str(d), xyz, rgb


@pytest.mark.parametrize("extra", [{}, {"applied_transform": [[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, -1, 0]], "applied_scale": 0.5}])
def test_load_3D_points_transform_and_scale(tmp_path, extra):
    from nerfstudio_thermal_amd.dataparser import auto_orient_and_center_poses

    d, xyz, rgb = _scene(tmp_path, extra)
    o = ThermalNerfDataParserConfig(data=d, downscale_factor=1, load_3D_points=True, scale_factor=1.5).setup().get_dataparser_outputs("train")
    meta = json.load(open(os.path.join(d, "transforms.json")))
    poses = torch.from_numpy(np.array([f["transform_matrix"] for f in meta["frames"]]).astype(np.float32))
    oriented, transform = auto_orient_and_center_poses(poses)
    scale = 1.0 / float(torch.max(torch.abs(oriented[:, :3, 3]))) * 1.5 * float(extra.get("applied_scale", 1.0))
    assert abs(o.dataparser_scale - scale) <= 1e-12 * scale
    p = torch.from_numpy(xyz)
    want = torch.cat((p, torch.ones_like(p[..., :1])), -1) @ transform.T
    want *= o.dataparser_scale
    got = o.metadata["points3D_xyz"]
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(o.metadata["points3D_rgb"], torch.from_numpy(rgb))
    # the points move with the cameras: the camera centres, transformed the same way, are the dataparser's c2w translations
    # (applied_scale scales the points but not the poses: the reference multiplies it in after scaling the poses)
    c = torch.cat((poses[:, :3, 3], torch.ones(poses.shape[0], 1)), -1) @ transform.T * (o.dataparser_scale / float(extra.get("applied_scale", 1.0)))
    assert float((c - o.cameras["c2w"][:, :, 3]).abs().max()) < 1e-5
    if extra:  # the points use the orient / centre transform, not dataparser_transform (which also holds applied_transform)
        assert not torch.equal(o.dataparser_transform, transform)


def test_load_3D_points_off_and_missing(tmp_path, capsys):
    d, _, _ = _scene(tmp_path)
    cfg = ThermalNerfDataParserConfig(data=d, downscale_factor=1)
    off = cfg.setup().get_dataparser_outputs("train")
    assert list(off.metadata.keys()) == ["is_thermal"]
    on = ThermalNerfDataParserConfig(data=d, downscale_factor=1, load_3D_points=True).setup().get_dataparser_outputs("train")
    assert set(on.metadata.keys()) == {"is_thermal", "points3D_xyz", "points3D_rgb"}
    for k in ("image_filenames", "dataparser_scale"):
        assert getattr(on, k) == getattr(off, k)
    for k in off.cameras:
        assert torch.equal(on.cameras[k], off.cameras[k])
    assert torch.equal(on.dataparser_transform, off.dataparser_transform) and on.metadata["is_thermal"] == off.metadata["is_thermal"]
    d2, _, _ = _scene(tmp_path / "x", ply=False) if (tmp_path / "x").mkdir() is None else None
    capsys.readouterr()
    miss = ThermalNerfDataParserConfig(data=d2, downscale_factor=1, load_3D_points=True).setup().get_dataparser_outputs("train")
    assert list(miss.metadata.keys()) == ["is_thermal"]
    assert "no point cloud found" in capsys.readouterr().out


# ---- tn_knn without a device (validation happens on the host before the first launch)
def test_knn_arguments_are_refused_before_any_launch(lib):
    fake = C.c_void_p(256 * 4096)  # non-NULL, never dereferenced
    n, k = 10, 3
    need = lib.tn_knn_workspace_bytes(n, k)
    assert need > 0
    assert lib.tn_knn_workspace_bytes(-1, 3) == -1 and lib.tn_knn_workspace_bytes(2**31, 3) == -1
    assert lib.tn_knn_workspace_bytes(10, 0) == -1 and lib.tn_knn_workspace_bytes(10, 9) == -1
    assert lib.tn_knn_workspace_bytes(0, 3) == 0
    assert lib.tn_knn(None, n, k, fake, None, fake, need, None) == EINVAL
    assert b"null pointer" in lib.tn_last_error()
    assert lib.tn_knn(fake, n, k, None, None, fake, need, None) == EINVAL
    assert lib.tn_knn(fake, n, k, fake, None, None, need, None) == EINVAL
    for bad_k in (0, 9):
        assert lib.tn_knn(fake, n, bad_k, fake, fake, fake, need, None) == EINVAL
    assert lib.tn_knn(fake, 3, 3, fake, fake, fake, need, None) == EINVAL  # n < k + 1
    assert b"k + 1" in lib.tn_last_error()
    assert lib.tn_knn(fake, 2**31, 3, fake, fake, fake, need, None) == EINVAL
    assert lib.tn_knn(fake, n, k, fake, fake, fake, need - 1, None) == EINVAL
    assert b"workspace of" in lib.tn_last_error()
    assert lib.tn_knn(None, 0, 3, None, None, None, 0, None) == 0  # n == 0: nothing to do
