"""The point-cloud export without a GPU: the host-side argument checks of tn_cloud_append / tn_cloud_remove_outliers, the `thermal` property through
the PLY writer and readers, the dataparser's points3D_thermal, cloud.to_dataset_frame against load_3D_points, and the export script's --help."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib
from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig, load_3D_points, read_ply, read_ply_thermal, write_ply

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
def test_cloud_append_arguments_are_refused_before_any_launch(lib):
    fake, R, cap = C.c_void_p(256 * 4096), 1000, 500
    need = lib.tn_cloud_append_workspace_bytes(R)
    assert need > 0 and lib.tn_cloud_append_workspace_bytes(0) == 0
    assert lib.tn_cloud_append_workspace_bytes(-1) == -1 and lib.tn_cloud_append_workspace_bytes(2**31) == -1

    def call(**kw):
        a = dict(origins=fake, directions=fake, depth=fake, accumulation=fake, rgb=fake, rgb_stride=4, thermal=fake, thermal_stride=4, R=R, alpha=0.5,
                 box=None, xyz=fake, out_rgb=fake, out_thermal=fake, cap=cap, count=fake, ws=fake, ws_bytes=need)
        a.update(kw)
        return lib.tn_cloud_append(a["origins"], a["directions"], a["depth"], a["accumulation"], a["rgb"], a["rgb_stride"], a["thermal"],
                                   a["thermal_stride"], a["R"], a["alpha"], a["box"], a["xyz"], a["out_rgb"], a["out_thermal"], a["cap"], a["count"],
                                   a["ws"], a["ws_bytes"], None)

    for name in ("origins", "directions", "depth", "accumulation", "rgb", "thermal", "xyz", "out_rgb", "out_thermal", "count", "ws"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null pointer" in lib.tn_last_error()
    assert call(xyz=None, out_rgb=None, out_thermal=None, cap=0, ws_bytes=need - 1) == EINVAL and b"workspace of" in lib.tn_last_error()  # cap 0 needs no outputs
    assert call(R=-1) == EINVAL and b"rays" in lib.tn_last_error()
    assert call(R=2**31) == EINVAL
    assert call(cap=-1) == EINVAL
    assert call(rgb_stride=2) == EINVAL and call(thermal_stride=0) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and b"workspace of" in lib.tn_last_error()
    # R == 0 is TN_OK and touches nothing, whatever else is passed
    assert lib.tn_cloud_append(None, None, None, None, None, 3, None, 1, 0, 0.5, None, None, None, None, 0, None, None, 0, None) == 0


def test_cloud_remove_outliers_arguments_are_refused_before_any_launch(lib):
    fake, n, nb = C.c_void_p(256 * 4096), 1000, 20
    need = lib.tn_cloud_remove_outliers_workspace_bytes(n, nb)
    assert need > 0
    for bad in ((n, 1), (n, 33), (19, 20), (2**31, 20), (-1, 20)):
        assert lib.tn_cloud_remove_outliers_workspace_bytes(*bad) == -1, bad
    assert lib.tn_cloud_remove_outliers_workspace_bytes(20, 20) > 0 and lib.tn_cloud_remove_outliers_workspace_bytes(32, 32) > 0

    def call(**kw):
        a = dict(xyz=fake, rgb=fake, thermal=fake, n=n, nb=nb, ratio=10.0, out_xyz=fake, out_rgb=fake, out_thermal=fake, count=fake, stats=fake,
                 mean=None, keep=None, ws=fake, ws_bytes=need)
        a.update(kw)
        return lib.tn_cloud_remove_outliers(a["xyz"], a["rgb"], a["thermal"], a["n"], a["nb"], a["ratio"], a["out_xyz"], a["out_rgb"], a["out_thermal"],
                                            a["count"], a["stats"], a["mean"], a["keep"], a["ws"], a["ws_bytes"], None)

    for name in ("xyz", "rgb", "thermal", "out_xyz", "out_rgb", "out_thermal", "count", "stats", "ws"):
        assert call(**{name: None}) == EINVAL, name
        assert b"null pointer" in lib.tn_last_error()
    for bad_nb in (1, 33, 0, -3):
        assert call(nb=bad_nb) == EINVAL and b"nb_neighbors" in lib.tn_last_error()
    assert call(n=19) == EINVAL and b"needs at least" in lib.tn_last_error()  # n < nb_neighbors
    assert call(n=2**31) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and b"workspace of" in lib.tn_last_error()
    # tn_knn itself keeps refusing k = 9: the wide search is the outlier rule's alone
    assert lib.tn_knn_workspace_bytes(100, 9) == -1


def test_wrappers_refuse_host_tensors():
    from nerfstudio_thermal_amd import cloud
    from nerfstudio_thermal_amd.rays import RayBundle

    pc = cloud.PointCloud(torch.zeros(40, 3), torch.zeros(40, 3), torch.zeros(40, 1))
    with pytest.raises(ValueError, match="no CPU fallback"):
        cloud.remove_outliers(pc)
    rb = RayBundle(origins=torch.zeros(4, 3), directions=torch.zeros(4, 3), pixel_area=torch.ones(4, 1))
    out = {"rgb": torch.zeros(4, 3), "rgb_thermal": torch.zeros(4, 1), "depth": torch.zeros(4, 1), "accumulation": torch.ones(4, 1)}
    with pytest.raises(ValueError, match="no CPU fallback"):
        cloud.append_points(out, rb, pc, torch.zeros(1, dtype=torch.int64), None)


# ---- the thermal property through the PLY
def _cloud(n=57, seed=5):
    g = np.random.default_rng(seed)
    return (g.standard_normal((n, 3)).astype(np.float32), g.integers(0, 256, (n, 3)).astype(np.uint8), g.integers(0, 256, (n, 1)).astype(np.uint8))


@pytest.mark.parametrize("binary", [True, False])
def test_ply_round_trip_with_thermal(tmp_path, binary):
    xyz, rgb, th = _cloud()
    th[:3, 0] = (0, 255, 128)
    path = write_ply(str(tmp_path / "c.ply"), xyz, rgb, binary=binary, thermal=th)
    head = open(path, "rb").read().split(b"end_header")[0].decode()
    assert head.splitlines()[-1] == "property uchar thermal" and head.count("property") == 7
    x, c, t = read_ply_thermal(path)
    assert np.array_equal(x, xyz) and np.array_equal(c, rgb) and t.dtype == np.uint8 and t.shape == (57, 1) and np.array_equal(t, th)
    two = read_ply(path)  # read_ply keeps its 2-tuple
    assert isinstance(two, tuple) and len(two) == 2 and np.array_equal(two[0], xyz) and np.array_equal(two[1], rgb)
    # [M] works like [M,1]; a wrong length or type is refused
    assert open(write_ply(str(tmp_path / "d.ply"), xyz, rgb, binary=binary, thermal=th[:, 0]), "rb").read() == open(path, "rb").read()
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "e.ply"), xyz, rgb, thermal=th[:-1])
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "e.ply"), xyz, rgb, thermal=th.astype(np.float32))


def test_ply_without_thermal_reads_none_and_float_thermal_is_scaled(tmp_path):
    xyz, rgb, _ = _cloud()
    x, c, t = read_ply_thermal(write_ply(str(tmp_path / "a.ply"), xyz, rgb))
    assert t is None and np.array_equal(c, rgb)
    body = "".join(f"{p[0]} {p[1]} {p[2]} {v}\n" for p, v in zip(xyz[:3].tolist(), (0.0, 0.5, 1.0)))
    (tmp_path / "f.ply").write_text("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                                    "property float thermal\nend_header\n" + body)
    _, c, t = read_ply_thermal(str(tmp_path / "f.ply"))
    assert c.shape == (0, 3) and t[:, 0].tolist() == [0, 127, 255]


def test_write_ply_without_thermal_is_byte_identical_to_the_parents(tmp_path, golden_dir):
    """tests/golden/cloud_parent_*.ply were written by write_ply as it was before the thermal property existed, from these arrays."""
    g = np.random.default_rng(11)
    xyz, rgb = g.standard_normal((24, 3)).astype(np.float32), g.integers(0, 256, (24, 3)).astype(np.uint8)
    for name, args, kw in (("binary", (xyz, rgb), {"binary": True}), ("ascii", (xyz, rgb), {"binary": False}),
                           ("xyz_only", (xyz.astype(np.float64), None), {"binary": True})):
        want = open(os.path.join(golden_dir, f"cloud_parent_{name}.ply"), "rb").read()
        assert open(write_ply(str(tmp_path / f"{name}.ply"), *args, **kw), "rb").read() == want, name
        assert open(write_ply(str(tmp_path / f"{name}_none.ply"), *args, thermal=None, **kw), "rb").read() == want, name


# ---- the dataparser and the frames
def test_load_3D_points_adds_the_thermal_key_only_for_files_that_have_it(tmp_path):
    d, xyz, rgb = _scene(tmp_path)
    cfg = lambda: ThermalNerfDataParserConfig(data=d, downscale_factor=1, load_3D_points=True)  # noqa: E731
    plain = cfg().setup().get_dataparser_outputs("train")
    assert set(plain.metadata.keys()) == {"is_thermal", "points3D_xyz", "points3D_rgb"}
    th = np.random.default_rng(1).integers(0, 256, (xyz.shape[0], 1)).astype(np.uint8)
    write_ply(os.path.join(d, "points.ply"), xyz, rgb, thermal=th)
    with_th = cfg().setup().get_dataparser_outputs("train")
    assert set(with_th.metadata.keys()) == {"is_thermal", "points3D_xyz", "points3D_rgb", "points3D_thermal"}
    t = with_th.metadata["points3D_thermal"]
    assert t.dtype == torch.uint8 and tuple(t.shape) == (xyz.shape[0], 1) and torch.equal(t, torch.from_numpy(th))
    assert torch.equal(with_th.metadata["points3D_xyz"], plain.metadata["points3D_xyz"])
    assert torch.equal(with_th.metadata["points3D_rgb"], plain.metadata["points3D_rgb"])


@pytest.mark.parametrize("extra", [{}, {"applied_transform": [[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, -1, 0]], "applied_scale": 0.5}])
def test_to_dataset_frame_then_load_3D_points_returns_the_points(tmp_path, extra):
    """A cloud in the model's frame, taken to the dataset's frame (float64, rounded once), written as the dataset's PLY and loaded back by
    load_3D_points (float32: p @ T^T, then * scale) lands where it was.  The float64 restatement of that round trip is the identity, so the
    cloud itself is the reference.  Error budget per coordinate, in units of u = 2^-24 times the magnitude M below: one rounding of the stored
    dataset coordinate, one per product, three for the sums of the row, one for the scale -- under 8 u M, the project's usual factor, with
    M = scale * max_i (sum_j |T_ij| |q_j| + |t_i|), the largest magnitude the float64 evaluation of the row can reach."""
    from nerfstudio_thermal_amd import cloud
    from nerfstudio_thermal_amd.dataparser import auto_orient_and_center_poses

    d, _, rgb = _scene(tmp_path, extra)
    o = ThermalNerfDataParserConfig(data=d, downscale_factor=1, load_3D_points=True, scale_factor=1.5).setup().get_dataparser_outputs("train")
    g = torch.Generator().manual_seed(2)
    pts = (torch.rand((500, 3), generator=g) * 2 - 1).float()
    q = cloud.to_dataset_frame(pts, o, extra.get("applied_transform"))
    assert q.dtype == torch.float32 and tuple(q.shape) == (500, 3)
    write_ply(os.path.join(d, "points.ply"), q.numpy(), rgb)
    meta = json.load(open(os.path.join(d, "transforms.json")))
    poses = torch.from_numpy(np.array([f["transform_matrix"] for f in meta["frames"]]).astype(np.float32))
    _, transform = auto_orient_and_center_poses(poses)
    back = load_3D_points(os.path.join(d, "points.ply"), transform, o.dataparser_scale)["points3D_xyz"]
    again = ThermalNerfDataParserConfig(data=d, downscale_factor=1, load_3D_points=True, scale_factor=1.5).setup().get_dataparser_outputs("train")
    assert torch.equal(again.metadata["points3D_xyz"], back)  # the dataparser applies exactly this
    T = transform.double()
    M = float(o.dataparser_scale) * float((q.double().abs() @ T[:, :3].abs().T + T[:, 3].abs()).max())
    bound = 8 * 2.0**-24 * M
    err = float((back.double() - pts.double()).abs().max())
    print(f"to_dataset_frame -> load_3D_points: max error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound
    # without the inverse the cloud would move: the test scene's transform is not the identity
    assert float((load_3D_points(os.path.join(d, "points.ply"), transform, o.dataparser_scale)["points3D_xyz"] - q).abs().max()) > 1e-2


def test_export_script_help_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "export_point_cloud.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--num-points" in r.stdout and "--set-ply-file-path" in r.stdout and "--obb-center" in r.stdout
