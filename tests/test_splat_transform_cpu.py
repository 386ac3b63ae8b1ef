"""Moving thermal splats by a similarity, without a GPU: the SH band rotation matrices against the oracle's basis, `Similarity` and `dataset_frame`
against cloud.to_dataset_frame and load_3D_points, the quaternion of a rotation, the host-side argument checks of tn_transform_splat, and the
render invariance of the restatement (tests/splat_transform_functional.py) on the CPU oracle, which also records the float32 floors the GPU test
is held to."""
import ctypes as C
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
import splat_oracle as so
import splat_transform_functional as stf
from nerfstudio_thermal_amd import _lib, cloud
from nerfstudio_thermal_amd import splat_transform as st
from nerfstudio_thermal_amd.splat_camera import OrientedBox, PinholeCamera

from test_splat_seed_cpu import _scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
EYE = lambda n: torch.eye(n, dtype=F64)  # noqa: E731


def make_fields(scale, R, t):
    """The TnSplatTransform fields as the package fills them."""
    return stf.fields(scale, R, t, st.rotation_quaternion(R), st.sh_rotation_matrices(R))


def _rot(seed):
    return stf.seeded_rotation(seed)[0]


def _axis_pi(axis):
    d = [-1.0, -1.0, -1.0]
    d[axis] = 1.0
    return torch.diag(torch.tensor(d, dtype=F64))


# ---------------------------------------------------------------------------------------------------- the band matrices
def test_band_matrices_of_the_identity_are_identities():
    for M, n in zip(st.sh_rotation_matrices(EYE(3)), (3, 5, 7)):
        assert M.dtype == F64 and tuple(M.shape) == (n, n)
        assert float((M - EYE(n)).abs().max()) <= 1e-12


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_band_matrices_are_orthogonal_and_compose(seed):
    R1, R2 = _rot(seed), _rot(seed + 10)
    for M1, M2, M12, n in zip(st.sh_rotation_matrices(R1), st.sh_rotation_matrices(R2), st.sh_rotation_matrices(R1 @ R2), (3, 5, 7)):
        assert float((M1 @ M1.T - EYE(n)).abs().max()) <= 1e-12
        assert float((M12 - M1 @ M2).abs().max()) <= 1e-12


def test_the_package_basis_is_the_oracles():
    """sh_basis (the product's restatement of sh_eval's 16 functions) against the oracle, coefficient by coefficient."""
    g = torch.Generator().manual_seed(4)
    d = torch.randn(500, 3, generator=g, dtype=F64)
    d = d / d.norm(dim=-1, keepdim=True)
    B = st.sh_basis(d)
    for k in range(16):
        c = torch.zeros(500, 16, 1, dtype=F64)
        c[:, k] = 1.0
        assert float((so.spherical_harmonics(3, d, c)[:, 0] - B[:, k]).abs().max()) <= 1e-15, k


@pytest.mark.parametrize("seed", [1, 7])
def test_rotated_coefficients_show_the_same_colours_in_the_rotated_frame(seed):
    """SH(c')(R d) = SH(c)(d) in float64 at degrees 1, 2, 3, with c' from the band matrices directly and from the restatement of the kernel (which
    rounds c' to float32: compared there at float32's precision)."""
    R = _rot(seed)
    mats = st.sh_rotation_matrices(R)
    g = torch.Generator().manual_seed(seed)
    n = 2000
    c = torch.randn(n, 16, 3, generator=g, dtype=F64)
    d = torch.randn(n, 3, generator=g, dtype=F64)
    c2 = c.clone()
    for (a, b), M in zip(st.BANDS, mats):
        c2[:, a:b] = torch.einsum("ij,njc->nic", M, c[:, a:b])
    worst = 0.0
    for deg in (1, 2, 3):
        err = float((so.spherical_harmonics(deg, d @ R.T, c2) - so.spherical_harmonics(deg, d, c)).abs().max())
        worst = max(worst, err)
        assert err <= 1e-12, (deg, err)
    print(f"SH(c')(R d) - SH(c)(d), float64: {worst:.2e}")
    # through the restatement: float32 coefficients in, float64 evaluation, one rounding to float32 out
    f = make_fields(1.0, R, torch.zeros(3, dtype=F64))
    c32 = c.float()
    moved = torch.cat([c32[:, :1], stf.rotate_rest(f, c32[:, 1:].contiguous())], 1)
    exact = c32.double().clone()
    for (a, b), M in zip(st.BANDS, mats):
        exact[:, a:b] = torch.einsum("ij,njc->nic", M, c32.double()[:, a:b])
    assert float((moved.double() - exact).abs().max()) <= 2.0 ** -24 * float(exact.abs().max())  # half an ulp of the largest, and 1e-12 of slack
    for deg in (1, 2, 3):  # 15 coefficients each within half a float32 ulp, basis values below 3
        err = float((so.spherical_harmonics(deg, d @ R.T, moved.double()) - so.spherical_harmonics(deg, d, c32.double())).abs().max())
        assert err <= 15 * 3 * 2.0 ** -24 * float(exact.abs().max()), (deg, err)


@pytest.mark.parametrize("seed", [1, 2])
def test_band_1_is_the_rotation_in_the_basis_minus_y_z_minus_x(seed):
    R = _rot(seed)
    P = torch.tensor([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]], dtype=F64)  # Y_1(d) = C1 P d
    assert float((st.sh_rotation_matrices(R)[0] - P @ R @ P.T).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------- Similarity
def test_from_matrix_refuses_what_is_not_a_similarity():
    R = _rot(3)
    t = torch.tensor([[0.1], [0.2], [0.3]], dtype=F64)
    shear = R.clone()
    shear[0, 1] += 1e-3
    with pytest.raises(ValueError, match="shears and non-uniform"):
        st.Similarity.from_matrix(torch.cat([shear, t], 1))
    with pytest.raises(ValueError, match="shears and non-uniform"):
        st.Similarity.from_matrix(torch.cat([R @ torch.diag(torch.tensor([1.0, 1.0, 1.01], dtype=F64)), t], 1))
    with pytest.raises(ValueError, match="reflections"):
        st.Similarity.from_matrix(torch.cat([R @ torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=F64)), t], 1))
    with pytest.raises(ValueError):
        st.Similarity.from_matrix(torch.zeros(3, 3))
    with pytest.raises(ValueError):
        st.Similarity(0.0, R, t.reshape(-1))
    T = st.Similarity.from_matrix(torch.cat([2.5 * R, t], 1))
    assert abs(T.scale - 2.5) <= 1e-12 and float((T.R - R).abs().max()) <= 1e-12 and float((T.t - t.reshape(-1)).abs().max()) == 0.0
    T4 = st.Similarity.from_matrix(torch.cat([T.matrix(), torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=F64)], 0))
    assert float((T4.matrix() - T.matrix()).abs().max()) <= 1e-12


def test_inverse_compose_and_identity():
    T = st.Similarity(0.4, _rot(5), torch.tensor(stf.T_VEC))
    for I in (T.inverse().compose(T), T.compose(T.inverse())):  # noqa: E741
        assert float((I.matrix() - st.Similarity.identity().matrix()).abs().max()) <= 1e-12
    assert st.Similarity.identity().is_identity and not T.is_identity
    U = st.Similarity(2.0, _rot(8), torch.tensor([0.0, 1.0, -1.0]))
    p = torch.randn(50, 3, dtype=F64, generator=torch.Generator().manual_seed(0))
    assert float((T.compose(U).apply_points(p) - T.apply_points(U.apply_points(p))).abs().max()) <= 1e-12
    assert float((T.apply_points(p) - (p @ (0.4 * T.R).T + T.t)).abs().max()) <= 1e-12
    q = T.apply_points(p.float())
    assert q.dtype == torch.float32 and torch.equal(q, T.apply_points(p.float().double()).float())  # float64 inside, rounded once


def test_apply_camera_keeps_everything_but_the_pose():
    T = st.Similarity(2.5, _rot(5), torch.tensor(stf.T_VEC))
    cam = PinholeCamera(stf.camera_c2w(), 80.0, 81.0, 48.0, 36.0, 96, 72, cam_idx=3, is_thermal=True)
    got = T.apply_camera(cam)
    assert (got.fx, got.fy, got.cx, got.cy, got.width, got.height, got.cam_idx, got.is_thermal) == (80.0, 81.0, 48.0, 36.0, 96, 72, 3, True)
    assert got.camera_to_world.dtype == torch.float32 and torch.equal(got.camera_to_world, stf.moved_c2w(2.5, T.R, T.t, cam.camera_to_world))
    assert torch.equal(cam.camera_to_world, stf.camera_c2w())  # the caller's camera is left alone


@pytest.mark.parametrize("extra", [{}, {"applied_transform": [[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, -1, 0]], "applied_scale": 0.5}])
def test_dataset_frame_is_the_map_of_to_dataset_frame(tmp_path, extra):
    """dataset_frame against cloud.to_dataset_frame on random points, through a dataparser output with a transform, a scale and (second case) an
    applied_transform: both evaluate the same float64 map and round once, in different orders, so they agree within 2 float32 ulp of the largest
    coordinate.  The inverse takes the file's points where load_3D_points (float32 arithmetic) puts them, within that function's own error."""
    from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig

    d, xyz, _ = _scene(tmp_path, extra)
    o = ThermalNerfDataParserConfig(data=d, downscale_factor=1, load_3D_points=True, scale_factor=1.5).setup().get_dataparser_outputs("train")
    T = st.dataset_frame(o, extra.get("applied_transform"))
    assert not T.is_identity and abs(T.scale * float(o.dataparser_scale) - 1.0) <= 1e-6  # (the dataparser's float32 rotation is orthogonal to ~1e-7)
    pts = (torch.rand((500, 3), generator=torch.Generator().manual_seed(2)) * 2 - 1).float()
    want = cloud.to_dataset_frame(pts, o, extra.get("applied_transform"))
    got = T.apply_points(pts)
    ulp = float(stf_ulp(want.abs().max()))
    assert got.dtype == torch.float32 and float((got.double() - want.double()).abs().max()) <= 2 * ulp
    # the file's points -> the model's frame: load_3D_points' result, up to its float32 arithmetic (8 u M as in test_cloud_cpu.py)
    model_pts = o.metadata["points3D_xyz"]
    file_pts = torch.from_numpy(xyz).float()
    back = T.inverse().apply_points(file_pts)
    M = float(model_pts.abs().max()) + float(T.inverse().t.abs().max())
    assert float((back.double() - model_pts.double()).abs().max()) <= 8 * 2.0 ** -24 * M
    assert float((T.apply_points(model_pts).double() - file_pts.double()).abs().max()) <= 8 * 2.0 ** -24 * M / T.inverse().scale


def stf_ulp(x):
    a = torch.as_tensor(x).float().abs()
    return (torch.nextafter(a, torch.tensor(float("inf"))) - a).double()


def test_apply_box_keeps_the_same_points():
    T = st.Similarity(0.4, _rot(5), torch.tensor(stf.T_VEC))
    box = OrientedBox.from_params((0.1, -0.05, 0.0), (0.3, -0.2, 0.5), (0.9, 0.7, 0.8))
    p = (torch.rand((4000, 3), generator=torch.Generator().manual_seed(1)) * 1.6 - 0.8).float()
    q = (box.world_to_box().double()[:, :3] @ p.double().T).T + box.world_to_box().double()[:, 3]
    clear = ((q.abs() - 0.5 * box.S.double()).abs() >= 1e-3).all(-1)  # at least 1e-3 from every face
    p = p[clear]
    inside = box.within(p)
    assert 200 < int(inside.sum()) < int(inside.numel()) - 200
    moved = T.apply_box(box)
    assert moved.R.dtype == torch.float32 and torch.equal(moved.S, (0.4 * box.S.double()).float())
    assert torch.equal(moved.within(T.apply_points(p)), inside)


def test_rotation_quaternion():
    cases = [_rot(s) for s in range(1, 6)] + [_axis_pi(a) for a in range(3)] + [EYE(3)]
    cases += [so.quat_to_rotmat(torch.tensor([[1e-9, 1.0, 0.2, -0.3]], dtype=F64))[0]]  # almost a half turn
    for R in cases:
        q = st.rotation_quaternion(R)
        assert q.dtype == F64 and float(q[0]) >= 0.0 and abs(float(q.norm()) - 1.0) <= 1e-15
        assert float((so.quat_to_rotmat(q[None])[0] - R).abs().max()) <= 1e-14
    with pytest.raises(ValueError):
        st.rotation_quaternion(_rot(1) * 1.1)


def test_quaternion_product_rotates_the_gaussian():
    """R(q_R (x) q) = R R(q), through the restatement's product (float32 quaternions in and out: float32's precision)."""
    R, qR = stf.seeded_rotation()
    assert float((st.rotation_quaternion(R) - qR).abs().max()) <= 1e-15
    p = stf.scene()
    f = make_fields(1.0, R, torch.zeros(3, dtype=F64))
    moved = stf.transform_ref(f, p)["quats"]
    assert float((so.quat_to_rotmat(moved.double()) - R @ so.quat_to_rotmat(p["quats"].double())).abs().max()) <= 8 * 2.0 ** -24
    # the stored norm is kept (the renderer normalises)
    assert float((moved.double().norm(dim=-1) / p["quats"].double().norm(dim=-1) - 1).abs().max()) <= 4 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- the entry point, on the host
def test_struct_is_the_headers_and_holds_the_similarity(tmp_path):
    T = st.Similarity(0.4, _rot(5), torch.tensor(stf.T_VEC))
    s = st.transform_struct(T)
    f = make_fields(T.scale, T.R, T.t)
    assert list(s.A) == f["A"].reshape(-1).tolist() and list(s.t) == f["t"].tolist() and s.log_scale == math.log(0.4)
    assert list(s.q) == f["q"].tolist() and list(s.sh1) == f["sh1"].reshape(-1).tolist() and list(s.sh2) == f["sh2"].reshape(-1).tolist()
    assert list(s.sh3) == f["sh3"].reshape(-1).tolist()
    assert C.sizeof(_lib.TnSplatTransform) == 8 * (9 + 3 + 1 + 4 + 9 + 25 + 49)
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    names = [n for n, _ in _lib.TnSplatTransform._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n  printf("%%zu\\n", sizeof(TnSplatTransform));\n%s  return 0;\n}\n'
                   % (os.path.join(ROOT, "include", "thermal_nerf_hip.h"),
                      "".join('  printf("%%zu\\n", offsetof(TnSplatTransform, %s));\n' % n for n in names)))
    subprocess.run(["gcc", "-o", str(tmp_path / "layout"), str(src)], check=True)
    vals = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()]
    assert vals == [C.sizeof(_lib.TnSplatTransform)] + [getattr(_lib.TnSplatTransform, n).offset for n in names]


def test_arguments_are_checked_before_any_launch():
    """Validation happens on the host before the launch, so it runs here without a device; the pointers only have to be non-null."""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = _lib.load()
    s = st.transform_struct(st.Similarity(0.4, _rot(5), torch.tensor(stf.T_VEC)))
    fake = C.c_void_p(256 * 4096)  # never dereferenced
    five = [fake] * 5
    call = lambda tr, ins, n, R, outs: lib.tn_transform_splat(tr, *ins, n, R, *outs, None)  # noqa: E731
    assert call(None, five, 4, 15, five) == -22 and b"null pointer (transform)" in lib.tn_last_error()
    assert call(C.byref(s), five, -1, 15, five) == -22 and b"Gaussians" in lib.tn_last_error()
    assert call(C.byref(s), five, 2 ** 31, 15, five) == -22
    for R in (-1, 1, 2, 4, 9, 14, 16, 24, 45):
        assert call(C.byref(s), five, 4, R, five) == -22 and b"rest coefficients" in lib.tn_last_error(), R
    for hole in range(5):  # a null input or output the call needs
        for side in (0, 1):
            ins, outs = list(five), list(five)
            (ins if side == 0 else outs)[hole] = None
            assert call(C.byref(s), ins, 4, 15, outs) == -22 and b"null pointer" in lib.tn_last_error(), (hole, side)
    nothing = [None] * 5
    for R in (0, 3, 8, 15):  # no Gaussians: nothing is read, nothing launched
        assert call(C.byref(s), nothing, 0, R, nothing) == 0


def test_transform_call_passes_the_bindings_arguments_and_checks_shapes(monkeypatch):
    """On CPU placeholders with the pointer check and the library call replaced: the segments add up to the binding's argument list, the rest
    pointers are null for a degree-0 model, and a tensor of another shape is refused before the call."""
    from nerfstudio_thermal_amd import splat_calls as sc

    seen = []
    monkeypatch.setattr(sc, "_call", lambda name, *args: seen.append((name, args)))
    monkeypatch.setattr(sc, "_ptr", lambda t, dtype, name: None if t is None else C.c_void_p(1))
    s = _lib.TnSplatTransform()
    Z = torch.zeros
    for R in (15, 0):
        t = [Z(5, 3), Z(5, 3), Z(5, 4), Z(5, R, 3), Z(5, R, 1)]
        sc.transform_call(s, *t, *t)
        name, args = seen[-1]
        assert name == "tn_transform_splat" and len(args) + 1 == len(_lib.SIGNATURES[name][1])  # + the stream
        assert args[6:8] == (5, R) and [a is None for a in args[4:6] + args[11:13]] == [R == 0] * 4
    with pytest.raises(ValueError, match="quats"):
        sc.transform_call(s, Z(5, 3), Z(5, 3), Z(5, 3), Z(5, 15, 3), Z(5, 15, 1), *t)
    with pytest.raises(ValueError, match="features_rest_thermal"):
        sc.transform_call(s, *t[:4], Z(5, 0, 3), *t)


def test_the_exporters_offer_the_dataset_frame():
    for script, flags in (("export_gaussian_splat.py", ("--save-world-frame", "--load-world-frame")), ("train_splat_scene.py", ("--export-world-frame",)),
                          ("time_splat_transform.py", ("--gaussians",))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True, check=True).stdout
        for flag in flags:
            assert flag in out, (script, flag)


# ---------------------------------------------------------------------------------------------------- render invariance on the oracle
@pytest.mark.parametrize("scale", stf.SCALES)
def test_the_moved_scene_from_the_moved_camera_renders_the_same_frame(scale):
    """The oracle's float32 render of the restatement-moved parameters from the moved camera against its render of the original: rgb, thermal and
    accumulation, and depth against scale * depth where accumulation > 0.5.  A wrong band matrix, quaternion order or scale rule shows as O(0.1);
    the float32 floor of the two frames is ~1e-5 (measured with this file's seeded rotation: rgb 3.3e-6 / 2.0e-6 / 7.6e-6 and thermal 2.3e-6 /
    9.5e-7 / 4.2e-6 at scales 1 / 2.5 / 0.4), so the limit 1e-4 separates the two with a margin a different libm cannot use up.  The differences printed here are the floors
    tests/test_splat_transform_gpu.py multiplies by 8."""
    a, b = stf.oracle_pair(scale, 3, "classic", False, make_fields)
    d = stf.image_differences(a, b, scale)
    print(f"scale {scale}: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert float((a["accumulation"] > 0.5).float().mean()) > 0.2 and float(a["rgb"].max() - a["rgb"].min()) > 0.5  # a scene, not a flat frame
    assert torch.equal(a["projection"]["radii"], b["projection"]["radii"]) and int((a["projection"]["radii"] > 0).sum()) > 250
    for k, v in d.items():
        assert v <= 1e-4, (k, v)


@pytest.mark.parametrize("deg,mode", [(1, "classic"), (-1, "classic"), (3, "antialiased")])
def test_invariance_holds_with_fewer_bands_and_antialiased(deg, mode):
    """Degree 1 active (bands 2 and 3 are moved but not read), the sh_degree == 0 model (only geometry moves) and the antialiased compensation."""
    a, b = stf.oracle_pair(0.4, deg, mode, False, make_fields)
    for k, v in stf.image_differences(a, b, 0.4).items():
        assert v <= 1e-4, (k, v)


def test_a_wrong_move_is_far_above_the_limit():
    """The limit can tell: the same comparison with the band-3 matrix transposed, and with the quaternion product the other way round."""
    R, _ = stf.seeded_rotation()
    t = torch.tensor(stf.T_VEC, dtype=F64)
    p = {k: v for k, v in stf.scene().items() if k != "opacities_thermal"}
    c2w = stf.camera_c2w()
    a = stf._render(p, c2w, 3, "classic")
    f = make_fields(1.0, R, t)
    bad = dict(f, sh3=f["sh3"].T.contiguous())
    b = stf._render(stf.moved_params(bad, p), stf.moved_c2w(1.0, R, t, c2w), 3, "classic")
    assert stf.image_differences(a, b, 1.0)["rgb"] > 1e-2
    plain = dict(f, q=torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=F64))  # Gaussians moved but not turned
    b = stf._render(stf.moved_params(plain, p), stf.moved_c2w(1.0, R, t, c2w), 3, "classic")
    assert stf.image_differences(a, b, 1.0)["rgb"] > 1e-2
