"""The host side of the Gaussian-splat PLY export and import (nerfstudio_thermal_amd/splat_io.py): the property lists, the file layer's round
trip, files written by hand, every refusal, the entry point's argument validation (before any launch: no device needed), and the conditions the
GPU tests' inputs must meet."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest
import torch

import splat_crop_functional as scf
import splat_export_functional as sxf
import splat_sep_functional as ssf

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib, splat_io


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _params(d, separate):
    p = scf.crop_scene(0, d)
    return p if separate else ssf.shared_params(p)


# ---------------------------------------------------------------------------------------------------- 1. the property lists
@pytest.mark.parametrize("K", [1, 4, 9, 16])
@pytest.mark.parametrize("separate", [False, True], ids=["shared", "separate"])
def test_ply_properties_are_the_documented_lists(K, separate):
    R = K - 1
    head = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    tail = ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    rgb = head + ["f_rest_%d" % i for i in range(3 * R)] + tail
    assert splat_io.ply_properties("rgb", K, separate) == rgb and len(rgb) == 14 + 3 * K
    assert splat_io.ply_properties("thermal", K, separate) == rgb  # the same names: any viewer shows the thermal scene in grey
    both = rgb + ["f_dc_thermal"] + ["f_rest_thermal_%d" % i for i in range(R)] + (["opacity_thermal"] if separate else [])
    assert splat_io.ply_properties("both", K, separate) == both and len(both) == 14 + 3 * K + K + int(separate)
    for s in ("rgb", "thermal", "both"):
        assert splat_io.ply_properties(s, K, separate) == sxf.properties(s, K, separate)
    if K == 16:
        assert len(rgb) == 62
    if K == 1:  # the degree-0 layout has the same names as K = 1
        for s in ("rgb", "thermal", "both"):
            assert splat_io.ply_properties(s, 1, separate, colour_mode=1) == splat_io.ply_properties(s, 1, separate)
    else:
        with pytest.raises(ValueError):
            splat_io.ply_properties("rgb", K, separate, colour_mode=1)
    with pytest.raises(ValueError):
        splat_io.ply_properties("infrared", K, separate)


# ---------------------------------------------------------------------------------------------------- 2. write -> read, bit for bit
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("separate", [False, True], ids=["shared", "separate"])
def test_write_then_read_returns_every_parameter_bit_for_bit(tmp_path, d, separate):
    p = _params(d, separate)
    K = (d + 1) ** 2
    rows, kept = sxf.pack_ref(p, "both")
    assert kept.tolist() == list(range(scf.N_SCENE)) and rows.shape == (scf.N_SCENE, 14 + 3 * K + K + int(separate))
    props = splat_io.ply_properties("both", K, separate)
    path = splat_io.write_gaussian_ply(str(tmp_path / "splat.ply"), rows.numpy(), props)
    got, info = splat_io.read_gaussian_ply(path)
    assert info["num_gaussians"] == scf.N_SCENE and info["K"] == K and info["sh_degree"] == d and info["has_thermal"] and info["separate"] == separate
    assert info["properties"] == props and info["colour_mode"] == 0
    assert set(got) == set(p)
    for k in p:
        assert got[k].dtype == torch.float32 and got[k].shape == p[k].shape, k
        assert torch.equal(_bits(got[k]), _bits(p[k])), k
    # the header is the Inria one
    head = open(path, "rb").read(4096).split(b"end_header\n")[0].decode("ascii").splitlines()
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex %d" % scf.N_SCENE]
    assert head[3:] == ["property float " + n for n in props]
    assert os.path.getsize(path) == len("\n".join(head)) + 1 + len("end_header\n") + 4 * rows.numel()


# ---------------------------------------------------------------------------------------------------- 3. a hand-built Inria-order file
def _hand_file(path, order, values, extra_uchar=None, fmt="binary_little_endian", count=None, drop_bytes=0):
    """A PLY of float properties `order` (values[name] -> float32 [M]) with, unless None, a uchar property `extra_uchar` after the third float."""
    M = len(next(iter(values.values())))
    head = ["ply", "format %s 1.0" % fmt, "comment written by hand", "element vertex %d" % (M if count is None else count)]
    fields = []
    for i, n in enumerate(order):
        if extra_uchar is not None and i == 3:
            head.append("property uchar " + extra_uchar)
            fields.append((extra_uchar, "u1"))
        head.append("property float " + n)
        fields.append((n, "<f4"))
    head.append("end_header")
    rec = np.zeros(M, dtype=fields)
    for n in order:
        rec[n] = values[n]
    if extra_uchar is not None:
        rec[extra_uchar] = np.arange(M) % 251
    body = rec.tobytes()
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii") + body[:len(body) - drop_bytes])
    return path


def _inria_values(M, K, seed=0):
    names = [n for n in splat_io.ply_properties("rgb", K, False) if n not in ("nx", "ny", "nz")]
    rng = np.random.default_rng(seed)
    return names, {n: rng.standard_normal(M).astype(np.float32) for n in names}


def test_a_hand_built_inria_file_loads_to_the_right_tensors(tmp_path):
    M, K = 7, 4
    R = K - 1
    names, vals = _inria_values(M, K)
    order = list(reversed(names))  # shuffled: nothing is where the writer would put it
    order[1], order[5] = order[5], order[1]
    path = _hand_file(str(tmp_path / "inria.ply"), order, vals, extra_uchar="label")
    p, info = splat_io.read_gaussian_ply(path)
    assert info["K"] == K and info["sh_degree"] == 1 and not info["has_thermal"] and not info["separate"] and info["num_gaussians"] == M
    col = lambda *ns: torch.from_numpy(np.stack([vals[n] for n in ns], -1))  # noqa: E731
    assert torch.equal(p["means"], col("x", "y", "z")) and torch.equal(p["scales"], col("scale_0", "scale_1", "scale_2"))
    assert torch.equal(p["quats"], col("rot_0", "rot_1", "rot_2", "rot_3")) and torch.equal(p["opacities"], col("opacity"))
    assert torch.equal(p["features_dc"], col("f_dc_0", "f_dc_1", "f_dc_2"))
    assert p["features_rest"].shape == (M, R, 3)
    for k in range(R):
        for c in range(3):
            assert torch.equal(p["features_rest"][:, k, c], torch.from_numpy(vals["f_rest_%d" % (c * R + k)])), (k, c)
    # thermal by the project's rule for Gaussians without thermal values: zeros, mid-grey
    assert p["features_dc_thermal"].shape == (M, 1) and not bool(p["features_dc_thermal"].any())
    assert p["features_rest_thermal"].shape == (M, R, 1) and not bool(p["features_rest_thermal"].any())
    assert "opacities_thermal" not in p


def test_a_file_without_f_rest_read_for_a_degree_0_model_inverts_the_colour_convention(tmp_path):
    M = 9
    names, vals = _inria_values(M, 1, seed=1)
    colour = np.linspace(0.02, 0.98, 3 * M).reshape(M, 3)
    for c in range(3):
        vals["f_dc_%d" % c] = ((colour[:, c] - 0.5) / sxf.SH_C0).astype(np.float32)
    path = _hand_file(str(tmp_path / "deg0.ply"), names, vals)
    as_sh, info = splat_io.read_gaussian_ply(path)  # no degree wanted: the coefficients as stored
    assert info["K"] == 1 and info["colour_mode"] == 0
    assert torch.equal(as_sh["features_dc"][:, 0], torch.from_numpy(vals["f_dc_0"]))
    p, info = splat_io.read_gaussian_ply(path, sh_degree=0)
    assert info["colour_mode"] == 1 and p["features_rest"].shape == (M, 0, 3) and p["features_rest_thermal"].shape == (M, 0, 1)
    f = torch.from_numpy(np.stack([vals["f_dc_%d" % c] for c in range(3)], -1)).double()
    want = torch.log((0.5 + sxf.SH_C0 * f) / (0.5 - sxf.SH_C0 * f))  # logit(0.5 + C0 f) in float64
    assert float((p["features_dc"].double() - want).abs().max()) <= 4.0 * 2.0 ** -24 * float(want.abs().max())
    assert float((torch.sigmoid(p["features_dc"].double()) - torch.from_numpy(colour)).abs().max()) < 1e-6
    assert not bool(p["features_dc_thermal"].any())  # sigmoid(0) = 0.5: mid-grey in this convention too
    # a file with rest coefficients is not a degree-0 file
    names4, vals4 = _inria_values(M, 4)
    with pytest.raises(ValueError, match="degree-0"):
        splat_io.read_gaussian_ply(_hand_file(str(tmp_path / "deg1.ply"), names4, vals4), sh_degree=0)


# ---------------------------------------------------------------------------------------------------- 4. the refusals
def test_read_refusals(tmp_path):
    M, K = 5, 4
    names, vals = _inria_values(M, K)
    ok = _hand_file(str(tmp_path / "ok.ply"), names, vals)
    assert splat_io.read_gaussian_ply(ok)[1]["K"] == K
    with pytest.raises(ValueError, match="binary_little_endian"):
        splat_io.read_gaussian_ply(_hand_file(str(tmp_path / "ascii.ply"), names, vals, fmt="ascii"))
    with pytest.raises(ValueError, match="big-endian"):
        splat_io.read_gaussian_ply(_hand_file(str(tmp_path / "be.ply"), names, vals, fmt="binary_big_endian"))
    for gone in ("x", "f_dc_1", "opacity", "scale_2", "rot_0"):
        with pytest.raises(ValueError, match="lack the properties"):
            splat_io.read_gaussian_ply(_hand_file(str(tmp_path / "missing.ply"), [n for n in names if n != gone], vals))
    # K that is no square: 3 (K - 1) = 12 -> K = 5; and a count that is no multiple of 3
    for n_rest in (12, 10):
        extra = ["f_rest_%d" % i for i in range(n_rest)]
        v = dict(vals, **{n: np.zeros(M, np.float32) for n in extra})
        with pytest.raises(ValueError, match="square K"):
            splat_io.read_gaussian_ply(_hand_file(str(tmp_path / "k.ply"), [n for n in names if not n.startswith("f_rest_")] + extra, v))
    with pytest.raises(ValueError, match="not numbered"):
        splat_io.read_gaussian_ply(_hand_file(str(tmp_path / "gap.ply"), [n for n in names if n != "f_rest_4"], vals))
    # a payload shorter than the header promises: a byte short, and a vertex count one too high
    with pytest.raises(ValueError, match="truncated"):
        splat_io.read_gaussian_ply(_hand_file(str(tmp_path / "short.ply"), names, vals, drop_bytes=1))
    with pytest.raises(ValueError, match="truncated"):
        splat_io.read_gaussian_ply(_hand_file(str(tmp_path / "count.ply"), names, vals, count=M + 1))
    # thermal properties that do not fit K
    v = dict(vals, f_dc_thermal=np.zeros(M, np.float32), f_rest_thermal_0=np.zeros(M, np.float32))
    with pytest.raises(ValueError, match="thermal properties"):
        splat_io.read_gaussian_ply(_hand_file(str(tmp_path / "th.ply"), names + ["f_dc_thermal", "f_rest_thermal_0"], v))
    with pytest.raises(ValueError, match="thermal properties"):
        splat_io.read_gaussian_ply(_hand_file(str(tmp_path / "th2.ply"), names + ["opacity_thermal"], dict(vals, opacity_thermal=np.zeros(M, np.float32))))
    with pytest.raises(ValueError, match="not a PLY"):
        bad = tmp_path / "bad.ply"
        bad.write_bytes(b"solid\n")
        splat_io.read_gaussian_ply(str(bad))
    with pytest.raises(ValueError):
        splat_io.write_gaussian_ply(str(tmp_path / "w.ply"), np.zeros((3, 4), np.float32), ["x", "y", "z"])
    with pytest.raises(ValueError):
        splat_io.write_gaussian_ply(str(tmp_path / "w.ply"), np.zeros((3, 3), np.float64), ["x", "y", "z"])


class _Model:
    """What load_gaussian_ply touches of a model."""

    def __init__(self, sh_degree, separate):
        self.config = type("Cfg", (), {"sh_degree": sh_degree, "thermal_opacity_mode": "separate" if separate else "shared"})()
        self.separate = separate
        self.loaded = None

    def load_gaussians(self, params):
        self.loaded = params


def test_load_checks_the_degree_and_the_opacity_mode(tmp_path):
    p = _params(3, True)
    rows, _ = sxf.pack_ref(p, "both")
    sep = splat_io.write_gaussian_ply(str(tmp_path / "sep.ply"), rows.numpy(), splat_io.ply_properties("both", 16, True))
    m = _Model(3, True)
    assert splat_io.load_gaussian_ply(m, sep)["separate"] and torch.equal(m.loaded["opacities_thermal"], p["opacities_thermal"])
    with pytest.raises(ValueError, match="opacity_thermal"):
        splat_io.load_gaussian_ply(_Model(3, False), sep)
    with pytest.raises(ValueError, match="sh_degree 1"):
        splat_io.load_gaussian_ply(_Model(1, True), sep)
    with pytest.raises(ValueError, match="degree-0"):
        splat_io.load_gaussian_ply(_Model(0, True), sep)
    # a shared file into a separate model: no opacities_thermal in what load_gaussians receives (its rule copies the opacities)
    rows, _ = sxf.pack_ref(ssf.shared_params(p), "both")
    shared = splat_io.write_gaussian_ply(str(tmp_path / "shared.ply"), rows.numpy(), splat_io.ply_properties("both", 16, False))
    m = _Model(3, True)
    assert not splat_io.load_gaussian_ply(m, shared)["separate"] and "opacities_thermal" not in m.loaded


def test_opacity_logit():
    assert splat_io.opacity_logit(0.0) == -math.inf
    assert splat_io.opacity_logit(0.5) == 0.0
    assert splat_io.opacity_logit(0.005) == float(np.float32(math.log(0.005 / 0.995)))
    for bad in (-0.1, 1.0, 2.0, float("nan")):
        with pytest.raises(ValueError):
            splat_io.opacity_logit(bad)


# ---------------------------------------------------------------------------------------------------- 5. zero vertices
@pytest.mark.parametrize("separate", [False, True], ids=["shared", "separate"])
def test_a_zero_vertex_file_round_trips(tmp_path, separate):
    props = splat_io.ply_properties("both", 16, separate)
    path = splat_io.write_gaussian_ply(str(tmp_path / "empty.ply"), np.zeros((0, len(props)), np.float32), props)
    assert b"element vertex 0\n" in open(path, "rb").read() and open(path, "rb").read().endswith(b"end_header\n")
    p, info = splat_io.read_gaussian_ply(path)
    assert info["num_gaussians"] == 0 and info["K"] == 16 and info["separate"] == separate
    assert p["means"].shape == (0, 3) and p["features_rest"].shape == (0, 15, 3) and p["features_rest_thermal"].shape == (0, 15, 1)
    assert ("opacities_thermal" in p) == separate


# ---------------------------------------------------------------------------------------------------- the entry point, before any launch
def test_the_header_declares_the_export_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "thermal_nerf_hip.h")).read()
    assert "TN_API int tn_export_splat_pack(" in hdr and "TN_API int64_t tn_export_splat_workspace_bytes(int64_t num_gaussians);" in hdr
    assert len(_lib.SIGNATURES["tn_export_splat_pack"][1]) == 20 and _lib.SIGNATURES["tn_export_splat_pack"][1][13] is C.c_float


def test_the_library_refuses_bad_export_arguments_before_any_launch():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = _lib.load()
    assert lib.tn_export_splat_workspace_bytes(-1) == -1 and lib.tn_export_splat_workspace_bytes(1 << 31) == -1
    assert lib.tn_export_splat_workspace_bytes(0) == 0
    need = lib.tn_export_splat_workspace_bytes(1000)
    assert need >= 1000 + 4 * 4 + 4 * 8 and lib.tn_export_splat_workspace_bytes((1 << 31) - 1) > (1 << 31)
    fake = C.c_void_p(256 * 4096)  # aligned, non-null, never dereferenced
    ten = [fake] * 9
    inf = -math.inf

    def call(ptrs=ten, n=1000, R=15, spectrum=2, colour=0, thr=inf, out=fake, count=fake, ws=fake, ws_bytes=need):
        return lib.tn_export_splat_pack(*ptrs, n, R, spectrum, colour, thr, None, out, count, ws, ws_bytes, None)

    assert call(ptrs=[None] * 9) == -22 and b"null pointer" in lib.tn_last_error()
    for i in range(8):  # each of the eight required tensors; opacities_thermal (the ninth) may be null: shared mode
        assert call(ptrs=[None if j == i else fake for j in range(9)]) == -22, i
    assert call(out=None) == -22 and call(count=None) == -22 and call(ws=None) == -22
    assert call(n=-1) == -22 and b"Gaussians" in lib.tn_last_error()
    assert call(n=1 << 31) == -22
    assert call(R=-1) == -22 and b"rest coefficients" in lib.tn_last_error()
    assert call(spectrum=3) == -22 and b"spectrum" in lib.tn_last_error()
    assert call(spectrum=-1) == -22
    assert call(colour=2) == -22 and b"colour_mode" in lib.tn_last_error()
    assert call(colour=1, R=15) == -22 and b"no f_rest columns" in lib.tn_last_error()
    assert call(thr=float("nan")) == -22
    assert call(ws_bytes=need - 1) == -22 and b"workspace of" in lib.tn_last_error()
    assert call(ws=C.c_void_p(256 * 4096 + 4)) == -22 and b"aligned" in lib.tn_last_error()
    # the rest tensors may be null without rest coefficients -- then the first thing refused is the short workspace
    assert call(ptrs=[fake] * 5 + [None, fake, None, None], R=0, ws_bytes=0) == -22 and b"workspace of" in lib.tn_last_error()


# ---------------------------------------------------------------------------------------------------- 6. the inputs of the GPU tests
@pytest.mark.parametrize("d", [0, 3])
def test_the_gpu_inputs_meet_their_conditions(d):
    """Exact keep sets need every mean outside the rounding band of the boxes' faces (so the kernel's fp32 test, its restatement here and the
    float64 rule agree); the degree-0 tolerance is derived for colours inside [0.02, 0.98]."""
    p = scf.crop_scene(0, d)
    for box in (scf.MAIN_BOX, scf.SECOND_BOX):
        assert int(scf.near_boundary(box, p["means"]).sum()) == 0
        assert torch.equal(sxf.in_box_fp32(box, p["means"]), scf.within64(box, p["means"]))
        kept = int(scf.within64(box, p["means"]).sum())
        assert 40 < kept < 260
    for k, v in p.items():
        assert bool(torch.isfinite(v).all()), k
    if d == 0:
        for k in ("features_dc", "features_dc_thermal"):
            c = torch.sigmoid(p[k].double())
            assert 0.02 <= float(c.min()) and float(c.max()) <= 0.98, (k, float(c.min()), float(c.max()))


def test_pack_ref_drops_what_the_rule_says():
    """The restatement against the rule spelled out by hand on a small case: a defect in a thermal-only attribute leaves the rgb row, a defect in
    an RGB-only attribute leaves the thermal row, `both` in separate mode keeps by the larger logit."""
    p = sxf.random_params(12, 4, True, 0)
    p["features_rest_thermal"][3, 1, 0] = float("nan")
    p["features_rest"][4, 2, 1] = float("inf")
    p["means"][5, 0] = float("-inf")
    p["opacities"][6, 0], p["opacities_thermal"][6, 0] = -9.0, 1.0
    p["opacities"][7, 0], p["opacities_thermal"][7, 0] = 1.0, -9.0
    p["opacities"][8, 0], p["opacities_thermal"][8, 0] = -9.0, -8.0
    for k in ("opacities", "opacities_thermal"):
        for g in (0, 1, 2, 3, 4, 5, 9, 10, 11):
            p[k][g, 0] = 0.5
    every = set(range(12))
    kept = lambda s, thr=-math.inf: set(sxf.pack_ref(p, s, 0, thr)[1].tolist())  # noqa: E731
    assert kept("rgb") == every - {4, 5} and kept("thermal") == every - {3, 5} and kept("both") == every - {3, 4, 5}
    assert kept("rgb", 0.0) == every - {4, 5, 6, 8} and kept("thermal", 0.0) == every - {3, 5, 7, 8} and kept("both", 0.0) == every - {3, 4, 5, 8}
    rows, idx = sxf.pack_ref(p, "both")
    assert rows.shape == (9, 14 + 3 * 4 + 4 + 1)
    g = int(idx[0])
    assert rows[0, 9 + 1 * 3 + 2] == p["features_rest"][g, 2, 1] and rows[0, -1] == p["opacities_thermal"][g, 0] and rows[0, 18] == p["opacities"][g, 0]
    assert struct.pack("<f", float(rows[0, 3])) == b"\0\0\0\0"
