"""Frame rendering without a GPU: the torch restatement of the colour-map rule (render_functional) against the reference's recorded outputs
(tests/golden/render_reference.npz, scripts/make_golden_render.py) bit for bit, the finite-only min / max rule, the committed colour-map tables against
matplotlib, the float64 camera paths against the reference's recorded float64 results within a derived bound, the JSON path and crop, and the
host-side argument checks of the entry points."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import render_functional as rf
from nerfstudio_thermal_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "render_reference.npz")
# The float64 paths against the reference's float64 results.  Both sides run the same formulas in IEEE double; what may differ is the last bit of a
# library call (sin, cos, acos, sqrt of a sum whose order a BLAS picks, the eigenvector routine) and how that travels: a pose entry is reached from the
# inputs in well under 64 operations of relative error 2^-53 each (quaternion from the eigenvector: ~10; slerp: ~12; quaternion to matrix: ~10; the
# spiral: 2 normalisations, 2 cross products and a 4-term dot product: ~30), on values of magnitude <= max(1, |value|).
PATH_TOL = 64 * 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def lut():
    return rf.tables()


def _render():
    from nerfstudio_thermal_amd import render

    return render


def _all_finite(c):
    return c["kind"] != "inf"


# ---------------------------------------------------------------------------------------------------- 1. the restatement and the reference
def test_golden_file_is_small_and_holds_the_cases(golden):
    assert os.path.getsize(GOLDEN) < 1 << 20
    for prefix, cases in (("cm", rf.colormap_cases()), ("dp", rf.depth_cases())):
        for i, c in enumerate(cases):
            image, acc = rf.case_inputs(c)
            key = rf.case_key(prefix, i)
            assert np.array_equal(golden[key + "_in"], image.numpy(), equal_nan=True), key  # the recorded inputs are the ones the cases make
            assert golden[key + "_out"].shape == (c["H"], c["W"], 3)
            if acc is not None:
                assert np.array_equal(golden[key + "_acc"], acc.numpy())
    kinds = {c["kind"] for c in rf.colormap_cases() + rf.depth_cases()}
    assert kinds == {"unit", "wide", "inf", "depth", "const"}
    assert {c["colormap"] for c in rf.colormap_cases()} == set(rf.COLORMAPS)


@pytest.mark.parametrize("prefix,cases", [("cm", rf.colormap_cases()), ("dp", rf.depth_cases())], ids=["apply_colormap", "apply_depth_colormap"])
def test_restatement_equals_the_reference_bit_for_bit(golden, lut, prefix, cases):
    """On all-finite frames every colour of the restatement is the reference's recorded one, bit for bit (apply_colormap: every colour map, normalize,
    invert, colormap_min / max, values on k / 255, at and just outside 0 and 1; apply_depth_colormap: planes given, absent and 0.0, accumulation
    exactly 0 and 1, a constant frame).  Frames with +-inf agree where no min / max is taken (normalize off, both planes given); where one is taken the
    finite-only rule differs on purpose and the case is not compared."""
    compared = 0
    for i, c in enumerate(cases):
        takes_minmax = c["normalize"] or ("near" in c and not (c["near"] and c["far"]))
        if not _all_finite(c) and takes_minmax:
            continue
        got = rf.case_colours(c, lut)
        want = torch.from_numpy(golden[rf.case_key(prefix, i) + "_out"])
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got, want), (rf.case_key(prefix, i), c, float((got - want).abs().max()))
        compared += 1
    assert compared >= len(cases) - 2


def test_inf_frames_are_among_the_compared_cases():
    cases = [c for c in rf.colormap_cases() + rf.depth_cases() if c["kind"] == "inf"]
    assert len(cases) == 6 and all(not c["normalize"] and ("near" not in c or (c["near"] and c["far"])) for c in cases)


def test_one_nan_follows_the_finite_only_rule(lut):
    """A frame with one NaN (and one +inf): min and max are those of the finite values, the NaN pixel becomes value 0 (row 0 of the table, or row 255
    inverted), every other pixel is what the same frame without the NaN gives.  torch.min would have made the whole frame NaN -> black."""
    x = rf.frame(5, 7, "depth")
    bad = x.clone()
    bad[2, 3, 0], bad[4, 1, 0] = float("nan"), float("inf")
    mn, mx = rf.finite_minmax(bad)
    keep = torch.ones(5, 7, dtype=torch.bool)
    keep[2, 3] = keep[4, 1] = False
    assert float(mn) == float(x[keep].min()) and float(mx) == float(x[keep].max())
    got = rf.colours(bad, "turbo", normalize=True, lut=lut)
    clean = x.clone()
    clean[2, 3, 0], clean[4, 1, 0] = mn, mx  # values that leave min and max where they are
    want = rf.colours(clean, "turbo", normalize=True, lut=lut)
    assert torch.equal(got[keep], want[keep])
    assert torch.equal(got[2, 3], lut["turbo"][0]) and torch.equal(got[4, 1], lut["turbo"][255])
    assert torch.equal(rf.colours(bad, "turbo", normalize=True, invert=True, lut=lut)[2, 3], lut["turbo"][0])  # NaN -> 0 comes after the inversion
    none = torch.full((3, 4, 1), float("nan"))
    assert [float(v) for v in rf.finite_minmax(none)] == [0.0, 0.0]
    assert torch.equal(rf.colours(none, "gray", normalize=True, lut=lut), torch.zeros(3, 4, 3))
    d = rf.colours(bad, "viridis", depth=True, accumulation=rf.accumulation(5, 7), lut=lut)
    assert bool(torch.isfinite(d).all())


def test_bytes_rule():
    c = torch.tensor([0.0, 1.0, 0.5, 0.99999994, -3.0, 7.0, float("nan"), float("inf"), 254.5 / 255, 127.5 / 255])
    want = [0, 255, 128, 255, 0, 255, 0, 255, int(np.float32(np.float32(254.5 / 255) * np.float32(255)) + np.float32(0.5)),
            int(np.float32(np.float32(127.5 / 255) * np.float32(255)) + np.float32(0.5))]
    assert rf.to_bytes(c).tolist() == want


def test_committed_tables_are_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    render = _render()
    names, luts = render.colormap_tables()
    assert names == ("turbo", "viridis", "magma", "inferno", "cividis", "gray") and luts.shape == (6, 256, 3) and luts.dtype == np.float32
    for name, table in zip(names, luts):
        cmap = matplotlib.colormaps[name]
        want = np.asarray(cmap.colors if hasattr(cmap, "colors") else cmap(np.arange(256))[:, :3], dtype=np.float64).astype(np.float32)
        assert np.array_equal(table, want), name
    assert os.path.getsize(render.LUT_PATH) < 1 << 17


def test_colormap_names_and_pca():
    render = _render()
    assert render.ColormapOptions() == render.ColormapOptions("default", False, 0, 1, False)
    assert render.COLORMAPS == ("default", "turbo", "viridis", "magma", "inferno", "cividis", "gray", "pca")
    with pytest.raises(NotImplementedError, match="pca"):
        render._check_colormap("pca")
    with pytest.raises(NotImplementedError, match="pca"):
        render.compose_frame({"rgb": torch.zeros(2, 2, 3)}, ["rgb"], render.ColormapOptions(colormap="pca"))
    with pytest.raises(ValueError):
        render._check_colormap("jet")
    with pytest.raises(KeyError, match=r"\['depth', 'rgb'\]"):
        render.compose_frame({"rgb": torch.zeros(2, 2, 3), "depth": torch.zeros(2, 2, 1), "background": torch.zeros(3)}, ["rgb", "normals"])
    with pytest.raises(ValueError, match="no CPU fallback"):
        render.apply_colormap(torch.zeros(2, 2, 1))


# ---------------------------------------------------------------------------------------------------- 2. camera paths
def _close64(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{what}: largest miss {err.max():.3g} (bound {PATH_TOL:.3g})")
    assert err.max() <= PATH_TOL, (what, err.max())


@pytest.mark.parametrize("n,steps,order", rf.PATH_CASES)
def test_interpolated_poses_against_the_float64_reference(golden, n, steps, order):
    """interpolated_poses_many in float64 against the reference's float64 parts (get_ordered_poses_and_k, get_interpolated_poses,
    get_interpolated_k), and, rounded to float32, against what get_interpolated_poses_many itself returns (it rounds to float32 at its end): two
    doubles within PATH_TOL round to the same float32 or to neighbours, so at most one float32 spacing."""
    render = _render()
    poses, Ks = rf.random_poses(n, seed=10 * n + steps)
    got_p, got_k = render.interpolated_poses_many(poses, Ks, steps, order)
    key = f"path_f64_n{n}_s{steps}_o{int(order)}"
    assert got_p.dtype == np.float64 and got_p.shape == ((n - 1) * steps, 3, 4) and got_k.shape == ((n - 1) * steps, 3, 3)
    _close64(got_p, golden[key + "_poses"], key + " poses")
    _close64(got_k, golden[key + "_Ks"], key + " Ks")
    for got, want in ((got_p, golden[key + "_many_poses"]), (got_k, golden[key + "_many_Ks"])):
        assert want.dtype == np.float32
        assert np.all(np.abs(got.astype(np.float32) - want) <= np.spacing(np.abs(want))), key


def test_ordering_is_the_reference_greedy_one():
    render = _render()
    poses = np.tile(np.eye(3, 4), (5, 1, 1))
    poses[:, 0, 3] = [0.0, 5.0, 1.0, 1.0, 3.0]  # from 0: the nearest is 1.0 (the first of the two equals: index 2), then 3, then 4, then 1
    Ks = np.tile(np.eye(3), (5, 1, 1)) * np.arange(1, 6)[:, None, None]
    op, ok = render.ordered_poses(poses, Ks)
    assert op[:, 0, 3].tolist() == [0.0, 1.0, 1.0, 3.0, 5.0] and ok[:, 0, 0].tolist() == [1.0, 3.0, 4.0, 5.0, 2.0]


def _cam(render, pose, K, W=640, H=480):
    return render.PinholeCamera(torch.from_numpy(np.asarray(pose, dtype=np.float64)), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), W, H)


def test_interpolated_path_returns_cameras(golden):
    render = _render()
    poses, Ks = rf.random_poses(3, seed=34)
    cams = render.interpolated_path([_cam(render, p, K) for p, K in zip(poses, Ks)], 4, order_poses=True)
    key = "path_f64_n3_s4_o1"
    assert len(cams) == 8 and all(isinstance(c, render.PinholeCamera) and (c.width, c.height, c.cx, c.cy) == (640, 480, 320.0, 240.0) for c in cams)
    _close64(np.stack([c.camera_to_world.numpy() for c in cams]), golden[key + "_poses"], "interpolated_path poses")
    _close64([c.fx for c in cams], golden[key + "_Ks"][:, 0, 0], "interpolated_path fx")
    _close64([c.fy for c in cams], golden[key + "_Ks"][:, 1, 1], "interpolated_path fy")


@pytest.mark.parametrize("i", range(len(rf.SPIRAL_CASES)))
def test_spiral_path_against_the_float64_reference(golden, i):
    render = _render()
    s = rf.SPIRAL_CASES[i]
    cam = _cam(render, golden["spiral_base_pose"][0], golden["spiral_base_K"][0])
    cams = render.spiral_path(cam, steps=s["steps"], radius=s["radius"], radiuses=s["radiuses"], rots=s["rots"], zrate=s["zrate"])
    assert len(cams) == s["steps"]
    _close64(np.stack([c.camera_to_world.numpy() for c in cams]), golden[f"spiral_f64_{i}_poses"], f"spiral {i}")
    assert [cams[0].fx, cams[0].fy, cams[0].cx, cams[0].cy] == golden[f"spiral_f64_{i}_fxfycxcy"].tolist()
    with pytest.raises(ValueError):
        render.spiral_path(cam, radius=1.0, radiuses=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        render.spiral_path(cam)


def test_path_and_crop_from_json_equal_the_reference(golden):
    render = _render()
    cams = render.path_from_json(rf.CAMERA_PATH_JSON)
    assert len(cams) == 3 and all(isinstance(c, render.PinholeCamera) for c in cams)
    assert np.array_equal(np.stack([c.camera_to_world.numpy() for c in cams]), golden["json_f64_poses"])
    assert np.array_equal(np.array([[c.fx, c.fy, c.cx, c.cy] for c in cams]), golden["json_f64_fxfycxcy"])
    assert [(c.width, c.height) for c in cams] == [tuple(golden["json_f64_size"].tolist())] * 3
    box, background = render.crop_from_json(rf.CAMERA_PATH_JSON)
    assert isinstance(box, render.OrientedBox)
    assert np.array_equal(box.R.numpy(), golden["crop_R"].astype(np.float32))  # (the golden's rotation is not viser's: scripts/make_golden_render.py)
    assert np.array_equal(box.T.numpy(), golden["crop_T"].astype(np.float32)) and np.array_equal(box.S.numpy(), golden["crop_S"].astype(np.float32))
    assert np.array_equal(background.numpy(), golden["crop_background"])
    assert render.crop_from_json({"camera_path": []}) is None and render.crop_from_json({"crop": None}) is None
    no_rot = {"crop": {k: v for k, v in rf.CAMERA_PATH_JSON["crop"].items() if k != "crop_rot"}}
    assert torch.equal(render.crop_from_json(no_rot)[0].R, torch.eye(3))


@pytest.mark.parametrize("kind", ["fisheye", "equirectangular", "omnidirectional", "VR180"])
def test_non_perspective_paths_raise(kind):
    with pytest.raises(NotImplementedError, match="perspective"):
        _render().path_from_json({**rf.CAMERA_PATH_JSON, "camera_type": kind})
    assert len(_render().path_from_json({**rf.CAMERA_PATH_JSON, "camera_type": "perspective"})) == 3


def test_float32_reference_distance_is_reported(golden):
    """For information (profiles/render.md): how far the reference's float32 results are from its float64 ones."""
    for name in ("spiral_{}_0_poses", "spiral_{}_1_poses", "json_{}_poses", "json_{}_fxfycxcy"):
        print(name.format("f32"), float(np.abs(golden[name.format("f32")] - golden[name.format("f64")]).max()))
    worst = max(float(np.abs(golden[k].astype(np.float64) - golden[k.replace("_many_", "_")]).max()) for k in golden if k.startswith("path_f64") and "_many_" in k)
    print("get_interpolated_poses_many (float32 result) vs its float64 parts:", worst)
    assert any("path_f32" in str(n) for n in golden["notes"])  # the reference's interpolation does not run on float32 poses under this numpy


# ---------------------------------------------------------------------------------------------------- 3. host-side validation
def _record(ptr, channels=1, flags=0, minmax=None, table=None, acc=None):
    r = _lib.TnFramePanel()
    r.src, r.channels, r.flags, r.minmax, r.table, r.accumulation = ptr, channels, flags, minmax, table, acc
    r.colormap_max = 1.0
    return r


def test_entry_points_validate_on_the_host(lib):
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p).value
    err = lambda: lib.tn_last_error().decode()  # noqa: E731
    ws = _lib.TN_FRAME_MINMAX_WORKSPACE_BYTES
    assert lib.tn_frame_minmax(None, 4, ptr, ptr, ws, None) == -22 and "null pointer" in err()
    assert lib.tn_frame_minmax(ptr, 4, None, ptr, ws, None) == -22 and "null pointer" in err()
    assert lib.tn_frame_minmax(ptr, 4, ptr, None, ws, None) == -22 and "null pointer" in err()
    assert lib.tn_frame_minmax(ptr, 0, ptr, ptr, ws, None) == -22 and "at least 1" in err()
    assert lib.tn_frame_minmax(ptr, 4, ptr, ptr, ws - 1, None) == -22 and "workspace of" in err()
    assert lib.tn_frame_minmax(ptr + 1, 4, ptr, ptr, ws, None) == -22 and "misaligned" in err()

    def compose(records, n=None, H=2, W=2, out=ptr):
        arr = (_lib.TnFramePanel * max(len(records), 1))(*records)
        return lib.tn_frame_compose(arr, len(records) if n is None else n, H, W, out, None)

    ok = _record(ptr, 3)
    assert lib.tn_frame_compose(None, 1, 2, 2, ptr, None) == -22 and "null pointer (panels)" in err()
    assert compose([ok], n=0) == -22 and "0 panels (1..8)" in err()
    assert compose([ok] * 9) == -22 and "9 panels (1..8)" in err()
    assert compose([ok], H=0) == -22 and "positive" in err()
    assert compose([ok], W=-3) == -22 and "positive" in err()
    assert compose([ok], H=1 << 15, W=1 << 15) == -22 and "2^31" in err()
    assert compose([ok], out=None) == -22 and "null pointer (out_u8)" in err()
    assert compose([_record(ptr, 2)]) == -22 and "2 channels (1 or 3)" in err()
    assert compose([ok, _record(ptr, 4)]) == -22 and "panel 1 has 4 channels" in err()
    assert compose([_record(None, 1)]) == -22 and "null pointer (source of panel 0)" in err()
    assert compose([_record(ptr, 1, flags=_lib.TN_FRAME_NORMALIZE)]) == -22 and "has no min / max" in err()
    assert compose([_record(ptr, 1, flags=_lib.TN_FRAME_DEPTH | _lib.TN_FRAME_NEAR)]) == -22 and "has no min / max" in err()
    assert compose([_record(ptr, 1, table=ptr + 2)]) == -22 and "misaligned" in err()
    one = _record(ptr, 1)
    assert lib.tn_frame_colors(None, 2, 2, ptr, None) == -22 and "null pointer" in err()
    assert lib.tn_frame_colors(C.byref(one), 2, 2, None, None) == -22 and "out_rgb" in err()
    assert lib.tn_frame_colors(C.byref(_record(ptr, 5)), 2, 2, ptr, None) == -22 and "5 channels" in err()


def test_panel_record_matches_the_header(tmp_path):
    """The ctypes mirror of TnFramePanel against the C compiler's layout, and the constants against the header's."""
    import re
    import shutil
    import subprocess

    hdr_path = os.path.join(ROOT, "include", "thermal_nerf_hip.h")
    hdr = open(hdr_path).read()
    for name in ("TN_FRAME_MAX_PANELS", "TN_FRAME_MINMAX_WORKSPACE_BYTES", "TN_FRAME_NORMALIZE", "TN_FRAME_INVERT", "TN_FRAME_DEPTH", "TN_FRAME_NEAR",
                 "TN_FRAME_FAR"):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == getattr(_lib, name), name
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    names = [f[0] for f in _lib.TnFramePanel._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n  printf("%%zu\\n", sizeof(TnFramePanel));\n%s  return 0;\n}\n'
                   % (hdr_path, "".join('  printf("%s %%zu\\n", offsetof(TnFramePanel, %s));\n' % (n, n) for n in names)))
    subprocess.run(["gcc", "-o", str(tmp_path / "layout"), str(src)], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == C.sizeof(_lib.TnFramePanel)
    assert {out[i]: int(out[i + 1]) for i in range(1, len(out), 2)} == {n: getattr(_lib.TnFramePanel, n).offset for n in names}
