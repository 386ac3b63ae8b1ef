"""The splat path's undistortion without a GPU: the float64 restatement (undistort_functional.py) against an independent gather, the camera rule
(splat.undistorted_camera against the restatement and against its own guarantees), the C ABI of tn_image_undistort and its argument checks, and
the sampling order of ThermalFullImageDatamanager on raw frames."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib

import undistort_functional as uf

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((64, 48), (33, 21), (640, 480))  # W x H
FOV = 0.9375  # focal length / width of synth.synth_cameras (600 / 640, 150 / 160)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _camera(W, H, f=None, cx=None, cy=None):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    f = FOV * W if f is None else f
    return PinholeCamera(torch.eye(4)[:3], f, f, W / 2 if cx is None else cx, H / 2 if cy is None else cy, W, H)


def _intr(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_gather_is_scipys_linear_map_coordinates():
    """order=1, mode="nearest" reads the nearest edge value outside the frame: the clamped taps.  Both sides are float64 sums of at most four
    products of values in [0, 1] with weights in [0, 1], ordered differently: a few ulp of 1."""
    ndimage = pytest.importorskip("scipy.ndimage")
    H, W = 23, 31
    img = uf.random_image(H, W, 3, seed=1)
    rng = np.random.default_rng(2)
    sx, sy = rng.uniform(-1, W, (40, 50)), rng.uniform(-1, H, (40, 50))
    sx[0, :4], sy[0, :4] = (-1.0, 0.0, W - 1.0, float(W)), (-1.0, 0.0, H - 1.0, float(H))  # the corners and the clamp's ends
    got = uf.gather(img, sx, sy)
    for c in range(3):
        want = ndimage.map_coordinates(img[..., c].astype(np.float64), [sy, sx], order=1, mode="nearest")
        assert np.abs(got[..., c] - want).max() <= 8 * np.finfo(np.float64).eps
    # and at integer positions the image itself
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    assert np.array_equal(uf.gather(img, u, v), img.astype(np.float64))


def test_restatement_conversions():
    u8 = uf.random_image(5, 7, 2, seed=3, u8=True)
    assert uf.as_input(u8).dtype == np.float32 and np.array_equal(uf.as_input(u8), u8.astype(np.float32) / np.float32(255))
    assert np.array_equal(uf.to_u8(uf.as_input(u8).astype(np.float64)), u8)  # v / 255 rounds back to v
    assert uf.to_u8(np.array([-0.5, 0.0, 0.5 / 255, 1.5 / 255, 1.0, 7.0])).tolist() == [0, 0, 0, 2, 255, 255]  # clamp; halves go to even
    k = uf.SYNTH_RGB
    x, y = np.float64(0.3), np.float64(-0.2)
    r = x * x + y * y
    d = 1 + k[0] * r + k[1] * r * r
    xd, yd = uf.distort(x, y, k)
    assert abs(xd - (d * x + 2 * k[4] * x * y + k[5] * (r + 2 * x * x))) < 1e-15 and abs(yd - (d * y + 2 * k[5] * x * y + k[4] * (r + 2 * y * y))) < 1e-15


# ------------------------------------------------------------------------------------------------ the camera rule
@pytest.mark.parametrize("name", sorted(uf.SETS))
@pytest.mark.parametrize("W,H", SIZES)
def test_camera_rule(name, W, H):
    from nerfstudio_thermal_amd.splat import undistorted_camera

    k = uf.SETS[name]
    cam = _camera(W, H)
    # the set is invertible on the whole frame: Newton from every pixel centre comes back under the forward polynomial
    u, v = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    x, y, res = uf.undistort_points((u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy, k)
    assert res <= uf.NEWTON_TOL and np.all(np.diff(x, axis=1) > 0) and np.all(np.diff(y, axis=0) > 0)
    new = undistorted_camera(cam, k)
    assert new is not cam and (new.width, new.height) == (W, H) and new.camera_to_world is cam.camera_to_world
    assert (cam.fx, cam.fy, cam.cx, cam.cy) == (FOV * W, FOV * W, W / 2, H / 2)  # the input is untouched
    want = uf.new_intrinsics(_intr(cam), W, H, k)
    assert max(abs(a - b) for a, b in zip(_intr(new), want)) <= 1e-9 * new.fx  # two float64 evaluations of one rule
    sx, sy = uf.source_positions(_intr(cam), _intr(new), W, H, k, clamp=False)
    over = max(-sx.min(), sx.max() - (W - 1), -sy.min(), sy.max() - (H - 1))
    tight = [np.abs(sx[:, 0]).min(), np.abs(sx[:, -1] - (W - 1)).min(), np.abs(sy[0]).min(), np.abs(sy[-1] - (H - 1)).min()]
    print(f"{name} {W}x{H}: f {cam.fx:.4f} -> {new.fx:.4f}, {new.fy:.4f}, c -> {new.cx:.4f}, {new.cy:.4f}; reads {over:.2e} px beyond the frame, "
          f"nearest border pixel per side {max(tight):.2e} px off its edge")
    assert over <= 1e-6  # every output pixel reads inside the source frame
    assert max(tight) <= 1e-6  # and on every side one border pixel reads the very edge: the rectangle is tight


def test_camera_rule_off_centre_and_anisotropic():
    from nerfstudio_thermal_amd.splat import PinholeCamera, undistorted_camera

    cam = PinholeCamera(torch.eye(4)[:3], 71.0, 55.0, 29.25, 26.5, 64, 48)
    new = undistorted_camera(cam, torch.tensor(uf.STRONG))  # a float32 tensor, as the dataparser hands it over
    k32 = [float(np.float32(v)) for v in uf.STRONG]
    sx, sy = uf.source_positions(_intr(cam), _intr(new), 64, 48, k32, clamp=False)
    assert min(sx.min(), sy.min()) >= -1e-6 and sx.max() <= 63 + 1e-6 and sy.max() <= 47 + 1e-6
    assert _intr(new) == uf.new_intrinsics(_intr(cam), 64, 48, k32) or max(abs(a - b) for a, b in zip(_intr(new), uf.new_intrinsics(_intr(cam), 64, 48, k32))) <= 1e-7


def test_zero_distortion_returns_the_camera_itself():
    from nerfstudio_thermal_amd.splat import undistorted_camera

    cam = _camera(64, 48)
    for zero in ([0.0] * 6, torch.zeros(6), np.zeros(6, dtype=np.float32), (0, 0, 0, 0, 0, -0.0)):
        assert undistorted_camera(cam, zero) is cam


def test_camera_rule_refusals():
    from nerfstudio_thermal_amd.splat import undistorted_camera

    wide = _camera(640, 480, f=300.0)
    with pytest.raises(ValueError, match="cannot be inverted"):
        undistorted_camera(wide, (-5.0, 0, 0, 0, 0, 0))
    with pytest.raises(ValueError):
        uf.new_intrinsics(_intr(wide), 640, 480, (-5.0, 0, 0, 0, 0, 0))
    for bad in ((float("nan"), 0, 0, 0, 0, 0), (0, 0, 0, 0, float("inf"), 0)):
        with pytest.raises(ValueError, match="not finite"):
            undistorted_camera(wide, bad)
    with pytest.raises(ValueError, match="six coefficients"):
        undistorted_camera(wide, (0.1, 0.0, 0.0, 0.0))
    with pytest.raises(ValueError):  # the frame folds over inside the border: no rectangle, or no inverse
        undistorted_camera(wide, (-1.2, 0, 0, 0, 0, 0))


def test_undistort_image_refuses_cpu_tensors():
    from nerfstudio_thermal_amd.splat import undistort_image

    with pytest.raises(ValueError, match="no CPU fallback"):
        undistort_image(torch.zeros(48, 64, 3), _camera(64, 48), uf.SYNTH_RGB)
    with pytest.raises(ValueError, match="no CPU fallback"):
        undistort_image(torch.zeros(48, 64, 3, dtype=torch.uint8), _camera(64, 48), uf.SYNTH_RGB)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_binding_and_exports_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "thermal_nerf_hip.h")).read()
    assert "tn_image_undistort" in set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", hdr)) and "tn_image_undistort" in _lib.SIGNATURES
    assert _lib.ABI_VERSION == lib.tn_version()
    res, args = _lib.SIGNATURES["tn_image_undistort"]
    assert res is C.c_int and len(args) == 10 and args[8] is C.POINTER(_lib.TnUndistort) or args[8]._type_ is _lib.TnUndistort
    assert hasattr(lib, "tn_image_undistort")
    # the struct: fourteen floats in the header's order
    body = hdr[hdr.index("typedef struct TnUndistort {"):hdr.index("} TnUndistort;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct TnUndistort {", "")
    names = [re.sub(r"\[.*\]", "", n).strip() for stmt in body.split(";") if stmt.strip() for n in stmt.replace("float", "").split(",")]
    assert names == [f[0] for f in _lib.TnUndistort._fields_]
    assert C.sizeof(_lib.TnUndistort) == 14 * 4 and _lib.TnUndistort.k.offset == 32 and _lib.TnUndistort.new_fx.offset == 16


def _params(**kw):
    p = _lib.TnUndistort()
    p.fx = p.fy = p.new_fx = p.new_fy = 30.0
    p.cx = p.new_cx = 15.0
    p.cy = p.new_cy = 10.0
    for name, v in kw.items():
        if name == "k":
            for i, kv in enumerate(v):
                p.k[i] = kv
        else:
            setattr(p, name, v)
    return p


def test_image_undistort_argument_validation(lib):
    d = C.c_void_p(256)  # never dereferenced: every call below is refused before anything is read or launched

    def call(src=d, dtype=_lib.TN_IMAGE_F32, ps=3, H=20, W=30, c=3, out=d, odtype=_lib.TN_IMAGE_F32, params="default"):
        p = _params() if params == "default" else params
        return lib.tn_image_undistort(src, dtype, ps, H, W, c, out, odtype, C.byref(p) if p is not None else None, None)

    for kw in ({"src": None}, {"out": None}, {"params": None}):
        assert call(**kw) == EINVAL
        assert b"null pointer" in lib.tn_last_error()
    for bad in (2, -1):
        assert call(dtype=bad) == EINVAL
        assert b"input type" in lib.tn_last_error()
        assert call(odtype=bad) == EINVAL
        assert b"output type" in lib.tn_last_error()
    assert call(c=0) == EINVAL
    assert call(c=5, ps=5) == EINVAL
    assert b"channels" in lib.tn_last_error()
    assert call(ps=2) == EINVAL
    assert call(dtype=_lib.TN_IMAGE_U8, c=4, ps=3) == EINVAL
    assert b"pixel stride" in lib.tn_last_error()
    for kw in ({"H": 0}, {"W": 0}, {"H": -1}):
        assert call(**kw) == EINVAL
        assert b"positive" in lib.tn_last_error()
    for kw in ({"H": (1 << 15) + 1}, {"W": 1 << 16}):
        assert call(**kw) == EINVAL
        assert b"larger than" in lib.tn_last_error()
    for name in ("fx", "fy", "new_fx", "new_fy"):
        for v in (0.0, -30.0, float("nan"), float("inf")):
            assert call(params=_params(**{name: v})) == EINVAL
            assert b"focal lengths" in lib.tn_last_error()
    for kw in ({"cx": float("nan")}, {"new_cy": float("inf")}, {"k": (0, 0, float("nan"), 0, 0, 0)}, {"k": (0, 0, 0, 0, 0, float("-inf"))}):
        assert call(params=_params(**kw)) == EINVAL
        assert b"non-finite" in lib.tn_last_error()


# ------------------------------------------------------------------------------------------------ the datamanager's order
@pytest.fixture(scope="module")
def raw_dataset(tmp_path_factory):
    """7 + 7 frames of 16 x 12 (RGB) and 8 x 6 (thermal) with the synthetic distortions, written by the package's dataset writer."""
    from nerfstudio_thermal_amd import synth
    from nerfstudio_thermal_amd.dataparser import write_rgbt_dataset

    cams = synth.synth_cameras(7, 7)
    th = cams["is_thermal"] == 1
    cams["width"], cams["height"] = np.where(th, 8, 16), np.where(th, 6, 12)
    cams["fx"] = cams["fy"] = np.where(th, 7.5, 15.0).astype(np.float32)
    cams["cx"], cams["cy"] = (cams["width"] / 2).astype(np.float32), (cams["height"] / 2).astype(np.float32)
    rng = np.random.default_rng(0)
    images = [rng.random((int(h), int(w), 3), dtype=np.float32) for h, w in zip(cams["height"], cams["width"])]
    out = tmp_path_factory.mktemp("rgbt")
    write_rgbt_dataset(str(out), cams, images)
    return str(out)


def _manager(data, seed=0, **kw):
    from nerfstudio_thermal_amd import ThermalFullImageDatamanagerConfig
    from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig

    return ThermalFullImageDatamanagerConfig(dataparser=ThermalNerfDataParserConfig(data=data, train_split_fraction=0.7), undistort=False, seed=seed,
                                             **kw).setup(device="cpu")  # 5 of 7 frames per spectrum train, 2 are held out


def test_datamanager_config_defaults():
    from nerfstudio_thermal_amd import ThermalFullImageDatamanager, ThermalFullImageDatamanagerConfig
    from nerfstudio_thermal_amd.splat_datamanager import ThermalFullImageDatamanager as direct

    cfg = ThermalFullImageDatamanagerConfig()
    assert (cfg.cache_images_type, cfg.undistort, cfg.eval_split, cfg.seed) == ("uint8", True, "val", 0)
    assert ThermalFullImageDatamanager is direct
    with pytest.raises(ValueError, match="cache_images_type"):
        ThermalFullImageDatamanagerConfig(cache_images_type="float16")


def test_datamanager_serves_every_train_frame_once_per_epoch(raw_dataset):
    import random

    from nerfstudio_thermal_amd.dataparser import load_image_uint8

    state = random.getstate()
    dm = _manager(raw_dataset)
    n = dm.num_train_data
    assert n == len(dm.cached_train) == len(dm.train_cameras) == 14 - len(dm.cached_eval) and len(dm.cached_eval) >= 2
    assert dm.get_param_groups() == {} and dm.seed_points is None and dm.get_train_rays_per_batch() == 0
    parsed = dm.train_dataparser_outputs
    for epoch in range(3):
        seen = []
        for step in range(n):
            cam, batch = dm.next_train(epoch * n + step)
            i = batch["image_idx"]
            seen.append(i)
            assert set(batch) == {"image", "is_thermal", "image_idx"} and cam is dm.train_cameras[i]
            assert batch["is_thermal"] == bool(parsed.metadata["is_thermal"][i]) and batch["image"].dtype == torch.uint8
            assert torch.equal(batch["image"], load_image_uint8(parsed.image_filenames[i]))  # undistort=False: the file's pixels
            assert (cam.fx, cam.width, cam.height) == (float(parsed.cameras["fx"][i]), batch["image"].shape[1], batch["image"].shape[0])
            assert dm.get_train_rays_per_batch() == cam.width * cam.height
        assert sorted(seen) == list(range(n))
    assert random.getstate() == state  # the global generator is left alone
    evals = dm.fixed_indices_eval_dataloader
    assert [b["image_idx"] for _, b in evals] == list(range(len(dm.cached_eval)))
    seen = [dm.next_eval(0)[1]["image_idx"] for _ in range(len(evals))]
    assert sorted(seen) == list(range(len(evals)))
    assert dm.next_eval_image(0)[1]["image_idx"] in range(len(evals))


def test_datamanager_order_follows_the_seed(raw_dataset):
    def order(seed):
        dm = _manager(raw_dataset, seed=seed)
        return [dm.next_train(s)[1]["image_idx"] for s in range(3 * dm.num_train_data)]

    a, b, c = order(0), order(0), order(1)
    assert a == b and a != c


def test_datamanager_float32_cache_and_no_device_undistortion(raw_dataset):
    from nerfstudio_thermal_amd import ThermalFullImageDatamanagerConfig
    from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig, load_image_float32

    dm = _manager(raw_dataset, cache_images_type="float32")
    assert all(b["image"].dtype == torch.float32 for b in dm.cached_train + dm.cached_eval)
    assert torch.equal(dm.cached_train[0]["image"], load_image_float32(dm.train_dataparser_outputs.image_filenames[0]))
    with pytest.raises(ValueError, match="no CPU fallback"):  # undistortion is a device kernel; nothing quietly falls back
        ThermalFullImageDatamanagerConfig(dataparser=ThermalNerfDataParserConfig(data=raw_dataset)).setup(device="cpu")
