"""The splat path's undistortion on the GPU: tn_image_undistort against the float64 restatement (undistort_functional.py) with the float32 run of
the same formulas as the floor, its geometry against the ray generator's own Newton (tn_raygen), the identities, and
ThermalFullImageDatamanager on a small RGB+T dataset, through to one training step per spectrum.

Every case prints its floor and the kernel's error; profiles/splat_undistort.md records them."""
import math

import numpy as np
import pytest
import torch

import undistort_functional as uf

pytestmark = pytest.mark.gpu
DEV = "cuda"
FOV = 0.9375  # focal length / width of synth.synth_cameras
SHAPES = ((37, 53), (48, 64))  # H x W: odd sides below one 64-pixel wave, and a full wave with several 4-row blocks


def _splat():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import splat

    return splat


def _camera(W, H, f=None):
    splat = _splat()
    f = FOV * W if f is None else f
    return splat.PinholeCamera(torch.eye(4)[:3], f, f, W / 2, H / 2, W, H)


def _intr(cam):
    return (cam.fx, cam.fy, cam.cx, cam.cy)


def _check(image: np.ndarray, view, cam, new, k, label: str):
    """One input (numpy [H,W,C] uint8 or float32; `view` = the device tensor the kernel reads, possibly strided) in both output types against the
    float64 restatement; returns (floor, e_hip)."""
    splat = _splat()
    H, W = image.shape[:2]
    want = uf.undistort(image, _intr(cam), k, _intr(new))
    floor = float(np.abs(uf.undistort(image, _intr(cam), k, _intr(new), dtype=np.float32).astype(np.float64) - want).max())
    bound = 8 * floor
    got, cam_out = splat.undistort_image(view, cam, k, new_camera=new, out_dtype=torch.float32)
    assert cam_out is new and got.shape == image.shape and got.dtype == torch.float32 and got.is_contiguous()
    e_hip = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"{label}: floor (float32 restatement) = {floor:.3e}, e_hip = {e_hip:.3e}, bound = {bound:.3e}")
    assert floor > 0.0 and e_hip <= bound, (e_hip, floor)
    got8, _ = splat.undistort_image(view, cam, k, new_camera=new, out_dtype=torch.uint8)
    assert got8.dtype == torch.uint8 and got8.shape == image.shape and got8.is_contiguous()
    want8 = uf.to_u8(want).astype(np.int64)
    diff = got8.cpu().numpy().astype(np.int64) - want8
    assert np.abs(diff).max() <= 1
    scaled = want[diff != 0] * 255.0
    off_half = np.abs(scaled - np.floor(scaled) - 0.5)
    print(f"{label}: uint8 output, {int((diff != 0).sum())} of {diff.size} values one level off"
          + (f", at most {off_half.max():.3e} levels from a half" if off_half.size else ""))
    assert np.all(off_half <= 255.0 * bound)  # only values the fp32 bound cannot tell from a tie may round the other way
    return floor, e_hip


# ------------------------------------------------------------------------------------------------ the kernel against the restatement
@pytest.mark.parametrize("name", sorted(uf.SETS))
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_against_the_restatement(H, W, channels, name):
    splat = _splat()
    k = uf.SETS[name]
    cam = _camera(W, H)
    new = splat.undistorted_camera(cam, k)
    for u8 in (False, True):
        image = uf.random_image(H, W, channels, seed=H + channels, u8=u8)
        _check(image, torch.from_numpy(image).to(DEV), cam, new, k, f"{name} {H}x{W}x{channels} {'uint8' if u8 else 'fp32'} input")


@pytest.mark.parametrize("name", sorted(uf.SETS))
@pytest.mark.parametrize("H,W", SHAPES)
def test_views_of_an_rgbt_buffer_are_read_in_place(H, W, name):
    splat = _splat()
    k = uf.SETS[name]
    cam = _camera(W, H)
    new = splat.undistorted_camera(cam, k)
    for u8 in (False, True):
        image = uf.random_image(H, W, 4, seed=7, u8=u8)
        buf = torch.from_numpy(image).to(DEV)
        for sl in (slice(0, 3), slice(3, 4)):
            view = buf[..., sl]
            assert view.stride(1) == 4 and not (view.is_contiguous() and sl.stop - sl.start > 1)
            _check(np.ascontiguousarray(image[..., sl]), view, cam, new, k, f"{name} {H}x{W} [..., {sl.start}:{sl.stop}] of {'uint8' if u8 else 'fp32'} RGBT")
            for dt in (torch.float32, torch.uint8):
                assert torch.equal(splat.undistort_image(view, cam, k, new, dt)[0], splat.undistort_image(view.contiguous(), cam, k, new, dt)[0])


# ------------------------------------------------------------------------------------------------ geometry against the ray generator
def _g(x, y):
    """A smooth low-frequency pattern of the undistorted normalised coordinates, three channels in [0, 1]."""
    return np.stack([0.5 + 0.25 * np.sin(2.0 * x + 0.3 + c) + 0.25 * np.cos(3.0 * y - 0.2 * c) for c in range(3)], axis=-1)


@pytest.mark.parametrize("name", ["synth_rgb", "synth_thermal"])
def test_geometry_against_the_ray_generator(name):
    from nerfstudio_thermal_amd import ops

    splat = _splat()
    W, H, f = 64, 48, 60.0
    k = uf.SETS[name]
    cam = _camera(W, H, f)
    v, u = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    idx = torch.stack([torch.zeros_like(u), v, u], dim=-1).reshape(-1, 3).to(DEV)
    one = lambda val: torch.tensor([val], device=DEV)  # noqa: E731
    c2w = torch.eye(4)[:3].reshape(1, 3, 4).contiguous().to(DEV)
    _, d, _, _ = ops.raygen(idx, c2w, one(f), one(f), one(W / 2), one(H / 2), torch.tensor([k], device=DEV))
    d = d.cpu().numpy().astype(np.float64).reshape(H, W, 3)
    # identity pose: direction = normalise(x, -y, -1) of the pixel's undistorted coordinates (tn_raygen's own fp32 Newton)
    x, y = d[..., 0] / -d[..., 2], d[..., 1] / d[..., 2]
    image = _g(x, y).astype(np.float32)  # the distorted frame: what a camera with this distortion records of the pattern
    new = splat.undistorted_camera(cam, k)
    nu, nv = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    truth = _g((nu - new.cx) / new.fx, (nv - new.cy) / new.fy)  # the pattern as the new pinhole camera sees it
    want = uf.undistort(image, _intr(cam), k, _intr(new))
    floor = float(np.abs(uf.undistort(image, _intr(cam), k, _intr(new), dtype=np.float32).astype(np.float64) - want).max())
    e_interp = float(np.abs(want - truth).max())  # the restatement's own error: bilinear interpolation of the pattern
    got, _ = splat.undistort_image(torch.from_numpy(image).to(DEV), cam, k, new)
    e_hip = float(np.abs(got.cpu().numpy().astype(np.float64) - truth).max())
    e_raw = float(np.abs(image.astype(np.float64) - truth).max())  # today's behaviour: the frame passed through, the camera kept
    bound = e_interp + 8 * floor + 1e-5
    print(f"{name}: e_interp = {e_interp:.3e}, fp32 floor = {floor:.3e}, e_hip = {e_hip:.3e} (bound {bound:.3e}), untouched frame = {e_raw:.3e}")
    assert e_hip <= bound, (e_hip, bound)
    assert e_raw > 10 * bound, (e_raw, bound)  # the untouched frame misses by a wide margin: the check is not vacuous


# ------------------------------------------------------------------------------------------------ identities
def test_zero_distortion_returns_the_inputs_themselves():
    splat = _splat()
    cam = _camera(64, 48)
    for img in (torch.rand(48, 64, 3, device=DEV), torch.zeros(48, 64, 4, dtype=torch.uint8, device=DEV)):
        out, cam_out = splat.undistort_image(img, cam, torch.zeros(6))
        assert out is img and cam_out is cam
    with pytest.raises(ValueError, match="48 x 64"):
        splat.undistort_image(torch.rand(48, 63, 3, device=DEV), cam, uf.SYNTH_RGB)
    with pytest.raises(ValueError):
        splat.undistort_image(torch.rand(48, 64, 5, device=DEV), cam, uf.SYNTH_RGB)
    with pytest.raises(ValueError, match="out_dtype"):
        splat.undistort_image(torch.rand(48, 64, 3, device=DEV), cam, uf.SYNTH_RGB, out_dtype=torch.float16)


def test_a_vanishing_distortion_leaves_a_uint8_frame_unchanged():
    splat = _splat()
    cam = _camera(64, 48)
    u8 = torch.from_numpy(uf.random_image(48, 64, 3, seed=11, u8=True)).to(DEV)
    keep = u8.clone()
    out, new = splat.undistort_image(u8, cam, [1e-12] * 6)
    assert out is not u8 and new is not cam and out.dtype == torch.uint8
    assert torch.equal(out, keep) and torch.equal(u8, keep)
    again, _ = splat.undistort_image(u8, cam, [1e-12] * 6)
    assert torch.equal(out, again)


# ------------------------------------------------------------------------------------------------ the datamanager
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """2 + 2 frames, RGB 64 x 48 and thermal 32 x 24, synth.synth_cameras' distortions, written by the package's dataset writer."""
    from nerfstudio_thermal_amd import synth
    from nerfstudio_thermal_amd.dataparser import write_rgbt_dataset

    cams = synth.synth_cameras(2, 2)
    th = cams["is_thermal"] == 1
    cams["width"], cams["height"] = np.where(th, 32, 64), np.where(th, 24, 48)
    cams["fx"] = cams["fy"] = np.where(th, 30.0, 60.0).astype(np.float32)
    cams["cx"], cams["cy"] = (cams["width"] / 2).astype(np.float32), (cams["height"] / 2).astype(np.float32)
    images = [uf.random_image(int(h), int(w), 3, seed=20 + i) for i, (h, w) in enumerate(zip(cams["height"], cams["width"]))]
    out = tmp_path_factory.mktemp("rgbt")
    write_rgbt_dataset(str(out), cams, images)
    return str(out)


def _manager(data, **kw):
    from nerfstudio_thermal_amd import ThermalFullImageDatamanagerConfig
    from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig

    # half of each spectrum's two frames trains, the other is held out
    return ThermalFullImageDatamanagerConfig(dataparser=ThermalNerfDataParserConfig(data=data, train_split_fraction=0.5), **kw).setup(device=DEV)


@pytest.mark.parametrize("cache", ["uint8", "float32"])
def test_datamanager_caches_the_undistorted_frames(dataset, cache):
    from nerfstudio_thermal_amd.dataparser import load_image_float32, load_image_uint8
    from nerfstudio_thermal_amd.splat_datamanager import parsed_camera

    splat = _splat()
    dm = _manager(dataset, cache_images_type=cache)
    load, dtype = (load_image_uint8, torch.uint8) if cache == "uint8" else (load_image_float32, torch.float32)
    assert dm.num_train_data == 2 and len(dm.cached_eval) == 2
    for cached, cameras, parsed in ((dm.cached_train, dm.train_cameras, dm.train_dataparser_outputs),
                                    (dm.cached_eval, dm.eval_cameras, dm.eval_dataparser_outputs)):
        assert sorted(b["is_thermal"] for b in cached) == [False, True]
        for i, (batch, cam) in enumerate(zip(cached, cameras)):
            raw_cam, k = parsed_camera(parsed, i), parsed.cameras["distortion"][i]
            assert float(k.abs().max()) > 0
            want_cam = splat.undistorted_camera(raw_cam, k)
            assert _intr(cam) == _intr(want_cam) and (cam.width, cam.height) == (raw_cam.width, raw_cam.height) and cam.fx != raw_cam.fx
            assert torch.equal(cam.camera_to_world, raw_cam.camera_to_world)
            want, _ = splat.undistort_image(load(parsed.image_filenames[i]).to(DEV), raw_cam, k)
            assert batch["image"].dtype == dtype and batch["image"].is_cuda and torch.equal(batch["image"], want)
            assert (batch["image"].shape[1], batch["image"].shape[0]) == ((32, 24) if batch["is_thermal"] else (64, 48)) and batch["image_idx"] == i
    evals = dm.fixed_indices_eval_dataloader
    assert [b["image_idx"] for _, b in evals] == [0, 1] and all(c is dm.eval_cameras[b["image_idx"]] for c, b in evals)
    assert all(torch.equal(b["image"], dm.cached_eval[b["image_idx"]]["image"]) for _, b in evals)


def test_datamanager_without_undistortion_serves_the_files(dataset):
    from nerfstudio_thermal_amd.dataparser import load_image_uint8
    from nerfstudio_thermal_amd.splat_datamanager import parsed_camera

    dm = _manager(dataset, undistort=False)
    for i, (batch, cam) in enumerate(zip(dm.cached_train, dm.train_cameras)):
        assert torch.equal(batch["image"].cpu(), load_image_uint8(dm.train_dataparser_outputs.image_filenames[i]))
        assert _intr(cam) == _intr(parsed_camera(dm.train_dataparser_outputs, i))


def test_datamanager_batches_train_the_model(dataset):
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

    dm = _manager(dataset)
    model = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(random_scale=1.0), num_points=200, device=DEV, seed=1, num_train_data=dm.num_train_data)
    seen = set()
    for step in range(dm.num_train_data):
        cam, batch = dm.next_train(step)
        assert set(batch) == {"image", "is_thermal", "image_idx"} and batch["image"].dtype == torch.uint8
        assert dm.get_train_rays_per_batch() == cam.width * cam.height
        seen.add(batch["is_thermal"])
        model.zero_grad(set_to_none=True)
        loss = model.get_loss_dict(model.get_train_outputs(cam), batch)
        sum(loss.values()).backward()
        assert math.isfinite(float(loss["main_loss"]))
        grads = [p.grad for p in model.gauss_params.values()]
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
        key = "features_dc_thermal" if batch["is_thermal"] else "features_dc"
        assert float(model.gauss_params[key].grad.abs().max()) > 0.0
    assert seen == {False, True}  # one RGB and one thermal batch
    model.eval()
    with torch.no_grad():
        for cam, batch in dm.fixed_indices_eval_dataloader:
            metrics, _ = model.get_image_metrics_and_images(model.get_outputs(cam), batch)
            assert all(math.isfinite(v) for v in metrics.values())
