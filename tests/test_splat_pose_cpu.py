"""Pose refinement of the splat model without a GPU: the restatement the GPU tests compare against (tests/splat_pose_functional.py) is checked
against itself -- identity at the zero row, its float64 autograd pose gradient against central differences -- and the conditions the GPU tests'
scenes must meet (float32 floor, flagged pixels) are asserted here; then the host side of the feature: config validation, camera fields,
the pose optimiser's rows."""
import dataclasses

import pytest
import torch

import splat_backward_cases as bc
import splat_pose_functional as pf

FLOOR_CONFIGS = [("single", "classic", 3, None), ("ragged", "classic", 3, None), ("subtile", "classic", 3, None), ("opaque", "antialiased", 3, None)]


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_zero_row_is_the_identity_bit_for_bit(dt):
    R, t = pf.exp_map(torch.zeros(6, dtype=dt))
    assert torch.equal(R, torch.eye(3, dtype=dt)) and torch.equal(t, torch.zeros(3, dtype=dt))
    for case in ("single", "ragged", "deep"):
        c2w = bc.case_camera(case)[0].to(dt)
        assert torch.equal(pf.apply_pose(c2w, torch.zeros(6, dtype=dt)), c2w[:3])


def test_small_row_is_below_the_theta_clamp_and_moved_above():
    assert float((pf.pose_row("small")[3:] ** 2).sum()) < 1e-4 < float((pf.pose_row("moved")[3:] ** 2).sum())


def test_float64_pose_gradient_matches_central_differences():
    """`single-classic-3` flags no pixel, so no decision flips under the probe: h = 1e-5 leaves a truncation error of about h^2 and a rounding
    error of about 1e-11 / h; the bound is 1e-6 of the gradient's largest entry."""
    case, mode, deg, sep = "single", "classic", 3, None
    for name in pf.POSES:
        ref = pf.reference(case, mode, deg, sep, name)
        assert ref["flagged"] == 0.0
        p64 = {k: v.double() for k, v in ref["p"].items()}
        position = pf.apply_pose(bc.case_camera(case)[0].double(), ref["pose"])[:, 3]  # the view directions carry no gradient: held fixed

        def loss(row):
            with torch.no_grad():
                out = pf.render(p64, bc.case_camera(case), row, mode, deg, viewdir_position=position)
                return float(sum((out[k] * ref["w"][k]).sum() for k in ref["w"]))

        h, fd = 1e-5, torch.zeros(6, dtype=torch.float64)
        for i in range(6):
            e = torch.zeros(6, dtype=torch.float64)
            e[i] = h
            fd[i] = (loss(ref["pose"] + e) - loss(ref["pose"] - e)) / (2 * h)
        err = pf.vec_err(fd, ref["g64"]["pose"])
        print(f"{name}: autograd {ref['g64']['pose'].tolist()}, central differences err {err:.2e}")
        assert bc.amax(ref["g64"]["pose"]) > 0
        assert err <= 1e-6, (name, err)


@pytest.mark.parametrize("name", list(pf.POSES))
@pytest.mark.parametrize("cfg", FLOOR_CONFIGS, ids=[bc.config_id(c) for c in FLOOR_CONFIGS])
def test_float32_floor_and_flagged_pixels(cfg, name):
    ref = pf.reference(*cfg, name)
    fl = pf.floor(ref)
    print(f"{bc.config_id(cfg)} {name}: floor {fl:.2e}, flagged pixels {100 * ref['flagged']:.2f} %, d pose {[f'{v:.3e}' for v in ref['g64']['pose'].tolist()]}")
    assert fl <= bc.MAX_FLOOR, (name, fl)
    assert ref["flagged"] <= bc.MAX_FLAGGED_PIXELS, (name, ref["flagged"])
    assert bc.amax(ref["g64"]["pose"]) > 0 and bc.amax(ref["g64"]["dview"]) > 0


def test_config_validation_and_defaults():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import optim
    from nerfstudio_thermal_amd.config import CameraOptimizerConfig
    from nerfstudio_thermal_amd.splat import PinholeCamera, ThermalSplatfactoModelConfig, rescaled_camera, undistorted_camera

    cfg = ThermalSplatfactoModelConfig()
    assert cfg.camera_optimizer.mode == "off" and cfg.camera_optimizer_thermal.mode == "off"
    assert cfg.camera_optimizer is not cfg.camera_optimizer_thermal
    for mode in ("SO3xR3", "shared_SO3xR3"):
        assert ThermalSplatfactoModelConfig(camera_optimizer_thermal=CameraOptimizerConfig(mode=mode)).camera_optimizer_thermal.mode == mode
    for field in ("camera_optimizer", "camera_optimizer_thermal"):
        with pytest.raises(ValueError, match="SE3"):
            ThermalSplatfactoModelConfig(**{field: CameraOptimizerConfig(mode="SE3")})
    cam = PinholeCamera(torch.eye(4)[:3], 30.0, 31.0, 16.0, 8.0, 33, 17)
    assert cam.cam_idx is None and cam.is_thermal is False
    cam = dataclasses.replace(cam, cam_idx=5, is_thermal=True)
    for other in (rescaled_camera(cam, 2), undistorted_camera(cam, (0.05, 0.0, 0.0, 0.0, 0.0, 0.0))):
        assert other is not cam and other.cam_idx == 5 and other.is_thermal is True
    assert optim.SPLAT_CAMERA_OPTIMIZERS == {"camera_opt": (1e-3, 1e-4, 5000), "camera_opt_thermal": (1e-3, 1e-4, 5000)}
    assert not set(optim.SPLAT_CAMERA_OPTIMIZERS) & set(optim.SPLAT_OPTIMIZERS)


def test_pose_optimiser_rows_on_the_host():
    """Which row a frame reads is decided from the camera's fields alone (SplatCameraOptimizer on the CPU: it owns a parameter, runs no kernel)."""
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd.config import CameraOptimizerConfig
    from nerfstudio_thermal_amd.splat import PinholeCamera, SplatCameraOptimizer

    cam = lambda idx, th: PinholeCamera(torch.eye(4)[:3], 30.0, 30.0, 16.0, 8.0, 33, 17, cam_idx=idx, is_thermal=th)  # noqa: E731
    per = SplatCameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), 4, "cpu", thermal=True, non_trainable_camera_indices=torch.tensor([0, 2]))
    assert per.pose_adjustment.shape == (4, 6) and float(per.pose_adjustment.abs().max()) == 0.0 and per._frozen.tolist() == [1, 0, 1, 0]
    assert per.row(cam(1, True), True) == 1 and per.row(cam(3, True), True) == 3
    assert per.row(cam(1, True), False) is None  # per-frame rows: training renders only
    assert per.row(cam(1, False), True) is None  # an RGB frame never reads the thermal optimiser
    assert per.row(cam(None, True), True) is None and per.row(cam(2, True), True) is None  # no index / a non-trainable row: uncorrected
    with pytest.raises(ValueError, match="4 rows"):
        per.row(cam(4, True), True)
    shared = SplatCameraOptimizer(CameraOptimizerConfig(mode="shared_SO3xR3"), 4, "cpu", thermal=False)
    assert shared.pose_adjustment.shape == (1, 6)
    assert shared.row(cam(None, False), False) == 0 and shared.row(cam(3, False), True) == 0 and shared.row(cam(3, True), True) is None
    groups, losses = {}, {}
    per.get_param_groups(groups)
    shared.get_param_groups(groups)
    assert set(groups) == {"camera_opt", "camera_opt_thermal"} and groups["camera_opt_thermal"][0] is per.pose_adjustment
    for cfg in (CameraOptimizerConfig(mode="off"), CameraOptimizerConfig(mode="SO3xR3", penalty_scale=-1.0)):
        off = SplatCameraOptimizer(cfg, 4, "cpu")
        off.get_param_groups(losses)
        off.get_metrics_dict(losses)
        off.get_loss_dict(losses)
        assert losses == {} and list(off.parameters()) == [] and off.state_dict() == {} and off.row(cam(1, False), True) is None
    with pytest.raises(ValueError, match="num_train_data"):
        SplatCameraOptimizer(CameraOptimizerConfig(mode="SO3xR3"), 0, "cpu")
    with pytest.raises(ValueError, match="SE3"):
        SplatCameraOptimizer(CameraOptimizerConfig(mode="SE3"), 4, "cpu")
