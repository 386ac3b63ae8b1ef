"""The differentiable depth of the splat training render on the GPU (ThermalSplatfactoModelConfig.differentiable_depth: the DEPTH instantiations of
k_splat_raster_bwd, k_splat_pair_fold and k_splat_project_bwd behind the depth groups of tn_splat_raster_backward / tn_splat_project_backward, through
ThermalSplatfactoModel.get_train_outputs and .backward()) and the fused depth losses (tn_depth_loss), against the float64 references of
tests/splat_depth_functional.py on scenes of tests/splat_backward_cases.py, all classic:

  subtile-3, opaque-3, deep-3, ragged-1, clamped-3, single-3      shared opacity
  opaque-3-sep-thermal_low, opaque-3-sep-rgb_low                  separate opacity: the depth rides chain 1 while chain 2 stops elsewhere
  ragged-1 with use_absgrad                                       the statistic's slots move behind the new one
  subtile-3-pose-moved                                            the pose instantiation: dL/d pose through row 2 of dL/d view'

each under two depth upstreams drawn together with random v_rgbt and v_alpha ("acc": w * accumulation, "raw": w; splat_depth_functional).
Bound of the parity tests: err <= 8 x floor per gradient tensor (the project's margin, profiles/splat_backward_parity.md), the floor being
max(float32 autograd's error, the float32 walk's error, 2^-23) and every error relative to the larger of the two float64 partial gradients'
largest entries.  Conditions on the scenes: floor <= 2e-5 ("acc") or MAX_FLOOR_RAW ("raw"), flagged pixels <= 10 %, excluded Gaussians <= 1 %.
Nothing is calibrated on the kernels' output; every figure is printed before it is asserted, and profiles/splat_depth_grad.md holds them."""
import pytest
import torch

import splat_backward_cases as bc
import splat_depth_functional as df
import splat_pose_functional as pf
import test_splat_forward_cpu as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
TRAIN_FRAMES = 4
ROW = 2
CASES = [(cfg, name) for cfg in df.CONFIGS for name in df.UPSTREAMS]
IDS = [f"{df.config_id(cfg)}-{name}" for cfg, name in CASES]


def _model(cfg, p, depth=True, absgrad=False, **kw):
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd.config import CameraOptimizerConfig
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

    _, deg, sep, pose = cfg
    c = ThermalSplatfactoModelConfig(sh_degree=deg, sh_degree_interval=1, rasterize_mode="classic", thermal_opacity_mode="separate" if sep else "shared",
                                     use_absgrad=absgrad, differentiable_depth=depth, camera_optimizer=CameraOptimizerConfig(mode="SO3xR3" if pose else "off"), **kw)
    m = ThermalSplatfactoModel(c, num_points=4, device=DEV, num_train_data=TRAIN_FRAMES)
    m.load_gaussians(p)
    m.step = 10**6
    bg, bgt = fc.background()
    m._background4 = lambda training: bg.tolist() + [bgt]  # the frame's background: the test's RGB + thermal colour
    if pose:
        with torch.no_grad():
            m.camera_optimizer.pose_adjustment[ROW] = pf.pose_row(pose).float().to(DEV)
    return m


def _camera(case, cam_idx=ROW):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    return PinholeCamera(*bc.case_camera(case), cam_idx=cam_idx)


def _backward(m, cam, w, v_depth=None):
    m.zero_grad(set_to_none=True)
    out = m.get_train_outputs(cam)
    loss = sum((out[k] * w[k].float().to(DEV)).sum() for k in w)
    if v_depth is not None:
        loss = loss + (out["depth"] * v_depth.float().to(DEV)).sum()
    loss.backward()
    g = {k: m.gauss_params[k].grad.detach().cpu().clone() for k in m.param_names}
    g["xys"] = m.last_xys_grad.detach().cpu().clone()
    if m.last_xys_absgrad is not None:
        g["xys_abs"] = m.last_xys_absgrad.detach().cpu().clone()
    pose = getattr(m.camera_optimizer, "pose_adjustment", None)
    if pose is not None and pose.grad is not None:
        g["pose"] = pose.grad[ROW].detach().cpu().clone()
    return g, out


def _excluded(m, ref):
    radii_hip = m.last_projection["radii"].cpu()
    excl = ref["excl"] | ((radii_hip > 0) != (ref["out64"]["projection"]["radii"] > 0))
    assert int(excl.sum()) <= bc.MAX_EXCLUDED_GAUSSIANS * excl.numel(), int(excl.sum())
    return excl, radii_hip


def _check_parity(cfg, name, hip, m, ref):
    excl, radii_hip = _excluded(m, ref)
    fl = df.floors(ref, name, excl, cfg)
    assert ref["flagged"] <= bc.MAX_FLAGGED_PIXELS, ref["flagged"]
    worst = []
    for k in df.grad_keys(cfg):
        floor, ea, ew = fl[k]
        e = df.err(hip[k], ref, name, k, excl)
        print(f"{df.config_id(cfg)}-{name} {k}: err {e:.2e}, floor {floor:.2e} (float32 autograd {ea:.2e}, float32 walk {ew:.2e}), ratio {e / floor:.2f}, "
              f"scale {df.scale(ref, name, k, excl):.3e}")
        worst.append((k, e, floor))
    for k, e, floor in worst:
        assert bool(torch.isfinite(hip[k]).all()), k
        assert floor <= df.max_floor(name), (k, floor)
        assert e <= TOL_FACTOR * floor, (k, e, floor)
    for k in m.param_names:  # culled Gaussians get exactly zero
        assert bc.amax(hip[k][radii_hip == 0]) == 0.0, k
    return excl


@pytest.mark.parametrize("cfg,name", CASES, ids=IDS)
def test_gradients_match_float64(cfg, name):
    ref = df.reference(cfg)
    m = _model(cfg, ref["p"])
    hip, out = _backward(m, _camera(cfg[0]), ref["w"], ref["v_depth"][name])
    assert out["depth"].requires_grad
    _check_parity(cfg, name, hip, m, ref)
    assert bc.amax(hip["means"]) > 0


@pytest.mark.parametrize("name", df.UPSTREAMS)
def test_gradients_match_float64_with_absgrad(name):
    """The absgrad slots sit behind the depth slot: every gradient as without the flag, and last_xys_absgrad against the float64 walk of the same
    chains (five channels, v_alpha_eff), at 8 x max(float32 walk's error on it, the signed xys floor, 2^-23) of its largest entry: the rule of
    tests/test_splat_absgrad_gpu.py."""
    cfg = df.ABS_CONFIG
    ref = df.reference(cfg)
    m = _model(cfg, ref["p"], absgrad=True)
    hip, _ = _backward(m, _camera(cfg[0]), ref["w"], ref["v_depth"][name])
    excl = _check_parity(cfg, name, hip, m, ref)
    a64, a32 = df.walk64(cfg)[name]["xys_abs"], ref["walk32"][name]["xys_abs"]
    floor = max(bc.rel_err(a32, a64, ~excl), df.floors(ref, name, excl, cfg)["xys"][0], bc.EPS)
    e = bc.rel_err(hip["xys_abs"], a64, ~excl)
    print(f"{df.config_id(cfg)}-{name} xys_abs: err {e:.2e}, floor {floor:.2e}, ratio {e / floor:.2f}")
    assert e <= TOL_FACTOR * floor, (e, floor)
    assert float(hip["xys_abs"].min()) >= 0.0 and bc.amax(hip["xys_abs"]) > 0
    plain, _ = _backward(_model(cfg, ref["p"]), _camera(cfg[0]), ref["w"], ref["v_depth"][name])
    for k in list(m.param_names) + ["xys"]:
        assert torch.equal(hip[k], plain[k]), k


@pytest.mark.parametrize("cfg", [df.SHARED_CONFIGS[1], df.SEP_CONFIGS[0], df.POSE_CONFIG], ids=df.config_id)
def test_backward_is_bit_reproducible(cfg):
    ref = df.reference(cfg)
    m = _model(cfg, ref["p"], absgrad=True)
    a, _ = _backward(m, _camera(cfg[0]), ref["w"], ref["v_depth"]["raw"])
    b, _ = _backward(m, _camera(cfg[0]), ref["w"], ref["v_depth"]["raw"])
    assert set(a) == set(b) and ("pose" in a) == bool(cfg[3])
    for k in a:
        assert torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k]).all()), k


@pytest.mark.parametrize("cfg", [df.SHARED_CONFIGS[2], df.SEP_CONFIGS[1], df.POSE_CONFIG], ids=df.config_id)
def test_a_loss_without_depth_gives_the_flag_off_bits(cfg):
    """differentiable_depth on and a loss that never touches depth: the backward receives no depth upstream, runs the entry points of before and
    gives, bit for bit, what the model without the flag gives."""
    ref = df.reference(cfg)
    on, off = _model(cfg, ref["p"], depth=True, absgrad=True), _model(cfg, ref["p"], depth=False, absgrad=True)
    g_on, out_on = _backward(on, _camera(cfg[0]), ref["w"])
    g_off, out_off = _backward(off, _camera(cfg[0]), ref["w"])
    assert out_on["depth"].requires_grad and not out_off["depth"].requires_grad
    assert torch.equal(out_on["depth"].detach(), out_off["depth"])
    assert set(g_on) == set(g_off)
    for k in g_on:
        assert bc.amax(g_off[k]) > 0 and torch.equal(g_on[k], g_off[k]), k
    with_depth, _ = _backward(on, _camera(cfg[0]), ref["w"], ref["v_depth"]["raw"])
    assert not torch.equal(with_depth["means"], g_on["means"])  # and the depth upstream does change them


def test_training_depth_requires_grad_and_equals_the_eval_depth():
    cfg = df.SHARED_CONFIGS[0]
    ref = df.reference(cfg)
    m = _model(cfg, ref["p"])
    cam = _camera(cfg[0])
    tr, ev = m.get_train_outputs(cam), m.get_outputs(cam)
    assert tr["depth"].requires_grad
    assert torch.equal(tr["depth"].detach(), ev["depth"])
    covered = (ref["out64"]["accumulation"] > 0) & ~ref["out64"]["flag_pixels"][..., None]
    d64 = ref["out64"]["depth"]
    assert float(((tr["depth"].detach().cpu().double() - d64).abs() * covered).max()) <= 1e-4 * float(d64.max())


def test_depth_only_loss_on_an_empty_frame_gives_zeros():
    import dataclasses

    from nerfstudio_thermal_amd.synth import look_at_camera

    cfg = df.SHARED_CONFIGS[5]
    m = _model(cfg, df.reference(cfg)["p"])
    away = dataclasses.replace(_camera("single"), camera_to_world=look_at_camera((2.5, 0.0, 0.0), target=(5.0, 0.0, 0.0)))
    out = m.get_train_outputs(away)
    assert m.last_num_intersections == 0
    out["depth"].sum().backward()
    for k in m.param_names:
        assert bc.amax(m.gauss_params[k].grad) == 0.0, k


# ------------------------------------------------------------------------------------------------ tn_depth_loss
D_MULT, TV_MULT = 0.75, 1.5  # exact in fp32
LOSS_FRAMES = {"33x17": (17, 33, 1, 0, 0.0), "70x37": (37, 70, 2, 0, 0.05), "border": (40, 70, 3, 5, 0.0)}  # (h, w, seed, uncovered border, share of holes)


def _loss_hip(depth, acc, sensor, d_mult, tv_mult):
    from nerfstudio_thermal_amd.splat import depth_losses

    x = depth.detach().clone().requires_grad_(True)
    l_d, l_tv = depth_losses(x, acc, sensor, d_mult, tv_mult)
    (l_d + l_tv).backward()
    return l_d.detach(), l_tv.detach(), x.grad


@pytest.mark.parametrize("mults", [(D_MULT, 0.0), (0.0, TV_MULT), (D_MULT, TV_MULT)])
@pytest.mark.parametrize("frame", list(LOSS_FRAMES))
def test_depth_losses_against_restatement(frame, mults):
    """tests/test_splat_thermal_reg_gpu.py's rule: losses within 1e-5 relative; the gradient within 1e-4 of its largest entry on every pixel none of
    whose terms is a near-tie in float64 (|argument| < 1e-5: a sign decided in fp32 may differ there), such pixels being at most 0.5 % of the frame
    (a pixel holds up to five terms where that test counts terms: 2e-3 of the terms there)."""
    depth, acc, sensor = df.loss_frame(*LOSS_FRAMES[frame])
    l_d, l_tv, g = _loss_hip(depth.to(DEV), acc.to(DEV), sensor.to(DEV), *mults)
    x = depth.double().requires_grad_(True)
    r_d, r_tv = df.depth_losses(x, acc.double(), sensor.double(), *mults)
    (r_d + r_tv).backward()
    r_d, r_tv = r_d.detach(), r_tv.detach()
    mask, share = df.near_ties(depth, acc, sensor, *mults)
    err = float(((g.cpu().double() - x.grad).abs()[..., 0] * (~mask)).max())
    scale = float(x.grad.abs().max())
    print(f"{frame} mults {mults}: depth_loss {float(l_d):.8e} (ref {float(r_d):.8e}) depth_tv_loss {float(l_tv):.8e} (ref {float(r_tv):.8e}) gradient error "
          f"{err:.2e} of {scale:.2e}, near-tie pixels {share:.2e}")
    assert abs(float(l_d) - float(r_d)) <= 1e-5 * abs(float(r_d)), (float(l_d), float(r_d))
    assert abs(float(l_tv) - float(r_tv)) <= 1e-5 * abs(float(r_tv)), (float(l_tv), float(r_tv))
    assert share <= 5e-3, share
    assert scale > 0 and err <= 1e-4 * scale, (err, scale)
    assert g.shape == depth.shape and bool(torch.isfinite(g).all())
    if frame == "border":  # windows straddle accumulation == 0: the uncovered pixels and everything beyond them take no TV gradient
        assert bc.amax(g.cpu()[(acc == 0)]) == 0.0


def test_depth_losses_are_reproducible_and_degenerate_to_zero():
    depth, acc, sensor = (t.to(DEV) for t in df.loss_frame(*LOSS_FRAMES["70x37"]))
    a, b = _loss_hip(depth, acc, sensor, D_MULT, TV_MULT), _loss_hip(depth, acc, sensor, D_MULT, TV_MULT)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    none = _loss_hip(depth, torch.zeros_like(acc), sensor, D_MULT, TV_MULT)  # nothing covered: both 0, no gradient
    assert float(none[0]) == 0.0 and float(none[1]) == 0.0 and bc.amax(none[2].cpu()) == 0.0
    no_sensor = _loss_hip(depth, acc, None, D_MULT, TV_MULT)
    only_tv = _loss_hip(depth, acc, sensor, 0.0, TV_MULT)
    assert float(no_sensor[0]) == 0.0 and torch.equal(no_sensor[1], only_tv[1]) and torch.equal(no_sensor[2], only_tv[2])


def test_model_step_with_both_depth_losses():
    cfg = df.SHARED_CONFIGS[1]  # opaque: 43 x 37, silhouettes inside the frame
    ref = df.reference(cfg)
    m = _model(cfg, ref["p"], depth_loss_mult=0.1, depth_tv_loss_mult=0.05)
    m.train()
    cam = _camera(cfg[0])
    _, W, H = bc.case_camera(cfg[0])[4:]
    gen = torch.Generator().manual_seed(3)
    batch = {"image": torch.rand(H, W, 3, generator=gen).to(DEV), "is_thermal": False,
             "depth_image": (ref["out64"]["depth"].float() + 0.2 * torch.randn(H, W, 1, generator=gen)).to(DEV)}
    out = m.get_train_outputs(cam)
    losses = m.get_loss_dict(out, batch)
    assert {"depth_loss", "depth_tv_loss"} <= set(losses)
    assert float(losses["depth_loss"]) > 0 and float(losses["depth_tv_loss"]) > 0
    m.zero_grad(set_to_none=True)
    (losses["depth_loss"] + losses["depth_tv_loss"]).backward()  # the depth alone carries this gradient
    g = m.gauss_params["means"].grad
    assert bool(torch.isfinite(g).all()) and bc.amax(g.cpu()) > 0
    out = m.get_train_outputs(cam)
    losses = m.get_loss_dict(out, {k: v for k, v in batch.items() if k != "depth_image"})
    assert float(losses["depth_loss"]) == 0.0 and "depth_tv_loss" in losses  # the keys depend on the config alone
