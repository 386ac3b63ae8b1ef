"""Camera pose gradients and pose refinement of the splat model on the GPU: tn_splat_pose_camera, the pose instantiations of k_splat_project /
k_splat_project_bwd and k_splat_pose_finish, through ThermalSplatfactoModel, against the float64 restatement of tests/splat_pose_functional.py.

Bounds.  The pose gradient (and dL/d view', the parameter gradients and xys at the `moved` row): err <= 8 x floor, the floor being the float32
restatement's own distance from float64 on the same scene and row, never below 2^-23 (tests/test_splat_pose_cpu.py holds it under 2e-5), the
factor 8 the project's margin over the float32 floor (profiles/splat_backward_parity.md); and, independently, err <= 2e-4 of the largest entry.
Images at `moved`: 8 x the float32 restatement's own largest error outside the flagged pixels (never below 2^-23).  Nothing is calibrated on
the kernels' output; every figure is printed before it is asserted, profiles/splat_pose.md holds the measured ones."""
import dataclasses

import pytest
import torch

import splat_backward_cases as bc
import splat_pose_functional as pf
import test_splat_forward_cpu as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
FIXED_BOUND = 2e-4
CONFIGS = [("single", "classic", 3, None), ("subtile", "classic", 3, None), ("ragged", "classic", 3, None), ("ragged", "antialiased", 0, None),
           ("opaque", "antialiased", 3, None), ("faint", "classic", 3, "mirror"), ("deep", "classic", 3, None)]
IDS = [bc.config_id(c) for c in CONFIGS]
TRAIN_FRAMES = 4
ROW = 2  # the training frame the tests' camera is


def _model(p, mode, deg, sep, rgb_mode="off", thermal_mode="off", train_is_thermal=None):
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd.config import CameraOptimizerConfig
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

    cfg = ThermalSplatfactoModelConfig(sh_degree=deg, sh_degree_interval=1, rasterize_mode=mode, thermal_opacity_mode="separate" if sep else "shared",
                                       camera_optimizer=CameraOptimizerConfig(mode=rgb_mode), camera_optimizer_thermal=CameraOptimizerConfig(mode=thermal_mode))
    m = ThermalSplatfactoModel(cfg, num_points=4, device=DEV, num_train_data=TRAIN_FRAMES, train_is_thermal=train_is_thermal)
    m.load_gaussians(p)
    m.step = 10**6
    bg, bgt = fc.background()
    m._background4 = lambda training: bg.tolist() + [bgt]  # the frame's background: the test's RGB + thermal colour on both paths
    return m


def _camera(case, cam_idx=ROW, is_thermal=False):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    return PinholeCamera(*bc.case_camera(case), cam_idx=cam_idx, is_thermal=is_thermal)


def _set_row(opt, row, pose):
    with torch.no_grad():
        opt.pose_adjustment[row] = pose.float().to(DEV)


def _grads(m, cam, w, zero=True):
    if zero:
        m.zero_grad(set_to_none=True)
    out = m.get_train_outputs(cam)
    sum((out[k] * w[k].float().to(DEV)).sum() for k in w).backward()
    g = {k: m.gauss_params[k].grad.detach().cpu().clone() for k in m.param_names}
    g["xys"] = m.last_xys_grad.detach().cpu().clone()
    for name, opt in (("pose", m.camera_optimizer), ("pose_thermal", m.camera_optimizer_thermal)):
        if opt.mode != "off" and opt.pose_adjustment.grad is not None:
            g[name] = opt.pose_adjustment.grad.detach().cpu().clone()
    return g, out


def _simple_upstream(case, sep=None):
    _, W, H = bc.case_camera(case)[4:]
    return bc.upstream(case, sep, torch.zeros(H, W, dtype=torch.bool))


@pytest.mark.parametrize("cfg", [("ragged", "classic", 3, None), ("faint", "classic", 3, "mirror")], ids=["ragged-classic-3", "faint-classic-3-sep-mirror"])
def test_zero_row_is_mode_off_bit_for_bit(cfg):
    """The pose instantiations at a zero row against the kernels without the pack: images, every parameter gradient and last_xys_grad."""
    case, mode, deg, sep = cfg
    ref = pf.reference(*cfg, "zero")
    cam = _camera(case)
    m_off = _model(ref["p"], mode, deg, sep)
    m_on = _model(ref["p"], mode, deg, sep, "SO3xR3", "SO3xR3")
    g_off, o_off = _grads(m_off, cam, ref["w"])
    g_on, o_on = _grads(m_on, cam, ref["w"])
    assert m_on.last_view_grad is not None and "pose" in g_on and "pose" not in g_off
    for k in [k for k, _ in bc.images(sep)] + ["depth"]:
        assert torch.equal(o_on[k].detach(), o_off[k].detach()), k
    for k in list(m_off.param_names) + ["xys"]:
        assert torch.equal(g_on[k], g_off[k]), k
    for k in ("xys", "depths", "radii", "conics", "compensation", "num_tiles_hit", "tile_box"):
        assert torch.equal(m_on.last_projection[k], m_off.last_projection[k]), k
    assert bc.amax(g_on["pose"][ROW]) > 0


def test_zero_row_record_equals_the_host_camera():
    """tn_splat_pose_camera at a zero row: every number of the device record equals the host struct's (D is exactly the identity)."""
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd.splat import camera_struct, pose_camera_record

    for case in ("single", "ragged", "deep", "subtile"):
        cam = _camera(case)
        s = camera_struct(cam)
        rec = pose_camera_record(cam, s, torch.zeros((TRAIN_FRAMES, 6), device=DEV), ROW).cpu()
        proj = torch.tensor(list(s.projmat))
        assert torch.equal(rec[:12], torch.tensor(list(s.viewmat))), case
        assert torch.equal(rec[12:20], proj[:8]) and torch.equal(rec[24:28], proj[12:]), case
        assert torch.equal(rec[28:31], torch.tensor(list(s.position))), case


def _excluded(m, out64):
    radii_hip = m.last_projection["radii"].cpu()
    pj = out64["projection"]
    excl = (pj["near_clamp"] & pj["ok"]) | ((radii_hip > 0) != (pj["radii"] > 0))
    assert int(excl.sum()) <= bc.MAX_EXCLUDED_GAUSSIANS * excl.numel(), int(excl.sum())
    return excl


@pytest.mark.parametrize("name", list(pf.POSES))
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_pose_gradient_matches_float64(cfg, name):
    case, mode, deg, sep = cfg
    ident = f"{bc.config_id(cfg)} {name}"
    ref = pf.reference(*cfg, name)
    cam = _camera(case)
    m = _model(ref["p"], mode, deg, sep, "SO3xR3")
    _set_row(m.camera_optimizer, ROW, ref["pose"])
    hip, out = _grads(m, cam, ref["w"])
    floor = pf.floor(ref)
    err = pf.vec_err(hip["pose"][ROW], ref["g64"]["pose"])
    print(f"{ident}: d pose err {err:.2e}, floor {floor:.2e}, ratio {err / floor:.2f}; {100 * ref['flagged']:.2f} % of the pixels without upstream gradient")
    assert bool(torch.isfinite(hip["pose"]).all())
    assert err <= TOL_FACTOR * floor, (err, floor)
    assert err <= FIXED_BOUND, err
    rows = torch.arange(TRAIN_FRAMES) != ROW
    assert bc.amax(hip["pose"][rows]) == 0.0  # exactly zero outside the frame's row
    if cfg == ("ragged", "classic", 3, None):  # the optional dL/d view' output
        floor_v = pf.floor(ref, "dview")
        err_v = pf.vec_err(m.last_view_grad.cpu(), ref["g64"]["dview"])
        print(f"{ident}: d view' err {err_v:.2e}, floor {floor_v:.2e}, ratio {err_v / floor_v:.2f}")
        assert err_v <= TOL_FACTOR * floor_v and err_v <= FIXED_BOUND, (err_v, floor_v)
    if name != "moved":
        return
    # the forward used the corrected camera: parameter gradients, xys and the images against float64 at the moved camera
    excl = _excluded(m, ref["out64"])
    for k in list(bc.param_names(sep)) + ["xys"]:
        fl = max(bc.rel_err(ref["g32"][k], ref["g64"][k], ~excl), bc.EPS)
        e = bc.rel_err(hip[k], ref["g64"][k], ~excl)
        print(f"{ident} d {k}: err {e:.2e}, floor {fl:.2e}, ratio {e / fl:.2f}")
        assert e <= TOL_FACTOR * fl and e <= FIXED_BOUND, (k, e, fl)
    keep = ~(ref["out64"]["flag_pixels"] | ref["out32"]["flag_pixels"])
    for k in ("rgb", "thermal"):
        own = max(bc.amax((ref["out32"][k].double() - ref["out64"][k])[keep]), bc.EPS)
        e = bc.amax((out[k].detach().cpu().double() - ref["out64"][k])[keep])
        print(f"{ident} {k}: err {e:.2e}, the float32 restatement's {own:.2e}, ratio {e / own:.2f}")
        assert e <= TOL_FACTOR * own, (k, e, own)


def test_pose_gradient_is_bit_reproducible():
    """Two backward passes of one frame, and a model whose workspaces served a larger scene (upstream x 1000) against a fresh one."""
    deep, ragged = pf.reference("deep", "classic", 3, None, "moved"), pf.reference("ragged", "classic", 3, None, "moved")
    fresh = _model(ragged["p"], "classic", 3, None, "SO3xR3")
    _set_row(fresh.camera_optimizer, ROW, ragged["pose"])
    a, _ = _grads(fresh, _camera("ragged"), ragged["w"])
    b, _ = _grads(fresh, _camera("ragged"), ragged["w"])
    view_a = fresh.last_view_grad.cpu().clone()
    assert bc.amax(a["pose"]) > 0 and torch.equal(a["pose"], b["pose"])
    used = _model(deep["p"], "classic", 3, None, "SO3xR3")
    _set_row(used.camera_optimizer, ROW, deep["pose"])
    dirty, _ = _grads(used, _camera("deep"), {k: 1e3 * v for k, v in deep["w"].items()})
    assert bc.amax(dirty["pose"]) > 0
    used.load_gaussians(ragged["p"])
    _set_row(used.camera_optimizer, ROW, ragged["pose"])
    c, _ = _grads(used, _camera("ragged"), ragged["w"])
    assert torch.equal(c["pose"], a["pose"]) and torch.equal(used.last_view_grad.cpu(), view_a)
    for k in a:
        assert torch.equal(c[k], a[k]), k


def test_rows_and_spectra():
    case = "single"
    p, w = bc.scene(case, 3), _simple_upstream(case)
    m = _model(p, "classic", 3, None, "SO3xR3", "SO3xR3", train_is_thermal=[False, False, True, True])
    _set_row(m.camera_optimizer, 1, pf.pose_row("small"))
    g, _ = _grads(m, _camera(case, 1, False), w)
    assert bc.amax(g["pose"][1]) > 0 and bc.amax(g["pose"][[0, 2, 3]]) == 0.0 and "pose_thermal" not in g
    first = g["pose"].clone()
    g, _ = _grads(m, _camera(case, 0, False), w, zero=False)  # a second frame accumulates into its own row
    assert torch.equal(g["pose"][1], first[1]) and bc.amax(g["pose"][0]) > 0 and bc.amax(g["pose"][[2, 3]]) == 0.0
    g, _ = _grads(m, _camera(case, 2, True), w)  # a thermal frame touches only camera_optimizer_thermal
    assert "pose" not in g and bc.amax(g["pose_thermal"][2]) > 0 and bc.amax(g["pose_thermal"][[0, 1, 3]]) == 0.0
    g_plain, o_plain = _grads(_model(p, "classic", 3, None), _camera(case, 0, False), w)
    g, o = _grads(m, _camera(case, 0, True), w)  # thermal frame on a row marked RGB: non-trainable, rendered uncorrected
    assert "pose" not in g and "pose_thermal" not in g and torch.equal(o["rgb"].detach(), o_plain["rgb"].detach())
    g, o = _grads(m, _camera(case, None, False), w)  # no cam_idx under a per-frame mode: uncorrected
    assert "pose" not in g and torch.equal(g["means"], g_plain["means"])
    shared = _model(p, "classic", 3, None, "shared_SO3xR3")
    assert shared.camera_optimizer.pose_adjustment.shape == (1, 6)
    g, _ = _grads(shared, _camera(case, 3, False), w)
    assert g["pose"].shape == (1, 6) and bc.amax(g["pose"][0]) > 0
    per = _model(p, "classic", 3, None, "SO3xR3")
    gp, _ = _grads(per, _camera(case, 3, False), w)
    assert torch.equal(g["pose"][0], gp["pose"][3])  # the same frame and (zero) row: the same numbers, whichever row they land in


def test_eval_applies_a_shared_row_only():
    case = "ragged"
    p = bc.scene(case, 3)
    cam = _camera(case, 1, True)
    plain = _model(p, "classic", 3, None).get_outputs(cam)
    shared = _model(p, "classic", 3, None, "off", "shared_SO3xR3")
    _set_row(shared.camera_optimizer_thermal, 0, pf.pose_row("moved"))
    ev = shared.get_outputs(cam)
    assert not torch.equal(ev["thermal"], plain["thermal"]) and float((ev["thermal"] - plain["thermal"]).abs().max()) > 1e-3
    tr = shared.get_train_outputs(cam)
    for k in ("rgb", "thermal", "accumulation", "depth"):
        assert torch.equal(tr[k].detach(), ev[k]), k  # fixed background: the training render is the eval render
    rgb = shared.get_outputs(dataclasses.replace(cam, is_thermal=False))  # the RGB spectrum has no row
    assert torch.equal(rgb["rgb"], plain["rgb"])
    per = _model(p, "classic", 3, None, "off", "SO3xR3")
    _set_row(per.camera_optimizer_thermal, 1, pf.pose_row("moved"))
    ev = per.get_outputs(cam)
    for k in ("rgb", "thermal", "accumulation", "depth"):
        assert torch.equal(ev[k], plain[k]), k  # a per-frame row never reaches an eval render
    assert not torch.equal(per.get_train_outputs(cam)["thermal"].detach(), plain["thermal"])


def test_pose_refinement_recovers_a_rigid_error():
    """40 Gaussians, 4 RGB cameras around them; ground truth rendered from the true poses, the model given cameras off by one rigid error
    c2w_bad = c2w A(e), so that the row that repairs a frame is p* with A(p*) = A(e)^-1: p* = (-R(w)^T t, -w).  Gaussians frozen, HipAdam on
    camera_opt alone: after the run the loss over the four frames and |p - p*| are both below where they started (conditions); the values
    reached are printed (profiles/splat_pose.md)."""
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import optim
    from nerfstudio_thermal_amd.splat import PinholeCamera
    from nerfstudio_thermal_amd.synth import look_at_camera
    import splat_functional as sf

    deg, steps = 3, 60
    p = fc._with(sf.scene(40, 33, deg, extent=0.6, scale_range=(-2.6, -2.0)), opacities=torch.full((40, 1), 1.5))
    W, H = 48, 40
    fx = sf.fov_focal(W, 50.0)
    eyes = [(2.4, 0.2, 0.5), (0.3, 2.4, 0.6), (-2.3, 0.4, 0.7), (0.2, -2.4, 0.4)]
    err = torch.tensor([0.03, -0.02, 0.015, 0.01, -0.015, 0.02], dtype=torch.float64)
    R, t = pf.exp_map(err)
    p_star = torch.cat([-(R.T @ t), -err[3:]]).float()
    true = [PinholeCamera(look_at_camera(e), fx, fx, W / 2, H / 2, W, H, cam_idx=i) for i, e in enumerate(eyes)]
    bad = [dataclasses.replace(c, camera_to_world=pf.apply_pose(c.camera_to_world.double(), err).float()) for c in true]
    m = _model(p, "classic", deg, None, "SO3xR3")
    plain = _model(p, "classic", deg, None)
    gt = [{"image": plain.get_outputs(c)["rgb"].clone(), "is_thermal": False} for c in true]
    for q in m.gauss_params.values():
        q.requires_grad_(False)
    groups = {"camera_opt": m.get_param_groups()["camera_opt"]}
    opts = optim.Optimizers(groups, optim.SPLAT_CAMERA_OPTIMIZERS, optimizer_cls=optim.HipAdam)

    def total_loss():
        with torch.no_grad():
            return sum(float(m.get_loss_dict(m.get_train_outputs(c), b)["main_loss"]) for c, b in zip(bad, gt))

    def distance():
        return float((m.camera_optimizer.pose_adjustment.detach().cpu() - p_star).norm(dim=-1).mean())

    loss0, dist0 = total_loss(), distance()
    for step in range(steps):
        for c, b in zip(bad, gt):
            opts.zero_grad_all()
            losses = m.get_loss_dict(m.get_train_outputs(c), b)
            assert "camera_opt_regularizer" in losses
            sum(losses.values()).backward()
            opts.optimizer_step_all()
            opts.scheduler_step_all()
    loss1, dist1 = total_loss(), distance()
    print(f"pose refinement: {steps} passes over 4 frames; main loss {loss0:.4e} -> {loss1:.4e}; mean |p - p*| {dist0:.4e} -> {dist1:.4e}")
    assert loss1 < loss0 and dist1 < dist0


def test_refinement_and_state_dict_leave_the_poses_alone():
    from nerfstudio_thermal_amd import optim

    case = "ragged"
    p, w = bc.scene(case, 3), _simple_upstream(case)
    m = _model(p, "classic", 3, None, "SO3xR3", "shared_SO3xR3")
    m.config.warmup_length, m.config.refine_every, m.config.stop_split_at = 0, 1, 10**7
    m.config.densify_grad_thresh, m.config.cull_alpha_thresh = 0.0, 0.3  # every visible Gaussian splits or duplicates, faint ones are culled
    groups = m.get_param_groups()
    assert {"camera_opt", "camera_opt_thermal"} <= set(groups)
    opts = optim.Optimizers(groups, {**optim.SPLAT_OPTIMIZERS, **optim.SPLAT_CAMERA_OPTIMIZERS}, optimizer_cls=optim.HipAdam)
    m.step = 7
    opts.zero_grad_all()
    out = m.get_train_outputs(_camera(case))
    losses = m.get_loss_dict(out, {"image": torch.rand(out["rgb"].shape, device=DEV), "is_thermal": False})
    assert {"camera_opt_regularizer", "camera_opt_regularizer_thermal"} <= set(losses)
    metrics = m.get_metrics_dict(out, {"image": torch.rand(out["rgb"].shape, device=DEV), "is_thermal": False})
    assert {"camera_opt_translation", "camera_opt_rotation", "camera_opt_translation_thermal", "camera_opt_rotation_thermal"} <= set(metrics)
    sum(losses.values()).backward()
    opts.optimizer_step_all()
    m.after_train(7)
    pose = m.camera_optimizer.pose_adjustment
    o = opts.optimizers["camera_opt"]
    before = (pose.detach().clone(), o.state[pose]["exp_avg"].clone(), o.state[pose]["exp_avg_sq"].clone())
    assert bc.amax(before[0].cpu()) > 0 and bc.amax(before[1].cpu()) > 0
    n0 = m.num_points
    m.refinement_after(opts, 7)
    assert m.num_points != n0 and m.last_refine_counts[2] + m.last_refine_counts[3] > 0
    assert m.camera_optimizer.pose_adjustment is pose and o.param_groups[0]["params"][0] is pose
    assert torch.equal(pose.detach(), before[0]) and torch.equal(o.state[pose]["exp_avg"], before[1]) and torch.equal(o.state[pose]["exp_avg_sq"], before[2])
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    assert "camera_optimizer.pose_adjustment" in sd and "camera_optimizer_thermal.pose_adjustment" in sd
    other = _model(bc.scene("single", 3), "classic", 3, None, "SO3xR3", "shared_SO3xR3")
    other.load_state_dict(sd)
    assert other.num_points == m.num_points and torch.equal(other.camera_optimizer.pose_adjustment.detach(), pose.detach())
    off = _model(p, "classic", 3, None)  # both modes off: the groups, the state dict and the dict keys are what they were
    assert set(off.get_param_groups()) == set(off.group_params) and not [k for k in off.state_dict() if "camera" in k]
    out = off.get_train_outputs(_camera(case))
    batch = {"image": torch.rand(out["rgb"].shape, device=DEV), "is_thermal": False}
    assert not [k for k in list(off.get_loss_dict(out, batch)) + list(off.get_metrics_dict(out, batch)) if "camera" in k]
