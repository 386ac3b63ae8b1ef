"""Shared (rig) pose corrections of thermal-nerfacto on the GPU: the two entry points against the float64 restatement
(tests/nerf_shared_pose_functional.py), a whole training step on the engine's own sample bins against the oracle, evaluation renders, the
optimiser groups and the state dict.

Bounds.  A float32 kernel against its float64 restatement: 8 x the largest error of the SAME expressions evaluated in float32 torch against
float64, on the same rays and over all outputs of the call (the project's rule; nothing here is calibrated on the kernel's output).  The
whole step: the tolerances of tests/test_fullsize_parity_gpu.py::test_separate_mode_train_step_8192 (losses 2e-4 relative, pose gradients
2e-2 of the largest entry, composites 1e-3).  Shapes: 1027 rays = four full reduction blocks of 256 and a last one of 3, block 2 made of
frozen cameras only; 1 ray; 0 rays; 8 cameras, 4 per spectrum.  The whole step runs at 1028 rays: the training losses take batches of 2x2
pixel patches only (tn_train_losses refuses a ray count that is no multiple of 4), and 1028 is the nearest one -- still four full blocks and
a short last one."""
import types

import numpy as np
import pytest
import torch

import nerf_shared_pose_functional as fn
import thermal_nerfacto_oracle as orc
from helpers import make_params, tiny_cfg
from nerfstudio_thermal_amd import _lib, ops, synth
from nerfstudio_thermal_amd.arena import ParamArena
from nerfstudio_thermal_amd.config import CameraOptimizerConfig
from test_hip_ops_gpu import pkg_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 1027
STEP_N = 1028  # whole training steps: a multiple of 4 (2x2 patches)
IS_THERMAL = (0, 0, 0, 0, 1, 1, 1, 1)
# frozen masks by branch: the RGB branch's row leaves thermal cameras alone, the thermal branch's row RGB cameras
FROZEN = {"": torch.tensor(IS_THERMAL, dtype=torch.bool), "_thermal": ~torch.tensor(IS_THERMAL, dtype=torch.bool)}
SHARED_KEY = {"": "shared_camera_optimizer.pose_adjustment", "_thermal": "shared_camera_optimizer_thermal.pose_adjustment"}
POSE_KEY = {"": "camera_optimizer.pose_adjustment", "_thermal": "camera_optimizer_thermal.pose_adjustment"}


def g(x):
    return x.to(DEV).contiguous()


def md(a, b):
    return float((a.detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max())


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def rays_for(n, sfx):
    frozen = FROZEN[sfx]
    return fn.rays(n, frozen_block=(512, 768), frozen_cams=tuple(int(i) for i in torch.nonzero(frozen).reshape(-1)))


def per_camera_pose(seed=1):
    """[8,6] per-camera rows with rotations of ~0.2 rad: leaving R_c^T out of the pull-back moves the shared gradient by ~20 %"""
    return (0.2 * torch.randn(8, 6, generator=torch.Generator().manual_seed(seed))).contiguous()


# ------------------------------------------------------------------------------------------------ 1. tn_pose_shared_apply
@pytest.mark.parametrize("sfx", ["", "_thermal"])
@pytest.mark.parametrize("n", [N, 1, 0])
@pytest.mark.parametrize("row_name", ["zero", "tiny", "rig"])
def test_shared_apply_against_the_restatement(row_name, n, sfx):
    frozen = FROZEN[sfx]
    o, d, cam = rays_for(n, sfx)
    if n == 1:
        cam[:] = int(torch.nonzero(~frozen)[0])  # the one ray is a corrected one
    row = fn.rows(torch.float32)[row_name]
    fz8 = g(frozen.to(torch.uint8))
    got_o, got_d = ops.pose_shared_apply(g(row), fz8, g(cam), g(o), g(d))
    assert got_o.shape == (n, 3) and got_d.shape == (n, 3)
    if n == 0:
        return
    got_o, got_d = got_o.cpu(), got_d.cpu()
    fz = frozen[cam]
    # frozen rays come back bit-identical
    assert torch.equal(bits(got_o[fz]), bits(o[fz])) and torch.equal(bits(got_d[fz]), bits(d[fz]))
    # the others: 8 x the float32 restatement's own error against float64, on those rays
    r64 = fn.shared_apply(row.double(), frozen, cam, o.double(), d.double())
    r32 = fn.shared_apply(row, frozen, cam, o, d)
    live = ~fz
    base = max(md(r32[0][live], r64[0][live]), md(r32[1][live], r64[1][live]))
    err = max(md(got_o[live], r64[0][live]), md(got_d[live], r64[1][live]))
    print(f"shared apply {row_name} n={n} branch '{sfx}': kernel error {err:.3e}, float32 restatement error {base:.3e}")
    assert err <= 8 * base, (err, base)
    if row_name == "zero":
        assert torch.equal(got_o, o) and torch.equal(got_d, d)
    # bit-identical to the per-camera kernel fed the row tiled to [C,6]
    t_o, t_d = ops.pose_apply_fwd(g(row.expand(8, 6)), fz8, g(cam), g(o), g(d))
    assert torch.equal(bits(t_o.cpu()), bits(got_o)) and torch.equal(bits(t_d.cpu()), bits(got_d))


# ------------------------------------------------------------------------------------------------ 2. tn_pose_shared_bwd
def _bwd_inputs(n, sfx, seed=11):
    o, d, cam = rays_for(n, sfx)
    gen = torch.Generator().manual_seed(seed)
    return d, cam, torch.randn(n, 3, generator=gen), torch.randn(n, 3, generator=gen)


def _run_bwd(row, frozen, cam, d0, g_o, g_d, pose, grad=None):
    grad = torch.zeros(1, 6, device=DEV) if grad is None else grad
    ops.pose_shared_bwd(g(row), g(frozen.to(torch.uint8)), g(cam), g(d0), g(g_o), g(g_d), None if pose is None else g(pose), grad)
    return grad


@pytest.mark.parametrize("sfx", ["", "_thermal"])
@pytest.mark.parametrize("with_pose", [False, True])
@pytest.mark.parametrize("n", [N, 1])
@pytest.mark.parametrize("row_name", ["zero", "tiny", "rig"])
def test_shared_bwd_against_the_restatement(row_name, n, with_pose, sfx):
    frozen = FROZEN[sfx]
    d0, cam, g_o, g_d = _bwd_inputs(n, sfx)
    if n == 1:
        cam[:] = int(torch.nonzero(~frozen)[0])
    row = fn.rows(torch.float32)[row_name]
    pose = per_camera_pose() if with_pose else None
    o0 = torch.zeros_like(d0)  # (the gradient does not depend on the origins)
    got = _run_bwd(row, frozen, cam, d0, g_o, g_d, pose).cpu()
    r64 = fn.row_gradient(row.double(), None if pose is None else pose.double(), frozen, cam, o0.double(), d0.double(), g_o.double(), g_d.double())
    r32 = fn.row_gradient(row, pose, frozen, cam, o0, d0, g_o, g_d)
    base, err = md(r32, r64), md(got, r64)
    print(f"shared bwd {row_name} n={n} pose={with_pose} branch '{sfx}': kernel error {err:.3e}, float32 restatement error {base:.3e}, "
          f"largest entry {float(r64.abs().max()):.3e}")
    assert err <= 8 * base, (err, base)
    # the same inputs give the same bits
    again = _run_bwd(row, frozen, cam, d0, g_o, g_d, pose).cpu()
    assert torch.equal(bits(again), bits(got))
    # ... and the call ACCUMULATES: one float32 addition of the sum onto what the row's gradient held
    ones = _run_bwd(row, frozen, cam, d0, g_o, g_d, pose, grad=torch.ones(1, 6, device=DEV)).cpu()
    assert torch.equal(ones, torch.ones(1, 6) + got)


@pytest.mark.parametrize("with_pose", [False, True])
def test_shared_bwd_all_frozen_is_exactly_zero_and_empty_batch_touches_nothing(with_pose):
    d0, cam, g_o, g_d = _bwd_inputs(N, "")
    row, pose = fn.rows(torch.float32)["rig"], (per_camera_pose() if with_pose else None)
    got = _run_bwd(row, torch.ones(8, dtype=torch.bool), cam, d0, g_o, g_d, pose)
    assert torch.equal(got.cpu(), torch.zeros(1, 6))
    keep = torch.arange(6.0, device=DEV).reshape(1, 6) + 0.5
    got = _run_bwd(row, torch.ones(8, dtype=torch.bool), cam, d0, g_o, g_d, pose, grad=keep.clone())
    assert torch.equal(bits(got), bits(keep))
    e3, ei = torch.zeros(0, 3), torch.zeros(0, dtype=torch.int64)
    got = _run_bwd(row, FROZEN[""], ei, e3, e3, e3, pose, grad=keep.clone())
    assert torch.equal(bits(got), bits(keep))


# ------------------------------------------------------------------------------------------------ 3. / 4. a whole step on the engine's own bins
ROW = {"": fn.rows(torch.float32)["rig"],
       "_thermal": torch.tensor([[-0.03, 0.05, 0.02, 0.12, 0.21, -0.16]])}


def shared_cfg(ocfg, camera=True):
    cfg = pkg_cfg(ocfg)
    cfg.shared_camera_optimizer = CameraOptimizerConfig(mode="shared_SO3xR3", penalty_scale=1.0)
    cfg.shared_camera_optimizer_thermal = CameraOptimizerConfig(mode="shared_SO3xR3", penalty_scale=10.0)
    if not camera:
        cfg.camera_optimizer = CameraOptimizerConfig(mode="off")
        cfg.camera_optimizer_thermal = CameraOptimizerConfig(mode="off")
    return cfg


def step_rays(n=STEP_N):
    """n rays of the bench workload's kind (2x2 patches, grouped by camera): the first n of a 1056-ray batch -- 528 RGB rays, then the thermal
    ones (500 of them at n = 1028)"""
    cams = synth.synth_cameras()
    idx = synth.synth_ray_indices(cams, 1056, seed=42)[:n]
    t = lambda k: torch.from_numpy(cams[k])  # noqa: E731
    o, d, _, _ = orc.generate_rays(torch.from_numpy(idx), t("c2w"), t("fx"), t("fy"), t("cx"), t("cy"), t("distortion"))
    img, is_th = (torch.from_numpy(a) for a in synth.synth_gt(idx, cams, seed=42))
    return o, d, torch.from_numpy(idx[:, 0]).contiguous(), img, is_th


@pytest.mark.parametrize("mode,camera", [("separate", True), ("shared", True), ("separate", False)])
def test_whole_step_on_the_engines_bins(mode, camera):
    """The pattern of test_separate_mode_train_step_8192 at 1028 rays with both shared rows (and, camera=True, the per-camera rows) non-zero:
    the engine runs the training forward and loss_and_backward, the oracle is handed the engine's own bins and evaluates everything behind them.
    camera=False: the per-camera optimisers are off and the shared gradients must still arrive (d origins / d directions are produced).

    Identical samples on both sides, as in that test: a sample is origin + t * direction, so besides the engine's bins the oracle is handed
    the VALUES of the engine's corrected rays, with its own graph from the pose rows to the rays kept (value swap, derivative untouched).  In
    that test the rows are ~1e-3 rad, the pose map is all but the identity on both sides; with the rotations used here (0.15-0.3 rad)
    about half of the directions differ in their last bit between the kernels' float32 pose map and torch's, a handful of samples then fall
    into another hash-grid cell, and the comparison would measure that conditioning instead of the backward.  Measured on
    an MI355X with the oracle on its OWN float32 rays: pose gradients 0.5 % / 1.2 % / 0.7 % / 2.1 % of their largest entries (shared, shared
    thermal, per-camera, per-camera thermal; the oracle's own gradients move by 1.4 % / 1.3 % / 1.7 % / 2.6 % when its rays move by one
    float32 ulp); on the engine's rays: 1e-6 / 1.2e-4 / 2e-6 / 2.3e-4.  The rays themselves are held to the float64 restatement by the
    kernels' rule: 8 x the error of the float32 restatement."""
    from nerfstudio_thermal_amd.engine import RenderEngine

    ocfg = tiny_cfg(mode)
    params = make_params(ocfg)
    for k in POSE_KEY.values():
        params[k] = (params[k] * 150.0).contiguous()  # rotations of up to ~0.15 rad: the pull-back through R_c matters
    sfxs = ("", "_thermal") if mode == "separate" else ("",)
    for sfx in sfxs:
        params[SHARED_KEY[sfx]] = ROW[sfx].clone()
    cfg = shared_cfg(ocfg, camera)
    arena = ParamArena(cfg, ocfg.num_images, DEV)
    arena.load(params)
    eng = RenderEngine(cfg, arena, ocfg.num_images, list(ocfg.is_thermal_cam))
    o0, d0, cam, img, is_th = step_rays()
    jit = [torch.from_numpy(j).reshape(-1) for j in synth.synth_jitters(STEP_N)]
    jit_t = [torch.from_numpy(j).reshape(-1) for j in synth.synth_jitters(STEP_N, tag="_thermal")]
    eng.set_anneal_for_step(500)
    arena.zero_grad()
    out, branches = eng.get_outputs(g(o0), g(d0), g(cam), True, [g(j) for j in jit], [g(j) for j in jit_t])
    losses = eng.loss_and_backward(out, branches, g(cam), g(img), g(is_th))
    torch.cuda.synchronize()

    # ---- the oracle on the engine's bins
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    oo, rays = {}, {}
    for sfx in sfxs:
        fprefix, pprefix = "field" + sfx, "proposal_networks" + sfx
        pose = p[POSE_KEY[sfx]] if camera else None
        o, d = fn.composed_apply(p[SHARED_KEY[sfx]], pose, FROZEN[sfx], cam, o0, d0)
        # the engine's corrected rays against the float64 restatement: 8 x the float32 restatement's own error, origins and directions together
        eo, ed = branches[sfx].origins.detach().cpu(), branches[sfx].directions.detach().cpu()
        with torch.no_grad():
            o64, d64 = fn.composed_apply(p[SHARED_KEY[sfx]].double(), None if pose is None else pose.double(), FROZEN[sfx], cam, o0.double(), d0.double())
        base, err = max(md(o, o64), md(d, d64)), max(md(eo, o64), md(ed, d64))
        print(f"{mode} camera={camera} rays{sfx}: engine error {err:.3e}, float32 restatement error {base:.3e}; "
              f"directions that differ from the float32 restatement's in some bit: {int((ed != d.detach()).any(dim=1).sum())} of {len(d)}")
        assert err <= 8 * base, (sfx, err, base)
        # identical samples: the engine's ray values on the oracle's graph
        o, d = o + (eo - o.detach()), d + (ed - d.detach())
        rays[sfx] = (o, d)
        lv = branches[sfx].levels
        smp = [orc.Samples(s_bins=l.s_bins.detach().cpu(), e_bins=l.e_bins.detach().cpu()) for l in lv]
        wl = [orc.get_weights(smp[i].deltas, orc.prop_density(p, pprefix, i, ocfg, smp[i].positions(o, d))) for i in range(2)]
        dens, geo, _, _ = orc.field_density(p, fprefix, ocfg, smp[2].positions(o, d))
        rgb = orc.field_color(p, fprefix, ocfg, d, geo, cam, True)
        w = orc.get_weights(smp[2].deltas, dens)
        wl.append(w)
        oo[f"rgb{sfx}"] = orc.composite_rgb(rgb, w, True)
        oo[f"density{sfx}"] = dens
        oo[f"weights_list{sfx}"], oo[f"samples_list{sfx}"] = wl, smp
    if mode == "separate":
        oo["density2"] = orc.field_density(p, "field", ocfg, oo["samples_list_thermal"][2].positions(*rays["_thermal"]))[0]
        oo["density2_thermal"] = orc.field_density(p, "field_thermal", ocfg, oo["samples_list"][2].positions(*rays[""]))[0]
        comps = {"": oo["rgb"], "_thermal": oo["rgb_thermal"]}
    else:
        comps = {"": oo["rgb"]}
        oo["rgb"], oo["rgb_thermal"] = comps[""][..., :3], comps[""][..., 3:]
    ref_losses = orc.loss_dict(p, ocfg, oo, img, is_th, training=True)
    if not camera:
        for sfx in ("", "_thermal"):
            ref_losses.pop("camera_opt_regularizer" + sfx, None)
    for sfx in sfxs:
        sc = getattr(cfg, "shared_camera_optimizer" + sfx)
        ref_losses["camera_opt_regularizer_shared" + sfx] = fn.regularizer(p[SHARED_KEY[sfx]], sc.trans_l2_penalty, sc.rot_l2_penalty, sc.penalty_scale)
    sum(ref_losses.values()).backward()

    # ---- composites (1e-3), every loss key (2e-4 relative), the new regulariser keys
    for sfx in sfxs:
        got = out["rgbt"] if mode == "shared" else out[f"rgb{sfx}"]
        print(f"{mode} camera={camera} composite{sfx}: {md(got, comps[sfx]):.3e}")
        assert md(got, comps[sfx]) <= 1e-3, (sfx, md(got, comps[sfx]))
    assert sorted(losses) == sorted(ref_losses), (sorted(losses), sorted(ref_losses))
    assert {"camera_opt_regularizer_shared" + sfx for sfx in sfxs} <= set(losses)
    for k, v in ref_losses.items():
        a, b = float(losses[k]), float(v)
        print(f"{mode} camera={camera} loss {k}: {a:.6e} vs {b:.6e}")
        assert abs(a - b) <= 2e-4 * abs(b) + 1e-9, (k, a, b)
    # ---- the shared rows' and the per-camera rows' gradients (2e-2 of the largest entry)
    names = [SHARED_KEY[s] for s in sfxs] + ([POSE_KEY[s] for s in sfxs] if camera else [])
    for name in names:
        ref, got = p[name].grad, arena.grad_view(name)
        scale = float(ref.abs().max())
        print(f"{mode} camera={camera} grad {name}: error {md(got, ref):.3e}, largest entry {scale:.3e}")
        assert scale > 0 and md(got, ref) <= 2e-2 * scale, (name, md(got, ref), scale)


# ------------------------------------------------------------------------------------------------ 5.-7. the model
def build(mode, shared=True, camera=True):
    """shared: True = both shared optimisers on; False = the default configuration (off by penalty_scale = -1); "off" = off by the mode of that name"""
    from nerfstudio_thermal_amd.model import SceneBox

    ocfg = tiny_cfg(mode)
    cfg = shared_cfg(ocfg, camera) if shared is True else pkg_cfg(ocfg)
    if shared == "off":
        cfg.shared_camera_optimizer = CameraOptimizerConfig(mode="off")
        cfg.shared_camera_optimizer_thermal = CameraOptimizerConfig(mode="off")
    model = cfg.setup(scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1, -1], [1, 1, 1]])), num_train_data=ocfg.num_images,
                      metadata={"is_thermal": list(ocfg.is_thermal_cam)}, device=DEV)
    model.arena.load(make_params(ocfg))
    return ocfg, model


def small_camera(c, H=12, W=16):
    cams = synth.synth_cameras()
    s = W / float(cams["width"][c])
    return types.SimpleNamespace(camera_to_worlds=torch.from_numpy(cams["c2w"][c]), fx=float(cams["fx"][c]) * s, fy=float(cams["fy"][c]) * s,
                                 cx=W / 2.0, cy=H / 2.0, width=W, height=H, camera_index=c)


def same_bits(a, b, keys):
    for k in keys:
        assert torch.equal(bits(a[k]), bits(b[k])), k


def test_eval_render_applies_the_shared_rows_by_camera_index():
    """A 16 x 12 frame of RGB camera 1 in separate mode: the RGB branch renders the corrected rays, the thermal branch -- whose row is frozen on
    RGB cameras -- the uncorrected ones; with the rows at exactly 0 the render is the one of a model without the switch."""
    from nerfstudio_thermal_amd.rays import RayBundle

    _, model = build("separate")
    _, plain_model = build("separate", shared=False)
    model.eval(), plain_model.eval()
    cam = small_camera(1)
    rgb_keys, th_keys = ("rgb", "depth", "accumulation", "expected_depth"), ("rgb_thermal", "depth_thermal", "accumulation_thermal")
    rows = {sfx: model.arena.view(SHARED_KEY[sfx]) for sfx in ("", "_thermal")}
    for sfx in rows:
        rows[sfx].copy_(g(ROW[sfx]))
    A = model.get_outputs_for_camera(cam)
    for sfx in rows:
        rows[sfx].zero_()
    B = model.get_outputs_for_camera(cam)
    # the hand-corrected rays through the model with the rows zeroed
    H, W = cam.height, cam.width
    yy, xx = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    idx = torch.stack([torch.zeros(H * W, dtype=torch.int64, device=DEV), yy.reshape(-1), xx.reshape(-1)], dim=1).contiguous()
    f = lambda v: torch.tensor([v], dtype=torch.float32, device=DEV)  # noqa: E731
    o, d, area, _ = ops.raygen(idx, g(cam.camera_to_worlds).reshape(1, 3, 4), f(cam.fx), f(cam.fy), f(cam.cx), f(cam.cy), None)
    cidx = torch.full((H * W,), 1, dtype=torch.int64, device=DEV)
    o1, d1 = ops.pose_shared_apply(g(ROW[""]), g(FROZEN[""].to(torch.uint8)), cidx, o, d)
    assert md(d1, d) > 1e-2  # (camera 1 is an RGB camera: the RGB branch's row corrects it)
    Cc = model.get_outputs_for_camera_ray_bundle(RayBundle(origins=o1.view(H, W, 3), directions=d1.view(H, W, 3), pixel_area=area.view(H, W, 1),
                                                           camera_indices=cidx.view(H, W, 1)))
    same_bits(A, Cc, rgb_keys)   # corrected branch = the render of the hand-corrected rays
    same_bits(A, B, th_keys)     # a frozen camera index renders uncorrected
    assert md(A["rgb"], B["rgb"]) > 0
    # thermal camera 5: the other way round
    for sfx in rows:
        rows[sfx].copy_(g(ROW[sfx]))
    A5 = model.get_outputs_for_camera(small_camera(5))
    for sfx in rows:
        rows[sfx].zero_()
    B5 = model.get_outputs_for_camera(small_camera(5))
    same_bits(A5, B5, rgb_keys)
    assert md(A5["rgb_thermal"], B5["rgb_thermal"]) > 0
    # rows at exactly 0 = the render of a model without the switch
    P = plain_model.get_outputs_for_camera(cam)
    assert set(P) == set(B)
    same_bits(B, P, sorted(P))


class _Recorder:
    """the C library behind a proxy that notes the name of every entry point called"""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn_ = getattr(self._lib, name)
        if not name.startswith("tn_"):
            return fn_

        def call(*a):
            self._log.append(name)
            return fn_(*a)

        return call


def _train_batch():
    from nerfstudio_thermal_amd.rays import RayBundle

    o, d, cam, img, is_th = step_rays(1024)
    rb = RayBundle(origins=g(o), directions=g(d), pixel_area=torch.ones(1024, 1, device=DEV), camera_indices=g(cam)[:, None])
    return rb, {"image": g(img), "is_thermal": g(is_th)}


def _recorded_steps(monkeypatch, model, steps=3):
    from nerfstudio_thermal_amd.optim import DeviceGradScaler

    rb, batch = _train_batch()
    model.train()
    scaler = DeviceGradScaler(model.device, num_groups=len(model.arena.optimised_groups))
    log = []
    real = _lib.load()
    monkeypatch.setattr(_lib, "_lib", _Recorder(real, log))
    try:
        for step in range(steps):
            model.train_iteration(rb, batch, step, grad_scaler=scaler)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(_lib, "_lib", real)
    return log


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_adam_step_moves_the_rows_and_the_switch_off_keeps_the_call_sequence(mode, monkeypatch):
    """One fused training iteration moves every shared row (Adam at the camera optimisers' rate).  Switch off: the sequence of library calls of
    three training iterations is the same whether the shared optimisers are off by the default's penalty_scale = -1 or by mode "off", names no
    shared-pose entry point, and in shared-density mode is still the one-call step.  (Two runs of a step do not give the same parameter bits --
    float atomics in the table scatters, see tests/test_trainer_sequence_gpu.py -- so the calls are compared, not the parameters.)"""
    ocfg, on = build(mode)
    sfxs = ("", "_thermal") if mode == "separate" else ("",)
    assert all(float(on.arena.view(SHARED_KEY[s]).abs().max()) == 0.0 for s in sfxs)
    log_on = _recorded_steps(monkeypatch, on, steps=1)
    for s in sfxs:
        row = on.arena.view(SHARED_KEY[s]).cpu()
        assert bool(torch.isfinite(row).all()) and float(row.abs().min()) > 0 and float(row.abs().max()) <= 1.001e-3, (s, row)
    assert log_on.count("tn_pose_shared_apply") == len(sfxs) and log_on.count("tn_pose_shared_bwd") == len(sfxs) and "tn_train_step" not in log_on
    _, default = build(mode, shared=False)
    _, off = build(mode, shared="off")
    log_default, log_off = _recorded_steps(monkeypatch, default), _recorded_steps(monkeypatch, off)
    assert log_default == log_off
    assert not any("pose_shared" in n for n in log_default)
    if mode == "shared":
        assert [n for n in log_default if not n.endswith("_bytes") and not n.endswith("_layout")].count("tn_train_step") == 3


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_model_groups_keys_trainer_path_and_state_dict(mode):
    """get_param_groups / get_loss_dict / get_metrics_dict carry the shared optimisers' entries (the thermal ones in separate mode only), an
    autograd step through Optimizers moves the rows, and the state dict round-trips the new keys."""
    from nerfstudio_thermal_amd.optim import Optimizers
    from test_model_api_gpu import _trainer_step

    ocfg, model = build(mode)
    sfxs = ("", "_thermal") if mode == "separate" else ("",)
    groups = model.get_param_groups()
    for s in ("", "_thermal"):
        assert (("shared_camera_opt" + s) in groups) == (s in sfxs)
        assert ((SHARED_KEY[s]) in model.state_dict()) == (s in sfxs)
    for s in sfxs:
        assert [tuple(p.shape) for p in groups["shared_camera_opt" + s]] == [(1, 6)]
    assert list(groups)[-len(sfxs):] == ["shared_camera_opt" + s for s in sfxs]
    model.train()
    rb, batch = _train_batch()
    opt = Optimizers(groups)
    losses = _trainer_step(model, opt, rb, batch, 0)
    out = model.get_outputs(model.collider(rb[...]))
    metrics = model.get_metrics_dict(out, batch)
    for s in ("", "_thermal"):
        present = s in sfxs
        assert (("camera_opt_regularizer_shared" + s) in losses) == present
        assert (("camera_opt_translation_shared" + s) in metrics) == present and (("camera_opt_rotation_shared" + s) in metrics) == present
    for s in sfxs:
        row = model.arena.view(SHARED_KEY[s]).cpu()
        assert float(row.abs().min()) > 0 and float(row.abs().max()) <= 1.001e-3, (s, row)  # one Adam step at lr 1e-3
        assert float(metrics["camera_opt_translation_shared" + s]) == pytest.approx(float(row[:, :3].norm()), rel=1e-5)
    # evaluation: the loss keys are there too (the reference adds them outside `if self.training`)
    model.eval()
    with torch.no_grad():
        ev = model.get_outputs(model.collider(rb[...]))
        ev_losses = model.get_loss_dict(ev, batch, model.get_metrics_dict(ev, batch))
    assert {"camera_opt_regularizer_shared" + s for s in sfxs} <= set(ev_losses)
    assert not any(k.startswith("camera_opt_regularizer") and "shared" not in k for k in ev_losses)
    # state dict round trip
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    _, other = build(mode)
    other.load_state_dict(sd)
    for s in sfxs:
        assert torch.equal(other.arena.view(SHARED_KEY[s]), model.arena.view(SHARED_KEY[s]))
        assert float(other.arena.view(SHARED_KEY[s]).abs().max()) > 0
    # correction matrices: identity rows on the frozen cameras, the row's [R | t] on the others
    m = model.shared_camera_optimizer.get_correction_matrices().cpu()
    ref = orc.exp_map_so3xr3(model.arena.view(SHARED_KEY[""]).cpu())[0]
    assert m.shape == (8, 3, 4) and torch.equal(m[4:], torch.eye(4)[None, :3, :4].expand(4, 3, 4)) and md(m[:4], ref[None].expand(4, 3, 4)) <= 1e-6
