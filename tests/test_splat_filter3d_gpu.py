"""Mip-Splatting's 3D smoothing filter on the GPU: tn_filter3d_splat_compute / _apply / _apply_backward against the float64 restatement
(splat_filter3d_functional.py), and ThermalSplatfactoModel's use_3d_filter through renders, refinement, export and a short training run.

Tolerances.  Compute and apply forward: 1 float32 ulp of the float64 restatement rounded to float32 -- the kernels evaluate in double and round
once, so only a rounding tie flipped by the last bit of a device exp / log can differ.  The compute test first asserts, on the CPU, that no
Gaussian of its scene lies within 1e-4 (relative) of a visibility boundary, so that no flip of a visibility decision can hide behind that
tolerance.  Apply backward: |err| <= 2^-22 x the sum of the absolute terms of the closed form.  Everything about the model is bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

import splat_filter3d_functional as ff
import splat_functional as sf
import splat_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 1037  # a ragged last wave and a ragged last block of 256
NEAR, VARIANCE = 0.2, 0.2
RGB_SIZE, THERMAL_SIZE = (96, 72, 100.0), (48, 36, 25.0)  # width, height, focal length in pixels: the sampling rates differ by 4 x


def _mods():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import optim, splat, splat_calls, splat_filter, splat_io

    return splat, optim, splat_calls, splat_filter, splat_io


def _ulp_ok(got32: np.ndarray, ref64: np.ndarray) -> bool:
    ref32 = ref64.astype(np.float32)
    return bool(np.all(np.abs(got32.astype(np.float64) - ref32.astype(np.float64)) <= np.spacing(np.abs(ref32)).astype(np.float64)))


# ------------------------------------------------------------------------------------------------ the filter value
def filter_scene(C: int):
    """(means [N,3] fp32, camera table [C,18] fp32) on the host: C cameras in a cluster on the +x side looking towards the origin, "RGB" (even
    rows) and "thermal" (odd rows) intrinsics alternating, and N Gaussians in a box that reaches behind the cluster and far to its sides.  A
    Gaussian drawn within 2e-4 (relative) of a visibility boundary of any camera is drawn again: with 300 cameras there are 1.5 million boundaries,
    and no seed keeps every Gaussian off all of them."""
    from nerfstudio_thermal_amd.splat import PinholeCamera
    from nerfstudio_thermal_amd.splat_filter import filter_camera_table

    rng = np.random.default_rng(1000 + C)
    cams = []
    for i in range(C):
        W, H, f = THERMAL_SIZE if i % 2 else RGB_SIZE
        eye = (3.0 + rng.uniform(-0.3, 0.3), rng.uniform(-1.0, 1.0), rng.uniform(-0.5, 0.5))
        target = tuple(rng.uniform(-0.3, 0.3, 3))
        cams.append(PinholeCamera(so.look_at_camera(eye, target), f, f * 1.01, W / 2, H / 2, W, H, cam_idx=i, is_thermal=bool(i % 2)))
    lo, hi = np.array([-4.0, -8.0, -6.0]), np.array([6.0, 8.0, 6.0])
    means = torch.from_numpy(rng.uniform(lo, hi, (N, 3)).astype(np.float32))
    table = filter_camera_table(cams)
    for _ in range(100):
        close = ff.boundary_distance(means, table, NEAR) < 2e-4
        if not bool(close.any()):
            break
        means[close] = torch.from_numpy(rng.uniform(lo, hi, (int(close.sum()), 3)).astype(np.float32))
    return means, table


def scene_census(means, table):
    """how many Gaussians are: behind every camera | seen only by thermal cameras | seen, but by no camera inside its frame | seen by none"""
    seen, in_frame, _ = ff.visibility(means, table, NEAR)
    _, _, z, _ = ff._camera_space(means, table)
    thermal = torch.arange(table.shape[0]) % 2 == 1
    any_seen = seen.any(1)
    return {"behind": int((z <= 0).all(1).sum()), "thermal_only": int((seen[:, thermal].any(1) & ~seen[:, ~thermal].any(1)).sum()),
            "margin_only": int((any_seen & ~in_frame.any(1)).sum()), "none": int((~any_seen).sum()), "seen": int(any_seen.sum())}


@pytest.mark.parametrize("C", [1, 5, 300])  # 300: more cameras than one staging chunk (128) holds
def test_compute_matches_the_restatement(C):
    _, _, _, splat_filter, _ = _mods()
    means, table = filter_scene(C)
    census = scene_census(means, table)
    print(f"C = {C}: {census}, smallest boundary distance {float(ff.boundary_distance(means, table, NEAR).min()):.3e}")
    assert census["behind"] >= 20 and census["margin_only"] >= 1 and census["none"] >= 20 and census["seen"] >= 50
    if C > 1:  # (the single camera is an RGB one)
        assert census["thermal_only"] >= 20
    assert float(ff.boundary_distance(means, table, NEAR).min()) > 1e-4  # a condition on the inputs: no visibility decision is a near-tie
    ref = ff.compute_filter(means, table, NEAR, VARIANCE).numpy()
    assert (ref > 0).all()
    got = splat_filter.compute_3d_filter(means.to(DEV), table.to(DEV), NEAR, VARIANCE)
    again = splat_filter.compute_3d_filter(means.to(DEV), table.to(DEV), NEAR, VARIANCE)
    assert got.shape == (N,) and got.dtype == torch.float32
    assert _ulp_ok(got.cpu().numpy(), ref)
    assert torch.equal(got, again)  # the same bits on every run
    seen = ff.visibility(means, table, NEAR)[0].any(1)
    assert float(got[~seen.to(DEV)].min()) == float(got.max())  # unseen rows: the largest filter of the seen ones


def test_nothing_seen_switches_the_filter_off():
    _, _, _, splat_filter, _ = _mods()
    means, table = filter_scene(5)
    away = means + torch.tensor([100.0, 0.0, 0.0])  # everything behind every camera
    assert scene_census(away, table)["seen"] == 0
    got = splat_filter.compute_3d_filter(away.to(DEV), table.to(DEV), NEAR, VARIANCE)
    assert got.shape == (N,) and not got.any()
    none = splat_filter.compute_3d_filter(means.to(DEV), table[:0].to(DEV), NEAR, VARIANCE)  # no cameras at all
    assert none.shape == (N,) and not none.any()
    assert splat_filter.compute_3d_filter(means[:0].to(DEV), table.to(DEV)).shape == (0,)


# ------------------------------------------------------------------------------------------------ applying it
RATIOS = (0.0, 1e-4, 1.0, 1e4)  # f / s_0: off, far below the scale, at it, far above
LOG_SCALES = (-12.0, None, 3.0)  # None: random in [-6, 0.5]
LOGITS = (-30.0, 0.0, 30.0, None)  # None: random in [-6, 6]


@functools.lru_cache(maxsize=None)
def apply_rows():
    """N rows that cycle through every combination of RATIOS x LOG_SCALES x LOGITS x LOGITS (thermal), the other two axes of the log-scale a
    little off the first; upstream gradients random normal.  Host float32 tensors."""
    rng = np.random.default_rng(77)
    i = np.arange(N)
    pick = lambda table, idx, lo, hi: np.array([rng.uniform(lo, hi) if table[j] is None else table[j] for j in idx])  # noqa: E731
    ls0 = pick(LOG_SCALES, (i // 4) % 3, -6.0, 0.5)
    scales = np.stack([ls0, ls0 + rng.uniform(-0.5, 0.5, N), ls0 + rng.uniform(-0.5, 0.5, N)], -1).astype(np.float32)
    o = pick(LOGITS, (i // 12) % 4, -6.0, 6.0).astype(np.float32).reshape(N, 1)
    oth = pick(LOGITS, (i // 48) % 4, -6.0, 6.0).astype(np.float32).reshape(N, 1)
    f = (np.array(RATIOS)[i % 4] * np.exp(scales[:, 0].astype(np.float64))).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    ups = [t(rng.standard_normal(s).astype(np.float32)) for s in ((N, 3), (N, 1), (N, 1))]
    return t(scales), t(o), t(oth), t(f), ups


@functools.lru_cache(maxsize=None)
def apply_reference(sep: bool):
    scales, o, oth, f, ups = apply_rows()
    fwd = ff.apply_forward(scales, o, f, oth if sep else None)
    bwd, terms = ff.apply_backward(scales, o, f, ups[0], ups[1], oth if sep else None, ups[2] if sep else None)
    return fwd, bwd, terms


@pytest.mark.parametrize("sep", [False, True])
def test_apply_forward_and_backward_match_the_restatement(sep):
    _, _, _, splat_filter, _ = _mods()
    scales, o, oth, f, ups = apply_rows()
    fwd, bwd, terms = apply_reference(sep)
    off = f == 0
    assert int(off.sum()) >= 250 and all(bool(torch.isfinite(t).all()) for t in fwd + bwd)
    leaves = [t.to(DEV).requires_grad_(True) for t in ((scales, o, oth) if sep else (scales, o))]
    outs = splat_filter.apply_3d_filter(leaves[0], leaves[1], f.to(DEV), leaves[2] if sep else None)
    assert len(outs) == len(leaves)
    grads = torch.autograd.grad(outs, leaves, [u.to(DEV) for u in ups[:len(outs)]])
    for name, got, ref, src in zip(("scales", "opacities", "opacities_thermal"), outs, fwd, (scales, o, oth)):
        got = got.detach().cpu()
        assert got.shape == src.shape and _ulp_ok(got.numpy(), ref.numpy()), name
        assert torch.equal(got[off], src[off]), name  # f == 0: the row itself
        assert not torch.equal(got[~off], src[~off]), name
    for name, got, ref, t, up in zip(("scales", "opacities", "opacities_thermal"), grads, bwd, terms, ups):
        got = got.cpu()
        err = (got.double() - ref).abs()
        print(f"{name} gradient ({'separate' if sep else 'shared'}): largest |err| / sum of |terms| = {float((err / t.clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= 2.0 ** -22 * t).all()), name
        assert torch.equal(got[off], up[off]), name  # f == 0: the upstream gradient itself
    for leaf, src in zip(leaves, (scales, o, oth)):
        assert torch.equal(leaf.detach().cpu(), src)  # inputs untouched


# ------------------------------------------------------------------------------------------------ the model
W, H = 96, 72


def _camera(eye, thermal=False, idx=None):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    w, h = (W // 2, H // 2) if thermal else (W, H)
    fx = sf.fov_focal(w)
    return PinholeCamera(so.look_at_camera(eye), fx, fx, w / 2, h / 2, w, h, cam_idx=idx, is_thermal=thermal)


def _model(params, seed=0, **cfg_kw):
    splat = _mods()[0]
    m = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(**cfg_kw), num_points=4, device=DEV, seed=seed, num_train_data=3)
    m.load_gaussians(params)
    return m


def _gaussians(n, seed, sep):
    p = so.synth_gaussians(n, seed=seed, extent=1.0, scale_range=(-4.5, -2.0))
    if sep:
        p["opacities_thermal"] = p["opacities"].flip(0).clone()
    return p


EYES = ((2.4, 0.5, 0.7), (-0.6, 2.3, 0.5), (0.4, -2.2, 1.0))


def _cameras():
    """three RGB cameras and two thermal ones at half the resolution: the training rig"""
    return [_camera(e, idx=i) for i, e in enumerate(EYES)] + [_camera(e, thermal=True) for e in ((2.2, -0.8, 0.4), (-1.0, -2.0, 0.8))]


def _same_frame(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _mode(sep):
    return {"thermal_opacity_mode": "separate" if sep else "shared"}


@pytest.mark.parametrize("sep", [False, True])
def test_without_cameras_the_render_is_the_plain_one(sep):
    p = _gaussians(400, 41, sep)
    plain, filt = _model(p, sh_degree=3, **_mode(sep)), _model(p, sh_degree=3, use_3d_filter=True, **_mode(sep))
    assert "filter_3D" in dict(filt.named_buffers()) and not any("filter_3D" in k for k in filt.state_dict())
    assert not hasattr(plain, "filter_3D")
    assert all(q is not filt.filter_3D for ps in filt.get_param_groups().values() for q in ps)
    cam = _camera(EYES[0])
    _same_frame(plain.get_outputs(cam), filt.get_outputs(cam))
    a, b = plain.get_train_outputs(cam), filt.get_train_outputs(cam)
    _same_frame({k: v.detach() for k, v in a.items()}, {k: v.detach() for k, v in b.items()})
    assert filt.filter_3D.shape == (400,) and not filt.filter_3D.any() and filt.filter_refreshes == 0


@pytest.mark.parametrize("sep", [False, True])
def test_with_cameras_the_render_is_that_of_the_filtered_parameters(sep):
    _, _, splat_calls, splat_filter, _ = _mods()
    p = _gaussians(400, 42, sep)
    cams = _cameras()
    filt = _model(p, sh_degree=3, use_3d_filter=True, **_mode(sep))
    filt.set_filter_cameras(cams)
    raw = {k: v.to(DEV) for k, v in p.items()}
    f = splat_filter.compute_3d_filter(raw["means"], splat_filter.filter_camera_table(cams, DEV), filt.config.filter_3d_near, filt.config.filter_3d_variance)
    assert bool((f > 0).all())
    with torch.no_grad():
        out = splat_filter.apply_3d_filter(raw["scales"], raw["opacities"], f, raw["opacities_thermal"] if sep else None)
    fused = {**raw, "scales": out[0], "opacities": out[1], **({"opacities_thermal": out[2]} if sep else {})}
    assert not torch.equal(fused["scales"], raw["scales"]) and not torch.equal(fused["opacities"], raw["opacities"])
    plain = _model(fused, sh_degree=3, **_mode(sep))
    for cam in (cams[0], cams[3]):
        _same_frame(plain.get_outputs(cam), filt.get_outputs(cam))
    assert torch.equal(filt.filter_3D, f) and filt.filter_refreshes == 1
    _same_frame({k: v.detach() for k, v in fused.items()}, filt.filtered_gaussians())
    # the training render and its gradients
    g = torch.Generator(device=DEV).manual_seed(3)
    wts = None
    grads = []
    for m in (plain, filt):
        o = m.get_train_outputs(cams[1])
        if wts is None:
            wts = {k: torch.randn(o[k].shape, device=DEV, generator=g) for k in ("rgb", "thermal", "accumulation")}
        sum((o[k] * wts[k]).sum() for k in wts).backward()
        grads.append({k: m.gauss_params[k].grad.clone() for k in m.param_names})
        grads[-1]["frame"] = {k: o[k].detach() for k in o}
    _same_frame(grads[0].pop("frame"), grads[1].pop("frame"))
    gp, gf = grads
    touched = ("scales", "opacities", "opacities_thermal")
    for k in gp:
        if k not in touched:
            assert torch.equal(gp[k], gf[k]), k
    v_s, v_o = torch.empty_like(gp["scales"]), torch.empty_like(gp["opacities"])
    v_th = torch.empty_like(gp["opacities"]) if sep else None
    splat_calls.filter3d_apply_backward(raw["scales"], raw["opacities"], f, gp["scales"], gp["opacities"], v_s, v_o,
                                        raw["opacities_thermal"] if sep else None, gp["opacities_thermal"] if sep else None, v_th)
    assert torch.equal(gf["scales"], v_s) and torch.equal(gf["opacities"], v_o) and not torch.equal(gf["scales"], gp["scales"])
    if sep:
        assert torch.equal(gf["opacities_thermal"], v_th)
    assert filt.filter_refreshes == 1  # nothing changed: no second compute
    filt.set_filter_cameras(None)  # the cameras taken away: the plain render of the raw parameters again
    _same_frame(_model(p, sh_degree=3, **_mode(sep)).get_outputs(cams[0]), filt.get_outputs(cams[0]))
    assert not filt.filter_3D.any()


def test_the_buffer_follows_a_densify_and_cull_step():
    _, _, _, splat_filter, _ = _mods()
    n = 400
    p = _gaussians(n, 43, False)
    p["opacities"][:60] = -6.0  # culled
    p["scales"][60:200] = math.log(0.005)  # duplicated; the others are split
    m = _model(p, sh_degree=3, use_3d_filter=True)
    cams = _cameras()
    m.set_filter_cameras(cams)
    m.get_outputs(cams[0])
    assert m.filter_3D.shape == (n,) and m.filter_refreshes == 1
    m.xys_grad_norm, m.vis_counts, m.max_2Dsize = torch.ones(n, device=DEV), torch.ones(n, device=DEV), torch.zeros(n, device=DEV)
    m.last_size, m.step = (H, W), 600
    m.refinement_after(None, 600)
    n_split, n_orig, n_child, n_dup = m.last_refine_counts
    assert n_split > 0 and n_dup > 0 and n_orig < n and m.num_points == n_orig + n_child + n_dup != n
    out = m.get_train_outputs(cams[1])  # must not read the old buffer
    assert m.filter_3D.shape == (m.num_points,) and m.filter_refreshes == 2
    fresh = splat_filter.compute_3d_filter(m.means.detach(), splat_filter.filter_camera_table(cams, DEV), m.config.filter_3d_near,
                                           m.config.filter_3d_variance)
    assert torch.equal(m.filter_3D, fresh)
    (out["rgb"].sum() + out["thermal"].sum()).backward()
    assert m.gauss_params["scales"].grad.shape == (m.num_points, 3)
    m.load_gaussians(_gaussians(123, 44, False))  # other Gaussians altogether
    m.get_outputs(cams[0])
    assert m.filter_3D.shape == (123,) and m.filter_refreshes == 3


@pytest.mark.parametrize("sep", [False, True])
def test_the_export_fuses_the_filter(sep, tmp_path):
    _, _, _, _, splat_io = _mods()
    p = _gaussians(300, 45, sep)
    cams = _cameras()
    filt = _model(p, sh_degree=3, use_3d_filter=True, **_mode(sep))
    filt.set_filter_cameras(cams)
    info = splat_io.export_gaussian_ply(filt, str(tmp_path / "fused.ply"))
    assert info["exported"] == 300
    plain = _model(_gaussians(4, 1, sep), sh_degree=3, **_mode(sep))
    splat_io.load_gaussian_ply(plain, str(tmp_path / "fused.ply"))
    _same_frame(plain.get_outputs(cams[0]), filt.get_outputs(cams[0]))
    splat_io.export_gaussian_ply(filt, str(tmp_path / "raw.ply"), fuse_3d_filter=False)
    raw, _ = splat_io.read_gaussian_ply(str(tmp_path / "raw.ply"))
    for k in filt.param_names:
        assert torch.equal(raw[k], p[k]), k
    fused, _ = splat_io.read_gaussian_ply(str(tmp_path / "fused.ply"))
    assert not torch.equal(fused["scales"], p["scales"]) and torch.equal(fused["means"], p["means"])


def test_thirty_training_steps_with_the_filter_on():
    from nerfstudio_thermal_amd.model import TrainingCallbackLocation as L

    _, optim, _, _, _ = _mods()
    cams = _cameras()
    teacher = _model(_gaussians(400, 31, False), sh_degree=3)
    teacher.step = 10 ** 6
    gts = [teacher.get_outputs(c)["rgb"].clone() for c in cams[:3]]
    m = _model(_gaussians(300, 32, False), seed=5, sh_degree=3, use_3d_filter=True, filter_3d_every=10)
    m.set_filter_cameras(cams)
    opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=optim.HipAdam)
    assert "filter_3D" not in opts.optimizers
    cbs = m.get_training_callbacks(opts)
    losses = []
    for step in range(30):
        for cb in cbs:
            cb.run_callback_at_location(step, L.BEFORE_TRAIN_ITERATION)
        opts.zero_grad_all()
        loss = m.get_loss_dict(m.get_train_outputs(cams[step % 3]), {"image": gts[step % 3], "is_thermal": False})
        functools.reduce(torch.add, loss.values()).backward()
        opts.optimizer_step_all()
        opts.scheduler_step_all()
        for cb in cbs:
            cb.run_callback_at_location(step, L.AFTER_TRAIN_ITERATION)
        losses.append(float(loss["main_loss"].detach()))
    print("main_loss, steps 0-2 and 27-29:", losses[:3], losses[-3:])
    assert all(math.isfinite(v) for v in losses)
    assert all(losses[27 + i] < losses[i] for i in range(3))  # lower at the end, camera by camera
    assert m.filter_refreshes == 3 and m.filter_3D.shape == (m.num_points,)  # steps 0, 10 and 20
