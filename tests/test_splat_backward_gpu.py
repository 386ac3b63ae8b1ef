"""The splat backward on the GPU (get_train_outputs -> tn_splat_raster_backward / tn_splat_project_backward): HIP gradients of every
parameter and of xys against float64 autograd of the functional restatement (tests/splat_functional.py), bit-identity of the training
render with the eval render, bit-reproducibility, edge cases, a small fit, and a 1080p / 1 M Gaussian smoke."""
import math

import pytest
import torch

import splat_functional as sf
import splat_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(params, sh_degree, mode="classic", white=False, bg_thermal=0.3):
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

    cfg = ThermalSplatfactoModelConfig(sh_degree=sh_degree, sh_degree_interval=1, rasterize_mode=mode, background_color="white" if white else "black",
                                       background_thermal=bg_thermal)
    m = ThermalSplatfactoModel(cfg, num_points=4, device=DEV)
    m.load_gaussians(params)
    m.step = 10**6
    return m


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _camera(c2w, fx, cx, cy, W, H):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    return PinholeCamera(c2w, fx, fx, cx, cy, W, H)


def _hip_grads(m, cam, w):
    m.zero_grad(set_to_none=True)
    out = m.get_train_outputs(cam)
    loss = sum((out[k] * w[k].to(DEV)).sum() for k in w)
    loss.backward()
    g = {k: m.gauss_params[k].grad.detach().cpu().clone() for k in sf.PARAM_NAMES}
    g["xys"] = m.last_xys_grad.detach().cpu().clone()
    return g, out


@pytest.mark.parametrize("sh_degree", [0, 1, 3])
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("white", [False, True])
def test_gradients_match_autograd_of_the_restatement(sh_degree, mode, white):
    seed = 10 * sh_degree + (mode == "antialiased") * 2 + int(white)
    p = sf.scene(200, seed, sh_degree)
    W, H = 64, 48
    fx = sf.fov_focal(W)
    c2w = so.look_at_camera((2.3, 0.4 - 0.2 * sh_degree, 0.6))
    cx, cy = 31.5, 23.0
    bg = torch.ones(3) if white else torch.zeros(3)
    deg = sh_degree if sh_degree > 0 else -1
    # float64 reference; pixels where float32 / float64 could disagree on a discrete decision get no upstream gradient (in both)
    leaves = {k: v.double().requires_grad_(True) for k, v in p.items()}
    ref_out = sf.render(leaves, c2w, fx, fx, cx, cy, W, H, sh_degree_to_use=deg, rasterize_mode=mode, background=bg, background_thermal=0.3)
    ref_out["xys"].retain_grad()
    gen = torch.Generator().manual_seed(seed)
    keep = (~ref_out["flag_pixels"]).double()[..., None]
    w = {k: torch.randn(H, W, c, generator=gen, dtype=torch.float64) * keep for k, c in (("rgb", 3), ("thermal", 1), ("accumulation", 1))}
    sum((ref_out[k] * w[k]).sum() for k in w).backward()
    ref = {k: leaves[k].grad.float() for k in sf.PARAM_NAMES}
    ref["xys"] = ref_out["xys"].grad.float()
    m = _model(p, sh_degree, mode, white)
    hip, out = _hip_grads(m, _camera(c2w, fx, cx, cy, W, H), {k: v.float() for k, v in w.items()})
    assert float(ref_out["accumulation"].detach().max()) > 0.5
    # Gaussians kept out of the comparison: a flagged pair, an SH value or a view-space position on a clamp, a knife-edge radius
    radii_hip = m.last_projection["radii"].cpu()
    excl = ref_out["flag_gaussians"] | ((radii_hip > 0) != (ref_out["projection"]["radii"] > 0))
    n_excl, n_pix = int(excl.sum()), int(ref_out["flag_pixels"].sum())
    print(f"near-threshold: {n_excl} Gaussians excluded, {n_pix} pixels without upstream gradient")
    assert n_excl <= 0.01 * p["means"].shape[0], n_excl
    for k in list(sf.PARAM_NAMES) + ["xys"]:
        a, b = hip[k][~excl], ref[k][~excl]
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), k
        scale = _amax(b)
        if scale == 0.0:
            assert _amax(a) == 0.0, k
            continue
        err = float((a - b).abs().max())
        assert err <= 2e-4 * scale, (k, err, scale)
        na, nb = float(a.norm()), float(b.norm())
        assert abs(na - nb) <= 1e-4 * nb, (k, na, nb)
    # culled Gaussians get exactly zero
    culled = radii_hip == 0
    for k in sf.PARAM_NAMES:
        assert _amax(hip[k][culled]) == 0.0, k


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_train_render_is_bit_identical_to_the_eval_render(mode):
    p = so.synth_gaussians(3000, seed=3, extent=1.0)
    m = _model(p, 3, mode, white=True)
    cam = _camera(so.look_at_camera((2.6, 0.4, 0.9)), 170.0, 81.0, 58.5, 160, 120)
    ev = m.get_outputs(cam)
    tr = m.get_train_outputs(cam)
    assert tr["rgb"].requires_grad and tr["thermal"].requires_grad and tr["accumulation"].requires_grad and not tr["depth"].requires_grad
    for k in ("rgb", "thermal", "accumulation", "depth"):
        assert torch.equal(tr[k].detach(), ev[k]), k


def test_backward_is_bit_reproducible():
    p = so.synth_gaussians(5000, seed=4, extent=1.0)
    m = _model(p, 3, "antialiased")
    cam = _camera(so.look_at_camera((2.4, -0.6, 0.8)), 150.0, 80.0, 60.0, 160, 120)
    gen = torch.Generator().manual_seed(1)
    w = {k: torch.randn(120, 160, c, generator=gen) for k, c in (("rgb", 3), ("thermal", 1), ("accumulation", 1))}
    g1, _ = _hip_grads(m, cam, w)
    g2, _ = _hip_grads(m, cam, w)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
        assert bool(torch.isfinite(g1[k]).all()), k
    assert float(g1["means"].abs().max()) > 0


def test_nothing_on_screen_gives_zero_gradients():
    p = sf.scene(100, 5, 3)
    m = _model(p, 3)
    cam = _camera(so.look_at_camera((3.0, 0.0, 0.0), target=(10.0, 0.0, 0.0)), 60.0, 32.0, 24.0, 64, 48)  # looking away from the scene
    ev = m.get_outputs(cam)
    tr = m.get_train_outputs(cam)
    assert m.last_num_intersections == 0
    for k in ("rgb", "thermal", "accumulation"):
        assert torch.equal(tr[k].detach(), ev[k]), k
    (tr["rgb"].sum() + tr["thermal"].sum() + tr["accumulation"].sum()).backward()
    for k in sf.PARAM_NAMES:
        assert _amax(m.gauss_params[k].grad) == 0.0, k
    assert m.last_xys_grad.shape == (100, 2) and float(m.last_xys_grad.abs().max()) == 0.0


def test_gaussians_behind_the_camera_get_zero_gradients():
    eye = torch.tensor([2.3, 0.4, 0.6])
    c2w = so.look_at_camera(tuple(eye.tolist()))
    p = sf.scene(200, 6, 3)
    # the first half moves behind the camera (0.5 .. 2 units back along its optical axis, spread sideways)
    g = torch.Generator().manual_seed(6)
    back = c2w[:3, 2]
    p["means"][:100] = eye + back * (0.5 + 1.5 * torch.rand(100, 1, generator=g)) + 0.8 * (torch.rand(100, 3, generator=g) - 0.5)
    W, H = 64, 48
    fx = sf.fov_focal(W)
    leaves = {k: v.double().requires_grad_(True) for k, v in p.items()}
    ref_out = sf.render(leaves, c2w, fx, fx, 32.0, 24.0, W, H, sh_degree_to_use=3, background_thermal=0.3)
    gen = torch.Generator().manual_seed(2)
    keep = (~ref_out["flag_pixels"]).double()[..., None]
    w = {k: torch.randn(H, W, c, generator=gen, dtype=torch.float64) * keep for k, c in (("rgb", 3), ("thermal", 1), ("accumulation", 1))}
    sum((ref_out[k] * w[k]).sum() for k in w).backward()
    m = _model(p, 3)
    hip, _ = _hip_grads(m, _camera(c2w, fx, 32.0, 24.0, W, H), {k: v.float() for k, v in w.items()})
    assert m.last_num_intersections > 0 and int((m.last_projection["radii"][:100] > 0).sum()) == 0
    excl = ref_out["flag_gaussians"]
    for k in sf.PARAM_NAMES:
        assert bool(torch.isfinite(hip[k]).all()), k
        assert _amax(hip[k][:100]) == 0.0, k
        b = leaves[k].grad.float()[~excl]
        assert _amax(hip[k][~excl] - b) <= 2e-4 * _amax(b), k


def test_intersection_overflow_grows_the_workspace_and_keeps_the_gradients():
    """A frame with more (Gaussian, tile) pairs than the first workspace holds (65536) is redone with a larger one; its gradients equal
    those of the next frame, which starts with the larger workspace."""
    p = so.synth_gaussians(6000, seed=8, extent=1.0, scale_range=(-3.0, -2.0))
    m = _model(p, 3)
    cam = _camera(so.look_at_camera((2.2, 0.3, 0.5)), 300.0, 160.0, 120.0, 320, 240)
    gen = torch.Generator().manual_seed(3)
    w = {k: torch.randn(240, 320, c, generator=gen) for k, c in (("rgb", 3), ("thermal", 1), ("accumulation", 1))}
    g1, out = _hip_grads(m, cam, w)
    assert m.last_num_intersections > 1 << 16, m.last_num_intersections
    g2, _ = _hip_grads(m, cam, w)
    for k in g1:
        assert bool(torch.isfinite(g1[k]).all()), k
        assert torch.equal(g1[k], g2[k]), k
    assert torch.equal(out["rgb"].detach(), m.get_outputs(cam)["rgb"])


def test_fit_recovers_a_perturbed_scene():
    """Fit a perturbed copy of a 2 000-Gaussian RGB+T scene to its own renders from two cameras (128x96): 300 Adam steps on L1 over rgb and
    thermal bring the loss to <= 25 % of its start."""
    target = so.synth_gaussians(2000, seed=12, extent=1.0, scale_range=(-4.0, -2.8))
    W, H = 128, 96
    fx = sf.fov_focal(W)
    cams = [_camera(so.look_at_camera(e), fx, 64.0, 48.0, W, H) for e in ((2.4, 0.5, 0.7), (-0.6, 2.3, 0.5))]
    tm = _model(target, 3)
    gts = [tm.get_outputs(c) for c in cams]
    g = torch.Generator().manual_seed(5)
    pert = {k: v.clone() for k, v in target.items()}
    pert["means"] += 0.02 * torch.randn(pert["means"].shape, generator=g)
    pert["scales"] += 0.3 * torch.randn(pert["scales"].shape, generator=g)
    pert["opacities"] += 1.0 * torch.randn(pert["opacities"].shape, generator=g)
    for k in ("features_dc", "features_dc_thermal"):
        pert[k] += 0.5 * torch.randn(pert[k].shape, generator=g)
    m = _model(pert, 3)
    lrs = {"means": 1e-3, "scales": 1e-2, "quats": 1e-2, "opacities": 5e-2, "features_dc": 2e-2, "features_rest": 2e-3, "features_dc_thermal": 2e-2,
           "features_rest_thermal": 2e-3}
    opt = torch.optim.Adam([{"params": [m.gauss_params[k]], "lr": lr} for k, lr in lrs.items()], eps=1e-15)

    def loss_of():
        tot = 0.0
        for c, gt in zip(cams, gts):
            o = m.get_train_outputs(c)
            tot = tot + (o["rgb"] - gt["rgb"]).abs().mean() + (o["thermal"] - gt["thermal"]).abs().mean()
        return tot

    start = None
    for it in range(300):
        opt.zero_grad(set_to_none=True)
        L = loss_of()
        if start is None:
            start = float(L.detach())
        L.backward()
        opt.step()
    with torch.no_grad():
        end = float(loss_of())
    print(f"fit: L1 {start:.4f} -> {end:.4f} ({end / start:.3f} of the start)")
    assert math.isfinite(end) and end <= 0.25 * start, (start, end)


def test_1080p_one_million_gaussians_backward_is_finite():
    from nerfstudio_thermal_amd import synth

    p = synth.synth_gaussians(1_000_000, seed=11, extent=1.5, scale_range=(-5.5, -3.5))
    m = _model(p, 3)
    cam = _camera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 960.0, 540.0, 1920, 1080)
    out = m.get_train_outputs(cam)
    (out["rgb"].mean() + out["thermal"].mean() + out["accumulation"].mean()).backward()
    for k in sf.PARAM_NAMES:
        assert bool(torch.isfinite(m.gauss_params[k].grad).all()), k
    assert bool(torch.isfinite(m.last_xys_grad).all())
    assert float(m.gauss_params["means"].grad.abs().max()) > 0
