"""The splat training loss on the GPU: tn_image_loss (loss and d loss / d prediction in one call) against float64 autograd of the restatement
(ssim_functional.py), bit-reproducibility, ThermalSplatfactoModel.get_loss_dict through the render backward, backgrounds and ground truth,
metrics, edge cases, a fit with refinement and a 1080p / 1 M-Gaussian smoke."""
import math

import pytest
import torch

import splat_functional as spf
import splat_oracle as so
import ssim_functional as sf

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest", "features_dc_thermal", "features_rest_thermal")


def _splat():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import optim, splat

    return splat, optim


def _camera(c2w, fx, cx, cy, W, H):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    return PinholeCamera(c2w, fx, fx, cx, cy, W, H)


def _model(params, seed=0, **cfg_kw):
    splat, _ = _splat()
    cfg_kw.setdefault("sh_degree", 3)
    m = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(**cfg_kw), num_points=4, device=DEV, seed=seed)
    m.load_gaussians(params)
    m.step = 10**6
    return m


def _scene(n=2000, seed=3, W=96, H=72, **cfg_kw):
    m = _model(so.synth_gaussians(n, seed=seed, extent=1.0, scale_range=(-4.0, -2.5)), **cfg_kw)
    return m, _camera(so.look_at_camera((2.4, 0.5, 0.7)), spf.fov_focal(W), W / 2, H / 2, W, H)


def _hip(pred, gt, lam, weight=1.0):
    splat, _ = _splat()
    x = pred.detach().clone().requires_grad_(True) if pred.is_contiguous() else pred.detach().requires_grad_(True)
    main, l1, ss = splat.image_loss(x, gt, lam, weight)
    main.backward()
    return main.detach(), l1, ss, x.grad


def _ref(pred, gt, lam, weight=1.0):
    x = pred.detach().double().requires_grad_(True)
    loss = sf.main_loss(x, gt.double(), lam, weight)
    loss.backward()
    return float(loss.detach()), float(sf.l1(x.detach(), gt.double())), float(sf.ssim(x.detach(), gt.double())), x.grad


def _check(pred, gt, lam, weight=1.0):
    main, l1, ss, g = _hip(pred, gt, lam, weight)
    r_main, r_l1, r_ss, r_g = _ref(pred, gt, lam, weight)
    assert abs(float(main) - r_main) <= 1e-5 * abs(r_main), (float(main), r_main)
    assert abs(float(l1) - r_l1) <= 1e-5 * r_l1 and abs(float(ss) - r_ss) <= 1e-5, (float(l1), r_l1, float(ss), r_ss)
    err = float((g.double() - r_g).abs().max())
    assert err <= 1e-4 * float(r_g.abs().max()), (err, float(r_g.abs().max()))
    return err / float(r_g.abs().max())


def _pair(h, w, c, seed):
    p, g = sf.correlated_pair(h, w, c, seed=seed, dtype=torch.float32)
    return p.to(DEV).contiguous(), g.to(DEV).contiguous()


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("hw", [(11, 11), (37, 53)])
def test_loss_and_gradient_against_restatement_small(hw, lam, c):
    pred, gt = _pair(*hw, c, seed=hw[0] + c)
    _check(pred, gt, lam, weight=1.3)


@pytest.mark.parametrize("hw,c,lam", [((480, 640), 3, 0.2), ((480, 640), 1, 1.0), ((480, 640), 4, 0.0), ((1080, 1920), 3, 0.2),
                                      ((1080, 1920), 1, 0.2), ((1080, 1920), 4, 1.0)])
def test_loss_and_gradient_against_restatement_large(hw, c, lam):
    pred, gt = _pair(*hw, c, seed=7)
    rel = _check(pred, gt, lam)
    print(f"{hw} C={c} lambda={lam}: gradient max-abs error / max |grad| = {rel:.2e}")


def test_strided_prediction_from_an_rgbt_buffer():
    pred, gt = _pair(37, 53, 4, seed=11)
    view = pred[..., :3]
    assert view.stride(1) == 4
    main, l1, ss, g = _hip(view, gt[..., :3], 0.2)
    main_c, l1_c, ss_c, g_c = _hip(view.contiguous(), gt[..., :3], 0.2)
    assert torch.equal(torch.stack([main, l1, ss]), torch.stack([main_c, l1_c, ss_c])) and torch.equal(g, g_c)
    _check(view, gt[..., :3], 0.2)


def test_two_calls_are_bit_identical():
    pred, gt = _pair(480, 640, 3, seed=2)
    a, b = _hip(pred, gt, 0.2), _hip(pred, gt, 0.2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_ssim_of_an_image_with_itself_is_one_and_gradient_zero():
    splat, _ = _splat()
    _, gt = _pair(64, 80, 3, seed=4)
    assert abs(float(splat.ssim(gt, gt)) - 1.0) < 1e-6
    main, l1, ss, g = _hip(gt, gt, 0.2)
    assert float(l1) == 0.0 and abs(float(main)) < 1e-6
    assert float(g.abs().max()) < 1e-9  # sign(0) = 0 and SSIM's maximum


def test_small_images_raise():
    splat, _ = _splat()
    with pytest.raises(ValueError, match="11 x 11"):
        splat.image_loss(torch.zeros(10, 40, 3, device=DEV), torch.zeros(10, 40, 3, device=DEV))
    m, _ = _scene()
    cam = _camera(so.look_at_camera((2.4, 0.5, 0.7)), 8.0, 4.0, 4.0, 8, 8)
    out = m.get_train_outputs(cam)
    with pytest.raises(ValueError):
        m.get_loss_dict(out, {"image": torch.zeros(8, 8, 3, device=DEV), "is_thermal": False})


def _frame_grads(m, cam, batch, loss_fn=None):
    m.zero_grad(set_to_none=True)
    out = m.get_train_outputs(cam)
    loss = m.get_loss_dict(out, batch)["main_loss"] if loss_fn is None else loss_fn(out)
    loss.backward()
    return float(loss.detach()), {k: m.gauss_params[k].grad.clone() for k in NAMES}


@pytest.mark.parametrize("thermal", [False, True])
def test_model_gradients_match_the_restatement(thermal):
    m, cam = _scene(background_thermal=0.3, thermal_loss_mult=1.7)
    with torch.no_grad():
        target = _model(so.synth_gaussians(2000, seed=4, extent=1.0, scale_range=(-4.0, -2.5))).get_outputs(cam)
    img = target["thermal"].expand(-1, -1, 3).contiguous() if thermal else target["rgb"].contiguous()
    batch = {"image": img, "is_thermal": torch.tensor([float(thermal)])}
    loss, g = _frame_grads(m, cam, batch)
    w = 1.7 if thermal else 1.0
    gt = img[..., 0:1] if thermal else img
    r_loss, r_g = _frame_grads(m, cam, batch, lambda o: sf.main_loss((o["thermal"] if thermal else o["rgb"]).double(), gt.double(), 0.2, w))
    assert abs(loss - r_loss) <= 1e-5 * abs(r_loss), (loss, r_loss)
    for k in NAMES:
        scale = float(r_g[k].abs().max())
        err = float((g[k] - r_g[k]).abs().max())
        assert err <= 1e-3 * scale + 1e-12, (k, err, scale)
    if thermal:
        assert float(g["features_dc"].abs().max()) == 0.0 and float(g["features_rest"].abs().max()) == 0.0
        assert float(g["features_dc_thermal"].abs().max()) > 0.0
    # thermal_loss_mult (or, on an RGB frame, nothing) scales the loss and every gradient linearly
    m.config.thermal_loss_mult = 2 * 1.7
    loss2, g2 = _frame_grads(m, cam, batch)
    f = 2.0 if thermal else 1.0
    assert loss2 == pytest.approx(f * loss, rel=1e-6)
    for k in NAMES:
        assert torch.allclose(g2[k], f * g[k], rtol=1e-5, atol=1e-12 * float(g[k].abs().max() + 1)), k


def test_two_training_frames_are_bit_identical():
    m, cam = _scene(background_color="random")
    batch = {"image": torch.rand(72, 96, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1)), "is_thermal": False}
    m.background_generator.manual_seed(5)
    la, ga = _frame_grads(m, cam, batch)
    m.background_generator.manual_seed(5)
    lb, gb = _frame_grads(m, cam, batch)
    assert la == lb and all(torch.equal(ga[k], gb[k]) for k in NAMES)


def test_rgba_ground_truth_is_composited_with_the_frame_background():
    m, cam = _scene(background_color="white", background_thermal=0.25)
    out = m.get_train_outputs(cam)
    g = torch.Generator(DEV).manual_seed(2)
    rgba = torch.rand(72, 96, 4, device=DEV, generator=g)
    a = rgba[..., 3:]
    want_rgb = a * rgba[..., :3] + (1 - a) * 1.0
    want_th = (a * rgba[..., :3] + (1 - a) * 0.25)[..., 0:1]
    rgb_loss = m.get_loss_dict(out, {"image": rgba, "is_thermal": False})["main_loss"]
    th_loss = m.get_loss_dict(out, {"image": rgba, "is_thermal": True})["main_loss"]
    splat, _ = _splat()
    assert torch.equal(rgb_loss, splat.image_loss(out["rgb"], want_rgb, 0.2)[0])
    assert torch.equal(th_loss, splat.image_loss(out["thermal"], want_th, 0.2)[0])
    u8 = (rgba[..., :3] * 255).to(torch.uint8)
    assert torch.equal(m.get_gt_img(u8.cpu()), (u8.cpu().float() / 255.0).to(DEV))


def test_random_background_draws():
    m, cam = _scene(background_color="random", seed=9)
    m2, _ = _scene(background_color="random", seed=9)
    draws = [m.get_train_outputs(cam) for _ in range(3)]
    draws2 = [m2.get_train_outputs(cam) for _ in range(3)]
    bgs = [torch.cat([d["background"], d["background_thermal"]]).cpu() for d in draws]
    bgs2 = [torch.cat([d["background"], d["background_thermal"]]).cpu() for d in draws2]
    assert all(torch.equal(a, b) for a, b in zip(bgs, bgs2))  # the same seed repeats them
    assert not torch.equal(bgs[0], bgs[1]) and not torch.equal(bgs[1], bgs[2])  # every frame draws anew
    assert all(float(b.min()) >= 0.0 and float(b.max()) < 1.0 for b in bgs)
    # the draw is the render's background: pixels nothing covers show it (RGB and thermal)
    d = draws[2]
    empty = d["accumulation"][..., 0] == 0
    assert bool(empty.any())
    assert torch.equal(d["rgb"][empty], bgs[2][:3].to(DEV).expand(int(empty.sum()), 3))
    assert torch.equal(d["thermal"][empty][:, 0], bgs[2][3].to(DEV).expand(int(empty.sum())))
    ev = m.get_outputs(cam)
    splat, _ = _splat()
    assert torch.equal(ev["background"].cpu(), torch.tensor(splat.VIEWER_BACKGROUND))
    assert float(ev["background_thermal"]) == m.config.background_thermal


@pytest.mark.parametrize("color", ["black", "white"])
def test_fixed_backgrounds_render_as_before(color):
    m, cam = _scene(background_color=color, background_thermal=0.4)
    tr, ev = m.get_train_outputs(cam), m.get_outputs(cam)
    for k in ("rgb", "thermal", "accumulation", "depth", "background", "background_thermal"):
        assert torch.equal(tr[k], ev[k]), k
    v = 1.0 if color == "white" else 0.0
    empty = ev["accumulation"][..., 0] == 0
    assert bool(empty.any())
    assert bool((ev["rgb"][empty] == v).all()) and bool((ev["thermal"][empty] == 0.4).all())
    assert torch.equal(ev["background"].cpu(), torch.full((3,), v))


def test_metrics():
    m, cam = _scene()
    out = m.get_outputs(cam)
    img = out["rgb"].clamp(0, 1).contiguous()
    md = m.get_metrics_dict(out, {"image": img * 0.9, "is_thermal": False})
    assert set(md) == {"psnr", "gaussian_count"} and math.isfinite(float(md["psnr"])) and md["gaussian_count"] == m.num_points
    met, imgs = m.get_image_metrics_and_images(out, {"image": img, "is_thermal": False})
    assert set(met) == {"psnr_rgb", "ssim_rgb"} and abs(met["ssim_rgb"] - 1.0) < 1e-6 and met["psnr_rgb"] > 60
    th = out["thermal"].expand(-1, -1, 3).contiguous()
    met, imgs = m.get_image_metrics_and_images(out, {"image": th * 0.8, "is_thermal": torch.tensor([1.0])})
    assert set(met) == {"psnr_thermal", "ssim_thermal"} and all(math.isfinite(v) for v in met.values()) and met["ssim_thermal"] < 1.0
    assert imgs["img"].shape == (72, 3 * 96, 3)


def test_nothing_on_screen_and_masks():
    m = _model({k: torch.zeros((0,) + s) for k, s in zip(NAMES, ((3,), (3,), (4,), (1,), (3,), (15, 3), (1,), (15, 1)))})
    cam = _camera(so.look_at_camera((2.4, 0.5, 0.7)), 80.0, 48.0, 36.0, 96, 72)
    out = m.get_train_outputs(cam)
    batch = {"image": torch.rand(72, 96, 3, device=DEV), "is_thermal": False}
    loss = m.get_loss_dict(out, batch)
    assert math.isfinite(float(loss["main_loss"].detach())) and float(loss["scale_reg"]) == 0.0
    loss["main_loss"].backward()
    for k in NAMES:
        g = m.gauss_params[k].grad
        assert g is None or g.numel() == 0 or float(g.abs().max()) == 0.0
    with pytest.raises(NotImplementedError):
        m.get_loss_dict(out, {**batch, "mask": torch.ones(72, 96, 1, device=DEV)})


def test_scale_regularization_every_tenth_step():
    m, cam = _scene(use_scale_regularization=True)
    out = m.get_train_outputs(cam)
    batch = {"image": torch.rand(72, 96, 3, device=DEV), "is_thermal": False}
    m.step = 20
    s = torch.exp(m.gauss_params["scales"].detach())
    want = 0.1 * (torch.clamp(s.amax(-1) / s.amin(-1), min=10.0) - 10.0).mean()
    assert torch.allclose(m.get_loss_dict(out, batch)["scale_reg"], want, rtol=1e-6)
    m.step = 21
    assert float(m.get_loss_dict(out, batch)["scale_reg"]) == 0.0


def _fit(ssim_lambda: float, steps: int = 900):
    """The end-to-end scene of test_splat_refine_gpu._fit (300 Gaussians fitted to 3000, three views) trained through get_loss_dict with the
    callbacks and refinement; every view is an RGB frame and a thermal frame.  Returns (main_loss at the start, at the end, mean SSIM)."""
    splat, optim = _splat()
    from nerfstudio_thermal_amd.model import TrainingCallbackLocation

    target = so.synth_gaussians(3000, seed=21, extent=1.0, scale_range=(-4.5, -3.0))
    W, H = 128, 96
    fx = spf.fov_focal(W)
    cams = [_camera(so.look_at_camera(e), fx, 64.0, 48.0, W, H) for e in ((2.4, 0.5, 0.7), (-0.6, 2.3, 0.5), (0.4, -2.2, 1.0))]
    tm = _model(target)
    gts = [tm.get_outputs(c) for c in cams]
    frames = [(c, {"image": gt["rgb"].contiguous(), "is_thermal": False}) for c, gt in zip(cams, gts)]
    frames += [(c, {"image": gt["thermal"].expand(-1, -1, 3).contiguous(), "is_thermal": True}) for c, gt in zip(cams, gts)]
    n0 = 300
    g = torch.Generator().manual_seed(22)
    init = {"means": (torch.rand((n0, 3), generator=g) - 0.5) * 2.0, "scales": torch.full((n0, 3), math.log(0.08)),
            "quats": torch.nn.functional.normalize(torch.randn((n0, 4), generator=g), dim=-1), "opacities": torch.zeros((n0, 1)),
            "features_dc": torch.rand((n0, 3), generator=g) - 0.5, "features_rest": torch.zeros((n0, 15, 3)),
            "features_dc_thermal": torch.rand((n0, 1), generator=g) - 0.5, "features_rest_thermal": torch.zeros((n0, 15, 1))}
    m = _model(init, seed=23, sh_degree_interval=300, refine_every=50, warmup_length=100, ssim_lambda=ssim_lambda)
    m.step = 0
    m.num_train_data = len(frames)
    opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=optim.HipAdam)
    cbs = m.get_training_callbacks(opts)

    def eval_loss():
        with torch.no_grad():
            return sum(float(m.get_loss_dict(m.get_outputs(c), b)["main_loss"]) for c, b in frames) / len(frames)

    start = eval_loss()
    for step in range(steps):
        for cb in cbs:
            cb.run_callback_at_location(step, TrainingCallbackLocation.BEFORE_TRAIN_ITERATION)
        opts.zero_grad_all()
        c, b = frames[step % len(frames)]
        loss = m.get_loss_dict(m.get_train_outputs(c), b)
        (loss["main_loss"] + loss["scale_reg"]).backward()
        opts.optimizer_step_all()
        opts.scheduler_step_all()
        for cb in cbs:
            cb.run_callback_at_location(step, TrainingCallbackLocation.AFTER_TRAIN_ITERATION)
    m.config.ssim_lambda = 0.2  # the same objective for both runs' reports
    end = eval_loss()
    with torch.no_grad():
        ss = [m.get_image_metrics_and_images(m.get_outputs(c), b)[0] for c, b in frames]
    mean_ssim = sum(v for d in ss for k, v in d.items() if k.startswith("ssim")) / len(ss)
    return start, end, mean_ssim, m.num_points


def test_fit_with_the_ssim_loss():
    """Measured on an MI355X: main_loss 0.3037 -> 0.0021, SSIM 0.9991 against 0.9971 when trained on L1 alone; the SSIM margin asked for is half
    the measured gap."""
    start, end, ssim_full, n = _fit(0.2)
    _, end_l1, ssim_l1, _ = _fit(0.0)
    print(f"fit: main_loss {start:.4f} -> {end:.4f} ({n} Gaussians), SSIM {ssim_full:.4f}; with ssim_lambda = 0: SSIM {ssim_l1:.4f}")
    assert math.isfinite(end) and end <= 0.3 * start, (start, end)
    assert ssim_full > ssim_l1 + 0.001, (ssim_full, ssim_l1)


def test_1080p_one_million_gaussians_loss_smoke():
    from nerfstudio_thermal_amd import synth

    p = synth.synth_gaussians(1_000_000, seed=11, extent=1.5, scale_range=(-5.5, -3.5))
    m = _model(p, background_color="random")
    cam = _camera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 960.0, 540.0, 1920, 1080)
    gt = torch.rand(1080, 1920, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    for th in (False, True):
        m.zero_grad(set_to_none=True)
        loss = m.get_loss_dict(m.get_train_outputs(cam), {"image": gt, "is_thermal": th})
        loss["main_loss"].backward()
        torch.cuda.synchronize()
        assert math.isfinite(float(loss["main_loss"].detach()))
        assert all(bool(torch.isfinite(m.gauss_params[k].grad).all()) for k in NAMES)
