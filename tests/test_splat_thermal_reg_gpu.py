"""The splat model's thermal regularisers on the GPU: tn_thermal_reg (both losses and the gradient of their sum in one call) against float64
autograd of the restatement (thermal_reg_functional.py) on the same fp32 inputs, bit-reproducibility, the multipliers, constant images, and
ThermalSplatfactoModel.get_loss_dict with tv_pixel_loss_mult / cross_channel_loss_mult through the render backward."""
import math

import pytest
import torch

import splat_oracle as so
import thermal_reg_functional as trf
from test_splat_loss_gpu import NAMES, _model, _scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
TV, CROSS = 0.75, 1.5  # exact in fp32: the op's multipliers are the reference's bit for bit
MULTS = [(TV, 0.0), (0.0, CROSS), (TV, CROSS)]


def _splat():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import splat

    return splat


def _hip(pred, gt, tv_mult, cross_mult):
    x = pred.detach().clone().requires_grad_(True) if pred.is_contiguous() else pred.detach().requires_grad_(True)
    tv, cc = _splat().thermal_regularizers(x, gt, tv_mult, cross_mult)
    (tv + cc).backward()
    return tv.detach(), cc.detach(), x.grad


def _ref(pred, gt, tv_mult, cross_mult):
    x = pred.detach().double().requires_grad_(True)
    tv, cc = trf.regularizers(x, gt.double(), tv_mult, cross_mult)
    if tv_mult or cross_mult:
        (tv + cc).backward()
    return float(tv.detach()), float(cc.detach()), x.grad if x.grad is not None else torch.zeros_like(x)


def _check(pred, gt, tv_mult, cross_mult):
    """Losses within 1e-5 relative; the gradient within 1e-4 of its largest entry on every pixel none of whose terms is a near-tie in float64 (a
    sign decided in fp32 may differ there), such terms being at most 0.2 % of all."""
    tv, cc, g = _hip(pred, gt, tv_mult, cross_mult)
    r_tv, r_cc, r_g = _ref(pred, gt, tv_mult, cross_mult)
    mask, share = trf.near_ties(pred.detach().double(), gt.double(), tv_mult, cross_mult)
    err = float(((g.double() - r_g).abs()[..., 0] * (~mask)).max())
    scale = float(r_g.abs().max())
    print(f"{tuple(pred.shape[:2])} mults {tv_mult} / {cross_mult}: tv {float(tv):.8e} (ref {r_tv:.8e}) cc {float(cc):.8e} (ref {r_cc:.8e}) "
          f"gradient error {err:.2e} of {scale:.2e}, near-tie terms {share:.2e}, pixels left out {int(mask.sum())}")
    assert abs(float(tv) - r_tv) <= 1e-5 * abs(r_tv), (float(tv), r_tv)
    assert abs(float(cc) - r_cc) <= 1e-5 * abs(r_cc), (float(cc), r_cc)
    assert share <= 2e-3, share
    assert err <= 1e-4 * scale, (err, scale)
    assert g.shape == pred.shape and bool(torch.isfinite(g).all())


def _pair(h, w, seed, make=trf.random_pair):
    p, g = make(h, w, seed=seed, dtype=torch.float32)
    return p.to(DEV).contiguous(), g.to(DEV).contiguous()


@pytest.mark.parametrize("mults", MULTS)
@pytest.mark.parametrize("hw", [(72, 96), (480, 640), (37, 53), (2, 2), (2, 67), (65, 2), (17, 129)])
def test_losses_and_gradient_against_restatement(hw, mults):
    pred, gt = _pair(*hw, seed=hw[0] + hw[1])
    _check(pred, gt, *mults)


@pytest.mark.parametrize("mults", MULTS)
@pytest.mark.parametrize("hw", [(72, 96), (37, 53)])
def test_losses_and_gradient_against_restatement_smooth(hw, mults):
    pred, gt = _pair(*hw, seed=3, make=trf.smooth_pair)
    _check(pred, gt, *mults)


@pytest.mark.parametrize("mults", MULTS)
def test_strided_views(mults):
    """The thermal channel of an [H,W,4] render and the RGB of an [H,W,4] image, read in place."""
    gen = torch.Generator().manual_seed(5)
    rgbt = torch.rand((37, 53, 4), generator=gen).to(DEV)
    rgba = torch.rand((37, 53, 4), generator=gen).to(DEV)
    pred, gt = rgbt[..., 3:], rgba[..., :3]
    assert pred.stride(1) == 4 and gt.stride(1) == 4
    tv, cc, g = _hip(pred, gt, *mults)
    tv_c, cc_c, g_c = _hip(pred.contiguous(), gt.contiguous(), *mults)
    assert torch.equal(tv, tv_c) and torch.equal(cc, cc_c) and torch.equal(g, g_c)
    _check(pred, gt, *mults)


def test_two_calls_are_bit_identical():
    pred, gt = _pair(480, 640, seed=2)
    a, b = _hip(pred, gt, TV, CROSS), _hip(pred, gt, TV, CROSS)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    with torch.no_grad():  # the loss alone (no gradient buffer) has the same bits
        tv, cc = _splat().thermal_regularizers(pred, gt, TV, CROSS)
    assert torch.equal(tv, a[0]) and torch.equal(cc, a[1])


def test_a_zero_multiplier_switches_its_term_off():
    pred, gt = _pair(72, 96, seed=4)
    tv_b, cc_b, g_b = _hip(pred, gt, TV, CROSS)
    tv_t, cc_t, g_t = _hip(pred, gt, TV, 0.0)
    tv_c, cc_c, g_c = _hip(pred, gt, 0.0, CROSS)
    assert float(cc_t) == 0.0 and float(tv_c) == 0.0
    assert torch.equal(tv_t, tv_b) and torch.equal(cc_c, cc_b)
    assert float(tv_b) > 0 and float(cc_b) > 0
    # the gradient of the sum is the sum of the terms' gradients (each a small integer times its constant: one rounding apart at most)
    assert float((g_b - (g_t + g_c)).abs().max()) <= 1e-6 * float(g_b.abs().max())
    assert not torch.equal(g_t, g_c)
    tv_0, cc_0, g_0 = _hip(pred, gt, 0.0, 0.0)
    assert float(tv_0) == 0.0 and float(cc_0) == 0.0 and float(g_0.abs().max()) == 0.0
    # without the cross term the ground truth is not read: any values give the same bits
    tv_n, _, g_n = _hip(pred, torch.full_like(gt, float("nan")), TV, 0.0)
    assert torch.equal(tv_n, tv_t) and torch.equal(g_n, g_t)


def test_outputs_are_differentiable_one_by_one():
    """Upstream gradients that differ between the two outputs: each term's own gradient, scaled."""
    splat = _splat()
    pred, gt = _pair(37, 53, seed=6)
    _, _, g_t = _hip(pred, gt, TV, 0.0)
    _, _, g_c = _hip(pred, gt, 0.0, CROSS)
    x = pred.clone().requires_grad_(True)
    tv, cc = splat.thermal_regularizers(x, gt, TV, CROSS)
    (2.0 * tv + 0.5 * cc).backward()
    assert torch.allclose(x.grad, 2.0 * g_t + 0.5 * g_c, rtol=1e-6, atol=1e-7 * float(g_t.abs().max()))
    x = pred.clone().requires_grad_(True)
    tv, cc = splat.thermal_regularizers(x, gt, TV, CROSS)
    cc.backward()
    assert torch.equal(x.grad, g_c)


def test_identical_constant_images_give_zero_loss_and_gradient():
    pred = torch.full((40, 70, 1), 0.3, device=DEV)
    gt = torch.full((40, 70, 3), 0.3, device=DEV)
    tv, cc, g = _hip(pred, gt, TV, CROSS)
    assert float(tv) == 0.0 and float(cc) == 0.0 and float(g.abs().max()) == 0.0  # sign(0) = 0


def test_small_images_and_cpu_tensors_raise():
    splat = _splat()
    with pytest.raises(ValueError, match="2 x 2"):
        splat.thermal_regularizers(torch.zeros(1, 40, 1, device=DEV), torch.zeros(1, 40, 3, device=DEV), TV, CROSS)
    with pytest.raises(ValueError, match="no CPU fallback"):
        splat.thermal_regularizers(torch.zeros(4, 4, 1), torch.zeros(4, 4, 3, device=DEV), TV, CROSS)


# ---------------------------------------------------------------------------------------------------- the model
def _target_image(cam, thermal=False):
    with torch.no_grad():
        target = _model(so.synth_gaussians(2000, seed=4, extent=1.0, scale_range=(-4.0, -2.5))).get_outputs(cam)
    return target["thermal"].expand(-1, -1, 3).contiguous() if thermal else target["rgb"].contiguous()


def _frame(m, cam, batch):
    m.zero_grad(set_to_none=True)
    losses = m.get_loss_dict(m.get_train_outputs(cam), batch)
    sum(losses.values()).backward()
    return {k: v.detach().clone() for k, v in losses.items()}, {k: m.gauss_params[k].grad.clone() for k in NAMES}


def test_multipliers_zero_leave_the_loss_dict_and_gradients_as_they_were():
    m0, cam = _scene()
    m1, _ = _scene(tv_pixel_loss_mult=0.0, cross_channel_loss_mult=0.0)
    for thermal in (False, True):
        batch = {"image": _target_image(cam, thermal), "is_thermal": thermal}
        l0, g0 = _frame(m0, cam, batch)
        l1, g1 = _frame(m1, cam, batch)
        assert list(l0) == list(l1) == ["main_loss", "scale_reg"]
        assert all(torch.equal(l0[k], l1[k]) for k in l0) and all(torch.equal(g0[k], g1[k]) for k in NAMES)


def test_rgb_frames_reach_the_thermal_coefficients():
    m, cam = _scene()
    batch = {"image": _target_image(cam), "is_thermal": False}
    _, g = _frame(m, cam, batch)
    assert float(g["features_dc_thermal"].abs().max()) == 0.0 and float(g["features_rest_thermal"].abs().max()) == 0.0
    for kw, keys in (({"tv_pixel_loss_mult": 1e-3}, ["tv_pixel_loss"]), ({"cross_channel_loss_mult": 1e-3}, ["cross_channel_loss"]),
                     ({"tv_pixel_loss_mult": 1e-3, "cross_channel_loss_mult": 2e-3}, ["tv_pixel_loss", "cross_channel_loss"])):
        m, _ = _scene(**kw)
        losses, g = _frame(m, cam, batch)
        assert list(losses) == ["main_loss", "scale_reg"] + keys
        assert all(float(losses[k]) > 0 for k in keys)
        assert float(g["features_dc_thermal"].abs().max()) > 0.0 and float(g["features_rest_thermal"].abs().max()) > 0.0


def test_model_gradients_are_the_render_backward_of_the_image_space_gradients():
    splat = _splat()
    tv_mult, cross_mult = 1e-3, 2e-3
    m, cam = _scene(tv_pixel_loss_mult=tv_mult, cross_channel_loss_mult=cross_mult)
    image = _target_image(cam)
    losses, g = _frame(m, cam, {"image": image, "is_thermal": False})
    # the same render, the image-space gradients of the two ops pushed through its backward by hand
    m.zero_grad(set_to_none=True)
    out = m.get_train_outputs(cam)
    rgb = out["rgb"].detach().requires_grad_(True)
    th = out["thermal"].detach().requires_grad_(True)
    main = splat.image_loss(rgb, image, m.config.ssim_lambda)[0]
    tv, cc = splat.thermal_regularizers(th, image, tv_mult, cross_mult)
    (main + tv + cc).backward()
    assert torch.equal(main.detach(), losses["main_loss"]) and torch.equal(tv.detach(), losses["tv_pixel_loss"])
    assert torch.equal(cc.detach(), losses["cross_channel_loss"])
    torch.autograd.backward([out["rgb"], out["thermal"]], [rgb.grad, th.grad])
    for k in NAMES:
        want = m.gauss_params[k].grad
        assert float(want.abs().max()) > 0.0, k
        assert torch.allclose(g[k], want, rtol=1e-5, atol=0.0), (k, float((g[k] - want).abs().max()), float(want.abs().max()))


def test_thermal_frames_carry_both_keys_at_zero():
    m0, cam = _scene(thermal_loss_mult=1.7)
    m1, _ = _scene(thermal_loss_mult=1.7, tv_pixel_loss_mult=1e-3, cross_channel_loss_mult=2e-3)
    batch = {"image": _target_image(cam, thermal=True), "is_thermal": torch.tensor([1.0])}
    l0, g0 = _frame(m0, cam, batch)
    l1, g1 = _frame(m1, cam, batch)
    assert list(l1) == ["main_loss", "scale_reg", "tv_pixel_loss", "cross_channel_loss"]
    assert float(l1["tv_pixel_loss"]) == 0.0 and float(l1["cross_channel_loss"]) == 0.0
    assert l1["tv_pixel_loss"].is_cuda and l1["tv_pixel_loss"].dim() == 0
    assert torch.equal(l0["main_loss"], l1["main_loss"]) and all(torch.equal(g0[k], g1[k]) for k in NAMES)


def test_the_regularisers_frame_follows_the_resolution_schedule():
    splat = _splat()
    m, cam = _scene(tv_pixel_loss_mult=1e-3, cross_channel_loss_mult=2e-3, num_downscales=1, resolution_schedule=250)
    m.step = 0
    assert m._get_downscale_factor() == 2
    image = _target_image(cam)
    out = m.get_train_outputs(cam)
    assert out["thermal"].shape == (36, 48, 1)
    losses = m.get_loss_dict(out, {"image": image, "is_thermal": False})
    small = splat.resize_image(image, (36, 48))
    tv, cc = splat.thermal_regularizers(out["thermal"].detach(), small, 1e-3, 2e-3)
    assert torch.equal(losses["tv_pixel_loss"].detach(), tv) and torch.equal(losses["cross_channel_loss"].detach(), cc)
    full_tv, _ = splat.thermal_regularizers(m.get_outputs(cam)["thermal"], image, 1e-3, 2e-3)
    assert not torch.equal(full_tv, tv)


def test_masks_are_still_refused():
    m, cam = _scene(tv_pixel_loss_mult=1e-3, cross_channel_loss_mult=2e-3)
    out = m.get_train_outputs(cam)
    batch = {"image": torch.rand(72, 96, 3, device=DEV), "is_thermal": False, "mask": torch.ones(72, 96, 1, device=DEV)}
    with pytest.raises(NotImplementedError):
        m.get_loss_dict(out, batch)


def test_rgba_ground_truth_is_composited_for_the_regularisers():
    """The regularisers see what the main loss sees: an [H,W,4] image composited over the frame's background."""
    splat = _splat()
    m, cam = _scene(background_color="white", tv_pixel_loss_mult=1e-3, cross_channel_loss_mult=2e-3)
    out = m.get_train_outputs(cam)
    rgba = torch.rand(72, 96, 4, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    a = rgba[..., 3:]
    want = a * rgba[..., :3] + (1 - a) * 1.0
    losses = m.get_loss_dict(out, {"image": rgba, "is_thermal": False})
    tv, cc = splat.thermal_regularizers(out["thermal"].detach(), want, 1e-3, 2e-3)
    assert torch.equal(losses["tv_pixel_loss"].detach(), tv) and torch.equal(losses["cross_channel_loss"].detach(), cc)


def test_1080p_smoke():
    pred, gt = _pair(1080, 1920, seed=0)
    tv, cc, g = _hip(pred, gt, TV, CROSS)
    torch.cuda.synchronize()
    assert math.isfinite(float(tv)) and math.isfinite(float(cc)) and float(tv) > 0 and float(cc) > 0
    assert g.shape == (1080, 1920, 1) and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
