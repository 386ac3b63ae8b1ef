"""The bilateral grid on the GPU: tn_bilagrid_slice and its backward against float64 autograd of the restatement (bilagrid_functional.py) on the
same fp32 inputs, within 8 x the fp32 restatement's own error; exactness on identity and constant grids; bit-reproducibility; tn_bilagrid_tv; and
ThermalSplatfactoModel with use_bilateral_grid through the render backward."""
import dataclasses
import functools
import math

import pytest
import torch

import bilagrid_functional as bf
from test_splat_loss_gpu import NAMES, _camera, _model, _scene, so, spf

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 8.0  # what the splat parity tests give a different summation order
EPS = 2.0 ** -23

# name -> (C, H, W, grid_shape (GW, GH, L), F, row)
CASES = {
    "rgb_37x53": (3, 37, 53, (16, 16, 8), 1, 0),
    "thermal_29x41": (1, 29, 41, (16, 16, 8), 1, 0),
    "rgb_5x7_mostly_empty_vertices": (3, 5, 7, (16, 16, 8), 1, 0),
    "rgb_40x64_grid_5x3x4": (3, 40, 64, (5, 3, 4), 1, 0),
    "rgb_21x19_smallest_grid": (3, 21, 19, (2, 2, 2), 1, 0),
    "thermal_21x19_smallest_grid": (1, 21, 19, (2, 2, 2), 1, 0),
    "rgb_1x40": (3, 1, 40, (16, 16, 8), 1, 0),
    "rgb_40x1": (3, 40, 1, (16, 16, 8), 1, 0),
    "rgb_13x17_row_1_of_3": (3, 13, 17, (4, 3, 2), 3, 1),
    "thermal_130x9_two_row_slices": (1, 130, 9, (3, 4, 2), 2, 1),  # H >= 128: the vertex rectangles are cut into two slices of rows
    "thermal_16x16_two_level_chunks": (1, 16, 16, (2, 2, 9), 1, 0),  # L > 8: two chunks of levels
}


def _splat():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import optim, splat

    return splat, optim


def _inputs(name):
    C, H, W, shape, F, row = CASES[name]
    seed = sum(map(ord, name))
    return bf.random_grids(F, C, shape, seed), row, bf.random_image(H, W, C, seed + 1), bf.random_upstream(H, W, C, seed + 2)


def _restatement(grids, row, image, v, dtype):
    g, x = grids.detach().to(dtype).clone().requires_grad_(True), image.detach().to(dtype).clone().requires_grad_(True)
    out = bf.slice(g[row], x)
    out.backward(v.to(dtype))
    return out.detach().double(), x.grad.double(), g.grad.double()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(float64 results, floors): computed once per case on the CPU and shared; the floor of a quantity is the fp32 restatement's largest error
    against float64 on this case, never less than 2^-23 of the largest reference entry (the image gradient's over the pixels compared)."""
    grids, row, image, v = _inputs(name)
    ref = _restatement(grids, row, image, v, torch.float64)
    low = _restatement(grids, row, image, v, torch.float32)
    keep = ~bf.near_planes(image, grids.shape[2])
    floors = []
    for i, (a, b) in enumerate(zip(low, ref)):
        err = (a - b).abs()
        if i == 1:
            err = err * keep[..., None]
        floors.append(max(float(err.max()), EPS * float(b.abs().max())))
    return ref, floors, keep


def _hip(grids, row, image, v):
    splat, _ = _splat()
    g = grids.detach().to(DEV).requires_grad_(True)
    x = image.detach().to(DEV).requires_grad_(True)
    out = splat.bilateral_slice(g, row, x)
    out.backward(v.to(DEV))
    return out.detach(), x.grad, g.grad


@pytest.mark.parametrize("name", list(CASES))
def test_slice_and_backward_against_float64(name):
    grids, row, image, v = _inputs(name)
    (r_out, r_img, r_grid), floors, keep = _reference(name)
    out, g_img, g_grid = _hip(grids, row, image, v)
    assert out.shape == image.shape and g_img.shape == image.shape and g_grid.shape == grids.shape
    share = 1.0 - float(keep.float().mean())
    errs = [float((out.cpu().double() - r_out).abs().max()), float(((g_img.cpu().double() - r_img).abs() * keep[..., None]).max()),
            float((g_grid.cpu().double() - r_grid).abs().max())]
    print(f"{name}: " + ", ".join(f"{what} error {e:.2e} floor {f:.2e} largest {float(r.abs().max()):.2e}"
                                   for what, e, f, r in zip(("output", "image gradient", "grid gradient"), errs, floors, (r_out, r_img, r_grid)))
          + f", pixels left out {share:.2%}")
    assert share <= 0.01
    for what, e, f in zip(("output", "image gradient", "grid gradient"), errs, floors):
        assert e <= MARGIN * f, (what, e, f)
    assert bool(torch.isfinite(g_img).all()) and bool(torch.isfinite(g_grid).all())
    others = [r for r in range(grids.shape[0]) if r != row]
    assert all(float(g_grid[r].abs().max()) == 0.0 for r in others)  # the other frames' rows: exactly zero
    # vertices no pixel reaches: exact zeros, as in the reference
    assert bool((g_grid.cpu()[r_grid == 0] == 0).all())
    if name == "rgb_5x7_mostly_empty_vertices":
        assert float((r_grid[row] == 0).double().mean()) > 0.5


@pytest.mark.parametrize("C", [3, 1])
def test_strided_views_give_the_bits_of_the_contiguous_call(C):
    H, W, shape = 37, 53, (16, 16, 8)
    rgbt = bf.random_image(H, W, 4, seed=7).to(DEV)
    view = rgbt[..., :3] if C == 3 else rgbt[..., 3:]
    assert view.stride(1) == 4
    grids, v = bf.random_grids(2, C, shape, seed=8), bf.random_upstream(H, W, C, seed=9)
    a = _hip(grids, 1, view.detach(), v)
    b = _hip(grids, 1, view.detach().contiguous(), v)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    r_out = bf.slice(grids[1].double(), view.cpu().double())
    assert float((a[0].cpu().double() - r_out).abs().max()) <= 1e-5


def test_saturated_pixels():
    """Pixels at exactly 0 and exactly 1 (what the render's clamp produces): the forward everywhere and the whole grid gradient against float64 --
    both are continuous there -- and finite gradients; the image gradient's guidance path is one-sided on the clamp and is not compared."""
    C, H, W, shape = 1, 24, 30, (4, 4, 5)
    grids, v = bf.random_grids(1, C, shape, seed=21), bf.random_upstream(H, W, C, seed=22)
    image = bf.random_image(H, W, C, seed=23)
    image[::3, ::2] = 1.0
    image[1::3, 1::2] = 0.0
    assert int((image == 1).sum()) > 50 and int((image == 0).sum()) > 50
    ref = _restatement(grids, 0, image, v, torch.float64)
    low = _restatement(grids, 0, image, v, torch.float32)
    out, g_img, g_grid = _hip(grids, 0, image, v)
    for what, got, i in (("output", out, 0), ("grid gradient", g_grid, 2)):
        floor = max(float((low[i] - ref[i]).abs().max()), EPS * float(ref[i].abs().max()))
        err = float((got.cpu().double() - ref[i]).abs().max())
        print(f"saturated {what}: error {err:.2e} floor {floor:.2e}")
        assert err <= MARGIN * floor, (what, err, floor)
    assert bool(torch.isfinite(g_img).all()) and bool(torch.isfinite(g_grid).all())


@pytest.mark.parametrize("C", [3, 1])
def test_identity_grid_returns_the_input_bit_for_bit(C):
    splat, _ = _splat()
    image = bf.random_image(37, 53, C, seed=3).to(DEV)
    image[0, 0] = 0.0
    image[0, 1] = 1.0
    grids = splat.identity_bilateral_grids(3, C, (16, 16, 8), DEV)
    assert torch.equal(splat.bilateral_slice(grids, 2, image), image)
    rgbt = bf.random_image(37, 53, 4, seed=4).to(DEV)
    view = rgbt[..., :3] if C == 3 else rgbt[..., 3:]
    assert torch.equal(splat.bilateral_slice(grids, 0, view), view)
    # and its backward hands the upstream gradient to the image bit for bit
    v = bf.random_upstream(37, 53, C, seed=5)
    _, g_img, _ = _hip(grids.cpu(), 1, image.clone(), v)
    assert torch.equal(g_img, v.to(DEV))


@pytest.mark.parametrize("C", [3, 1])
def test_constant_grid_is_the_affine_map_to_one_rounding_per_term(C):
    splat, _ = _splat()
    gen = torch.Generator().manual_seed(11)
    affine = torch.randn((C, C + 1), generator=gen)
    image = bf.random_image(40, 64, C, seed=12)
    out = splat.bilateral_slice(bf.constant_grids(2, affine, (5, 3, 4)).to(DEV), 1, image.to(DEV)).cpu().double()
    a, x = affine.double(), image.double()
    want = x @ a[:, :C].T + a[:, C]
    size = x.abs() @ a[:, :C].abs().T + a[:, C].abs()  # the sum of the terms' magnitudes: each product and each sum rounds once
    assert bool(((out - want).abs() <= (C + 1) * EPS * size).all()), float(((out - want).abs() / size).max())


def test_two_calls_give_identical_bits():
    splat, _ = _splat()
    grids, row, image, v = bf.random_grids(2, 3, (16, 16, 8), 31), 1, bf.random_image(150, 200, 3, 32), bf.random_upstream(150, 200, 3, 33)
    a, b = _hip(grids, row, image, v), _hip(grids, row, image, v)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    g = grids.detach().to(DEV).requires_grad_(True)
    tv = [splat.bilateral_grid_tv(g, 10.0) for _ in range(2)]
    grads = [torch.autograd.grad(t, g)[0] for t in tv]
    assert torch.equal(tv[0], tv[1]) and torch.equal(grads[0], grads[1])
    with torch.no_grad():  # the value alone has the same bits
        assert torch.equal(splat.bilateral_grid_tv(g, 10.0), tv[0].detach())


@pytest.mark.parametrize("shape", [(16, 16, 8), (2, 2, 2)])
@pytest.mark.parametrize("K", [12, 2])
@pytest.mark.parametrize("F", [1, 5])
def test_total_variation_against_float64(F, K, shape):
    splat, _ = _splat()
    C, mult = (3 if K == 12 else 1), 10.0
    grids = bf.random_grids(F, C, shape, seed=F + K + shape[0])

    def ref(dtype):
        g = grids.detach().to(dtype).clone().requires_grad_(True)
        t = mult * bf.tv(g)
        t.backward()
        return float(t.detach()), g.grad.double()

    (r_tv, r_grad), (_, low_grad) = ref(torch.float64), ref(torch.float32)
    g = grids.detach().to(DEV).requires_grad_(True)
    tv = splat.bilateral_grid_tv(g, mult)
    tv.backward()
    assert tv.is_cuda and tv.dim() == 0 and g.grad.shape == grids.shape
    floor = max(float((low_grad - r_grad).abs().max()), EPS * float(r_grad.abs().max()))
    err = float((g.grad.cpu().double() - r_grad).abs().max())
    print(f"tv F {F} K {K} {shape}: value {float(tv.detach()):.8e} (ref {r_tv:.8e}), gradient error {err:.2e} floor {floor:.2e} largest {float(r_grad.abs().max()):.2e}")
    assert r_tv > 0 and abs(float(tv.detach()) - r_tv) <= 1e-5 * r_tv
    assert err <= MARGIN * floor, (err, floor)
    const = splat.identity_bilateral_grids(F, C, shape, DEV).requires_grad_(True)
    zero = splat.bilateral_grid_tv(const, mult)
    zero.backward()
    assert float(zero.detach()) == 0.0 and float(const.grad.abs().max()) == 0.0


def test_bad_shapes_and_cpu_tensors_raise():
    splat, _ = _splat()
    grids, image = bf.identity_grids(2, 3, (4, 4, 2)).to(DEV), torch.zeros(5, 6, 3, device=DEV)
    with pytest.raises(ValueError, match="no CPU fallback"):
        splat.bilateral_slice(grids.cpu(), 0, image)
    with pytest.raises(ValueError, match="no CPU fallback"):
        splat.bilateral_slice(grids, 0, image.cpu())
    with pytest.raises(ValueError, match="coefficients"):
        splat.bilateral_slice(grids, 0, torch.zeros(5, 6, 1, device=DEV))
    with pytest.raises(ValueError, match="row 2"):
        splat.bilateral_slice(grids, 2, image)
    with pytest.raises(ValueError, match="2..256"):
        splat.bilateral_slice(torch.zeros(1, 12, 1, 4, 4, device=DEV), 0, image)
    with pytest.raises(ValueError, match="2..256"):
        splat.bilateral_grid_tv(torch.zeros(1, 12, 2, 4, 257, device=DEV), 1.0)


# ---------------------------------------------------------------------------------------------------- the model
W, H = 96, 72


def _bscene(num_train_data=4, train_is_thermal=None, **cfg_kw):
    """The small scene of test_splat_loss_gpu with training frames, so that the model has grids."""
    splat, _ = _splat()
    cfg_kw.setdefault("sh_degree", 3)
    m = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(**cfg_kw), num_points=4, device=DEV, seed=0, num_train_data=num_train_data,
                                     train_is_thermal=train_is_thermal)
    m.load_gaussians(so.synth_gaussians(2000, seed=3, extent=1.0, scale_range=(-4.0, -2.5)))
    m.step = 10**6
    return m, _camera(so.look_at_camera((2.4, 0.5, 0.7)), spf.fov_focal(W), W / 2, H / 2, W, H)


def _shake(m, seed=41):
    """Grids away from the identity, as training leaves them."""
    with torch.no_grad():
        for i, name in enumerate(("bil_grids", "bil_grids_thermal")):
            if hasattr(m, name):
                p = getattr(m, name)
                p.add_(0.2 * (2 * torch.rand(p.shape, generator=torch.Generator().manual_seed(seed + i)) - 1).to(DEV))


def _target(cam, thermal=False):
    with torch.no_grad():  # another cloud's render
        out = _model(so.synth_gaussians(2000, seed=4, extent=1.0, scale_range=(-4.0, -2.5))).get_outputs(cam)
    return out["thermal"].expand(-1, -1, 3).contiguous() if thermal else out["rgb"].contiguous()


def _frame(m, cam, batch):
    m.zero_grad(set_to_none=True)
    losses = m.get_loss_dict(m.get_train_outputs(cam), batch)
    sum(losses.values()).backward()
    return {k: v.detach().clone() for k, v in losses.items()}, {k: m.gauss_params[k].grad.clone() for k in NAMES}


def _idx(cam, idx, thermal=False):
    return dataclasses.replace(cam, cam_idx=idx, is_thermal=thermal)


def test_switch_off_is_the_model_of_before():
    m0, cam = _scene()
    m1, _ = _bscene(use_bilateral_grid=False)
    assert list(m1.state_dict()) == list(m0.state_dict()) and set(m0.state_dict()) == {f"gauss_params.{k}" for k in NAMES}
    assert list(m1.get_param_groups()) == list(m0.get_param_groups()) and m1.param_names == m0.param_names == NAMES
    assert not hasattr(m1, "bil_grids") and not hasattr(m1, "bil_grids_thermal")
    for thermal in (False, True):
        batch = {"image": _target(cam, thermal), "is_thermal": thermal}
        l0, g0 = _frame(m0, cam, batch)
        l1, g1 = _frame(m1, _idx(cam, 1, thermal), batch)
        assert list(l0) == list(l1) == ["main_loss", "scale_reg"]
        assert all(torch.equal(l0[k], l1[k]) for k in l0) and all(torch.equal(g0[k], g1[k]) for k in NAMES)


def test_fresh_grids_leave_loss_and_gradients_bit_for_bit():
    m0, cam = _scene()
    m1, _ = _bscene(use_bilateral_grid=True)
    assert m1.param_names == NAMES
    assert set(m1.state_dict()) == set(m0.state_dict()) | {"bil_grids", "bil_grids_thermal"}
    assert list(m1.get_param_groups()) == list(m0.get_param_groups()) + ["bilateral_grid", "bilateral_grid_thermal"]
    assert m1.bil_grids.shape == (4, 12, 8, 16, 16) and m1.bil_grids_thermal.shape == (4, 2, 8, 16, 16)
    assert torch.equal(m1.bil_grids.detach().cpu(), bf.identity_grids(4, 3, (16, 16, 8)))
    assert torch.equal(m1.bil_grids_thermal.detach().cpu(), bf.identity_grids(4, 1, (16, 16, 8)))
    for thermal in (False, True):
        batch = {"image": _target(cam, thermal), "is_thermal": thermal}
        l0, g0 = _frame(m0, cam, batch)
        l1, g1 = _frame(m1, _idx(cam, 2, thermal), batch)
        assert list(l1) == ["main_loss", "scale_reg", "tv_loss"]
        assert torch.equal(l0["main_loss"], l1["main_loss"]) and all(torch.equal(g0[k], g1[k]) for k in NAMES)
        assert float(l1["tv_loss"]) == 0.0 and l1["tv_loss"].is_cuda and l1["tv_loss"].dim() == 0
        own = m1.bil_grids_thermal if thermal else m1.bil_grids
        assert float(own.grad[2].abs().max()) > 0.0  # the frame's own grid learns from the first step


def test_frames_reach_their_own_row_alone():
    flags = [False, True, False, True, False]
    m, cam = _bscene(num_train_data=5, train_is_thermal=flags, use_bilateral_grid=True, grid_shape=(5, 3, 4), bilateral_grid_tv_mult=0.0)
    assert m.bil_grids.shape == (3, 12, 4, 3, 5) and m.bil_grids_thermal.shape == (2, 2, 4, 3, 5)
    _shake(m)
    for idx, thermal, row in ((4, False, 2), (0, False, 0), (3, True, 1), (1, True, 0)):
        _frame(m, _idx(cam, idx, thermal), {"image": _target(cam, thermal), "is_thermal": thermal})
        own, other = (m.bil_grids_thermal, m.bil_grids) if thermal else (m.bil_grids, m.bil_grids_thermal)
        assert float(own.grad[row].abs().max()) > 0.0
        assert all(float(own.grad[r].abs().max()) == 0.0 for r in range(own.shape[0]) if r != row)
        assert other.grad is None or float(other.grad.abs().max()) == 0.0
    with pytest.raises(ValueError, match="cam_idx"):
        m.get_train_outputs(_idx(cam, 5))
    # without the flags both tensors have a row per training frame and the row is cam_idx
    m, cam = _bscene(num_train_data=3, use_bilateral_grid=True, grid_shape=(2, 2, 2), bilateral_grid_tv_mult=0.0)
    assert m.bil_grids.shape == (3, 12, 2, 2, 2) and m.bil_grids_thermal.shape == (3, 2, 2, 2, 2)
    _frame(m, _idx(cam, 2, True), {"image": _target(cam, True), "is_thermal": True})
    assert float(m.bil_grids_thermal.grad[2].abs().max()) > 0.0 and float(m.bil_grids_thermal.grad[:2].abs().max()) == 0.0


@pytest.mark.parametrize("thermal", [False, True])
def test_model_gradients_are_the_render_backward_of_the_slices_image_gradient(thermal):
    splat, _ = _splat()
    m, cam = _bscene(use_bilateral_grid=True, thermal_loss_mult=1.0)
    _shake(m)
    image = _target(cam, thermal)
    batch = {"image": image, "is_thermal": thermal}
    losses, g = _frame(m, _idx(cam, 1, thermal), batch)
    grid_grad = (m.bil_grids_thermal if thermal else m.bil_grids).grad.clone()
    assert float(losses["tv_loss"]) > 0.0
    # the same render without the correction, and the slice's image gradient pushed through its backward by hand
    m.zero_grad(set_to_none=True)
    out = m.get_train_outputs(cam)  # no cam_idx: uncorrected
    key = "thermal" if thermal else "rgb"
    raw = out[key].detach().requires_grad_(True)
    grids = (m.bil_grids_thermal if thermal else m.bil_grids).detach().clone().requires_grad_(True)
    corrected = splat.bilateral_slice(grids, 1, raw)
    main = splat.image_loss(corrected, image[..., :1] if thermal else image, m.config.ssim_lambda)[0]
    (main + splat.bilateral_grid_tv(grids, m.config.bilateral_grid_tv_mult)).backward()
    assert torch.equal(main.detach(), losses["main_loss"])
    torch.autograd.backward([out[key]], [raw.grad])
    for k in NAMES:
        want = m.gauss_params[k].grad
        if k.endswith("_thermal") != thermal and k.startswith("features"):
            assert float(want.abs().max()) == 0.0 and float(g[k].abs().max()) == 0.0  # the other spectrum's colours
            continue
        assert float(want.abs().max()) > 0.0, k
        assert torch.allclose(g[k], want, rtol=1e-5, atol=0.0), (k, float((g[k] - want).abs().max()), float(want.abs().max()))
    assert torch.equal(grid_grad, grids.grad)


def test_eval_renders_and_cameras_without_an_index_are_not_corrected():
    m0, cam = _scene()
    m1, _ = _bscene(use_bilateral_grid=True)
    _shake(m1)
    want = m0.get_outputs(cam)
    for c in (cam, _idx(cam, 1), _idx(cam, 1, True)):
        got = m1.get_outputs(c)
        assert all(torch.equal(got[k], want[k]) for k in ("rgb", "thermal", "depth", "accumulation"))
    train0, train1 = m0.get_train_outputs(cam), m1.get_train_outputs(cam)  # a camera without cam_idx
    assert torch.equal(train0["rgb"], train1["rgb"]) and torch.equal(train0["thermal"], train1["thermal"])
    # with one, its own spectrum alone is corrected, and not clamped again
    rgb_frame, th_frame = m1.get_train_outputs(_idx(cam, 1)), m1.get_train_outputs(_idx(cam, 1, True))
    assert not torch.equal(rgb_frame["rgb"], train0["rgb"]) and torch.equal(rgb_frame["thermal"], train0["thermal"])
    assert not torch.equal(th_frame["thermal"], train0["thermal"]) and torch.equal(th_frame["rgb"], train0["rgb"])
    splat, _ = _splat()
    assert torch.equal(rgb_frame["rgb"], splat.bilateral_slice(m1.bil_grids.detach(), 1, train0["rgb"].detach()))


def test_the_corrected_frame_follows_the_resolution_schedule():
    splat, _ = _splat()
    m, cam = _bscene(use_bilateral_grid=True, num_downscales=1, resolution_schedule=250)
    _shake(m)
    m.step = 0
    assert m._get_downscale_factor() == 2
    out = m.get_train_outputs(_idx(cam, 3))
    raw = m.get_train_outputs(cam)
    assert out["rgb"].shape == (36, 48, 3) and raw["rgb"].shape == (36, 48, 3)
    assert torch.equal(out["rgb"], splat.bilateral_slice(m.bil_grids.detach(), 3, raw["rgb"].detach()))
    losses = m.get_loss_dict(out, {"image": _target(cam), "is_thermal": False})
    assert math.isfinite(float(losses["main_loss"].detach())) and float(losses["tv_loss"].detach()) > 0.0


def test_masks_are_still_refused():
    m, cam = _bscene(use_bilateral_grid=True)
    out = m.get_train_outputs(_idx(cam, 0))
    batch = {"image": torch.rand(H, W, 3, device=DEV), "is_thermal": False, "mask": torch.ones(H, W, 1, device=DEV)}
    with pytest.raises(NotImplementedError):
        m.get_loss_dict(out, batch)


def test_the_grid_learns_a_frames_gain_and_offset():
    """The Gaussians held fixed, the ground truth 0.8 render + 0.1: 50 HipAdam steps on the grid group alone lower the main loss."""
    _, optim = _splat()
    m, cam = _bscene(use_bilateral_grid=True)
    frame = _idx(cam, 1)
    with torch.no_grad():
        batch = {"image": (0.8 * m.get_outputs(cam)["rgb"] + 0.1).contiguous(), "is_thermal": False}
    opts = optim.Optimizers({"bilateral_grid": [m.bil_grids]}, optim.SPLAT_BILAGRID_OPTIMIZERS, optimizer_cls=optim.HipAdam)
    before = m.bil_grids.detach().clone()
    mains = []
    for _ in range(50):
        m.zero_grad(set_to_none=True)
        losses = m.get_loss_dict(m.get_train_outputs(frame), batch)
        mains.append(losses["main_loss"].detach())
        sum(losses.values()).backward()
        opts.optimizer_step_all()
        opts.scheduler_step_all()
    with torch.no_grad():
        last = m.get_loss_dict(m.get_train_outputs(frame), batch)["main_loss"]
    print(f"drift: main_loss {float(mains[0]):.6f} -> {float(last):.6f} after 50 steps on the grid")
    assert float(last) < float(mains[0])
    assert not torch.equal(m.bil_grids.detach()[1], before[1])
    assert torch.equal(m.bil_grids.detach()[0], before[0])  # a frame never visited: zero gradient, zero moments, no movement


def test_1080p_smoke():
    grids, image, v = bf.random_grids(1, 3, (16, 16, 8), 51), bf.random_image(1080, 1920, 3, 52), bf.random_upstream(1080, 1920, 3, 53)
    out, g_img, g_grid = _hip(grids, 0, image, v)
    torch.cuda.synchronize()
    for t, shape in ((out, (1080, 1920, 3)), (g_img, (1080, 1920, 3)), (g_grid, (1, 12, 8, 16, 16))):
        assert t.shape == shape and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0
    assert float(g_grid.abs().min()) > 0  # every vertex is reached


def test_1080p_every_pixel_is_gathered_exactly_once():
    """The interpolation weights of a pixel add up to 1, so with an upstream gradient of ones the offset's gradient over the whole grid adds up to
    the number of pixels and the gain's to the sum of the image: a pixel the vertex rectangles or their eight row slices missed, or took twice,
    would change either sum by about 1.  (Rounding: 4096 entries of about 500 each, a few 1e-5 apiece.)"""
    H, W = 1080, 1920
    image = bf.random_image(H, W, 1, 61)
    _, g_img, g_grid = _hip(bf.random_grids(1, 1, (16, 16, 8), 62), 0, image, torch.ones(H, W, 1))
    gain, offset = g_grid[0, 0].double().sum().item(), g_grid[0, 1].double().sum().item()
    print(f"1080p partition of unity: offset gradient sums to {offset:.4f} for {H * W} pixels, gain gradient to {gain:.4f} for {image.double().sum().item():.4f}")
    assert abs(offset - H * W) < 0.5 and abs(gain - image.double().sum().item()) < 0.5
