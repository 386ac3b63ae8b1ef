"""The splat training loss without a GPU: the torch restatement (ssim_functional.py) against an independent numpy / scipy computation of the
definition, known answers and float64 finite differences, and the host-side argument checks of tn_image_loss."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib

import ssim_functional as sf

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _numpy_ssim(x: np.ndarray, y: np.ndarray) -> float:
    """The definition from scratch: scipy's 1-D correlation along each axis (valid part only), per channel."""
    from scipy.ndimage import correlate1d

    coords = np.arange(11, dtype=np.float32) - 5
    g = np.exp(-(coords ** 2) / (2 * np.float32(1.5) ** 2)).astype(np.float32)
    g = (g / g.sum()).astype(np.float64)
    assert np.abs(g - sf.gauss_window().numpy()).max() < 1e-7

    def filt(a):
        a = correlate1d(a, g, axis=0, mode="constant")[5:-5]
        return correlate1d(a, g, axis=1, mode="constant")[:, 5:-5]

    vals = []
    for c in range(x.shape[2]):
        a, b = x[..., c], y[..., c]
        mx, my = filt(a), filt(b)
        sxx, syy, sxy = filt(a * a) - mx * mx, filt(b * b) - my * my, filt(a * b) - mx * my
        s = (2 * mx * my + sf.C1) / (mx * mx + my * my + sf.C1) * (2 * sxy + sf.C2) / (sxx + syy + sf.C2)
        vals.append(s.mean())
    return float(np.mean(vals))


@pytest.mark.parametrize("h,w,c", [(11, 11, 1), (23, 31, 3), (40, 29, 4)])
def test_restatement_matches_numpy(h, w, c):
    pred, gt = sf.correlated_pair(h, w, c, seed=h + w)
    want = _numpy_ssim(pred.numpy(), gt.numpy())
    got = float(sf.ssim(pred, gt))
    # numpy's and torch's fp32 exp round a few window taps differently (1 ulp); the variances amplify that to ~1e-6
    assert abs(got - want) < 1e-5, (got, want)
    assert 0.0 < got < 0.99  # a real, imperfect match (the GPU tests rely on these pairs being non-trivial)


def test_known_answers():
    pred, gt = sf.correlated_pair(30, 40, 3, seed=3)
    assert abs(float(sf.ssim(gt, gt)) - 1.0) < 1e-12
    x = gt.clone().requires_grad_(True)
    sf.ssim(x, gt).backward()
    assert float(x.grad.abs().max()) < 1e-12  # SSIM is at its maximum at x = y
    x = gt.clone().requires_grad_(True)
    sf.l1(x, gt).backward()
    assert float(x.grad.abs().max()) == 0.0  # sign(0) = 0, as torch's abs backward
    assert float(sf.main_loss(gt, gt, 0.2)) == pytest.approx(0.0, abs=1e-12)


def test_restatement_gradient_against_finite_differences():
    pred, gt = sf.correlated_pair(14, 17, 2, seed=5)
    x = pred.clone().requires_grad_(True)
    sf.main_loss(x, gt, 0.2, 1.7).backward()
    gen = torch.Generator().manual_seed(0)
    eps = 1e-6
    for _ in range(25):
        i, j, c = (int(torch.randint(0, n, (1,), generator=gen)) for n in pred.shape)
        if abs(float(pred[i, j, c] - gt[i, j, c])) < 10 * eps:
            continue  # the L1 kink
        p, m = pred.clone(), pred.clone()
        p[i, j, c] += eps
        m[i, j, c] -= eps
        fd = float(sf.main_loss(p, gt, 0.2, 1.7) - sf.main_loss(m, gt, 0.2, 1.7)) / (2 * eps)
        assert abs(fd - float(x.grad[i, j, c])) < 1e-7 + 1e-5 * abs(fd), (i, j, c, fd, float(x.grad[i, j, c]))


def test_gradient_formula_of_the_kernel_matches_autograd():
    """The a / b / c maps and the transposed filtering that k_ssim_fwd / k_ssim_bwd implement, in float64, against autograd."""
    pred, gt = sf.correlated_pair(25, 21, 3, seed=9)
    x = pred.clone().requires_grad_(True)
    sf.ssim(x, gt).backward()
    g = sf.gauss_window()
    X, Y = pred.permute(2, 0, 1)[None], gt.permute(2, 0, 1)[None]
    mx, my = sf.gaussian_filter(X, g), sf.gaussian_filter(Y, g)
    sxx = sf.gaussian_filter(X * X, g) - mx * mx
    syy = sf.gaussian_filter(Y * Y, g) - my * my
    sxy = sf.gaussian_filter(X * Y, g) - mx * my
    ad, D = mx * mx + my * my + sf.C1, sxx + syy + sf.C2
    A, B = (2 * mx * my + sf.C1) / ad, (2 * sxy + sf.C2) / D
    a = B * (2 * my - 2 * mx * A) / ad + A * (2 * mx * B - 2 * my) / D
    b = -A * B / D
    c = 2 * A / D
    Cc = X.shape[1]

    def gt_filter(m):  # the transposed ("full") correlation of a valid-region map
        k = (g[:, None] * g[None, :]).view(1, 1, 11, 11).repeat(Cc, 1, 1, 1)
        return torch.nn.functional.conv_transpose2d(m, k, groups=Cc)

    n = Cc * mx.shape[2] * mx.shape[3]
    grad = (gt_filter(a) + 2 * X * gt_filter(b) + Y * gt_filter(c)) / n
    assert float((grad[0].permute(1, 2, 0) - x.grad).abs().max()) < 1e-14


def test_workspace_size(lib):
    assert lib.tn_image_loss_workspace_bytes(10, 11, 3) == -1
    assert lib.tn_image_loss_workspace_bytes(11, 10, 3) == -1
    assert lib.tn_image_loss_workspace_bytes(11, 11, 0) == -1
    assert lib.tn_image_loss_workspace_bytes(11, 11, 5) == -1
    small, big = lib.tn_image_loss_workspace_bytes(100, 100, 1), lib.tn_image_loss_workspace_bytes(100, 100, 3)
    assert 0 < small < big and big - small >= 2 * 3 * 90 * 90 * 4 - 512  # three derivative maps per channel over the valid pixels


def test_image_loss_argument_validation(lib):
    d = C.c_void_p(256)  # never dereferenced: every call below is refused before anything is read or launched
    need = lib.tn_image_loss_workspace_bytes(20, 30, 3)

    def call(pred=d, ps=3, gt=d, gs=3, h=20, w=30, c=3, ws=d, wsb=need, out=d, grad=d):
        return lib.tn_image_loss(pred, ps, gt, gs, h, w, c, 0.2, 1.0, ws, wsb, out, grad, None)

    for kw in ({"pred": None}, {"gt": None}, {"ws": None}, {"out": None}):
        assert call(**kw) == EINVAL
        assert b"null pointer" in lib.tn_last_error()
    assert call(h=10) == EINVAL
    assert call(w=10) == EINVAL
    assert b"window" in lib.tn_last_error()
    assert call(c=0) == EINVAL
    assert call(c=5) == EINVAL
    assert b"channels" in lib.tn_last_error()
    assert call(ps=2) == EINVAL
    assert call(gs=2) == EINVAL
    assert b"pixel strides" in lib.tn_last_error()
    assert call(wsb=need - 1) == EINVAL
    assert b"workspace" in lib.tn_last_error()
    assert call(h=1 << 16) == EINVAL


def test_model_config_has_the_reference_loss_defaults():
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModelConfig

    cfg = ThermalSplatfactoModelConfig()
    assert (cfg.ssim_lambda, cfg.use_scale_regularization, cfg.max_gauss_ratio, cfg.thermal_loss_mult) == (0.2, False, 10.0, 1.0)
    assert cfg.background_color == "black"


def test_image_loss_refuses_cpu_tensors():
    from nerfstudio_thermal_amd.splat import image_loss

    with pytest.raises(ValueError, match="no CPU fallback"):
        image_loss(torch.zeros(16, 16, 3), torch.zeros(16, 16, 3))
