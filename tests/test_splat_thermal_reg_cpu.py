"""The splat model's thermal regularisers without a GPU: the torch restatement (thermal_reg_functional.py) against the oracle's tv_pixel_loss /
cross_channel_loss (pinned to the reference's goldens) fed the stacked stride-1 windows, the gather formula tn_thermal_reg's kernel implements
against autograd, the header / binding / export of the two new entry points, the host-side argument checks and the model's config."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib

import thermal_nerfacto_oracle as orc
import thermal_reg_functional as trf

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"tn_thermal_reg", "tn_thermal_reg_workspace_bytes"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize("make", [trf.random_pair, trf.smooth_pair])
@pytest.mark.parametrize("h,w", [(2, 2), (2, 7), (5, 3), (23, 31), (72, 96)])
def test_restatement_matches_the_oracle_on_the_stacked_windows(h, w, make):
    pred, gt = make(h, w, seed=h * w)
    assert pred.dtype == torch.float64
    # the reference's batch: 4 rays per window, window after window
    rows = torch.stack([trf.windows(pred[..., 0])] + [trf.windows(gt[..., c]) for c in range(3)], dim=-1).reshape(-1, 4)
    assert rows.shape[0] == 4 * (h - 1) * (w - 1)
    is_thermal = torch.zeros(rows.shape[0], dtype=torch.float64)
    want_tv = orc.tv_pixel_loss(rows[:, 0:1], is_thermal)
    want_cc = orc.cross_channel_loss(rows[:, 0:1], rows[:, 1:4], is_thermal)
    assert float(want_tv) > 0 and float(want_cc) > 0
    torch.testing.assert_close(trf.tv(pred), want_tv, rtol=1e-12, atol=0)
    torch.testing.assert_close(trf.cross(pred, gt), want_cc, rtol=1e-12, atol=0)
    tv, cc = trf.regularizers(pred, gt, 0.75, 1.5)
    torch.testing.assert_close(tv, 0.75 * want_tv, rtol=1e-12, atol=0)
    torch.testing.assert_close(cc, 1.5 * want_cc, rtol=1e-12, atol=0)


def test_window_order():
    img = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    assert trf.windows(img).tolist() == [[0, 1, 4, 5], [1, 2, 5, 6], [2, 3, 6, 7], [4, 5, 8, 9], [5, 6, 9, 10], [6, 7, 10, 11]]


def test_known_answers():
    flat = torch.full((6, 9, 1), 0.3, dtype=torch.float64, requires_grad=True)
    gt = torch.full((6, 9, 3), 0.8, dtype=torch.float64)
    tv, cc = trf.regularizers(flat, gt, 1.0, 1.0)
    (tv + cc).backward()
    assert float(tv.detach()) == 0.0 and float(cc.detach()) == 0.0 and float(flat.grad.abs().max()) == 0.0  # sign(0) = 0, as torch.abs' backward
    # a horizontal ramp of slope s: two of a window's four TV terms are s, and a grey ramp of the same slope cancels the cross term
    ramp = (0.01 * torch.arange(9, dtype=torch.float64)).expand(6, 9)[..., None]
    assert float(trf.tv(ramp)) == pytest.approx(0.25 * 2 * 0.01, rel=1e-12)
    assert float(trf.cross(ramp, ramp.expand(-1, -1, 3))) == pytest.approx(0.0, abs=1e-15)
    assert float(trf.cross(ramp, gt)) == pytest.approx(float(trf.tv(ramp)), rel=1e-12)  # a flat ground truth: the cross term is the TV
    tv0, cc0 = trf.regularizers(ramp, gt, 0.0, 0.0)
    assert float(tv0) == 0.0 and float(cc0) == 0.0


def _gather_gradient(pred, gt, tv_mult, cross_mult):
    """What k_thermal_reg computes per pixel, in torch: an edge is in as many windows as it has window rows (columns) around it, the loss sums
    every pixel's right and lower edge with that weight, and a pixel's gradient is the signed count over its four edges."""
    t, q = pred[..., 0], gt.mean(-1)
    H, W = t.shape
    rows, cols = torch.arange(H), torch.arange(W)
    mh = ((rows > 0).to(t.dtype) + (rows < H - 1).to(t.dtype))[:, None]  # windows holding a horizontal edge of this row
    mv = ((cols > 0).to(t.dtype) + (cols < W - 1).to(t.dtype))[None, :]
    loss, grad = [], torch.zeros_like(t)
    for mult, right, down, s in ((tv_mult, t[:, :-1] - t[:, 1:], t[:-1] - t[1:], 1.0),
                                 (cross_mult, (t[:, 1:] - t[:, :-1]) - (q[:, 1:] - q[:, :-1]), (t[1:] - t[:-1]) - (q[1:] - q[:-1]), -1.0)):
        c = mult * 0.25 / ((H - 1) * (W - 1))
        loss.append(c * ((mh * right.abs()).sum() + (mv * down.abs()).sum()))
        gr, gd = s * c * mh * torch.sign(right), s * c * mv * torch.sign(down)  # d / d the edge's earlier pixel; the later one gets the negative
        grad[:, :-1] += gr
        grad[:, 1:] -= gr
        grad[:-1] += gd
        grad[1:] -= gd
    return loss[0], loss[1], grad[..., None]


@pytest.mark.parametrize("h,w", [(2, 2), (2, 5), (4, 3), (17, 23)])
@pytest.mark.parametrize("mults", [(0.75, 0.0), (0.0, 1.5), (0.75, 1.5)])
def test_gather_formula_of_the_kernel_matches_autograd(h, w, mults):
    pred, gt = trf.random_pair(h, w, seed=h + w)
    x = pred.clone().requires_grad_(True)
    tv, cc = trf.regularizers(x, gt, *mults)
    (tv + cc).backward()
    g_tv, g_cc, g = _gather_gradient(pred, gt, *mults)
    torch.testing.assert_close(g_tv, tv.detach(), rtol=1e-12, atol=0)
    torch.testing.assert_close(g_cc, cc.detach(), rtol=1e-12, atol=0)
    assert float((g - x.grad).abs().max()) <= 1e-14 * float(x.grad.abs().max())


def test_near_tie_share_of_the_gpu_tests_inputs():
    """The shares the GPU test's exclusion rule relies on (bound: 0.2 % of the terms)."""
    for pair in (trf.random_pair(72, 96, seed=1), trf.random_pair(480, 640, seed=2), trf.smooth_pair(72, 96, seed=3)):
        pred, gt = (v.float().double() for v in pair)  # the GPU test's inputs are fp32
        mask, share = trf.near_ties(pred, gt, 1.0, 1.0)
        print(f"{tuple(pred.shape[:2])}: share of near-tie terms {share:.2e}")
        assert share <= 2e-3, share
        assert int(mask.sum()) <= 2 * share * 8 * mask.numel() + 1e-9
    mask, share = trf.near_ties(torch.zeros(4, 4, 1, dtype=torch.float64), torch.zeros(4, 4, 3, dtype=torch.float64), 1.0, 0.0)
    assert share == 1.0 and bool(mask.all())


def _header_symbols():
    hdr = open(os.path.join(ROOT, "include", "thermal_nerf_hip.h")).read()
    return set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", hdr))


def test_header_binding_and_exports_agree(lib):
    assert SYMBOLS <= _header_symbols()
    assert SYMBOLS <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 314 and lib.tn_version() == 314
    res, args = _lib.SIGNATURES["tn_thermal_reg"]
    assert res is C.c_int and len(args) == 13 and args[6] is C.c_float and args[7] is C.c_float
    assert _lib.SIGNATURES["tn_thermal_reg_workspace_bytes"] == (C.c_int64, [C.c_int32, C.c_int32])
    # csrc/exports.map exports the header's tn_ prefix and nothing else
    exports = open(os.path.join(ROOT, "nerfstudio-thermal_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*tn_\*;", exports) and re.search(r"local:\s*\*;", exports)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    if shutil.which("nm") is not None:
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert SYMBOLS <= {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_workspace_size(lib):
    for h, w in ((1, 8), (8, 1), (0, 0), (-3, 8), (32769, 8), (8, 32769)):
        assert lib.tn_thermal_reg_workspace_bytes(h, w) == -1
    small, big = lib.tn_thermal_reg_workspace_bytes(2, 2), lib.tn_thermal_reg_workspace_bytes(1080, 1920)
    assert 0 < small < big < 1 << 20  # per-block partial sums only
    assert lib.tn_thermal_reg_workspace_bytes(32768, 32768) > big


def test_thermal_reg_argument_validation(lib):
    d = C.c_void_p(256)  # never dereferenced: every call below is refused before anything is read or launched
    need = lib.tn_thermal_reg_workspace_bytes(20, 30)

    def call(pred=d, ps=1, gt=d, gs=3, h=20, w=30, ws=d, wsb=need, out=d, grad=d):
        return lib.tn_thermal_reg(pred, ps, gt, gs, h, w, 1.0, 1.0, ws, wsb, out, grad, None)

    for kw in ({"pred": None}, {"gt": None}, {"ws": None}, {"out": None}):
        assert call(**kw) == EINVAL
        assert b"null pointer" in lib.tn_last_error()
    for kw in ({"h": 1}, {"w": 1}, {"h": 0}, {"w": -2}):
        assert call(**kw) == EINVAL
        assert b"2 x 2" in lib.tn_last_error()
    for kw in ({"h": 32769}, {"w": 1 << 16}):
        assert call(**kw) == EINVAL
        assert b"larger than" in lib.tn_last_error()
    for kw in ({"ps": 0}, {"gs": 2}, {"gs": 1}):
        assert call(**kw) == EINVAL
        assert b"pixel strides" in lib.tn_last_error()
    assert call(wsb=need - 1) == EINVAL
    assert b"workspace" in lib.tn_last_error()
    assert call(wsb=0) == EINVAL


def test_model_config_has_the_regularisers_off_by_default():
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModelConfig

    cfg = ThermalSplatfactoModelConfig()
    assert cfg.tv_pixel_loss_mult == 0.0 and cfg.cross_channel_loss_mult == 0.0
    cfg = ThermalSplatfactoModelConfig(tv_pixel_loss_mult=1e-6, cross_channel_loss_mult=2e-6)
    assert (cfg.tv_pixel_loss_mult, cfg.cross_channel_loss_mult) == (1e-6, 2e-6)
    with pytest.raises(ValueError, match="tv_pixel_loss_mult"):
        ThermalSplatfactoModelConfig(tv_pixel_loss_mult=-1e-6)
    with pytest.raises(ValueError, match="cross_channel_loss_mult"):
        ThermalSplatfactoModelConfig(cross_channel_loss_mult=-1.0)


def test_thermal_regularizers_refuses_cpu_tensors_and_bad_shapes():
    from nerfstudio_thermal_amd.splat import thermal_regularizers

    with pytest.raises(ValueError, match="no CPU fallback"):
        thermal_regularizers(torch.zeros(16, 16, 1), torch.zeros(16, 16, 3), 1.0, 1.0)
    with pytest.raises(ValueError, match=r"\[H,W,1\]"):
        thermal_regularizers(torch.zeros(16, 16, 3), torch.zeros(16, 16, 3), 1.0, 1.0)
    with pytest.raises(ValueError, match=r"\[H,W,1\]"):
        thermal_regularizers(torch.zeros(16, 16, 1), torch.zeros(16, 15, 3), 1.0, 1.0)
    with pytest.raises(ValueError, match="negative"):
        thermal_regularizers(torch.zeros(16, 16, 1), torch.zeros(16, 16, 3), -1.0, 1.0)
