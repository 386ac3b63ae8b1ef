"""Mip-Splatting's 3D smoothing filter without a GPU: the float64 restatement (splat_filter3d_functional.py) against autograd and against the rule
it states, the host helper `filter_camera_table`, the config's refusals, and the binding of the three entry points."""
import ctypes as C
import inspect
import math
import os

import pytest
import torch

import splat_filter3d_functional as ff

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib, splat, splat_calls, splat_filter, splat_io
from nerfstudio_thermal_amd.splat_camera import PinholeCamera, camera_struct
from nerfstudio_thermal_amd.synth import look_at_camera

F64 = torch.float64
NAMES = ("tn_filter3d_splat_compute", "tn_filter3d_splat_apply", "tn_filter3d_splat_apply_backward")


def _rows(n: int, seed: int, lo_scale=-4.0, hi_scale=1.0, max_logit=6.0, ratios=(0.1, 10.0)):
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(*s, generator=g, dtype=F64)  # noqa: E731
    scales = u(lo_scale, hi_scale, n, 3)
    ratio = torch.exp(u(math.log(ratios[0]), math.log(ratios[1]), n))
    f = ratio * torch.exp(scales[:, 0])
    f[::7] = 0.0
    return scales, u(-max_logit, max_logit, n, 1), u(-max_logit, max_logit, n, 1), f, g


@pytest.mark.parametrize("sep", [False, True])
def test_closed_form_backward_matches_float64_autograd(sep):
    scales, o, oth, f, g = _rows(257, 3)
    leaves = [t.clone().requires_grad_(True) for t in ([scales, o, oth] if sep else [scales, o])]
    outs = ff.apply_forward(leaves[0], leaves[1], f, leaves[2] if sep else None)
    ups = [torch.randn(t.shape, generator=g, dtype=F64) for t in outs]
    auto = torch.autograd.grad(outs, leaves, ups)
    closed, abs_terms = ff.apply_backward(scales, o, f, ups[0], ups[1], oth if sep else None, ups[2] if sep else None)
    for a, c, t in zip(auto, closed, abs_terms):
        err = float((a - c).abs().max())
        print(f"closed form against autograd ({'separate' if sep else 'shared'}): max |err| {err:.3e}, largest term {float(t.max()):.3e}")
        assert err <= 1e-12


@pytest.mark.parametrize("sep", [False, True])
def test_closed_form_backward_at_the_extremes(sep):
    """log-scales -12 and +3, logits +-30, f / s from 1e-4 to 1e4: the error against autograd stays below 1e-12 of the sum of the absolute terms.
    The terms are those of the closed form plus the upstream gradient itself: autograd differentiates o' = (o + log c) - log1p(e^o (1 - c)) as
    g (1 - x / (1 + x)), two terms of size |g| that cancel where the opacity saturates (the closed form has g (1 - p) / (1 - p') there, 1e-13 g,
    without a cancellation), so its own rounding error is of the order of 1e-16 |g| whatever the result."""
    n = 3 * 3 * 3
    ls = torch.tensor([-12.0, 0.0, 3.0], dtype=F64)
    og = torch.tensor([-30.0, 0.0, 30.0], dtype=F64)
    rt = torch.tensor([1e-4, 1.0, 1e4], dtype=F64)
    a, b, c = torch.meshgrid(ls, og, rt, indexing="ij")
    scales = a.reshape(n, 1).repeat(1, 3) + torch.tensor([0.0, 0.3, -0.2], dtype=F64)
    o, oth = b.reshape(n, 1).clone(), b.reshape(n, 1).flip(0).clone()
    f = c.reshape(n) * torch.exp(scales[:, 0])
    leaves = [t.clone().requires_grad_(True) for t in ([scales, o, oth] if sep else [scales, o])]
    outs = ff.apply_forward(leaves[0], leaves[1], f, leaves[2] if sep else None)
    assert all(bool(torch.isfinite(t).all()) for t in outs)
    g = torch.Generator().manual_seed(5)
    ups = [torch.randn(t.shape, generator=g, dtype=F64) for t in outs]
    auto = torch.autograd.grad(outs, leaves, ups)
    closed, abs_terms = ff.apply_backward(scales, o, f, ups[0], ups[1], oth if sep else None, ups[2] if sep else None)
    for x, y, t, up in zip(auto, closed, abs_terms, ups):
        assert bool(torch.isfinite(y).all())
        bound = 1e-12 * (t + up.abs())
        assert bool(((x - y).abs() <= bound).all()), float(((x - y).abs() / bound).max())


def test_the_filtered_opacity_is_the_logit_of_the_compensated_opacity():
    scales, o, _, f, _ = _rows(200, 11)
    s_out, o_out = ff.apply_forward(scales, o, f)
    s2, f2 = torch.exp(2 * scales), (f * f).unsqueeze(-1)
    torch.testing.assert_close(torch.exp(2 * s_out), s2 + f2, rtol=1e-12, atol=0)
    comp = torch.sqrt((s2 / (s2 + f2)).prod(-1, keepdim=True))  # Mip-Splatting eq. 9: sqrt(det Sigma / det(Sigma + f^2 I))
    torch.testing.assert_close(torch.sigmoid(o_out), torch.sigmoid(o) * comp, rtol=1e-12, atol=0)


def test_rows_with_a_zero_filter_are_the_identity():
    scales, o, oth, f, g = _rows(64, 7)
    scales, o, oth = scales.float(), o.float(), oth.float()
    off = f == 0
    assert int(off.sum()) >= 5
    s_out, o_out, th_out = ff.apply_forward(scales, o, f, oth)
    assert torch.equal(s_out[off].float(), scales[off]) and torch.equal(o_out[off].float(), o[off]) and torch.equal(th_out[off].float(), oth[off])
    assert not torch.equal(s_out[~off].float(), scales[~off])
    ups = [torch.randn(t.shape, generator=g, dtype=F64).float() for t in (scales, o, oth)]
    (gs, go, gth), _ = ff.apply_backward(scales, o, f, ups[0], ups[1], oth, ups[2])
    assert torch.equal(gs[off].float(), ups[0][off]) and torch.equal(go[off].float(), ups[1][off]) and torch.equal(gth[off].float(), ups[2][off])
    # a filter of zeros everywhere: nothing changes at all
    z = torch.zeros_like(f)
    assert all(torch.equal(a.float(), b) for a, b in zip(ff.apply_forward(scales, o, z, oth), (scales, o, oth)))


def _cameras():
    rgb = PinholeCamera(look_at_camera((3.0, 0.2, 0.4)), 100.0, 101.0, 48.0, 36.0, 96, 72)
    th = PinholeCamera(look_at_camera((3.0, -0.3, 0.1)), 25.0, 25.5, 24.0, 18.0, 48, 36, cam_idx=1, is_thermal=True)
    return [rgb, th]


def test_filter_camera_table_values_and_shape():
    cams = _cameras()
    table = splat_filter.filter_camera_table(cams)
    assert table.shape == (2, 18) and table.dtype == torch.float32 and table.device.type == "cpu"
    assert splat_calls.FILTER_CAMERA_FLOATS == 18
    for row, cam in zip(table, cams):
        view = torch.tensor(list(camera_struct(cam).viewmat))
        torch.testing.assert_close(row[:12], view, rtol=0, atol=2e-6)  # camera_struct inverts in fp32, the table in float64
        assert row[12:].tolist() == [cam.fx, cam.fy, cam.cx, cam.cy, float(cam.width), float(cam.height)]
        # world -> camera: the camera's own position maps to the origin, a point one unit along its viewing direction to z = +1
        c2w = cam.camera_to_world.double()
        M = row[:12].double().reshape(3, 4)
        eye, ahead = c2w[:, 3], c2w[:, 3] - c2w[:, 2]
        torch.testing.assert_close(M[:, :3] @ eye + M[:, 3], torch.zeros(3, dtype=F64), rtol=0, atol=1e-6)
        torch.testing.assert_close(M[:, :3] @ ahead + M[:, 3], torch.tensor([0.0, 0.0, 1.0], dtype=F64), rtol=0, atol=1e-6)
    assert splat_filter.filter_camera_table([]).shape == (0, 18)


def test_the_rule_is_per_camera_not_the_global_shortcut():
    """A Gaussian only the thermal camera sees is filtered by the thermal focal length over its depth there -- four times the value of the
    official code's shortcut (the largest focal length of all cameras over the smallest depth)."""
    cams = _cameras()
    table = splat_filter.filter_camera_table(cams)
    means = torch.tensor([[0.0, 0.0, 0.0], [0.0, 2.2, 0.0], [9.0, 0.0, 0.0]])  # seen by both | outside the RGB frame's margin | behind both
    seen, _, nu = ff.visibility(means, table, 0.2)
    assert seen.tolist() == [[True, True], [False, True], [False, False]]
    f = ff.compute_filter(means, table, 0.2, 0.2)
    x, y, z, _ = ff._camera_space(means, table)
    sv = math.sqrt(0.2)
    assert float(f[0]) == pytest.approx(sv * float(z[0, 0]) / 101.0, rel=1e-12)  # the RGB camera samples it finest
    assert float(f[1]) == pytest.approx(sv * float(z[1, 1]) / 25.5, rel=1e-12)
    shortcut = sv * float(z[1].min()) / 101.0
    assert float(f[1]) > 3.5 * shortcut
    assert float(f[2]) == float(f.max()) == float(f[1])  # unseen: the largest filter of the seen ones
    assert not ff.compute_filter(means + torch.tensor([50.0, 0.0, 0.0]), table, 0.2, 0.2).any()  # nothing seen: the filter is off
    assert not ff.compute_filter(means, table[:0], 0.2, 0.2).any()
    d = ff.boundary_distance(means, table, 0.2)
    assert d.shape == (3,) and bool((d > 1e-4).all())


def test_config_defaults_and_refusals():
    cfg = splat.ThermalSplatfactoModelConfig()
    assert (cfg.use_3d_filter, cfg.filter_3d_variance, cfg.filter_3d_near, cfg.filter_3d_every) == (False, 0.2, 0.2, 100)
    assert splat.ThermalSplatfactoModelConfig(use_3d_filter=True, rasterize_mode="antialiased", thermal_opacity_mode="separate").use_3d_filter
    with pytest.raises(ValueError, match="mcmc"):
        splat.ThermalSplatfactoModelConfig(use_3d_filter=True, strategy="mcmc")
    for kw in ({"filter_3d_variance": -0.1}, {"filter_3d_near": float("nan")}, {"filter_3d_every": 0}, {"filter_3d_every": 2.5}):
        with pytest.raises(ValueError):
            splat.ThermalSplatfactoModelConfig(**kw)


def test_the_entry_points_are_bound_and_spelled_in_the_call_layer():
    src = inspect.getsource(splat_calls)
    for name in NAMES:
        assert name in _lib.SIGNATURES and f'"{name}"' in src, name
    assert "tn_filter3d_splat_workspace_bytes" in _lib.SIGNATURES
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "thermal_nerf_hip.h")).read()
    assert all(name + "(" in hdr for name in NAMES)
    assert "fuse_3d_filter" in inspect.signature(splat_io.export_gaussian_ply).parameters
    assert splat.apply_3d_filter is splat_filter.apply_3d_filter and splat.compute_3d_filter is splat_filter.compute_3d_filter


def test_arguments_are_validated_on_the_host():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 314 and lib.tn_version() == 314  # additions only: the version stays
    assert lib.tn_filter3d_splat_workspace_bytes(-1) == -1 and lib.tn_filter3d_splat_workspace_bytes(1 << 31) == -1
    assert lib.tn_filter3d_splat_workspace_bytes(0) == 8 and lib.tn_filter3d_splat_workspace_bytes(1037) == 8 * 5
    fake = C.c_void_p(256 * 4096)  # never dereferenced: validation comes before any launch
    assert lib.tn_filter3d_splat_compute(None, 0, None, 0, 0.2, 0.2, None, None, 0, None) == 0  # no Gaussians: nothing to do
    assert lib.tn_filter3d_splat_compute(None, 8, fake, 1, 0.2, 0.2, fake, fake, 8, None) == -22
    assert b"null pointer" in lib.tn_last_error()
    assert lib.tn_filter3d_splat_compute(fake, 1037, fake, 1, 0.2, 0.2, fake, fake, 39, None) == -22
    assert b"workspace of" in lib.tn_last_error()
    assert lib.tn_filter3d_splat_compute(fake, 8, fake, 1, 0.2, -1.0, fake, fake, 8, None) == -22
    assert lib.tn_filter3d_splat_compute(fake, 8, fake, 1, float("nan"), 0.2, fake, fake, 8, None) == -22
    assert lib.tn_filter3d_splat_compute(fake, 8, fake, -1, 0.2, 0.2, fake, fake, 8, None) == -22
    assert lib.tn_filter3d_splat_apply(fake, fake, fake, fake, 8, fake, fake, None, None) == -22  # half a thermal pair
    assert b"thermal" in lib.tn_last_error()
    assert lib.tn_filter3d_splat_apply(fake, fake, None, None, 8, fake, fake, None, None) == -22
    assert lib.tn_filter3d_splat_apply(None, None, None, None, 0, None, None, None, None) == 0
    assert lib.tn_filter3d_splat_apply_backward(fake, fake, None, fake, fake, fake, fake, 8, fake, fake, None, None) == -22
    assert lib.tn_filter3d_splat_apply_backward(fake, fake, None, fake, fake, fake, None, 1 << 31, fake, fake, None, None) == -22
    with pytest.raises(ValueError, match="no CPU fallback"):
        splat_filter.compute_3d_filter(torch.zeros(4, 3), torch.zeros(1, 18))
    with pytest.raises(ValueError):
        splat_filter.apply_3d_filter(torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(5))
