"""The differentiable depth without a GPU: the restatement of tests/splat_depth_functional.py against splat_functional's own depth and against
central finite differences, the float32 floors of every configuration the GPU test runs (a condition on the scenes, measured here), the depth
losses' restatement, the config's refusals, and the new entry points in the header, the bindings and the call layer."""
import ctypes as C
import os
import re

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
import splat_abi
import splat_backward_cases as bc
import splat_depth_functional as df
import thermal_reg_functional as trf
from nerfstudio_thermal_amd import _lib, splat_calls
from nerfstudio_thermal_amd.splat import ThermalSplatfactoModelConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the depth groups live in the two backward entry points and their size function (the names they replaced: splat_abi.RETIRED)
NEW_NAMES = ("tn_splat_backward_workspace_bytes", "tn_splat_raster_backward", "tn_splat_project_backward", "tn_depth_loss_workspace_bytes", "tn_depth_loss")


@pytest.mark.parametrize("cfg", [df.SHARED_CONFIGS[0], df.SHARED_CONFIGS[5], df.SEP_CONFIGS[0]], ids=df.config_id)
def test_float64_depth_equals_the_forward_restatement(cfg):
    case, deg, sep, _ = cfg
    p = {k: v.double() for k, v in df.scene(cfg).items()}
    with torch.no_grad():
        mine = df.render(p, cfg)
        theirs = bc._render(p, case, df.MODE, deg, sep, with_depth=True)
    for k in ("depth", "rgb", "thermal", "accumulation"):
        assert torch.equal(mine[k], theirs[k]), k
    assert torch.equal(mine["flag_pixels"], theirs["flag_pixels"])
    assert bool((mine["accumulation"] > 0).any())
    if case == "single":  # both branches of the depth are on the frame
        assert bool((mine["accumulation"] == 0).any()) and float(mine["depth"][mine["accumulation"] == 0].max()) == float(mine["depth_raw"].max())


@pytest.mark.parametrize("cfg", [df.SHARED_CONFIGS[5], df.SHARED_CONFIGS[0]], ids=df.config_id)
def test_float64_gradient_passes_a_central_difference_check(cfg):
    """g64 = gA + gB (the two partial graphs) against central differences of the UNDIVIDED loss sum(output * w) + sum(depth * v_depth) along random
    directions in every parameter: 1e-6 of the directional derivative's own scale (h = 1e-6 in float64: truncation h^2, rounding 1e-16 / h)."""
    ref = df.reference(cfg)
    p64 = {k: v.double() for k, v in ref["p"].items()}
    gen = torch.Generator().manual_seed(11)
    fill = ref["out64"]["depth_raw"].max()
    for name in df.UPSTREAMS:
        vd = ref["v_depth"][name]

        def loss(q):
            with torch.no_grad():
                out = df.render(q, cfg, colors_from={**q, "means": p64["means"]})  # view directions of the unperturbed means: they carry no gradient
                depth = torch.where(out["accumulation"] > 0, out["depth"], fill)  # the fill value is detached: a constant of the frame
                return float(sum((out[k] * ref["w"][k]).sum() for k in ref["w"]) + (depth * vd).sum())

        for k in bc.param_names(cfg[2]):
            if p64[k].numel() == 0:
                continue
            direction = torch.randn(p64[k].shape, generator=gen, dtype=torch.float64)
            h = 1e-6
            fd = (loss({**p64, k: p64[k] + h * direction}) - loss({**p64, k: p64[k] - h * direction})) / (2 * h)
            an = float((ref["g64"][name][k] * direction).sum())
            size = float((ref["gA"][name][k].abs() * direction.abs()).sum() + (ref["gB"][name][k].abs() * direction.abs()).sum())
            print(f"{df.config_id(cfg)}-{name} {k}: finite difference {fd:.9e}, autograd {an:.9e}, scale {size:.3e}")
            assert abs(fd - an) <= 1e-6 * size, (name, k, fd, an)


def test_single_cancels_under_a_depth_only_upstream():
    """One Gaussian: depth = z wherever it is seen, whatever alpha is.  The two partial gradients of a depth-only loss are each of order 1 and cancel
    for the scales, quats, opacities and xys to ~1e-13: the reason errors are measured against the partials."""
    cfg = df.SHARED_CONFIGS[5]
    ref = df.reference(cfg)
    zero_w = {k: torch.zeros_like(v) for k, v in ref["w"].items()}
    parts, _ = df.autograd_grads(ref["p"], cfg, zero_w, {"raw": ref["v_depth"]["raw"]}, torch.float64, parts=True)
    gA, gB = parts["raw"]
    for k in ("scales", "quats", "opacities", "xys"):
        part, total = max(bc.amax(gA[k]), bc.amax(gB[k])), bc.amax(gA[k] + gB[k])
        print(f"single {k}: partials {part:.3e}, sum {total:.3e}")
        assert part > 1e-3 and total <= 1e-10 * part, (k, part, total)
    assert bc.amax(gA["means"] + gB["means"]) > 1e-3  # the mean moves z itself


@pytest.mark.parametrize("cfg", df.CONFIGS, ids=df.config_id)
def test_float32_floors_meet_the_caps(cfg):
    """Per configuration and gradient tensor the floor max(err(g32), err(walk32), 2^-23) against g64, relative to the partial gradients' scale: under
    the suite's cap for both upstreams, with the scene conditions of tests/splat_backward_cases.py.  The float64 walk agrees with float64 autograd to
    1e-9: the walk with five channels and v_alpha_eff IS the derivative."""
    ref = df.reference(cfg)
    excl = ref["excl"]
    assert ref["flagged"] <= bc.MAX_FLAGGED_PIXELS and int(excl.sum()) <= bc.MAX_EXCLUDED_GAUSSIANS * excl.numel()
    w64 = df.walk64(cfg) if cfg in (df.SHARED_CONFIGS[0], df.SHARED_CONFIGS[5], df.POSE_CONFIG) else None
    for name in df.UPSTREAMS:
        fl = df.floors(ref, name, excl, cfg)
        print(f"{df.config_id(cfg)}-{name}: flagged {ref['flagged']:.4f}, " + ", ".join(f"{k} {v[0]:.2e}" for k, v in fl.items()))
        for k, (floor, _, _) in fl.items():
            assert floor <= df.max_floor(name), (name, k, floor)
            if w64 is not None:
                assert df.err(w64[name][k], ref, name, k, excl) <= 1e-9, (name, k)


def test_depth_losses_restatement_agrees_with_autograd_and_the_plain_tv():
    depth, acc, sensor = (t.double() for t in df.loss_frame(17, 33, 1, border=3))
    x = depth.clone().requires_grad_(True)
    l_d, l_tv = df.depth_losses(x, acc, sensor, 0.75, 1.5)
    (l_d + l_tv).backward()
    cov = acc[..., 0] > 0
    s = sensor[..., 0]
    valid = cov & torch.isfinite(s) & (s > 0)
    assert 0 < int(valid.sum()) < int(cov.sum()) < cov.numel()
    want_d = 0.75 * float((depth[..., 0] - s)[valid].abs().mean())
    assert abs(float(l_d.detach()) - want_d) <= 1e-12 * want_d
    g_d = torch.zeros_like(depth[..., 0])
    g_d[valid] = 0.75 * torch.sign(depth[..., 0] - s)[valid] / int(valid.sum())
    # the TV on the covered interior alone is thermal_reg_functional.tv of that crop (every window of the crop is covered)
    inner = depth[3:-3, 3:-3].clone().requires_grad_(True)
    tv = 1.5 * trf.tv(inner)
    tv.backward()
    assert abs(float(l_tv.detach()) - float(tv.detach())) <= 1e-12 * float(tv.detach())
    g_tv = torch.zeros_like(depth[..., 0])
    g_tv[3:-3, 3:-3] = inner.grad[..., 0]
    assert float((x.grad[..., 0] - (g_d + g_tv)).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    assert bc.amax(x.grad[..., 0][~cov]) == 0.0
    none = df.depth_losses(depth, torch.zeros_like(acc), sensor, 0.75, 1.5)
    assert float(none[0]) == 0.0 and float(none[1]) == 0.0
    assert float(df.depth_losses(depth, acc, None, 0.75, 1.5)[0]) == 0.0


def test_config_refusals():
    with pytest.raises(ValueError, match="chain of its own"):
        ThermalSplatfactoModelConfig(differentiable_depth=True, rasterize_mode="antialiased")
    for name in ("depth_loss_mult", "depth_tv_loss_mult"):
        with pytest.raises(ValueError, match="needs differentiable_depth"):
            ThermalSplatfactoModelConfig(**{name: 0.1})
        with pytest.raises(ValueError, match="negative"):
            ThermalSplatfactoModelConfig(differentiable_depth=True, **{name: -0.1})
        assert getattr(ThermalSplatfactoModelConfig(differentiable_depth=True, **{name: 0.1}), name) == 0.1
    cfg = ThermalSplatfactoModelConfig()
    assert cfg.differentiable_depth is False and cfg.depth_loss_mult == 0.0 and cfg.depth_tv_loss_mult == 0.0


def test_new_names_are_in_the_header_the_map_and_the_bindings():
    hdr = splat_abi.header()
    declared = set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", hdr))
    exports = open(os.path.join(ROOT, "nerfstudio-thermal_amd", "csrc", "exports.map")).read()
    assert "global: tn_*;" in exports  # the map exports the prefix, so every declared name is covered
    src = open(os.path.join(ROOT, "nerfstudio-thermal_amd", "splat_calls.py")).read()
    for name in NEW_NAMES:
        assert name in declared and name.startswith("tn_"), name
        assert name in _lib.SIGNATURES, name
        assert f'"{name}"' in src, name  # spelled as a literal in the call layer
    for name in splat_abi.RETIRED:
        assert name not in declared and name not in _lib.SIGNATURES and name not in src, name
    assert _lib.ABI_VERSION == 314
    for name, group in (("tn_splat_raster_backward", ["depth", "v_depth", "v_depths"]), ("tn_splat_project_backward", ["v_depths"])):
        assert [p for p in splat_abi.param_names(hdr, name) if p in group] == group and "antialiased" in splat_abi.param_names(hdr, name)


def test_library_exports_and_refuses_without_a_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = _lib.load()
    assert lib.tn_version() == 314
    splat_abi.assert_unified(lib, NEW_NAMES)
    size = lib.tn_splat_backward_workspace_bytes
    for sep in (0, 1):
        for absgrad in (0, 1):
            al = lambda x: (x + 255) // 256 * 256  # noqa: E731
            sums = 10 + sep + 2 * absgrad  # per pair without the depth slot
            assert size(1000, 5000, sep, absgrad, 0) == al(4 * sums * 5000) + al(4 * 1000)
            assert size(1000, 5000, sep, absgrad, 1) == al(4 * (sums + 1) * 5000) + al(4 * 1000)
            assert (size(10, 100, sep, absgrad, 1), size(1000, 5000, sep, absgrad, 1)) == splat_abi.BACKWARD_WORKSPACE_BYTES[(sep, absgrad, 1)]
    assert size(-1, 0, 0, 0, 1) == -1 and size(0, -1, 1, 1, 1) == -1
    assert lib.tn_depth_loss_workspace_bytes(1, 5) == -1 and lib.tn_depth_loss_workspace_bytes(37, 70) > 0
    cam = _lib.TnSplatCamera()
    one = C.c_void_p(256)  # never read: the refusal comes first
    rc = lib.tn_splat_raster_backward(C.byref(cam), 1, one, 1, 1, one, 1, *[one] * 9, 1 << 20, *[one] * 9, None)
    assert rc == -22 and b"classic mode only" in lib.tn_last_error()
    rc = lib.tn_splat_project_backward(C.byref(cam), None, None, *[one] * 8, None, 1, 0, 0, 1, *[one] * 6, one, *[one] * 8, None, None, 0, None, None, None)
    assert rc == -22 and b"classic mode only" in lib.tn_last_error()
    assert lib.tn_depth_loss(None, None, None, 8, 8, 1.0, 1.0, None, 0, None, None, None) == -22 and b"null pointer" in lib.tn_last_error()
    assert lib.tn_depth_loss(one, one, None, 8, 8, -1.0, 1.0, one, 1 << 20, one, None, None) == -22 and b"negative" in lib.tn_last_error()


def test_the_call_layer_passes_as_many_arguments_as_the_bindings_declare(monkeypatch):
    """The depth tensors through the call layer (tests/test_splat_calls_cpu.py checks every combination of every stage's groups and where the Nones
    sit): with and without them the two backward stages go to their one entry point, and the depth loss to its own."""
    sc, seen = splat_calls, []
    monkeypatch.setattr(sc, "_call", lambda name, *args: seen.append((name, len(args) + 1)))  # + the stream
    monkeypatch.setattr(sc, "_ptr", lambda t, dtype, name: None if t is None else C.c_void_p(1))
    monkeypatch.setattr(sc, "_raw", lambda t: None if t is None else C.c_void_p(1))
    monkeypatch.setattr(sc, "_pose_row_ptr", lambda *a, **k: C.c_void_p(1))
    monkeypatch.setattr(sc, "workspace", lambda *a, **k: torch.empty(4, dtype=torch.uint8))
    cam, bg, T = _lib.TnSplatCamera(), (C.c_float * 4)(), torch.zeros
    for n in (8, 9):
        P = [T(5, 3), T(5, 3), T(5, 4), T(5, 1), T(5, 3), T(5, 15, 3), T(5, 1), T(5, 15, 1), T(5, 1)][:n]
        th = T(5) if n == 9 else None
        for pose in ((), (T(40), T(2, 6), 0, T(2, 6), T(3, 4))):
            sc.project_backward(cam, P, 3, 0, T(5), T(5), T(5), T(5), T(5), P, th, *pose, v_depths=T(5))
        for v_abs in (None, T(1)):
            sc.raster_backward(cam, 5, T(4), 10, 7, bg, *[T(1)] * 9, *([th] * 4 if n == 9 else []), v_xys_abs=v_abs, aa=0, depth=T(1), v_depth=T(1), v_depths=T(5))
            sc.raster_backward(cam, 5, T(4), 10, 7, bg, *[T(1)] * 9, *([th] * 4 if n == 9 else []), v_xys_abs=v_abs)
    sc.depth_loss(T(1), T(1), None, 8, 8, 1.0, 1.0, T(2), None)
    assert {name for name, _ in seen} == {"tn_splat_raster_backward", "tn_splat_project_backward", "tn_depth_loss"}
    assert [(name, n) for name, n in seen if n != len(_lib.SIGNATURES[name][1])] == []
