"""The separate thermal opacity (thermal_opacity_mode "separate") without a GPU: configuration, the key sets of both modes, the float64
restatement (tests/splat_sep_functional.py) against the shared one and against hand-written gradient formulas, the both-below cull rule, the
density loss and its detaches, and the ABI of the thermal groups (declared, exported, bound, refusing bad arguments before any launch)."""
import ctypes as C
import os

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib, optim, splat
from nerfstudio_thermal_amd.splat import ThermalSplatfactoModelConfig

import splat_abi
import splat_functional as sf
import splat_oracle as so
import splat_sep_functional as ssf

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the entry points that take the thermal opacity as a nullable group (the _sep names they replaced are splat_abi.RETIRED)
SEP_SYMBOLS = ("tn_splat_project", "tn_splat_raster_chains", "tn_splat_backward_workspace_bytes", "tn_splat_raster_backward", "tn_splat_project_backward",
               "tn_splat_refine_plan", "tn_splat_refine_apply")
# the shared mode's sets as they were before the separate mode existed
SHARED_PARAMS = ("means", "scales", "quats", "opacities", "features_dc", "features_rest", "features_dc_thermal", "features_rest_thermal")
SHARED_GROUPS = {"xyz": "means", "features_dc": "features_dc", "features_rest": "features_rest", "opacity": "opacities", "scaling": "scales",
                 "rotation": "quats", "features_dc_thermal": "features_dc_thermal", "features_rest_thermal": "features_rest_thermal"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ configuration and key sets
def test_config_validation():
    cfg = ThermalSplatfactoModelConfig()
    assert cfg.thermal_opacity_mode == "shared" and cfg.opacity_loss_mult == 0.0 and cfg.rgb_opacity_loss_mult == 0.01
    assert ThermalSplatfactoModelConfig(thermal_opacity_mode="separate").thermal_opacity_mode == "separate"
    for bad in ("both", "", "Separate", None):
        with pytest.raises(ValueError, match="thermal_opacity_mode"):
            ThermalSplatfactoModelConfig(thermal_opacity_mode=bad)
    for name in ("opacity_loss_mult", "rgb_opacity_loss_mult", "tv_pixel_loss_mult", "cross_channel_loss_mult"):
        with pytest.raises(ValueError, match=name):
            ThermalSplatfactoModelConfig(**{name: -1e-3})


def test_key_sets_of_both_modes():
    assert splat.param_names("shared") == SHARED_PARAMS and splat._PARAM_NAMES == SHARED_PARAMS
    assert splat.GROUP_PARAMS == SHARED_GROUPS
    assert splat.param_names("separate") == SHARED_PARAMS + ("opacities_thermal",)
    assert splat.GROUP_PARAMS_SEP == {**SHARED_GROUPS, "opacities_thermal": "opacities_thermal"}
    # the optimiser table: a group per entry of either mode, the thermal opacity at the opacity group's rate and schedule
    assert set(optim.SPLAT_OPTIMIZERS) == set(splat.GROUP_PARAMS_SEP)
    assert optim.SPLAT_OPTIMIZERS["opacities_thermal"] == optim.SPLAT_OPTIMIZERS["opacity"]
    assert ssf.PARAM_NAMES == splat.param_names("separate")


# ------------------------------------------------------------------------------------------------ the restatement
def _camera(W, H):
    return so.look_at_camera((2.3, 0.4, 0.6)), sf.fov_focal(W), W / 2 - 0.5, H / 2 + 0.25


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_equal_opacities_give_the_shared_render_exactly(mode):
    W, H = 40, 24
    c2w, fx, cx, cy = _camera(W, H)
    for dt in (torch.float32, torch.float64):
        p = {k: v.to(dt) for k, v in sf.scene(120, 3, 1).items()}
        ref = sf.render(p, c2w, fx, fx, cx, cy, W, H, sh_degree_to_use=1, rasterize_mode=mode, background=torch.tensor([0.2, 0.5, 0.7]),
                        background_thermal=0.3, with_depth=True)
        out = ssf.render({**p, "opacities_thermal": p["opacities"].clone()}, c2w, fx, fx, cx, cy, W, H, sh_degree_to_use=1, rasterize_mode=mode,
                         background=torch.tensor([0.2, 0.5, 0.7]), background_thermal=0.3, with_depth=True)
        assert float(ref["accumulation"].max()) > 0.5
        for k in ("rgb", "thermal", "accumulation", "raw", "depth"):
            assert torch.equal(out[k], ref[k]), (k, dt)
        assert torch.equal(out["accumulation_thermal"], ref["accumulation"])
        assert torch.equal(out["pair_used"], ref["pair_used"])


def test_the_two_chains_are_independent():
    """Opaque in RGB, clear in thermal: the thermal image is its background where only such Gaussians lie, and does not move with `opacities`."""
    W, H = 33, 17
    c2w, fx, cx, cy = _camera(W, H)
    p = {k: v.double() for k, v in sf.scene(60, 5, 0).items()}
    p["opacities"] = torch.full_like(p["opacities"], 4.0)
    p["opacities_thermal"] = torch.full_like(p["opacities"], -9.0)  # sigmoid < 1/255: no thermal contributor anywhere
    out = ssf.render(p, c2w, fx, fx, cx, cy, W, H, sh_degree_to_use=-1, background_thermal=0.3)
    assert float(out["accumulation"].max()) > 0.9 and float(out["accumulation_thermal"].abs().max()) == 0.0
    assert torch.equal(out["thermal"], torch.full_like(out["thermal"], float(torch.tensor(0.3))))  # (the background is a float32 value)
    p2 = {**p, "opacities": p["opacities"] - 3.0}
    out2 = ssf.render(p2, c2w, fx, fx, cx, cy, W, H, sh_degree_to_use=-1, background_thermal=0.3)
    assert torch.equal(out2["thermal"], out["thermal"]) and not torch.equal(out2["rgb"], out["rgb"])


def test_analytic_chain_gradients_agree_with_autograd():
    """The formulas the HIP backward evaluates per pixel and chain, back to front: T_i = T_{i+1} / (1 - a_i), d L / d a_i = T_i <c_i, v> -
    rest_i / (1 - a_i), rest_i = sum_{j > i} a_j T_j <c_j, v> + T_final (<bg, v> - v_acc) -- one pixel, float64, both chains."""
    g = torch.Generator().manual_seed(0)
    n = 12
    a1 = (0.05 + 0.9 * torch.rand(n, generator=g, dtype=torch.float64)).requires_grad_(True)
    a2 = (0.05 + 0.9 * torch.rand(n, generator=g, dtype=torch.float64)).requires_grad_(True)
    col = torch.rand(n, 4, generator=g, dtype=torch.float64)
    bg = torch.rand(4, generator=g, dtype=torch.float64)
    v = torch.randn(4, generator=g, dtype=torch.float64)
    v_acc, v_acc_t = torch.randn(2, generator=g, dtype=torch.float64)

    def chain(a, c, b):
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=a.dtype), 1 - a]), 0)
        return (a * T[:-1]) @ c + T[-1] * b, 1 - T[-1], T

    rgb, acc, T1 = chain(a1, col[:, :3], bg[:3])
    th, acc_t, T2 = chain(a2, col[:, 3:], bg[3:])
    (rgb @ v[:3] + th @ v[3:] + acc * v_acc + acc_t * v_acc_t).backward()

    def analytic(a, T, cv, rest):
        grads, Tc = torch.zeros_like(a), T[-1]
        for i in range(n - 1, -1, -1):
            om = 1 - a[i]
            Tc = Tc / om
            grads[i] = Tc * cv[i] - rest / om
            rest = rest + a[i] * Tc * cv[i]
        return grads

    with torch.no_grad():
        g1 = analytic(a1, T1, col[:, :3] @ v[:3], T1[-1] * (bg[:3] @ v[:3] - v_acc))
        g2 = analytic(a2, T2, col[:, 3:] @ v[3:], T2[-1] * (bg[3:] @ v[3:] - v_acc_t))
    for got, ref in ((g1, a1.grad), (g2, a2.grad)):
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("case", ssf.CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-sh{c[3]}-{'rev' if c[4] else 'fwd'}")
def test_gpu_test_scenes_are_awkward(case):
    """The GPU tests' scenes do what those tests rely on (checked here on the restatement): a tile with more than 256 list entries, one chain
    stopping where the other runs on, Gaussians below 1/255 in one spectrum that contribute in the other, and at most 1 % near-threshold pixels in
    float32 and in float64 (the cap of the GPU tests)."""
    W, H, mode, sh, reverse, seed = case
    c2w, fx, cx, cy = _camera(W, H)
    p = ssf.awkward_scene(300, seed, sh, reverse=reverse)
    kw = dict(sh_degree_to_use=sh if sh > 0 else -1, rasterize_mode=mode, background_thermal=0.3, with_depth=True)
    out = ssf.render({k: v.double() for k, v in p.items()}, c2w, fx, fx, cx, cy, W, H, **kw)
    assert int(out["contributors_per_tile"].max()) > 256, int(out["contributors_per_tile"].max())
    one, other = (out["stopped_thermal"], out["stopped"]) if reverse else (out["stopped"], out["stopped_thermal"])
    assert int((one & ~other).sum()) >= 10, int((one & ~other).sum())
    gone = torch.sigmoid(p["opacities" if reverse else "opacities_thermal"])[:, 0] < 1 / 255
    assert int(gone.sum()) >= 5 and bool(out["pair_used"][gone].any())
    out32 = ssf.render(p, c2w, fx, fx, cx, cy, W, H, **kw)
    assert float(out["flag_pixels"].float().mean()) <= 0.01 and float(out32["flag_pixels"].float().mean()) <= 0.01


# ------------------------------------------------------------------------------------------------ refinement rule and loss
def test_cull_rule_needs_both_opacities_low():
    cfg = ThermalSplatfactoModelConfig(thermal_opacity_mode="separate")
    lo, hi = -3.0, 1.0  # sigmoid 0.047 < 0.1 < 0.73
    p = {"opacities": torch.tensor([[lo], [lo], [hi], [hi]]), "opacities_thermal": torch.tensor([[lo], [hi], [lo], [hi]]),
         "scales": torch.full((4, 3), -5.0)}
    assert ssf.cull_mask(p, None, None, 600, cfg).tolist() == [True, False, False, False]
    # through a whole cull-only refinement: rows 1..3 survive with both logits and their moments
    cfg2 = ThermalSplatfactoModelConfig(thermal_opacity_mode="separate", stop_split_at=500)
    p.update(means=torch.zeros(4, 3), quats=torch.ones(4, 4))
    m = {k: (torch.arange(4.0)[:, None] + 1, torch.arange(4.0)[:, None] + 5) for k in ("opacities", "opacities_thermal")}
    q, mq, info = ssf.refine(p, m, None, (24, 40), 600, cfg2, 0, lambda n: torch.zeros(n, 3))
    assert info["culled"].tolist() == [True, False, False, False]
    assert q["opacities_thermal"][:, 0].tolist() == [hi, lo, hi] and mq["opacities_thermal"][0][:, 0].tolist() == [2.0, 3.0, 4.0]


def test_opacity_reset_clamps_both_logits_and_zeroes_both_moments():
    cfg = ThermalSplatfactoModelConfig(thermal_opacity_mode="separate", warmup_length=0)
    step = cfg.refine_every  # step % (reset_alpha_every * refine_every) == refine_every: a reset, no densification
    p = {"opacities": torch.tensor([[3.0], [-4.0]]), "opacities_thermal": torch.tensor([[-4.0], [3.0]]), "scales": torch.full((2, 3), -5.0),
         "means": torch.zeros(2, 3), "quats": torch.ones(2, 4)}
    m = {k: (torch.ones(2, 1), torch.ones(2, 1)) for k in ("opacities", "opacities_thermal", "means")}
    q, mq, info = ssf.refine(p, m, None, (24, 40), step, cfg, 0, lambda n: torch.zeros(n, 3))
    reset = torch.logit(torch.tensor(2.0 * cfg.cull_alpha_thresh)).item()
    assert info["reset"] and q["opacities"][:, 0].tolist() == [reset, -4.0] and q["opacities_thermal"][:, 0].tolist() == [-4.0, reset]
    for k in ("opacities", "opacities_thermal"):
        assert float(mq[k][0].abs().max()) == 0.0 and float(mq[k][1].abs().max()) == 0.0
    assert float(mq["means"][0].min()) == 1.0


def test_density_loss_value_and_detaches():
    g = torch.Generator().manual_seed(2)
    o = torch.randn(50, 1, generator=g, dtype=torch.float64)
    o_t = torch.randn(50, 1, generator=g, dtype=torch.float64)
    s, s_t = torch.sigmoid(o), torch.sigmoid(o_t)
    want = 0.3 * ((s_t - s).abs().mean() + 0.01 * (s - s_t).abs().mean())
    assert abs(float(ssf.density_loss(o, o_t, 0.3, 0.01)) - float(want)) <= 1e-15
    # the model's expression (get_loss_dict calls it on gauss_params when the mode is "separate" and opacity_loss_mult > 0)
    for mult, rgb_mult in ((0.3, 0.01), (0.3, 0.0), (2.0, 0.5)):
        a, b = o.clone().requires_grad_(True), o_t.clone().requires_grad_(True)
        loss = splat.opacity_density_loss(a, b, mult, rgb_mult)
        assert abs(float(loss) - float(ssf.density_loss(o, o_t, mult, rgb_mult))) <= 1e-15
        loss.backward()
        # each term's gradient reaches only its own tensor: d/d o_th sees the first term alone, d/d o the second alone
        sign = torch.sign(s_t - s)
        assert torch.allclose(b.grad, mult * sign * s_t * (1 - s_t) / 50, rtol=0, atol=1e-15)
        assert torch.allclose(a.grad, mult * rgb_mult * (-sign) * s * (1 - s) / 50, rtol=0, atol=1e-15)


# ------------------------------------------------------------------------------------------------ ABI
def test_sep_symbols_are_declared_exported_and_bound(lib):
    splat_abi.assert_unified(lib, SEP_SYMBOLS)
    assert lib.tn_version() == _lib.ABI_VERSION == 314


def test_sep_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    """The thermal group of every entry point.  (A null opacities_thermal of tn_splat_project / tn_splat_refine_plan and a null out_alpha_thermal of
    the eval raster are no refusals any more: a group of one pointer left out is the shared mode.)"""
    d = C.c_void_p(256)
    cam = _lib.TnSplatCamera()
    cam.fx = cam.fy = 30.0
    cam.width, cam.height = 40, 24
    bad_cam = _lib.TnSplatCamera()
    c, bc = C.byref(cam), C.byref(bad_cam)
    size = lib.tn_splat_backward_workspace_bytes
    assert size(-1, 0, 1, 0, 0) == -1 and size(0, -1, 1, 0, 0) == -1
    n, cap = 100, 1000
    assert size(n, cap, 1, 0, 0) >= 11 * 4 * cap > size(n, cap, 0, 0, 0) - 4 * n - 512 >= 10 * 4 * cap - 512
    # project: camera, Gaussian count, SH degree, the capacity
    proj = lambda cam=c, oth=d, n=10, deg=0, k=0, cap=100: lib.tn_splat_project(cam, None, d, d, d, d, d, d, d, d, oth, n, k, deg, 0, d, d, d, d, d, d, d, d, cap, None, None)  # noqa: E731
    assert proj(cam=None) == EINVAL and proj(cam=bc) == EINVAL
    assert proj(n=-1) == EINVAL and proj(deg=4) == EINVAL and proj(deg=3, k=3) == EINVAL
    assert proj(cap=-1) == EINVAL and b"tn_splat_project: bad workspace capacity" in lib.tn_last_error()
    assert proj(n=0, oth=None) == 0
    # raster / training raster
    assert lib.tn_splat_raster_chains(c, -1, d, 100, d, 0, d, d, d, d, None, None, None, None, None) == EINVAL
    assert lib.tn_splat_raster_chains(bc, 10, d, 100, d, 0, d, d, d, d, None, None, None, None, None) == EINVAL
    tr = lambda **kw: lib.tn_splat_raster_chains(c, kw.get("n", 10), d, kw.get("cap", 100), d, 0, d, d, d, kw.get("ath", d), d, d, kw.get("tth", d), kw.get("lth", d), None)  # noqa: E731
    assert tr(ath=None) == EINVAL and tr(tth=None) == EINVAL and tr(lth=None) == EINVAL and tr(n=-1) == EINVAL and tr(cap=-1) == EINVAL
    # raster backward
    need = size(10, 100, 1, 0, 0)
    bw = lambda **kw: lib.tn_splat_raster_backward(c, kw.get("n", 10), d, 100, kw.get("tot", 50), d, 0, d, d, kw.get("tth", d), kw.get("lth", d), d, d, d,  # noqa: E731
                                                   kw.get("vath", d), d, kw.get("bytes", need), d, None, d, d, d, kw.get("vlt", d), None, None, None, None)
    assert bw(tth=None) == EINVAL and bw(lth=None) == EINVAL and bw(vath=None) == EINVAL and bw(vlt=None) == EINVAL
    assert bw(tot=101) == EINVAL and bw(n=-1) == EINVAL
    assert bw(bytes=need - 1) == EINVAL and b"workspace" in lib.tn_last_error()
    assert bw(bytes=size(10, 100, 0, 0, 0)) == EINVAL  # the shared mode's size is too small
    assert bw(n=0, tth=None) == 0
    # projection backward
    pb = lambda **kw: lib.tn_splat_project_backward(c, None, None, d, d, d, d, d, d, d, d, kw.get("oth", d), kw.get("n", 10), 0, kw.get("deg", 0), 0, d, d, d, d, d,  # noqa: E731
                                                    kw.get("vlt", d), None, d, d, d, d, d, d, d, d, kw.get("goth", d), None, 0, None, None, None)
    assert pb(oth=None) == EINVAL and pb(vlt=None) == EINVAL and pb(goth=None) == EINVAL and pb(deg=5) == EINVAL and pb(n=-3) == EINVAL
    # refinement
    rs = _lib.TnSplatRefine()
    rs.cull_alpha_thresh, rs.cull_scale_thresh, rs.densify_grad_thresh, rs.densify_size_thresh = 0.1, 0.5, 0.0002, 0.01
    rs.cull_screen_size, rs.split_screen_size, rs.refine_every, rs.reset_alpha_every = 0.15, 0.05, 100, 30
    rs.stop_screen_size_at, rs.stop_split_at, rs.n_split_samples, rs.continue_cull_post_densification, rs.max_size = 4000, 15000, 2, 1, 40
    counts = (C.c_int64 * 4)()
    wneed = lib.tn_splat_refine_workspace_bytes(10, 2)
    plan = lambda **kw: lib.tn_splat_refine_plan(C.byref(rs), kw.get("step", 600), d, d, kw.get("oth", d), d, d, d, kw.get("n", 10), d,  # noqa: E731
                                                 kw.get("bytes", wneed), counts, None)
    assert plan(n=-1) == EINVAL and plan(step=-1) == EINVAL and plan(bytes=wneed - 1) == EINVAL
    assert plan(step=3100, oth=None, bytes=0) == 0 and list(counts) == [0, 10, 0, 0]  # a step that neither densifies nor culls: nothing launched
    arr9 = (C.c_void_p * 9)(*([256] * 9))
    null9 = (C.c_void_p * 9)()
    cnt = (C.c_int64 * 4)(0, 10, 0, 0)
    ap = lambda params=arr9, new=arr9, cnt=cnt, bytes=wneed: lib.tn_splat_refine_apply(C.byref(rs), 10, 0, d, bytes, cnt, None, 9, params, null9, null9, new, null9, null9, None)  # noqa: E731
    assert ap(bytes=wneed - 1) == EINVAL
    assert ap(cnt=(C.c_int64 * 4)(0, 11, 0, 0)) == EINVAL
    p8 = (C.c_void_p * 9)(*([256] * 8 + [None]))
    assert ap(params=p8) == EINVAL and b"null parameter 8" in lib.tn_last_error()
    assert ap(new=p8) == EINVAL
