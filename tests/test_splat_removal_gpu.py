"""The removal renders of the separate thermal opacity on the GPU (removal_min_opacity_diff: tn_splat_raster_removal_sep through
ThermalSplatfactoModel.get_outputs) against the float64 restatement tests/splat_removal_functional.py.

Scenes (srf.removal_scene, ~300 Gaussians, frames of 40 x 24 and 33 x 17: partial tiles and quadrants): ssf.awkward_scene with the thermal
opacities rewritten so that each of the four (kept in `removal`, kept in `removal_thermal`) combinations holds a tenth of the Gaussians or more and
none is within 1e-4 of a threshold; a tile list longer than one 256-record batch; both removal walks hit their 1e-4 stop.
tests/test_splat_removal_cpu.py checks those properties on the restatement.

Tolerance rule (tests/test_splat_separate_gpu.py's): the kernel's error against float64 is at most TOL_FACTOR = 8 times the float32 restatement's
own error against float64 on the same pixels, and never less than one float32 epsilon of the output's scale.  Pixels the float64 walks flag (a
decision within 1e-4 of the 1/255 gate, the 0.999 clamp, the 1e-4 stop or an output clamp) are left out; at most 1 % of them."""
import ctypes as C
import functools

import pytest
import torch

import splat_functional as sf
import splat_oracle as so
import splat_removal_functional as srf
import splat_sep_functional as ssf

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
EPS = 2.0 ** -23
CASES = srf.CASES
IDS = lambda c: f"{c[0]}x{c[1]}-{c[2]}-sh{c[3]}-{'rev' if c[4] else 'fwd'}"  # noqa: E731
BASE_KEYS = {"rgb", "thermal", "depth", "accumulation", "accumulation_thermal", "background", "background_thermal"}
REMOVAL_KEYS = {"removal", "removal_thermal"}


def _model(params, sh_degree, mode="classic", thr=srf.THR, **kw):
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

    cfg = ThermalSplatfactoModelConfig(sh_degree=sh_degree, sh_degree_interval=1, rasterize_mode=mode, background_thermal=0.3, thermal_opacity_mode="separate",
                                       removal_min_opacity_diff=thr, **kw)
    m = ThermalSplatfactoModel(cfg, num_points=4, device=DEV)
    m.load_gaussians(params)
    m.step = 10**6
    return m


def _view(W, H):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    c2w, fx, cx, cy = so.look_at_camera((2.3, 0.4, 0.6)), sf.fov_focal(W), W / 2 - 0.5, H / 2 + 0.25
    return (c2w, fx, fx, cx, cy, W, H), PinholeCamera(c2w, fx, fx, cx, cy, W, H)


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


@functools.lru_cache(maxsize=None)
def reference(case):
    """Float64 and float32 restatement of one case at THR, computed once."""
    W, H, mode, sh, rev, seed = case
    p = srf.removal_scene(300, seed, sh, reverse=rev)
    view, _ = _view(W, H)
    res = {}
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            res[dt] = srf.render({k: v.to(dt) for k, v in p.items()}, *view, srf.THR, sh_degree_to_use=sh if sh > 0 else -1, rasterize_mode=mode,
                                 background_thermal=0.3)
    return p, res[torch.float64], res[torch.float32]


def _within_bound(name, got, ref64, ref32, ok):
    ref, f32 = ref64.double()[ok], ref32.double()[ok]
    floor = max(_amax(f32 - ref), EPS * _amax(ref))
    err = _amax(got.detach().cpu().double()[ok] - ref)
    print(f"{name}: err {err:.2e}, float32 restatement {floor:.2e} ({err / floor:.1f}x)")
    assert err <= TOL_FACTOR * floor, (name, err, floor)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_removal_renders_match_the_float64_restatement(case):
    W, H, mode, sh, rev, seed = case
    p, out64, out32 = reference(case)
    _, cam = _view(W, H)
    m = _model(p, sh, mode)
    ev = m.get_outputs(cam)
    flag = out64["flag_pixels"]
    share = float(flag.float().mean())
    print(f"near-threshold pixels left out: {int(flag.sum())} of {flag.numel()} ({100 * share:.2f} %); tile lists up to {int(out64['contributors_per_tile'].max())}")
    assert share <= 0.01
    assert m.last_num_intersections > 256
    assert ev["removal"].shape == (H, W, 3) and ev["removal_thermal"].shape == (H, W, 1)
    ok = ~flag
    for k in ("removal", "removal_thermal", "rgb", "thermal"):
        _within_bound(k, ev[k], out64[k], out32[k], ok)
    assert _amax(ev["removal"] - ev["rgb"]) > 0.05 and _amax(ev["removal_thermal"] - ev["thermal"]) > 0.05


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_removal_is_the_render_of_the_kept_subset(case):
    """`removal` against the rgb of a model that holds only the keep_rgb Gaussians, `removal_thermal` against the thermal of the keep_th ones: two
    float32 computations of one float64 image, each within the bound of it -- so their difference is within twice the bound."""
    W, H, mode, sh, rev, seed = case
    p, out64, out32 = reference(case)
    _, cam = _view(W, H)
    ev = _model(p, sh, mode).get_outputs(cam)
    ok = ~out64["flag_pixels"]
    for key, keep, sub_key in (("removal", out64["keep_rgb"], "rgb"), ("removal_thermal", out64["keep_th"], "thermal")):
        sub = _model(srf.subset(p, keep), sh, mode, thr=None).get_outputs(cam)[sub_key]
        print(f"{key} vs the {sub_key} of the {int(keep.sum())} kept Gaussians: bit-equal {torch.equal(sub, ev[key])}, max diff {_amax(sub - ev[key]):.2e}")
        _within_bound(f"{sub_key} of the subset", sub, out64[key], out32[key], ok)
        floor = max(_amax((out32[key].double() - out64[key])[ok]), EPS * _amax(out64[key][ok]))
        assert _amax((sub - ev[key]).cpu().double()[ok]) <= TOL_FACTOR * floor, (key, floor)


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_thresholds_that_keep_everything_and_nothing(mode):
    W, H, _, sh, rev, seed = CASES[0]
    p = srf.removal_scene(300, seed, sh, reverse=rev)
    _, cam = _view(W, H)
    everything = _model(p, sh, mode, thr=1e30).get_outputs(cam)
    assert torch.equal(everything["removal"], everything["rgb"]) and torch.equal(everything["removal_thermal"], everything["thermal"])
    assert _amax(everything["rgb"]) > 0.5
    nothing = _model(p, sh, mode, thr=0.0, background_color="white").get_outputs(cam)
    assert torch.equal(nothing["removal"], nothing["background"].expand(H, W, 3))
    assert torch.equal(nothing["removal_thermal"], nothing["background_thermal"].expand(H, W, 1))
    assert not torch.equal(nothing["rgb"], nothing["removal"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_other_outputs_are_untouched_and_the_key_sets(case):
    W, H, mode, sh, rev, seed = case
    p, _, _ = reference(case)
    _, cam = _view(W, H)
    on, off = _model(p, sh, mode), _model(p, sh, mode, thr=None)
    a, b = on.get_outputs(cam), off.get_outputs(cam)
    assert set(b) == BASE_KEYS and set(a) == BASE_KEYS | REMOVAL_KEYS
    for k in ("rgb", "thermal", "depth", "accumulation", "accumulation_thermal"):
        assert torch.equal(a[k], b[k]), k
    on.train()
    tr = on.get_train_outputs(cam)
    assert set(tr) == BASE_KEYS
    # two calls are bit-identical
    again = on.get_outputs(cam)
    for k in REMOVAL_KEYS:
        assert torch.equal(a[k], again[k]) and bool(torch.isfinite(a[k]).all()), k
    # get_image_metrics_and_images shows them beside the other images
    batch = {"image": torch.rand(H, W, 3, device=DEV), "is_thermal": False}
    on.eval()
    _, images = on.get_image_metrics_and_images(a, batch)
    assert torch.equal(images["removal"], a["removal"]) and torch.equal(images["removal_thermal"], a["removal_thermal"])
    assert "removal" not in off.get_image_metrics_and_images(b, batch)[1]


def test_images_are_resized_to_a_smaller_ground_truth():
    """Scored in training mode while the resolution schedule's factor is 2: the removal renders -- channel views of one [H,W,4] buffer -- come back
    at the ground truth's size, as rgb and thermal do, by the same resize."""
    from nerfstudio_thermal_amd.splat import resize_image

    W, H, mode, sh, rev, seed = CASES[0]
    p, _, _ = reference(CASES[0])
    _, cam = _view(W, H)
    m = _model(p, sh, mode, num_downscales=1)
    out = m.get_outputs(cam)
    m.train()
    m.step = 0
    assert m._get_downscale_factor() == 2
    _, images = m.get_image_metrics_and_images(out, {"image": torch.rand(H, W, 3, device=DEV), "is_thermal": False})
    for k, c in (("removal", 3), ("removal_thermal", 1)):
        assert images[k].shape == (H // 2, W // 2, c) and not out[k].is_contiguous()
        assert torch.equal(images[k], resize_image(out[k].contiguous(), (H // 2, W // 2))), k
    assert images["img"].shape == (H // 2, 3 * (W // 2), 3)


def test_background_shortcuts_and_empty_models():
    W, H, mode, sh, rev, seed = CASES[0]
    p = srf.removal_scene(300, seed, sh, reverse=rev)
    _, cam = _view(W, H)
    bg, bg_t = torch.tensor([1.0, 1.0, 1.0], device=DEV).expand(H, W, 3), torch.full((H, W, 1), 0.3, device=DEV)
    empty = _model({k: v[:0] for k, v in p.items()}, sh, mode, background_color="white")
    behind = _model({**p, "means": p["means"] + torch.tensor([100.0, 0.0, 0.0])}, sh, mode, background_color="white")  # everything behind the camera
    for m in (empty, behind):
        out = m.get_outputs(cam)
        assert set(out) == BASE_KEYS | REMOVAL_KEYS
        assert torch.equal(out["removal"], bg) and torch.equal(out["removal_thermal"], bg_t)
    assert behind.last_num_intersections == 0
    # the entry point itself with no Gaussians: tn_splat_bin leaves every list empty, every pixel receives the background
    from nerfstudio_thermal_amd import _lib
    from nerfstudio_thermal_amd.splat import camera_struct

    lib = _lib.load()
    cs = camera_struct(cam)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    ws = torch.empty(int(lib.tn_splat_workspace_bytes(0, 64, tiles)), dtype=torch.uint8, device=DEV)
    total = C.c_int64(-1)
    assert lib.tn_splat_bin(C.byref(cs), None, 0, C.c_void_p(ws.data_ptr()), 64, C.byref(total), None) == 0 and total.value == 0
    out = torch.full((H, W, 4), -1.0, device=DEV)
    assert lib.tn_splat_raster_removal_sep(C.byref(cs), 0, C.c_void_p(ws.data_ptr()), 64, (C.c_float * 4)(0.25, 0.5, 2.0, 0.3), 0.05, C.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, torch.tensor([0.25, 0.5, 1.0, 0.3], device=DEV).expand(H, W, 4))  # (clamped to 1)


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from nerfstudio_thermal_amd import _lib
    from nerfstudio_thermal_amd.splat import camera_struct

    lib = _lib.load()
    _, cam = _view(40, 24)
    c = C.byref(camera_struct(cam))
    buf = torch.zeros(1 << 16, device=DEV)
    d = C.c_void_p(buf.data_ptr())
    bg = (C.c_float * 4)(0.0, 0.0, 0.0, 0.3)
    torch.cuda.synchronize()
    assert lib.tn_splat_raster_removal_sep(c, 10, d, 100, bg, 0.05, None, None) == -22
    assert lib.tn_splat_raster_removal_sep(c, 10, d, 100, bg, -0.05, d, None) == -22
    assert lib.tn_splat_raster_removal_sep(c, 10, d, 100, bg, float("nan"), d, None) == -22
    assert lib.tn_splat_raster_removal_sep(c, 10, d, -1, bg, 0.05, d, None) == -22
    assert lib.tn_splat_raster_removal_sep(c, -1, d, 100, bg, 0.05, d, None) == -22
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0  # nothing ran


def test_full_size_frame_is_finite():
    """1080p, 1 M Gaussians, thr = 0.05: index arithmetic and list lengths of the real size."""
    from nerfstudio_thermal_amd import synth
    from nerfstudio_thermal_amd.splat import PinholeCamera

    n = 1_000_000
    p = synth.synth_gaussians(n, seed=11, extent=1.5, scale_range=(-5.5, -3.5))
    g = torch.Generator().manual_seed(1)
    p["opacities_thermal"] = p["opacities"] + 0.2 * torch.randn(n, 1, generator=g)  # some within 5 % of each other, some not
    cam = PinholeCamera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 1400.0, 960.0, 540.0, 1920, 1080)
    out = _model(p, 3).get_outputs(cam)
    for k, c in (("removal", 3), ("removal_thermal", 1)):
        assert out[k].shape == (1080, 1920, c) and bool(torch.isfinite(out[k]).all()), k
        assert float(out[k].min()) >= 0.0 and float(out[k].max()) <= 1.0
    assert _amax(out["removal"] - out["rgb"]) > 0.05 and _amax(out["removal"]) > 0.05
