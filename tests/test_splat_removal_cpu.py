"""The removal renders of the separate thermal opacity (removal_min_opacity_diff) without a GPU: the GPU tests' scenes have the properties those
tests rely on (checked on the restatement tests/splat_removal_functional.py in float64 and float32), the restatement's identities, the ABI of
tn_splat_raster_removal_sep (declared, exported, bound, refusing bad arguments before any launch) and the configuration."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib
from nerfstudio_thermal_amd.splat import ThermalSplatfactoModelConfig

import splat_functional as sf
import splat_oracle as so
import splat_removal_functional as srf
import splat_sep_functional as ssf

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = lambda c: f"{c[0]}x{c[1]}-{c[2]}-sh{c[3]}-{'rev' if c[4] else 'fwd'}"  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _camera(W, H):
    return so.look_at_camera((2.3, 0.4, 0.6)), sf.fov_focal(W), W / 2 - 0.5, H / 2 + 0.25


@functools.lru_cache(maxsize=None)
def _rendered(case, dt, thr=srf.THR):
    W, H, mode, sh, reverse, seed = case
    c2w, fx, cx, cy = _camera(W, H)
    p = {k: v.to(dt) for k, v in srf.removal_scene(300, seed, sh, reverse=reverse).items()}
    out = srf.render(p, c2w, fx, fx, cx, cy, W, H, thr, sh_degree_to_use=sh if sh > 0 else -1, rasterize_mode=mode, background_thermal=0.3)
    return p, out


def test_cases_cover_both_sizes_modes_and_colour_paths():
    assert len(srf.CASES) == 3
    assert {(c[0], c[1]) for c in srf.CASES} == {(40, 24), (33, 17)}
    assert {c[2] for c in srf.CASES} == {"classic", "antialiased"} and {c[3] for c in srf.CASES} == {0, 3}


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", srf.CASES, ids=IDS)
def test_gpu_test_scenes_have_what_the_gpu_tests_rely_on(case, dt):
    p, out = _rendered(case, dt)
    ok = out["projection"]["ok"]
    kr, kt = out["keep_rgb"][ok], out["keep_th"][ok]
    shares = {(a, b): float(((kr == a) & (kt == b)).float().mean()) for a in (True, False) for b in (True, False)}
    print(f"on screen {int(ok.sum())}; (keep_rgb, keep_th) shares {shares}")
    assert min(shares.values()) >= 0.10, shares  # kept in both, out of RGB only, out of thermal only, out of both
    band = float(srf.threshold_distance(p, srf.THR).min())
    assert band > srf.BAND, band
    share = float(out["flag_pixels"].float().mean())
    assert share <= 0.01, share
    assert int(out["contributors_per_tile"].max()) > 256
    assert int(out["stopped_removal"].sum()) > 0 and int(out["stopped_removal_thermal"].sum()) > 0
    assert float((out["removal"] - out["rgb"]).abs().max()) > 0.05
    assert float((out["removal_thermal"] - out["thermal"]).abs().max()) > 0.05


@pytest.mark.parametrize("case", srf.CASES, ids=IDS)
def test_keep_decisions_agree_between_float32_and_float64(case):
    p64, out64 = _rendered(case, torch.float64)
    _, out32 = _rendered(case, torch.float32)
    assert torch.equal(out64["keep_rgb"], out32["keep_rgb"]) and torch.equal(out64["keep_th"], out32["keep_th"])
    # the kernel's form of the decision: float32, from exp2(log2(opacity))
    o, ot = (torch.exp2(torch.log2(torch.sigmoid(p64[k].float())))[:, 0] for k in ("opacities", "opacities_thermal"))
    d = (o - ot).abs()
    thr = torch.tensor(srf.THR)
    assert torch.equal(d < thr * o, out64["keep_rgb"]) and torch.equal(d < thr * ot, out64["keep_th"])


@pytest.mark.parametrize("case", srf.CASES, ids=IDS)
def test_restatement_identities(case):
    W, H, mode, sh, reverse, seed = case
    p, out = _rendered(case, torch.float64)
    _, huge = _rendered(case, torch.float64, 1e30)
    assert bool(huge["keep_rgb"].all()) and bool(huge["keep_th"].all())
    assert torch.equal(huge["removal"], huge["rgb"]) and torch.equal(huge["removal_thermal"], huge["thermal"])
    _, none = _rendered(case, torch.float64, 0.0)
    assert not bool(none["keep_rgb"].any()) and not bool(none["keep_th"].any())
    assert torch.equal(none["removal"], torch.zeros_like(none["removal"]))  # the tests' RGB background is black, the thermal one 0.3 (a float32 value)
    assert torch.equal(none["removal_thermal"], torch.full_like(none["removal_thermal"], float(torch.tensor(0.3))))
    # removal = the separate-mode render of the kept subset, spectrum by spectrum
    c2w, fx, cx, cy = _camera(W, H)
    kw = dict(sh_degree_to_use=sh if sh > 0 else -1, rasterize_mode=mode, background_thermal=0.3)
    sub = ssf.render(srf.subset(p, out["keep_rgb"]), c2w, fx, fx, cx, cy, W, H, **kw)
    assert torch.equal(sub["rgb"], out["removal"])
    sub_t = ssf.render(srf.subset(p, out["keep_th"]), c2w, fx, fx, cx, cy, W, H, **kw)
    assert torch.equal(sub_t["thermal"], out["removal_thermal"])


def test_keep_masks_rule():
    logit = lambda v: torch.logit(torch.tensor(v, dtype=torch.float64))  # noqa: E731
    o = torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5])
    ot = torch.tensor([0.5, 0.5 * srf.RATIO, 0.5 / srf.RATIO, 0.75, 0.1])
    p = {"opacities": logit(o.tolist())[:, None], "opacities_thermal": logit(ot.tolist())[:, None]}
    kr, kt = srf.keep_masks(p, srf.THR)
    assert kr.tolist() == [True, False, True, False, False] and kt.tolist() == [True, True, False, False, False]
    kr, kt = srf.keep_masks(p, 0.0)  # strict: equal opacities are not kept at thr = 0
    assert not bool(kr.any()) and not bool(kt.any())
    gone = {"opacities": torch.full((1, 1), -800.0, dtype=torch.float64), "opacities_thermal": torch.full((1, 1), -800.0, dtype=torch.float64)}
    assert srf.keep_masks(gone, 1e30)[0].tolist() == [False]  # o = 0: nothing to keep, and no division


# ------------------------------------------------------------------------------------------------ ABI
def test_symbol_is_declared_exported_and_bound(lib):
    name = "tn_splat_raster_removal_sep"
    hdr = open(os.path.join(ROOT, "include", "thermal_nerf_hip.h")).read()
    m = re.search(r"TN_API int " + name + r"\s*\(([^;]*)\);", hdr)
    assert m, "not declared"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    ctype = lambda a: C.c_int64 if a.startswith("int64_t ") else C.c_float if a.startswith("float ") else C.c_void_p  # noqa: E731
    assert [a.split()[-1].lstrip("*") for a in args] == ["camera", "num_gaussians", "workspace", "max_intersections", "background4", "min_opacity_diff",
                                                        "out_removal", "stream"]
    assert _lib.SIGNATURES[name] == (C.c_int, [ctype(a) for a in args])
    assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    nm = shutil.which("nm")
    if nm:
        exported = set(re.findall(r" T (tn_\w+)", subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout))
        assert name in exported
    assert lib.tn_version() == _lib.ABI_VERSION == 314


def test_entry_point_refuses_bad_arguments_without_a_gpu(lib):
    d = C.c_void_p(256)
    bg = (C.c_float * 4)(0.0, 0.0, 0.0, 0.3)
    cam = _lib.TnSplatCamera()
    cam.fx = cam.fy = 30.0
    cam.width, cam.height = 40, 24
    c, bc = C.byref(cam), C.byref(_lib.TnSplatCamera())

    def call(camera=c, n=10, ws=d, cap=100, background=bg, thr=0.05, out=d):
        return lib.tn_splat_raster_removal_sep(camera, n, ws, cap, background, thr, out, None)

    assert call(camera=None) == EINVAL and call(camera=bc) == EINVAL
    assert call(ws=None) == EINVAL and b"tn_splat_raster_removal_sep: null pointer" in lib.tn_last_error()
    assert call(background=None) == EINVAL and call(out=None) == EINVAL
    assert call(n=-1) == EINVAL and call(cap=-1) == EINVAL
    assert call(thr=-1e-3) == EINVAL and b"min_opacity_diff" in lib.tn_last_error()
    assert call(thr=float("nan")) == EINVAL and call(thr=-float("inf")) == EINVAL


# ------------------------------------------------------------------------------------------------ configuration
def test_config_validation():
    assert ThermalSplatfactoModelConfig().removal_min_opacity_diff is None
    assert ThermalSplatfactoModelConfig(thermal_opacity_mode="separate").removal_min_opacity_diff is None
    assert ThermalSplatfactoModelConfig(thermal_opacity_mode="separate", removal_min_opacity_diff=0.05).removal_min_opacity_diff == 0.05
    assert ThermalSplatfactoModelConfig(thermal_opacity_mode="separate", removal_min_opacity_diff=0.0).removal_min_opacity_diff == 0.0
    for bad in (-0.05, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="removal_min_opacity_diff"):
            ThermalSplatfactoModelConfig(thermal_opacity_mode="separate", removal_min_opacity_diff=bad)
    for v in (0.05, 0.0):
        with pytest.raises(ValueError, match="separate"):
            ThermalSplatfactoModelConfig(removal_min_opacity_diff=v)
        with pytest.raises(ValueError, match="separate"):
            ThermalSplatfactoModelConfig(thermal_opacity_mode="shared", removal_min_opacity_diff=v)
