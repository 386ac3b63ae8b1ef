"""The absgrad densification statistic without a GPU: the float64 walk of tests/splat_absgrad_functional.py against float64 autograd (its
signed sum on every configuration, its absolute sum on the two small scenes against autograd restricted to one pixel at a time), the
properties the GPU tests lean on (abs >= |signed|, a float32 walk within bc.MAX_FLOOR, a median norm ratio above 2 so that an absolute value
taken after the sum cannot pass), and the ABI of the _abs entry points (declared, bound, refusing bad arguments before any launch)."""
import ctypes as C
import os
import re

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib
from nerfstudio_thermal_amd.splat import ThermalSplatfactoModelConfig

import splat_absgrad_functional as af
import splat_backward_cases as bc

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABS_SYMBOLS = ("tn_splat_backward_workspace_bytes_abs", "tn_splat_backward_workspace_bytes_abs_sep", "tn_splat_raster_backward_abs",
               "tn_splat_raster_backward_abs_sep")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("cfg", af.CONFIGS, ids=af.IDS)
def test_walk_properties(cfg):
    """Signed sum = float64 autograd's d xys (1e-9), abs >= |signed| componentwise, the float32 walk within bc.MAX_FLOOR of the float64 one,
    and the median ratio of norms above 2."""
    ref = af.reference(*cfg)
    keep = ~bc.cpu_excluded(ref["bc"]["st"])
    err = bc.rel_err(ref["signed64"], ref["bc"]["g64"]["xys"], keep)
    slack = float((ref["abs64"] - ref["signed64"].abs())[keep].min())
    err32 = bc.rel_err(ref["abs32"], ref["abs64"], keep)
    ratio = af.norm_ratio(ref["abs64"], ref["signed64"], keep)
    print(f"{bc.config_id(cfg)}: signed sum against autograd {err:.2e}; min(abs - |signed|) {slack:.2e}; float32 walk's error on abs {err32:.2e}; "
          f"median |abs| / |signed| {ratio:.2f}; largest abs entry {bc.amax(ref['abs64'][keep]):.3e}")
    assert err <= 1e-9, err
    assert slack >= 0.0, slack
    assert err32 <= bc.MAX_FLOOR, err32
    assert ratio > 2.0, ratio
    assert bc.amax(ref["abs64"][ref["bc"]["st"]["projection"]["radii"] == 0]) == 0.0  # no pair: exactly (0, 0)


@pytest.mark.parametrize("cfg", af.SMALL_CONFIGS, ids=[bc.config_id(c) for c in af.SMALL_CONFIGS])
def test_walk_abs_equals_per_pixel_autograd(cfg):
    ref = af.reference(*cfg)
    keep = ~bc.cpu_excluded(ref["bc"]["st"])
    want = af.per_pixel_autograd_abs(*cfg)
    err = bc.rel_err(ref["abs64"], want, keep)
    print(f"{bc.config_id(cfg)}: the walk's abs against one autograd pass per pixel {err:.2e}")
    assert bc.amax(want) > 0 and err <= 1e-9, err


def test_single_separates_the_two_statistics():
    """What the GPU decision test leans on: on `single` the absolute statistic's norm is at least 4 x the signed one's."""
    ref = af.reference("single", "classic", 3, None)
    n_s, n_a = float(ref["signed64"][0].norm()), float(ref["abs64"][0].norm())
    print(f"single: |signed| {n_s:.4e}, |abs| {n_a:.4e}, ratio {n_a / n_s:.2f}")
    assert n_s > 0 and n_a >= 4.0 * n_s


# ------------------------------------------------------------------------------------------------ ABI
def _declaration(hdr, name):
    m = re.search(r"TN_API\s+\w+\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_abs_entry_points_are_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "thermal_nerf_hip.h")).read()
    for name in ABS_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    for name, plain in (("tn_splat_raster_backward_abs", "tn_splat_raster_backward"), ("tn_splat_raster_backward_abs_sep", "tn_splat_raster_backward_sep")):
        args, base = _declaration(hdr, name), _declaration(hdr, plain)
        at = base.index("float* v_xys")
        assert args == base[:at + 1] + ["float* v_xys_abs"] + base[at + 1:], name  # the plain entry point's arguments, v_xys_abs directly after v_xys
        # _lib.SIGNATURES agrees with the header: one more pointer, at that place
        sig, sig_base = _lib.SIGNATURES[name][1], _lib.SIGNATURES[plain][1]
        assert sig == sig_base[:at + 1] + [C.c_void_p] + sig_base[at + 1:] and len(sig) == len(args), name
    for name in ABS_SYMBOLS[:2]:
        assert _declaration(hdr, name) == ["int64_t num_gaussians", "int64_t max_intersections"], name
    assert lib.tn_version() == _lib.ABI_VERSION == 313
    assert ThermalSplatfactoModelConfig().use_absgrad is False and ThermalSplatfactoModelConfig(use_absgrad=True).use_absgrad is True
    assert ThermalSplatfactoModelConfig().densify_grad_thresh == 0.0002  # the flag leaves the default alone


def test_abs_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    for f in (lib.tn_splat_backward_workspace_bytes_abs, lib.tn_splat_backward_workspace_bytes_abs_sep):
        assert f(-1, 10) == -1 and f(10, -1) == -1
    # the pair part (what grows with the capacity) is the plain functions' scaled by 12/10 and 13/11; the per-Gaussian part is the same
    n, cap0, cap1 = 100, 1024, 3072  # multiples of 64: every pair part is whole 256-byte pieces
    pair = lambda f: f(n, cap1) - f(n, cap0)  # noqa: E731
    assert pair(lib.tn_splat_backward_workspace_bytes_abs) * 10 == pair(lib.tn_splat_backward_workspace_bytes) * 12 == 12 * 10 * 4 * (cap1 - cap0)
    assert pair(lib.tn_splat_backward_workspace_bytes_abs_sep) * 11 == pair(lib.tn_splat_backward_workspace_bytes_sep) * 13 == 13 * 11 * 4 * (cap1 - cap0)
    rest = lambda f, k: f(n, cap0) - 4 * k * cap0  # noqa: E731
    assert rest(lib.tn_splat_backward_workspace_bytes_abs, 12) == rest(lib.tn_splat_backward_workspace_bytes, 10)
    assert rest(lib.tn_splat_backward_workspace_bytes_abs_sep, 13) == rest(lib.tn_splat_backward_workspace_bytes_sep, 11)
    d = C.c_void_p(256)
    cam = _lib.TnSplatCamera()
    cam.fx = cam.fy = 30.0
    cam.width, cam.height = 40, 24
    c = C.byref(cam)
    need = lib.tn_splat_backward_workspace_bytes_abs(10, 100)
    bw = lambda **kw: lib.tn_splat_raster_backward_abs(kw.get("cam", c), kw.get("n", 10), d, 100, kw.get("tot", 50), d, d, d, d, d, d, d,  # noqa: E731
                                                       kw.get("bytes", need), kw.get("vx", d), kw.get("vabs", d), d, d, d, None)
    assert bw(vabs=None) == EINVAL and b"tn_splat_raster_backward_abs: null pointer" in lib.tn_last_error()
    assert bw(vx=None) == EINVAL and bw(cam=None) == EINVAL and bw(tot=101) == EINVAL and bw(n=-1) == EINVAL
    assert bw(bytes=need - 1) == EINVAL and b"workspace" in lib.tn_last_error()
    assert bw(bytes=lib.tn_splat_backward_workspace_bytes(10, 100)) == EINVAL  # the size without the two slots is too small
    assert bw(n=0, vabs=None) == 0
    need = lib.tn_splat_backward_workspace_bytes_abs_sep(10, 100)
    bws = lambda **kw: lib.tn_splat_raster_backward_abs_sep(c, kw.get("n", 10), d, 100, kw.get("tot", 50), d, d, d, kw.get("tth", d), d, d, d, d, d, d,  # noqa: E731
                                                            kw.get("bytes", need), d, kw.get("vabs", d), d, d, d, kw.get("vlt", d), None)
    assert bws(vabs=None) == EINVAL and b"tn_splat_raster_backward_abs_sep: null pointer" in lib.tn_last_error()
    assert bws(tth=None) == EINVAL and bws(vlt=None) == EINVAL and bws(tot=101) == EINVAL and bws(n=-1) == EINVAL
    assert bws(bytes=need - 1) == EINVAL and b"workspace" in lib.tn_last_error()
    assert bws(bytes=lib.tn_splat_backward_workspace_bytes_sep(10, 100)) == EINVAL
    assert bws(n=0, vabs=None) == 0
