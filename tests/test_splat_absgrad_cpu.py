"""The absgrad densification statistic without a GPU: the float64 walk of tests/splat_absgrad_functional.py against float64 autograd (its
signed sum on every configuration, its absolute sum on the two small scenes against autograd restricted to one pixel at a time), the
properties the GPU tests lean on (abs >= |signed|, a float32 walk within bc.MAX_FLOOR, a median norm ratio above 2 so that an absolute value
taken after the sum cannot pass), and the ABI of v_xys_abs (declared, bound, refusing bad arguments before any launch)."""
import ctypes as C
import os
import re

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib
from nerfstudio_thermal_amd.splat import ThermalSplatfactoModelConfig

import splat_abi
import splat_absgrad_functional as af
import splat_backward_cases as bc

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABS_SYMBOLS = ("tn_splat_backward_workspace_bytes", "tn_splat_raster_backward")  # v_xys_abs is a nullable group of one (the _abs names: splat_abi.RETIRED)


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
    hdr = splat_abi.header()
    splat_abi.assert_unified(lib, ABS_SYMBOLS)
    args = _declaration(hdr, "tn_splat_raster_backward")
    at = args.index("float* v_xys")
    assert args[at + 1] == "float* v_xys_abs"  # v_xys_abs directly after v_xys
    sig = _lib.SIGNATURES["tn_splat_raster_backward"][1]
    assert sig[at] is C.c_void_p and sig[at + 1] is C.c_void_p and len(sig) == len(args)  # _lib.SIGNATURES agrees with the header
    assert _declaration(hdr, ABS_SYMBOLS[0]) == ["int64_t num_gaussians", "int64_t max_intersections", "int32_t sep", "int32_t absgrad", "int32_t depth"]
    assert lib.tn_version() == _lib.ABI_VERSION == 314
    assert ThermalSplatfactoModelConfig().use_absgrad is False and ThermalSplatfactoModelConfig(use_absgrad=True).use_absgrad is True
    assert ThermalSplatfactoModelConfig().densify_grad_thresh == 0.0002  # the flag leaves the default alone


def test_abs_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    """(A null v_xys_abs is no refusal any more: it is the backward without absgrad.)"""
    size = lib.tn_splat_backward_workspace_bytes
    plain, plain_sep, with_abs, with_abs_sep = (lambda n, cap, s=s, a=a: size(n, cap, s, a, 0) for s, a in ((0, 0), (1, 0), (0, 1), (1, 1)))  # noqa: E731
    for f in (with_abs, with_abs_sep):
        assert f(-1, 10) == -1 and f(10, -1) == -1
    # the pair part (what grows with the capacity) is the plain sizes' scaled by 12/10 and 13/11; the per-Gaussian part is the same
    n, cap0, cap1 = 100, 1024, 3072  # multiples of 64: every pair part is whole 256-byte pieces
    pair = lambda f: f(n, cap1) - f(n, cap0)  # noqa: E731
    assert pair(with_abs) * 10 == pair(plain) * 12 == 12 * 10 * 4 * (cap1 - cap0)
    assert pair(with_abs_sep) * 11 == pair(plain_sep) * 13 == 13 * 11 * 4 * (cap1 - cap0)
    rest = lambda f, k: f(n, cap0) - 4 * k * cap0  # noqa: E731
    assert rest(with_abs, 12) == rest(plain, 10)
    assert rest(with_abs_sep, 13) == rest(plain_sep, 11)
    d = C.c_void_p(256)
    cam = _lib.TnSplatCamera()
    cam.fx = cam.fy = 30.0
    cam.width, cam.height = 40, 24
    c = C.byref(cam)
    need = with_abs(10, 100)
    bw = lambda **kw: lib.tn_splat_raster_backward(kw.get("cam", c), kw.get("n", 10), d, 100, kw.get("tot", 50), d, 0, d, d, None, None, d, d, d, None, d,  # noqa: E731
                                                   kw.get("bytes", need), kw.get("vx", d), kw.get("vabs", d), d, d, d, None, None, None, None, None)
    assert bw(vx=None) == EINVAL and b"tn_splat_raster_backward: null pointer" in lib.tn_last_error()
    assert bw(cam=None) == EINVAL and bw(tot=101) == EINVAL and bw(n=-1) == EINVAL
    assert bw(bytes=need - 1) == EINVAL and b"workspace" in lib.tn_last_error()
    assert bw(bytes=plain(10, 100)) == EINVAL  # the size without the two slots is too small
    assert bw(n=0, vabs=None) == 0
    need = with_abs_sep(10, 100)
    bws = lambda **kw: lib.tn_splat_raster_backward(c, kw.get("n", 10), d, 100, kw.get("tot", 50), d, 0, d, d, kw.get("tth", d), d, d, d, d, d, d,  # noqa: E731
                                                    kw.get("bytes", need), d, kw.get("vabs", d), d, d, d, kw.get("vlt", d), None, None, None, None)
    assert bws(tth=None) == EINVAL and bws(vlt=None) == EINVAL and bws(tot=101) == EINVAL and bws(n=-1) == EINVAL
    assert bws(bytes=need - 1) == EINVAL and b"workspace" in lib.tn_last_error()
    assert bws(bytes=plain_sep(10, 100)) == EINVAL
    assert bws(n=0, vabs=None) == 0
