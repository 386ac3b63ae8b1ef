"""The MCMC densification strategy without a GPU: configuration, the C ABI's new names, the host-side refusals of tn_splat_mcmc_relocate /
tn_splat_mcmc_noise, and the float64 restatement's own properties (splat_mcmc_functional.py)."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib, splat
from nerfstudio_thermal_amd.splat import ThermalSplatfactoModelConfig

import splat_abi
import splat_mcmc_functional as mf

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tn_splat_mcmc_workspace_bytes", "tn_splat_mcmc_relocate", "tn_splat_mcmc_noise")  # (the _sep names they absorbed: splat_abi.RETIRED)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_config_defaults():
    cfg = dataclasses.asdict(ThermalSplatfactoModelConfig())
    want = {"strategy": "default", "max_gs_num": 1_000_000, "noise_lr": 5e5, "mcmc_opacity_reg": 0.01, "mcmc_scale_reg": 0.01,
            "mcmc_min_opacity": 0.005, "mcmc_grow_factor": 1.05}
    assert {k: cfg[k] for k in want} == want
    assert ThermalSplatfactoModelConfig(strategy="mcmc").strategy == "mcmc"
    assert splat.STRATEGIES == ("default", "mcmc") and splat.MCMC_N_MAX == mf.N_MAX == 51


@pytest.mark.parametrize("kw", [{"strategy": "MCMC"}, {"strategy": "absgrad"}, {"strategy": None}, {"max_gs_num": 0}, {"max_gs_num": -5},
                                {"noise_lr": -1.0}, {"noise_lr": float("nan")}, {"mcmc_opacity_reg": -0.01}, {"mcmc_scale_reg": -0.01},
                                {"mcmc_min_opacity": 0.0}, {"mcmc_min_opacity": 1.0}, {"mcmc_min_opacity": -0.1}, {"mcmc_grow_factor": 0.99},
                                {"mcmc_grow_factor": float("nan")}])
def test_config_refuses(kw):
    with pytest.raises(ValueError):
        ThermalSplatfactoModelConfig(**kw)


@pytest.mark.parametrize("kw", [{"max_gs_num": 1}, {"noise_lr": 0.0}, {"mcmc_opacity_reg": 0.0}, {"mcmc_scale_reg": 0.0}, {"mcmc_min_opacity": 1e-6},
                                {"mcmc_min_opacity": 0.999}, {"mcmc_grow_factor": 1.0}])
def test_config_accepts_the_edges(kw):
    cfg = ThermalSplatfactoModelConfig(strategy="mcmc", **kw)
    assert all(getattr(cfg, k) == v for k, v in kw.items())


def test_header_binding_and_exports_agree_on_the_new_names(lib):
    hdr = open(os.path.join(ROOT, "include", "thermal_nerf_hip.h")).read()
    declared = set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    splat_abi.assert_unified(lib, NEW)
    assert {n for n in declared if "mcmc" in n} == set(NEW) == {n for n in _lib.SIGNATURES if "mcmc" in n}
    assert _lib.ABI_VERSION == 314 and lib.tn_version() == 314
    src = open(os.path.join(ROOT, "nerfstudio-thermal_amd", "csrc", "build.sh")).read()
    assert "tn_splat_mcmc" in src  # the new translation unit is in the build


def test_workspace_size(lib):
    ws = lib.tn_splat_mcmc_workspace_bytes
    assert ws(-1, 1) == -1 and ws(1, -1) == -1 and ws(1 << 31, 1) == -1 and ws(1, 1 << 31) == -1
    assert ws(0, 0) > 0
    small, big = ws(1000, 10), ws(2000, 10)
    assert 0 < small < big and big - small >= 1000 * (4 + 5 * 4) - 512  # a counter and five values per row (256-byte aligned)
    assert ws(1000, 5000) - ws(1000, 1000) >= 4000 * 4 - 256  # a flag per draw


@pytest.mark.parametrize("sep", [False, True])
def test_relocate_refusals_before_any_launch(lib, sep):
    n = 9 if sep else 8
    d = C.c_void_p(256)  # never dereferenced: every call below is refused (or returns) before anything is read or launched
    ptrs = (C.c_void_p * n)(*([256] * n))
    nulls = (C.c_void_p * n)()
    half = (C.c_void_p * n)(*([256] * 4 + [None] * (n - 4)))
    need = lib.tn_splat_mcmc_workspace_bytes(10, 4)

    def call(rows=10, K=3, src=d, dst=d, M=4, min_op=0.005, params=ptrs, m1=ptrs, m2=ptrs, ws=d, ws_bytes=need):
        return lib.tn_splat_mcmc_relocate(rows, K, src, dst, M, min_op, n, params, m1, m2, ws, ws_bytes, None)

    assert call(rows=-1) == EINVAL
    assert call(M=-1) == EINVAL
    assert b"draw count" in lib.tn_last_error()
    assert call(K=-1) == EINVAL and call(K=16) == EINVAL
    assert b"higher-order" in lib.tn_last_error()
    assert call(min_op=0.0) == EINVAL and call(min_op=1.0) == EINVAL
    assert call(rows=0) == EINVAL  # draws on no rows
    assert call(src=None) == EINVAL and call(dst=None) == EINVAL and call(ws=None) == EINVAL
    assert b"null pointer" in lib.tn_last_error()
    assert call(params=None) == EINVAL and call(m1=None) == EINVAL and call(m2=None) == EINVAL
    assert call(params=nulls) == EINVAL
    assert b"null parameter" in lib.tn_last_error()
    assert call(m1=half) == EINVAL  # a parameter's moments are both set or both null
    assert b"partly null" in lib.tn_last_error()
    assert call(ws_bytes=need - 1) == EINVAL
    assert b"workspace" in lib.tn_last_error()
    assert call(M=0, src=None, dst=None, params=None, m1=None, m2=None, ws=None, ws_bytes=0) == 0  # nothing drawn: nothing launched


def test_relocate_short_workspace_is_refused(lib):
    d = C.c_void_p(256)
    ptrs = (C.c_void_p * 8)(*([256] * 8))
    need = lib.tn_splat_mcmc_workspace_bytes(100000, 4)
    assert lib.tn_splat_mcmc_relocate(100000, 0, d, d, 4, 0.005, 8, ptrs, ptrs, ptrs, d, lib.tn_splat_mcmc_workspace_bytes(10, 4), None) == EINVAL
    assert need > lib.tn_splat_mcmc_workspace_bytes(10, 4)


def test_noise_refusals_before_any_launch(lib):
    d = C.c_void_p(256)
    odd = C.c_void_p(260)
    g = lib.tn_splat_mcmc_noise  # opacities_thermal fifth: null is the shared opacity (and so no refusal)
    f = lambda means, scales, quats, opacities, randn, *rest: g(means, scales, quats, opacities, None, randn, *rest)  # noqa: E731
    assert f(d, d, d, d, d, -1, 1.0, None) == EINVAL
    assert f(d, d, d, d, d, 1 << 31, 1.0, None) == EINVAL
    assert f(d, d, d, d, d, 10, -1.0, None) == EINVAL
    assert f(d, d, d, d, d, 10, float("nan"), None) == EINVAL
    assert f(d, d, d, d, d, 10, float("inf"), None) == EINVAL
    assert b"scaler" in lib.tn_last_error()
    for i in range(5):
        args = [d] * 5
        args[i] = None
        assert f(*args, 10, 1.0, None) == EINVAL
        assert b"null pointer" in lib.tn_last_error()
    assert f(d, d, odd, d, d, 10, 1.0, None) == EINVAL
    assert b"aligned" in lib.tn_last_error()
    for i in (0, 1, 2, 3, 5):
        args = [d] * 6
        args[i] = None
        assert g(*args, 10, 1.0, None) == EINVAL and b"null pointer" in lib.tn_last_error()
    assert g(d, d, d, d, d, d, -1, 1.0, None) == EINVAL
    assert f(None, None, None, None, None, 0, 1.0, None) == 0 and g(None, None, None, None, None, None, 0, 1.0, None) == 0  # N = 0: nothing launched


# ------------------------------------------------------------------------------------------------ the restatement's own properties
@pytest.mark.parametrize("o", [1e-4, 0.004, 0.005, 0.1, 0.5, 0.9, 1 - 1e-6])
def test_ratio_one_is_the_identity_up_to_the_clamp(o):
    logit = math.log(o / (1 - o))
    scales = np.array([-3.0, 0.5, -7.25])
    for th in (None, logit - 1.0, logit + 2.0):
        new_o, new_th, new_s = mf.relocation_value(logit, scales, 1, 0.005, th)
        clamped = min(max(o, 0.005), 1 - mf.EPS32)
        assert new_o == pytest.approx(math.log(clamped / (1 - clamped)), rel=1e-12, abs=1e-12)
        np.testing.assert_allclose(new_s, scales, rtol=0, atol=1e-12)  # denom = p' = p: the scale is unchanged whatever the clamp does
        if th is not None:
            c = min(max(float(mf.sigmoid(th)), 0.005), 1 - mf.EPS32)
            assert new_th == pytest.approx(math.log(c / (1 - c)), rel=1e-12, abs=1e-12)


@pytest.mark.parametrize("p", [0.01, 0.3, 0.75, 0.999])
def test_ratio_two_is_the_closed_form(p):
    logit = math.log(p / (1 - p))
    p_new = 1 - math.sqrt(1 - p)
    denom = 2 * p_new - p_new * p_new / math.sqrt(2)
    assert mf.denominator(p_new, 2) == pytest.approx(denom, rel=1e-14)
    new_o, _, new_s = mf.relocation_value(logit, [0.0, -1.0, 1.0], 2, 1e-9)
    assert new_o == pytest.approx(math.log(p_new / (1 - p_new)), rel=1e-10)
    np.testing.assert_allclose(new_s, np.array([0.0, -1.0, 1.0]) + math.log(p / denom), rtol=0, atol=1e-12)


@pytest.mark.parametrize("r", [1, 2, 3, 7, 20, 51])
def test_the_double_sum_folds_to_one_sum(r):
    """sum_{i=k+1..r} binom(i-1, k) = binom(r, k+1) (the hockey-stick identity): what the kernel sums"""
    for p_new in (1e-3, 0.05, 0.27):
        one = sum(float(math.comb(r, k + 1)) * (-1.0) ** k * p_new ** (k + 1) / math.sqrt(k + 1) for k in range(r))
        assert mf.denominator(p_new, r) == pytest.approx(one, rel=1e-9)


def test_the_ratio_is_clamped_to_n_max():
    a = mf.relocation_value(0.3, [0.1, 0.2, 0.3], 51, 0.005, -0.2)
    for r in (52, 70, 1000):
        b = mf.relocation_value(0.3, [0.1, 0.2, 0.3], r, 0.005, -0.2)
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert mf.relocation_value(0.3, [0.1, 0.2, 0.3], 0, 0.005)[0] == mf.relocation_value(0.3, [0.1, 0.2, 0.3], 1, 0.005)[0]


def test_the_dominant_chain_sets_the_scale_and_a_tie_goes_to_rgb():
    s = [0.0, 0.0, 0.0]
    rgb_only = mf.relocation_value(1.0, s, 3, 0.005)[2]
    np.testing.assert_array_equal(mf.relocation_value(1.0, s, 3, 0.005, -1.0)[2], rgb_only)  # o > o_th
    np.testing.assert_array_equal(mf.relocation_value(1.0, s, 3, 0.005, 1.0)[2], rgb_only)  # o = o_th
    np.testing.assert_array_equal(mf.relocation_value(-1.0, s, 3, 0.005, 1.0)[2], rgb_only)  # o < o_th: the thermal chain's value
    assert not np.array_equal(mf.relocation_value(-1.0, s, 3, 0.005, 1.0)[2], mf.relocation_value(-1.0, s, 3, 0.005)[2])


@pytest.mark.parametrize("n,cap,want", [(1, 100, 0), (19, 100, 0), (20, 100, 1), (300, 340, 15), (315, 340, 15), (330, 340, 10), (339, 340, 1),
                                        (340, 340, 0), (341, 340, 0), (1_000_000, 1_000_000, 0), (960_000, 1_000_000, 40_000)])
def test_growth_arithmetic(n, cap, want):
    assert mf.num_added(n, cap, 1.05) == want
    assert splat.mcmc_num_added(n, cap, 1.05) == want


def test_relocate_restatement_bookkeeping():
    rng = np.random.default_rng(0)
    n = 12
    params = {"means": rng.normal(size=(n, 3)), "scales": rng.normal(size=(n, 3)), "quats": rng.normal(size=(n, 4)),
              "opacities": rng.normal(size=(n, 1)), "features_dc": rng.normal(size=(n, 3)), "features_rest": rng.normal(size=(n, 3, 3)),
              "features_dc_thermal": rng.normal(size=(n, 1)), "features_rest_thermal": rng.normal(size=(n, 3, 1)),
              "opacities_thermal": rng.normal(size=(n, 1))}
    m1 = {k: rng.normal(size=v.shape) for k, v in params.items()}
    m2 = {k: rng.normal(size=v.shape) ** 2 for k, v in params.items()}
    src, dst = [0, 0, 3], [9, 10, 11]
    out, o1, o2 = mf.relocate(params, m1, m2, src, dst, 0.005)
    v0 = mf.relocation_value(params["opacities"][0, 0], params["scales"][0], 3, 0.005, params["opacities_thermal"][0, 0])
    assert out["opacities"][0, 0] == v0[0] and out["opacities_thermal"][0, 0] == v0[1] and np.array_equal(out["scales"][0], v0[2])
    for k in params:
        for s, d in zip(src, dst):
            assert np.array_equal(out[k][d], out[k][s]), k
        assert not o1[k][[0, 3]].any() and not o2[k][[0, 3]].any()
        untouched = [i for i in range(n) if i not in (0, 3)]
        assert np.array_equal(o1[k][untouched], m1[k][untouched]) and np.array_equal(o2[k][untouched], m2[k][untouched])
        rest = [i for i in range(n) if i not in (0, 3, 9, 10, 11)]
        assert np.array_equal(out[k][rest], params[k][rest])


def test_noise_restatement_leaves_visible_gaussians_alone():
    rng = np.random.default_rng(1)
    n = 64
    scales, quats, z = rng.uniform(-3, 0, (n, 3)), rng.normal(size=(n, 4)) * 3, rng.normal(size=(n, 3))
    op = np.where(np.arange(n) % 2 == 0, 3.0, -7.0).reshape(n, 1)
    d = mf.noise_delta(scales, quats, op, z, 80.0)
    assert np.abs(d[::2]).max() < 1e-15 and np.abs(d[1::2]).max() > 1e-6
    d_sep = mf.noise_delta(scales, quats, np.full((n, 1), -7.0), z, 80.0, op)  # the thermal opacity alone keeps the even ones in place
    np.testing.assert_allclose(d_sep, d, rtol=1e-12, atol=0)
    R = mf.rotation(quats)
    np.testing.assert_allclose(np.einsum("nij,nkj->nik", R, R), np.broadcast_to(np.eye(3), (n, 3, 3)), atol=1e-12)
    import torch

    t = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
    np.testing.assert_allclose(mf.noise_delta_torch(t(scales), t(quats), t(op), t(z), 80.0).numpy(), d, rtol=1e-9, atol=1e-18)
