"""The bilateral grid without a GPU: the torch restatement (bilagrid_functional.py) against closed forms, the header / binding / export of the
new entry points, their host-side argument checks (before any launch), the call layer's argument counts, the model's config and the optimiser table."""
import ctypes as C
import dataclasses
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib, optim, splat, splat_calls, splat_image

import bilagrid_functional as bf

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"tn_bilagrid_slice", "tn_bilagrid_slice_backward", "tn_bilagrid_workspace_bytes", "tn_bilagrid_tv", "tn_bilagrid_tv_workspace_bytes"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("C_,hw,shape", [(3, (37, 53), (16, 16, 8)), (1, (29, 41), (16, 16, 8)), (3, (5, 7), (5, 3, 4)), (1, (1, 40), (2, 2, 2))])
def test_identity_grid_gives_the_input(C_, hw, shape):
    image = bf.random_image(*hw, C_, seed=1).double()
    grid = bf.identity_grids(1, C_, shape, dtype=torch.float64)[0]
    assert grid.shape == (C_ * (C_ + 1), shape[2], shape[1], shape[0])
    torch.testing.assert_close(bf.slice(grid, image), image, rtol=0, atol=1e-15)


@pytest.mark.parametrize("C_", [3, 1])
def test_constant_grid_gives_the_affine_map(C_):
    g = torch.Generator().manual_seed(2)
    affine = torch.randn((C_, C_ + 1), generator=g, dtype=torch.float64)
    image = bf.random_image(23, 31, C_, seed=3).double()
    out = bf.slice(bf.constant_grids(1, affine, (5, 3, 4))[0], image)
    want = image @ affine[:, :C_].T + affine[:, C_]
    torch.testing.assert_close(out, want, rtol=0, atol=1e-14)


def test_slice_reads_position_and_brightness():
    """A grid whose offset is a linear ramp along one axis returns that axis' coordinate: x along GW, y along GH, the guidance along L."""
    image = bf.random_image(12, 20, 1, seed=4).double()
    H, W = image.shape[:2]
    for axis, want in ((4, ((torch.arange(W, dtype=torch.float64) + 0.5) / W).expand(H, W)), (3, ((torch.arange(H, dtype=torch.float64) + 0.5) / H).reshape(H, 1).expand(H, W)),
                       (2, image[..., 0])):
        grid = torch.zeros((2, 4, 5, 6), dtype=torch.float64)
        n = grid.shape[axis - 1]
        ramp = torch.linspace(0, 1, n, dtype=torch.float64).reshape([n if d == axis - 1 else 1 for d in range(1, 4)])
        grid[1] = ramp  # gain 0, offset = the ramp
        torch.testing.assert_close(bf.slice(grid, image)[..., 0], want.double(), rtol=0, atol=1e-14)


def test_guidance_is_the_luma():
    image = torch.tensor([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]]], dtype=torch.float64)
    torch.testing.assert_close(bf.guidance(image), torch.tensor([[0.299, 0.587, 0.114, 1.0]], dtype=torch.float64), rtol=0, atol=1e-15)


def test_tv_of_a_hand_written_grid():
    grids = torch.zeros((1, 1, 2, 2, 2), dtype=torch.float64)
    grids[0, 0, 1, 1, 1] = 3.0  # one corner: one difference of 3 along each axis, each difference tensor has 4 entries
    assert float(bf.tv(grids)) == pytest.approx(3 * 9.0 / 4.0, rel=1e-15)
    grids = torch.arange(8, dtype=torch.float64).reshape(1, 1, 2, 2, 2)  # differences 1 along x, 2 along y, 4 along z
    assert float(bf.tv(grids)) == pytest.approx(1.0 + 4.0 + 16.0, rel=1e-15)
    two = torch.cat([grids, torch.zeros_like(grids)])  # a second, constant frame halves it
    assert float(bf.tv(two)) == pytest.approx(21.0 / 2, rel=1e-15)


def test_tv_is_zero_for_constant_grids():
    assert float(bf.tv(bf.identity_grids(3, 3, (16, 16, 8), dtype=torch.float64))) == 0.0
    assert float(bf.tv(bf.constant_grids(2, torch.tensor([[0.8, 0.1]], dtype=torch.float64), (2, 2, 2)))) == 0.0


def test_near_planes_flags_the_planes_only():
    image = torch.tensor([[[0.5], [0.50001], [0.25], [0.3]]])
    assert bf.near_planes(image, 3).tolist() == [[True, True, False, False]]  # g (L - 1) = 1, 1.00002, 0.5, 0.6
    for C_, hw, L in ((3, (37, 53), 8), (1, (29, 41), 8), (3, (40, 64), 4)):
        assert float(bf.near_planes(bf.random_image(*hw, C_, seed=hw[0]), L).float().mean()) <= 0.01  # planes are 2e-4 (L - 1) of the range


# ---------------------------------------------------------------------------------------------------- header, binding, exports
def test_header_binding_and_exports_hold_the_new_symbols(lib):
    hdr = open(os.path.join(ROOT, "include", "thermal_nerf_hip.h")).read()
    declared = set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", hdr))
    assert SYMBOLS <= declared and SYMBOLS <= set(_lib.SIGNATURES)
    assert {k for k in _lib.SIGNATURES if k.startswith("tn_bilagrid")} == SYMBOLS
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 314 and lib.tn_version() == 314  # additions only: the version stays
    if shutil.which("nm") is not None:
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert SYMBOLS <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    build = open(os.path.join(ROOT, "nerfstudio-thermal_amd", "csrc", "build.sh")).read()
    assert build.count("tn_splat_bilagrid") == 2  # compiled and linked


def test_signatures_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "thermal_nerf_hip.h")).read()
    for name in SYMBOLS:
        decl = re.search(r"TN_API\s+\w+\s+%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_the_call_layer_passes_as_many_arguments_as_the_binding_declares(monkeypatch):
    sc, seen, T = splat_calls, {}, torch.zeros
    monkeypatch.setattr(sc, "_call", lambda name, *args: seen.__setitem__(name, len(args) + 1))  # + the stream
    monkeypatch.setattr(sc, "_ptr", lambda t, dtype, name: None if t is None else C.c_void_p(1))
    monkeypatch.setattr(sc, "_raw", lambda t: None if t is None else C.c_void_p(1))
    monkeypatch.setattr(sc, "workspace", lambda *a, **k: torch.empty(4, dtype=torch.uint8))
    grids = T(2, 12, 4, 3, 5)
    sc.bilagrid_slice(grids, 1, T(6, 7, 3), 3, T(6, 7, 3))
    sc.bilagrid_slice_backward(grids, 1, T(6, 7, 3), 3, T(6, 7, 3), T(6, 7, 3), T(12, 4, 3, 5))
    sc.bilagrid_tv(grids, 10.0, T(1), None)
    assert set(seen) == {"tn_bilagrid_slice", "tn_bilagrid_slice_backward", "tn_bilagrid_tv"}
    assert {name: n for name, n in seen.items() if n != len(_lib.SIGNATURES[name][1])} == {}
    assert set(re.findall(r'"(tn_bilagrid\w+)"', inspect.getsource(splat_calls))) == SYMBOLS


# ---------------------------------------------------------------------------------------------------- host-side checks, before any launch
def test_entry_points_refuse_bad_arguments_before_any_launch(lib):
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    fake = C.c_void_p(256 * 4096)  # a non-NULL address that is never dereferenced
    ok = dict(F=3, row=1, C_=3, gw=16, gh=16, gl=8, ps=4, H=37, W=53)

    def fwd(**kw):
        a = {**ok, **kw}
        return lib.tn_bilagrid_slice(ptr, a["F"], a["row"], a["C_"], a["gw"], a["gh"], a["gl"], ptr, a["ps"], a["H"], a["W"], ptr, None)

    def bwd(ws_bytes, **kw):
        a = {**ok, **kw}
        return lib.tn_bilagrid_slice_backward(ptr, a["F"], a["row"], a["C_"], a["gw"], a["gh"], a["gl"], ptr, a["ps"], a["H"], a["W"], ptr, fake, ws_bytes,
                                              ptr, ptr, None)

    need = lib.tn_bilagrid_workspace_bytes(3, 16, 16, 8, 37, 53)
    assert need == 12 * 8 * 16 * 16 * 4  # one row slice at this height
    assert lib.tn_bilagrid_workspace_bytes(3, 16, 16, 8, 1080, 1920) == 8 * need and lib.tn_bilagrid_workspace_bytes(1, 2, 2, 2, 1, 1) == 2 * 8 * 4
    bad = [dict(gw=1), dict(gh=1), dict(gl=1), dict(gw=257), dict(gh=257), dict(gl=257), dict(row=3), dict(row=-1), dict(F=0), dict(C_=2), dict(C_=4),
           dict(H=0), dict(W=0), dict(H=32769), dict(ps=2)]
    for kw in bad:
        assert fwd(**kw) == EINVAL, kw
        assert lib.tn_last_error().startswith(b"tn_bilagrid_slice:"), kw
        assert bwd(need, **kw) == EINVAL, kw
    for sizes in ((3, 1, 16, 8, 37, 53), (3, 16, 1, 8, 37, 53), (3, 16, 16, 1, 37, 53), (3, 257, 16, 8, 37, 53), (2, 16, 16, 8, 37, 53),
                  (3, 16, 16, 8, 0, 53), (3, 16, 16, 8, 37, 32769)):
        assert lib.tn_bilagrid_workspace_bytes(*sizes) == -1, sizes
    assert bwd(need - 1) == EINVAL
    assert b"workspace of" in lib.tn_last_error() and b"tn_bilagrid_workspace_bytes" in lib.tn_last_error()
    assert lib.tn_bilagrid_slice(None, 3, 1, 3, 16, 16, 8, ptr, 4, 37, 53, ptr, None) == EINVAL
    assert b"null pointer" in lib.tn_last_error()
    assert lib.tn_bilagrid_slice_backward(ptr, 3, 1, 3, 16, 16, 8, ptr, 4, 37, 53, ptr, fake, need, None, ptr, None) == EINVAL
    # the total variation
    need_tv = lib.tn_bilagrid_tv_workspace_bytes(5, 12, 16, 16, 8)
    assert need_tv == -(-5 * 12 * 8 * 16 * 16 // 256) * 4
    for sizes in ((0, 12, 16, 16, 8), (5, 0, 16, 16, 8), (5, 65, 16, 16, 8), (5, 12, 1, 16, 8), (5, 12, 16, 1, 8), (5, 12, 16, 16, 1), (5, 12, 16, 16, 257)):
        assert lib.tn_bilagrid_tv_workspace_bytes(*sizes) == -1, sizes
        assert lib.tn_bilagrid_tv(ptr, *sizes, 10.0, fake, 1 << 30, ptr, None, None) == EINVAL, sizes
    assert lib.tn_bilagrid_tv(ptr, 5, 12, 16, 16, 8, 10.0, fake, need_tv - 1, ptr, None, None) == EINVAL
    assert b"workspace of" in lib.tn_last_error()
    assert lib.tn_bilagrid_tv(ptr, 5, 12, 16, 16, 8, 10.0, fake, need_tv, None, None, None) == EINVAL


def test_python_functions_refuse_cpu_tensors_and_bad_shapes():
    grids = bf.identity_grids(2, 3, (4, 4, 2))
    with pytest.raises(ValueError, match="no CPU fallback"):
        splat_image.bilateral_slice(grids, 0, torch.zeros(5, 6, 3))
    with pytest.raises(ValueError, match="no CPU fallback"):
        splat_image.bilateral_grid_tv(grids, 10.0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        splat_image.bilateral_grid_tv(grids.clone().requires_grad_(True), 10.0)
    assert splat.bilateral_slice is splat_image.bilateral_slice and splat.bilateral_grid_tv is splat_image.bilateral_grid_tv
    for shape in ((2, 12, 2, 4), (2, 12, 1, 4, 4), (2, 12, 2, 257, 4), (0, 12, 2, 4, 4)):
        with pytest.raises(ValueError, match="2..256|F, K, L, GH, GW"):
            splat_calls._bilagrid_sizes(torch.zeros(shape), "test")
    assert splat_calls._bilagrid_sizes(grids, "test") == (2, 12, 2, 4, 4)
    assert splat_calls.BILAGRID_MAX_SIDE == 256


# ---------------------------------------------------------------------------------------------------- config, optimiser table, the model's names
def test_config_keys_and_validation():
    cfg = splat.ThermalSplatfactoModelConfig()
    assert cfg.use_bilateral_grid is False and cfg.grid_shape == (16, 16, 8) and cfg.bilateral_grid_tv_mult == 10.0
    assert splat.ThermalSplatfactoModelConfig(grid_shape=[5, 3, 4]).grid_shape == (5, 3, 4)
    assert splat.ThermalSplatfactoModelConfig(use_bilateral_grid=True, grid_shape=(2, 2, 2), bilateral_grid_tv_mult=0.0).use_bilateral_grid
    for shape in ((1, 16, 8), (16, 1, 8), (16, 16, 1), (16, 16), (16, 16, 8, 2), (257, 16, 8), (16.0, 16, 8), 16, None):
        with pytest.raises(ValueError, match="grid_shape"):
            splat.ThermalSplatfactoModelConfig(grid_shape=shape)
    with pytest.raises(ValueError, match="bilateral_grid_tv_mult"):
        splat.ThermalSplatfactoModelConfig(bilateral_grid_tv_mult=-1.0)
    names = [f.name for f in dataclasses.fields(splat.ThermalSplatfactoModelConfig)]
    assert names[-3:] == ["use_bilateral_grid", "grid_shape", "bilateral_grid_tv_mult"]  # appended: positional construction is as before


def test_optimiser_table():
    assert optim.SPLAT_BILAGRID_OPTIMIZERS == {"bilateral_grid": (2e-3, 1e-4, 30000), "bilateral_grid_thermal": (2e-3, 1e-4, 30000)}
    assert not set(optim.SPLAT_BILAGRID_OPTIMIZERS) & (set(optim.SPLAT_OPTIMIZERS) | set(optim.SPLAT_CAMERA_OPTIMIZERS))
    assert set(optim.SPLAT_OPTIMIZERS) == set(splat.GROUP_PARAMS_SEP)  # the Gaussian table is as it was


def test_identity_grids_of_the_model_are_the_restatements():
    for C_, shape in ((3, (16, 16, 8)), (1, (5, 3, 4))):
        assert torch.equal(splat.identity_bilateral_grids(3, C_, shape), bf.identity_grids(3, C_, shape))


def test_param_names_do_not_depend_on_the_switch():
    """The Gaussian parameters the C entry points take are those of before; the grids are module parameters of their own, outside gauss_params
    (the state-dict keys of a built model are checked on the device, in the GPU file: the model cannot be built without one)."""
    assert splat.param_names("shared") == splat._PARAM_NAMES and len(splat._PARAM_NAMES) == 8
    assert set(splat.GROUP_PARAMS) == {"xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation", "features_dc_thermal",
                                       "features_rest_thermal"}
    src = inspect.getsource(splat.ThermalSplatfactoModel.param_names.fget)
    assert "bil" not in src
