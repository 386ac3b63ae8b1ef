"""The splat backward without a GPU: host-side argument checks of its entry points, and the reference its GPU tests differentiate -- the
functional restatement in splat_functional.py -- against the oracle's render and against float64 finite differences."""
import ctypes as C
import os

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib

import splat_abi
import splat_functional as sf
import splat_oracle as so

EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _camera(W=64, H=48):
    from nerfstudio_thermal_amd.splat import PinholeCamera, camera_struct

    return camera_struct(PinholeCamera(so.look_at_camera((2.5, 0.3, 0.6)), 60.0, 60.0, W / 2, H / 2, W, H))


def test_backward_workspace_size(lib):
    size = lib.tn_splat_backward_workspace_bytes
    assert size(-1, 10, 0, 0, 0) == -1
    assert size(10, -1, 0, 0, 0) == -1
    small, big = size(100, 1000, 0, 0, 0), size(100, 2000, 0, 0, 0)
    assert 0 < small < big and big - small >= 1000 * 10 * 4 - 256  # one record of 10 floats per (Gaussian, tile) pair (256-byte aligned)
    # every combination of the groups asks for exactly what its own size function used to
    assert {flags: (size(10, 100, *flags), size(1000, 5000, *flags)) for flags in splat_abi.BACKWARD_WORKSPACE_BYTES} == splat_abi.BACKWARD_WORKSPACE_BYTES
    for flags in splat_abi.BACKWARD_WORKSPACE_BYTES:
        assert size(-1, 5, *flags) == -1 and size(5, -1, *flags) == -1


def test_raster_train_argument_validation(lib):
    cam, bad = _camera(), _camera()
    bad.width = 0
    bg = (C.c_float * 4)()
    d = C.c_void_p(256)  # never dereferenced: every call below is refused before anything is read or launched
    train = lambda camera, n, out_t, out_last: lib.tn_splat_raster_chains(camera, n, d, 100, bg, 0, d, d, d, None, out_t, out_last, None, None, None)  # noqa: E731
    assert train(None, 10, d, d) == EINVAL
    assert train(C.byref(bad), 10, d, d) == EINVAL
    assert train(C.byref(cam), 10, None, d) == EINVAL
    assert b"null pointer" in lib.tn_last_error()
    assert train(C.byref(cam), 10, d, None) == EINVAL
    assert train(C.byref(cam), -1, d, d) == EINVAL


def test_raster_backward_argument_validation(lib):
    cam = _camera()
    bg = (C.c_float * 4)()
    d = C.c_void_p(256)
    need = lib.tn_splat_backward_workspace_bytes(10, 100, 0, 0, 0)

    def call(camera=C.byref(cam), n=10, cap=100, total=50, bws=need, v_xys=d):
        return lib.tn_splat_raster_backward(camera, n, d, cap, total, bg, 0, d, d, None, None, d, d, d, None, d, bws, v_xys, None, d, d, d, None, None, None, None, None)

    assert call(camera=None) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(total=101) == EINVAL  # more pairs than the forward workspace holds
    assert b"intersections" in lib.tn_last_error()
    assert call(total=-1) == EINVAL
    assert call(v_xys=None) == EINVAL
    assert b"null pointer" in lib.tn_last_error()
    assert call(bws=need - 1) == EINVAL
    assert b"backward workspace" in lib.tn_last_error()
    assert call(n=0) == 0  # nothing to do, nothing launched


def test_project_backward_argument_validation(lib):
    cam = _camera()
    d = C.c_void_p(256)

    def call(n=10, K=15, deg=3, rest=d, v_rest=d, radii=d):
        return lib.tn_splat_project_backward(C.byref(cam), None, None, d, d, d, d, d, rest, d, rest, None, n, K, deg, 0, radii, d, d, d, d, None, None, d, d, d, d, d, v_rest, d,
                                             v_rest, None, None, 0, None, None, None)

    assert call(deg=4) == EINVAL
    assert b"sh_degree" in lib.tn_last_error()
    assert call(deg=-2) == EINVAL
    assert call(K=8, deg=3) == EINVAL  # degree 3 needs 15 higher-order coefficients
    assert call(K=16) == EINVAL
    assert call(rest=None) == EINVAL
    assert call(v_rest=None) == EINVAL
    assert call(radii=None) == EINVAL
    assert call(n=-5) == EINVAL
    assert call(n=0) == 0


@pytest.mark.parametrize("mode,deg,seed,white", [("classic", 3, 1, False), ("antialiased", 3, 2, True), ("classic", 1, 3, True), ("antialiased", 0, 4, False)])
def test_functional_restatement_equals_the_oracle(mode, deg, seed, white):
    p = sf.scene(150, seed, max(deg, 0) if deg > 0 else 0)
    c2w = so.look_at_camera((2.4, 0.5 * seed - 1.0, 0.7))
    W, H = 64, 48
    fx = sf.fov_focal(W)
    bg = torch.ones(3) if white else torch.zeros(3)
    ref = so.render(p, c2w, fx, fx, 31.0, 24.5, W, H, sh_degree_to_use=deg if deg > 0 else -1, rasterize_mode=mode, background=bg, background_thermal=0.3)
    out = sf.render(p, c2w, fx, fx, 31.0, 24.5, W, H, sh_degree_to_use=deg if deg > 0 else -1, rasterize_mode=mode, background=bg, background_thermal=0.3)
    assert float(ref["accumulation"].max()) > 0.5  # the scene is on screen
    assert torch.equal(out["projection"]["radii"], ref["projection"]["radii"])
    for k in ("rgb", "thermal", "accumulation"):
        assert torch.allclose(out[k], ref[k], rtol=0, atol=1e-6), (k, float((out[k] - ref[k]).abs().max()))


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_float64_finite_differences_agree_with_autograd(mode):
    """Central differences of a random linear functional of (rgb, thermal, accumulation) in float64, element by element of every parameter,
    against autograd of the restatement on a tiny scene (8 Gaussians, 24x16 pixels, degree-3 SH).  The view directions of the SH colours stay
    those of the unperturbed means (they carry no gradient, splatfacto.py:770)."""
    torch.manual_seed(0)
    p = {k: v.double() for k, v in sf.scene(8, 7, 3, extent=0.4, scale_range=(-2.6, -1.8)).items()}
    c2w = so.look_at_camera((2.0, 0.2, 0.4))
    W, H = 24, 16
    fx = sf.fov_focal(W)
    args = (c2w, fx, fx, 11.5, 8.25, W, H)
    kw = dict(sh_degree_to_use=3, rasterize_mode=mode, background=torch.tensor([0.2, 0.1, 0.0]), background_thermal=0.4, viewdir_means=p["means"])
    w = {k: torch.randn(H, W, c, dtype=torch.float64) for k, c in (("rgb", 3), ("thermal", 1), ("accumulation", 1))}

    def loss(q):
        o = sf.render(q, *args, **kw)
        return sum((o[k] * w[k]).sum() for k in w), o

    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    L, o = loss(leaves)
    assert float(o["accumulation"].detach().max()) > 0.3
    L.backward()
    eps = 1e-6
    for name in sf.PARAM_NAMES:
        g = leaves[name].grad.reshape(-1)
        num = torch.zeros_like(g)
        for i in range(g.numel()):
            hi, lo = dict(p), dict(p)
            hi[name] = p[name].clone().reshape(-1)
            hi[name][i] += eps
            hi[name] = hi[name].reshape(p[name].shape)
            lo[name] = p[name].clone().reshape(-1)
            lo[name][i] -= eps
            lo[name] = lo[name].reshape(p[name].shape)
            with torch.no_grad():
                num[i] = (loss(hi)[0] - loss(lo)[0]) / (2 * eps)
        scale = float(g.abs().max()) + 1e-12
        assert float((num - g).abs().max()) <= 1e-5 * scale + 1e-9, (name, float((num - g).abs().max()), scale)
        assert float(g.abs().max()) > 0 or name == "features_rest", name
