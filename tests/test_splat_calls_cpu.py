"""The call layer of the splat path (splat_calls.py) without a GPU: every tn_splat_* entry point is reachable from the module, every stage passes
its entry point as many arguments as the binding declares with None exactly at the parameters of the groups the caller left out, the library
refuses a group given in part, and splat.py hands out the moved names as the same objects."""
import ctypes as C
import inspect
import itertools
import os
import re

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib, splat, splat_calls, splat_camera, splat_image

import splat_abi

# what anything imports from splat today (tests, bench.py, scripts, splat_datamanager.py)
SPLAT_NAMES = ("ThermalSplatfactoModel", "ThermalSplatfactoModelConfig", "PinholeCamera", "OrientedBox", "SplatCameraOptimizer", "camera_struct",
               "pose_camera_record", "rescaled_camera", "downscale_factor", "undistorted_camera", "undistort_image", "resize_image", "image_loss",
               "thermal_regularizers", "knn_distances", "mcmc_relocate", "mcmc_noise", "mcmc_num_added", "param_names", "GROUP_PARAMS",
               "GROUP_PARAMS_SEP", "_PARAM_NAMES", "projection_matrix", "ssim", "RGB2SH", "SH_C0", "BLOCK_WIDTH", "KNN_MAX_K", "MCMC_N_MAX",
               "STRATEGIES", "VIEWER_BACKGROUND")
REST = {"features_rest", "thermal_rest", "v_features_rest", "v_thermal_rest"}  # null without higher-order SH coefficients (K == 0)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_every_splat_entry_point_is_reachable():
    """Spelled out as a fixed name in the module's source: nothing the library binds is orphaned, and nothing spelled is unknown to it."""
    fixed = set(re.findall(r'"(tn_splat_\w+)"', inspect.getsource(splat_calls)))
    bound = {k for k in _lib.SIGNATURES if k.startswith("tn_splat_")}
    assert bound - fixed == set()
    assert fixed - bound == set()
    assert "tn_splat_raster_contrib" in fixed and not hasattr(splat_calls, "entry") and not hasattr(splat_calls, "FAMILIES")


def _on(flags, names):
    return dict(zip(names, flags))


def test_every_stage_passes_the_bindings_arguments_with_none_at_the_absent_groups(monkeypatch):
    """Every stage in every combination of its optional groups, on CPU placeholders with the pointer checks and the library call replaced.  The
    argument list is fixed, so a miscount is ctypes' TypeError only on the device, and a None in the wrong place is not an error at all: here the
    count must be the binding's, and None must sit exactly at the header's parameters of the groups left out (and at the rest coefficients of a
    frame without any)."""
    sc, seen, hdr = splat_calls, [], splat_abi.header()
    monkeypatch.setattr(sc, "_call", lambda name, *args: seen.append((name, args)))
    monkeypatch.setattr(sc, "_ptr", lambda t, dtype, name: None if t is None else C.c_void_p(1))
    monkeypatch.setattr(sc, "_raw", lambda t: None if t is None else C.c_void_p(1))
    monkeypatch.setattr(sc, "_pose_row_ptr", lambda *a, **k: C.c_void_p(1))
    monkeypatch.setattr(sc, "workspace", lambda *a, **k: torch.empty(4, dtype=torch.uint8))
    cam, crop, rs, bg, T = _lib.TnSplatCamera(), _lib.TnSplatCrop(), _lib.TnSplatRefine(), (C.c_float * 4)(), torch.zeros
    idx, proj, counts = torch.zeros(2, dtype=torch.int64), {k: T(5) for k in "abcdefg"}, (C.c_int64 * 4)()
    calls = 0

    def check(name, absent, k=15):
        """The one call recorded since the last check went to `name`, with the binding's count and None exactly at `absent`'s parameters."""
        nonlocal calls
        assert len(seen) == calls + 1, (name, [n for n, _ in seen[calls:]])
        got, args = seen[-1]
        calls += 1
        names = splat_abi.param_names(hdr, name)
        assert got == name and len(args) + 1 == len(names) == len(_lib.SIGNATURES[name][1]), (name, got, len(args) + 1, len(names))
        want = {p for g in absent for p in splat_abi.GROUPS[name][g]} | ({p for p in REST if p in names} if k == 0 else set())
        assert {n for n, a in zip(names, args) if a is None} == want, (name, absent, k)

    def params(sep, k=15):
        return [T(5, 3), T(5, 3), T(5, 4), T(5, 1), T(5, 3), T(5, k, 3), T(5, 1), T(5, k, 1), T(5, 1)][:9 if sep else 8]

    two, three = list(itertools.product((False, True), repeat=2)), list(itertools.product((False, True), repeat=3))
    for (crop_on, pose_on, sep), k in [(c, 15) for c in three] + [((False, False, False), 0), ((True, True, True), 0)]:
        sc.project(cam, params(sep, k), 3 if k else 0, 0, proj, T(4), 10, crop=crop if crop_on else None, pose_rec=T(40) if pose_on else None)
        check("tn_splat_project", [g for g, on in (("crop", crop_on), ("pose", pose_on), ("sep", sep)) if not on], k)
    for (sep, pose_on, depth), k in [(c, 15) for c in three] + [((False, False, False), 0), ((True, True, True), 0)]:
        P, th = params(sep, k), (T(5) if sep else None)
        pose = (T(40), T(2, 6), 0, T(2, 6), T(3, 4)) if pose_on else ()
        sc.project_backward(cam, P, 3 if k else 0, 0, T(5), T(5), T(5), T(5), T(5), P, th, *pose, v_depths=T(5) if depth else None)
        check("tn_splat_project_backward", [g for g, on in (("sep", sep), ("pose", pose_on), ("depth", depth)) if not on], k)
    for sep in (False, True):
        th = T(1) if sep else None
        sc.raster(cam, 5, T(4), 10, bg, 0, T(1), T(1), T(1), th)
        check(*(("tn_splat_raster_chains", ["train", "train_sep"]) if sep else ("tn_splat_raster", [])))
        sc.raster_train(cam, 5, T(4), 10, bg, 0, T(1), T(1), T(1), T(1), T(1), *([th] * 3 if sep else []))
        check("tn_splat_raster_chains", [] if sep else ["sep", "train_sep"])
    for sep, absgrad, depth in three:
        sc.raster_backward(cam, 5, T(4), 10, 7, bg, *[T(1)] * 9, *([T(1)] * 4 if sep else [None] * 4), v_xys_abs=T(1) if absgrad else None,
                           **(dict(aa=0, depth=T(1), v_depth=T(1), v_depths=T(5)) if depth else {}))
        check("tn_splat_raster_backward", [g for g, on in (("sep", sep), ("abs", absgrad), ("depth", depth)) if not on])
    for sep in (False, True):
        P, n, th = params(sep), 9 if sep else 8, (T(5) if sep else None)
        sc.refine_plan(rs, 600, T(5, 3), T(5, 1), [T(5)] * 3, 5, 2, counts, th)
        check("tn_splat_refine_plan", [] if sep else ["sep"])
        sc.mcmc_noise(T(5, 3), T(5, 3), T(5, 4), T(5, 1), T(5, 3), 1.0, th)
        check("tn_splat_mcmc_noise", [] if sep else ["sep"])
        sc.refine_apply(rs, 5, 15, T(4), counts, T(2, 3), P, P, P, P, P, P)
        check("tn_splat_refine_apply", [])
        sc.mcmc_relocate(P, [None] * n, [None] * n, idx, idx, 0.1)
        check("tn_splat_mcmc_relocate", [])
        for name in ("tn_splat_refine_apply", "tn_splat_mcmc_relocate"):  # the count the library is told is the length of every array it is handed
            args = dict(zip(splat_abi.param_names(hdr, name), [a for got, a in seen if got == name][-1]))
            assert args["num_tensors"] == n and len(args["params"]) == len(args["exp_avg"]) == len(args["exp_avg_sq"]) == n
    for weight in (None, T(0, 0)):
        sc.raster_contrib(cam, 5, T(4), 10, 0, 0, weight, T(5), T(5), T(5), T(5))
        check("tn_splat_raster_contrib", [] if weight is not None else ["weight"])
    for name, absent in splat_abi.GROUPS.items():  # every group of every entry point was seen both given and left out
        for g, members in absent.items():
            nulls = {all(a is None for n, a in zip(splat_abi.param_names(hdr, name), args) if n in members) for got, args in seen if got == name}
            assert nulls == {False, True}, (name, g)
    sc.raster_removal(cam, 5, T(4), 10, bg, 0.1, T(1))
    sc.pose_camera(cam, 1.0, 1.0, T(2, 6), 0, T(40))
    sc.crop_mask(crop, T(5, 3), T(5))
    sc.grad_stats(T(5, 2), T(5), 5, 100, True, T(5), T(5), T(5))
    sc.knn(T(5, 3), 5, 3, T(5, 3), None)
    sc.image_loss_call(T(1), 3, T(1), 3, 11, 11, 3, 0.2, 1.0, T(3), None)
    sc.thermal_reg(T(1), 1, T(1), 3, 11, 11, 1.0, 1.0, T(2), None)
    sc.image_resize(T(4, 4, 3), 3, T(2, 2, 3))
    sc.image_undistort(T(4, 4, 3), 3, T(4, 4, 3), _lib.TnUndistort())
    assert {name: len(args) + 1 for name, args in seen if len(args) + 1 != len(_lib.SIGNATURES[name][1])} == {}
    launches = {k for k in _lib.SIGNATURES if k.startswith(("tn_splat_", "tn_knn", "tn_image_", "tn_thermal_reg")) and "workspace_bytes" not in k}
    assert "tn_splat_raster_contrib" in launches
    assert launches - {name for name, _ in seen} == {"tn_splat_bin"}  # (its return code is read before the check, so it does not go through _call)


def test_the_library_refuses_a_partly_given_group_before_any_launch(lib):
    """Every group of every unified entry point with one member missing, and with one member alone: TN_EINVAL with the entry point's name, on the
    host (nothing here is a device pointer).  num_tensors other than 8 or 9 likewise."""
    hdr, d, EINVAL = splat_abi.header(), C.c_void_p(256), splat_abi.EINVAL
    cam = _lib.TnSplatCamera(fx=30.0, fy=30.0, width=40, height=24)
    N, cap = 10, 100
    full = {  # every pointer given, every size good: name -> arguments by the header's parameter names (stream last, null)
        "tn_splat_raster_chains": dict(camera=C.byref(cam), num_gaussians=N, max_intersections=cap, antialiased=0),
        "tn_splat_raster_backward": dict(camera=C.byref(cam), num_gaussians=N, max_intersections=cap, num_intersections=50, antialiased=0,
                                         bwd_workspace_bytes=lib.tn_splat_backward_workspace_bytes(N, cap, 1, 1, 1)),
        "tn_splat_project_backward": dict(camera=C.byref(cam), num_gaussians=N, num_rest_coeffs=0, sh_degree=0, antialiased=0,
                                          workspace_bytes=lib.tn_splat_pose_workspace_bytes(N)),
    }

    def call(name, **null):
        args = [None if n in null or n == "stream" else full[name].get(n, d) for n in splat_abi.param_names(hdr, name)]
        return getattr(lib, name)(*args)

    for name in full:
        for g, members in splat_abi.GROUPS[name].items():
            members = tuple(m for m in members if m != "dview_out")
            if len(members) < 2:
                continue
            for m in members:
                others = {o: None for o in members if o != m}
                for null in ({m: None}, others):  # one member missing; one member alone
                    assert call(name, **null) == EINVAL, (name, g, m, null)
                    err = lib.tn_last_error()
                    assert name.encode() + b":" in err and (b"partly given" in err or b"go with" in err), (name, g, err)
    # the raster's thermal pair goes with the other two groups, and only with them
    assert call("tn_splat_raster_chains", out_alpha_thermal=None) == EINVAL and b"go with" in lib.tn_last_error()
    assert call("tn_splat_raster_chains", out_transmittance=None, out_last=None) == EINVAL and b"go with" in lib.tn_last_error()
    assert call("tn_splat_raster_chains", out_transmittance_thermal=None, out_last_thermal=None) == EINVAL and b"go with" in lib.tn_last_error()
    # dview_out is optional inside the pose group, and is no group of its own
    pose = {m: None for m in splat_abi.GROUPS["tn_splat_project_backward"]["pose"] if m != "dview_out"}
    assert call("tn_splat_project_backward", **pose) == EINVAL and b"partly given" in lib.tn_last_error()
    # the depth groups are still refused in antialiased mode
    full["tn_splat_raster_backward"]["antialiased"] = full["tn_splat_project_backward"]["antialiased"] = 1
    assert call("tn_splat_raster_backward") == EINVAL and b"tn_splat_raster_backward: the depth gradient exists in classic mode only" in lib.tn_last_error()
    assert call("tn_splat_project_backward") == EINVAL and b"tn_splat_project_backward: the depth gradient exists in classic mode only" in lib.tn_last_error()
    # eight or nine tensors per array
    rs = _lib.TnSplatRefine(n_split_samples=2)
    counts, arr = (C.c_int64 * 4)(0, N, 0, 0), (C.c_void_p * 10)(*([256] * 10))
    wb, mb = lib.tn_splat_refine_workspace_bytes(N, 2), lib.tn_splat_mcmc_workspace_bytes(N, 4)
    for nt in (7, 10, 0, -1):
        assert lib.tn_splat_refine_apply(C.byref(rs), N, 0, d, wb, counts, None, nt, arr, arr, arr, arr, arr, arr, None) == EINVAL
        assert b"tn_splat_refine_apply: %d tensors" % nt in lib.tn_last_error()
        assert lib.tn_splat_mcmc_relocate(N, 0, d, d, 4, 0.005, nt, arr, arr, arr, d, mb, None) == EINVAL
        assert b"tn_splat_mcmc_relocate: %d tensors" % nt in lib.tn_last_error()


def test_splat_hands_out_the_moved_names_themselves():
    homes = (splat_camera, splat_image, splat_calls)
    moved = 0
    for name in SPLAT_NAMES:
        assert hasattr(splat, name), name
        at_home = [m for m in homes if hasattr(m, name)]
        assert all(getattr(splat, name) is getattr(m, name) for m in at_home), name
        moved += bool(at_home)
    assert moved >= 20  # the cameras, the image functions and the raw wrappers live in the three modules; the model and its constants in splat
    assert nerfstudio_thermal_amd.OrientedBox is splat_camera.OrientedBox
