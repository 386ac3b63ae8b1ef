"""The call layer of the splat path (splat_calls.py) without a GPU: `entry` composes exactly the variant names the library binds, every tn_splat_*
entry point is reachable from the module, every stage passes its variant as many arguments as the binding declares, and splat.py hands out the
moved names as the same objects."""
import ctypes as C
import inspect
import itertools
import re

import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib, splat, splat_calls, splat_camera, splat_image

FLAGS = ("abs", "crop", "pose", "sep")
# the variants include/thermal_nerf_hip.h declares, family by family: the flags that may be on, and the pairs that never go together
HEADER = {"tn_splat_project": ({"crop", "pose", "sep"}, [{"crop", "pose"}]), "tn_splat_raster": ({"sep"}, []), "tn_splat_raster_train": ({"sep"}, []),
          "tn_splat_raster_backward": ({"abs", "sep"}, []), "tn_splat_backward_workspace_bytes": ({"abs", "sep"}, []),
          "tn_splat_project_backward": ({"pose", "sep"}, []), "tn_splat_refine_plan": ({"sep"}, []), "tn_splat_refine_apply": ({"sep"}, []),
          "tn_splat_mcmc_relocate": ({"sep"}, []), "tn_splat_mcmc_noise": ({"sep"}, [])}
# what anything imports from splat today (tests, bench.py, scripts, splat_datamanager.py)
SPLAT_NAMES = ("ThermalSplatfactoModel", "ThermalSplatfactoModelConfig", "PinholeCamera", "OrientedBox", "SplatCameraOptimizer", "camera_struct",
               "pose_camera_record", "rescaled_camera", "downscale_factor", "undistorted_camera", "undistort_image", "resize_image", "image_loss",
               "thermal_regularizers", "knn_distances", "mcmc_relocate", "mcmc_noise", "mcmc_num_added", "param_names", "GROUP_PARAMS",
               "GROUP_PARAMS_SEP", "_PARAM_NAMES", "projection_matrix", "ssim", "RGB2SH", "SH_C0", "BLOCK_WIDTH", "KNN_MAX_K", "MCMC_N_MAX",
               "STRATEGIES", "VIEWER_BACKGROUND")


def _combinations():
    for base in HEADER:
        for bits in itertools.product((False, True), repeat=len(FLAGS)):
            yield base, dict(zip(FLAGS, bits))


def _composed():
    names = set()
    for base, on in _combinations():
        try:
            names.add(splat_calls.entry(base, **on))
        except ValueError:
            pass
    return names


def test_entry_composes_the_bound_names_and_refuses_the_rest():
    assert set(splat_calls.FAMILIES) == set(HEADER)
    for base, on in _combinations():
        allowed, never = HEADER[base]
        chosen = {f for f in FLAGS if on[f]}
        if chosen <= allowed and not any(pair <= chosen for pair in never):
            name = splat_calls.entry(base, **on)
            assert name in _lib.SIGNATURES, (base, on, name)
            assert name == base + "".join("_" + f for f in FLAGS if on[f])  # abs / crop / pose before sep, as the header spells them
        else:
            try:
                got = splat_calls.entry(base, **on)
            except ValueError:
                continue
            raise AssertionError(f"entry({base!r}, {on}) = {got!r}: the header has no such variant")
    try:
        splat_calls.entry("tn_splat_bin", sep=True)
    except ValueError:
        pass
    else:
        raise AssertionError("a name outside the families must be refused")
    assert splat_calls.entry("tn_splat_project") == "tn_splat_project" and splat_calls.entry("tn_splat_project", pose=True, sep=True) == "tn_splat_project_pose_sep"


def test_every_splat_entry_point_is_reachable():
    """Composed by `entry`, or spelled out as a fixed name in the module's source: nothing the library binds is orphaned, and nothing composed
    or spelled is unknown to it."""
    fixed = set(re.findall(r'"(tn_splat_\w+)"', inspect.getsource(splat_calls)))
    bound = {k for k in _lib.SIGNATURES if k.startswith("tn_splat_")}
    assert bound - (_composed() | fixed) == set()
    assert (_composed() | fixed) - bound == set()


def test_every_stage_passes_as_many_arguments_as_the_binding_declares(monkeypatch):
    """Every stage in every variant, on CPU placeholders with the pointer checks and the library call replaced: the segments add up to the
    argument list of the name they go to (a miscount would otherwise show only on the device, as ctypes' TypeError)."""
    sc, seen = splat_calls, {}
    monkeypatch.setattr(sc, "_call", lambda name, *args: seen.__setitem__(name, len(args) + 1))  # + the stream
    monkeypatch.setattr(sc, "_ptr", lambda t, dtype, name: None if t is None else C.c_void_p(1))
    monkeypatch.setattr(sc, "_raw", lambda t: None if t is None else C.c_void_p(1))
    monkeypatch.setattr(sc, "_pose_row_ptr", lambda *a, **k: C.c_void_p(1))
    monkeypatch.setattr(sc, "workspace", lambda *a, **k: torch.empty(4, dtype=torch.uint8))
    cam, crop, rs, bg, T = _lib.TnSplatCamera(), _lib.TnSplatCrop(), _lib.TnSplatRefine(), (C.c_float * 4)(), torch.zeros
    idx, proj = torch.zeros(2, dtype=torch.int64), {k: T(5) for k in "abcdefg"}
    for n in (8, 9):
        P = [T(5, 3), T(5, 3), T(5, 4), T(5, 1), T(5, 3), T(5, 15, 3), T(5, 1), T(5, 15, 1), T(5, 1)][:n]
        th = T(5) if n == 9 else None
        for kw in ({}, {"crop": crop}, {"pose_rec": T(40)}, {"crop": crop, "pose_rec": T(40)}):
            sc.project(cam, P, 3, 0, proj, T(4), 10, **kw)
        sc.project_backward(cam, P, 3, 0, T(5), T(5), T(5), T(5), T(5), P, th)
        sc.project_backward(cam, P, 3, 0, T(5), T(5), T(5), T(5), T(5), P, th, T(40), T(2, 6), 0, T(2, 6), T(3, 4))
        sc.refine_apply(rs, 5, 15, T(4), None, None, P, P, P, P, P, P)
        sc.mcmc_relocate(P, [None] * n, [None] * n, idx, idx, 0.1)
        sc.refine_plan(rs, 600, T(5, 3), T(5, 1), [T(5)] * 3, 5, 2, None, th)
        sc.mcmc_noise(T(5, 3), T(5, 3), T(5, 4), T(5, 1), T(5, 3), 1.0, th)
        sc.raster(cam, 5, T(4), 10, bg, 0, T(1), T(1), T(1), th)
        sc.raster_train(cam, 5, T(4), 10, bg, 0, T(1), T(1), T(1), T(1), T(1), *([th] * 3 if n == 9 else []))
        for v_abs in (None, T(1)):
            sc.raster_backward(cam, 5, T(4), 10, 7, bg, *[T(1)] * 9, *([th] * 4 if n == 9 else []), v_xys_abs=v_abs)
    sc.raster_removal(cam, 5, T(4), 10, bg, 0.1, T(1))
    sc.pose_camera(cam, 1.0, 1.0, T(2, 6), 0, T(40))
    sc.crop_mask(crop, T(5, 3), T(5))
    sc.grad_stats(T(5, 2), T(5), 5, 100, True, T(5), T(5), T(5))
    sc.knn(T(5, 3), 5, 3, T(5, 3), None)
    sc.image_loss_call(T(1), 3, T(1), 3, 11, 11, 3, 0.2, 1.0, T(3), None)
    sc.thermal_reg(T(1), 1, T(1), 3, 11, 11, 1.0, 1.0, T(2), None)
    sc.image_resize(T(4, 4, 3), 3, T(2, 2, 3))
    sc.image_undistort(T(4, 4, 3), 3, T(4, 4, 3), _lib.TnUndistort())
    assert {name: n for name, n in seen.items() if n != len(_lib.SIGNATURES[name][1])} == {}
    launches = {k for k in _lib.SIGNATURES if k.startswith(("tn_splat_", "tn_knn", "tn_image_", "tn_thermal_reg")) and "workspace_bytes" not in k}
    assert launches - set(seen) == {"tn_splat_bin"}  # (its return code is read before the check, so it does not go through _call)


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
