"""The splat C ABI as the tests see it: the entry points that were folded into one call per stage (and must stay gone), the header's parameter
names, the optional groups of every unified entry point, and the backward workspace sizes the retired size functions returned."""
import os
import re
import shutil
import subprocess

from nerfstudio_thermal_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22

# every name the one-call-per-stage ABI retired: variants that became nullable groups, and the two names that moved into the tn_splat_* family
RETIRED = ("tn_splat_project_sep", "tn_splat_project_crop", "tn_splat_project_crop_sep", "tn_splat_project_pose", "tn_splat_project_pose_sep",
           "tn_splat_raster_sep", "tn_splat_raster_train", "tn_splat_raster_train_sep",
           "tn_splat_backward_workspace_bytes_sep", "tn_splat_backward_workspace_bytes_abs", "tn_splat_backward_workspace_bytes_abs_sep",
           "tn_splat_depth_backward_workspace_bytes",
           "tn_splat_raster_backward_sep", "tn_splat_raster_backward_abs", "tn_splat_raster_backward_abs_sep", "tn_depth_splat_raster_backward",
           "tn_splat_project_backward_sep", "tn_splat_project_backward_pose", "tn_splat_project_backward_pose_sep", "tn_depth_splat_project_backward",
           "tn_splat_refine_plan_sep", "tn_splat_refine_apply_sep", "tn_splat_mcmc_relocate_sep", "tn_splat_mcmc_noise_sep",
           "tn_contrib_splat_raster", "tn_contrib_splat_workspace_bytes")

# entry point -> group -> the header's parameter names.  A group is given whole or left out whole; dview_out is optional inside the pose group.
GROUPS = {
    "tn_splat_project": {"pose": ("pose_camera",), "sep": ("opacities_thermal",), "crop": ("crop",)},
    "tn_splat_raster": {},
    "tn_splat_raster_chains": {"sep": ("out_alpha_thermal",), "train": ("out_transmittance", "out_last"),
                               "train_sep": ("out_transmittance_thermal", "out_last_thermal")},
    "tn_splat_raster_backward": {"sep": ("transmittance_thermal", "last_thermal", "v_alpha_thermal", "v_log_opacity_thermal"), "abs": ("v_xys_abs",),
                                 "depth": ("depth", "v_depth", "v_depths")},
    "tn_splat_project_backward": {"sep": ("opacities_thermal", "v_log_opacity_thermal", "v_opacities_thermal"),
                                  "pose": ("pose_camera", "pose_row", "workspace", "grad_pose_row", "dview_out"), "depth": ("v_depths",)},
    "tn_splat_refine_plan": {"sep": ("opacities_thermal",)},
    "tn_splat_refine_apply": {},
    "tn_splat_mcmc_relocate": {},
    "tn_splat_mcmc_noise": {"sep": ("opacities_thermal",)},
    "tn_splat_raster_contrib": {"weight": ("pixel_weight",)},
}

# tn_splat_backward_workspace_bytes(N, max_intersections, sep, absgrad, depth) at (10, 100) and (1000, 5000): what the retired size function of
# each combination returned (the four names, and tn_splat_depth_backward_workspace_bytes(N, M, sep, absgrad) for the depth ones)
BACKWARD_WORKSPACE_BYTES = {(0, 0, 0): (4352, 204288), (1, 0, 0): (4864, 224256), (0, 1, 0): (5120, 244224), (1, 1, 0): (5632, 264192),
                            (0, 0, 1): (4864, 224256), (1, 0, 1): (5120, 244224), (0, 1, 1): (5632, 264192), (1, 1, 1): (5888, 284160)}


def header() -> str:
    return open(os.path.join(ROOT, "include", "thermal_nerf_hip.h")).read()


def declaration(hdr: str, name: str) -> str:
    m = re.search(r"TN_API\s+int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m, name
    return m.group(1)


def param_names(hdr: str, name: str) -> list:
    """The parameter names of `name`'s declaration, in order (the stream last)."""
    return [re.search(r"(\w+)\s*$", a).group(1) for a in declaration(hdr, name).split(",")]


def exported(lib_path: str):
    """The tn_* symbols the built library exports, or None without nm."""
    nm = shutil.which("nm")
    if not nm:
        return None
    return set(re.findall(r" T (tn_\w+)", subprocess.run([nm, "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout))


def assert_unified(lib, present) -> None:
    """`present` are declared, bound with the binding's types and exported; every retired name is gone from the header, the binding and the exports."""
    declared = set(re.findall(r"\b(tn_[a-z0-9_]+)\s*\(", header()))
    exp = exported(_lib.LIB_PATH)
    for name in present:
        assert name in declared and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
        assert exp is None or name in exp, name
    for name in RETIRED:
        assert name not in declared and name not in _lib.SIGNATURES, name
        assert exp is None or name not in exp, name
