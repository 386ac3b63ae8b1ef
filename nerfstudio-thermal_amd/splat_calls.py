"""The call layer of the splat path: the one module that names the tn_splat_* / tn_knn / tn_image_* / tn_thermal_reg / tn_depth_loss / tn_bilagrid_* /
tn_transform_splat / tn_filter3d_splat_* entry points of libthermal_nerf_hip.so and knows their argument order (include/thermal_nerf_hip.h).  The
three gsplat calls (project_gaussians, spherical_harmonics, rasterize_gaussians x2) run as tn_splat_project / tn_splat_bin / tn_splat_raster_chains.
Every stage has ONE entry point with a fixed argument list; what a frame may or may not have -- the thermal opacity of separate mode, a crop box,
a pose record, absgrad, the depth gradient -- is a group of nullable pointers, and a tensor the caller does not pass goes in as None (null): the
library picks the kernel instantiation from the groups it is given and refuses a group given in part.  The caller decides which tensors exist:
nothing is allocated here but workspaces.  Everything goes to the current stream; nothing but refine_plan's counts is read back.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from .ops import _stream

KNN_MAX_K = 8  # tn_knn's largest k
F32, I32 = torch.float32, torch.int32

_PARAM_NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest", "features_dc_thermal", "features_rest_thermal")
# thermal_opacity_mode "separate": the thermal opacity logits come ninth, in a group of their own
_PARAM_NAMES_SEP = _PARAM_NAMES + ("opacities_thermal",)

def param_names(mode: str) -> Tuple[str, ...]:
    """The gauss_params entries of a thermal_opacity_mode, in the order the C entry points take them."""
    return _PARAM_NAMES_SEP if mode == "separate" else _PARAM_NAMES


def _ptr(t: Optional[Tensor], dtype, name: str):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} HIP tensor (the splat path has no CPU fallback)")
    return C.c_void_p(t.data_ptr())


def _raw(t: Optional[Tensor]):
    """The pointer of a tensor its caller has already checked (or allocated); None stays null."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(**named) -> list:
    """Checked pointers of fp32 tensors, each reported under its keyword."""
    return [_ptr(t, F32, n) for n, t in named.items()]


def _pose_row_ptr(pose: Tensor, row: int, name: str = "pose_adjustment"):
    """Device pointer of row `row` of a contiguous fp32 [C,6] tensor (a host offset: nothing is read)."""
    _ptr(pose, F32, name)
    if pose.dim() != 2 or pose.shape[1] != 6 or not 0 <= row < pose.shape[0]:
        raise ValueError(f"{name} must be [C,6] with the frame's row {row} inside, got {tuple(pose.shape)}")
    return C.c_void_p(pose.data_ptr() + 24 * row)


def _param_ptrs(tensors) -> list:
    """Pointers of eight tensors laid out as the gauss_params, in _PARAM_NAMES order, as the C entry points take them: without higher-order SH
    coefficients (K == 0) the two features_rest tensors are null, and opacities [N,1] goes in flat.  Nine tensors (separate thermal opacity):
    opacities_thermal [N,1] follows, flat too."""
    K = tensors[5].shape[1]
    pp = [_ptr(t, F32, n) if (K or not n.startswith("features_rest")) else None for t, n in zip(tensors, _PARAM_NAMES_SEP)]
    for j in (3, 8)[:len(tensors) - 7]:
        pp[j] = _ptr(tensors[j].reshape(-1), F32, _PARAM_NAMES_SEP[j])
    return pp


def _call(name: str, *args) -> None:
    _lib.check(getattr(_lib.load(), name)(*args, _stream()), name)


def workspace_bytes(size_fn_name: str, *sizes, what: str = "bad sizes", exc=RuntimeError) -> int:
    """What `size_fn_name`(*sizes) asks for; a negative answer (sizes the library refuses) raises `exc`."""
    need = int(getattr(_lib.load(), size_fn_name)(*sizes))
    if need < 0:
        raise exc(f"{size_fn_name}: {what}")
    return need


def workspace(size_fn_name: str, *sizes, device, what: str = "bad sizes", exc=RuntimeError) -> Tensor:
    """A uint8 workspace of the size `size_fn_name`(*sizes) asks for."""
    return torch.empty(workspace_bytes(size_fn_name, *sizes, what=what, exc=exc), dtype=torch.uint8, device=device)


frame_workspace_bytes = functools.partial(workspace_bytes, "tn_splat_workspace_bytes")  # (Gaussians, room for (Gaussian, tile) pairs, tiles)


# ---------------------------------------------------------------------------------------------------- the frame: project -> bin -> raster
def _param_ptrs9(tensors) -> list:
    """_param_ptrs in the fixed nine places of the frame's entry points: eight tensors (shared opacity) leave the thermal opacity's place null."""
    return _param_ptrs(tensors) + [None] * (9 - len(tensors))


def project(cam, params, deg, aa, proj, ws, cap, crop=None, pose_rec=None) -> None:
    """tn_splat_project of the 8 (9: separate thermal opacity) `params` into the seven tensors of `proj` (in the header's order) and the frame
    workspace `ws`.  With `crop` (a TnSplatCrop) Gaussians outside the box leave with radius 0; with `pose_rec` (pose_camera's record) the
    corrected camera is read from that record."""
    _call("tn_splat_project", C.byref(cam), _ptr(pose_rec, F32, "pose camera"), *_param_ptrs9(params), params[0].shape[0], params[5].shape[1], deg, aa,
          *[_ptr(t, t.dtype, k) for k, t in proj.items()], _raw(ws), cap, C.byref(crop) if crop is not None else None)


def bin(cam, depths, N, ws, cap, total, may_grow: bool) -> bool:  # noqa: A001
    """tn_splat_bin: the frame's tile lists, the number of (Gaussian, tile) pairs into `total` (a c_int64).  False -- with `may_grow` only -- when
    the frame has more pairs than `cap`: the caller grows the workspace and redoes the frame.  Any other failure raises."""
    rc = _lib.load().tn_splat_bin(C.byref(cam), _raw(depths), N, _raw(ws), cap, C.byref(total), _stream())
    if rc != 0 and may_grow and total.value > cap:
        return False
    _lib.check(rc, "tn_splat_bin")
    return True


def raster_train(cam, N, ws, cap, bg4, aa, rgbt, depth, alpha, final_t, last, alpha_th=None, final_t_th=None, last_th=None) -> None:
    """tn_splat_raster_chains.  The training render: the eval render plus what the backward reads (`final_t`, `last`: final transmittance and last
    blended index per pixel); a separate-opacity frame adds the thermal chain's three (`alpha_th`, `final_t_th`, `last_th`)."""
    _call("tn_splat_raster_chains", C.byref(cam), N, _raw(ws), cap, bg4, aa, *_f32(rgbt=rgbt, depth=depth, alpha=alpha, alpha_thermal=alpha_th, transmittance=final_t),
          _ptr(last, I32, "last"), *_f32(transmittance_thermal=final_t_th), _ptr(last_th, I32, "last_thermal"))


def raster(cam, N, ws, cap, bg4, aa, rgbt, depth, alpha, alpha_th=None) -> None:
    """The eval render: tn_splat_raster, the short form (three images, shared opacity); with `alpha_th`, the thermal chain's accumulation of a
    separate-opacity frame, tn_splat_raster_chains without the backward's images."""
    if alpha_th is None:
        _call("tn_splat_raster", C.byref(cam), N, _raw(ws), cap, bg4, aa, *_f32(rgbt=rgbt, depth=depth, alpha=alpha))
    else:
        _call("tn_splat_raster_chains", C.byref(cam), N, _raw(ws), cap, bg4, aa, *_f32(rgbt=rgbt, depth=depth, alpha=alpha, alpha_thermal=alpha_th), None, None, None, None)


def raster_removal(cam, N, ws, cap, bg4, thr, rem) -> None:
    """tn_splat_raster_removal_sep: the removal renders [H,W,4], one more walk over the frame's tile lists (separate mode only)."""
    _call("tn_splat_raster_removal_sep", C.byref(cam), N, _raw(ws), cap, bg4, float(thr), *_f32(removal=rem))


def raster_contrib(cam, N, ws, cap, aa, chain, pixel_weight, max_acc, sum_acc, hits_acc, views_acc) -> None:
    """tn_splat_raster_contrib over the projected and binned frame in `ws`: every Gaussian's ray contribution w = pixel_weight * alpha * T on
    `chain` (0: the RGB chain, 1: the thermal chain of a separate-mode frame) accumulated in place into max_acc [N] fp32, sum_acc [N] fp64,
    hits_acc [N] int64 and views_acc [N] int32.  pixel_weight: [H,W] fp32, non-negative, or None for 1.  The pair records' scratch is this call's."""
    if pixel_weight is not None and tuple(pixel_weight.shape) != (int(cam.height), int(cam.width)):
        raise ValueError(f"raster_contrib: pixel_weight must be [{int(cam.height)},{int(cam.width)}], got {tuple(pixel_weight.shape)}")
    for name, t in (("max_acc", max_acc), ("sum_acc", sum_acc), ("hits_acc", hits_acc), ("views_acc", views_acc)):
        if tuple(t.shape) != (N,):
            raise ValueError(f"raster_contrib: {name} must be [{N}], got {tuple(t.shape)}")
    scratch = workspace("tn_splat_contrib_workspace_bytes", N, cap, device=max_acc.device)
    _call("tn_splat_raster_contrib", C.byref(cam), N, _raw(ws), cap, int(aa), int(chain), _ptr(pixel_weight, F32, "pixel_weight"), _raw(scratch), scratch.numel(),
          _ptr(max_acc, F32, "max_acc"), _ptr(sum_acc, torch.float64, "sum_acc"), _ptr(hits_acc, torch.int64, "hits_acc"), _ptr(views_acc, I32, "views_acc"))


def raster_backward(cam, N, ws, cap, total, bg4, final_t, last, conics, v_rgbt, v_alpha, v_xys, v_conics, v_colors, v_lnop, final_t_th=None, last_th=None,
                    v_alpha_th=None, v_lnop_th=None, v_xys_abs=None, aa=0, depth=None, v_depth=None, v_depths=None) -> None:
    """tn_splat_raster_backward over the training frame's workspace `ws`.  Optional groups: the thermal chain's four tensors (`final_t_th`, `last_th`,
    `v_alpha_th`, `v_lnop_th`), `v_xys_abs` (absgrad), and the depth gradient -- `v_depth` (dL / d depth [H,W,1]) with `depth`, the forward's
    normalised image, and `v_depths` [N] to fill; `aa` is the frame's flag.  The backward's own workspace is this call's."""
    bws = workspace("tn_splat_backward_workspace_bytes", N, cap, int(final_t_th is not None), int(v_xys_abs is not None), int(v_depth is not None), device=v_xys.device)
    _call("tn_splat_raster_backward", C.byref(cam), N, _raw(ws), cap, total, bg4, int(aa), *_f32(transmittance=final_t), _ptr(last, I32, "last"),
          *_f32(transmittance_thermal=final_t_th), _ptr(last_th, I32, "last_thermal"), *_f32(conics=conics, v_rgbt=v_rgbt, v_alpha=v_alpha, v_alpha_thermal=v_alpha_th),
          _raw(bws), bws.numel(), *_f32(v_xys=v_xys, v_xys_abs=v_xys_abs, v_conics=v_conics, v_colors=v_colors, v_log_opacity=v_lnop, v_log_opacity_thermal=v_lnop_th,
                                        depth=depth, v_depth=v_depth, v_depths=v_depths))


def project_backward(cam, params, deg, aa, radii, v_xys, v_conics, v_colors, v_lnop, grads, v_lnop_th=None, pose_rec=None, pose=None, row=None,
                     g_pose=None, dview=None, v_depths=None) -> None:
    """tn_splat_project_backward: fills `grads` (laid out as `params`; nine of each and `v_lnop_th` with the separate thermal opacity).  With
    `pose_rec` the pose group: the kernel reads the corrected camera and row `row` of `pose` [C,6], adds dL/d pose into that row of `g_pose`
    through its finishing kernel and leaves dL/d view' in `dview` [3,4]; the partials' workspace is this call's own.  With `v_depths` (dL / d depths
    [N], what the depth raster backward left) the depth gradient."""
    N = params[0].shape[0]
    head, tail = [None, None], [None, 0, None, None]
    if pose_rec is not None:
        pws = workspace("tn_splat_pose_workspace_bytes", N, device=pose.device, what="bad Gaussian count")
        head = [_ptr(pose_rec, F32, "pose camera"), _pose_row_ptr(pose, row)]
        tail = [_raw(pws), pws.numel(), _pose_row_ptr(g_pose, row, "grad_pose"), *_f32(dview=dview)]
    _call("tn_splat_project_backward", C.byref(cam), *head, *_param_ptrs9(params), N, params[5].shape[1], deg, aa, _ptr(radii, I32, "radii"),
          *_f32(v_xys=v_xys, v_conics=v_conics, v_colors=v_colors, v_log_opacity=v_lnop, v_log_opacity_thermal=v_lnop_th, v_depths=v_depths),
          *_param_ptrs9(grads), *tail)


def pose_camera(cam, p00, p11, pose, row, rec) -> None:
    """tn_splat_pose_camera: the camera `cam` corrected by row `row` of `pose` [C,6] into the device record `rec` (one launch, the pose is never
    read on the host); p00 / p11 are the two intrinsic entries of the projection matrix."""
    _call("tn_splat_pose_camera", C.byref(cam), float(p00), float(p11), _pose_row_ptr(pose, row), _ptr(rec, F32, "pose camera"))


def crop_mask(crop, pts, mask) -> None:
    """tn_splat_crop_mask: uint8 `mask` [n] of which `pts` [n,3] are strictly inside the box -- the device function the cropped projection uses."""
    _call("tn_splat_crop_mask", C.byref(crop), *_f32(pts=pts), pts.shape[0], _raw(mask))


def transform_call(transform, means, scales, quats, rest, rest_thermal, means_out, scales_out, quats_out, rest_out, rest_thermal_out) -> None:
    """tn_transform_splat: the similarity of the TnSplatTransform `transform` applied to means, scales [N,3], quats [N,4], features_rest [N,R,3] and
    features_rest_thermal [N,R,1] into the five outputs.  An output may be its own input (in place); otherwise it must overlap no other tensor of the
    call.  R must be 0, 3, 8 or 15; with R == 0 the rest tensors go in as null."""
    N, R = means.shape[0], rest.shape[1]
    for name, t, o, shape in (("means", means, means_out, (N, 3)), ("scales", scales, scales_out, (N, 3)), ("quats", quats, quats_out, (N, 4)),
                              ("features_rest", rest, rest_out, (N, R, 3)), ("features_rest_thermal", rest_thermal, rest_thermal_out, (N, R, 1))):
        if tuple(t.shape) != shape or tuple(o.shape) != shape:
            raise ValueError(f"transform_call: {name} and its output must be {shape}, got {tuple(t.shape)} and {tuple(o.shape)}")
    geo = _f32(means=means, scales=scales, quats=quats), _f32(means_out=means_out, scales_out=scales_out, quats_out=quats_out)
    sh = ([None, None], [None, None]) if R == 0 else (_f32(features_rest=rest, features_rest_thermal=rest_thermal),
                                                    _f32(features_rest_out=rest_out, features_rest_thermal_out=rest_thermal_out))
    _call("tn_transform_splat", C.byref(transform), *geo[0], *sh[0], N, R, *geo[1], *sh[1])


FILTER_CAMERA_FLOATS = 18  # a row of the 3D filter's camera table: viewmat 12 | fx fy cx cy | width height


def filter3d_compute(means, camera_table, near: float, variance: float, out) -> None:
    """tn_filter3d_splat_compute: Mip-Splatting's 3D filter value of every Gaussian, `out` [N], from means [N,3] and the camera table
    [C,18] (splat_filter.filter_camera_table).  Two launches, no read-back; the partial minima's workspace is this call's own."""
    N, Cn = means.shape[0], camera_table.shape[0]
    if tuple(means.shape) != (N, 3) or tuple(camera_table.shape) != (Cn, FILTER_CAMERA_FLOATS) or tuple(out.shape) != (N,):
        raise ValueError(f"filter3d_compute: means [N,3], a camera table [C,{FILTER_CAMERA_FLOATS}] and out [N] expected, got {tuple(means.shape)}, "
                         f"{tuple(camera_table.shape)} and {tuple(out.shape)}")
    ws = workspace("tn_filter3d_splat_workspace_bytes", N, device=means.device, what="bad Gaussian count")
    _call("tn_filter3d_splat_compute", *_f32(means=means), N, *_f32(camera_table=camera_table if Cn else None), Cn, float(near), float(variance),
          *_f32(filter_3D=out), _raw(ws), ws.numel())


def filter3d_apply(scales, opacities, filter_3d, scales_out, opacities_out, opacities_thermal=None, opacities_thermal_out=None) -> None:
    """tn_filter3d_splat_apply: the filtered log-scales [N,3] and opacity logits [N,1] (and thermal logits, where given) of one launch."""
    N = scales.shape[0]
    th = [None, None] if opacities_thermal is None else _f32(opacities_thermal=opacities_thermal.reshape(-1),
                                                              opacities_thermal_out=opacities_thermal_out.reshape(-1))
    _call("tn_filter3d_splat_apply", *_f32(scales=scales, opacities=opacities.reshape(-1)), th[0], *_f32(filter_3D=filter_3d), N,
          *_f32(scales_out=scales_out, opacities_out=opacities_out.reshape(-1)), th[1])


def filter3d_apply_backward(scales, opacities, filter_3d, v_scales_out, v_opacities_out, v_scales, v_opacities, opacities_thermal=None,
                            v_opacities_thermal_out=None, v_opacities_thermal=None) -> None:
    """tn_filter3d_splat_apply_backward: dL/d raw log-scales and logits from the gradients of the filtered ones, one launch."""
    N = scales.shape[0]
    th = [None, None, None] if opacities_thermal is None else _f32(opacities_thermal=opacities_thermal.reshape(-1),
                                                                    v_opacities_thermal_out=v_opacities_thermal_out.reshape(-1),
                                                                    v_opacities_thermal=v_opacities_thermal.reshape(-1))
    _call("tn_filter3d_splat_apply_backward", *_f32(scales=scales, opacities=opacities.reshape(-1)), th[0], *_f32(filter_3D=filter_3d),
          *_f32(v_scales_out=v_scales_out, v_opacities_out=v_opacities_out.reshape(-1)), th[1], N,
          *_f32(v_scales=v_scales, v_opacities=v_opacities.reshape(-1)), th[2])


# ---------------------------------------------------------------------------------------------------- refinement
def grad_stats(xys_grad, radii, N, max_size, first, grad_norm_sum, vis_counts, max_2d_size) -> None:
    """tn_splat_grad_stats: accumulate (first: start) the refinement statistics of one training frame."""
    _call("tn_splat_grad_stats", *_f32(xys_grad=xys_grad), _ptr(radii, I32, "radii"), N, max_size, int(first),
          *_f32(grad_norm_sum=grad_norm_sum, vis_counts=vis_counts, max_2d_size=max_2d_size))


def refine_plan(rs, step, scales, opacities, stats, N, S, counts, opacities_thermal=None) -> Tensor:
    """tn_splat_refine_plan (the both-below cull rule with `opacities_thermal`): classify every Gaussian from `stats` = (grad_norm_sum, vis_counts, max_2d_size) and
    leave (n_split, n_orig, n_child, n_dup) in `counts`, a host (c_int64 * 4): one host synchronisation.  Returns the workspace with the plan for
    S split samples, which refine_apply reads."""
    ws = workspace("tn_splat_refine_workspace_bytes", N, S, device=scales.device)
    _call("tn_splat_refine_plan", C.byref(rs), int(step), *_f32(scales=scales, opacities=opacities.reshape(-1)),
          *_f32(opacities_thermal=None if opacities_thermal is None else opacities_thermal.reshape(-1)),
          *_f32(grad_norm_sum=stats[0], vis_counts=stats[1], max_2d_size=stats[2]), N, _raw(ws), ws.numel(), counts)
    return ws


def refine_apply(rs, N, K, ws, counts, noise, old, exp_avg, exp_avg_sq, new, new_exp_avg, new_exp_avg_sq) -> None:
    """tn_splat_refine_apply (eight or nine tensors per list): gather / split / duplicate `old` and its Adam moments into `new` and theirs by the
    plan in `ws`.  Each list holds a tensor or None per parameter; None and empty tensors go in as null."""
    arr = lambda ts: (C.c_void_p * len(old))(*[t.data_ptr() if t is not None and t.numel() else None for t in ts])  # noqa: E731
    _call("tn_splat_refine_apply", C.byref(rs), N, K, _raw(ws), ws.numel(), counts,
          *_f32(noise=noise if noise is not None and noise.numel() else None), len(old), arr(old), arr(exp_avg), arr(exp_avg_sq), arr(new), arr(new_exp_avg),
          arr(new_exp_avg_sq))


def mcmc_relocate(params: List[Tensor], exp_avg: List[Optional[Tensor]], exp_avg_sq: List[Optional[Tensor]], src_idx: Tensor, dst_idx: Tensor,
                  min_opacity: float) -> None:
    """tn_splat_mcmc_relocate in place on the current stream, without a host synchronisation.  params: the 8 (9: separate thermal opacity)
    gauss_params tensors in param_names order, contiguous fp32 on the device, all with the same number of rows; exp_avg / exp_avg_sq: per tensor
    its Adam moments or None (both); src_idx / dst_idx: int64 [M] on the device.  Row dst_idx[j] becomes a copy of row src_idx[j] with gsplat's
    relocation opacity and scale (ratio = 1 + how often the source was drawn, capped at 51; evaluated in double), every drawn source takes that
    opacity and scale once and loses its moments; destination moments and every row not named stay.  No destination may be a source or repeat."""
    if len(params) not in (8, 9):
        raise ValueError(f"mcmc_relocate takes the 8 or 9 gauss_params tensors, got {len(params)}")
    if len(exp_avg) != len(params) or len(exp_avg_sq) != len(params):
        raise ValueError("mcmc_relocate: one exp_avg and one exp_avg_sq entry (a tensor or None) per parameter")
    rows, K = params[0].shape[0], params[5].shape[1]
    for t, m1, m2, n in zip(params, exp_avg, exp_avg_sq, _PARAM_NAMES_SEP):
        if t.shape[0] != rows:
            raise ValueError(f"mcmc_relocate: {n} has {t.shape[0]} rows, means {rows}")
        if (m1 is None) != (m2 is None) or (m1 is not None and (m1.shape != t.shape or m2.shape != t.shape)):
            raise ValueError(f"mcmc_relocate: the moments of {n} must both be None or both have its shape")
    if src_idx.shape != dst_idx.shape or src_idx.dim() != 1:
        raise ValueError(f"mcmc_relocate: src_idx and dst_idx must be [M], got {tuple(src_idx.shape)} and {tuple(dst_idx.shape)}")
    M = src_idx.shape[0]
    if M == 0:
        return
    pp = _param_ptrs(params)  # checks device, dtype and contiguity; the two features_rest entries are null without higher-order coefficients

    def arr(ts, what):  # a HOST array of device pointers; an entry is null where the tensor is None or the parameter itself is
        return (C.c_void_p * len(params))(*[_ptr(t, F32, what).value if t is not None and p is not None else None for t, p in zip(ts, pp)])

    ws = workspace("tn_splat_mcmc_workspace_bytes", rows, M, device=params[0].device)
    _call("tn_splat_mcmc_relocate", rows, K, _ptr(src_idx, torch.int64, "src_idx"), _ptr(dst_idx, torch.int64, "dst_idx"), M,
          float(min_opacity), len(params), arr(params, "params"), arr(exp_avg, "exp_avg"), arr(exp_avg_sq, "exp_avg_sq"), _raw(ws), ws.numel())


def mcmc_noise(means: Tensor, scales: Tensor, quats: Tensor, opacities: Tensor, randn: Tensor, scaler: float,
               opacities_thermal: Optional[Tensor] = None) -> None:
    """tn_splat_mcmc_noise: means [N,3] += Sigma (randn * g * scaler) in place, one launch on the current stream, fp32.  Sigma =
    R diag(exp(scales)^2) R^T with R the rotation of quats / |quats|; g = 1 / (1 + exp(-100 ((1 - o_vis) - 0.995))), o_vis = sigmoid(opacities)
    or, with opacities_thermal, the larger of the two sigmoids: a Gaussian anyone can see stays where it is.  Contiguous fp32 device tensors."""
    N, sep = means.shape[0], opacities_thermal is not None
    if means.shape != (N, 3) or scales.shape != (N, 3) or quats.shape != (N, 4) or randn.shape != (N, 3) or opacities.numel() != N or \
            (sep and opacities_thermal.numel() != N):
        raise ValueError("mcmc_noise: means, scales, randn [N,3], quats [N,4], opacities [N,1] of one N expected")
    _call("tn_splat_mcmc_noise", *_f32(means=means, scales=scales, quats=quats, opacities=opacities.reshape(-1),
                                       opacities_thermal=opacities_thermal.reshape(-1) if sep else None, randn=randn), N, float(scaler))


# ---------------------------------------------------------------------------------------------------- seeding and the image kernels
def knn(points, n, k, dist, idx) -> None:
    """tn_knn: distances [n,k] fp32 (and, with `idx`, neighbour indices [n,k] int32) of every point to its k nearest OTHER points."""
    ws = workspace("tn_knn_workspace_bytes", n, k, device=points.device, what=f"({n}, {k}) failed")
    _call("tn_knn", *_f32(points=points), n, k, *_f32(distances=dist), _ptr(idx, I32, "indices"), _raw(ws), ws.numel())


def knn_distances(points: Tensor, k: int = 3, return_index: bool = False):
    """Exact k-nearest-neighbour distances of every point to the OTHER points (k_nearest_sklearn, splatfacto.py:272-290: NearestNeighbors(k + 1)
    over the cloud, the point itself dropped) in one tn_knn call on the current stream.  points: contiguous [N,3] fp32 on the device ->
    distances [N,k] fp32, ascending (and neighbour indices [N,k] int64 with return_index).  d = sqrtf((dx*dx + dy*dy) + dz*dz) in fp32, ties go
    to the smaller index: bit-identical to a brute force with that formula, and deterministic.  Raises ValueError for non-finite points (one
    host synchronisation) and for N < k + 1."""
    if not isinstance(points, Tensor) or not points.is_cuda or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("knn_distances takes an [N,3] float32 HIP tensor (the splat path has no CPU fallback)")
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"knn_distances: k = {k}, tn_knn supports 1..{KNN_MAX_K}")
    n = points.shape[0]
    if n < k + 1:
        raise ValueError(f"knn_distances: {n} points, k = {k} needs at least k + 1")
    pts = points.contiguous()
    if not bool(torch.isfinite(pts).all()):
        raise ValueError("knn_distances: the points must be finite")
    dist = torch.empty((n, k), device=pts.device)
    idx = torch.empty((n, k), dtype=torch.int32, device=pts.device) if return_index else None
    knn(pts, n, k, dist, idx)
    return (dist, idx.long()) if return_index else dist


def image_loss_call(pred, ps, gt, gs, H, W, Cc, ssim_lambda, weight, out, grad) -> None:
    """tn_image_loss: [weight * main loss, L1, SSIM] into `out` [3] and, with `grad`, d main / d pred; ps / gs are the pixel strides."""
    ws = workspace("tn_image_loss_workspace_bytes", H, W, Cc, device=pred.device, what=f"bad sizes {H} x {W} x {Cc}", exc=ValueError)
    _call("tn_image_loss", _raw(pred), ps, _raw(gt), gs, H, W, Cc, float(ssim_lambda), float(weight), _raw(ws), ws.numel(), _raw(out), _raw(grad))


def thermal_reg(pred, ps, gt, gs, H, W, tv_mult, cross_mult, out, grad) -> None:
    """tn_thermal_reg: (tv_mult * tv, cross_mult * cc) into `out` [2] and, with `grad`, the gradient of their sum in pred."""
    ws = workspace("tn_thermal_reg_workspace_bytes", H, W, device=pred.device, what=f"bad sizes {H} x {W}", exc=ValueError)
    _call("tn_thermal_reg", _raw(pred), ps, _raw(gt), gs, H, W, float(tv_mult), float(cross_mult), _raw(ws), ws.numel(), _raw(out), _raw(grad))


def depth_loss(depth, alpha, depth_image, H, W, depth_mult, tv_mult, out, grad) -> None:
    """tn_depth_loss: (depth_mult * depth_loss, tv_mult * depth_tv_loss) into `out` [2] and, with `grad`, the gradient of their sum in depth;
    `depth_image` (the sensor depth) may be None."""
    ws = workspace("tn_depth_loss_workspace_bytes", H, W, device=depth.device, what=f"bad sizes {H} x {W}", exc=ValueError)
    _call("tn_depth_loss", *_f32(depth=depth, accumulation=alpha, depth_image=depth_image), H, W, float(depth_mult), float(tv_mult), _raw(ws), ws.numel(),
          _raw(out), _raw(grad))


def _image_code(t) -> int:
    return _lib.TN_IMAGE_U8 if t.dtype == torch.uint8 else _lib.TN_IMAGE_F32


def image_resize(image, ps, out) -> None:
    """tn_image_resize of an [H,W,C] uint8 or fp32 image with pixel stride ps into `out` [h,w,C] fp32."""
    _call("tn_image_resize", _raw(image), _image_code(image), ps, *image.shape, _raw(out), out.shape[0], out.shape[1])


def image_undistort(image, ps, out, p) -> None:
    """tn_image_undistort of an [H,W,C] uint8 or fp32 image with pixel stride ps into `out` [H,W,C] (uint8 or fp32) by the TnUndistort `p`."""
    _call("tn_image_undistort", _raw(image), _image_code(image), ps, *image.shape, _raw(out), _image_code(out), C.byref(p))


# ---------------------------------------------------------------------------------------------------- bilateral grids
BILAGRID_MAX_SIDE = 256  # every side of a bilateral grid is 2..256 (tn_bilagrid_*)


def _bilagrid_sizes(grids: Tensor, what: str) -> Tuple[int, int, int, int, int]:
    """(F, K, L, GH, GW) of a grids tensor [F,K,L,GH,GW]; a ValueError for another shape or a side outside 2..BILAGRID_MAX_SIDE."""
    if grids.dim() != 5:
        raise ValueError(f"{what}: grids must be [F, K, L, GH, GW], got {tuple(grids.shape)}")
    F, K, L, GH, GW = (int(v) for v in grids.shape)
    if F < 1 or not all(2 <= v <= BILAGRID_MAX_SIDE for v in (L, GH, GW)):
        raise ValueError(f"{what}: {F} grids of {GW} x {GH} x {L}, every side must be in 2..{BILAGRID_MAX_SIDE}")
    return F, K, L, GH, GW


def bilagrid_slice(grids, row, image, ps, out) -> None:
    """tn_bilagrid_slice: row `row` of `grids` [F,C(C+1),L,GH,GW] applied to `image` [H,W,C] (pixel stride ps) into `out` [H,W,C]."""
    F, K, L, GH, GW = _bilagrid_sizes(grids, "bilagrid_slice")
    H, W, Cc = image.shape
    _call("tn_bilagrid_slice", *_f32(grids=grids), F, int(row), Cc, GW, GH, L, _raw(image), ps, H, W, *_f32(out=out))


def bilagrid_slice_backward(grids, row, image, ps, v_out, v_image, v_grid) -> None:
    """tn_bilagrid_slice_backward: `v_image` [H,W,C] and `v_grid` [K,L,GH,GW], the whole gradient of row `row`; the workspace is this call's."""
    F, K, L, GH, GW = _bilagrid_sizes(grids, "bilagrid_slice_backward")
    H, W, Cc = image.shape
    ws = workspace("tn_bilagrid_workspace_bytes", Cc, GW, GH, L, H, W, device=grids.device, what=f"bad sizes {H} x {W} x {Cc}, grid {GW} x {GH} x {L}",
                   exc=ValueError)
    _call("tn_bilagrid_slice_backward", *_f32(grids=grids), F, int(row), Cc, GW, GH, L, _raw(image), ps, H, W, *_f32(v_out=v_out), _raw(ws), ws.numel(),
          *_f32(v_image=v_image, v_grid=v_grid))


def bilagrid_tv(grids, mult, out, grad) -> None:
    """tn_bilagrid_tv: mult * total variation of `grids` [F,K,L,GH,GW] into `out` [1] and, with `grad`, its gradient in the same call."""
    F, K, L, GH, GW = _bilagrid_sizes(grids, "bilagrid_tv")
    ws = workspace("tn_bilagrid_tv_workspace_bytes", F, K, GW, GH, L, device=grids.device, what=f"bad sizes {F} x {K} x {L} x {GH} x {GW}", exc=ValueError)
    _call("tn_bilagrid_tv", *_f32(grids=grids), F, K, GW, GH, L, float(mult), _raw(ws), ws.numel(), *_f32(out=out, grad=grad))
