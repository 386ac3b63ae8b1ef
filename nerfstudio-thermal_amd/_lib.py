"""ctypes binding of libthermal_nerf_hip.so (the C ABI declared in include/thermal_nerf_hip.h).

There is deliberately no fallback: if the HIP library is missing the first op raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# TN_LIB names another build of the same library (A/B timing of kernel variants); there is still no fallback if it cannot be loaded
LIB_PATH = os.path.abspath(os.environ["TN_LIB"]) if os.environ.get("TN_LIB") else os.path.join(_HERE, "libthermal_nerf_hip.so")
ABI_VERSION = 314  # include/thermal_nerf_hip.h as this binding was written for (tn_version() of the library must match)
TN_MAX_LEVELS = 16
TN_MAX_SAMPLES = 256
TN_RENDER_SCRATCH_FLOATS = 4096
TN_LOSS_LINES = 64
TN_RENDER_TRAIN_OFFSETS = 25
TN_SPLAT_POSE_CAMERA_FLOATS = 40  # the corrected-camera record of tn_splat_pose_camera
TN_IMAGE_F32, TN_IMAGE_U8 = 0, 1  # tn_image_resize's input types, tn_image_undistort's input and output types
TN_FRAME_MAX_PANELS = 8  # tn_frame_compose
TN_FRAME_MINMAX_WORKSPACE_BYTES = 2048  # tn_frame_minmax
TN_FRAME_NORMALIZE, TN_FRAME_INVERT, TN_FRAME_DEPTH, TN_FRAME_NEAR, TN_FRAME_FAR = 1, 2, 4, 8, 16  # TnFramePanel.flags
TN_BWD_MLP, TN_BWD_SCATTER, TN_BWD_JOIN, TN_BWD_SCATTER_BIN, TN_BWD_SCATTER_FOLD, TN_BWD_FORK_DPOS, TN_BWD_COUNTERS_CLEAN = 1, 2, 4, 8, 16, 32, 64

_p = C.c_void_p
_i32 = C.c_int32
_i64 = C.c_int64
_f = C.c_float
_d = C.c_double


class TnGrid(C.Structure):
    _fields_ = [
        ("table", _p),
        ("table_grad", _p),
        ("num_levels", _i32),
        ("log2_hashmap_size", _i32),
        ("res", _f * TN_MAX_LEVELS),
        ("nonfinite_flag", _p),
        ("table_grad_is_zero", _i32),
    ]


class TnPropNet(C.Structure):
    _fields_ = [("grid", TnGrid)] + [(n, _p) for n in ("w0", "b0", "w1", "b1", "gw0", "gb0", "gw1", "gb1")]


_FIELD_PTRS = ("w0", "b0", "w1", "b1", "hw0", "hb0", "hw1", "hb1", "hw2", "hb2", "emb",
               "gw0", "gb0", "gw1", "gb1", "ghw0", "ghb0", "ghw1", "ghb1", "ghw2", "ghb2", "gemb")


class TnField(C.Structure):
    _fields_ = [("grid", TnGrid)] + [(n, _p) for n in _FIELD_PTRS] + [("num_channels", _i32), ("num_images", _i32)]


TN_TRAIN_STEP_MAX_RANGES = 8
_R = TN_TRAIN_STEP_MAX_RANGES


class TnSampleRays(C.Structure):
    """include/thermal_nerf_hip.h: the arguments of tn_sample_rays as a block (TnTrainStep.next_sample)"""
    _fields_ = [("images", _p), ("image_offsets", _p), ("heights", _p), ("widths", _p), ("is_thermal", _p), ("image_idx", _p), ("num_images", _i32),
                ("u", _p), ("num_rays", _i64), ("patch_size", _i32), ("ray_indices", _p), ("image", _p), ("is_thermal_out", _p), ("camera_indices", _p),
                ("c2w", _p), ("fx", _p), ("fy", _p), ("cx", _p), ("cy", _p), ("distortion", _p), ("num_cameras", _i32), ("origins", _p),
                ("directions", _p), ("pixel_area", _p), ("directions_norm", _p)]


class TnNextSampling(C.Structure):
    """include/thermal_nerf_hip.h: the NEXT iteration's sampling front as co-work of this iteration's optimiser launch (TnTrainStep.next_sampling)"""
    _fields_ = [("fwd_out", _p), ("jitter0", _p), ("jitter1", _p), ("jitter2", _p), ("anneal", _f), ("prop_grad", _i32)]


class TnTrainStep(C.Structure):
    """The argument block of tn_train_step: field for field the struct of include/thermal_nerf_hip.h (tests/test_abi_cpu.py compares the two)."""
    _fields_ = [
        ("prop0", C.POINTER(TnPropNet)), ("prop1", C.POINTER(TnPropNet)), ("field", C.POINTER(TnField)),
        ("origins_in", _p), ("directions_in", _p), ("camera_indices", _p), ("image", _p), ("is_thermal", _p), ("nears", _p), ("fars", _p),
        ("N", _i64), ("S0", _i32), ("S1", _i32), ("S2", _i32),
        ("pose_adjustment", _p), ("frozen", _p), ("num_cameras", _i32), ("grad_pose", _p),
        ("trans_pen", _f), ("rot_pen", _f), ("pen_scale", _f),
        ("anneal", _f), ("prop_grad", _i32),
        ("jitter0", _p), ("jitter1", _p), ("jitter2", _p), ("lin_spaced0", _p), ("lin_pdf1", _p), ("lin_pdf2", _p),
        ("field_workspace", _p), ("field_workspace_bytes", _i64),
        ("prop_workspace0", _p), ("prop_workspace_bytes0", _i64), ("prop_workspace1", _p), ("prop_workspace_bytes1", _i64),
        ("fwd_out", _p), ("bwd_tmp", _p), ("acc", _p), ("acc_bytes", _i64),
        ("losses16", _p), ("loss_lines", _p), ("d_comp", _p), ("d_weights0", _p), ("d_weights1", _p), ("d_weights2", _p), ("d_origins", _p),
        ("d_directions", _p),
        ("thermal_mult", _f), ("tv_mult", _f), ("cross_mult", _f), ("distortion_mult", _f), ("interlevel_mult", _f),
        ("num_check", _i32), ("check_offsets", _i64 * _R), ("check_counts", _i64 * _R), ("check_flags", _i32 * _R), ("pose_flag", _i32),
        ("params", _p), ("grads", _p), ("exp_avg", _p), ("exp_avg_sq", _p),
        ("num_ranges", _i32), ("offsets", _i64 * _R), ("counts", _i64 * _R), ("steps", _i32 * _R),
        ("lrs", _d * _R), ("lr_finals", _d * _R), ("sched_max_steps", _i32 * _R), ("flag_index", _i32 * _R), ("sched_step", _i32),
        ("beta1", _d), ("beta2", _d), ("eps", _d),
        ("found_inf", _p), ("num_flags", _i32), ("skipped", _p), ("lag_index", _i32),
        ("scale", _p), ("growth_tracker", _p), ("done_counter", _p), ("growth_factor", _d), ("backoff_factor", _d), ("growth_interval", _i32),
        ("next_sample", C.POINTER(TnSampleRays)), ("next_sample_taken", C.POINTER(_i32)),
        ("next_sampling", C.POINTER(TnNextSampling)), ("next_sampling_taken", C.POINTER(_i32)), ("sampling_done", _i32),
    ]


class TnSplatCamera(C.Structure):
    _fields_ = [("viewmat", _f * 12), ("projmat", _f * 16), ("fx", _f), ("fy", _f), ("cx", _f), ("cy", _f), ("position", _f * 3),
                ("clip_thresh", _f), ("width", _i32), ("height", _i32)]


class TnSplatRefine(C.Structure):
    """include/thermal_nerf_hip.h: the thresholds and step rules of one refinement (tn_splat_refine_plan / tn_splat_refine_apply)"""
    _fields_ = [("cull_alpha_thresh", _f), ("cull_scale_thresh", _f), ("densify_grad_thresh", _f), ("densify_size_thresh", _f), ("cull_screen_size", _f),
                ("split_screen_size", _f), ("refine_every", _i32), ("reset_alpha_every", _i32), ("stop_screen_size_at", _i32), ("stop_split_at", _i32),
                ("n_split_samples", _i32), ("continue_cull_post_densification", _i32), ("num_train_data", _i32), ("max_size", _i32)]


class TnSplatCrop(C.Structure):
    """include/thermal_nerf_hip.h: the crop box of the eval render, rows of the 3x4 world -> box matrix and S / 2 (tn_splat_project, tn_splat_crop_mask)"""
    _fields_ = [("world_to_box", _f * 12), ("half_extent", _f * 3)]


class TnSplatTransform(C.Structure):
    """include/thermal_nerf_hip.h: a similarity of the Gaussians -- A = s R, t, log s, the quaternion of R and its three SH band matrices, row-major doubles (tn_transform_splat)"""
    _fields_ = [("A", _d * 9), ("t", _d * 3), ("log_scale", _d), ("q", _d * 4), ("sh1", _d * 9), ("sh2", _d * 25), ("sh3", _d * 49)]


class TnUndistort(C.Structure):
    """include/thermal_nerf_hip.h: the source camera, the pinhole camera of the output and k1 k2 k3 k4 p1 p2 (tn_image_undistort)"""
    _fields_ = [("fx", _f), ("fy", _f), ("cx", _f), ("cy", _f), ("new_fx", _f), ("new_fy", _f), ("new_cx", _f), ("new_cy", _f), ("k", _f * 6)]


class TnFramePanel(C.Structure):
    """include/thermal_nerf_hip.h: one panel of a frame (tn_frame_compose, tn_frame_colors)"""
    _fields_ = [("src", _p), ("accumulation", _p), ("minmax", _p), ("table", _p), ("near_plane", _d), ("far_plane", _d), ("colormap_min", _d),
                ("colormap_max", _d), ("channels", _i32), ("flags", _i32)]


# name -> (restype, argtypes); must list every symbol include/thermal_nerf_hip.h declares
SIGNATURES = {
    "tn_last_error": (C.c_char_p, []),
    "tn_version": (C.c_int, []),
    "tn_field_workspace_bytes": (_i64, [_i64, _i32]),
    "tn_field_encode_plan": (_i32, [_p, _i64, _p]),
    "tn_prop_workspace_bytes": (_i64, [_i64]),
    "tn_sample_pixels": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _p, _i64, _i32, _p, _p, _p, _p, _p]),
    "tn_raygen": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i32, _i64, _p, _p, _p, _p, _p]),
    "tn_sample_rays": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _p, _i64, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _p, _p, _p]),
    "tn_pose_spaced_bins": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i32, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _p]),
    "tn_pose_bwd_finish": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _p, _p, _p, _f, _f, _f, _p, _p]),
    "tn_pose_bwd_finish_check": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _p, _p, _p, _f, _f, _f, _p, _p, _i32, _p, _p, _p, _i32, _p, _i32, _p]),
    "tn_pose_apply_fwd": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i32, _p, _p, _p]),
    "tn_pose_apply_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _p, _p]),
    # shared (rig) pose correction: one row for every camera of a spectrum
    "tn_pose_shared_apply": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i32, _p, _p, _p]),
    "tn_pose_shared_bwd_workspace_bytes": (_i64, [_i64]),
    "tn_pose_shared_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i64, _i32, _p, _i64, _p, _p]),
    "tn_spaced_bins": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _p, _p, _p]),
    "tn_prop_density_fwd": (C.c_int, [C.POINTER(TnPropNet), _p, _p, _p, _i64, _i32, _p, _p]),
    "tn_prop_density_bwd": (C.c_int, [C.POINTER(TnPropNet), _p, _p, _p, _p, _i64, _i32, _p, _i64, _p, _p, _p]),
    "tn_hash_scatter_workspace_bytes": (_i64, [_i64, _i32]),
    "tn_hash_scatter": (C.c_int, [C.POINTER(TnGrid), _p, _p, _p, _p, _i32, _i64, _i32, _p, _p, _p, _i64, _p]),
    "tn_weights_fwd": (C.c_int, [_p, _p, _i64, _i32, _p, _p, _p]),
    "tn_weights_bwd": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _p, _p]),
    "tn_weights_resample": (C.c_int, [_p, _p, _p, _i32, _f, _p, _p, _p, _p, _i64, _i32, _p, _p, _p, _p, _p]),
    "tn_pdf_resample": (C.c_int, [_p, _p, _i32, _f, _p, _p, _p, _p, _i64, _i32, _p, _p, _p]),
    "tn_field_pack_weights": (C.c_int, [C.POINTER(TnField), _p, _p]),
    "tn_field_fwd": (C.c_int, [C.POINTER(TnField), _p, _p, _p, _p, _i64, _i32, _i32, _p, _i64, _p, _p, _p, _p]),
    "tn_field_bwd": (C.c_int, [C.POINTER(TnField), _p, _p, _p, _p, _p, _p, _i64, _i32, _p, _i64, _p, _p, _p]),
    "tn_field_bwd_phase": (C.c_int, [C.POINTER(TnField), _p, _p, _p, _p, _p, _p, _i64, _i32, _p, _i64, _p, _p, _i32, _i32, _i32, _p]),
    "tn_field_bwd_max_blocks": (_i32, [_i32]),
    "tn_field_dense_count": (_i64, [C.POINTER(TnField), _i64, _i32, _i32]),
    "tn_field_bwd_scatter_dense": (C.c_int, [C.POINTER(TnField), _p, _p, _p, _i64, _i32, _p, _i64, _p, _p, _i32, _i32, _p, _p]),
    "tn_field_dense_fold": (C.c_int, [C.POINTER(TnField), _i64, _i32, _i32, _p, _p]),
    "tn_field_density_fwd": (C.c_int, [C.POINTER(TnField), _p, _p, _p, _i64, _i32, _i32, _p, _i64, _p, _p]),
    "tn_minmax_init": (C.c_int, [_p, _p]),
    "tn_composite_fwd": (C.c_int, [_p, _p, _p, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p]),
    "tn_clip_depth": (C.c_int, [_p, _p, _i64, _p]),
    "tn_composite_bwd": (C.c_int, [_p, _p, _p, _i64, _i32, _i32, _p, _p, _p]),
    "tn_render_rays_eval_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32, _i32]),
    "tn_render_rays_eval": (C.c_int, [C.POINTER(TnPropNet), C.POINTER(TnPropNet), C.POINTER(TnField), _p, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _f,
                                      _p, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "tn_render_rays_train_layout": (C.c_int, [_i64, _i32, _i32, _i32, _i32, _p, _i32]),
    "tn_render_rays_train": (C.c_int, [C.POINTER(TnPropNet), C.POINTER(TnPropNet), C.POINTER(TnField), _p, _p, _i32, _p, _p, _p, _p, _p, _i64, _i32, _i32,
                                       _i32, _f, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _i64, _i32, _p]),
    "tn_render_fwd": (C.c_int, [_p, _p, _p, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p]),
    "tn_render_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _p, _p, _p]),
    "tn_distortion_loss": (C.c_int, [_p, _p, _i64, _i32, _f, _p, _p, _p]),
    "tn_interlevel_loss": (C.c_int, [_p, _p, _i32, _p, _p, _i32, _i64, _f, _p, _p, _p]),
    "tn_proposal_losses": (C.c_int, [_p, _p, _i32, _i32, _p, _p, _p, _p, _i64, _f, _f, _p, _p, _p, _p]),
    "tn_pixel_losses": (C.c_int, [_p, _i32, _p, _i32, _p, _p, _i64, _f, _f, _f, _p, _p, _p, _p]),
    "tn_sample_rays_args": (C.c_int, [C.POINTER(TnSampleRays), _p]),
    "tn_render_losses_bwd": (C.c_int, [_p, _p, _p, _i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _p, _p, _f, _f, _p, _p, _p, _f, _f, _f, _p, _p, _p, _p,
                                       _i32, _p]),
    "tn_train_losses": (C.c_int, [_p, _p, _i32, _i32, _p, _p, _p, _p, _i64, _f, _f, _p, _p, _i32, _p, _i32, _p, _p, _f, _f, _f, _p, _p, _p, _p]),
    "tn_losses_finish": (C.c_int, [_p, _p, _p, _i32, _f, _f, _f, _p, _p, _p]),
    "tn_l1_loss": (C.c_int, [_p, _p, _i64, _f, _f, _p, _p, _p, _p]),
    "tn_camera_reg": (C.c_int, [_p, _i32, _f, _f, _f, _p, _p, _p]),
    "tn_train_metrics": (C.c_int, [_p, _i64, _f, _p, _i32, _p, _i32, _p, _p]),
    "tn_adam_step": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _d, _d, _d, _d, _p]),
    "tn_adam_step_ranges": (C.c_int, [_p, _p, _p, _p, _i32, _p, _p, _p, _p, _d, _d, _d, _p]),
    "tn_grad_nonfinite": (C.c_int, [_p, _i64, _p, _p]),
    "tn_adam_step_ranges_amp": (C.c_int, [_p, _p, _p, _p, _i32, _p, _p, _p, _p, _p, _p, _i32, _d, _d, _d, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _p]),
    "tn_grad_nonfinite_ranges": (C.c_int, [_p, _i32, _p, _p, _p, _i32, _p, _p]),
    "tn_grad_scaler_update": (C.c_int, [_p, _p, _p, _i32, _p, _d, _d, _i32, _i32, _p]),
    "tn_adam_step_ranges_amp_update": (C.c_int, [_p, _p, _p, _p, _i32, _p, _p, _p, _p, _p, _p, _i32, _d, _d, _d, _p, _p, _p, _i32, _p, _i32, _i32, _i32,
                                                 _p, _p, _p, _d, _d, _i32, _p]),
    "tn_fill_zero": (C.c_int, [_p, _i64, _p]),
    "tn_train_step": (C.c_int, [C.POINTER(TnTrainStep), _p]),
    "tn_shutdown": (C.c_int, []),
    "tn_comm_unique_id": (C.c_int, [_p]),
    "tn_comm_create": (C.c_int, [_p, _i32, _i32, C.POINTER(_p)]),
    "tn_comm_destroy": (C.c_int, [_p]),
    "tn_allreduce_grads": (C.c_int, [_p, _p, _i64, _i32, _p]),
    "tn_render_rays_train_bwd_tmp_floats": (_i64, [_i64, _i32, _i32, _i32, _i32]),
    "tn_render_rays_train_bwd": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _i32] + [_p] * 7 + [_i64, _p, _i64, _p, _i64] + [_p] * 3 + [_i32, _p]),
    "tn_splat_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    # the splat frame, its backward and refinement: one entry point per stage; optional inputs (pose camera, thermal opacity, crop box, absgrad,
    # depth gradient) are groups of nullable pointers
    "tn_splat_project": (C.c_int, [_p] * 11 + [_i64, _i32, _i32, _i32] + [_p] * 8 + [_i64, C.POINTER(TnSplatCrop), _p]),
    "tn_splat_bin": (C.c_int, [_p, _p, _i64, _p, _i64, _p, _p]),
    "tn_splat_raster": (C.c_int, [_p, _i64, _p, _i64, _p, _i32, _p, _p, _p, _p]),
    "tn_splat_raster_chains": (C.c_int, [_p, _i64, _p, _i64, _p, _i32] + [_p] * 8 + [_p]),
    "tn_splat_raster_removal_sep": (C.c_int, [_p, _i64, _p, _i64, _p, _f, _p, _p]),
    "tn_splat_backward_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32, _i32]),
    "tn_splat_raster_backward": (C.c_int, [_p, _i64, _p, _i64, _i64, _p, _i32] + [_p] * 9 + [_i64] + [_p] * 10),
    "tn_splat_project_backward": (C.c_int, [_p] * 12 + [_i64, _i32, _i32, _i32] + [_p] * 17 + [_i64, _p, _p, _p]),
    "tn_splat_grad_stats": (C.c_int, [_p, _p, _i64, _i32, _i32, _p, _p, _p, _p]),
    "tn_splat_refine_workspace_bytes": (_i64, [_i64, _i32]),
    "tn_splat_refine_plan": (C.c_int, [C.POINTER(TnSplatRefine), _i32] + [_p] * 6 + [_i64, _p, _i64, _p, _p]),
    "tn_splat_refine_apply": (C.c_int, [C.POINTER(TnSplatRefine), _i64, _i32, _p, _i64, _p, _p, _i32] + [_p] * 6 + [_p]),
    "tn_splat_crop_mask": (C.c_int, [C.POINTER(TnSplatCrop), _p, _i64, _p, _p]),
    "tn_splat_pose_camera": (C.c_int, [_p, _f, _f, _p, _p, _p]),
    "tn_splat_pose_workspace_bytes": (_i64, [_i64]),
    "tn_image_loss_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "tn_image_loss": (C.c_int, [_p, _i64, _p, _i64, _i32, _i32, _i32, _f, _f, _p, _i64, _p, _p, _p]),
    "tn_image_resize": (C.c_int, [_p, _i32, _i64, _i32, _i32, _i32, _p, _i32, _i32, _p]),
    "tn_image_undistort": (C.c_int, [_p, _i32, _i64, _i32, _i32, _i32, _p, _i32, C.POINTER(TnUndistort), _p]),
    "tn_thermal_reg_workspace_bytes": (_i64, [_i32, _i32]),
    "tn_thermal_reg": (C.c_int, [_p, _i64, _p, _i64, _i32, _i32, _f, _f, _p, _i64, _p, _p, _p]),
    "tn_depth_loss_workspace_bytes": (_i64, [_i32, _i32]),
    "tn_depth_loss": (C.c_int, [_p, _p, _p, _i32, _i32, _f, _f, _p, _i64, _p, _p, _p]),
    # bilateral grids: slice-and-apply of one frame's grid, its backward (image and the whole grid row), the grids' total variation
    "tn_bilagrid_workspace_bytes": (_i64, [_i32] * 6),
    "tn_bilagrid_slice": (C.c_int, [_p, _i32, _i32, _i32, _i32, _i32, _i32, _p, _i64, _i32, _i32, _p, _p]),
    "tn_bilagrid_slice_backward": (C.c_int, [_p, _i32, _i32, _i32, _i32, _i32, _i32, _p, _i64, _i32, _i32, _p, _p, _i64, _p, _p, _p]),
    "tn_bilagrid_tv_workspace_bytes": (_i64, [_i32] * 5),
    "tn_bilagrid_tv": (C.c_int, [_p, _i32, _i32, _i32, _i32, _i32, _f, _p, _i64, _p, _p, _p]),
    "tn_knn_workspace_bytes": (_i64, [_i64, _i32]),
    "tn_knn": (C.c_int, [_p, _i64, _i32, _p, _p, _p, _i64, _p]),
    # MCMC strategy: relocation / growth in place (8 or 9 tensors with their moments) and the per-step position noise
    "tn_splat_mcmc_workspace_bytes": (_i64, [_i64, _i64]),
    "tn_splat_mcmc_relocate": (C.c_int, [_i64, _i32, _p, _p, _i64, _f, _i32, _p, _p, _p, _p, _i64, _p]),
    "tn_splat_mcmc_noise": (C.c_int, [_p] * 6 + [_i64, _f, _p]),
    # Gaussian-splat PLY export: the parameters of tn_splat_project -> the kept Gaussians' file rows, compacted in order
    "tn_export_splat_workspace_bytes": (_i64, [_i64]),
    "tn_export_splat_pack": (C.c_int, [_p] * 9 + [_i64, _i32, _i32, _i32, _f, C.POINTER(TnSplatCrop), _p, _p, _p, _i64, _p]),
    # a similarity applied to every Gaussian (means, log scales, quaternions and the SH bands 1 to 3 of both spectra), in place or not
    "tn_transform_splat": (C.c_int, [C.POINTER(TnSplatTransform)] + [_p] * 5 + [_i64, _i32] + [_p] * 5 + [_p]),
    # Mip-Splatting's 3D smoothing filter: the filter value per Gaussian from the training cameras, its application to log-scales and opacity
    # logits (a NULL thermal pointer group is shared mode) and the closed-form backward
    "tn_filter3d_splat_workspace_bytes": (_i64, [_i64]),
    "tn_filter3d_splat_compute": (C.c_int, [_p, _i64, _p, _i32, _d, _d, _p, _p, _i64, _p]),
    "tn_filter3d_splat_apply": (C.c_int, [_p] * 4 + [_i64] + [_p] * 3 + [_p]),
    "tn_filter3d_splat_apply_backward": (C.c_int, [_p] * 7 + [_i64] + [_p] * 3 + [_p]),
    # ray contribution of every Gaussian on one chain of a projected and binned frame, accumulated in place: max fp32, sum fp64, hits int64,
    # views int32
    "tn_splat_contrib_workspace_bytes": (_i64, [_i64, _i64]),
    "tn_splat_raster_contrib": (C.c_int, [C.POINTER(TnSplatCamera), _i64, _p, _i64, _i32, _i32, _p, _p, _i64, _p, _p, _p, _p, _p]),
    # point-cloud export of the NeRF: stable append of a rendered batch, statistical outlier removal
    "tn_cloud_append_workspace_bytes": (_i64, [_i64]),
    "tn_cloud_append": (C.c_int, [_p] * 5 + [_i64, _p, _i64, _i64, _f, C.POINTER(TnSplatCrop), _p, _p, _p, _i64, _p, _p, _i64, _p]),
    "tn_cloud_remove_outliers_workspace_bytes": (_i64, [_i64, _i32]),
    "tn_cloud_remove_outliers": (C.c_int, [_p, _p, _p, _i64, _i32, C.c_double] + [_p] * 8 + [_i64, _p]),
    # the same two with the view directions carried beside the points, and the oriented normals of the cloud (a kNN PCA)
    "tn_cloud_append_view": (C.c_int, [_p] * 5 + [_i64, _p, _i64, _i64, _f, C.POINTER(TnSplatCrop), _p, _p, _p, _p, _i64, _p, _p, _i64, _p]),
    "tn_cloud_remove_outliers_view": (C.c_int, [_p, _p, _p, _p, _i64, _i32, C.c_double] + [_p] * 9 + [_i64, _p]),
    "tn_cloud_normals_workspace_bytes": (_i64, [_i64, _i32]),
    "tn_cloud_estimate_normals": (C.c_int, [_p, _i64, _i32, _p, _p, _p, _i64, _p]),
    "tn_tsdf_integrate": (C.c_int, [_p, _p, _p, _i32, _i32, _i32] + [_f] * 8 + [_p, _p, _p, _f, _p, _i32, _i32, _i32, _i32, _p]),
    "tn_mesh_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "tn_mesh_count": (C.c_int, [_p, _p, _i32, _i32, _i32, _i32, _p, _p, _i64, _p]),
    "tn_mesh_emit": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32] + [_f] * 6 + [_p, _p, _p, _i64, _p, _i64, _p, _i64, _p]),
    "tn_mesh_simplify_workspace_bytes": (_i64, [_i64, _i64]),
    "tn_mesh_simplify_count": (C.c_int, [_p, _i64, _p, _i64] + [_f] * 6 + [_i32] * 3 + [_p, _p, _i64, _p]),
    "tn_mesh_simplify_plan": (C.c_int, [_p, _i64, _p, _i64] + [_f] * 6 + [_i32] * 3 + [_p, _p, _i64, _p]),
    "tn_mesh_simplify_emit": (C.c_int, [_p, _p, _p, _i64, _p, _i64] + [_f] * 6 + [_i32] * 3 + [_f, _p, _p, _p, _i64, _p, _i64, _p, _i64, _p]),
    # Poisson reconstruction on a dense grid: the plan of a cloud, the gather splat, the trilinear sample, -div, the operator and the CG solve
    "tn_poisson_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "tn_poisson_bin": (C.c_int, [_p, _i64] + [_i32] * 3 + [_f] * 6 + [_p, _i64, _p]),
    "tn_poisson_splat": (C.c_int, [_p, _i64, _p, _i32, _p, _i32] + [_i32] * 3 + [_f] * 6 + [_p, _p, _i64, _p]),
    "tn_poisson_sample": (C.c_int, [_p, _i64, _p] + [_i32] * 3 + [_f] * 6 + [_p, _p]),
    "tn_poisson_divergence": (C.c_int, [_p] + [_i32] * 3 + [_f] * 3 + [_p, _p]),
    "tn_poisson_apply": (C.c_int, [_p, _p] + [_i32] * 3 + [_f] * 3 + [_p, _p]),
    "tn_poisson_solve_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "tn_poisson_solve": (C.c_int, [_p, _p, _p] + [_i32] * 3 + [_f] * 3 + [_d, _i32, _i32, C.POINTER(_d), _p, _i64, _p]),
    # texture baking: the atlas layout (host only), texture coordinates, per-texel rays and vertex colours over a texel range, the image store
    "tn_texture_layout": (C.c_int, [_i64, _i32, C.POINTER(_i64)]),
    "tn_texture_coords": (C.c_int, [_i64, _i32, _p, _p]),
    "tn_texture_rays": (C.c_int, [_p, _p, _i64, _p, _i64, _i32, _f, _i64, _i64, _p, _p, _p]),
    "tn_texture_vertex": (C.c_int, [_p, _i64, _p, _i64, _i32, _i64, _i64, _p, _p]),
    "tn_texture_store": (C.c_int, [_p, _i64, _p, _i64, _i64, _i64, _i64, _p, _p, _p, _p]),
    "tn_mesh_mean_edge_workspace_bytes": (_i64, [_i64]),
    "tn_mesh_mean_edge": (C.c_int, [_p, _i64, _p, _i64, _p, _p, _i64, _p]),
    "tn_frame_minmax": (C.c_int, [_p, _i64, _p, _p, _i64, _p]),
    "tn_frame_compose": (C.c_int, [C.POINTER(TnFramePanel), _i32, _i32, _i32, _p, _p]),
    "tn_frame_colors": (C.c_int, [C.POINTER(TnFramePanel), _i32, _i32, _p, _p]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load (once) and return the HIP library; raise loudly when it is not built."""
    global _lib
    if _lib is None:
        # torch bundles its own libamdhip64.so.7; /opt/rocm ships another with the SAME soname.  Whichever is loaded first serves the whole
        # process, and a process that ends up with ROCm's runtime under torch's HSA loses the device ("no ROCm-capable device").  Importing
        # torch first makes its runtime the one this library binds to, so kernels launched here and by torch share streams and memory.
        import torch  # noqa: F401

        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback for the thermal-nerfacto hot path."
            )
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if lib.tn_version() != ABI_VERSION:  # signatures are positional: a stale build would take a workspace pointer for a flag
            raise RuntimeError(f"{LIB_PATH} reports ABI version {lib.tn_version()}, this binding needs {ABI_VERSION}: rebuild it (__graft_entry__.build())")
        _lib = lib
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().tn_last_error()
        raise RuntimeError(f"libthermal_nerf_hip {what} failed (code {rc}): {msg.decode() if msg else ''}")
