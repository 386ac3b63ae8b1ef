"""Writes tests/golden/render_reference.npz from the reference's own colour maps and camera paths (build container only; writes data, never source).

The reference is imported unchanged (nerfstudio/utils/colormaps.py, cameras/camera_paths.py, cameras/camera_utils.py, scripts/render.py; absent
third-party packages are stubbed and, one exception aside, never called).  The exception: get_crop_from_json builds its box's rotation with viser's
SO3.from_rpy_radians, and viser is absent, so that one call is answered by the project's own Rz(yaw) Ry(pitch) Rx(roll) (splat_camera._rotation_rpy)
-- the recorded crop pins the reference's reading of the JSON (centre, scale, rotation order, background / 255), not viser's arithmetic.

Recorded, for the cases of tests/render_functional.py: apply_colormap / apply_depth_colormap (float32, as the reference runs them); the camera path
functions with float64 inputs under torch.set_default_dtype(torch.float64) -- get_interpolated_poses_many rounds its result to float32 itself, so its
float64 parts (get_ordered_poses_and_k, get_interpolated_poses, get_interpolated_k) are recorded beside it --, get_spiral_path, get_path_from_json;
and, for information, the same path functions fed float32.

    python scripts/make_golden_render.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_import  # noqa: E402
import render_functional as rf  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "render_reference.npz")


def import_reference():
    if not ref_import.reference_available():
        raise SystemExit("the reference tree is not present: the golden file can only be written where it is")
    ref_import.install_extended_stubs()
    for name in ("mediapy", "xatlas", "pymeshlab"):
        if name not in sys.modules:
            ref_import._perm_mod(name)
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    from nerfstudio.cameras import camera_paths, camera_utils
    from nerfstudio.cameras.cameras import Cameras
    from nerfstudio.data import scene_box
    from nerfstudio.scripts import render
    from nerfstudio.utils import colormaps

    from nerfstudio_thermal_amd.splat_camera import _rotation_rpy

    class SO3:  # viser is absent: the one call the crop makes of it (see the module docstring)
        def __init__(self, m):
            self.m = m

        @staticmethod
        def from_rpy_radians(roll, pitch, yaw):
            return SO3(_rotation_rpy(roll, pitch, yaw).numpy())

        def as_matrix(self):
            return self.m

    scene_box.vtf.SO3 = SO3
    return colormaps, camera_paths, camera_utils, Cameras, render


def main():
    colormaps, camera_paths, camera_utils, Cameras, render = import_reference()
    f32 = lambda t: np.ascontiguousarray(torch.as_tensor(t).detach().cpu().numpy().astype(np.float32))  # noqa: E731
    f64 = lambda t: np.ascontiguousarray(torch.as_tensor(t).detach().cpu().numpy().astype(np.float64))  # noqa: E731
    arrays = {}
    for i, c in enumerate(rf.colormap_cases()):
        image, _ = rf.case_inputs(c)
        opts = colormaps.ColormapOptions(colormap=c["colormap"], normalize=c["normalize"], colormap_min=c["cmin"], colormap_max=c["cmax"], invert=c["invert"])
        arrays[rf.case_key("cm", i) + "_in"] = f32(image)
        arrays[rf.case_key("cm", i) + "_out"] = f32(colormaps.apply_colormap(image, opts))
    for i, c in enumerate(rf.depth_cases()):
        image, acc = rf.case_inputs(c)
        opts = colormaps.ColormapOptions(colormap=c["colormap"], normalize=c["normalize"], colormap_min=c["cmin"], colormap_max=c["cmax"], invert=c["invert"])
        arrays[rf.case_key("dp", i) + "_in"] = f32(image)
        if acc is not None:
            arrays[rf.case_key("dp", i) + "_acc"] = f32(acc)
        arrays[rf.case_key("dp", i) + "_out"] = f32(colormaps.apply_depth_colormap(image, accumulation=acc, near_plane=c["near"], far_plane=c["far"],
                                                                                    colormap_options=opts))
    notes = []
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        torch.set_default_dtype(dtype)
        try:
            for n, steps, order in rf.PATH_CASES:
                poses, Ks = rf.random_poses(n, seed=10 * n + steps)
                key = f"path_{tag}_n{n}_s{steps}_o{int(order)}"
                tp, tk = torch.tensor(poses, dtype=dtype), torch.tensor(Ks, dtype=dtype)
                try:
                    many_p, many_k = camera_utils.get_interpolated_poses_many(tp, tk, steps_per_transition=steps, order_poses=order)
                    arrays[key + "_many_poses"], arrays[key + "_many_Ks"] = f32(many_p), f32(many_k)  # the reference rounds these to float32 itself
                    op, ok = camera_utils.get_ordered_poses_and_k(tp, tk) if order else (tp, tk)
                    parts_p, parts_k = [], []
                    for a in range(n - 1):
                        parts_p += camera_utils.get_interpolated_poses(op[a].cpu().numpy(), op[a + 1].cpu().numpy(), steps=steps)
                        parts_k += [f64(k) for k in camera_utils.get_interpolated_k(ok[a], ok[a + 1], steps=steps)]
                    arrays[key + "_poses"], arrays[key + "_Ks"] = np.stack(parts_p).astype(np.float64), np.stack(parts_k)
                except Exception as e:  # (float32 poses: numpy refuses np.array(..., copy=False) where a copy is needed)
                    notes.append(f"{key}: {type(e).__name__}: {str(e).splitlines()[0]}")
            base_pose, base_K = rf.random_poses(1, seed=5)
            for i, s in enumerate(rf.SPIRAL_CASES):
                cam = Cameras(camera_to_worlds=torch.tensor(base_pose, dtype=dtype), fx=torch.tensor([base_K[0, 0, 0]], dtype=dtype),
                              fy=torch.tensor([base_K[0, 1, 1]], dtype=dtype), cx=320.0, cy=240.0)
                out = camera_paths.get_spiral_path(cam, steps=s["steps"], radius=s["radius"], radiuses=s["radiuses"], rots=s["rots"], zrate=s["zrate"])
                arrays[f"spiral_{tag}_{i}_poses"] = f64(out.camera_to_worlds)
                arrays[f"spiral_{tag}_{i}_fxfycxcy"] = np.array([float(out.fx[0]), float(out.fy[0]), float(out.cx[0]), float(out.cy[0])])
            cams = camera_paths.get_path_from_json(rf.CAMERA_PATH_JSON)
            arrays[f"json_{tag}_poses"] = f64(cams.camera_to_worlds)
            arrays[f"json_{tag}_fxfycxcy"] = np.stack([f64(cams.fx)[:, 0], f64(cams.fy)[:, 0], f64(cams.cx)[:, 0], f64(cams.cy)[:, 0]], 1)
            arrays[f"json_{tag}_size"] = np.array([int(cams.width[0]), int(cams.height[0])], dtype=np.int64)
        finally:
            torch.set_default_dtype(torch.float32)
    crop = render.get_crop_from_json(rf.CAMERA_PATH_JSON)
    arrays["crop_R"], arrays["crop_T"], arrays["crop_S"] = f64(crop.obb.R), f64(crop.obb.T), f64(crop.obb.S)
    arrays["crop_background"] = f32(crop.background_color)
    arrays["spiral_base_pose"], arrays["spiral_base_K"] = base_pose, base_K
    arrays["notes"] = np.array(notes if notes else [""])
    arrays["versions"] = np.array([f"torch {torch.__version__}", f"numpy {np.__version__}"])
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(arrays)} arrays")
    for n in notes:
        print("note:", n)


if __name__ == "__main__":
    main()
