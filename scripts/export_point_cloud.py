"""Export an RGB+thermal point cloud from thermal-nerfacto (the counterpart of `ns-export pointcloud`, nerfstudio/scripts/exporter.py:90-186): train
a dataset -- or the generated RGB+T cube scene of scripts/train_eval_scene.py -- for --iterations steps, render training rays, keep the opaque points
inside the box, remove statistical outliers on the device and write `point_cloud.ply` with uchar red green blue and thermal.

    python scripts/export_point_cloud.py [--data DIR] [--iterations 3000] [--output-dir out/cloud] [--num-points 1000000] [--std-ratio 10]
                                         [--no-remove-outliers] [--obb-center X Y Z --obb-rotation R P Y --obb-scale SX SY SZ]
                                         [--no-save-world-frame] [--set-ply-file-path]
                                         [--normal-method none|knn] [--normals-knn 30] [--no-reorient-normals]

--save-world-frame (the default) writes the cloud in the dataset's own frame (cloud.to_dataset_frame), where a `ply_file_path` entry expects it.
--set-ply-file-path writes a COPY of the dataset's transforms.json next to the cloud, with `ply_file_path` naming it and the frames' file paths
made absolute; the dataset itself is never edited.  Point the splat trainer's dataparser (load_3D_points=True) at that copy to seed thermal splats
with the NeRF's colours and temperatures.  --normal-method knn (the reference's default, normal_method="open3d") estimates a unit normal per
point from its --normals-knn nearest points after the outliers are gone, flips it against the ray that produced the point unless
--no-reorient-normals, and writes float nx ny nz after x y z (rotated into the dataset's frame with the points); the default, none, writes the
file this script always wrote.  One JSON line reports the sizes and the seconds of every stage.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--data", default=None, help="an RGB+T nerfstudio dataset (default: the generated cube scene)")
    ap.add_argument("--frames", type=int, default=12, help="frames per spectrum of the generated scene")
    ap.add_argument("--iterations", type=int, default=3000, help="thermal-nerfacto training steps before the export")
    ap.add_argument("--density-mode", default="shared", choices=("shared", "separate"))
    ap.add_argument("--output-dir", default="out/cloud")
    ap.add_argument("--num-points", type=int, default=1_000_000)
    ap.add_argument("--std-ratio", type=float, default=10.0, help="outlier threshold in standard deviations of the neighbour means")
    ap.add_argument("--no-remove-outliers", dest="remove_outliers", action="store_false")
    ap.add_argument("--no-bounding-box", dest="use_bounding_box", action="store_false", help="keep opaque points wherever they are")
    ap.add_argument("--obb-center", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="centre of the oriented box")
    ap.add_argument("--obb-rotation", type=float, nargs=3, default=None, metavar=("ROLL", "PITCH", "YAW"), help="its rotation, radians")
    ap.add_argument("--obb-scale", type=float, nargs=3, default=None, metavar=("SX", "SY", "SZ"), help="its extents")
    ap.add_argument("--save-world-frame", dest="save_world_frame", action="store_true", default=True,
                    help="write the cloud in the dataset's frame (default)")
    ap.add_argument("--no-save-world-frame", dest="save_world_frame", action="store_false", help="write it in the model's frame")
    ap.add_argument("--set-ply-file-path", action="store_true", help="write a copy of transforms.json that names the cloud as ply_file_path")
    ap.add_argument("--normal-method", default="none", choices=("none", "knn"),
                    help="knn: estimate normals from each point's nearest neighbours and write nx ny nz (default: none)")
    ap.add_argument("--normals-knn", type=int, default=30, help="points per neighbourhood, the point itself counted (3..32)")
    ap.add_argument("--no-reorient-normals", dest="reorient_normals", action="store_false",
                    help="leave the normals' sign to the rule of the library, not to the view directions")
    ap.add_argument("--ascii", action="store_true", help="write an ASCII PLY")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    obb = (args.obb_center, args.obb_rotation, args.obb_scale)
    if any(v is not None for v in obb) and not all(v is not None for v in obb):
        ap.error("--obb-center, --obb-rotation and --obb-scale go together")
    if not 3 <= args.normals_knn <= 32:
        ap.error("--normals-knn must be in 3..32")
    return args


def transforms_copy(data: str, out_dir: str, ply_name: str) -> str:
    """transforms.json of `data` with ply_file_path = the cloud and absolute frame paths, written into out_dir (the dataset stays as it is)."""
    with open(os.path.join(data, "transforms.json"), encoding="utf-8") as f:
        meta = json.load(f)
    for fr in meta["frames"]:
        if not os.path.isabs(fr["file_path"]):
            fr["file_path"] = os.path.abspath(os.path.join(data, fr["file_path"]))
    meta["ply_file_path"] = ply_name
    path = os.path.join(out_dir, "transforms.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(meta, f, indent=4)
    return path


def main(argv=None):
    args = parse_args(argv)
    import torch

    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import cloud
    from nerfstudio_thermal_amd.config import ThermalNerfactoModelConfig
    from nerfstudio_thermal_amd.pipeline import ThermalPipeline
    from nerfstudio_thermal_amd.rays import RayBundle
    from nerfstudio_thermal_amd.splat_camera import OrientedBox

    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    os.makedirs(args.output_dir, exist_ok=True)
    data = args.data
    if data is None:  # the generated scene is written next to the cloud, so a transforms.json copy can go on naming its frames
        from train_eval_scene import write_cube_scene

        data = os.path.join(args.output_dir, "scene")
        write_cube_scene(data, args.frames, dev)
    pipe = ThermalPipeline(data, ThermalNerfactoModelConfig(density_mode=args.density_mode), device=dev, seed=args.seed)
    sync = torch.cuda.synchronize
    sync(); t0 = time.perf_counter()
    losses = pipe.train(args.iterations) if args.iterations > 0 else {}
    sync(); train_s = time.perf_counter() - t0

    def next_rays():
        o, d, cam, _, _ = pipe.datamanager.next_train(0)
        return RayBundle(origins=o, directions=d, pixel_area=torch.ones_like(o[:, :1]), camera_indices=cam[:, None])

    box = OrientedBox.from_params(args.obb_center, args.obb_rotation, args.obb_scale) if args.obb_center is not None else None
    t1 = time.perf_counter()
    want_normals = args.normal_method == "knn"
    raw = cloud.gather_points(pipe.model, next_rays, num_points=args.num_points, box=box, use_bounding_box=args.use_bounding_box,
                              with_view=want_normals)  # generate_point_cloud's loop; its other two stages follow, timed on their own
    sync(); gather_s = time.perf_counter() - t1
    t2 = time.perf_counter()
    details = {}
    pc = cloud.remove_outliers(raw, 20, args.std_ratio, details) if args.remove_outliers else raw
    sync(); clean_s = time.perf_counter() - t2
    t3 = time.perf_counter()
    if want_normals:
        cloud.estimate_normals(pc, args.normals_knn, reorient=args.reorient_normals)
    sync(); normals_s = time.perf_counter() - t3
    meta = json.load(open(os.path.join(data, "transforms.json"), encoding="utf-8"))
    xyz = cloud.to_dataset_frame(pc.xyz, pipe.train_outputs, meta.get("applied_transform")) if args.save_world_frame else pc.xyz
    nrm = cloud.normals_to_dataset_frame(pc.normals, pipe.train_outputs, meta.get("applied_transform")) if want_normals and args.save_world_frame else None
    ply = cloud.write_cloud_ply(os.path.join(args.output_dir, "point_cloud.ply"), pc, xyz, binary=not args.ascii, normals=nrm)
    copy = transforms_copy(data, args.output_dir, "point_cloud.ply") if args.set_ply_file_path else None
    print(json.dumps({"dataset": data if args.data is not None else f"generated cube scene ({data})", "iterations": args.iterations, "train_seconds": train_s,
                      "final_losses": losses, "num_points": args.num_points, "points_written": len(pc), "render_and_append_seconds": gather_s,
                      "remove_outliers_seconds": clean_s, "normal_method": args.normal_method,
                      "estimate_normals_seconds": normals_s if want_normals else None, "outlier_stats_m_s_thr": details["stats"].tolist() if details else None,
                      "frame": "dataset" if args.save_world_frame else "model", "ply": ply, "transforms_copy": copy}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
