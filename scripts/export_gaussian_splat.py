"""Export thermal splats as a Gaussian-splat PLY (the counterpart of `ns-export gaussian-splat`, nerfstudio/scripts/exporter.py:480-546): train
ThermalSplatfactoModel on a dataset -- or on the generated RGB+T cube scene of scripts/train_eval_scene.py -- for --iterations steps, or start from a
splat file (--load), and write `splat.ply` in the Inria layout every splat viewer reads.

    python scripts/export_gaussian_splat.py [--data DIR] [--iterations 3000] [--output-dir out/splat] [--spectrum both|rgb|thermal]
                                            [--min-opacity 0.005] [--obb-center X Y Z --obb-rotation ROLL PITCH YAW --obb-scale SX SY SZ]
                                            [--load PLY] [--thermal-opacity-mode shared|separate] [--sh-degree 3] [--gaussians 20000]
                                            [--save-world-frame] [--load-world-frame]
                                            [--prune-min-contribution X | --prune-keep-ratio R]

--prune-min-contribution X (RadSplat's rule; 0.01 is its value) or --prune-keep-ratio R scores every Gaussian of the in-memory model by its ray
contribution over the dataset's training cameras of both spectra (splat_prune.score_gaussians: tn_splat_raster_contrib) and removes the others
before the export; opacity (--min-opacity) says little about what a Gaussian adds to any frame.  Needs a dataset, as the frame options do.
--spectrum both (the default) writes the colour scene under the Inria property names followed by f_dc_thermal, f_rest_thermal_* and, in separate
mode, opacity_thermal: viewers ignore the extras, splat_io.load_gaussian_ply reads them back (bit for bit for --sh-degree > 0).  --spectrum thermal
writes the thermal parameters under the Inria names, so any viewer shows the thermal scene in grey.  Gaussians with sigmoid(opacity) below
--min-opacity (in a "both" file of a separate-mode model: in both spectra) and Gaussians with a parameter that is not finite are dropped; the
--obb-* arguments (all three or none; rotation in radians) keep only the Gaussians whose mean is strictly inside that oriented box, the eval
render's crop.  --load PLY starts from a splat file instead of random Gaussians -- an Inria file from any trainer, or one written here -- and
trains on from it for --iterations steps (0: load, filter, write).  Without --save-world-frame the file is in the model's frame; with it the
Gaussians are moved into the dataset's own frame (splat_transform.dataset_frame: the inverse of the dataparser's transform and scale, the SH bands
rotated with the geometry), where scripts/export_point_cloud.py and scripts/export_tsdf_mesh.py put theirs.  The generated scene's dataparser
transform is the identity, so there the two frames are one and the line says so.  --load-world-frame reads the --load file as a dataset-frame file.
Both need a dataset: --data, or the generated scene of a run that trains.  One JSON line reports the counts and the seconds of every stage.
"""
import argparse
import functools
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
    ap.add_argument("--iterations", type=int, default=3000, help="training steps before the export")
    ap.add_argument("--gaussians", type=int, default=20000, help="random initial Gaussians")
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--thermal-opacity-mode", default="shared", choices=("shared", "separate"))
    ap.add_argument("--output-dir", default="out/splat")
    ap.add_argument("--spectrum", default="both", choices=("rgb", "thermal", "both"))
    ap.add_argument("--min-opacity", type=float, default=0.005, help="drop Gaussians less opaque than this (0: keep every opacity)")
    ap.add_argument("--obb-center", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    ap.add_argument("--obb-rotation", type=float, nargs=3, default=None, metavar=("ROLL", "PITCH", "YAW"), help="radians")
    ap.add_argument("--obb-scale", type=float, nargs=3, default=None, metavar=("SX", "SY", "SZ"))
    ap.add_argument("--load", default=None, metavar="PLY", help="start from this Gaussian-splat PLY")
    ap.add_argument("--save-world-frame", action="store_true", help="write the file in the dataset's frame (default: the model's)")
    ap.add_argument("--load-world-frame", action="store_true", help="the --load file is in the dataset's frame")
    ap.add_argument("--seed", type=int, default=0)
    prune = ap.add_mutually_exclusive_group()
    prune.add_argument("--prune-min-contribution", type=float, default=None, metavar="X",
                       help="before the export, drop the Gaussians whose largest blending weight on any training ray is below X (RadSplat: 0.01)")
    prune.add_argument("--prune-keep-ratio", type=float, default=None, metavar="R", help="or keep the ceil(R N) Gaussians that contribute most")
    args = ap.parse_args(argv)
    if (args.prune_min_contribution is not None or args.prune_keep_ratio is not None) and args.data is None and args.iterations == 0:
        ap.error("--prune-min-contribution and --prune-keep-ratio score over a dataset's training cameras: --data, or a run that trains on the generated scene")
    if args.prune_min_contribution is not None and not args.prune_min_contribution >= 0:
        ap.error("--prune-min-contribution takes a number >= 0")
    if args.prune_keep_ratio is not None and not 0.0 <= args.prune_keep_ratio <= 1.0:
        ap.error("--prune-keep-ratio takes a ratio in [0, 1]")
    if args.load_world_frame and args.load is None:
        ap.error("--load-world-frame goes with --load")
    if (args.save_world_frame or args.load_world_frame) and args.data is None and args.iterations == 0:
        ap.error("--save-world-frame and --load-world-frame need a dataset: --data, or a run that trains on the generated scene")
    obb = (args.obb_center, args.obb_rotation, args.obb_scale)
    if any(a is not None for a in obb) and not all(a is not None for a in obb):
        ap.error("--obb-center, --obb-rotation and --obb-scale go together")
    if not 0.0 <= args.min_opacity < 1.0:
        ap.error("--min-opacity takes a value in [0, 1)")
    if args.iterations < 0 or args.sh_degree < 0:
        ap.error("--iterations and --sh-degree take numbers >= 0")
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch

    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import ThermalFullImageDatamanagerConfig, splat_io
    from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig
    from nerfstudio_thermal_amd.model import TrainingCallbackLocation
    from nerfstudio_thermal_amd.optim import SPLAT_BILAGRID_OPTIMIZERS, SPLAT_CAMERA_OPTIMIZERS, SPLAT_OPTIMIZERS, HipAdam, Optimizers
    from nerfstudio_thermal_amd.splat import OrientedBox, ThermalSplatfactoModel, ThermalSplatfactoModelConfig
    from nerfstudio_thermal_amd.splat_transform import dataset_frame

    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    os.makedirs(args.output_dir, exist_ok=True)
    cfg = ThermalSplatfactoModelConfig(num_random=args.gaussians, random_scale=1.0, background_color="random", sh_degree=args.sh_degree,
                                       thermal_opacity_mode=args.thermal_opacity_mode)
    sync = torch.cuda.synchronize
    dm = None
    data = args.data
    if args.iterations > 0:
        if data is None:
            from train_eval_scene import write_cube_scene

            data = os.path.join(args.output_dir, "scene")
            write_cube_scene(data, args.frames, dev)
        dm = ThermalFullImageDatamanagerConfig(dataparser=ThermalNerfDataParserConfig(data=data), seed=args.seed).setup(device=dev)
    model = ThermalSplatfactoModel(cfg, device=dev, seed=args.seed, num_train_data=dm.num_train_data if dm else 0,
                                   train_is_thermal=dm.train_is_thermal if dm else None)
    world = None  # model frame -> dataset frame
    if args.save_world_frame or args.load_world_frame:
        outputs = dm.train_dataparser_outputs if dm is not None else ThermalNerfDataParserConfig(data=data).setup().get_dataparser_outputs("train")
        meta = json.load(open(os.path.join(data, "transforms.json"), encoding="utf-8"))
        world = dataset_frame(outputs, meta.get("applied_transform"))
    loaded = None
    if args.load is not None:
        t = time.perf_counter()
        info = splat_io.load_gaussian_ply(model, args.load, transform=world.inverse() if args.load_world_frame else None)
        loaded = {"path": args.load, "gaussians": info["num_gaussians"], "sh_degree": info["sh_degree"], "has_thermal": info["has_thermal"],
                  "separate": info["separate"], "frame": "dataset" if args.load_world_frame else "model", "load_seconds": time.perf_counter() - t}
    sync(); t0 = time.perf_counter()
    if dm is not None:
        opts = Optimizers(model.get_param_groups(), {**SPLAT_OPTIMIZERS, **SPLAT_CAMERA_OPTIMIZERS, **SPLAT_BILAGRID_OPTIMIZERS}, optimizer_cls=HipAdam)
        cbs = model.get_training_callbacks(opts)
        for step in range(args.iterations):
            cam, batch = dm.next_train(step)
            for cb in cbs:
                cb.run_callback_at_location(step, TrainingCallbackLocation.BEFORE_TRAIN_ITERATION)
            opts.zero_grad_all()
            functools.reduce(torch.add, model.get_loss_dict(model.get_train_outputs(cam), batch).values()).backward()
            opts.optimizer_step_all()
            opts.scheduler_step_all()
            for cb in cbs:
                cb.run_callback_at_location(step, TrainingCallbackLocation.AFTER_TRAIN_ITERATION)
    sync(); train_s = time.perf_counter() - t0
    pruned = None
    if args.prune_min_contribution is not None or args.prune_keep_ratio is not None:  # the in-memory model, before the pack kernel sees it
        from nerfstudio_thermal_amd import splat_prune

        t = time.perf_counter()
        cams = (dm if dm is not None else ThermalFullImageDatamanagerConfig(dataparser=ThermalNerfDataParserConfig(data=data), seed=args.seed).setup(device=dev)).train_cameras
        model.eval()
        before = model.num_points
        keep = splat_prune.prune_mask(splat_prune.score_gaussians(model, cams), min_contribution=args.prune_min_contribution, keep_ratio=args.prune_keep_ratio)
        removed = splat_prune.prune_gaussians(model, keep)
        sync()
        pruned = {"min_contribution": args.prune_min_contribution, "keep_ratio": args.prune_keep_ratio, "cameras": len(cams), "gaussians_before": before,
                  "removed": removed, "seconds": time.perf_counter() - t}
    box = OrientedBox.from_params(args.obb_center, args.obb_rotation, args.obb_scale) if args.obb_center is not None else None
    t1 = time.perf_counter()
    out = splat_io.export_gaussian_ply(model, os.path.join(args.output_dir, "splat.ply"), spectrum=args.spectrum, min_opacity=args.min_opacity, crop=box,
                                       transform=world if args.save_world_frame else None)
    export_s = time.perf_counter() - t1
    print(json.dumps({"dataset": None if dm is None else (args.data if args.data is not None else "generated cube scene"), "loaded": loaded,
                      "iterations": args.iterations, "train_seconds": train_s, "pruned": pruned, "gaussians": model.num_points, "exported": out["exported"],
                      "dropped": out["dropped"], "spectrum": args.spectrum, "min_opacity": args.min_opacity, "sh_degree": args.sh_degree,
                      "thermal_opacity_mode": args.thermal_opacity_mode, "properties": len(out["properties"]),
                      "obb": None if box is None else {"center": args.obb_center, "rotation": args.obb_rotation, "scale": args.obb_scale},
                      "frame": ("dataset (the dataparser's transform is the identity: also the model's)" if world.is_identity else "dataset")
                      if args.save_world_frame else "model", "export_seconds": export_s, "file_bytes": os.path.getsize(out["path"]), "ply": out["path"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
