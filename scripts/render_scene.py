"""Render frames of a trained scene (the counterpart of `ns-render`, nerfstudio/scripts/render.py): train thermal-nerfacto or thermal splats on a
dataset -- or on the generated RGB+T cube scene of scripts/train_eval_scene.py -- for --iterations steps, or start splats from a file (--load), and
write PNG frames: rgb, the thermal image in false colour and depth side by side.

    python scripts/render_scene.py camera-path --json PATH.json [options]     the cameras (and the crop) of a viewer's camera-path file
    python scripts/render_scene.py interpolate [--interpolation-steps 10] [--order-poses] [--pose-source eval|train] [options]
    python scripts/render_scene.py spiral [--frames 30] [--radius 0.1] [options]          a spiral around the first eval camera
    python scripts/render_scene.py dataset [--split train|test] [options]    one PNG per frame and output, ground truth beside rgb / thermal

    options: --model nerf|splat  --data DIR  --iterations N  --load PLY (splats)  --output-dir DIR  --rendered-output-names rgb thermal depth
             --colormap default|turbo|viridis|magma|inferno|cividis|gray  --normalize  --colormap-min 0  --colormap-max 1  --invert
             --depth-near-plane D  --depth-far-plane D  --downscale N

Frames are written as 00000.png, ... (PNG sequences only: there is no video encoder here).  The default thermal panel is the model's own output
(`rgb_thermal` for thermal-nerfacto, `thermal` for splats).  A crop in the camera-path file goes to the splat model's render; thermal-nerfacto does
not crop and says so.  One JSON line reports the counts and the seconds of every stage.
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

COLORMAPS = ("default", "turbo", "viridis", "magma", "inferno", "cividis", "gray")


def parse_args(argv=None):
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument("--model", default="splat", choices=("nerf", "splat"))
    common.add_argument("--data", default=None, help="an RGB+T nerfstudio dataset (default: the generated cube scene)")
    common.add_argument("--frames", type=int, default=12, help="frames per spectrum of the generated scene; cameras of a spiral")
    common.add_argument("--iterations", type=int, default=3000, help="training steps before the render")
    common.add_argument("--density-mode", default="shared", choices=("shared", "separate"), help="thermal-nerfacto's density mode")
    common.add_argument("--gaussians", type=int, default=20000, help="random initial Gaussians of the splat model")
    common.add_argument("--load", default=None, metavar="PLY", help="start the splat model from this Gaussian-splat PLY")
    common.add_argument("--output-dir", default="out/render")
    common.add_argument("--rendered-output-names", nargs="+", default=None, metavar="NAME")
    common.add_argument("--colormap", default="default", choices=COLORMAPS)
    common.add_argument("--normalize", action="store_true")
    common.add_argument("--colormap-min", type=float, default=0.0)
    common.add_argument("--colormap-max", type=float, default=1.0)
    common.add_argument("--invert", action="store_true")
    common.add_argument("--depth-near-plane", type=float, default=None)
    common.add_argument("--depth-far-plane", type=float, default=None)
    common.add_argument("--downscale", type=float, default=1.0, help="render at 1 / this size")
    common.add_argument("--seed", type=int, default=0)
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    p = sub.add_parser("camera-path", parents=[common])
    p.add_argument("--json", required=True, help="a camera-path file written by the viewer")
    p = sub.add_parser("interpolate", parents=[common])
    p.add_argument("--interpolation-steps", type=int, default=10)
    p.add_argument("--order-poses", action="store_true")
    p.add_argument("--pose-source", default="eval", choices=("eval", "train"))
    p = sub.add_parser("spiral", parents=[common])
    p.add_argument("--radius", type=float, default=0.1)
    p = sub.add_parser("dataset", parents=[common])
    p.add_argument("--split", default="test", choices=("train", "test"))
    args = ap.parse_args(argv)
    if args.load is not None and args.model != "splat":
        ap.error("--load reads a Gaussian-splat PLY: use it with --model splat")
    if args.iterations < 0 or not args.downscale > 0:
        ap.error("--iterations takes a number >= 0, --downscale a number > 0")
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch

    import nerfstudio_thermal_amd  # noqa: F401
    from export_tsdf_mesh import train_nerf, train_splat
    from nerfstudio_thermal_amd import ThermalFullImageDatamanagerConfig, render
    from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig

    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    os.makedirs(args.output_dir, exist_ok=True)
    data = args.data
    if data is None:
        from train_eval_scene import write_cube_scene

        data = os.path.join(args.output_dir, "scene")
        write_cube_scene(data, args.frames, dev)
    sync = torch.cuda.synchronize
    sync(); t0 = time.perf_counter()
    if args.load is not None:
        from nerfstudio_thermal_amd import splat_io
        from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

        model = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(num_random=16), device=dev, seed=args.seed)
        splat_io.load_gaussian_ply(model, args.load)
    else:
        model, _, _ = (train_nerf if args.model == "nerf" else train_splat)(args, data, dev)
    sync(); train_s = time.perf_counter() - t0
    options = render.ColormapOptions(colormap=args.colormap, normalize=args.normalize, colormap_min=args.colormap_min, colormap_max=args.colormap_max,
                                     invert=args.invert)
    crop = None
    t1 = time.perf_counter()
    if args.command == "dataset":
        dm = ThermalFullImageDatamanagerConfig(dataparser=ThermalNerfDataParserConfig(data=data), seed=args.seed).setup(device=dev)
        pairs = list(zip(dm.train_cameras, dm.cached_train)) if args.split == "train" else dm.fixed_indices_eval_dataloader
        paths = render.render_dataset(model, pairs, os.path.join(args.output_dir, args.split), args.rendered_output_names, options, args.depth_near_plane,
                                      args.depth_far_plane)
    else:
        if args.command == "camera-path":
            with open(args.json, encoding="utf-8") as f:
                path_json = json.load(f)
            cameras, crop = render.path_from_json(path_json), render.crop_from_json(path_json)
        else:
            dm = ThermalFullImageDatamanagerConfig(dataparser=ThermalNerfDataParserConfig(data=data), seed=args.seed).setup(device=dev)
            source = dm.train_cameras if getattr(args, "pose_source", "eval") == "train" or not dm.eval_cameras else dm.eval_cameras
            if args.command == "interpolate":
                cameras = render.interpolated_path(source, args.interpolation_steps, args.order_poses)
            else:
                cameras = render.spiral_path(source[0], steps=args.frames, radius=args.radius)
        paths = render.render_trajectory(model, cameras, os.path.join(args.output_dir, args.command), args.rendered_output_names, crop, options,
                                         args.depth_near_plane, args.depth_far_plane, rendered_resolution_scaling_factor=1.0 / args.downscale)
    sync(); render_s = time.perf_counter() - t1
    print(json.dumps({"command": args.command, "model": args.model, "dataset": data if args.data is not None else f"generated cube scene ({data})",
                      "loaded": args.load, "iterations": 0 if args.load else args.iterations, "train_seconds": train_s, "frames": len(paths),
                      "cropped": crop is not None, "colormap": args.colormap, "render_seconds": render_s,
                      "seconds_per_frame": render_s / max(len(paths), 1), "first": paths[0] if paths else None}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
