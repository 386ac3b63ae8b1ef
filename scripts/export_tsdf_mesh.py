"""Export an RGB+thermal triangle mesh (the counterpart of `ns-export tsdf`, nerfstudio/exporter/tsdf_utils.py:278-361): train thermal-nerfacto or
thermal splats on a dataset -- or on the generated RGB+T cube scene of scripts/train_eval_scene.py -- for --iterations steps, render every training
camera (distortion off, as the reference renders them), fuse the depth frames into a TSDF volume with a colour and a temperature per voxel, extract
the surface and write `tsdf_mesh.ply`: float x y z nx ny nz, uchar red green blue thermal, triangles as `list uchar int vertex_indices`.

    python scripts/export_tsdf_mesh.py [--model nerf|splat] [--data DIR] [--iterations 3000] [--output-dir out/mesh] [--resolution 256 | X Y Z]
                                       [--downscale-factor 2] [--batch-size 10] [--bounding-box-min X Y Z --bounding-box-max X Y Z]
                                       [--no-bounding-box] [--truncation-margin 5] [--max-weight 1] [--observed-only] [--no-save-world-frame] [--ascii]
                                       [--target-num-faces N | --simplify-cell S]
                                       [--texture none|nerf|vertex] [--px-per-uv-triangle 4] [--usemtl rgb|thermal] [--chunk N]

--max-weight 1 is the reference's fusion (the weight is clamped to 1: every new frame counts for half); a large value gives the running mean over
all frames.  --observed-only drops the cells that touch a voxel no frame observed, and with them the shell the reference's meshes carry between
observed free space and the unobserved fill.  --no-bounding-box fuses over the dataparser's scene box.  --save-world-frame (the default) writes the
mesh in the dataset's own frame (mesh.mesh_to_dataset_frame).  --target-num-faces N simplifies the mesh to at most N faces by vertex clustering
(mesh.simplify_to_target; the reference's export decimates to 50 000 faces by default, with pymeshlab's quadric edge collapse, which this is not),
--simplify-cell S clusters with a cell of S voxels; neither is set by default, and the mesh is then written as extracted.  One JSON line reports the
sizes -- before and after the simplification, with the cell it used -- and the seconds of every stage.

--texture nerf|vertex also writes the reference's textured OBJ beside the PLY (texture.bake_texture / write_textured_obj: `mesh.obj`, `material_0.mtl`,
`material_0.png` and, for the thermal channel, `material_0_thermal.png`): "nerf" renders every texel of the atlas through the radiance field along the
interpolated normal (thermal-nerfacto only), "vertex" spreads the mesh's per-vertex colours and temperatures over the atlas (either model).
--px-per-uv-triangle is the side of a face's triangle in texels, --usemtl the material the OBJ names, --chunk the texels rendered per call (default:
the model's eval_num_rays_per_chunk).  The default, none, writes the PLY alone, as before.
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
    ap.add_argument("--model", default="nerf", choices=("nerf", "splat"), help="thermal-nerfacto (ray depth) or thermal splats (z depth)")
    ap.add_argument("--data", default=None, help="an RGB+T nerfstudio dataset (default: the generated cube scene)")
    ap.add_argument("--frames", type=int, default=12, help="frames per spectrum of the generated scene")
    ap.add_argument("--iterations", type=int, default=3000, help="training steps before the export")
    ap.add_argument("--density-mode", default="shared", choices=("shared", "separate"), help="thermal-nerfacto's density mode")
    ap.add_argument("--gaussians", type=int, default=20000, help="random initial Gaussians of the splat model")
    ap.add_argument("--output-dir", default="out/mesh")
    ap.add_argument("--resolution", type=int, nargs="+", default=[256], metavar="N", help="voxels per axis: one number or three")
    ap.add_argument("--downscale-factor", type=int, default=2, help="render the cameras at 1 / this size")
    ap.add_argument("--batch-size", type=int, default=10, help="frames fused per launch")
    ap.add_argument("--no-bounding-box", dest="use_bounding_box", action="store_false", help="fuse over the dataparser's scene box")
    ap.add_argument("--bounding-box-min", type=float, nargs=3, default=(-1.0, -1.0, -1.0), metavar=("X", "Y", "Z"))
    ap.add_argument("--bounding-box-max", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("X", "Y", "Z"))
    ap.add_argument("--truncation-margin", type=float, default=5.0, help="truncation distance in voxels")
    ap.add_argument("--max-weight", type=float, default=1.0, help="clamp of the fusion weight (1: the reference)")
    ap.add_argument("--min-accumulation", type=float, default=0.5, help="pixels rendered less opaque than this are no observation")
    ap.add_argument("--observed-only", action="store_true", help="drop cells that touch an unobserved voxel")
    ap.add_argument("--save-world-frame", dest="save_world_frame", action="store_true", default=True, help="write the mesh in the dataset's frame (default)")
    ap.add_argument("--no-save-world-frame", dest="save_world_frame", action="store_false", help="write it in the model's frame")
    ap.add_argument("--ascii", action="store_true", help="write an ASCII PLY")
    ap.add_argument("--target-num-faces", type=int, default=None, metavar="N", help="simplify the mesh to at most N faces (the reference's default: 50000)")
    ap.add_argument("--simplify-cell", type=float, default=None, metavar="S", help="simplify the mesh by clustering its vertices in cells of S voxels")
    ap.add_argument("--texture", default="none", choices=("none", "nerf", "vertex"), help="also write a textured OBJ: baked from the NeRF or from the vertices")
    ap.add_argument("--px-per-uv-triangle", type=int, default=4, metavar="PX", help="texels along a face's triangle in the atlas (at least 2)")
    ap.add_argument("--usemtl", default="rgb", choices=("rgb", "thermal"), help="the material the OBJ uses: the colour or the thermal texture")
    ap.add_argument("--chunk", type=int, default=None, metavar="N", help="texels rendered per call (default: the model's eval_num_rays_per_chunk)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if len(args.resolution) not in (1, 3):
        ap.error("--resolution takes one number or three")
    if args.target_num_faces is not None and args.simplify_cell is not None:
        ap.error("--target-num-faces and --simplify-cell exclude each other")
    if (args.target_num_faces is not None and args.target_num_faces < 0) or (args.simplify_cell is not None and not args.simplify_cell > 0):
        ap.error("--target-num-faces takes a number >= 0, --simplify-cell a size > 0")
    if args.texture == "nerf" and args.model != "nerf":
        ap.error("--texture nerf renders rays through the radiance field: use --texture vertex with --model splat")
    if args.px_per_uv_triangle < 2 or (args.chunk is not None and args.chunk < 1):
        ap.error("--px-per-uv-triangle takes a number >= 2, --chunk a number >= 1")
    return args


def pinhole_cameras(outputs, device):
    """The dataparser's cameras as PinholeCameras with the distortion dropped (the reference fuses with disable_distortion=True)."""
    from nerfstudio_thermal_amd.splat_camera import PinholeCamera

    c = outputs.cameras
    return [PinholeCamera(c["c2w"][i].float().to(device), float(c["fx"][i]), float(c["fy"][i]), float(c["cx"][i]), float(c["cy"][i]), int(c["width"][i]),
                          int(c["height"][i]), cam_idx=i, is_thermal=bool(outputs.metadata["is_thermal"][i])) for i in range(len(outputs.image_filenames))]


def train_nerf(args, data, dev):
    from nerfstudio_thermal_amd.config import ThermalNerfactoModelConfig
    from nerfstudio_thermal_amd.pipeline import ThermalPipeline

    pipe = ThermalPipeline(data, ThermalNerfactoModelConfig(density_mode=args.density_mode), device=dev, seed=args.seed)
    if args.iterations > 0:
        pipe.train(args.iterations)
    return pipe.model, pipe.train_outputs, pinhole_cameras(pipe.train_outputs, dev)


def train_splat(args, data, dev):
    import torch

    from nerfstudio_thermal_amd import ThermalFullImageDatamanagerConfig
    from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig
    from nerfstudio_thermal_amd.model import TrainingCallbackLocation
    from nerfstudio_thermal_amd.optim import SPLAT_BILAGRID_OPTIMIZERS, SPLAT_CAMERA_OPTIMIZERS, SPLAT_OPTIMIZERS, HipAdam, Optimizers
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

    dm = ThermalFullImageDatamanagerConfig(dataparser=ThermalNerfDataParserConfig(data=data), seed=args.seed).setup(device=dev)
    model = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(num_random=args.gaussians, random_scale=1.0, background_color="random"), device=dev,
                                   seed=args.seed, num_train_data=dm.num_train_data, train_is_thermal=dm.train_is_thermal)
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
    return model, dm.train_dataparser_outputs, list(dm.train_cameras)  # the datamanager's cameras are the undistorted ones it trained on


def main(argv=None):
    args = parse_args(argv)
    import torch

    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import mesh

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
    model, outputs, cameras = (train_nerf if args.model == "nerf" else train_splat)(args, data, dev)
    sync(); train_s = time.perf_counter() - t0
    resolution = args.resolution[0] if len(args.resolution) == 1 else list(args.resolution)
    t1 = time.perf_counter()
    m, volume = mesh.export_tsdf_mesh(model, cameras, resolution=resolution, downscale_factor=args.downscale_factor, batch_size=args.batch_size,
                                      use_bounding_box=args.use_bounding_box, bounding_box_min=args.bounding_box_min,
                                      bounding_box_max=args.bounding_box_max, scene_box=outputs.scene_box_aabb, truncation_margin=args.truncation_margin,
                                      max_weight=args.max_weight, min_accumulation=args.min_accumulation, observed_only=args.observed_only,
                                      return_volume=True)
    sync(); export_s = time.perf_counter() - t1
    simplified = None
    if args.target_num_faces is not None or args.simplify_cell is not None:
        before = {"vertices_extracted": int(m.vertices.shape[0]), "faces_extracted": int(m.faces.shape[0])}
        origin = mesh.lattice_centred_origin(volume)
        ts = time.perf_counter()
        if args.target_num_faces is not None:
            m, cell = mesh.simplify_to_target(m, args.target_num_faces, volume.voxel_size, origin=origin)
        else:
            cell = tuple(float(args.simplify_cell * v) for v in volume.voxel_size)
            m = mesh.simplify_mesh(m, cell, origin=origin)
        sync()
        simplified = dict(before, simplify_cell=None if cell is None else list(cell),
                          simplify_cell_voxels=None if cell is None else float(cell[0]) / float(volume.voxel_size[0]),
                          target_num_faces=args.target_num_faces, simplify_seconds=time.perf_counter() - ts)
    meta =json.load(open(os.path.join(data, "transforms.json"), encoding="utf-8"))
    t2 = time.perf_counter()
    ply = mesh.write_mesh_ply(os.path.join(args.output_dir, "tsdf_mesh.ply"), m, binary=not args.ascii,
                              dataparser_outputs=outputs if args.save_world_frame else None, applied_transform=meta.get("applied_transform"))
    write_s = time.perf_counter() - t2
    textured = None
    if args.texture != "none" and int(m.faces.shape[0]) > 0:
        from nerfstudio_thermal_amd import texture

        t3 = time.perf_counter()
        tex = texture.bake_texture(m, model, args.px_per_uv_triangle, source=args.texture, chunk=args.chunk)
        sync(); bake_s = time.perf_counter() - t3
        t4 = time.perf_counter()
        paths = texture.write_textured_obj(args.output_dir, m, tex, dataparser_outputs=outputs if args.save_world_frame else None,
                                           applied_transform=meta.get("applied_transform"), usemtl=args.usemtl)
        textured = {"texture": args.texture, "px_per_uv_triangle": args.px_per_uv_triangle, "texture_size": [int(tex.rgb.shape[1]), int(tex.rgb.shape[0])],
                    "raylen": tex.raylen, "usemtl": args.usemtl, "bake_seconds": bake_s, "obj_write_seconds": time.perf_counter() - t4, "obj": paths["obj"]}
    print(json.dumps({"dataset": data if args.data is not None else f"generated cube scene ({data})", "model": args.model, "iterations": args.iterations,
                      "train_seconds": train_s, "cameras": len(cameras), "volume_dims": list(volume.dims), "truncation": volume.truncation,
                      "max_weight": args.max_weight, "observed_only": args.observed_only, "observed_voxel_share": float((volume.weights > 0).float().mean()),
                      "vertices": int(m.vertices.shape[0]), "faces": int(m.faces.shape[0]), "render_fuse_and_mesh_seconds": export_s,
                      "write_seconds": write_s, "frame": "dataset" if args.save_world_frame else "model", "ply": ply, **(simplified or {}), **(textured or {})}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
