"""Export an RGB+thermal Poisson surface mesh (the counterpart of `ns-export poisson`, nerfstudio/scripts/exporter.py ExportPoissonMesh): train
thermal-nerfacto on a dataset -- or on the generated RGB+T cube scene of scripts/train_eval_scene.py -- for --iterations steps, export an oriented point
cloud (cloud.generate_point_cloud with estimate_normals), reconstruct the surface on a dense lattice (poisson.poisson_reconstruct: not Open3D's
adaptive octree) and write `poisson_mesh.ply`: float x y z nx ny nz, uchar red green blue thermal, triangles as `list uchar int vertex_indices`.

    python scripts/export_poisson_mesh.py [--data DIR] [--iterations 3000] [--output-dir out/poisson] [--resolution 256 | X Y Z] [--num-points 1000000]
                                          [--bounding-box-min X Y Z --bounding-box-max X Y Z] [--trim-quantile 0.1] [--screening 0]
                                          [--no-density-normalize] [--tol 1e-3] [--max-iterations N] [--target-num-faces N] [--save-point-cloud]
                                          [--no-save-world-frame] [--ascii] [--texture none|nerf|vertex] [--px-per-uv-triangle 4] [--usemtl rgb|thermal]
    python scripts/export_poisson_mesh.py --from-ply CLOUD.ply [...]

--from-ply meshes a PLY that has normals (x y z nx ny nz, and red green blue thermal where present: scripts/export_point_cloud.py --normal-method knn
writes one; so does any tool that orients its normals out of the surface) and needs neither a dataset nor a model: the mesh is written in the
file's own frame, and --texture nerf is not available.  --resolution 512 is the reference's depth 9.  --trim-quantile 0 keeps the closed surface;
the reference's 0.1 removes the vertices in the tenth of the surface the cloud supports least.  --target-num-faces N simplifies by vertex clustering
(mesh.simplify_to_target; the reference decimates to 50 000 faces with pymeshlab's edge collapse, which this is not).  --save-point-cloud also writes
the oriented cloud as `point_cloud.ply`.  One JSON line reports the sizes, the solve's iterations and residual and the seconds of every stage.
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
    ap.add_argument("--from-ply", default=None, metavar="PLY", help="mesh this point cloud with normals instead of training a model")
    ap.add_argument("--frames", type=int, default=12, help="frames per spectrum of the generated scene")
    ap.add_argument("--iterations", type=int, default=3000, help="thermal-nerfacto training steps before the export")
    ap.add_argument("--density-mode", default="shared", choices=("shared", "separate"))
    ap.add_argument("--output-dir", default="out/poisson")
    ap.add_argument("--resolution", type=int, nargs="+", default=[256], metavar="N", help="lattice points per axis: one number or three (512: the reference's depth 9)")
    ap.add_argument("--num-points", type=int, default=1_000_000)
    ap.add_argument("--std-ratio", type=float, default=10.0, help="outlier threshold of the cloud in standard deviations of the neighbour means")
    ap.add_argument("--no-remove-outliers", dest="remove_outliers", action="store_false")
    ap.add_argument("--normals-knn", type=int, default=30, help="points per normal neighbourhood (3..32)")
    ap.add_argument("--bounding-box-min", type=float, nargs=3, default=(-1.0, -1.0, -1.0), metavar=("X", "Y", "Z"))
    ap.add_argument("--bounding-box-max", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("X", "Y", "Z"))
    ap.add_argument("--no-density-normalize", dest="density_normalize", action="store_false", help="weigh every point 1 instead of 1 / density")
    ap.add_argument("--density-downscale", type=int, default=4, help="the density lattice has 1 / this many points per axis")
    ap.add_argument("--screening", type=float, default=0.0, help="lumped diagonal screening (0: none)")
    ap.add_argument("--tol", type=float, default=1e-3, help="relative residual at which conjugate gradients stop")
    ap.add_argument("--max-iterations", type=int, default=None, metavar="N", help="iteration cap (default: 4 x the largest dimension)")
    ap.add_argument("--trim-quantile", type=float, default=0.1, help="remove vertices below this quantile of the density (0: keep the closed mesh)")
    ap.add_argument("--target-num-faces", type=int, default=None, metavar="N", help="simplify the mesh to at most N faces (the reference's default: 50000)")
    ap.add_argument("--save-point-cloud", action="store_true", help="also write the oriented cloud as point_cloud.ply")
    ap.add_argument("--save-world-frame", dest="save_world_frame", action="store_true", default=True, help="write the mesh in the dataset's frame (default)")
    ap.add_argument("--no-save-world-frame", dest="save_world_frame", action="store_false", help="write it in the model's frame")
    ap.add_argument("--ascii", action="store_true", help="write an ASCII PLY")
    ap.add_argument("--texture", default="none", choices=("none", "nerf", "vertex"), help="also write a textured OBJ: baked from the NeRF or from the vertices")
    ap.add_argument("--px-per-uv-triangle", type=int, default=4, metavar="PX", help="texels along a face's triangle in the atlas (at least 2)")
    ap.add_argument("--usemtl", default="rgb", choices=("rgb", "thermal"), help="the material the OBJ uses: the colour or the thermal texture")
    ap.add_argument("--chunk", type=int, default=None, metavar="N", help="texels rendered per call (default: the model's eval_num_rays_per_chunk)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if len(args.resolution) not in (1, 3):
        ap.error("--resolution takes one number or three")
    if args.target_num_faces is not None and args.target_num_faces < 0:
        ap.error("--target-num-faces takes a number >= 0")
    if not 0.0 <= args.trim_quantile <= 1.0 or args.screening < 0:
        ap.error("--trim-quantile takes a number in 0..1, --screening a number >= 0")
    if args.from_ply is not None and args.texture == "nerf":
        ap.error("--texture nerf renders rays through the radiance field: use --texture vertex with --from-ply")
    if args.px_per_uv_triangle < 2 or (args.chunk is not None and args.chunk < 1):
        ap.error("--px-per-uv-triangle takes a number >= 2, --chunk a number >= 1")
    return args


def cloud_from_ply(path, dev):
    """A PLY with normals -> PointCloud on the device (colours and temperatures 0 where the file has none)."""
    import torch

    from nerfstudio_thermal_amd.cloud import PointCloud
    from nerfstudio_thermal_amd.dataparser import read_ply_normals, read_ply_thermal

    normals = read_ply_normals(path)
    if normals is None:
        raise SystemExit(f"{path}: no nx ny nz properties (scripts/export_point_cloud.py --normal-method knn writes them)")
    xyz, rgb, thermal = read_ply_thermal(path)
    n = xyz.shape[0]
    f = lambda a, w: (torch.from_numpy(a.astype("float32") / 255.0) if a is not None and a.shape[0] == n else torch.zeros(n, w)).reshape(n, w).to(dev)  # noqa: E731
    return PointCloud(torch.from_numpy(xyz.astype("float32")).to(dev), f(rgb, 3), f(thermal, 1), None, torch.from_numpy(normals).to(dev))


def main(argv=None):
    args = parse_args(argv)
    import torch

    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import cloud, mesh, poisson

    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    os.makedirs(args.output_dir, exist_ok=True)
    sync = torch.cuda.synchronize
    resolution = args.resolution[0] if len(args.resolution) == 1 else list(args.resolution)
    box = (tuple(args.bounding_box_min), tuple(args.bounding_box_max))
    model = outputs = meta = None
    report = {}
    if args.from_ply is not None:
        t0 = time.perf_counter()
        pc = cloud_from_ply(args.from_ply, dev)
        report.update(source=args.from_ply, read_seconds=time.perf_counter() - t0)
    else:
        from nerfstudio_thermal_amd.config import ThermalNerfactoModelConfig
        from nerfstudio_thermal_amd.pipeline import ThermalPipeline
        from nerfstudio_thermal_amd.rays import RayBundle
        from nerfstudio_thermal_amd.splat_camera import OrientedBox

        data = args.data
        if data is None:
            from train_eval_scene import write_cube_scene

            data = os.path.join(args.output_dir, "scene")
            write_cube_scene(data, args.frames, dev)
        pipe = ThermalPipeline(data, ThermalNerfactoModelConfig(density_mode=args.density_mode), device=dev, seed=args.seed)
        sync(); t0 = time.perf_counter()
        if args.iterations > 0:
            pipe.train(args.iterations)
        sync(); train_s = time.perf_counter() - t0
        model, outputs = pipe.model, pipe.train_outputs
        meta = json.load(open(os.path.join(data, "transforms.json"), encoding="utf-8"))

        def next_rays():
            o, d, cam, _, _ = pipe.datamanager.next_train(0)
            return RayBundle(origins=o, directions=d, pixel_area=torch.ones_like(o[:, :1]), camera_indices=cam[:, None])

        lo, hi = torch.tensor(box[0], dtype=torch.float64), torch.tensor(box[1], dtype=torch.float64)
        t1 = time.perf_counter()
        pc = cloud.generate_point_cloud(model, next_rays, num_points=args.num_points, remove_outliers=args.remove_outliers, std_ratio=args.std_ratio,
                                        box=OrientedBox.from_params(tuple(((lo + hi) / 2).tolist()), (0.0, 0.0, 0.0), tuple((hi - lo).tolist())),
                                        estimate_normals=True, normals_knn=args.normals_knn)
        sync()
        report.update(dataset=data if args.data is not None else f"generated cube scene ({data})", iterations=args.iterations, train_seconds=train_s,
                      point_cloud_seconds=time.perf_counter() - t1)
    world = outputs if (args.save_world_frame and outputs is not None) else None
    applied = None if meta is None else meta.get("applied_transform")
    if args.save_point_cloud:
        xyz = cloud.to_dataset_frame(pc.xyz, world, applied) if world is not None else pc.xyz
        nrm = cloud.normals_to_dataset_frame(pc.normals, world, applied) if world is not None else None
        report["point_cloud"] = cloud.write_cloud_ply(os.path.join(args.output_dir, "point_cloud.ply"), pc, xyz, binary=not args.ascii, normals=nrm)
    sync(); t2 = time.perf_counter()
    m, volume = poisson.poisson_reconstruct(pc, resolution, box, density_normalize=args.density_normalize, density_downscale=args.density_downscale,
                                            screening=args.screening, tol=args.tol, max_iterations=args.max_iterations,
                                            trim_quantile=args.trim_quantile, return_volume=True)
    sync(); reconstruct_s = time.perf_counter() - t2
    iterations, rr, bb = volume.solve_record
    report.update(points=len(pc), lattice=list(volume.dims), cg_iterations=iterations, relative_residual=(rr / bb) ** 0.5 if bb > 0 else 0.0,
                  iso=volume.iso, trim_quantile=args.trim_quantile, vertices_extracted=int(m.vertices.shape[0]), faces_extracted=int(m.faces.shape[0]),
                  reconstruct_seconds=reconstruct_s)
    if args.target_num_faces is not None:
        ts = time.perf_counter()
        m, cell = mesh.simplify_to_target(m, args.target_num_faces, volume.voxel_size, origin=mesh.lattice_centred_origin(volume))
        sync()
        report.update(target_num_faces=args.target_num_faces, simplify_cell=None if cell is None else list(cell), simplify_seconds=time.perf_counter() - ts)
    t3 = time.perf_counter()
    ply = mesh.write_mesh_ply(os.path.join(args.output_dir, "poisson_mesh.ply"), m, binary=not args.ascii, dataparser_outputs=world,
                              applied_transform=applied)
    report.update(vertices=int(m.vertices.shape[0]), faces=int(m.faces.shape[0]), write_seconds=time.perf_counter() - t3,
                  frame="dataset" if world is not None else ("file" if args.from_ply is not None else "model"), ply=ply)
    if args.texture != "none" and int(m.faces.shape[0]) > 0:
        from nerfstudio_thermal_amd import texture

        t4 = time.perf_counter()
        tex = texture.bake_texture(m, model, args.px_per_uv_triangle, source=args.texture, chunk=args.chunk)
        sync(); bake_s = time.perf_counter() - t4
        paths = texture.write_textured_obj(args.output_dir, m, tex, dataparser_outputs=world, applied_transform=applied, usemtl=args.usemtl)
        report.update(texture=args.texture, px_per_uv_triangle=args.px_per_uv_triangle, texture_size=[int(tex.rgb.shape[1]), int(tex.rgb.shape[0])],
                      bake_seconds=bake_s, obj=paths["obj"])
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
