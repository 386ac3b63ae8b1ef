"""The point-cloud export at 1 M points (profiles/nerf_point_cloud.md): thermal-nerfacto trained on the generated RGB+T cube scene, then the export
timed stage by stage -- render, append, outlier removal -- on the HIP path (cloud.append_points / cloud.remove_outliers) and, beside it on the same
device and the same rays, as the reference writes the loop: `point[mask]` boolean indexing per batch, one `torch.cat` at the end
(exporter_utils.py:163-197), and the neighbour means of the outlier rule from scipy's cKDTree on the host (Open3D is not a dependency).

    python scripts/time_point_cloud.py [--iterations 3000] [--num-points 1000000] [--repeats 3] [--no-yardstick]

Render and append times are HIP events around every batch's calls, summed; whole stages are a host clock around work that ends in a device
synchronise.  Every stage is warmed up on a small export first.  One JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import cloud  # noqa: E402
from nerfstudio_thermal_amd.pipeline import ThermalPipeline  # noqa: E402
from nerfstudio_thermal_amd.rays import RayBundle  # noqa: E402
from train_eval_scene import write_cube_scene  # noqa: E402


def _events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def gather_hip(model, next_rays, num_points, box):
    """generate_point_cloud's loop with events around the render and the append of every batch -> (buffers, stats)"""
    buf = cloud.PointCloud.empty(num_points, model.device)
    count = torch.zeros(1, dtype=torch.int64, device=model.device)
    crop = box.crop_struct()
    pairs, batches, rays, have = [], 0, 0, 0
    torch.cuda.synchronize(); t0 = time.perf_counter()
    with torch.no_grad():
        while have < num_points:
            rb = next_rays()
            a0, a1 = _events(); b0, b1 = _events()
            a0.record(); out = model(rb); a1.record()
            b0.record(); cloud.append_points(out, rb, buf, count, crop); b1.record()
            pairs.append((a0, a1, b0, b1))
            batches, rays = batches + 1, rays + len(rb)
            if batches % 8 == 0:
                have = int(count.item())
    torch.cuda.synchronize(); wall = time.perf_counter() - t0
    return buf, {"batches": batches, "rays": rays, "keep_rate": num_points / rays, "wall_s": wall,
                 "render_event_s": sum(a.elapsed_time(b) for a, b, _, _ in pairs) / 1e3, "append_event_s": sum(a.elapsed_time(b) for _, _, a, b in pairs) / 1e3}


def gather_torch(model, next_rays, num_points):
    """the reference's loop: boolean indexing per batch (each `point.shape[0]` is a host synchronisation, as progress.advance's is), cat at the end"""
    points, rgbs, thermals, pairs, have, batches, rays = [], [], [], [], 0, 0, 0
    lo, hi = torch.tensor([-1.0, -1, -1], device=model.device), torch.tensor([1.0, 1, 1], device=model.device)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    with torch.no_grad():
        while have < num_points:
            rb = next_rays()
            a0, a1 = _events(); b0, b1 = _events()
            a0.record(); out = model(rb); a1.record()
            b0.record()
            point = rb.origins + rb.directions * out["depth"]
            mask = out["accumulation"][..., 0] > 0.5
            point, rgb, th = point[mask], out["rgb"][mask], out["rgb_thermal"][mask]
            mask = torch.all(torch.concat([point > lo, point < hi], dim=-1), dim=-1)
            point, rgb, th = point[mask], rgb[mask], th[mask]
            b1.record()
            points.append(point); rgbs.append(rgb); thermals.append(th)
            pairs.append((a0, a1, b0, b1))
            have += point.shape[0]
            batches, rays = batches + 1, rays + len(rb)
        c0, c1 = _events()
        c0.record()
        pc = cloud.PointCloud(torch.cat(points)[:num_points], torch.cat(rgbs)[:num_points], torch.cat(thermals)[:num_points])
        c1.record()
    torch.cuda.synchronize(); wall = time.perf_counter() - t0
    return pc, {"batches": batches, "rays": rays, "wall_s": wall, "render_event_s": sum(a.elapsed_time(b) for a, b, _, _ in pairs) / 1e3,
                "index_event_s": sum(a.elapsed_time(b) for _, _, a, b in pairs) / 1e3, "cat_event_s": c0.elapsed_time(c1) / 1e3}


def outliers_scipy(pc, nb, std_ratio, workers):
    """Open3D's rule with the neighbour search on the host: the copy to the host, cKDTree over float64 points, the statistics in numpy"""
    from scipy.spatial import cKDTree

    torch.cuda.synchronize(); t0 = time.perf_counter()
    pts = pc.xyz.double().cpu().numpy()
    t1 = time.perf_counter()
    dist, _ = cKDTree(pts).query(pts, k=nb, workers=workers)
    t2 = time.perf_counter()
    mean = dist.sum(1) / nb
    pos = mean[mean > 0]
    thr = pos.mean() + std_ratio * pos.std(ddof=1)
    keep = torch.from_numpy((mean > 0) & (mean < thr)).to(pc.xyz.device)
    out = pc[keep]
    torch.cuda.synchronize(); t3 = time.perf_counter()
    return out, {"kept": len(out), "copy_s": t1 - t0, "ckdtree_s": t2 - t1, "stats_and_mask_s": t3 - t2, "wall_s": t3 - t0, "thr": float(thr)}


def outliers_hip(pc, nb, std_ratio):
    d = {}
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = cloud.remove_outliers(pc, nb, std_ratio, d)
    torch.cuda.synchronize()
    return out, {"kept": len(out), "wall_s": time.perf_counter() - t0, "thr": float(d["stats"][2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=3000)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--num-points", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--std-ratio", type=float, default=10.0)
    ap.add_argument("--workers", type=int, default=16, help="threads of the cKDTree query")
    ap.add_argument("--no-yardstick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_point_cloud.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as data:
        write_cube_scene(data, args.frames, dev)
        pipe = ThermalPipeline(data, device=dev)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        pipe.train(args.iterations)
        torch.cuda.synchronize(); train_s = time.perf_counter() - t0
    model = pipe.model
    model.eval()

    def next_rays():
        o, d, cam, _, _ = pipe.datamanager.next_train(0)
        return RayBundle(origins=o, directions=d, pixel_area=torch.ones_like(o[:, :1]), camera_indices=cam[:, None])

    box = cloud.default_box()
    warm, _ = gather_hip(model, next_rays, 50_000, box)  # warm-up of every shape and code object the timed windows use
    outliers_hip(warm, 20, args.std_ratio)
    if not args.no_yardstick:
        warm_t, _ = gather_torch(model, next_rays, 50_000)
        outliers_scipy(warm_t, 20, args.std_ratio, args.workers)
    runs = []
    for _ in range(args.repeats):  # the two paths alternate
        buf, g = gather_hip(model, next_rays, args.num_points, box)
        _, o = outliers_hip(buf, 20, args.std_ratio)
        run = {"hip": {"gather": g, "remove_outliers": o, "total_s": g["wall_s"] + o["wall_s"]}}
        if not args.no_yardstick:
            pc, gt = gather_torch(model, next_rays, args.num_points)
            _, ot = outliers_scipy(pc, 20, args.std_ratio, args.workers)
            # the same cloud through both outlier rules: float32 device distances against float64 host distances
            _, oh = outliers_hip(pc, 20, args.std_ratio)
            run["torch_scipy"] = {"gather": gt, "remove_outliers": ot, "total_s": gt["wall_s"] + ot["wall_s"], "hip_rule_on_the_same_cloud": oh}
        runs.append(run)
    print(json.dumps({"scene": "generated cube scene", "frames_per_spectrum": args.frames, "iterations": args.iterations, "train_seconds": train_s,
                      "num_points": args.num_points, "rays_per_batch": pipe.datamanager.num_rays, "std_ratio": args.std_ratio, "ckdtree_workers": args.workers,
                      "runs": runs}))


if __name__ == "__main__":
    main()
