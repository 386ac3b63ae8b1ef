"""Times the stages of poisson.poisson_reconstruct on a synthetic oriented cloud (a sphere of radius 0.6 and a floor plane z = -0.7, exact normals,
1e-3 noise; seeded), each stage alone between HIP events on torch's stream after a warm-up pass: the plan (tn_poisson_bin), the three splats, the
divergence, the solve (iterations, seconds per iteration), the extraction, the projection of the vertices and the trim.  Prints one JSON line per resolution.

    python scripts/time_poisson_mesh.py [--points 1000000] [--resolutions 256 512] [--repeats 5] [--tol 1e-3]

Beside the solve's time per iteration it prints the bytes an iteration must move -- 11 arrays of X Y Z floats: p -> A p; x p r A p -> x r;
r p -> p -- and their share of the 8 TB/s stream rate.  An observation, not a gate; there is no reference time to compare with.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STREAM_RATE = 8.0e12  # bytes per second
ARRAYS_PER_ITERATION = 11


def synthetic_cloud(n, dev, seed=0):
    import torch

    g = torch.Generator().manual_seed(seed)
    k = (2 * n) // 3
    d = torch.nn.functional.normalize(torch.randn((k, 3), generator=g, dtype=torch.float64), dim=1)
    plane = torch.cat([torch.rand((n - k, 2), generator=g, dtype=torch.float64) * 1.8 - 0.9, torch.full((n - k, 1), -0.7, dtype=torch.float64)], 1)
    xyz = torch.cat([0.6 * d, plane]) + 1e-3 * torch.randn((n, 3), generator=g, dtype=torch.float64)
    nrm = torch.cat([d, torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64).repeat(n - k, 1)])
    rgbt = torch.rand((n, 4), generator=g)
    return xyz.float().to(dev), nrm.float().to(dev), rgbt.to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-3)
    args = ap.parse_args(argv)
    import torch

    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import mesh, poisson

    assert torch.cuda.is_available(), "timing needs the GPU: there is no fallback"
    dev = torch.device("cuda", 0)
    xyz, nrm, rgbt = synthetic_cloud(args.points, dev)
    n = xyz.shape[0]
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))

    def timed(fn, repeats=args.repeats):
        fn()  # warm-up: code objects, allocator
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return out, {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    for res in args.resolutions:
        grid = poisson.Grid.over_box(box, res)
        coarse = poisson.Grid.over_box(box, max(res // 4, 2))
        total = res ** 3
        ws, ws_c = poisson.plan_workspace(n, grid, dev), poisson.plan_workspace(n, coarse, dev)
        report = {"points": n, "lattice": [res] * 3}
        _, report["bin"] = timed(lambda: poisson.bin_call(xyz, grid, ws))
        poisson.bin_call(xyz, coarse, ws_c)
        density_c = poisson.splat(xyz, coarse, ws_c)
        weights = (1.0 / poisson.sample(xyz, density_c, coarse).clamp_min(poisson.DENSITY_FLOOR)).float()
        density, report["splat_density"] = timed(lambda: poisson.splat(xyz, grid, ws))
        field, report["splat_normals"] = timed(lambda: poisson.splat(xyz, grid, ws, nrm, weights))
        colours, report["splat_rgbt_normalised"] = timed(lambda: poisson.splat(xyz, grid, ws, rgbt, None, normalize=True))
        b = torch.empty(grid.dims, device=dev)
        _, report["divergence"] = timed(lambda: poisson.divergence_call(field, grid, b))
        del field
        sws = poisson.solve_workspace(grid, dev)
        chi = torch.zeros(grid.dims, device=dev)

        def solve():
            chi.zero_()
            return poisson.solve_call(b, None, chi, grid, args.tol, 4 * res, 25, sws)

        (iterations, rr, bb), t = timed(solve, max(1, min(args.repeats, 3)))
        per_it = t["median_ms"] / max(iterations, 1)
        moved = ARRAYS_PER_ITERATION * 4 * total
        report["solve"] = dict(t, iterations=iterations, relative_residual=(rr / bb) ** 0.5, ms_per_iteration=per_it, bytes_per_iteration=moved,
                               stream_bound_ms=moved / STREAM_RATE * 1e3, share_of_stream_rate=moved / STREAM_RATE * 1e3 / per_it)
        values, _ = poisson.level_volume(chi, poisson.sample(xyz, chi, grid), weights, poisson.kept_mask(xyz, grid))
        volume = mesh.TSDFVolume(torch.from_numpy(grid.origin), torch.from_numpy(grid.voxel), (2, 2, 2), device=dev)
        volume.dims, volume.values, volume.weights, volume.rgbt = grid.dims, values, (density > 0).float(), colours
        m, report["extract"] = timed(volume.get_mesh, max(1, min(args.repeats, 3)))
        _, report["project"] = timed(lambda: poisson.project_vertices(m.vertices, values, grid, 2))
        trimmed, report["trim"] = timed(lambda: poisson.trim_mesh(m, poisson.sample(m.vertices, density_c, coarse), 0.1))
        report.update(vertices=int(m.vertices.shape[0]), faces=int(m.faces.shape[0]), vertices_trimmed=int(trimmed.vertices.shape[0]),
                      faces_trimmed=int(trimmed.faces.shape[0]), peak_memory_gib=torch.cuda.max_memory_allocated() / 2 ** 30)
        print(json.dumps(report), flush=True)
        del ws, ws_c, density, colours, b, sws, chi, values, volume, m, trimmed
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
