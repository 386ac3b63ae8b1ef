"""The Gaussian-splat PLY export at 1 M Gaussians (profiles/splat_export.md): degree 3, separate thermal opacity, spectrum "both", timed stage by
stage -- the pack launches (tn_export_splat_pack), the device-to-host copy of the kept rows, the file write -- and, beside it on the same
parameters, the reference's way of assembling the same table (exporter.py:497-542): one `.cpu().numpy()` per attribute, a column per property,
the finite filter column by column, and a host-side column stack where the reference hands its dict to Open3D's writer (Open3D is not a dependency
of this project; its write is not timed, this project's `tofile` of the stacked table stands in for it).

    python scripts/time_splat_export.py [--gaussians 1000000] [--sh-degree 3] [--repeats 5] [--dead 0.03] [--output-dir DIR]

--dead is the share of Gaussians given an opacity far below --min-opacity (a fixed-budget MCMC run keeps such Gaussians); a few more get a NaN.
The pack is timed with HIP events around its three launches; copy and write with a host clock (the copy ends in a synchronise).  Everything is
warmed up once.  The byte floor of the pack is (bytes of the parameters read + one flag byte written and read per Gaussian + count * W * 4 bytes
written) at the 6.29 TB/s of a float4 copy.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import splat_io  # noqa: E402
from nerfstudio_thermal_amd.splat_calls import param_names  # noqa: E402

COPY_BYTES_PER_S = 6.29e12  # float4 copy, measured (the HBM figure this project's profiles use)


def make_params(n, K, dead, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    p = {"means": r(n, 3), "scales": r(n, 3) - 3.0, "quats": torch.nn.functional.normalize(r(n, 4), dim=-1), "opacities": 2.0 * r(n, 1) + 1.0,
         "features_dc": r(n, 3), "features_rest": 0.1 * r(n, K - 1, 3), "features_dc_thermal": r(n, 1), "features_rest_thermal": 0.1 * r(n, K - 1, 1),
         "opacities_thermal": 2.0 * r(n, 1) + 1.0}
    is_dead = torch.rand(n, generator=g, device=dev) < dead
    p["opacities"][is_dead] = -12.0
    p["opacities_thermal"][is_dead] = -12.0
    p["features_rest"][:: max(n // 97, 1), 3, 1] = float("nan")
    return p


def reference_table(p):
    """exporter.py:497-542 with the thermal attributes added the same way: a host array per attribute, a [n,1] column per property, the finite filter
    over the columns, the selected columns stacked into the table the writer needs."""
    cols = {}
    positions = p["means"].cpu().numpy()
    n = positions.shape[0]
    cols["positions"] = positions
    cols["normals"] = np.zeros_like(positions, dtype=np.float32)
    shs_0 = p["features_dc"].contiguous().cpu().numpy()
    for i in range(3):
        cols[f"f_dc_{i}"] = shs_0[:, i, None]
    rest = p["features_rest"].transpose(1, 2).contiguous().cpu().numpy().reshape((n, -1))
    for i in range(rest.shape[-1]):
        cols[f"f_rest_{i}"] = rest[:, i, None]
    cols["opacity"] = p["opacities"].cpu().numpy()
    scales = p["scales"].cpu().numpy()
    for i in range(3):
        cols[f"scale_{i}"] = scales[:, i, None]
    quats = p["quats"].cpu().numpy()
    for i in range(4):
        cols[f"rot_{i}"] = quats[:, i, None]
    cols["f_dc_thermal"] = p["features_dc_thermal"].cpu().numpy()
    rest_th = p["features_rest_thermal"].contiguous().cpu().numpy().reshape((n, -1))
    for i in range(rest_th.shape[-1]):
        cols[f"f_rest_thermal_{i}"] = rest_th[:, i, None]
    cols["opacity_thermal"] = p["opacities_thermal"].cpu().numpy()
    select = np.ones(n, dtype=bool)
    for t in cols.values():
        select = np.logical_and(select, np.isfinite(t).all(axis=1))
    if np.sum(select) < n:
        for k in cols:
            cols[k] = cols[k][select, :]
    return np.concatenate(list(cols.values()), axis=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dead", type=float, default=0.03)
    ap.add_argument("--min-opacity", type=float, default=0.005)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--output-dir", default=None, help="where the timed files are written (default: a temporary directory)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_splat_export.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda", 0)
    n, K = args.gaussians, (args.sh_degree + 1) ** 2
    p = make_params(n, K, args.dead, dev)
    tensors = [p[k].contiguous() for k in param_names("separate")]
    props = splat_io.ply_properties("both", K, True)
    W = len(props)
    logit = splat_io.opacity_logit(args.min_opacity)
    out = torch.empty((n, W), device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(splat_io._lib.load().tn_export_splat_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    tmp = tempfile.TemporaryDirectory() if args.output_dir is None else None
    outdir = tmp.name if tmp is not None else args.output_dir
    os.makedirs(outdir, exist_ok=True)
    path = os.path.join(outdir, "splat.ply")

    def one(run_yardstick):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        splat_io.pack_call(tensors, 2, 0, logit, None, out, count, ws)
        e1.record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kept = int(count.item())
        rows = out[:kept].cpu().numpy()
        t1 = time.perf_counter()
        splat_io.write_gaussian_ply(path, rows, props)
        t2 = time.perf_counter()
        r = {"kept": kept, "pack_s": e0.elapsed_time(e1) / 1e3, "copy_s": t1 - t0, "write_s": t2 - t1}
        if run_yardstick:
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            table = reference_table(p)
            t4 = time.perf_counter()
            splat_io.write_gaussian_ply(os.path.join(outdir, "reference_way.ply"), table, props)
            t5 = time.perf_counter()
            # the reference has no opacity threshold: the tables agree where only the finite filter ran
            r.update(reference_assemble_s=t4 - t3, reference_write_s=t5 - t4, reference_rows=int(table.shape[0]))
        return r

    one(not args.no_yardstick)  # warm-up
    runs = [one(not args.no_yardstick) for _ in range(args.repeats)]
    kept = runs[0]["kept"]
    read_bytes = sum(t.numel() * 4 for t in tensors) + 2 * n
    floor_s = (read_bytes + kept * W * 4) / COPY_BYTES_PER_S
    med = lambda k: statistics.median(r[k] for r in runs)  # noqa: E731
    summary = {k: med(k) for k in runs[0] if k.endswith("_s")}
    summary.update(min_pack_s=min(r["pack_s"] for r in runs), max_pack_s=max(r["pack_s"] for r in runs))
    print(json.dumps({"gaussians": n, "sh_degree": args.sh_degree, "mode": "separate", "spectrum": "both", "row_floats": W, "kept": kept,
                      "dropped": n - kept, "min_opacity": args.min_opacity, "file_bytes": os.path.getsize(path), "repeats": args.repeats,
                      "pack_bytes_read": read_bytes, "pack_bytes_written": kept * W * 4, "pack_floor_s_at_6.29TBps": floor_s,
                      "pack_over_floor": med("pack_s") / floor_s, "median": summary, "runs": runs}))
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
