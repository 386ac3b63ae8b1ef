"""tn_cloud_estimate_normals at 10^5 and 10^6 points for knn = 30 (the reference's default, a list of 31) and knn = 10 (a list of 15), beside
tn_cloud_remove_outliers on the same cloud (nb_neighbors = 20, the reference's, a list of 19 -- and nb_neighbors = 32, the same list of 31 that
knn = 30 searches with, which separates the cost of the wide search from the cost of the covariance and the eigenvector): the surface cloud of tests/knn_functional.cloud (points on three
planes, 30 % of them in 64 tight clusters) and a uniform one.  HIP events on torch's current stream around each call alone (workspace and
outputs allocated once); the calls alternate inside every repeat; median, min and max of NORMALS_ITERS repeats after warm-up.  One JSON line with
milliseconds per call, the ratios to the two outlier calls at the same n, and nanoseconds per point.
For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_cloud_normals.py` (NORMALS_ITERS=3)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import knn_functional as kf  # noqa: E402

ITERS = int(os.environ.get("NORMALS_ITERS", 10))
SIZES = [int(s) for s in os.environ.get("NORMALS_SIZES", "100000,1000000").split(",")]
KNNS = (30, 10)
NB, NB_WIDE = 20, 32


def main():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import _lib
    from nerfstudio_thermal_amd.ops import _stream

    lib = _lib.load()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    res = {"iters": ITERS, "device": torch.cuda.get_device_name(0), "nb_neighbors": [NB, NB_WIDE], "ms": {}}
    for kind in ("surface", "uniform"):
        for n in SIZES:
            p = kf.cloud(kind, n, seed=7).cuda()
            view = torch.nn.functional.normalize(p - torch.tensor([0.0, 0.0, 5.0], device="cuda"), dim=-1).contiguous()
            rgb, th = torch.rand(n, 3, device="cuda"), torch.rand(n, 1, device="cuda")
            normals = torch.empty(n, 3, device="cuda")
            out = [torch.empty(n, w, device="cuda") for w in (3, 3, 1)]
            count, stats = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.empty(3, dtype=torch.float64, device="cuda")
            need_n = {k: int(lib.tn_cloud_normals_workspace_bytes(n, k)) for k in KNNS}
            need_o = {nb: int(lib.tn_cloud_remove_outliers_workspace_bytes(n, nb)) for nb in (NB, NB_WIDE)}
            ws = torch.empty(max(*need_o.values(), *need_n.values()), dtype=torch.uint8, device="cuda")

            def normals_call(knn, with_view=True):
                _lib.check(lib.tn_cloud_estimate_normals(ptr(p), n, knn, ptr(view) if with_view else None, ptr(normals), ptr(ws), need_n[knn], _stream()))

            def outliers_call(nb):
                _lib.check(lib.tn_cloud_remove_outliers(ptr(p), ptr(rgb), ptr(th), n, nb, 10.0, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(count),
                                                        ptr(stats), None, None, ptr(ws), need_o[nb], _stream()))

            calls = {**{f"outliers_nb{nb}": (lambda nb=nb: outliers_call(nb)) for nb in (NB, NB_WIDE)},
                     **{f"normals_knn{k}": (lambda k=k: normals_call(k)) for k in KNNS}}
            for _ in range(2):
                for f in calls.values():
                    f()
            torch.cuda.synchronize()
            ts = {name: [] for name in calls}
            for _ in range(ITERS):
                for name, f in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    torch.cuda.synchronize()
                    ts[name].append(e0.elapsed_time(e1))
            row = {}
            for name, t in ts.items():
                t.sort()
                row[name] = {"median": t[len(t) // 2], "min": t[0], "max": t[-1], "ns_per_point": 1e6 * t[len(t) // 2] / n}
            for k in KNNS:
                row[f"normals_knn{k}"]["ratio_to_outliers"] = row[f"normals_knn{k}"]["median"] / row[f"outliers_nb{NB}"]["median"]
                row[f"normals_knn{k}"]["ratio_to_outliers_wide"] = row[f"normals_knn{k}"]["median"] / row[f"outliers_nb{NB_WIDE}"]["median"]
            res["ms"][f"{kind}_{n}"] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
