"""Exact kNN (tn_knn, k = 3: splatfacto's seeding) at 50 k, 300 k, 1 M and 4 M points, for a uniform cloud and a surface cloud (points on
three planes, 30 % of them in 64 tight clusters: tests/knn_functional.cloud).  HIP events on torch's current stream around the tn_knn call
alone (workspace and outputs allocated once); median of KNN_ITERS after warm-up.  One JSON line.
  --sklearn   times scikit-learn's NearestNeighbors(n_neighbors=4).fit(x).kneighbors(x) on the same clouds instead (the reference's
              k_nearest_sklearn, on the host's CPUs; no GPU needed).
For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_splat_knn.py` (KNN_ITERS=3)."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import knn_functional as kf  # noqa: E402

iters = int(os.environ.get("KNN_ITERS", 10))
SIZES = [int(s) for s in os.environ.get("KNN_SIZES", "50000,300000,1000000,4000000").split(",")]
K = 3


def time_hip():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import _lib
    from nerfstudio_thermal_amd.ops import _stream

    lib = _lib.load()
    res = {"k": K, "iters": iters, "device": torch.cuda.get_device_name(0), "ms": {}}
    for kind in ("uniform", "surface"):
        for n in SIZES:
            p = kf.cloud(kind, n, seed=7).cuda()
            need = int(lib.tn_knn_workspace_bytes(n, K))
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            d = torch.empty((n, K), device="cuda")

            def call():
                _lib.check(lib.tn_knn(C.c_void_p(p.data_ptr()), n, K, C.c_void_p(d.data_ptr()), None, C.c_void_p(ws.data_ptr()), need, _stream()))

            for _ in range(2):
                call()
            ts = []
            for _ in range(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            ts.sort()
            res["ms"][f"{kind}_{n}"] = {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1], "workspace_mb": need / 2**20}
    return res


def time_sklearn():
    from sklearn.neighbors import NearestNeighbors

    res = {"k": K, "cpus": os.cpu_count(), "s": {}}
    for kind in ("uniform", "surface"):
        for n in SIZES:
            x = kf.cloud(kind, n, seed=7).numpy()
            t0 = time.perf_counter()
            NearestNeighbors(n_neighbors=K + 1).fit(x).kneighbors(x)
            res["s"][f"{kind}_{n}"] = time.perf_counter() - t0
    return res


if __name__ == "__main__":
    print(json.dumps(time_sklearn() if "--sklearn" in sys.argv else time_hip()))
