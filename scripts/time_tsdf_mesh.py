"""The TSDF fusion and the surface extraction at export sizes (profiles/tsdf_mesh.md): `TSDFVolume.integrate` of 10 frames of 640 x 480 into a 128^3 and
a 256^3 volume (tn_tsdf_integrate, one launch), then `get_mesh` of the result (tn_mesh_count + tn_mesh_emit), each against the plain-torch float32
restatement of tests/tsdf_functional.py on the same device -- the reference's algorithm: per frame a handful of whole-volume temporaries, then
masked updates of the volume.  The scene is the tests' analytic one (a sphere of radius 0.6 seen from a ring of cameras, accumulation 1 on it).

    python scripts/time_tsdf_mesh.py [--sizes 128 256] [--frames 10] [--repeats 20] [--warmup 3] [--torch-repeats 5] [--no-torch]

Times are HIP events around one call after warm-up, the median of --repeats (the spread is reported too).  Every integrate call starts from a
fresh volume, reset outside the events; `integrate` includes building the camera records on the host and copying them.  Bytes are what the
algorithm has to move: a fused voxel reads and writes its value, weight and RGB+T (2 x 24 bytes), the extraction reads the values twice and writes
its outputs; the share of the HBM roofline is those bytes over the time against 8 TB/s.  Peak temporary memory is torch's allocator high-water
mark above the inputs (the kernels' own scratch is the mesh workspace).  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
import tsdf_functional as tf  # noqa: E402
from nerfstudio_thermal_amd import mesh  # noqa: E402
from nerfstudio_thermal_amd.splat_camera import PinholeCamera  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def timed(fn, repeats, warmup, setup=None):
    """-> (median ms, min ms, max ms, peak bytes allocated above the start) of fn() by HIP events; setup() runs before each call, outside the events"""
    for _ in range(warmup):
        if setup is not None:
            setup()
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if setup is not None:
            setup()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms), torch.cuda.max_memory_allocated() - base


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the HIP path only")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "time_tsdf_mesh.py needs a GPU"
    dev = torch.device("cuda", 0)
    B, H, W = args.frames, args.height, args.width
    c2w, intr = tf.scene_cameras(B, H, W, seed=0)
    c2w, intr = c2w.float(), intr.float()
    depth, rgbt, acc = (t.to(dev) for t in tf.sphere_frames(c2w.double(), intr.double(), H, W, seed=0))
    cams = [PinholeCamera(c2w[b], *(float(v) for v in intr[b]), W, H) for b in range(B)]
    records = tf.camera_records(c2w, intr).to(dev)
    results = []
    for n in args.sizes:
        vol = mesh.TSDFVolume.from_aabb([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], (n, n, n), device=dev)
        fresh = (vol.values.clone(), vol.weights.clone(), vol.rgbt.clone())

        def reset():
            vol.values.copy_(fresh[0]), vol.weights.copy_(fresh[1]), vol.rgbt.copy_(fresh[2])

        hip = timed(lambda: vol.integrate(cams, depth, rgbt, acc), args.repeats, args.warmup, setup=reset)
        touched = int((vol.weights > 0).sum())
        fused_bytes = 48 * touched
        r = {"volume": n, "frames": B, "frame_size": [W, H], "observed_voxels": touched, "integrate_bytes": fused_bytes, "integrate_hip_ms": hip[0],
             "integrate_hip_ms_min_max": [hip[1], hip[2]], "integrate_hip_peak_temporary_bytes": hip[3],
             "integrate_hip_roofline_share": fused_bytes / (hip[0] * 1e-3) / HBM_PEAK}
        m = vol.get_mesh()
        V, Fn = int(m.vertices.shape[0]), int(m.faces.shape[0])
        mesh_hip = timed(lambda: vol.get_mesh(), args.repeats, args.warmup)
        mesh_bytes = 2 * 4 * n ** 3 + V * (12 + 12 + 16) + Fn * 12
        r.update({"vertices": V, "faces": Fn, "mesh_bytes": mesh_bytes, "mesh_hip_ms": mesh_hip[0], "mesh_hip_ms_min_max": [mesh_hip[1], mesh_hip[2]],
                  "mesh_hip_peak_temporary_bytes": mesh_hip[3], "mesh_hip_roofline_share": mesh_bytes / (mesh_hip[0] * 1e-3) / HBM_PEAK})
        if not args.no_torch:
            origin, voxel = vol.origin.to(dev), vol.voxel_size.to(dev)
            fused = (vol.values.clone(), vol.weights.clone(), vol.rgbt.clone())
            tor = timed(lambda: tf.integrate_ref(*fresh, origin, voxel, vol.truncation, 1.0, records, depth, rgbt, acc, 0.5, "ray", dtype=torch.float32),
                        args.torch_repeats, 1)
            got = tf.integrate_ref(*fresh, origin, voxel, vol.truncation, 1.0, records, depth, rgbt, acc, 0.5, "ray", dtype=torch.float32)
            r.update({"integrate_torch_ms": tor[0], "integrate_torch_ms_min_max": [tor[1], tor[2]], "integrate_torch_peak_temporary_bytes": tor[3],
                      "integrate_speedup": tor[0] / hip[0],
                      "integrate_max_abs_difference": float((got[0] - fused[0]).abs().max()), "integrate_weights_differ": int((got[1] != fused[1]).sum())})
            del got
            try:
                tor = timed(lambda: tf.extract_ref(*fused, origin, voxel), args.torch_repeats, 1)
                want = tf.extract_ref(*fused, origin, voxel)
                r.update({"mesh_torch_ms": tor[0], "mesh_torch_ms_min_max": [tor[1], tor[2]], "mesh_torch_peak_temporary_bytes": tor[3],
                          "mesh_speedup": tor[0] / mesh_hip[0],
                          "mesh_equal": bool(torch.equal(want["vertices"], m.vertices) and torch.equal(want["faces"], m.faces) and torch.equal(want["normals"], m.normals))})
                del want
            except torch.cuda.OutOfMemoryError:  # the restatement keeps a dozen whole-volume index tensors
                r["mesh_torch_ms"] = "out of memory"
            del fused
        results.append(r)
        del vol, fresh, m
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "results": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
