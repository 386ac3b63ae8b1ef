"""The splat backward with and without a depth upstream at the benchmark's splat shape (1 M synthetic Gaussians, 1920 x 1080, degree-3 SH, classic,
shared opacity; SPLAT_SEP=1: separate; SPLAT_ABS=1: with the absgrad statistic): device time of the raster backward (memset of the pair records,
k_splat_run_start, k_splat_raster_bwd, k_splat_pair_fold) plus the projection backward through splat_calls -- `off`, what a loss
without depth runs, against `depth`, tn_splat_raster_backward + tn_splat_project_backward with their depth groups on the same frame.  --parent-lib names
another build of the library with the same ABI (an earlier commit's): its backward without depth (`parent`) is timed in the same loop on the same workspace.
HIP events on torch's current stream; 4 back-to-back backwards per timed window, the variants alternated inside an iteration; every figure is the
median of SPLAT_ITERS iterations after warm-up, the whole measurement repeated SPLAT_REPEATS times and reported as [min, median, max] of those
medians (the in-process spread; run the script again for the process-to-process one).  The upstream images are random.  Also checks that the off
path's gradients are bit-equal between the two libraries, and that a zero depth upstream gives the off path's gradients.  One JSON line (also to
--out)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import _lib, splat, splat_calls, synth  # noqa: E402
from nerfstudio_thermal_amd.splat import PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig, camera_struct  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--parent-lib", default=None, help="libthermal_nerf_hip.so built from the parent commit")
args = ap.parse_args()
N = int(os.environ.get("SPLAT_N", 1_000_000))
iters = int(os.environ.get("SPLAT_ITERS", 20))
repeats = int(os.environ.get("SPLAT_REPEATS", 3))
sep = os.environ.get("SPLAT_SEP", "0") == "1"
absgrad = os.environ.get("SPLAT_ABS", "0") == "1"
BATCH = 4
H, W = 1080, 1920
dev = "cuda"
i32 = torch.int32

lib = _lib.load()
parent = None
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    for name in ("tn_splat_raster_backward", "tn_splat_backward_workspace_bytes", "tn_splat_project_backward"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
    parent.tn_last_error.restype = C.c_char_p

cam = PinholeCamera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 1400.0, 960.0, 540.0, W, H)
p = dict(synth.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5)))
if sep:
    p["opacities_thermal"] = p["opacities"] + 0.08 * torch.randn(N, 1, generator=torch.Generator().manual_seed(1))
m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(thermal_opacity_mode="separate" if sep else "shared"), num_points=4)
m.load_gaussians(p)
params = [m.gauss_params[k].detach() for k in m.param_names]
cs = camera_struct(cam)
bg4 = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0)

# the frame: project -> bin -> training raster, once
proj, ws, cap, total = splat._project_and_bin(m, cs, params, H, W, 3, 0, 1 << 22, m._new_workspace)
image = lambda *c, dtype=torch.float32: torch.empty((H, W) + c, dtype=dtype, device=dev)  # noqa: E731
rgbt, depth, alpha, final_t, last = image(4), image(1), image(1), image(), image(dtype=i32)
thermal = (image(1), image(), image(dtype=i32)) if sep else ()
splat_calls.raster_train(cs, N, ws, cap, bg4, 0, rgbt, depth, alpha, final_t, last, *thermal)
gen = torch.Generator(device=dev).manual_seed(3)
v_rgbt, v_alpha, v_alpha_th, v_depth = (torch.randn((H, W, c), device=dev, generator=gen) for c in (4, 1, 1, 1))
variants = (["parent"] if parent is not None else []) + ["off", "depth"]
per_gaussian = lambda *c: torch.empty((N,) + c, device=dev)  # noqa: E731
outs = {v: {"xys": per_gaussian(2), "xys_abs": per_gaussian(2) if absgrad else None, "conics": per_gaussian(3), "colors": per_gaussian(4), "lnop": per_gaussian(),
            "lnop_th": per_gaussian() if sep else None, "depths": per_gaussian(), "grads": [torch.empty_like(t) for t in params]} for v in variants + ["zero"]}


def backward(v, upstream=None):
    o = outs[v]
    th = {"final_t_th": thermal[1], "last_th": thermal[2], "v_alpha_th": v_alpha_th, "v_lnop_th": o["lnop_th"]} if sep else {}
    dz = {"aa": 0, "depth": depth, "v_depth": v_depth if upstream is None else upstream, "v_depths": o["depths"]} if v in ("depth", "zero") else {}
    real = _lib._lib
    if v == "parent":  # the call layer resolves its names in the library _lib holds: for this variant, the parent's build
        _lib._lib = parent
    try:
        splat_calls.raster_backward(cs, N, ws, cap, total, bg4, final_t, last, proj["conics"], v_rgbt, v_alpha, o["xys"], o["conics"], o["colors"], o["lnop"],
                                    v_xys_abs=o["xys_abs"], **th, **dz)
        splat_calls.project_backward(cs, params, 3, 0, proj["radii"], o["xys"], o["conics"], o["colors"], o["lnop"], o["grads"], o["lnop_th"],
                                     v_depths=dz.get("v_depths"))
    finally:
        _lib._lib = real


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(BATCH):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / BATCH


def median(ts):
    return sorted(ts)[len(ts) // 2]


for v in variants:
    backward(v)
backward("zero", torch.zeros_like(v_depth))
torch.cuda.synchronize()
res = {"gaussians": N, "image": [W, H], "iters": iters, "repeats": repeats, "thermal_opacity_mode": "separate" if sep else "shared", "absgrad": absgrad,
       "visible": int((proj["radii"] > 0).sum()), "pairs": total,
       "pair_record_bytes": {k: splat_calls.workspace_bytes("tn_splat_backward_workspace_bytes", N, cap, int(sep), int(absgrad), d) for k, d in (("off", 0), ("depth", 1))}}


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(outs[a]["grads"] + [outs[a]["xys"]], outs[b]["grads"] + [outs[b]["xys"]]))


res["zero_depth_upstream_equals_off"] = same("zero", "off")
res["depth_upstream_changes_the_means_gradient"] = not torch.equal(outs["depth"]["grads"][0], outs["off"]["grads"][0])
if parent is not None:
    res["off_gradients_equal_parent"] = same("parent", "off")
times = {v: [] for v in variants}
for _ in range(repeats):
    t = {v: [] for v in variants}
    for it in range(iters + 3):
        for v in variants:
            a = timed(lambda: backward(v))
            if it >= 3:
                t[v].append(a)
    for v in variants:
        times[v].append(median(t[v]))
res["backward_ms"] = {v: [round(min(ts), 4), round(median(ts), 4), round(max(ts), 4)] for v, ts in times.items()}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(line + "\n")
