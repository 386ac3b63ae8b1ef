"""The pose instantiations of the splat projection at the benchmark's splat shape (1 M synthetic Gaussians, 1920 x 1080, degree-3 SH, shared
opacity; SPLAT_SEP=1: separate): device time of
  * the projection forward launch -- tn_splat_project without a pose record against tn_splat_pose_camera + tn_splat_project with it,
  * the projection backward -- tn_splat_project_backward without the pose group against the call with it (the kernel with the per-block reduction of
    dL/d view' plus the single-block finishing launch),
with the row at zero and at a moved pose.  --parent-lib names another build of the library with the same ABI (an earlier commit's): its tn_splat_project /
tn_splat_project_backward without the pose are timed in the same loop (the two libraries share the process and the stream).
HIP events on torch's current stream; 8 back-to-back calls per timed window, the variants alternated inside an iteration; every figure is the
median of SPLAT_ITERS iterations after warm-up, the whole measurement repeated SPLAT_REPEATS times and reported as [min, median, max] of those
medians.  The upstream gradients of the backward are random (its cost does not depend on their values); radii come from the forward.  Also
checks that the off path's outputs are bit-equal between the two libraries and to the zero-row pose path.  One JSON line (also to --out)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import _lib, splat_calls, synth  # noqa: E402
from nerfstudio_thermal_amd.ops import _stream  # noqa: E402
from nerfstudio_thermal_amd.splat import PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig, camera_struct, pose_camera_record  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--parent-lib", default=None, help="libthermal_nerf_hip.so built from the parent commit")
args = ap.parse_args()
N = int(os.environ.get("SPLAT_N", 1_000_000))
iters = int(os.environ.get("SPLAT_ITERS", 20))
repeats = int(os.environ.get("SPLAT_REPEATS", 3))
sep = os.environ.get("SPLAT_SEP", "0") == "1"
BATCH = 8
H, W = 1080, 1920
dev = "cuda"
f32, i32 = torch.float32, torch.int32

lib = _lib.load()
parent = None
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    for name in ("tn_splat_project", "tn_splat_project_backward"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]

cam = PinholeCamera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 1400.0, 960.0, 540.0, W, H, cam_idx=0)
p = dict(synth.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5)))
if sep:
    p["opacities_thermal"] = p["opacities"] + 0.08 * torch.randn(N, 1, generator=torch.Generator().manual_seed(1))
m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(thermal_opacity_mode="separate" if sep else "shared"), num_points=4)
m.load_gaussians(p)
params = [m.gauss_params[k].detach() for k in m.param_names]
K, deg, aa, cap = params[5].shape[1], 3, 0, 1 << 22
tiles = ((W + 15) // 16) * ((H + 15) // 16)
ws = m._new_workspace(N, cap, tiles)
cs = camera_struct(cam)
ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731


def outputs():
    return [torch.empty((N, 2), device=dev), torch.empty(N, device=dev), torch.empty(N, dtype=i32, device=dev), torch.empty((N, 3), device=dev),
            torch.empty(N, device=dev), torch.empty(N, dtype=i32, device=dev), torch.empty((N, 4), dtype=i32, device=dev)]


pp = splat_calls._param_ptrs9(params)  # nine places: the thermal opacity's is null in shared mode
pose = torch.zeros((2, 6), device=dev)
pose[1] = torch.tensor([0.02, -0.015, 0.01, 0.012, -0.02, 0.015])


def forward(which, out):
    o = [ptr(t) for t in out]
    if which in ("off", "parent"):
        fn = (parent if which == "parent" else lib).tn_splat_project
        _lib.check(fn(C.byref(cs), None, *pp, N, K, deg, aa, *o, ptr(ws), cap, None, _stream()), "project")
        return None
    rec = pose_camera_record(cam, cs, pose, 0 if which == "pose_zero" else 1)
    _lib.check(lib.tn_splat_project(C.byref(cs), ptr(rec), *pp, N, K, deg, aa, *o, ptr(ws), cap, None, _stream()), "project with a pose record")
    return rec


gen = torch.Generator(device=dev).manual_seed(3)
up = [torch.randn((N, 2), device=dev, generator=gen), torch.randn((N, 3), device=dev, generator=gen), torch.randn((N, 4), device=dev, generator=gen),
      torch.randn(N, device=dev, generator=gen)] + ([torch.randn(N, device=dev, generator=gen)] if sep else [])
grads = [torch.empty_like(t) for t in params]
gp = splat_calls._param_ptrs9(grads)
need = int(lib.tn_splat_pose_workspace_bytes(N))
pws = torch.empty(need, dtype=torch.uint8, device=dev)
g_pose = torch.zeros((2, 6), device=dev)
dview = torch.empty((3, 4), device=dev)


def backward(which, radii, rec):
    u = [ptr(t) for t in up] + [None] * (5 - len(up)) + [None]  # v_log_opacity_thermal (separate mode only), no v_depths
    if which in ("off", "parent"):
        fn = (parent if which == "parent" else lib).tn_splat_project_backward
        _lib.check(fn(C.byref(cs), None, None, *pp, N, K, deg, aa, ptr(radii), *u, *gp, None, 0, None, None, _stream()), "project_backward")
        return
    row = 0 if which == "pose_zero" else 1
    _lib.check(lib.tn_splat_project_backward(C.byref(cs), ptr(rec), C.c_void_p(pose.data_ptr() + 24 * row), *pp, N, K, deg, aa, ptr(radii), *u, *gp, ptr(pws), need,
                                             C.c_void_p(g_pose.data_ptr() + 24 * row), ptr(dview), _stream()), "project_backward with the pose group")


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


variants = (["parent"] if parent is not None else []) + ["off", "pose_zero", "pose_moved"]
outs = {v: outputs() for v in variants}
recs = {v: forward(v, outs[v]) for v in variants}
torch.cuda.synchronize()
res = {"gaussians": N, "image": [W, H], "iters": iters, "repeats": repeats, "thermal_opacity_mode": "separate" if sep else "shared",
       "visible": int((outs["off"][2] > 0).sum())}
same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))  # noqa: E731
res["zero_row_projection_equals_off"] = same(outs["pose_zero"], outs["off"])
if parent is not None:
    res["off_projection_equals_parent"] = same(outs["parent"], outs["off"])
gsum = {}
for v in variants:
    backward(v, outs[v][2], recs[v])
    torch.cuda.synchronize()
    gsum[v] = [g.clone() for g in grads]
res["zero_row_gradients_equal_off"] = same(gsum["pose_zero"], gsum["off"])
if parent is not None:
    res["off_gradients_equal_parent"] = same(gsum["parent"], gsum["off"])
fwd = {v: [] for v in variants}
bwd = {v: [] for v in variants}
for _ in range(repeats):
    tf = {v: [] for v in variants}
    tb = {v: [] for v in variants}
    for it in range(iters + 3):
        for v in variants:
            a = timed(lambda: forward(v, outs[v]))
            b = timed(lambda: backward(v, outs[v][2], recs[v]))
            if it >= 3:
                tf[v].append(a)
                tb[v].append(b)
    for v in variants:
        fwd[v].append(median(tf[v]))
        bwd[v].append(median(tb[v]))
spread = lambda ms: [round(min(ms), 4), round(median(ms), 4), round(max(ms), 4)]  # noqa: E731
res["projection_forward_ms"] = {v: spread(fwd[v]) for v in variants}
res["projection_backward_ms"] = {v: spread(bwd[v]) for v in variants}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(line + "\n")
