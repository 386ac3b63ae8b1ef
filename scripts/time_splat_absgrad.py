"""The raster backward with and without the absgrad statistic at the benchmark's splat shape (1 M synthetic Gaussians, 1920 x 1080, degree-3 SH,
classic, shared opacity; SPLAT_SEP=1: separate): device time of one tn_splat_raster_backward call without v_xys_abs (memset of the pair records,
k_splat_run_start, k_splat_raster_bwd, k_splat_pair_fold) against the call with v_xys_abs on the same frame.  The projection
backward behind it is the same call either way and is not timed.  --parent-lib names another build of the library with the same ABI (an earlier
commit's): its tn_splat_raster_backward without v_xys_abs is timed in the same loop on the same workspace.
HIP events on torch's current stream; 4 back-to-back calls per timed window, the variants alternated inside an iteration; every figure is the
median of SPLAT_ITERS iterations after warm-up, the whole measurement repeated SPLAT_REPEATS times and reported as [min, median, max] of those
medians (the in-process spread; run the script again for the process-to-process one).  The upstream images are random.  Also checks that the off
path's gradients are bit-equal between the two libraries and to the _abs path's, and reports the median ratio of the two statistics' norms.  One JSON line (also to --out)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import _lib, splat, synth  # noqa: E402
from nerfstudio_thermal_amd.ops import _stream  # noqa: E402
from nerfstudio_thermal_amd.splat import PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig, camera_struct  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--parent-lib", default=None, help="libthermal_nerf_hip.so built from the parent commit")
args = ap.parse_args()
N = int(os.environ.get("SPLAT_N", 1_000_000))
iters = int(os.environ.get("SPLAT_ITERS", 20))
repeats = int(os.environ.get("SPLAT_REPEATS", 3))
sep = os.environ.get("SPLAT_SEP", "0") == "1"
BATCH = 4
H, W = 1080, 1920
dev = "cuda"
i32 = torch.int32

lib = _lib.load()
parent = None
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    name = "tn_splat_raster_backward"  # (a build with the same ABI)
    getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]

cam = PinholeCamera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 1400.0, 960.0, 540.0, W, H)
p = dict(synth.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5)))
if sep:
    p["opacities_thermal"] = p["opacities"] + 0.08 * torch.randn(N, 1, generator=torch.Generator().manual_seed(1))
m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(thermal_opacity_mode="separate" if sep else "shared"), num_points=4)
m.load_gaussians(p)
params = [m.gauss_params[k].detach() for k in m.param_names]
cs = camera_struct(cam)
ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
bg4 = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0)

# the frame: project -> bin -> training raster, once
proj, ws, cap, total = splat._project_and_bin(m, cs, params, H, W, 3, 0, 1 << 22, m._new_workspace)
rgbt, depth, alpha = torch.empty((H, W, 4), device=dev), torch.empty((H, W, 1), device=dev), torch.empty((H, W, 1), device=dev)
final_t, last = torch.empty((H, W), device=dev), torch.empty((H, W), dtype=i32, device=dev)
alpha_th = final_t_th = last_th = None  # the thermal chain's three: separate mode only
if sep:
    alpha_th, final_t_th, last_th = torch.empty((H, W, 1), device=dev), torch.empty((H, W), device=dev), torch.empty((H, W), dtype=i32, device=dev)
opt = lambda t: None if t is None else ptr(t)  # noqa: E731
_lib.check(lib.tn_splat_raster_chains(C.byref(cs), N, ptr(ws), cap, bg4, 0, ptr(rgbt), ptr(depth), ptr(alpha), opt(alpha_th), ptr(final_t), ptr(last), opt(final_t_th),
                                      opt(last_th), _stream()), "tn_splat_raster_chains")
gen = torch.Generator(device=dev).manual_seed(3)
v_rgbt = torch.randn((H, W, 4), device=dev, generator=gen)
v_alpha = torch.randn((H, W, 1), device=dev, generator=gen)
v_alpha_th = torch.randn((H, W, 1), device=dev, generator=gen)
need = {v: int(lib.tn_splat_backward_workspace_bytes(N, cap, int(sep), int(v == "abs"), 0)) for v in ("off", "abs")}
bws = torch.empty(need["abs"], dtype=torch.uint8, device=dev)
variants = (["parent"] if parent is not None else []) + ["off", "abs"]
outs = {v: {"xys": torch.empty((N, 2), device=dev), "xys_abs": torch.empty((N, 2), device=dev), "conics": torch.empty((N, 3), device=dev),
            "colors": torch.empty((N, 4), device=dev), "lnop": torch.empty(N, device=dev), "lnop_th": torch.empty(N, device=dev)} for v in variants}


def backward(v):
    o = outs[v]
    fn = (parent if v == "parent" else lib).tn_splat_raster_backward
    th = lambda t: ptr(t) if sep else None  # noqa: E731  (the thermal chain's group: all four or none)
    _lib.check(fn(C.byref(cs), N, ptr(ws), cap, total, bg4, 0, ptr(final_t), ptr(last), opt(final_t_th), opt(last_th), ptr(proj["conics"]), ptr(v_rgbt), ptr(v_alpha),
                  th(v_alpha_th), ptr(bws), need["off" if v == "parent" else v], ptr(o["xys"]), ptr(o["xys_abs"]) if v == "abs" else None, ptr(o["conics"]), ptr(o["colors"]),
                  ptr(o["lnop"]), th(o["lnop_th"]), None, None, None, _stream()), "raster backward " + v)


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
torch.cuda.synchronize()
res = {"gaussians": N, "image": [W, H], "iters": iters, "repeats": repeats, "thermal_opacity_mode": "separate" if sep else "shared",
       "visible": int((proj["radii"] > 0).sum()), "pairs": total, "pair_record_bytes": {v: need[v] for v in need}}
keys = ["xys", "conics", "colors", "lnop"] + (["lnop_th"] if sep else [])
res["abs_gradients_equal_off"] = all(torch.equal(outs["abs"][k], outs["off"][k]) for k in keys)
if parent is not None:
    res["off_gradients_equal_parent"] = all(torch.equal(outs["parent"][k], outs["off"][k]) for k in keys)
vis = proj["radii"] > 0
ns, na = outs["abs"]["xys"][vis].norm(dim=-1), outs["abs"]["xys_abs"][vis].norm(dim=-1)
ok = ns > 0
res["median_norm_ratio_abs_over_signed"] = round(float((na[ok] / ns[ok]).median()), 3)
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
res["raster_backward_ms"] = {v: [round(min(ts), 4), round(median(ts), 4), round(max(ts), 4)] for v, ts in times.items()}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(line + "\n")
