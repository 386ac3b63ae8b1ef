"""The removal renders of the separate thermal opacity at the benchmark's splat shape (1 M synthetic Gaussians, 1920 x 1080): device time of the
eval frame (get_outputs) with removal off and with removal on, alternated, and of the two rasteriser launches alone on the frame's own workspace
-- tn_splat_raster_chains with out_alpha_thermal alone (the separate-mode eval raster, the yardstick: three chains in classic mode, four in antialiased) and tn_splat_raster_removal_sep (two chains, no depth)
-- alternated as well.  HIP events on torch's current stream (the stream the library launches on), medians and minima over SPLAT_ITERS
iterations after warm-up.  opacities_thermal = opacities + SPLAT_NOISE * randn on the logits (default 0.08; the line reports the share each render
keeps); SPLAT_THR = removal_min_opacity_diff (0.05; 1e30 keeps everything, the launch's worst case).  One JSON line.
SPLAT_MODE = classic | antialiased."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import _lib, synth  # noqa: E402
from nerfstudio_thermal_amd.ops import _stream  # noqa: E402
from nerfstudio_thermal_amd.splat import PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig, camera_struct  # noqa: E402

N = int(os.environ.get("SPLAT_N", 1_000_000))
iters = int(os.environ.get("SPLAT_ITERS", 20))
mode = os.environ.get("SPLAT_MODE", "classic")
thr = float(os.environ.get("SPLAT_THR", 0.05))
noise = float(os.environ.get("SPLAT_NOISE", 0.08))
H, W = 1080, 1920
cam = PinholeCamera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 1400.0, 960.0, 540.0, W, H)
params = dict(synth.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5)))
params["opacities_thermal"] = params["opacities"] + noise * torch.randn(N, 1, generator=torch.Generator().manual_seed(1))


def model(removal):
    m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(rasterize_mode=mode, thermal_opacity_mode="separate", removal_min_opacity_diff=removal), num_points=4)
    m.load_gaussians(params)
    m.step = 10**6
    return m


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    ts = sorted(ts)
    return {"ms_median": ts[len(ts) // 2], "ms_min": ts[0]}


off, on = model(None), model(thr)
frames = {"frame_removal_off": lambda: off.get_outputs(cam), "frame_removal_on": lambda: on.get_outputs(cam)}
# the two launches alone, on the workspace the last frame of `on` left (projected and binned)
on.get_outputs(cam)
lib = _lib.load()
cs, ws, cap, aa = camera_struct(cam), on._ws, on._cap, int(mode == "antialiased")
bg = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0)
rgbt, rem = torch.empty((H, W, 4), device="cuda"), torch.empty((H, W, 4), device="cuda")
depth, alpha, alpha_th = (torch.empty((H, W, 1), device="cuda") for _ in range(3))
ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
launches = {
    "raster_sep_launch": lambda: _lib.check(lib.tn_splat_raster_chains(C.byref(cs), N, ptr(ws), cap, bg, aa, ptr(rgbt), ptr(depth), ptr(alpha), ptr(alpha_th), None, None, None, None, _stream())),
    "raster_removal_launch": lambda: _lib.check(lib.tn_splat_raster_removal_sep(C.byref(cs), N, ptr(ws), cap, bg, thr, ptr(rem), _stream())),
}
res = {}
for group in (frames, launches):
    for _ in range(3):
        for fn in group.values():
            timed(fn)
    ts = {k: [] for k in group}
    for _ in range(iters):
        for k, fn in group.items():  # alternated: both see the same machine state
            ts[k].append(timed(fn))
    res.update({k: stats(v) for k, v in ts.items()})
o, ot = torch.sigmoid(params["opacities"]), torch.sigmoid(params["opacities_thermal"])
line = {"gaussians": N, "mode": mode, "iters": iters, "removal_min_opacity_diff": thr, "intersections": on.last_num_intersections,
        "kept_rgb_share": float(((o - ot).abs() < thr * o).float().mean()), "kept_thermal_share": float(((o - ot).abs() < thr * ot).float().mean()), **res,
        "removal_over_raster_sep": res["raster_removal_launch"]["ms_median"] / res["raster_sep_launch"]["ms_median"],
        "frame_on_over_off": res["frame_removal_on"]["ms_median"] / res["frame_removal_off"]["ms_median"]}
print(json.dumps(line))
