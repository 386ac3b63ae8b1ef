"""The ray-contribution pass (tn_splat_raster_contrib: run starts, k_splat_raster_contrib, k_splat_contrib_fold) at the benchmark's splat shape
(1 M synthetic Gaussians) on a 1920 x 1080 frame, a 640 x 480 frame and a 160 x 120 frame, beside the eval rasteriser (tn_splat_raster) and the
training rasteriser's backward (tn_splat_raster_backward: k_splat_raster_bwd + k_splat_pair_fold) on the same projected and binned frame, the three
alternated in one loop so that all see the same machine state.  HIP events on torch's current stream (the stream the library launches on), medians
and minima over SPLAT_ITERS iterations after warm-up; the scratch buffers come from torch's caching allocator, which costs no device time.  Then
score_gaussians over a rig of SPLAT_CAMS cameras end to end (project + bin + contribution per frame), per frame.  One JSON line.
SPLAT_MODE = classic | antialiased."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import splat_calls, splat_prune, synth  # noqa: E402
from nerfstudio_thermal_amd.splat import PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig, camera_struct  # noqa: E402

N = int(os.environ.get("SPLAT_N", 1_000_000))
iters = int(os.environ.get("SPLAT_ITERS", 20))
mode = os.environ.get("SPLAT_MODE", "classic")
n_cams = int(os.environ.get("SPLAT_CAMS", 8))
SHAPES = {"1920x1080": (1920, 1080, 1400.0), "640x480": (640, 480, 1400.0 / 3), "160x120": (160, 120, 1400.0 / 12)}
dev = "cuda"
m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(rasterize_mode=mode), num_points=4)
m.load_gaussians(dict(synth.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5))))
m.step = 10**6
aa = int(mode == "antialiased")


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


def camera(W, H, f, eye=(3.2, 0.5, 0.8), thermal=False):
    return PinholeCamera(synth.look_at_camera(eye), f, f, W / 2, H / 2, W, H, is_thermal=thermal)


res = {}
for name, (W, H, f) in SHAPES.items():
    cam = camera(W, H, f)
    m.get_outputs(cam)  # projects and bins: the workspace the three launches below walk
    cs, ws, cap, total = camera_struct(cam), m._ws, m._cap, m.last_num_intersections
    conics = m.last_projection["conics"]
    img = lambda *c, dtype=torch.float32: torch.empty((H, W) + c, dtype=dtype, device=dev)  # noqa: E731
    bg = (C.c_float * 4)(0.0, 0.0, 0.0, 0.0)
    rgbt, depth, alpha, final_t, last = img(4), img(1), img(1), img(), img(dtype=torch.int32)
    splat_calls.raster_train(cs, N, ws, cap, bg, aa, rgbt, depth, alpha, final_t, last)
    v_rgbt, v_alpha = torch.randn((H, W, 4), device=dev), torch.randn((H, W, 1), device=dev)
    per = lambda *c: torch.empty((N,) + c, device=dev)  # noqa: E731
    v_xys, v_conics, v_colors, v_lnop = per(2), per(3), per(4), per()
    scores = splat_prune.GaussianScores.zeros(N, dev)
    group = {
        "raster": lambda: splat_calls.raster(cs, N, ws, cap, bg, aa, rgbt, depth, alpha),
        "contribution": lambda: splat_calls.raster_contrib(cs, N, ws, cap, aa, 0, None, *scores.spectrum(False)),
        "raster_backward": lambda: splat_calls.raster_backward(cs, N, ws, cap, total, bg, final_t, last, conics, v_rgbt, v_alpha, v_xys, v_conics, v_colors, v_lnop),
    }
    for _ in range(3):
        for fn in group.values():
            timed(fn)
    ts = {k: [] for k in group}
    for _ in range(iters):
        for k, fn in group.items():
            ts[k].append(timed(fn))
    r = {k: stats(v) for k, v in ts.items()}
    r["intersections"] = total
    r["contribution_over_raster"] = r["contribution"]["ms_median"] / r["raster"]["ms_median"]
    r["raster_backward_over_raster"] = r["raster_backward"]["ms_median"] / r["raster"]["ms_median"]
    res[name] = r

# score_gaussians end to end over a rig: RGB frames at 640 x 480 and thermal frames at 160 x 120 on a ring
ring = [(3.2 * torch.cos(torch.tensor(6.2832 * i / n_cams)).item(), 3.2 * torch.sin(torch.tensor(6.2832 * i / n_cams)).item(), 0.8) for i in range(n_cams)]
rig = [camera(640, 480, 1400.0 / 3, e) for e in ring] + [camera(160, 120, 1400.0 / 12, e, True) for e in ring]
splat_prune.score_gaussians(m, rig)
ts = [timed(lambda: splat_prune.score_gaussians(m, rig)) for _ in range(max(iters // 4, 3))]
s = splat_prune.score_gaussians(m, rig)
imp = s.importance()
line = {"gaussians": N, "mode": mode, "iters": iters, **res,
        "score_rig": {"cameras": len(rig), **stats(ts), "ms_per_frame_median": stats(ts)["ms_median"] / len(rig)},
        "rig_kept_at_0.01": int((imp >= 0.01).sum()), "rig_seen_by_no_frame": int(((s.views_rgb + s.views_thermal) == 0).sum())}
print(json.dumps(line))
