"""Training forward + backward of the thermal-splatfacto render at 1080p on 1 M synthetic Gaussians (the bench.py splat scene): device time
of get_train_outputs and of backward() after warm-up (HIP events on torch's current stream, the stream the library launches on).  One JSON
line.  For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_splat_backward.py` (SPLAT_ITERS=3)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import synth  # noqa: E402
from nerfstudio_thermal_amd.splat import PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig  # noqa: E402

N = int(os.environ.get("SPLAT_N", 1_000_000))
iters = int(os.environ.get("SPLAT_ITERS", 20))
mode = os.environ.get("SPLAT_MODE", "classic")
m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(rasterize_mode=mode), num_points=4)
m.load_gaussians(synth.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5)))
m.step = 10**6
cam = PinholeCamera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 1400.0, 960.0, 540.0, 1920, 1080)
g = torch.Generator(device="cuda").manual_seed(0)
v = {k: torch.rand((1080, 1920, c), device="cuda", generator=g) for k, c in (("rgb", 3), ("thermal", 1), ("accumulation", 1))}


def step():
    m.zero_grad(set_to_none=True)
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    e0.record()
    out = m.get_train_outputs(cam)
    loss = sum((out[k] * v[k]).sum() for k in v)
    e1.record()
    loss.backward()
    e2.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), e1.elapsed_time(e2)


for _ in range(3):
    step()
fw, bw = [], []
for _ in range(iters):
    a, b = step()
    fw.append(a)
    bw.append(b)
fw.sort()
bw.sort()
eval_ms = []
for _ in range(iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    m.get_outputs(cam)
    e1.record()
    torch.cuda.synchronize()
    eval_ms.append(e0.elapsed_time(e1))
eval_ms.sort()
print(json.dumps({"gaussians": N, "mode": mode, "intersections": m.last_num_intersections, "visible": int((m.last_projection["radii"] > 0).sum()),
                  "train_forward_ms_median": fw[len(fw) // 2], "backward_ms_median": bw[len(bw) // 2], "eval_forward_ms_median": eval_ms[len(eval_ms) // 2],
                  "train_forward_ms_min": fw[0], "backward_ms_min": bw[0], "iters": iters}))
