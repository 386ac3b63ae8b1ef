"""Training forward + backward of the thermal-splatfacto render at the benchmark's splat shape (1 M synthetic Gaussians, 1920 x 1080) in both
thermal opacity modes: device time of get_train_outputs and of backward() after warm-up (HIP events on torch's current stream, the stream the
library launches on), medians and minima over SPLAT_ITERS iterations, shared mode first, then separate mode (opacities_thermal = a permutation
of the opacities, so the two chains differ), and the ratio of the two.  One JSON line.  SPLAT_MODE = classic | antialiased."""
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
cam = PinholeCamera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 1400.0, 960.0, 540.0, 1920, 1080)
g = torch.Generator(device="cuda").manual_seed(0)
v = {k: torch.rand((1080, 1920, c), device="cuda", generator=g) for k, c in (("rgb", 3), ("thermal", 1), ("accumulation", 1), ("accumulation_thermal", 1))}
params = synth.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5))


def measure(opacity_mode):
    m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(rasterize_mode=mode, thermal_opacity_mode=opacity_mode), num_points=4)
    p = dict(params)
    if opacity_mode == "separate":
        p["opacities_thermal"] = params["opacities"][torch.randperm(N, generator=torch.Generator().manual_seed(1))].clone()
    m.load_gaussians(p)
    m.step = 10**6

    def step():
        m.zero_grad(set_to_none=True)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        out = m.get_train_outputs(cam)
        loss = sum((out[k] * v[k]).sum() for k in v if k in out)
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
    return {"intersections": m.last_num_intersections, "train_forward_ms_median": fw[len(fw) // 2], "backward_ms_median": bw[len(bw) // 2],
            "train_forward_ms_min": fw[0], "backward_ms_min": bw[0]}


modes = [s for s in ("shared", "separate") if hasattr(ThermalSplatfactoModelConfig(), "thermal_opacity_mode") or s == "shared"]  # (a tree without the mode: shared only)
res = {s: measure(s) for s in modes}
line = {"gaussians": N, "mode": mode, "iters": iters, **res}
if "separate" in res:
    line["separate_over_shared"] = {k: res["separate"][k] / res["shared"][k] for k in ("train_forward_ms_median", "backward_ms_median")}
print(json.dumps(line))
