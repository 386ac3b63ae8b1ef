"""The bilateral grid's kernels and what they cost a training step (HIP events on torch's current stream, the stream the library launches on; medians
of SPLAT_ITERS iterations after warm-up, the two sides of every comparison alternated inside an iteration).  One JSON line (also to --out) with:
  - per size (640x480, 1920x1080) and spectrum (RGB: 3 x 4 matrices; thermal: gain and offset), grid_shape (16, 16, 8): `bilateral_slice` forward +
    backward (tn_bilagrid_slice, tn_bilagrid_slice_backward: the image's gradient and the whole grid row's) against the plain-torch path on the same
    GPU -- tests/bilagrid_functional.py's F.grid_sample plus the per-pixel matrix product, fp32, with autograd -- and the forward alone;
  - `bilateral_grid_tv` (value and gradient, tn_bilagrid_tv) of SPLAT_FRAMES (200) frames' RGB grids against the torch restatement with autograd;
  - one training step of ThermalSplatfactoModel (get_train_outputs -> get_loss_dict -> backward) at 1080p on SPLAT_N synthetic Gaussians with
    use_bilateral_grid on and off, SPLAT_FRAMES training frames, an RGB frame: the switch's overhead per step.
For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_splat_bilagrid.py` (SPLAT_ITERS=3)."""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
import bilagrid_functional as bf  # noqa: E402
import splat_oracle as so  # noqa: E402
from nerfstudio_thermal_amd.splat import (PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig, bilateral_grid_tv,  # noqa: E402
                                          bilateral_slice)

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
iters = int(os.environ.get("SPLAT_ITERS", 30))
N = int(os.environ.get("SPLAT_N", 1_000_000))
frames = int(os.environ.get("SPLAT_FRAMES", 200))
SHAPE = (16, 16, 8)


def timed_pair(fns):
    """name -> median ms of each function, the functions alternated inside every iteration."""
    for _ in range(5):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


res = {"iters": iters, "grid_shape": SHAPE}
for W, H in ((640, 480), (1920, 1080)):
    for C, spectrum in ((3, "rgb"), (1, "thermal")):
        image = bf.random_image(H, W, C, seed=1).cuda().requires_grad_(True)
        grids = bf.random_grids(1, C, SHAPE, seed=2).cuda().requires_grad_(True)
        v = bf.random_upstream(H, W, C, seed=3).cuda()

        def hip(backward=True):
            def fn():
                if not backward:
                    with torch.no_grad():
                        bilateral_slice(grids, 0, image)
                    return
                image.grad = grids.grad = None
                bilateral_slice(grids, 0, image).backward(v)

            return fn

        def plain(backward=True):
            def fn():
                if not backward:
                    with torch.no_grad():
                        bf.slice(grids[0], image)
                    return
                image.grad = grids.grad = None
                bf.slice(grids[0], image).backward(v)

            return fn

        both = timed_pair({"hip": hip(), "torch": plain()})
        fwd = timed_pair({"hip": hip(False), "torch": plain(False)})
        res[f"{W}x{H}_{spectrum}"] = {"hip_forward_backward_ms": both["hip"], "torch_forward_backward_ms": both["torch"],
                                      "hip_forward_ms": fwd["hip"], "torch_forward_ms": fwd["torch"],
                                      "torch_over_hip_forward_backward": both["torch"] / both["hip"]}

g_tv = bf.random_grids(frames, 3, SHAPE, seed=4).cuda().requires_grad_(True)


def hip_tv():
    g_tv.grad = None
    bilateral_grid_tv(g_tv, 10.0).backward()


def torch_tv():
    g_tv.grad = None
    (10.0 * bf.tv(g_tv)).backward()


tv = timed_pair({"hip": hip_tv, "torch": torch_tv})
res["tv"] = {"frames": frames, "hip_value_and_gradient_ms": tv["hip"], "torch_value_and_gradient_ms": tv["torch"],
             "torch_over_hip": tv["torch"] / tv["hip"]}

W, H = 1920, 1080
fx = 0.5 * W / 0.57735  # about 60 degrees across
cam = PinholeCamera(so.look_at_camera((2.4, 0.5, 0.7)), fx, fx, W / 2, H / 2, W, H)
params = so.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5))
models = {}
for key, on in (("off", False), ("on", True)):
    m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(use_bilateral_grid=on), num_points=4, device="cuda", num_train_data=frames)
    m.load_gaussians(params)
    m.step = 10**6
    models[key] = m
with torch.no_grad():
    batch = {"image": (0.8 * models["off"].get_outputs(cam)["rgb"] + 0.1).contiguous(), "is_thermal": False}
frame = dataclasses.replace(cam, cam_idx=frames // 2)


def step(m):
    def fn():
        m.zero_grad(set_to_none=True)
        losses = m.get_loss_dict(m.get_train_outputs(frame), batch)
        sum(losses.values()).backward()

    return fn


st = timed_pair({k: step(m) for k, m in models.items()})
res["train_step_1080p"] = {"gaussians": N, "train_frames": frames, "switch_off_ms": st["off"], "switch_on_ms": st["on"],
                           "overhead_ms": st["on"] - st["off"]}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(line + "\n")
