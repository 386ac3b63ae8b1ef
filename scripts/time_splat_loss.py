"""The splat training loss at 1080p (HIP events on torch's current stream, the stream the library launches on; median of SPLAT_ITERS after
warm-up).  One JSON line with:
  - tn_image_loss alone (loss + gradient in one call; and the loss alone, no gradient), RGB (C = 3) and thermal (C = 1);
  - the same loss written in torch (tests/ssim_functional.py in fp32: grouped conv2d + autograd), forward + backward;
  - a whole training frame on the bench.py splat scene (1 M Gaussians): get_train_outputs -> get_loss_dict -> backward().
For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_splat_loss.py` (SPLAT_ITERS=3)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
import ssim_functional as sf  # noqa: E402
from nerfstudio_thermal_amd import synth  # noqa: E402
from nerfstudio_thermal_amd.splat import PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig, image_loss  # noqa: E402

iters = int(os.environ.get("SPLAT_ITERS", 20))
N = int(os.environ.get("SPLAT_N", 1_000_000))
H, W = 1080, 1920


def timed(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


res = {"size": f"{W}x{H}", "iters": iters}
for name, c in (("rgb", 3), ("thermal", 1)):
    pred, gt = sf.correlated_pair(H, W, c, seed=1, dtype=torch.float32)
    pred, gt = pred.cuda().requires_grad_(True), gt.cuda()

    def hip_fwd_bwd():
        pred.grad = None
        image_loss(pred, gt, 0.2)[0].backward()

    def hip_fwd_only():
        with torch.no_grad():
            image_loss(pred, gt, 0.2)

    def torch_fwd_bwd():
        pred.grad = None
        sf.main_loss(pred, gt, 0.2).backward()

    res[f"hip_loss_and_grad_ms_{name}"] = timed(hip_fwd_bwd)
    res[f"hip_loss_only_ms_{name}"] = timed(hip_fwd_only)
    res[f"torch_loss_and_grad_ms_{name}"] = timed(torch_fwd_bwd)

m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(), num_points=4)
m.load_gaussians(synth.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5)))
m.step = 10**6
cam = PinholeCamera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 1400.0, 960.0, 540.0, W, H)
gt_img = torch.rand((H, W, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
parts = {"render": [], "loss": [], "backward": []}


def frame():
    m.zero_grad(set_to_none=True)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    e[0].record()
    out = m.get_train_outputs(cam)
    e[1].record()
    loss = m.get_loss_dict(out, {"image": gt_img, "is_thermal": False})
    e[2].record()
    (loss["main_loss"] + loss["scale_reg"]).backward()
    e[3].record()
    torch.cuda.synchronize()
    for k, i in (("render", 0), ("loss", 1), ("backward", 2)):
        parts[k].append(e[i].elapsed_time(e[i + 1]))


res["frame_ms"] = timed(frame)
for k, v in parts.items():
    v = sorted(v[3:])
    res[f"frame_{k}_ms"] = v[len(v) // 2]
res["gaussians"] = N
print(json.dumps(res))
