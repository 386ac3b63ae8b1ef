"""The splat model's thermal regularisers at 640x480 and 1080p (HIP events on torch's current stream, the stream the library launches on; median of
SPLAT_ITERS after warm-up).  One JSON line with, per size:
  - tn_thermal_reg alone: both terms with the gradient (what a training frame runs), both terms without it, and each term alone with the gradient;
  - the bytes the call has to move (computed from the shapes: 4 B of thermal prediction and 12 B of RGB ground truth read per pixel -- the kernel
    re-reads a 1-pixel halo per 64 x 16 tile, ~20 B in all -- and 4 B of gradient written; the TV term alone reads no ground truth) and the share of
    the HBM roofline (8 TB/s) that makes of the measured time;
  - the same two terms written in torch (tests/thermal_reg_functional.py in fp32 + autograd), forward + backward;
  - tn_image_loss on the RGB frame of that size (loss + gradient), the call the regularisers run beside.
For per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_splat_thermal_reg.py` (SPLAT_ITERS=3)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
import thermal_reg_functional as trf  # noqa: E402
from nerfstudio_thermal_amd.splat import image_loss, thermal_regularizers  # noqa: E402

iters = int(os.environ.get("SPLAT_ITERS", 50))
HBM_BYTES_PER_S = 8e12
TV, CROSS = 1e-6, 1e-6  # the NeRF path's multipliers


def timed(fn):
    for _ in range(5):
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


res = {"iters": iters, "hbm_roofline_bytes_per_s": HBM_BYTES_PER_S}
for W, H in ((640, 480), (1920, 1080)):
    pred, gt = trf.smooth_pair(H, W, seed=1, dtype=torch.float32)
    pred, gt = pred.cuda().requires_grad_(True), gt.cuda()
    rgb = gt.clone().requires_grad_(True)
    target = (0.9 * gt + 0.05).contiguous()

    def reg(tv_mult, cross_mult, grad=True):
        def fn():
            if not grad:
                with torch.no_grad():
                    thermal_regularizers(pred, gt, tv_mult, cross_mult)
                return
            pred.grad = None
            tv, cc = thermal_regularizers(pred, gt, tv_mult, cross_mult)
            (tv + cc).backward()

        return fn

    def torch_fwd_bwd():
        pred.grad = None
        tv, cc = trf.regularizers(pred, gt, TV, CROSS)
        (tv + cc).backward()

    def hip_image_loss():
        rgb.grad = None
        image_loss(rgb, target, 0.2)[0].backward()

    r = {}
    px = H * W
    for name, fn, nbytes in (("both_and_grad", reg(TV, CROSS), 20 * px), ("both_loss_only", reg(TV, CROSS, False), 16 * px),
                             ("tv_and_grad", reg(TV, 0.0), 8 * px), ("cross_and_grad", reg(0.0, CROSS), 20 * px)):
        ms = timed(fn)
        r[f"hip_{name}_ms"] = ms
        r[f"hip_{name}_bytes"] = nbytes
        r[f"hip_{name}_share_of_hbm_roofline"] = nbytes / HBM_BYTES_PER_S / (ms * 1e-3)
    r["torch_both_and_grad_ms"] = timed(torch_fwd_bwd)
    r["hip_image_loss_and_grad_ms_rgb"] = timed(hip_image_loss)
    r["thermal_reg_over_image_loss"] = r["hip_both_and_grad_ms"] / r["hip_image_loss_and_grad_ms_rgb"]
    res[f"{W}x{H}"] = r
print(json.dumps(res))
