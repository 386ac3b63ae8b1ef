"""undistort_image (tn_image_undistort: a distorted frame resampled into the rasteriser's pinhole frame) on one 1080p frame of 3 channels: HIP
events on torch's current stream around UNDISTORT_CALLS back-to-back calls (output allocation and the argument block included; the new camera is
computed once, outside), the median of UNDISTORT_ITERS such windows after warm-up, per call.  One JSON line with fp32 -> fp32 and uint8 -> uint8
(the datamanager's two cache types).  For the kernel's own time run it under `rocprofv3 --kernel-trace --stats -- python
scripts/time_splat_undistort.py` (UNDISTORT_ITERS=3)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd.splat import PinholeCamera, undistort_image, undistorted_camera  # noqa: E402

iters = int(os.environ.get("UNDISTORT_ITERS", 20))
calls = int(os.environ.get("UNDISTORT_CALLS", 100))
H, W = 1080, 1920
K = (0.05, -0.01, 0.0, 0.0, 1e-3, -5e-4)  # synth.synth_cameras' RGB distortion


def timed(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / calls)
    ts.sort()
    return ts[len(ts) // 2]


g = torch.Generator(device="cuda").manual_seed(0)
u8 = torch.randint(0, 256, (H, W, 3), device="cuda", generator=g, dtype=torch.uint8)
f32 = torch.rand((H, W, 3), device="cuda", generator=g)
cam = PinholeCamera(torch.eye(4)[:3], 0.9375 * W, 0.9375 * W, W / 2, H / 2, W, H)
new = undistorted_camera(cam, K)

res = {"size": f"{W}x{H}", "channels": 3, "iters": iters, "calls_per_window": calls,
       "hip_f32_to_f32_ms": timed(lambda: undistort_image(f32, cam, K, new)),
       "hip_u8_to_u8_ms": timed(lambda: undistort_image(u8, cam, K, new)),
       "bytes_f32": 2 * H * W * 3 * 4, "bytes_u8": 2 * H * W * 3}
print(json.dumps(res))
