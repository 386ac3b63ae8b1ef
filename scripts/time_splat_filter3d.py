"""Mip-Splatting's 3D smoothing filter at SPLAT_N Gaussians (default 1 M) and SPLAT_CAMERAS cameras (default 200, RGB 640 x 480 and thermal
160 x 120 alternating, focal lengths 4 x apart):
  - the filter value: tn_filter3d_splat_compute (two launches) against the same rule as torch expressions on the device (float32, [N,C]
    temporaries, the cameras in chunks of 50), and the largest relative difference of the two results where they agree on visibility;
  - applying it: tn_filter3d_splat_apply and tn_filter3d_splat_apply_backward, shared and separate mode, with the bytes each has to move
    (forward 36 / 44 per Gaussian, backward 52 / 64) over the time, and that rate as a share of the 6.3 TB/s a streaming kernel reaches
    here (the figure profiles/splat_transform.md quotes);
  - the training step (render, loss, backward, HipAdam) of a model of SPLAT_TRAIN_N Gaussians (default 200 k) on a 640 x 480 RGB and a
    160 x 120 thermal frame in turn, with use_3d_filter off -- no new code runs: the step as it was -- and on, the two models alternating in
    blocks of steps; per step a device-event time, reported as median and mean, and for the switched-on model the mean over the steps that
    refresh the buffer (every filter_3d_every = 100) and over the others.
HIP events on torch's current stream; kernel figures are the median of SPLAT_ITERS iterations after warm-up, the measurement repeated SPLAT_REPEATS
times and reported as [min, median, max] of those medians.  One JSON line (also to --out)."""
import argparse
import functools
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import splat_calls, splat_filter, synth  # noqa: E402
from nerfstudio_thermal_amd.optim import SPLAT_OPTIMIZERS, HipAdam, Optimizers  # noqa: E402
from nerfstudio_thermal_amd.splat import PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
N = int(os.environ.get("SPLAT_N", 1_000_000))
C = int(os.environ.get("SPLAT_CAMERAS", 200))
TRAIN_N = int(os.environ.get("SPLAT_TRAIN_N", 200_000))
TRAIN_STEPS = int(os.environ.get("SPLAT_TRAIN_STEPS", 400))
iters = int(os.environ.get("SPLAT_ITERS", 20))
repeats = int(os.environ.get("SPLAT_REPEATS", 3))
STREAM_TBS = 6.3
NEAR, VARIANCE = 0.2, 0.2
dev = "cuda"
assert torch.cuda.is_available(), "a measurement needs the GPU"


def timed(fn):
    """[min, median, max] over the repeats of the median milliseconds of one fn() call"""
    meds = []
    for _ in range(repeats):
        ts = []
        for i in range(iters + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= 3:
                ts.append(a.elapsed_time(b))
        meds.append(statistics.median(ts))
    return [min(meds), statistics.median(meds), max(meds)]


def rig(count, radius=4.0, seed=0):
    """cameras on a sphere around the origin, looking at it: RGB 640 x 480 (even) and thermal 160 x 120 (odd) at the same field of view"""
    rng = np.random.default_rng(seed)
    cams = []
    for i in range(count):
        d = rng.standard_normal(3)
        eye = tuple(radius * d / np.linalg.norm(d) * rng.uniform(0.8, 1.2))
        th = bool(i % 2)
        w, h = (160, 120) if th else (640, 480)
        f = 0.5 * w / math.tan(math.radians(30.0))
        cams.append(PinholeCamera(synth.look_at_camera(eye), f, f, w / 2, h / 2, w, h, cam_idx=i, is_thermal=th))
    return cams


def filter_torch(means, table, near, variance, chunk=50):
    """the rule of tn_filter3d_splat_compute as float32 torch expressions"""
    x, y, z = means[:, 0:1], means[:, 1:2], means[:, 2:3]
    nu = torch.zeros(means.shape[0], device=means.device)
    for c0 in range(0, table.shape[0], chunk):
        t = table[c0:c0 + chunk]
        m = [t[:, j][None] for j in range(18)]
        zc = m[8] * x + m[9] * y + m[10] * z + m[11]
        xc = m[0] * x + m[1] * y + m[2] * z + m[3]
        yc = m[4] * x + m[5] * y + m[6] * z + m[7]
        u, v = m[12] * xc / zc + m[14], m[13] * yc / zc + m[15]
        seen = (zc > near) & (u >= -0.15 * m[16]) & (u <= 1.15 * m[16]) & (v >= -0.15 * m[17]) & (v <= 1.15 * m[17])
        nu = torch.maximum(nu, torch.where(seen, torch.maximum(m[12], m[13]) / zc, torch.zeros_like(zc)).amax(1))
    ok = nu > 0
    nu = torch.where(ok, nu, nu[ok].min() if bool(ok.any()) else nu)  # (the read-back the kernel does not need)
    return math.sqrt(variance) / nu


result = {"gaussians": N, "cameras": C, "iters": iters, "repeats": repeats, "stream_tb_per_s": STREAM_TBS}

# ---------------------------------------------------------------------------------------------------- the filter value
p = synth.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5))
means = p["means"].to(dev).contiguous()
table = splat_filter.filter_camera_table(rig(C), dev).contiguous()
out = torch.empty(N, device=dev)
hip = splat_filter.compute_3d_filter(means, table, NEAR, VARIANCE)
ref = filter_torch(means, table, NEAR, VARIANCE)
rel = ((hip - ref).abs() / ref)
result["compute"] = {"hip_ms": timed(lambda: splat_filter.compute_3d_filter(means, table, NEAR, VARIANCE, out=out)),
                     "torch_float32_ms": timed(lambda: filter_torch(means, table, NEAR, VARIANCE)),
                     "median_relative_difference_to_torch_float32": float(rel.median()),
                     "share_of_rows_within_1e-5_of_torch_float32": float((rel < 1e-5).float().mean()),
                     "pairs": N * C}
result["compute"]["pairs_per_second"] = N * C / (1e-3 * result["compute"]["hip_ms"][1])
del ref, rel

# ---------------------------------------------------------------------------------------------------- applying it
scales, o = p["scales"].to(dev).contiguous(), p["opacities"].to(dev).contiguous()
oth = (p["opacities"] + 0.1).to(dev).contiguous()
g = torch.Generator(device=dev).manual_seed(2)
gs, go, gth = (torch.randn(s, device=dev, generator=g) for s in ((N, 3), (N, 1), (N, 1)))
s_out, o_out, th_out = torch.empty_like(scales), torch.empty_like(o), torch.empty_like(oth)
for name, sep, fwd_bytes, bwd_bytes in (("shared", False, 36, 52), ("separate", True, 44, 64)):
    th = (oth, th_out) if sep else (None, None)
    fwd = timed(lambda: splat_calls.filter3d_apply(scales, o, hip, s_out, o_out, *th))
    bwd = timed(lambda: splat_calls.filter3d_apply_backward(scales, o, hip, gs, go, s_out, o_out, *((oth, gth, th_out) if sep else (None, None, None))))
    rate = lambda b, ms: b * N / (1e-3 * ms) / 1e12  # noqa: E731
    result["apply_" + name] = {"forward_ms": fwd, "forward_bytes_per_gaussian": fwd_bytes, "forward_tb_per_s": rate(fwd_bytes, fwd[1]),
                               "forward_share_of_stream_rate": rate(fwd_bytes, fwd[1]) / STREAM_TBS,
                               "backward_ms": bwd, "backward_bytes_per_gaussian": bwd_bytes, "backward_tb_per_s": rate(bwd_bytes, bwd[1]),
                               "backward_share_of_stream_rate": rate(bwd_bytes, bwd[1]) / STREAM_TBS}

# ---------------------------------------------------------------------------------------------------- the training step, switch off and on
cams = rig(8, radius=3.5, seed=1)
tp = synth.synth_gaussians(TRAIN_N, seed=12, extent=1.0, scale_range=(-5.0, -3.5))
gt = {}
for cam in cams[:2]:
    gt[cam.cam_idx] = torch.rand((cam.height, cam.width, 3), device=dev, generator=g)


def make(on):
    m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(use_3d_filter=on, warmup_length=10 ** 9), num_points=4, device=dev, seed=3, num_train_data=8)
    m.load_gaussians(tp)
    if on:
        m.set_filter_cameras(cams)
    return m, Optimizers(m.get_param_groups(), SPLAT_OPTIMIZERS, optimizer_cls=HipAdam)


def step(m, opts, k):
    cam = cams[k % 2]
    m.step = k
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    opts.zero_grad_all()
    loss = m.get_loss_dict(m.get_train_outputs(cam), {"image": gt[cam.cam_idx], "is_thermal": cam.is_thermal})
    functools.reduce(torch.add, loss.values()).backward()
    opts.optimizer_step_all()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


models = {False: make(False), True: make(True)}
times = {False: [], True: []}
for on in (False, True):  # warm-up: every shape both frames use
    for k in range(6):
        step(*models[on], k)
BLOCK = 50
for k0 in range(0, TRAIN_STEPS, BLOCK):
    for on in (False, True):
        for k in range(k0, k0 + BLOCK):
            times[on].append((k, step(*models[on], k)))
every = models[True][0].config.filter_3d_every
off, on_ = [t for _, t in times[False]], [t for _, t in times[True]]
refresh = [t for k, t in times[True] if k % every == 0 and k > 0]
plain = [t for k, t in times[True] if k % every != 0]
result["train_step"] = {"gaussians": TRAIN_N, "steps_each": TRAIN_STEPS, "frames": "640 x 480 RGB and 160 x 120 thermal in turn",
                        "off_ms_median": statistics.median(off), "off_ms_mean": statistics.fmean(off),
                        "on_ms_median": statistics.median(on_), "on_ms_mean": statistics.fmean(on_),
                        "on_refresh_steps_ms_mean": statistics.fmean(refresh) if refresh else None, "on_other_steps_ms_mean": statistics.fmean(plain),
                        "refreshes": models[True][0].filter_refreshes,
                        "off_ms_rgb_median": statistics.median([t for k, t in times[False] if k % 2 == 0]),
                        "on_ms_rgb_median": statistics.median([t for k, t in times[True] if k % 2 == 0]),
                        "off_ms_thermal_median": statistics.median([t for k, t in times[False] if k % 2 == 1]),
                        "on_ms_thermal_median": statistics.median([t for k, t in times[True] if k % 2 == 1])}
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
