"""The crop box of the splat eval render at the benchmark's splat shape (1 M synthetic Gaussians, 1920 x 1080, shared opacity; SPLAT_SEP=1:
separate): device time of the projection launch, of tn_splat_bin and of the whole eval frame, uncropped and through
get_outputs_for_camera with a box that keeps everything, about 10 % and about 1 % of the Gaussians -- for the Gaussians in random order and in
Morton order of their means (10 bits per axis: 128 neighbours in memory are neighbours in space, so whole projection blocks fall outside the box
and skip their SH slab; in random order every block holds a kept Gaussian until the box is tiny).  HIP events on torch's current stream (the stream
the library launches on); every figure is the median of SPLAT_ITERS iterations after warm-up (the projection launch: 8 back-to-back launches per iteration, divided by 8), the configurations alternated inside an
iteration, and the whole measurement is repeated SPLAT_REPEATS times: a figure is reported as [min, median, max] of those medians, the run-to-run
spread.  sha256 of the uncropped frame's images are printed so that two builds can be compared on the same inputs.  One JSON line (also written
to --out).  On a tree without the crop entry points (the parent commit) only the uncropped figures are taken, for the A/B of the existing path:
run this file from that tree, and with SPLAT_UNCROPPED_ONLY=1 from this one (the same loop: no cropped frames in between)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import _lib, splat, splat_calls, synth  # noqa: E402
from nerfstudio_thermal_amd.ops import _stream  # noqa: E402
from nerfstudio_thermal_amd.splat import PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig, camera_struct  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
N = int(os.environ.get("SPLAT_N", 1_000_000))
iters = int(os.environ.get("SPLAT_ITERS", 20))
repeats = int(os.environ.get("SPLAT_REPEATS", 3))
sep = os.environ.get("SPLAT_SEP", "0") == "1"
BATCH = 8  # projection launches per timed window
H, W = 1080, 1920
EXTENT = 1.5
# SPLAT_UNCROPPED_ONLY=1: time the existing path alone on this tree too, exactly as a tree without the crop entry points is timed
HAS_CROP = hasattr(ThermalSplatfactoModel, "get_outputs_for_camera") and os.environ.get("SPLAT_UNCROPPED_ONLY", "0") != "1"
cam = PinholeCamera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 1400.0, 960.0, 540.0, W, H)
base = dict(synth.synth_gaussians(N, seed=11, extent=EXTENT, scale_range=(-5.5, -3.5)))
if sep:
    base["opacities_thermal"] = base["opacities"] + 0.08 * torch.randn(N, 1, generator=torch.Generator().manual_seed(1))


def morton_order(means):
    lo, hi = means.min(0).values, means.max(0).values
    q = ((means - lo) / (hi - lo) * 1023.0).long().clamp(0, 1023)
    code = torch.zeros(means.shape[0], dtype=torch.int64)
    for b in range(10):
        for a in range(3):
            code |= ((q[:, a] >> b) & 1) << (3 * b + a)
    return torch.argsort(code)


def timed(fn, launches=1):
    """ms per call: `launches` back-to-back calls between one pair of events (a single launch of ~0.1 ms is near the events' own granularity)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def median(ts):
    return sorted(ts)[len(ts) // 2]


def spread(ms):
    return [min(ms), median(ms), max(ms)]


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
lib = _lib.load()
res = {"gaussians": N, "iters": iters, "repeats": repeats, "thermal_opacity_mode": "separate" if sep else "shared", "crop_entry_points": HAS_CROP}
for order in ("random", "morton"):
    params = base if order == "random" else {k: v[morton_order(base["means"])].contiguous() for k, v in base.items()}
    m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(thermal_opacity_mode="separate" if sep else "shared"), num_points=4)
    m.load_gaussians(params)
    m.step = 10**6
    m.eval()
    # rotated cubes about the cloud's centre: the share of the cloud's cube [-EXTENT, EXTENT]^3 they hold is side^3 / (2 EXTENT)^3
    boxes = {"uncropped": None}
    if HAS_CROP:
        for name, share in (("keep_all", None), ("keep_10pct", 0.10), ("keep_1pct", 0.01)):
            side = 100.0 if share is None else 2.0 * EXTENT * share ** (1.0 / 3.0)
            boxes[name] = splat.OrientedBox.from_params((0.0, 0.0, 0.0), (0.3, -0.2, 0.5), (side, side, side))
    out = {k: {} for k in boxes}
    full = m.get_outputs(cam)
    out["uncropped"]["sha256"] = {k: digest(full[k]) for k in ("rgb", "thermal", "depth", "accumulation")}
    out["uncropped"]["intersections"] = m.last_num_intersections
    for name, box in boxes.items():
        if box is not None:
            frame = m.get_outputs_for_camera(cam, box)
            out[name]["kept_share"] = float(box.within(m.means.detach()).float().mean())
            out[name]["intersections"] = m.last_num_intersections
            if name == "keep_all":
                out[name]["equals_uncropped_bit_for_bit"] = all(torch.equal(frame[k], full[k]) for k in full)
    if HAS_CROP:
        m.set_crop(None)
    m.get_outputs(cam)
    # the launches alone, on the eval workspace and the projection tensors the last frame left
    cs, ws, cap = camera_struct(cam), m._ws, m._cap
    proj = m.last_projection
    pp = splat_calls._param_ptrs9([m.gauss_params[k] for k in m.param_names])  # the thermal opacity's place is null in shared mode
    K = m.gauss_params["features_rest"].shape[1]
    outs = [ptr(proj[k]) for k in ("xys", "depths", "radii", "conics", "compensation", "num_tiles_hit", "tile_box")]
    total = C.c_int64(0)
    aa, deg = m._frame_settings()  # what the model's own frames pass

    def project(box):
        crop = box.crop_struct() if box is not None else None  # a null box is the uncropped frame
        return lambda: _lib.check(lib.tn_splat_project(C.byref(cs), None, *pp, N, K, deg, aa, *outs, ptr(ws), cap, C.byref(crop) if crop is not None else None, _stream()))

    def binning():
        _lib.check(lib.tn_splat_bin(C.byref(cs), outs[1], N, ptr(ws), cap, C.byref(total), _stream()))

    def frame_fn(box):
        if box is None and not HAS_CROP:
            return lambda: m.get_outputs(cam)
        return lambda: m.get_outputs_for_camera(cam, box)  # box None: clears the crop the frame before it set

    launches = {k: project(b) for k, b in boxes.items()}
    meds = {k: {"project_ms": [], "bin_ms": [], "frame_ms": []} for k in boxes}
    for _ in range(repeats):
        for _ in range(3):  # warm-up of every shape the timed window uses
            for k in boxes:
                launches[k](), binning(), frame_fn(boxes[k])()
        ts = {k: {"project_ms": [], "bin_ms": [], "frame_ms": []} for k in boxes}
        for _ in range(iters):
            for k in boxes:  # alternated: every configuration sees the same machine state
                ts[k]["project_ms"].append(timed(launches[k], BATCH))
                ts[k]["bin_ms"].append(timed(binning))  # on what this configuration's projection left (it reads its pair count back: one at a time)
            for k in boxes:
                ts[k]["frame_ms"].append(timed(frame_fn(boxes[k])))
        for k in boxes:
            for what, v in ts[k].items():
                meds[k][what].append(median(v))
    for k in boxes:
        out[k].update({what: spread(v) for what, v in meds[k].items()})
        if k != "uncropped":
            out[k].update({f"{what}_over_uncropped": median(v) / median(meds["uncropped"][what]) for what, v in meds[k].items()})
    res[order] = out
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
