"""The MCMC strategy's two device operations at SPLAT_N Gaussians (default 1 M, degree-3 SH; SPLAT_SEP=1: separate thermal opacity):
  - the position noise of one training step: one tn_splat_mcmc_noise launch against the same formula in plain torch ops (gsplat's
    inject_noise_to_position: covariances [N,3,3], two bmm), both from the same randn draw, which is not timed;
  - one refinement (ThermalSplatfactoModel.refinement_after under strategy "mcmc"): SPLAT_DEAD (default 5 %) of the Gaussians dead, relocated, and
    the population grown by 5 % -- two torch.multinomial draws, the growth of every tensor and both moments by torch.cat, and two
    tn_splat_mcmc_relocate calls; the relocate call alone is timed too, on fixed draws.
HIP events on torch's current stream; every figure is the median of SPLAT_ITERS iterations after warm-up, the whole measurement repeated
SPLAT_REPEATS times and reported as [min, median, max] of those medians.  One JSON line (also to --out)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import splat, synth  # noqa: E402
from nerfstudio_thermal_amd.optim import SPLAT_OPTIMIZERS, HipAdam, Optimizers  # noqa: E402
from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
N = int(os.environ.get("SPLAT_N", 1_000_000))
iters = int(os.environ.get("SPLAT_ITERS", 20))
repeats = int(os.environ.get("SPLAT_REPEATS", 3))
dead_share = float(os.environ.get("SPLAT_DEAD", 0.05))
sep = os.environ.get("SPLAT_SEP", "0") == "1"
dev = "cuda"


def noise_torch(means, scales, quats, opacities, z, scaler, opacities_thermal=None):
    o = torch.sigmoid(opacities).reshape(-1)
    if opacities_thermal is not None:
        o = torch.maximum(o, torch.sigmoid(opacities_thermal).reshape(-1))
    g = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - o) - 0.995)))
    q = quats / quats.norm(dim=-1, keepdim=True)
    w, x, y, zq = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - w * zq), 2 * (x * zq + w * y), 2 * (x * y + w * zq), 1 - 2 * (x * x + zq * zq),
                     2 * (y * zq - w * x), 2 * (x * zq - w * y), 2 * (y * zq + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    M = R * torch.exp(scales)[:, None, :]
    cov = torch.bmm(M, M.transpose(1, 2))
    means.add_(torch.bmm(cov, (z * g[:, None] * scaler)[:, :, None]).squeeze(-1))


def timed(fn, setup=None):
    """[min, median, max] over the repeats of the median milliseconds of one fn() call"""
    meds = []
    for _ in range(repeats):
        ts = []
        for i in range(iters + 3):
            state = setup() if setup else None
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(state) if setup else fn()
            b.record()
            b.synchronize()
            if i >= 3:
                ts.append(a.elapsed_time(b))
        meds.append(statistics.median(ts))
    return [min(meds), statistics.median(meds), max(meds)]


p = dict(synth.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5)))
g = torch.Generator().manual_seed(1)
dead = torch.rand(N, generator=g) < dead_share
p["opacities"][dead] = -7.0
if sep:
    p["opacities_thermal"] = p["opacities"] + 0.08 * torch.randn(N, 1, generator=g)
cfg = ThermalSplatfactoModelConfig(strategy="mcmc", max_gs_num=2 * N, warmup_length=0, refine_every=100,
                                   thermal_opacity_mode="separate" if sep else "shared")
scaler = cfg.noise_lr * SPLAT_OPTIMIZERS["xyz"][0]


def fresh_model():
    m = ThermalSplatfactoModel(cfg, num_points=4, device=dev, seed=3)
    m.load_gaussians(p)
    opts = Optimizers(m.get_param_groups(), SPLAT_OPTIMIZERS, optimizer_cls=HipAdam)
    for ps in m.get_param_groups().values():  # one Adam step: every group has moments to carry
        ps[0].grad = torch.full_like(ps[0], 1e-3)
    opts.optimizer_step_all()
    opts.zero_grad_all()
    m.step_cb(100)
    return m, opts


m, opts = fresh_model()
gp = m.gauss_params
th = gp["opacities_thermal"].data if sep else None
z = torch.randn((N, 3), device=dev)
means = gp["means"].data.clone()
t_noise = timed(lambda: splat.mcmc_noise(means, gp["scales"].data, gp["quats"].data, gp["opacities"].data, z, scaler, th))
t_noise_torch = timed(lambda: noise_torch(means, gp["scales"].data, gp["quats"].data, gp["opacities"].data, z, scaler, th))
a, b = gp["means"].data.clone(), gp["means"].data.clone()
splat.mcmc_noise(a, gp["scales"].data, gp["quats"].data, gp["opacities"].data, z, scaler, th)
noise_torch(b, gp["scales"].data, gp["quats"].data, gp["opacities"].data, z, scaler, th)
delta = (b - gp["means"].data).abs().max()
noise_diff = float((a - b).abs().max() / delta)

# the relocate call alone: the dead rows as destinations, sources drawn once from the live ones
o_vis = m._visible_opacity()
dst = (o_vis <= cfg.mcmc_min_opacity).nonzero().reshape(-1)
alive = (o_vis > cfg.mcmc_min_opacity).nonzero().reshape(-1)
src = alive[torch.multinomial(o_vis[alive], dst.numel(), replacement=True)]
names = m.param_names
tensors = [gp[k].data.clone() for k in names]
mom = m._adam_moments(opts.optimizers)
m1, m2 = [mom[k][0].clone() for k in names], [mom[k][1].clone() for k in names]
t_relocate = timed(lambda: splat.mcmc_relocate(tensors, m1, m2, src, dst, cfg.mcmc_min_opacity))

# the whole refinement, each time from a fresh model (the setup is not timed)
t_refine = timed(lambda s: s[0].refinement_after(s[1], 100), setup=fresh_model)
m2_, o2_ = fresh_model()
m2_.refinement_after(o2_, 100)
torch.cuda.synchronize()

row_bytes = 4 * sum(int(gp[k].data[0].numel()) for k in names)
res = {"what": "MCMC strategy: position noise and refinement", "gaussians": N, "separate": sep, "iters": iters, "repeats": repeats,
       "noise_ms_hip": t_noise, "noise_ms_torch": t_noise_torch, "noise_bytes_per_gaussian": 72 if sep else 68,
       "noise_GBps_hip": (72 if sep else 68) * N / (t_noise[1] * 1e-3) / 1e9, "noise_hip_vs_torch_max_diff_rel": noise_diff,
       "relocate_draws": int(dst.numel()), "relocate_ms_hip": t_relocate, "row_bytes": row_bytes, "refine_ms": t_refine,
       "refine_counts": list(m2_.last_refine_counts), "gaussians_after": m2_.num_points}
line = json.dumps(res)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(line + "\n")
