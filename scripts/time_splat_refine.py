"""Splat refinement at 1080p on 1 M synthetic Gaussians (the bench.py splat scene): device time (HIP events on torch's current stream, medians
after warm-up) of
  * after_train (tn_splat_grad_stats) + one Adam step over all eight groups (HipAdam: one tn_adam_step per parameter),
  * one refinement_after by the HIP path (tn_splat_refine_plan + its count read-back + split noise + tn_splat_refine_apply + the optimiser
    bookkeeping), and the same refinement by the torch restatement (tests/splat_refine_functional.py) on the same device tensors.
The statistics are set so that about 10 % of the Gaussians split and 10 % are duplicated.  One JSON line.  For per-kernel times run it under
`rocprofv3 --kernel-trace --stats -- python scripts/time_splat_refine.py` (SPLAT_ITERS=3)."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import optim, synth  # noqa: E402
from nerfstudio_thermal_amd.splat import GROUP_PARAMS, PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig  # noqa: E402

import splat_refine_functional as rf  # noqa: E402

N = int(os.environ.get("SPLAT_N", 1_000_000))
iters = int(os.environ.get("SPLAT_ITERS", 10))
STEP = 600  # densifies under the default schedule
dev = "cuda"
m = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(), num_points=4)
m.load_gaussians(synth.synth_gaussians(N, seed=11, extent=1.5, scale_range=(-5.5, -3.5)))
cam = PinholeCamera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 1400.0, 960.0, 540.0, 1920, 1080)
opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=optim.HipAdam)
m.step = STEP
out = m.get_train_outputs(cam)
(out["rgb"].mean() + out["thermal"].mean()).backward()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def train_tail():
    m.after_train(STEP)
    opts.optimizer_step_all()


for _ in range(3):
    train_tail()
tail_ms = median([timed(train_tail) for _ in range(iters)])

# the refinement's input state: ~20 % high gradients, half of them small (duplicated), half large (split)
g = torch.Generator(device=dev).manual_seed(4)
high = torch.rand(N, device=dev, generator=g) < 0.2
small = torch.rand(N, device=dev, generator=g) < 0.5
with torch.no_grad():
    m.gauss_params["scales"][small] = math.log(0.005)
    m.gauss_params["scales"][~small] = math.log(0.03)
state = {k: v.detach().clone() for k, v in m.gauss_params.items()}
moments = {}
for grp, k in GROUP_PARAMS.items():
    st = opts.optimizers[grp].state[m.gauss_params[k]]
    moments[k] = (st["step"].clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
stats = (torch.where(high, 1e-3, 1e-8).float(), torch.ones(N, device=dev), m.max_2Dsize.clone())


def reset():
    m.gauss_params = torch.nn.ParameterDict({k: torch.nn.Parameter(v.clone()) for k, v in state.items()})
    for grp, k in GROUP_PARAMS.items():
        o = opts.optimizers[grp]
        o.state.clear()
        p = m.gauss_params[k]
        o.param_groups[0]["params"] = [p]
        s, a, b = moments[k]
        o.state[p] = {"step": s.clone(), "exp_avg": a.clone(), "exp_avg_sq": b.clone()}
    m.xys_grad_norm, m.vis_counts, m.max_2Dsize = (t.clone() for t in stats)
    m.step = STEP
    torch.cuda.synchronize()


hip_ms = []
for i in range(iters + 2):
    reset()
    t = timed(lambda: m.refinement_after(opts, STEP))
    if i >= 2:
        hip_ms.append(t)
counts = m.last_refine_counts
n_out = m.num_points
torch_ms = []
mom_in = {k: (a, b) for k, (_, a, b) in moments.items()}
for i in range(iters + 2):
    t = timed(lambda: rf.refine(state, mom_in, stats, (1080, 1920), STEP, m.config, 0, lambda k: torch.randn((k, 3), device=dev)))
    if i >= 2:
        torch_ms.append(t)
row_floats = sum(v[0].numel() for v in state.values())  # parameter floats per Gaussian
print(json.dumps({"gaussians": N, "out": n_out, "split": counts[0], "originals_kept": counts[1], "children_kept": counts[2], "duplicates_kept": counts[3],
                  "param_floats_per_gaussian": row_floats, "after_train_plus_adam_ms_median": tail_ms, "refine_hip_ms_median": median(hip_ms),
                  "refine_hip_ms_min": min(hip_ms), "refine_torch_ms_median": median(torch_ms), "iters": iters}))
