"""Writes tests/golden/splat_refine_cases.npz from the reference's own splatfacto refinement (build container only; writes data, never source).

Each case builds a bare SplatfactoModel carrying the six reference tensors (sh_degree 1, 200 Gaussians), with one real torch.optim.Adam per
parameter group that has stepped three times, runs the reference's after_train a few times (random xys gradients, some Gaussians invisible)
and then its refinement_after, and records the inputs, the statistics, the split noise torch.randn returned, every output tensor and every
Adam moment.  gsplat and pytorch_msssim are not installed: they are stubbed, and the split's quat_to_rotmat is supplied here.
Also records the reference's SplatfactoModelConfig defaults of the refinement fields.

    python scripts/make_golden_splat_refine.py"""
import dataclasses
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402
from splat_refine_functional import quat_to_rotmat  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "splat_refine_cases.npz")
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
GROUPS = {"xyz": "means", "features_dc": "features_dc", "features_rest": "features_rest", "opacity": "opacities", "scaling": "scales", "rotation": "quats"}
REFINE_FIELDS = ("warmup_length", "refine_every", "cull_alpha_thresh", "cull_scale_thresh", "continue_cull_post_densification", "reset_alpha_every",
                 "densify_grad_thresh", "densify_size_thresh", "n_split_samples", "cull_screen_size", "split_screen_size", "stop_screen_size_at",
                 "stop_split_at", "sh_degree", "sh_degree_interval", "rasterize_mode", "num_random", "random_scale")
SIZE = (48, 64)  # the training frames' (H, W)
NUM_TRAIN_DATA = 10


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def import_splatfacto():
    ref_import.import_reference()
    _stub("gsplat")
    _stub("gsplat._torch_impl", quat_to_rotmat=quat_to_rotmat)
    _stub("gsplat.project_gaussians", project_gaussians=None)
    _stub("gsplat.rasterize", rasterize_gaussians=None)
    _stub("gsplat.sh", num_sh_bases=lambda d: (d + 1) ** 2, spherical_harmonics=None)
    _stub("pytorch_msssim", SSIM=None)
    from nerfstudio.models import splatfacto

    return splatfacto


def make_model(sf, g: torch.Generator, n: int, huge: int = 0):
    cfg = sf.SplatfactoModelConfig(sh_degree=1)
    m = sf.SplatfactoModel.__new__(sf.SplatfactoModel)
    torch.nn.Module.__init__(m)
    m.config = cfg
    m.device_indicator_param = torch.nn.Parameter(torch.empty(0))
    m.num_train_data = NUM_TRAIN_DATA
    P = torch.nn.Parameter
    m.means = P(torch.randn((n, 3), generator=g))
    # log-scales spread across densify_size_thresh (0.01): split, duplicated, and (0.01, 0.016] both split and duplicated after the shrink
    scales = torch.empty((n, 3)).uniform_(np.log(0.003), np.log(0.03), generator=g)
    scales[:8, :] = np.log(0.005)
    scales[:8, 0] = np.log(0.013)  # split and duplicate
    if huge:
        scales[8:8 + huge, 1] = np.log(0.8)  # above cull_scale_thresh
    m.scales = P(scales)
    m.quats = P(torch.randn((n, 4), generator=g))
    m.opacities = P(torch.randn((n, 1), generator=g) * 2.0)
    m.features_dc = P(torch.rand((n, 3), generator=g))
    m.features_rest = P(torch.randn((n, 3, 3), generator=g) * 0.1)
    m.xys_grad_norm = m.vis_counts = m.max_2Dsize = None
    m.last_size = SIZE
    return m


def params(m):
    return {k: getattr(m, k).detach().clone() for k in NAMES}


def make_optimizers(m, g):
    opts = {}
    for grp, k in GROUPS.items():
        p = getattr(m, k)
        o = torch.optim.Adam([p], lr=1e-3, eps=1e-15)
        for _ in range(3):
            p.grad = torch.randn(p.shape, generator=g)
            o.step()
        p.grad = None
        opts[grp] = o
    return types.SimpleNamespace(optimizers=opts)


def moments(m, opts):
    out = {}
    for grp, k in GROUPS.items():
        o = opts.optimizers[grp]
        p = o.param_groups[0]["params"][0]
        assert p is getattr(m, k)
        st = o.state[p]
        out[k] = (st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"]))
    return out


def frame(m, g, n):
    """one training frame as after_train reads it: radii (some 0 = invisible) and xys.grad"""
    radii = torch.randint(0, 20, (n,), generator=g, dtype=torch.int32)
    radii[torch.rand(n, generator=g) < 0.25] = 0
    xys = torch.zeros((n, 2), requires_grad=True)
    xys.grad = torch.randn((n, 2), generator=g) * 1e-5
    xys.grad[radii == 0] = 0.0  # an invisible Gaussian gets no gradient from the rasteriser
    m.radii, m.xys = radii, xys
    return radii, xys.grad.clone()


CASES = {  # name -> (step, after_train frames, huge Gaussians)
    "warmup": (500, 2, 0),
    "densify": (600, 3, 0),
    "huge": (3500, 3, 6),
    "late": (4500, 3, 6),
    "cull_only": (15100, 0, 6),
    "reset": (3100, 2, 0),
}


def run_case(sf, name, step, frames, huge, seed, rec):
    g = torch.Generator().manual_seed(seed)
    n = 200
    m = make_model(sf, g, n, huge)
    opts = make_optimizers(m, g)
    pre = f"{name}__"
    rec[pre + "step"] = np.int64(step)
    for k, v in params(m).items():
        rec[pre + "in__" + k] = v.numpy()
    for k, (a, b, s) in moments(m, opts).items():
        rec[pre + "m1_in__" + k], rec[pre + "m2_in__" + k], rec[pre + "adam_step_in__" + k] = a.numpy(), b.numpy(), np.float64(s)
    m.step = step
    for f in range(frames):
        radii, grad = frame(m, g, n)
        m.after_train(step)
        rec[pre + f"frame{f}__radii"], rec[pre + f"frame{f}__xys_grad"] = radii.numpy(), grad.numpy()
        for s, t in (("grad_norm_sum", m.xys_grad_norm), ("vis_counts", m.vis_counts), ("max_2d_size", m.max_2Dsize)):
            rec[pre + f"frame{f}__{s}"] = t.numpy().copy()
    rec[pre + "frames"] = np.int64(frames)
    drawn = []
    randn = torch.randn

    def recording_randn(*a, **k):
        k.pop("device", None)
        t = randn(*a, generator=torch.Generator().manual_seed(seed + 1000), **k)
        drawn.append(t.clone())
        return t

    torch.randn = recording_randn
    try:
        m.refinement_after(opts, step)
    finally:
        torch.randn = randn
    assert len(drawn) <= 1
    rec[pre + "noise"] = (drawn[0] if drawn else torch.zeros((0, 3))).numpy()
    for k, v in params(m).items():
        rec[pre + "out__" + k] = v.numpy()
    for k, (a, b, s) in moments(m, opts).items():
        rec[pre + "m1_out__" + k], rec[pre + "m2_out__" + k], rec[pre + "adam_step_out__" + k] = a.numpy(), b.numpy(), np.float64(s)
    print(f"{name}: step {step}, {n} -> {m.means.shape[0]} Gaussians, {len(drawn[0]) if drawn else 0} noise rows")


def main():
    sf = import_splatfacto()
    sf.CONSOLE = types.SimpleNamespace(log=lambda *a, **k: None)
    rec = {}
    cfg = sf.SplatfactoModelConfig()
    rec["config_defaults"] = np.array(json.dumps({f: getattr(cfg, f) for f in REFINE_FIELDS}, sort_keys=True))
    rec["size"] = np.array(SIZE, dtype=np.int64)
    rec["num_train_data"] = np.int64(NUM_TRAIN_DATA)
    rec["cases"] = np.array(list(CASES))
    assert all(f.name in {x.name for x in dataclasses.fields(cfg)} for f in dataclasses.fields(cfg))
    for i, (name, (step, frames, huge)) in enumerate(CASES.items()):
        run_case(sf, name, step, frames, huge, 100 + i, rec)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
