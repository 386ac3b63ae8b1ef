"""Scenes, references and floors of the splat backward parity tests (tests/test_splat_backward_cases_cpu.py, ..._gpu.py).  Not a test module.

Scenes: the forward parity suite's builders, cameras and backgrounds (tests/test_splat_forward_cpu.py), at the smallest shapes that keep the
property the backward must survive -- tile lists of three and more 256-record batches whose front batch is partial (`deep`), tiles where some
pixels hit the 1e-4 stop and others run on (`opaque`), ragged image edges, an image inside one tile, opacities around 1/255, Gaussians over
every tile, equal depths -- plus `single` (one Gaussian, N = 1) and `clamped` (blends on the 0.999 clamp, which no forward scene reaches).
Every scene but the tied pairs of `ties` is depth-separated (sf.separate_depths): two view-space depths closer than float32 can order make the float32 and the float64
reference composite in opposite orders, and the "float32 floor" of such a scene (1e-3 of the largest gradient entry) would hide a lost blend.

References per configuration (case, raster mode, SH degree, separate-opacity variant or None), computed once (`reference`):
  g64     float64 autograd through splat_functional.render / splat_sep_functional.render, upstream images zeroed on flagged pixels
  g32     the same in float32
  walk32  `raster_backward_walk` in float32, chained to the parameters through splat_functional's projection
The floor of a gradient is max(err(g32), err(walk32), 2^-23), each error max-abs against g64 relative to g64's largest entry over the kept
Gaussians (`floors`).  The walk is the published tile rasteriser's backward: back to front from each pixel's last contributor, the
transmittance rebuilt by T <- T / (1 - alpha); its float32 error is what an implementation of that algorithm cannot avoid."""
from __future__ import annotations

import functools
import math
import time
from typing import Optional

import torch
from torch import Tensor

import splat_functional as sf
import splat_oracle as so
import splat_sep_functional as ssf
import test_splat_forward_cpu as fc

EPS = 2.0 ** -23
MIN_GAP, MIN_GAP_KEPT = 2.5e-5, 2e-5  # asked of sf.separate_depths / what survives the rounding of the means to float32
MAX_FLAGGED_PIXELS, MAX_EXCLUDED_GAUSSIANS = 0.10, 0.01  # conditions on the scenes, not measurements
MAX_FLOOR = 2e-5
LOGIT_GATE = math.log((1.0 / 255.0) / (1.0 - 1.0 / 255.0))
SH_C0 = 0.28209479177387814
BW = so.BLOCK_WIDTH


def _single(deg):
    """One large Gaussian at the point the camera looks at: N = 1 and a run of 3 x 2 pairs on a 33 x 17 frame."""
    p = sf.scene(1, 28, deg)
    return fc._with(p, means=torch.zeros(1, 3), scales=torch.tensor([[-0.5, -0.9, -0.7]]), opacities=torch.tensor([[2.0]]))


def _clamped(deg):
    """No forward scene reaches the 0.999 clamp (their logits end at 4: alpha <= 0.982).  Here 15 Gaussians with logit 9 sit a tenth of a
    pixel from pixel centres 8 apart, in front of the cloud, each with a logit-2 Gaussian far behind it: the centre pixels blend the front
    one at alpha = 0.999 -- 1 - alpha = 1e-3 in the division that rebuilds T and under `rest`, the geometry and opacity gradient of that
    blend switched off -- and go on to what lies behind.  (One such Gaussian ALONE is no test scene: sigmoid' = o (1 - o) with
    1 - o = 1.2e-4 is known to 1e-4 only in float32; among others its opacity gradient is small against the largest entry.)"""
    p = sf.scene(200, 29, deg, extent=0.5, scale_range=(-3.2, -2.4))
    c2w, fx, fy, cx, cy, W, H = fc.case_camera("clamped", CASES)
    viewmat, _ = so.camera_matrices(c2w, fx, fy, W, H)
    iy, ix = (t.reshape(-1).float() for t in torch.meshgrid(torch.arange(4, H, 8), torch.arange(4, W, 8), indexing="ij"))
    n = ix.shape[0]
    mu, sc, op = p["means"].clone(), p["scales"].clone(), p["opacities"].clone()
    for k, (z, logit) in enumerate(((2.0, 9.0), (2.9, 2.0))):
        zs = z + 0.004 * torch.arange(n)
        view = torch.stack([(ix + 1.1 - cx) * zs / fx, (iy + 0.9 - cy) * zs / fy, zs], -1)  # xys = f X / Z + c - 0.5; the pixel's centre: i + 0.5
        mu[k * n:(k + 1) * n] = (view - viewmat[:3, 3]) @ viewmat[:3, :3]
        sc[k * n:(k + 1) * n] = -1.5
        op[k * n:(k + 1) * n] = logit
    return fc._with(p, means=mu, scales=sc, opacities=op)


# name -> (scene, W, H, fov in degrees (of W), (cx, cy), eye): the layout of fc.CASES
CASES = {
    "deep": (lambda deg: fc._deep(deg, 1200, 0.4), 32, 32, 40.0, (15.5, 16.5), (2.3, 0.3, 0.6)),
    "opaque": (lambda deg: fc._opaque(deg, 1500), 43, 37, 60.0, (21.0, 19.0), (2.6, 0.4, 0.9)),
    "ragged": (lambda deg: fc._ragged(deg, 600), 70, 37, 45.0, (36.3, 17.9), (2.6, 0.4, 0.9)),  # 45 degrees: the cloud reaches the last column
    "sliver": fc.CASES["sliver"],
    "subtile": fc.CASES["subtile"],
    "faint": fc.CASES["faint"],
    "huge": fc.CASES["huge"],
    "ties": fc.CASES["ties"],
    "single": (_single, 33, 17, 60.0, (17.1, 8.95), (2.5, 0.0, 0.0)),
    "clamped": (_clamped, 40, 24, 60.0, (19.7, 12.2), (2.4, 0.3, 0.5)),
}
FAINT = 500  # the Gaussians fc._faint spreads around the 1/255 gate
# (case, raster mode, SH degree, separate-opacity variant)
CONFIGS = [("deep", "classic", 3, None), ("deep", "antialiased", 3, None), ("opaque", "classic", 3, None), ("opaque", "antialiased", 3, None),
           ("ragged", "classic", 3, None), ("ragged", "antialiased", 0, None), ("ragged", "classic", 1, None), ("sliver", "antialiased", 3, None),
           ("subtile", "classic", 3, None), ("faint", "antialiased", 3, None), ("huge", "classic", 3, None), ("ties", "antialiased", 3, None),
           ("single", "classic", 3, None), ("clamped", "classic", 3, None)]  # (the compensation keeps antialiased opacities off the clamp)
SEP_CONFIGS = [("deep", "classic", 3, "noise"), ("opaque", "classic", 3, "thermal_low"), ("opaque", "classic", 3, "rgb_low"), ("faint", "classic", 3, "mirror")]
ALL_CONFIGS = CONFIGS + SEP_CONFIGS
# where single pixels are probed (probe_pixels)
PROBE_CONFIGS = [("deep", "classic", 3, None), ("opaque", "classic", 3, None), ("ragged", "classic", 3, None), ("sliver", "antialiased", 3, None),
                 ("huge", "classic", 3, None), ("opaque", "classic", 3, "thermal_low"), ("opaque", "classic", 3, "rgb_low")]


def config_id(cfg):
    case, mode, deg, sep = cfg
    return f"{case}-{mode}-{deg}" + (f"-sep-{sep}" if sep else "")


def case_camera(case):
    return fc.case_camera(case, CASES)


def images(sep):
    return (("rgb", 3), ("thermal", 1), ("accumulation", 1)) + ((("accumulation_thermal", 1),) if sep else ())


def param_names(sep):
    return ssf.PARAM_NAMES if sep else sf.PARAM_NAMES


def scene(case, deg, sep=None, swapped=False):
    """The case's Gaussians (float32), depth-separated for the case's camera; sep: with the variant's thermal opacity logits.
    swapped (`ties`): the members of every tied pair in the other order."""
    p = CASES[case][0](deg)
    c2w = case_camera(case)[0]
    fixed = None
    if case == "ties":
        fixed = torch.zeros(p["means"].shape[0], dtype=torch.bool)
        fixed[:2 * fc.TIE_PAIRS] = True
    p = fc._with(p, means=sf.separate_depths(p["means"], c2w, MIN_GAP, fixed))
    if swapped:
        p = fc.swap_ties(p)
    if sep is None:
        return p
    op = p["opacities"]
    if sep == "noise":
        g = torch.Generator().manual_seed(31)
        return fc._with(p, opacities_thermal=op + torch.rand(op.shape, generator=g) - 0.5)
    if sep == "thermal_low":  # the thermal chain runs batches further than the RGB chain
        return fc._with(p, opacities_thermal=torch.full_like(op, -1.0))
    if sep == "rgb_low":
        return fc._with(p, opacities=torch.full_like(op, -1.0), opacities_thermal=torch.full_like(op, 3.0))
    if sep == "mirror":  # the faint ones mirrored about logit(1/255): gated in one chain only
        op_t = op.clone()
        op_t[:FAINT] = 2.0 * LOGIT_GATE - op[:FAINT]
        return fc._with(p, opacities_thermal=op_t)
    raise ValueError(sep)


def _deg_use(deg):
    return deg if deg > 0 else -1


def _render(params, case, mode, deg, sep, **kw):
    bg, bgt = fc.background()
    return (ssf.render if sep else sf.render)(params, *case_camera(case), sh_degree_to_use=_deg_use(deg), rasterize_mode=mode, background=bg,
                                              background_thermal=bgt, flag_tol=fc.FLAG_TOL, **kw)


def stats64(p, case, mode, deg, sep):
    """The float64 render with the walk's statistics and every flag (no gradient)."""
    with torch.no_grad():
        return _render({k: v.double() for k, v in p.items()}, case, mode, deg, sep, with_depth=True)


def upstream(case, sep, flag_pixels, scale=1.0):
    """One random upstream image per differentiable output (float64), zero on the flagged pixels."""
    _, W, H = case_camera(case)[4:]
    gen = torch.Generator().manual_seed(sum(map(ord, case)))
    keep = (~flag_pixels)[..., None]
    return {k: scale * torch.randn(H, W, c, generator=gen, dtype=torch.float64) * keep for k, c in images(sep)}


def _leaves(p, dt):
    return {k: v.to(dt).requires_grad_(True) for k, v in p.items()}


def _named(leaves, grads, xys_grad):
    out = {k: (torch.zeros_like(v) if g is None else g).detach().double() for (k, v), g in zip(leaves.items(), grads)}
    out["xys"] = xys_grad.detach().double()
    return out


def autograd_grads(p, case, mode, deg, sep, w, dt, with_stats=False):
    """d sum(output * w) / d every parameter and d xys, by autograd through the restatement in `dt`.  with_stats (separate mode, whose
    restatement differentiates the render that also reports the statistics): w is drawn here, zero on the pixels this render flags;
    returns (gradients, the render, w)."""
    leaves = _leaves(p, dt)
    out = _render(leaves, case, mode, deg, sep, **({"with_depth": True} if with_stats else {}))
    if with_stats:
        w = upstream(case, sep, out["flag_pixels"])
    loss = sum((out[k] * w[k].to(dt)).sum() for k in w)
    grads = torch.autograd.grad(loss, list(leaves.values()) + [out["xys"]], allow_unused=True)
    named = _named(leaves, grads[:-1], grads[-1])
    if not with_stats:
        return named
    out["stopped_fraction"] = float(out["stopped"].float().mean())
    return named, {k: (v.detach() if isinstance(v, Tensor) else {a: b.detach() for a, b in v.items()} if isinstance(v, dict) else v) for k, v in out.items()}, w


# ------------------------------------------------------------------------------------------------ the published backward walk
def projected(params, case, mode, deg):
    """What the rasteriser reads, as sf.render prepares it (differentiable): sf.project's dict plus `colors` [N,4] (RGB + thermal), `op` [N]
    and, with opacities_thermal among the parameters, `op_t` [N]."""
    c2w, fx, fy, cx, cy, W, H = case_camera(case)
    dt = params["means"].dtype
    viewmat, projmat = (m.to(dt) for m in so.camera_matrices(c2w, fx, fy, W, H))
    quats = params["quats"] / params["quats"].norm(dim=-1, keepdim=True)
    pj = dict(sf.project(params["means"], torch.exp(params["scales"]), quats, viewmat, projmat, fx, fy, cx, cy, H, W, flag_tol=fc.FLAG_TOL))
    viewdirs = params["means"].detach() - c2w[:3, 3].to(dt)
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    col = torch.cat([params["features_dc"][:, None, :], params["features_rest"]], 1)
    col_t = torch.cat([params["features_dc_thermal"][:, None, :], params["features_rest_thermal"]], 1)
    if deg > 0:
        sh = torch.cat([so.spherical_harmonics(deg, viewdirs, col), so.spherical_harmonics(deg, viewdirs, col_t)], -1) + 0.5
        pj["near_sh"] = (sh.detach().abs() < fc.FLAG_TOL).any(-1)
        pj["colors"] = torch.clamp(sh, min=0.0)
    else:
        pj["near_sh"] = torch.zeros(col.shape[0], dtype=torch.bool)
        pj["colors"] = torch.sigmoid(torch.cat([col[:, 0], col_t[:, 0]], -1))
    scale = pj["compensation"] if mode == "antialiased" else 1.0
    pj["op"] = torch.sigmoid(params["opacities"])[:, 0] * scale
    if "opacities_thermal" in params:
        pj["op_t"] = torch.sigmoid(params["opacities_thermal"])[:, 0] * scale
    return pj


def _pixel_grid(H, W, dt):
    return torch.meshgrid(torch.arange(H, dtype=dt) + 0.5, torch.arange(W, dtype=dt) + 0.5, indexing="ij")


def _boxes(tile_min, tile_max, H, W):
    lo, hi = (tile_min * BW).tolist(), (tile_max * BW).tolist()
    return [(slice(y0, min(y1, H)), slice(x0, min(x1, W))) for (x0, y0), (x1, y1) in zip(lo, hi)]


def _alpha(xys, conics, opacity, g, px, py):
    dx, dy = xys[g, 0] - px, xys[g, 1] - py
    sigma = 0.5 * (conics[g, 0] * dx * dx + conics[g, 2] * dy * dy) + conics[g, 1] * dx * dy
    raw = opacity[g] * torch.exp(-sigma)
    alpha = torch.clamp(raw, max=0.999)
    return dx, dy, sigma, raw, alpha, (sigma >= 0) & (alpha >= 1.0 / 255.0)


@torch.no_grad()
def raster_forward_walk(xys, depths, radii, conics, tile_min, tile_max, colors, opacity, background, H, W):
    """The front-to-back walk of sf.rasterize, every Gaussian on the pixels of its tile box only.  `img` [H,W,C] (before the output clamp),
    `T` [H,W] (the final transmittance), `last` [H,W] (rank in `order` of the pixel's last contributor, -1: none), `count` [H,W]
    (contributors), `stopped` [H,W], `used` [N] (the Gaussian is some pixel's contributor), `order` (depth order of the visible ones)."""
    dt, N = colors.dtype, colors.shape[0]
    order = torch.argsort(depths, stable=True)
    order = order[radii[order] > 0]
    py, px = _pixel_grid(H, W, dt)
    box = _boxes(tile_min, tile_max, H, W)
    T = torch.ones(H, W, dtype=dt)
    img = torch.zeros(H, W, colors.shape[1], dtype=dt)
    done = torch.zeros(H, W, dtype=torch.bool)
    last = torch.full((H, W), -1)
    count = torch.zeros(H, W, dtype=torch.long)
    used = torch.zeros(N, dtype=torch.bool)
    for r, g in enumerate(order.tolist()):
        s = box[g]
        _, _, _, _, alpha, use = _alpha(xys, conics, opacity, g, px[s], py[s])
        use = use & ~done[s]
        next_T = T[s] * (1.0 - alpha)
        stop = use & (next_T <= 1e-4)
        done[s] |= stop
        use = use & ~stop
        img[s] += torch.where(use[..., None], (alpha * T[s])[..., None] * colors[g], torch.zeros((), dtype=dt))
        T[s] = torch.where(use, next_T, T[s])
        last[s] = torch.where(use, r, last[s])
        count[s] += use
        used[g] = bool(use.any())
    return {"img": img + T[..., None] * background, "T": T, "last": last, "count": count, "stopped": done, "used": used, "order": order}


@torch.no_grad()
def raster_backward_walk(xys, conics, colors, opacity, tile_min, tile_max, order, final_T, last, v_img, v_alpha, background):
    """The backward of the published tile rasteriser, in the dtype of its inputs.  Every pixel starts from its final transmittance
    `final_T` and walks its list back to front from its last contributor `last` (rank in `order`), with the forward's use rules:
        T <- T / (1 - alpha)                                  the transmittance in front of the Gaussian
        d alpha = T <c, v> - rest / (1 - alpha)               rest: what lies behind, through T -- sum of alpha_j T_j <c_j, v>, started
        rest <- rest + alpha T <c, v>                         at final_T (<background, v> - v_alpha)
    d colour = alpha T v; the 0.999 clamp passes d alpha to the raw value where torch.clamp does (raw <= 0.999).
    v_img [H,W,C]: the gradient of the image before the output clamp; v_alpha [H,W]: of the accumulation 1 - final_T.
    Returns d xys [N,2], d conics [N,3], d colors [N,C], d opacity [N]."""
    dt, N = colors.dtype, colors.shape[0]
    H, W = final_T.shape
    py, px = _pixel_grid(H, W, dt)
    box = _boxes(tile_min, tile_max, H, W)
    T = final_T.clone()
    rest = final_T * ((v_img * background).sum(-1) - v_alpha)
    d_xys, d_conics = torch.zeros(N, 2, dtype=dt), torch.zeros(N, 3, dtype=dt)
    d_colors, d_op = torch.zeros(N, colors.shape[1], dtype=dt), torch.zeros(N, dtype=dt)
    zero = torch.zeros((), dtype=dt)
    ranks = order.tolist()
    for r in range(len(ranks) - 1, -1, -1):
        g, s = ranks[r], box[ranks[r]]
        dx, dy, sigma, raw, alpha, use = _alpha(xys, conics, opacity, g, px[s], py[s])
        use = use & (last[s] >= r)
        if not bool(use.any()):
            continue
        om = 1.0 - alpha
        T_front = torch.where(use, T[s] / om, T[s])
        cv = (v_img[s] * colors[g]).sum(-1)
        vis = alpha * T_front
        d_alpha = torch.where(use, T_front * cv - rest[s] / om, zero)
        rest[s] = torch.where(use, rest[s] + vis * cv, rest[s])
        T[s] = T_front
        d_colors[g] = torch.where(use[..., None], vis[..., None] * v_img[s], zero).sum((0, 1))
        d_raw = torch.where(raw <= 0.999, d_alpha, zero)
        d_op[g] = (d_raw * torch.exp(-sigma)).sum()
        d_sigma = -d_raw * raw
        d_conics[g] = torch.stack([(0.5 * d_sigma * dx * dx).sum(), (d_sigma * dx * dy).sum(), (0.5 * d_sigma * dy * dy).sum()])
        d_xys[g] = torch.stack([(d_sigma * (conics[g, 0] * dx + conics[g, 1] * dy)).sum(), (d_sigma * (conics[g, 1] * dx + conics[g, 2] * dy)).sum()])
    return d_xys, d_conics, d_colors, d_op


def _chains(pj, w, sep, dt):
    """(colours, opacity, background, upstream image, upstream accumulation, columns of `colors`) of each compositing chain."""
    bg, bgt = fc.background()
    bg4 = torch.cat([bg, torch.tensor([bgt])]).to(dt)
    col = pj["colors"].detach()
    if not sep:
        return [(col, pj["op"].detach(), bg4, torch.cat([w["rgb"], w["thermal"]], -1).to(dt), w["accumulation"][..., 0].to(dt), slice(0, 4), "op")]
    return [(col[:, :3], pj["op"].detach(), bg4[:3], w["rgb"].to(dt), w["accumulation"][..., 0].to(dt), slice(0, 3), "op"),
            (col[:, 3:], pj["op_t"].detach(), bg4[3:], w["thermal"].to(dt), w["accumulation_thermal"][..., 0].to(dt), slice(3, 4), "op_t")]


def walk_grads(p, case, mode, deg, sep, w, dt):
    """The same gradients as autograd_grads from raster_backward_walk, chained to the parameters through `projected`."""
    _, W, H = case_camera(case)[4:]
    leaves = _leaves(p, dt)
    pj = projected(leaves, case, mode, _deg_use(deg))
    geom = {k: pj[k].detach() for k in ("xys", "depths", "radii", "conics", "tile_min", "tile_max")}
    N = geom["xys"].shape[0]
    d_xys, d_conics, d_colors = torch.zeros(N, 2, dtype=dt), torch.zeros(N, 3, dtype=dt), torch.zeros(N, 4, dtype=dt)
    outs, cots = [pj["xys"], pj["conics"], pj["colors"]], []
    for col, op, bg, v, v_acc, cols, op_key in _chains(pj, w, sep, dt):
        fw = raster_forward_walk(geom["xys"], geom["depths"], geom["radii"], geom["conics"], geom["tile_min"], geom["tile_max"], col, op, bg, H, W)
        v_img = torch.where(fw["img"] <= 1.0, v, torch.zeros((), dtype=dt))  # the output clamp passes gradient where torch.clamp does
        gx, gc, gcol, gop = raster_backward_walk(geom["xys"], geom["conics"], col, op, geom["tile_min"], geom["tile_max"], fw["order"], fw["T"],
                                                 fw["last"], v_img, v_acc, bg)
        d_xys, d_conics = d_xys + gx, d_conics + gc
        d_colors[:, cols] = gcol
        outs.append(pj[op_key])
        cots.append(gop)
    grads = torch.autograd.grad(outs, list(leaves.values()), grad_outputs=[d_xys, d_conics, d_colors] + cots, allow_unused=True)
    return _named(leaves, grads, d_xys)


# ------------------------------------------------------------------------------------------------ references and floors
@functools.lru_cache(maxsize=None)
def reference(case, mode, deg, sep=None, swapped=False):
    """Everything the tests of one configuration share, computed once and never modified: the scene `p`, the float64 statistics `st`, the
    upstream images `w`, the gradients `g64`, `g32`, `walk32` (dicts over the parameters and "xys", float64 tensors) and `seconds`."""
    t0 = time.perf_counter()
    p = scene(case, deg, sep, swapped)
    if sep:
        g64, st, w = autograd_grads(p, case, mode, deg, sep, None, torch.float64, with_stats=True)
    else:
        st = stats64(p, case, mode, deg, sep)
        w = upstream(case, sep, st["flag_pixels"])
        g64 = autograd_grads(p, case, mode, deg, sep, w, torch.float64)
    g32 = autograd_grads(p, case, mode, deg, sep, w, torch.float32)
    walk32 = walk_grads(p, case, mode, deg, sep, w, torch.float32)
    return {"p": p, "st": st, "w": w, "g64": g64, "g32": g32, "walk32": walk32, "seconds": time.perf_counter() - t0}


def amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def rel_err(a, b, keep):
    """max |a - b| over the kept rows, relative to the largest kept entry of b (0 when b is all zero and a too)."""
    a, b = a.double()[keep], b.double()[keep]
    scale = amax(b)
    if scale == 0.0:
        return 0.0 if amax(a) == 0.0 else math.inf
    return amax(a - b) / scale


def cpu_excluded(st):
    """Gaussians left out of a gradient comparison for a decision of their own that the CPU can see: a view-space position on the frustum
    clamp (the GPU test adds those whose integer radius differs on the GPU)."""
    return st["projection"]["near_clamp"] & st["projection"]["ok"]


def floors(ref, excl, sep):
    """Per gradient: (floor, err of float32 autograd, err of the float32 walk), over the Gaussians outside `excl`."""
    out = {}
    for k in list(param_names(sep)) + ["xys"]:
        ea, ew = rel_err(ref["g32"][k], ref["g64"][k], ~excl), rel_err(ref["walk32"][k], ref["g64"][k], ~excl)
        out[k] = (max(ea, ew, EPS), ea, ew)
    return out


@functools.lru_cache(maxsize=None)
def swapped_reference(case, mode, deg, sep=None):
    """`ties`: float64 gradients in index order (`own`) and with the members of every tied pair swapped (`other`, mapped back to the
    Gaussians' own rows), both under ONE upstream image `w`: the configuration's, zeroed also where the swapped walk flags a pixel."""
    ref = reference(case, mode, deg, sep)
    p_sw = scene(case, deg, sep, swapped=True)
    st_sw = stats64(p_sw, case, mode, deg, sep)
    w = {k: v * (~st_sw["flag_pixels"])[..., None] for k, v in ref["w"].items()}
    own = autograd_grads(ref["p"], case, mode, deg, sep, w, torch.float64)
    other = autograd_grads(p_sw, case, mode, deg, sep, w, torch.float64)
    n = fc.TIE_PAIRS
    back = torch.arange(ref["p"]["means"].shape[0])
    back[:n], back[n:2 * n] = torch.arange(n, 2 * n), torch.arange(n)  # row i of the swapped scene is Gaussian back[i]; the map is its own inverse
    return {"w": w, "own": own, "other": {k: v[back] for k, v in other.items()}}


def visible_depth_gap(st, tied: Optional[int] = None):
    """The smallest gap between sorted float64 depths of the visible Gaussians; tied: that many pairs (i, i + tied) count once."""
    ok = st["projection"]["ok"].clone()
    if tied:
        ok[tied:2 * tied] = False
    d = torch.sort(st["projection"]["depths"][ok]).values
    return float((d[1:] - d[:-1]).min()) if d.numel() > 1 else math.inf


# ------------------------------------------------------------------------------------------------ single-pixel probes
def probe_pixel(pj, opacity, ix, iy, flag_tol=fc.FLAG_TOL):
    """One pixel's list in float64, vectorised: sort, alpha per Gaussian, use mask, exclusive cumulative product, first stop.  Returns
    `weight` [N] = alpha_g T_g where the pixel blends g (else 0), `flagged` [N] (a decision of g at this pixel is within flag_tol of its
    threshold), `T` (the final transmittance) and `stopped`.  Independent of the loops above: nothing is walked."""
    N = opacity.shape[0]
    tile = torch.tensor([ix // BW, iy // BW])
    inbox = pj["ok"] & (pj["tile_min"] <= tile).all(-1) & (tile < pj["tile_max"]).all(-1)
    o = torch.argsort(pj["depths"], stable=True)
    o = o[inbox[o]]
    dx, dy = pj["xys"][o, 0] - (ix + 0.5), pj["xys"][o, 1] - (iy + 0.5)
    c = pj["conics"][o]
    sigma = 0.5 * (c[:, 0] * dx * dx + c[:, 2] * dy * dy) + c[:, 1] * dx * dy
    raw = opacity[o] * torch.exp(-sigma)
    alpha = torch.clamp(raw, max=0.999)
    use = (sigma >= 0) & (alpha >= 1.0 / 255.0)
    keep = torch.where(use, 1.0 - alpha, torch.ones_like(alpha))
    T_in = torch.cat([torch.ones(1, dtype=alpha.dtype), torch.cumprod(keep, 0)[:-1]])
    T_out = T_in * keep
    stop = (use & (T_out <= 1e-4)).nonzero()
    first = int(stop[0]) if stop.numel() else o.numel()
    live = torch.arange(o.numel()) <= first
    use = use & (torch.arange(o.numel()) < first)
    near = live & (((alpha * 255.0 - 1).abs() < flag_tol) | ((raw / 0.999 - 1).abs() < flag_tol) | ((sigma >= 0) & (alpha >= 1.0 / 255.0) & ((T_out * 1e4 - 1).abs() < 1e2 * flag_tol)))
    weight, flagged = torch.zeros(N, dtype=alpha.dtype), torch.zeros(N, dtype=torch.bool)
    weight[o] = torch.where(use, alpha * T_in, torch.zeros_like(alpha))
    flagged[o] = near
    T = float(T_in[first]) if first < o.numel() else (float(T_out[-1]) if o.numel() else 1.0)
    return {"weight": weight, "flagged": flagged, "T": T, "stopped": first < o.numel()}


def clamped_blends(pj, fw, opacity, H, W):
    """[H,W] each: how many of the pixel's contributors it blends on the 0.999 clamp (raw alpha above it), and how many of those are not
    its last contributor."""
    py, px = _pixel_grid(H, W, opacity.dtype)
    n, inner = torch.zeros(H, W, dtype=torch.long), torch.zeros(H, W, dtype=torch.long)
    for r, g in enumerate(fw["order"].tolist()):
        _, _, _, raw, _, use = _alpha(pj["xys"], pj["conics"], opacity, g, px, py)
        x0, y0 = (pj["tile_min"][g] * BW).tolist()
        x1, y1 = (pj["tile_max"][g] * BW).tolist()
        n[y0:y1, x0:x1] += (use & (fw["last"] >= r) & (raw > 0.999))[y0:y1, x0:x1]
        inner[y0:y1, x0:x1] += (use & (fw["last"] > r) & (raw > 0.999))[y0:y1, x0:x1]
    return n, inner


def walk_stats(p, case, mode, deg, sep=None, chain="op"):
    """The float64 forward walk of one chain on the case (per-pixel `count`, `stopped`, `last`, ..., see raster_forward_walk) and the
    projected quantities it used."""
    _, W, H = case_camera(case)[4:]
    with torch.no_grad():
        pj = projected({k: v.double() for k, v in p.items()}, case, mode, _deg_use(deg))
        dt = torch.float64
        w0 = {k: torch.zeros(H, W, c, dtype=dt) for k, c in images(sep)}
        col, op, bg, _, _, _, _ = [ch for ch in _chains(pj, w0, sep, dt) if ch[6] == chain][0]
        fw = raster_forward_walk(pj["xys"], pj["depths"], pj["radii"], pj["conics"], pj["tile_min"], pj["tile_max"], col, op, bg, H, W)
    return pj, fw


def _argmax2d(score, mask):
    """(ix, iy) of the largest `score` under `mask`, or None when the mask is empty."""
    if not bool(mask.any()):
        return None
    s = torch.where(mask, score.double(), torch.full((), -math.inf, dtype=torch.float64))
    i = int(s.argmax())
    return i % score.shape[1], i // score.shape[1]


def probe_pixels(case, mode, deg, sep=None):
    """Up to six pixels of the configuration, chosen from the float64 statistics, at which the thermal chain's list is probed: unflagged
    (in any walk) and with the thermal value below the output clamp.  Returns [(label, ix, iy)], the projection and the thermal chain's
    opacity."""
    ref = reference(case, mode, deg, sep)
    st = ref["st"]
    pj, fw = walk_stats(ref["p"], case, mode, deg, sep, "op_t" if sep else "op")
    H, W = fw["T"].shape
    ok = ~st["flag_pixels"] & (fw["img"][..., -1] < 1.0)
    iy, ix = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    acc = 1.0 - fw["T"]
    picks = [("most contributors", _argmax2d(fw["count"], ok)), ("last column", _argmax2d(acc, ok & (ix == W - 1) & (fw["count"] > 0))),
             ("last row", _argmax2d(acc, ok & (iy == H - 1) & (fw["count"] > 0)))]
    per_tile = st["contributors_per_tile"]
    ty, tx = divmod(int(per_tile.argmax()), per_tile.shape[1])
    if case == "opaque":
        tile = (iy // BW == ty) & (ix // BW == tx)
        quad = (iy // 8) * ((W + 7) // 8) + ix // 8
        for q in quad[tile].unique().tolist():
            a, b = ok & (quad == q) & fw["stopped"], ok & (quad == q) & ~fw["stopped"]
            if bool(a.any()) and bool(b.any()):
                picks += [("stopped, longest list", _argmax2d(fw["count"], a)), ("running, same quadrant", _argmax2d(fw["count"], b))]
                break
    if case == "huge":  # every tile is under the full-screen Gaussians: the far corner's
        picks.append(("corner tile", _argmax2d(fw["count"], ok & (iy // BW == (H - 1) // BW) & (ix // BW == (W - 1) // BW))))
    if sep:  # the thermal chain against the RGB chain
        _, rgb = walk_stats(ref["p"], case, mode, deg, sep, "op")
        picks += [("thermal runs longer than RGB", _argmax2d(fw["last"] - rgb["last"], ok & (fw["last"] > rgb["last"]) & rgb["stopped"])),
                  ("thermal stops earlier than RGB", _argmax2d(rgb["last"] - fw["last"], ok & (fw["last"] < rgb["last"]) & fw["stopped"]))]
    seen, out = set(), []
    for label, xy in picks:
        if xy is not None and xy not in seen:
            seen.add(xy)
            out.append((label, xy[0], xy[1]))
    return out, pj, pj["op_t" if sep else "op"]
