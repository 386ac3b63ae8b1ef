"""Float64 reference of the absgrad densification statistic (tests/test_splat_absgrad_cpu.py, ..._gpu.py).  Not a test module.

For Gaussian g and pixel p let d sigma[g,p] be the derivative of the frame's scalar loss with respect to the quadratic form sigma[g,p]
(alpha = opacity exp(-sigma)) through pixel p's compositing -- in separate-opacity mode the sum of the RGB chain's and the thermal chain's
term -- and J[g,p] = d sigma[g,p] (cx dx + cy dy, cy dx + cz dy) the pixel's term of d xys.  Then
    v_xys[g]     = sum_p J[g,p]                      what the backward has always produced (bc.reference(...)["g64"]["xys"])
    v_xys_abs[g] = sum_p (|J[g,p].x|, |J[g,p].y|)    the statistic of AbsGS / gsplat's `absgrad`
`raster_backward_walk_abs` is bc.raster_backward_walk with every chain of the frame advanced together, so that the absolute value is taken
after the chains are added.  Its signed sum is checked against float64 autograd, its absolute sum on the two small scenes against float64
autograd with the upstream image restricted to one pixel at a time (`per_pixel_autograd_abs`).  Scenes, cameras, upstream images, flagged
pixels and excluded Gaussians are those of tests/splat_backward_cases.py."""
from __future__ import annotations

import functools

import torch

import splat_backward_cases as bc

# (case, raster mode, SH degree, separate-opacity variant): what each one exercises is listed in tests/test_splat_absgrad_gpu.py
SHARED_CONFIGS = [("deep", "classic", 3, None), ("opaque", "antialiased", 3, None), ("ragged", "classic", 1, None), ("clamped", "classic", 3, None),
                  ("single", "classic", 3, None), ("faint", "antialiased", 3, None)]
SEP_CONFIGS = [("deep", "classic", 3, "noise"), ("faint", "classic", 3, "mirror"), ("opaque", "classic", 3, "thermal_low")]
CONFIGS = SHARED_CONFIGS + SEP_CONFIGS
IDS = [bc.config_id(c) for c in CONFIGS]
SMALL_CONFIGS = [("single", "classic", 3, None), ("clamped", "classic", 3, None)]  # where one autograd pass per pixel is affordable


@torch.no_grad()
def raster_backward_walk_abs(xys, conics, tile_min, tile_max, order, chains):
    """bc.raster_backward_walk over `order` (bc.raster_forward_walk's) for all chains of a frame at once, in the dtype of its inputs.
    chains: one (colors [N,C], opacity [N], final_T [H,W], last [H,W], v_img [H,W,C], v_alpha [H,W], background [C]) per compositing chain,
    each with the forward walk's results of that chain.  Returns (v_xys_abs [N,2], v_xys [N,2])."""
    dt, N = xys.dtype, xys.shape[0]
    H, W = chains[0][2].shape
    py, px = bc._pixel_grid(H, W, dt)
    box = bc._boxes(tile_min, tile_max, H, W)
    T = [ch[2].clone() for ch in chains]
    rest = [ch[2] * ((ch[4] * ch[6]).sum(-1) - ch[5]) for ch in chains]
    v_abs, v_sum = torch.zeros(N, 2, dtype=dt), torch.zeros(N, 2, dtype=dt)
    zero = torch.zeros((), dtype=dt)
    ranks = order.tolist()
    for r in range(len(ranks) - 1, -1, -1):
        g, s = ranks[r], box[ranks[r]]
        d_sigma, any_use = None, False
        for c, (colors, opacity, _, last, v_img, _, _) in enumerate(chains):
            dx, dy, _, raw, alpha, use = bc._alpha(xys, conics, opacity, g, px[s], py[s])
            use = use & (last[s] >= r)
            if not bool(use.any()):
                continue
            any_use = True
            om = 1.0 - alpha
            T_front = torch.where(use, T[c][s] / om, T[c][s])
            cv = (v_img[s] * colors[g]).sum(-1)
            d_alpha = torch.where(use, T_front * cv - rest[c][s] / om, zero)
            rest[c][s] = torch.where(use, rest[c][s] + alpha * T_front * cv, rest[c][s])
            T[c][s] = T_front
            term = -torch.where(raw <= 0.999, d_alpha, zero) * raw  # the clamp passes gradient where torch.clamp does
            d_sigma = term if d_sigma is None else d_sigma + term
        if not any_use:
            continue
        jx = d_sigma * (conics[g, 0] * dx + conics[g, 1] * dy)
        jy = d_sigma * (conics[g, 1] * dx + conics[g, 2] * dy)
        v_sum[g] = torch.stack([jx.sum(), jy.sum()])
        v_abs[g] = torch.stack([jx.abs().sum(), jy.abs().sum()])
    return v_abs, v_sum


def walk_abs(p, case, mode, deg, sep, w, dt):
    """(v_xys_abs, v_xys) of the scene `p` under the upstream images `w`, by the walk in `dt` (as bc.walk_grads prepares its chains)."""
    _, W, H = bc.case_camera(case)[4:]
    with torch.no_grad():
        pj = bc.projected({k: v.to(dt) for k, v in p.items()}, case, mode, bc._deg_use(deg))
        geom = [pj[k] for k in ("xys", "depths", "radii", "conics", "tile_min", "tile_max")]
        chains, order = [], None
        for col, op, bg, v, v_acc, _, _ in bc._chains(pj, w, sep, dt):
            fw = bc.raster_forward_walk(*geom, col, op, bg, H, W)
            v_img = torch.where(fw["img"] <= 1.0, v, torch.zeros((), dtype=dt))  # the output clamp passes gradient where torch.clamp does
            chains.append((col, op, fw["T"], fw["last"], v_img, v_acc, bg))
            order = fw["order"]  # the geometry's alone: the same for every chain
        return raster_backward_walk_abs(pj["xys"], pj["conics"], pj["tile_min"], pj["tile_max"], order, chains)


@functools.lru_cache(maxsize=None)
def reference(case, mode, deg, sep=None):
    """Computed once per configuration and never modified: `abs64`, `signed64` (the float64 walk), `abs32`, `signed32` (the float32 walk),
    all float64 tensors [N,2], beside bc.reference's own entries under `bc`."""
    ref = bc.reference(case, mode, deg, sep)
    a64, s64 = walk_abs(ref["p"], case, mode, deg, sep, ref["w"], torch.float64)
    a32, s32 = walk_abs(ref["p"], case, mode, deg, sep, ref["w"], torch.float32)
    return {"bc": ref, "abs64": a64, "signed64": s64, "abs32": a32.double(), "signed32": s32.double()}


def per_pixel_autograd_abs(case, mode, deg, sep=None):
    """The independent statement of v_xys_abs: float64 autograd of the render (sf.render / ssf.render through bc._render) with the upstream
    images of bc.reference restricted to ONE pixel at a time, the absolute values of the resulting xys gradients summed over the pixels.
    The pixels ride the batch dimension of one batched backward pass.  Nothing of the walk above is used."""
    ref = bc.reference(case, mode, deg, sep)
    leaves = {k: v.double().requires_grad_(True) for k, v in ref["p"].items()}
    out = bc._render(leaves, case, mode, deg, sep)
    H, W = out["rgb"].shape[:2]
    pix = torch.eye(H * W, dtype=torch.float64).reshape(H * W, H, W, 1)
    keys = list(ref["w"])
    cot = [pix * ref["w"][k][None] for k in keys]  # [P,H,W,C]: the upstream image of output k on pixel P only
    (g,) = torch.autograd.grad([out[k] for k in keys], [out["xys"]], grad_outputs=cot, is_grads_batched=True)
    return g.abs().sum(0)


def norm_ratio(v_abs, v_signed, keep):
    """Median over the kept Gaussians with a non-zero signed norm of |v_abs| / |v_signed| (row norms)."""
    na, ns = v_abs[keep].norm(dim=-1), v_signed[keep].norm(dim=-1)
    ok = ns > 0
    return float((na[ok] / ns[ok]).median())
