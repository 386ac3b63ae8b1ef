"""The ray contribution of every Gaussian restated in torch (csrc/tn_splat.hip: k_splat_raster_contrib -> k_splat_contrib_fold), for the tests of
tests/test_splat_contrib_cpu.py and ..._gpu.py.  Not a test module.

`contrib_walk` is splat_backward_cases.raster_forward_walk's loop -- front to back, every Gaussian on the pixels of its tile box, the same use,
stop and blend rules -- that returns per Gaussian instead of per pixel: with w = pixel_weight * alpha * T where the pixel blends the Gaussian
(else 0), `sum` = sum over pixels of w, `max` = max over pixels of w, `hits` = pixels with w > 0.  A Gaussian at which a pixel stops is not blended
there and scores nothing there.  It runs in the dtype of its inputs: float64 is the reference, float32 its own floor.  `contributions` builds its
inputs for a scene of splat_backward_cases from bc.projected / bc._chains, for either chain."""
from __future__ import annotations

import functools

import torch

import splat_backward_cases as bc

# the scenes the GPU test scores: (configuration, chain).  Shared mode: chain 0; separate mode: both chains
SHARED = [("deep", "classic", 3, None), ("deep", "antialiased", 3, None), ("opaque", "classic", 3, None), ("ragged", "classic", 3, None),
          ("subtile", "classic", 3, None), ("faint", "antialiased", 3, None), ("huge", "classic", 3, None), ("single", "classic", 3, None),
          ("clamped", "classic", 3, None)]
assert all(c in bc.CONFIGS for c in SHARED)
SCENES = [(c, 0) for c in SHARED] + [(c, ch) for c in bc.SEP_CONFIGS for ch in (0, 1)]


def scene_id(sc):
    return f"{bc.config_id(sc[0])}-chain{sc[1]}"


@torch.no_grad()
def contrib_walk(xys, depths, radii, conics, tile_min, tile_max, opacity, pixel_weight, H, W, probes=()):
    """`sum`, `max` [N] (the dtype of the inputs), `hits` [N] (int64), `T` [H,W] (the final transmittance), `stopped` [H,W], `order`, and for the
    pixels (ix, iy) of `probes` `probe_weight` [len(probes), N]: alpha T where that pixel blends the Gaussian (without the pixel weight)."""
    dt, N = opacity.dtype, opacity.shape[0]
    order = torch.argsort(depths, stable=True)
    order = order[radii[order] > 0]
    py, px = bc._pixel_grid(H, W, dt)
    box = bc._boxes(tile_min, tile_max, H, W)
    T = torch.ones(H, W, dtype=dt)
    done = torch.zeros(H, W, dtype=torch.bool)
    s, m = torch.zeros(N, dtype=dt), torch.zeros(N, dtype=dt)
    hits = torch.zeros(N, dtype=torch.long)
    probe_weight = torch.zeros(len(probes), N, dtype=dt)
    zero = torch.zeros((), dtype=dt)
    for g in order.tolist():
        sl = box[g]
        _, _, _, _, alpha, use = bc._alpha(xys, conics, opacity, g, px[sl], py[sl])
        use = use & ~done[sl]
        next_T = T[sl] * (1.0 - alpha)
        stop = use & (next_T <= 1e-4)
        done[sl] |= stop
        use = use & ~stop
        vis = torch.where(use, alpha * T[sl], zero)
        w = pixel_weight[sl] * vis
        if w.numel():
            s[g], m[g], hits[g] = w.sum(), w.max(), (w > 0).sum()
        for j, (ix, iy) in enumerate(probes):
            y, x = iy - sl[0].start, ix - sl[1].start
            if 0 <= y < vis.shape[0] and 0 <= x < vis.shape[1]:
                probe_weight[j, g] = vis[y, x]
        T[sl] = torch.where(use, next_T, T[sl])
    return {"sum": s, "max": m, "hits": hits, "T": T, "stopped": done, "order": order, "probe_weight": probe_weight}


def chain_opacity(pj, sep, chain):
    """The opacity [N] the chain blends with (bc._chains' `op` / `op_t`); shared mode has chain 0 only."""
    if chain not in (0, 1) or (chain == 1 and not sep):
        raise ValueError(f"chain {chain} of a {'separate' if sep else 'shared'}-mode scene")
    return pj["op_t" if chain else "op"].detach()


def contributions(p, case, mode, deg, sep, chain, dt, pixel_weight=None, probes=()):
    """contrib_walk of the scene `p` (float32 parameters) under the case's camera in dtype `dt`; pixel_weight [H,W] or None (1).  Returns the
    walk's dict plus `pj`, the projection it read."""
    _, W, H = bc.case_camera(case)[4:]
    with torch.no_grad():
        pj = bc.projected({k: v.to(dt) for k, v in p.items()}, case, mode, bc._deg_use(deg))
    pw = torch.ones(H, W, dtype=dt) if pixel_weight is None else pixel_weight.to(dt)
    out = contrib_walk(pj["xys"], pj["depths"], pj["radii"], pj["conics"], pj["tile_min"], pj["tile_max"], chain_opacity(pj, sep, chain), pw, H, W, probes)
    out["pj"] = pj
    return out


@functools.lru_cache(maxsize=None)
def scene_stats(case, mode, deg, sep=None):
    """The scene and its float64 render with every flag (bc.stats64), computed once and never modified."""
    p = bc.scene(case, deg, sep)
    return p, bc.stats64(p, case, mode, deg, sep)


@functools.lru_cache(maxsize=None)
def reference(cfg, chain):
    """What the tests of one (configuration, chain) share, computed once and never modified: the scene `p`, the float64 statistics `st`, the
    pixel weight `pw` (1, and 0 on the float64 render's flagged pixels), the float64 restatement `c64` and the float32 one `c32`."""
    case, mode, deg, sep = cfg
    p, st = scene_stats(*cfg)
    pw = (~st["flag_pixels"]).double()
    return {"p": p, "st": st, "pw": pw, "c64": contributions(p, case, mode, deg, sep, chain, torch.float64, pw),
            "c32": contributions(p, case, mode, deg, sep, chain, torch.float32, pw)}


def floor(ref, key, keep):
    """The float32 restatement's own error against float64 over the kept Gaussians, relative to the largest kept entry; at least 2^-23."""
    return max(bc.rel_err(ref["c32"][key], ref["c64"][key], keep), bc.EPS)


def conservation_error(c, pw):
    """|sum_g sum[g] - sum_p pw_p (1 - T_p)| relative to the right-hand side, in float64 from the walk's own dtype."""
    lhs, rhs = float(c["sum"].double().sum()), float((pw.double() * (1.0 - c["T"].double())).sum())
    return abs(lhs - rhs) / rhs if rhs > 0 else abs(lhs)
