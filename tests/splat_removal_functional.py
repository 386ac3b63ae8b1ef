"""Functional torch restatement of the removal renders of the separate thermal opacity (removal_min_opacity_diff), built on
splat_sep_functional.py / splat_functional.py: the reference of the removal tests, any dtype.

ThermalNeRF's rule (models/thermal_nerfacto.py:460-487) with opacities for densities.  With o = sigmoid(opacities), ot =
sigmoid(opacities_thermal) and thr = removal_min_opacity_diff: keep_rgb = |o - ot| < thr o, keep_th = |ot - o| < thr ot (strict: thr = 0 keeps
nothing; the reference's division form is NaN at zero density and compares false, as the product form does at o = 0).  `removal` is the RGB walk
of ssf.render over the same depth-sorted list with the opacity of every Gaussian outside keep_rgb set to 0 -- its own transmittance, stop and
background weight; `removal_thermal` likewise the thermal walk with keep_th.  The masks come from the plain opacities; "antialiased" multiplies
the blended opacities by the compensation, which would cancel in the comparison."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

import splat_functional as sf
import splat_oracle as so
import splat_sep_functional as ssf

THR = 0.05    # the tests' removal_min_opacity_diff
BAND = 1e-4   # no Gaussian of a test scene has | |o - ot| / o - THR | or | |o - ot| / ot - THR | below this: the kernel decides from a float32
#               log2 / exp2 round trip of each opacity (relative error ~1e-6), so no keep decision can differ between float32 and float64
STACK_KEPT = 2  # Gaussians of awkward_scene's opaque stack that both removal renders keep (removal_scene)
RATIO = 1.0512  # ot = RATIO o: |o - ot| / o = 0.0512 > THR > 0.0487 = |o - ot| / ot -- out of `removal`, in `removal_thermal`; o / RATIO: the reverse
# The GPU tests' frames, as ssf.CASES: (W, H, raster mode, config.sh_degree, roles of the two opacities reversed, seed of removal_scene).  Seeds
# for which test_splat_removal_cpu.py's scene conditions hold in float64 and in float32: four walks stop on these small frames, and 1 % of
# 33 x 17 pixels is five pixels -- a few hundred seeds were tried on the CPU for each frame.
CASES = [(40, 24, "classic", 0, False, 37), (33, 17, "antialiased", 3, True, 607), (33, 17, "classic", 3, False, 2222)]


def keep_masks(params: Dict[str, Tensor], thr: float) -> Tuple[Tensor, Tensor]:
    """(keep_rgb, keep_th) [N] bool, in the dtype of the parameters."""
    o, ot = torch.sigmoid(params["opacities"].detach())[:, 0], torch.sigmoid(params["opacities_thermal"].detach())[:, 0]
    d = (o - ot).abs()
    return d < thr * o, d < thr * ot


def threshold_distance(params: Dict[str, Tensor], thr: float) -> Tensor:
    """[N]: how far each Gaussian is from flipping a keep decision, relative to the opacity the comparison scales with:
    min(| |o - ot| / o - thr |, | |o - ot| / ot - thr |)."""
    o, ot = torch.sigmoid(params["opacities"].detach())[:, 0], torch.sigmoid(params["opacities_thermal"].detach())[:, 0]
    d = (o - ot).abs()
    return torch.minimum((d / o - thr).abs(), (d / ot - thr).abs())


def render(params: Dict[str, Tensor], c2w: Tensor, fx: float, fy: float, cx: float, cy: float, W: int, H: int, thr: float, sh_degree_to_use: int = 3,
           rasterize_mode: str = "classic", background: Optional[Tensor] = None, background_thermal: float = 0.0, flag_tol: float = 1e-4,
           with_depth: bool = False) -> Dict[str, Tensor]:
    """ssf.render plus the two removal walks.  Adds removal [H,W,3] and removal_thermal [H,W,1] (clamped), stopped_removal /
    stopped_removal_thermal [H,W] (the walk hit its stop), keep_rgb / keep_th [N]; flag_pixels also holds the removal walks' flags."""
    out = ssf.render(params, c2w, fx, fy, cx, cy, W, H, sh_degree_to_use=sh_degree_to_use, rasterize_mode=rasterize_mode, background=background,
                     background_thermal=background_thermal, flag_tol=flag_tol, with_depth=with_depth)
    with torch.no_grad():
        dt = params["means"].dtype
        pj = out["projection"]
        viewdirs = params["means"] - c2w[:3, 3].to(dt)
        viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
        col = torch.cat([params["features_dc"][:, None, :], params["features_rest"]], 1)
        col_t = torch.cat([params["features_dc_thermal"][:, None, :], params["features_rest_thermal"]], 1)
        if sh_degree_to_use >= 0 and col.shape[1] > 1:  # the colours as ssf.render computes them
            sh = torch.cat([so.spherical_harmonics(sh_degree_to_use, viewdirs, col), so.spherical_harmonics(sh_degree_to_use, viewdirs, col_t)], -1) + 0.5
            colors = torch.clamp(sh, min=0.0)
        else:
            colors = torch.sigmoid(torch.cat([col[:, 0], col_t[:, 0]], -1))
        keep_rgb, keep_th = keep_masks(params, thr)
        op, op_t = torch.sigmoid(params["opacities"])[:, 0], torch.sigmoid(params["opacities_thermal"])[:, 0]
        if rasterize_mode == "antialiased":
            op, op_t = op * pj["compensation"], op_t * pj["compensation"]
        zero = torch.zeros((), dtype=dt)
        bg4 = torch.cat([torch.zeros(3) if background is None else background, torch.tensor([background_thermal])]).to(dt)
        geom = (pj["xys"], pj["depths"], pj["radii"], pj["conics"], pj["tile_min"], pj["tile_max"])
        st: Dict[str, Tensor] = {}
        st_t: Dict[str, Tensor] = {}
        img, _, fp, _ = sf.rasterize(*geom, colors[:, :3], torch.where(keep_rgb, op, zero), H, W, bg4[:3], flag_tol=flag_tol, stats=st)
        img_t, _, fp_t, _ = sf.rasterize(*geom, colors[:, 3:], torch.where(keep_th, op_t, zero), H, W, bg4[3:], flag_tol=flag_tol, stats=st_t)
    out.update(removal=torch.clamp(img, max=1.0), removal_thermal=torch.clamp(img_t, max=1.0), stopped_removal=st["stopped"],
               stopped_removal_thermal=st_t["stopped"], keep_rgb=keep_rgb, keep_th=keep_th, flag_pixels=out["flag_pixels"] | fp | fp_t)
    return out


def subset(params: Dict[str, Tensor], keep: Tensor) -> Dict[str, Tensor]:
    return {k: v[keep].contiguous() for k, v in params.items()}


def removal_scene(num: int, seed: int, sh_degree: int, reverse: bool = False) -> Dict[str, Tensor]:
    """ssf.awkward_scene with opacities_thermal rewritten per Gaussian by a class drawn uniformly: 0 -- equal logits (kept in both renders);
    1 -- ot = RATIO o (out of `removal`, in `removal_thermal`); 2 -- ot = o / RATIO (the reverse); 3 -- the scene's own value where that is out
    of both with room to spare, else ot = 1.5 o, or o / 1.5 where 1.5 o would pass 0.99 (out of both).  Class 1 becomes class 2 where RATIO o
    would pass 0.99 (the opaque stack).  reverse: the two opacities then swap roles (and classes 1 and 2 with them).  Every Gaussian is at
    least 1e-3 from both thresholds at THR, ten times BAND."""
    p = ssf.awkward_scene(num, seed % 100, sh_degree, reverse=False)  # (seed // 100 varies the class draw alone)
    g = torch.Generator().manual_seed(2000 + seed)
    n = p["means"].shape[0]
    cls = torch.randint(0, 4, (n,), generator=g)
    stack = n - 240  # awkward_scene's opaque stack (30) and its Gaussians below 1/255 in one spectrum (10): class 3 with their own values, as the
    cls[stack:stack + 40] = 3  # separate-mode tests have them -- but for STACK_KEPT of the stack, which both renders keep: every walk that
    cls[stack:stack + STACK_KEPT] = 0  # stops on the stack flags pixels near its 1e-4 stop, and the tests allow 1 % over four walks
    o = torch.sigmoid(p["opacities"].double())[:, 0]
    own = torch.sigmoid(p["opacities_thermal"].double())[:, 0]
    d = (o - own).abs()
    own_ok = (d > 1.2 * THR * o) & (d > 1.2 * THR * own)
    cls = torch.where((cls == 1) & (RATIO * o > 0.99), torch.full_like(cls, 2), cls)
    far = torch.where(own_ok, own, torch.where(1.5 * o < 0.99, 1.5 * o, o / 1.5))
    ot = torch.where(cls == 1, RATIO * o, torch.where(cls == 2, o / RATIO, far))
    logit = torch.where(cls == 0, p["opacities"][:, 0].double(), torch.logit(ot))
    p["opacities_thermal"] = logit.float()[:, None].contiguous()
    if reverse:
        p["opacities"], p["opacities_thermal"] = p["opacities_thermal"], p["opacities"]
    return p
