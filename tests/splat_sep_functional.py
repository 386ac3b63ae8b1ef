"""Functional torch restatement of the splat render and refinement with a separate thermal opacity (thermal_opacity_mode "separate"), built on
splat_functional.py (projection, one front-to-back walk) and splat_refine_functional.py: the reference of the separate-mode tests, any dtype,
differentiable by autograd.

Render: ONE depth-sorted list, TWO walks over it.  RGB (and accumulation, and in classic mode the depth) composite with sigmoid(opacities); the
thermal channel composites with sigmoid(opacities_thermal) through its own transmittance, with its own stop (a pixel's walk stops before the
Gaussian that would take T to 1e-4 or below) and its own background weight; "antialiased" multiplies both opacities by the same compensation
and, as in shared mode, walks the depth a third time with the plain opacity.  With opacities_thermal == opacities every walk takes the shared
walk's decisions and does its arithmetic, so the images equal splat_functional.render's exactly.

Refinement: splat_refine_functional.refine with two changes -- a Gaussian is culled for low opacity only when BOTH sigmoids are below
cull_alpha_thresh, and the opacity reset clamps both logit tensors and zeroes both groups' moments.  opacities_thermal is one more row-wise
parameter: split children and duplicates copy it like every other tensor."""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import torch
from torch import Tensor

import splat_functional as sf
import splat_oracle as so
import splat_refine_functional as rf

PARAM_NAMES = sf.PARAM_NAMES + ("opacities_thermal",)
# The GPU tests' frames: (W, H, raster mode, config.sh_degree, roles of the two opacities reversed, seed of awkward_scene).  Sizes that are no
# multiple of 16 (nor of the 8 x 8 quadrants); seeds for which the float32 AND the float64 restatement flag at most 1 % of the pixels as
# near-threshold (test_splat_separate_cpu.py asserts it, with the other properties awkward_scene promises).
CASES = [(40, 24, "classic", 0, False, 6), (33, 17, "antialiased", 3, True, 1), (33, 17, "classic", 3, False, 10)]


def render(params: Dict[str, Tensor], c2w: Tensor, fx: float, fy: float, cx: float, cy: float, W: int, H: int, sh_degree_to_use: int = 3,
           rasterize_mode: str = "classic", background: Optional[Tensor] = None, background_thermal: float = 0.0, flag_tol: float = 1e-4,
           with_depth: bool = False) -> Dict[str, Tensor]:
    """sf.render in separate mode.  Returns rgb, thermal (clamped), accumulation, accumulation_thermal [H,W,1], raw [H,W,4] (before the clamp),
    xys, projection, flag_pixels / flag_gaussians (the union over the walks: where float32 may legitimately decide a 1/255 gate, a 0.999 clamp, a
    1e-4 stop or an output clamp the other way), stopped / stopped_thermal [H,W] (the walk hit its stop) and pair_used [N, tiles_y, tiles_x] (the
    union: what a tile's list must hold); with_depth (no gradient) also depth [H,W,1] as the shared functional defines it."""
    dt = params["means"].dtype
    background = torch.zeros(3) if background is None else background
    viewmat, projmat = so.camera_matrices(c2w, fx, fy, W, H)
    viewmat, projmat = viewmat.to(dt), projmat.to(dt)
    means = params["means"]
    quats = params["quats"] / params["quats"].norm(dim=-1, keepdim=True)
    pj = sf.project(means, torch.exp(params["scales"]), quats, viewmat, projmat, fx, fy, cx, cy, H, W, flag_tol=flag_tol)
    viewdirs = means.detach() - c2w[:3, 3].to(dt)
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    col = torch.cat([params["features_dc"][:, None, :], params["features_rest"]], 1)
    col_t = torch.cat([params["features_dc_thermal"][:, None, :], params["features_rest_thermal"]], 1)
    near_sh = torch.zeros(means.shape[0], dtype=torch.bool)
    if sh_degree_to_use >= 0 and col.shape[1] > 1:
        sh = torch.cat([so.spherical_harmonics(sh_degree_to_use, viewdirs, col), so.spherical_harmonics(sh_degree_to_use, viewdirs, col_t)], -1) + 0.5
        near_sh = (sh.detach().abs() < flag_tol).any(-1)
        colors = torch.clamp(sh, min=0.0)
    else:
        colors = torch.sigmoid(torch.cat([col[:, 0], col_t[:, 0]], -1))
    op_plain = op = torch.sigmoid(params["opacities"])[:, 0]
    op_t = torch.sigmoid(params["opacities_thermal"])[:, 0]
    if rasterize_mode == "antialiased":
        op, op_t = op * pj["compensation"], op_t * pj["compensation"]
    elif rasterize_mode != "classic":
        raise ValueError(f"Unknown rasterize_mode: {rasterize_mode}")
    bg4 = torch.cat([background, torch.tensor([background_thermal])]).to(dt)  # (as sf.render builds it: float32 values in either dtype)
    bg, bg_t = bg4[:3], bg4[3:]
    geom = (pj["xys"], pj["depths"], pj["radii"], pj["conics"], pj["tile_min"], pj["tile_max"])
    st: Dict[str, Tensor] = {}
    st_t: Dict[str, Tensor] = {}
    depth_cols = with_depth and rasterize_mode == "classic"
    c_rgb = torch.cat([colors[:, :3], pj["depths"][:, None].detach()], -1) if depth_cols else colors[:, :3]
    img, alpha, flag_pix, flag_g = sf.rasterize(*geom, c_rgb, op, H, W, torch.cat([bg, torch.zeros(1, dtype=dt)]) if depth_cols else bg, flag_tol=flag_tol,
                                                clamp_channels=3, stats=st)
    img_t, alpha_t, fp_t, fg_t = sf.rasterize(*geom, colors[:, 3:], op_t, H, W, bg_t, flag_tol=flag_tol, stats=st_t)
    flag_pix, flag_g, pair_used = flag_pix | fp_t, flag_g | fg_t, st["pair_used"] | st_t["pair_used"]
    raw = torch.cat([img[..., :3], img_t], -1)
    out = {"rgb": torch.clamp(raw[..., :3], max=1.0), "thermal": torch.clamp(raw[..., 3:], max=1.0), "accumulation": alpha[..., None],
           "accumulation_thermal": alpha_t[..., None], "raw": raw, "xys": pj["xys"], "projection": pj, "stopped": st["stopped"],
           "stopped_thermal": st_t["stopped"]}
    if with_depth:
        with torch.no_grad():
            if depth_cols:
                depth_raw = img[..., 3:]
            else:
                st_d: Dict[str, Tensor] = {}
                depth_raw, _, fp_d, fg_d = sf.rasterize(*geom, pj["depths"][:, None], op_plain, H, W, torch.zeros(1, dtype=dt), flag_tol=flag_tol,
                                                        clamp_channels=0, stats=st_d)
                flag_pix, flag_g, pair_used = flag_pix | fp_d, flag_g | fg_d, pair_used | st_d["pair_used"]
            a = alpha[..., None]
            out["depth"] = torch.where(a > 0, depth_raw / a, depth_raw.max())
    out["flag_pixels"] = flag_pix
    out["flag_gaussians"] = flag_g | (pj["near_clamp"] & pj["ok"]) | (near_sh & pj["ok"])
    out["pair_used"] = pair_used
    out["contributors_per_tile"] = pair_used.sum(0)
    return out


def shared_params(params: Dict[str, Tensor]) -> Dict[str, Tensor]:
    return {k: v for k, v in params.items() if k != "opacities_thermal"}


def density_loss(opacities: Tensor, opacities_thermal: Tensor, opacity_loss_mult: float, rgb_opacity_loss_mult: float) -> Tensor:
    """The NeRF model's density_loss on the two opacities (logits in): each term's gradient reaches only its own tensor."""
    o, o_t = torch.sigmoid(opacities), torch.sigmoid(opacities_thermal)
    return opacity_loss_mult * ((o_t - o.detach()).abs().mean() + rgb_opacity_loss_mult * (o - o_t.detach()).abs().mean())


def cull_mask(p: Dict[str, Tensor], m2d: Optional[Tensor], extra: Optional[Tensor], step: int, cfg) -> Tensor:
    """rf._cull_mask with the separate-mode opacity rule: transparent only when BOTH opacities are below the threshold."""
    culls = ((torch.sigmoid(p["opacities"]) < cfg.cull_alpha_thresh) & (torch.sigmoid(p["opacities_thermal"]) < cfg.cull_alpha_thresh)).reshape(-1)
    if extra is not None:
        culls = culls | extra
    if step > cfg.refine_every * cfg.reset_alpha_every:
        big = rf._max_scale(p["scales"]) > cfg.cull_scale_thresh
        if step < cfg.stop_screen_size_at:
            big = big | (m2d > cfg.cull_screen_size)
        culls = culls | big
    return culls


def refine(params: Dict[str, Tensor], moments: Dict[str, Tuple[Tensor, Tensor]], stats: rf.Stats, size: Tuple[int, int], step: int, cfg,
           num_train_data: int, noise: Callable[[int], Tensor]):
    """rf.refine for parameters that hold opacities_thermal: the same steps in the same order, with cull_mask above and both logit tensors reset."""
    if step <= cfg.warmup_length:
        return params, moments, None
    p = {k: v.clone() for k, v in params.items()}
    m = {k: (a.clone(), b.clone()) for k, (a, b) in moments.items()}
    R = cfg.reset_alpha_every * cfg.refine_every
    densify = step < cfg.stop_split_at and step % R > num_train_data + cfg.refine_every
    info = {"densify": densify, "culled": None}
    cull = None
    if densify:
        gsum, cnt, m2d = stats
        high = ((gsum / cnt) * 0.5 * max(size[0], size[1]) > cfg.densify_grad_thresh).reshape(-1)
        split = rf._max_scale(p["scales"]) > cfg.densify_size_thresh
        if step < cfg.stop_screen_size_at:
            split = split | (m2d > cfg.split_screen_size)
        split = split & high
        S, ns = cfg.n_split_samples, int(split.sum())
        z = noise(S * ns)
        sc = p["scales"][split]
        rots = rf.quat_to_rotmat(p["quats"][split].repeat(S, 1))
        offs = torch.bmm(rots, (torch.exp(sc.repeat(S, 1)) * z)[..., None])[..., 0]
        shrunk = torch.log(torch.exp(sc) / 1.6)
        child = {k: v[split].repeat(S, *([1] * (v.dim() - 1))) for k, v in p.items()}
        child["means"] = offs + p["means"][split].repeat(S, 1)
        child["scales"] = shrunk.repeat(S, 1)
        p["scales"][split] = shrunk
        dup = (rf._max_scale(p["scales"]) <= cfg.densify_size_thresh) & high
        dups = {k: v[dup] for k, v in p.items()}
        nd = int(dup.sum())
        p = {k: torch.cat([p[k], child[k], dups[k]]) for k in p}
        m = {k: (torch.cat([a, torch.zeros_like(child[k]), torch.zeros_like(dups[k])]), torch.cat([b, torch.zeros_like(child[k]), torch.zeros_like(dups[k])]))
             for k, (a, b) in m.items()}
        new = S * ns + nd
        m2d_all = torch.cat([m2d, torch.zeros(new, device=m2d.device)])
        cull = cull_mask(p, m2d_all, torch.cat([split, torch.zeros(new, dtype=torch.bool, device=split.device)]), step, cfg)
        info.update(split=split, dup=dup, num_split=ns, num_dup=nd)
    elif step >= cfg.stop_split_at and cfg.continue_cull_post_densification:
        cull = cull_mask(p, stats[2] if stats is not None else None, None, step, cfg)
    if cull is not None:
        keep = ~cull
        p = {k: v[keep] for k, v in p.items()}
        m = {k: (a[keep], b[keep]) for k, (a, b) in m.items()}
        info["culled"] = cull
    if step < cfg.stop_split_at and step % R == cfg.refine_every:
        reset = torch.logit(torch.tensor(cfg.cull_alpha_thresh * 2.0, device=p["opacities"].device)).item()
        for k in ("opacities", "opacities_thermal"):
            p[k] = torch.clamp(p[k], max=reset)
            if k in m:
                m[k] = (torch.zeros_like(m[k][0]), torch.zeros_like(m[k][1]))
        info["reset"] = True
    return p, m, info


def awkward_scene(num: int, seed: int, sh_degree: int, reverse: bool = False) -> Dict[str, Tensor]:
    """About `num` Gaussians for the separate-mode GPU tests.  A random cloud (sf.scene) with independent thermal opacities, plus, around the
    point the test cameras look at: a stack of large, nearly opaque Gaussians whose RGB opacity is ~0.99 and whose thermal opacity is ~0.02 (the
    RGB walk hits its 1e-4 stop while the thermal walk runs on), a few Gaussians with sigmoid(o_th) < 1/255 and sigmoid(o) ~ 0.99 (present in the
    tile lists only through the larger opacity), and enough small ones in one tile to push its list past 256 entries (two batches, a backward
    that starts mid-list).  reverse: the two opacities swap roles."""
    g = torch.Generator().manual_seed(1000 + seed)
    p = sf.scene(num - 240, seed, sh_degree)
    n0 = p["means"].shape[0]
    p["opacities_thermal"] = p["opacities"][torch.randperm(n0, generator=g)].clone() + 0.5 * torch.randn(n0, 1, generator=g)
    k = p["features_rest"].shape[1]

    def block(n, spread, log_scale, o, o_t):
        return {"means": spread * (torch.rand(n, 3, generator=g) - 0.5), "scales": log_scale + 0.2 * torch.rand(n, 3, generator=g),
                "quats": torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1), "opacities": torch.full((n, 1), o) + 0.1 * torch.rand(n, 1, generator=g),
                "opacities_thermal": torch.full((n, 1), o_t) + 0.1 * torch.rand(n, 1, generator=g), "features_dc": torch.rand(n, 3, generator=g),
                "features_rest": 0.1 * torch.randn(n, k, 3, generator=g), "features_dc_thermal": torch.rand(n, 1, generator=g),
                "features_rest_thermal": 0.1 * torch.randn(n, k, 1, generator=g)}

    hi, lo, gone = 4.6, -3.9, -6.5  # sigmoid: 0.990, 0.020, 0.0015 (< 1/255)
    blocks = [block(30, 0.5, -1.3, hi, lo), block(10, 0.6, -1.6, hi, gone), block(200, 0.15, -2.9, 0.0, 0.5)]
    for b in blocks:
        if reverse:
            b["opacities"], b["opacities_thermal"] = b["opacities_thermal"], b["opacities"]
        for key in p:
            p[key] = torch.cat([p[key], b[key]])
    return {key: v.contiguous() for key, v in p.items()}
