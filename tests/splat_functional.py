"""A functional (no in-place update) restatement of oracle/splat_oracle.render, so that torch autograd can differentiate it: the reference for
the splat backward tests.  Same arithmetic and order of operations as the oracle (equal to it in float32); any dtype.  Besides the images it
reports where a float32 / float64 disagreement could flip one of the forward's discrete decisions (alpha near 1/255 or 0.999, a transmittance
near the 1e-4 stop, a colour near the output clamp, an SH value near its clamp, a view-space position on the frustum clamp), so that tests can
keep those few pixels and Gaussians out of a gradient comparison."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
from torch import Tensor

import splat_oracle as so

PARAM_NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest", "features_dc_thermal", "features_rest_thermal")


def project(means: Tensor, scales: Tensor, quats: Tensor, viewmat: Tensor, projmat: Tensor, fx: float, fy: float, cx: float, cy: float, H: int, W: int,
            clip_thresh: float = so.CLIP_THRESH, flag_tol: float = 1e-4) -> Dict[str, Tensor]:
    """so.project_gaussians without the in-place construction of J; scales exponentiated, quats normalised by the caller."""
    N, dt = means.shape[0], means.dtype
    Rv, tv = viewmat[:3, :3], viewmat[:3, 3]
    p_view = means @ Rv.T + tv
    visible = p_view[:, 2] > clip_thresh
    M = so.quat_to_rotmat(quats) * scales[:, None, :]
    cov3d = M @ M.transpose(1, 2)
    tan_fovx, tan_fovy = 0.5 * W / fx, 0.5 * H / fy
    lim_x, lim_y = 1.3 * tan_fovx, 1.3 * tan_fovy
    tz = p_view[:, 2]
    ux, uy = p_view[:, 0] / tz, p_view[:, 1] / tz
    tx = tz * torch.clamp(ux, -lim_x, lim_x)
    ty = tz * torch.clamp(uy, -lim_y, lim_y)
    rz = 1.0 / tz
    rz2 = rz * rz
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx * rz, zero, -fx * tx * rz2], -1), torch.stack([zero, fy * rz, -fy * ty * rz2], -1)], 1)
    Tm = J @ Rv
    cov = Tm @ cov3d @ Tm.transpose(1, 2)
    a0, b0, c0 = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    det_orig = a0 * c0 - b0 * b0
    a, b, c = a0 + 0.3, b0, c0 + 0.3
    det = a * c - b * b
    comp = torch.sqrt(torch.clamp(det_orig / det, min=0.0))
    ok = visible & (det != 0)
    inv_det = 1.0 / det
    conics = torch.stack([c * inv_det, -b * inv_det, a * inv_det], -1)
    mid = 0.5 * (a + c)
    disc = torch.sqrt(torch.clamp(mid * mid - det, min=0.1))
    radius = torch.ceil(3.0 * torch.sqrt(torch.maximum(mid + disc, mid - disc)))
    ph = torch.cat([means, torch.ones(N, 1, dtype=dt)], -1) @ projmat.T
    rw = 1.0 / (ph[:, 3] + 1e-6)
    xys = torch.stack([0.5 * W * (ph[:, 0] * rw) + cx - 0.5, 0.5 * H * (ph[:, 1] * rw) + cy - 0.5], -1)
    bw = so.BLOCK_WIDTH
    tb_x, tb_y = (W + bw - 1) // bw, (H + bw - 1) // bw
    tcx, tcy, tr = xys[:, 0].detach() / bw, xys[:, 1].detach() / bw, radius.detach() / bw
    clampi = lambda v, hi: torch.clamp(v.to(torch.int32), 0, hi)  # noqa: E731
    safe = lambda v: torch.where(ok, v, torch.zeros_like(v))  # noqa: E731
    x0, x1 = clampi(safe(tcx - tr), tb_x), clampi(safe(tcx + tr + 1), tb_x)
    y0, y1 = clampi(safe(tcy - tr), tb_y), clampi(safe(tcy + tr + 1), tb_y)
    ok = ok & ((x1 - x0) * (y1 - y0) > 0)
    near_clamp = ok & (((ux.abs() / lim_x - 1).abs() < flag_tol) | ((uy.abs() / lim_y - 1).abs() < flag_tol))
    return {"xys": xys, "depths": tz, "radii": torch.where(ok, radius, torch.zeros_like(radius)).to(torch.int32), "conics": conics, "compensation": comp,
            "tile_min": torch.stack([x0, y0], -1), "tile_max": torch.stack([x1, y1], -1), "ok": ok, "near_clamp": near_clamp.detach()}


def rasterize(xys: Tensor, depths: Tensor, radii: Tensor, conics: Tensor, tile_min: Tensor, tile_max: Tensor, colors: Tensor, opacity: Tensor, H: int, W: int,
              background: Tensor, flag_tol: float = 1e-4, clamp_channels: Optional[int] = None, stats: Optional[Dict[str, Tensor]] = None):
    """so.rasterize_gaussians with out-of-place updates (every Gaussian is evaluated over the whole image and masked to its tile box).
    Returns the image before the clamp [H,W,C], 1 - T [H,W], the flagged pixels [H,W] and the Gaussians with a flagged pair [N].
    clamp_channels: only the first so many channels meet the output clamp (default: all); a depth channel behind them does not.
    stats: a dict that receives `pair_used` [N, tiles_y, tiles_x] (the Gaussian passed every test at a pixel of the tile that was still
    running -- the pixel it stops included: what a tile's list must hold) and `stopped` [H,W] (the pixel hit the T <= 1e-4 stop)."""
    dt, N = colors.dtype, colors.shape[0]
    bw = so.BLOCK_WIDTH
    tby, tbx = (H + bw - 1) // bw, (W + bw - 1) // bw
    pair_used = torch.zeros(N, tby, tbx, dtype=torch.bool) if stats is not None else None
    order = torch.argsort(depths.detach(), stable=True)
    order = order[radii[order] > 0]
    py, px = torch.meshgrid(torch.arange(H, dtype=dt) + 0.5, torch.arange(W, dtype=dt) + 0.5, indexing="ij")
    iy, ix = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    T = torch.ones(H, W, dtype=dt)
    done = torch.zeros(H, W, dtype=torch.bool)
    out = torch.zeros(H, W, colors.shape[1], dtype=dt)
    flag_pix = torch.zeros(H, W, dtype=torch.bool)
    flag_g = torch.zeros(N, dtype=torch.bool)
    for g in order.tolist():
        x0, y0 = (tile_min[g] * bw).tolist()
        x1, y1 = (tile_max[g] * bw).tolist()
        inbox = (ix >= x0) & (ix < x1) & (iy >= y0) & (iy < y1)
        dx = xys[g, 0] - px
        dy = xys[g, 1] - py
        sigma = 0.5 * (conics[g, 0] * dx * dx + conics[g, 2] * dy * dy) + conics[g, 1] * dx * dy
        raw = opacity[g] * torch.exp(-sigma)
        alpha = torch.clamp(raw, max=0.999)
        use = inbox & (sigma >= 0) & (alpha >= 1.0 / 255.0) & ~done
        next_T = T * (1.0 - alpha)
        stop = use & (next_T <= 1e-4)
        with torch.no_grad():
            if pair_used is not None:
                pair_used[g] = torch.nn.functional.pad(use, (0, tbx * bw - W, 0, tby * bw - H)).view(tby, bw, tbx, bw).any(3).any(1)
            live = inbox & ~done
            f = live & (((alpha * 255.0 - 1).abs() < flag_tol) | ((raw / 0.999 - 1).abs() < flag_tol) | (use & ((next_T * 1e4 - 1).abs() < 1e2 * flag_tol)))
            flag_pix |= f
            if bool(f.any()):
                flag_g[g] = True
        done = done | stop
        use = use & ~stop
        vis = alpha * T
        out = out + torch.where(use[..., None], vis[..., None] * colors[g], torch.zeros((), dtype=dt))
        T = torch.where(use, next_T, T)
    img = out + T[..., None] * background
    with torch.no_grad():
        flag_pix |= ((img[..., :clamp_channels] - 1).abs() < flag_tol).any(-1)
        if stats is not None:
            stats["pair_used"], stats["stopped"] = pair_used, done
    return img, 1.0 - T, flag_pix, flag_g


def render(params: Dict[str, Tensor], c2w: Tensor, fx: float, fy: float, cx: float, cy: float, W: int, H: int, sh_degree_to_use: int = 3,
           rasterize_mode: str = "classic", background: Optional[Tensor] = None, background_thermal: float = 0.0, flag_tol: float = 1e-4,
           viewdir_means: Optional[Tensor] = None, with_depth: bool = False) -> Dict[str, Tensor]:
    """so.render (rgb, thermal, accumulation) as a differentiable function of `params`, in the dtype of params["means"].
    `raw` is the RGB+T image before the output clamp.  viewdir_means: the means the SH view directions are taken from (default: the means
    themselves, detached); finite differences pass the unperturbed ones, since the view directions carry no gradient.
    with_depth (the forward tests; no gradient): also `depth` [H,W,1] as tn_splat_raster documents it -- sum(alpha T depth) / accumulation
    where accumulation > 0, else `depth_fill`, the maximum of the un-normalised image `depth_raw` -- and the walk's statistics:
    `contributors_per_tile` [tiles_y, tiles_x], `pair_used` [N, tiles_y, tiles_x], `stopped` [H,W], `stopped_fraction`.  "classic": the depth
    rides the colour walk as a fifth channel (same decisions, the colour arithmetic untouched); "antialiased": as in so.render a SECOND
    front-to-back walk with the uncompensated opacity, its own transmittance and stop, whose near-threshold decisions are flagged too and
    whose used pairs count as contributors (the GPU's one list serves both walks); `stopped` is the colour walk's."""
    dt = params["means"].dtype
    background = torch.zeros(3) if background is None else background
    viewmat, projmat = so.camera_matrices(c2w, fx, fy, W, H)
    viewmat, projmat = viewmat.to(dt), projmat.to(dt)
    means = params["means"]
    quats = params["quats"] / params["quats"].norm(dim=-1, keepdim=True)
    pj = project(means, torch.exp(params["scales"]), quats, viewmat, projmat, fx, fy, cx, cy, H, W, flag_tol=flag_tol)
    viewdirs = (means if viewdir_means is None else viewdir_means).detach() - c2w[:3, 3].to(dt)  # splatfacto.py:770: the view directions carry no gradient
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
    if rasterize_mode == "antialiased":
        op = op * pj["compensation"]
    elif rasterize_mode != "classic":
        raise ValueError(f"Unknown rasterize_mode: {rasterize_mode}")
    bg4 = torch.cat([background, torch.tensor([background_thermal])]).to(dt)
    geom = (pj["xys"], pj["depths"], pj["radii"], pj["conics"], pj["tile_min"], pj["tile_max"])
    if not with_depth:
        img, alpha, flag_pix, flag_g = rasterize(*geom, colors, op, H, W, bg4, flag_tol=flag_tol)
        return {"rgb": torch.clamp(img[..., :3], max=1.0), "thermal": torch.clamp(img[..., 3:], max=1.0), "accumulation": alpha[..., None], "raw": img,
                "xys": pj["xys"], "projection": pj, "flag_pixels": flag_pix, "flag_gaussians": flag_g | (pj["near_clamp"] & pj["ok"]) | (near_sh & pj["ok"])}
    with torch.no_grad():
        st: Dict[str, Tensor] = {}
        zero1 = torch.zeros(1, dtype=dt)
        if rasterize_mode == "classic":
            img5, alpha, flag_pix, flag_g = rasterize(*geom, torch.cat([colors, pj["depths"][:, None]], -1), op, H, W, torch.cat([bg4, zero1]),
                                                      flag_tol=flag_tol, clamp_channels=4, stats=st)
            img, depth_raw, pair_used = img5[..., :4], img5[..., 4:], st["pair_used"]
        else:
            img, alpha, flag_pix, flag_g = rasterize(*geom, colors, op, H, W, bg4, flag_tol=flag_tol, stats=st)
            st_d: Dict[str, Tensor] = {}
            depth_raw, _, fp_d, fg_d = rasterize(*geom, pj["depths"][:, None], op_plain, H, W, zero1, flag_tol=flag_tol, clamp_channels=0, stats=st_d)
            flag_pix, flag_g, pair_used = flag_pix | fp_d, flag_g | fg_d, st["pair_used"] | st_d["pair_used"]
        alpha = alpha[..., None]
        fill = depth_raw.max()
        depth = torch.where(alpha > 0, depth_raw / alpha, fill)  # splatfacto.py:809
    return {"rgb": torch.clamp(img[..., :3], max=1.0), "thermal": torch.clamp(img[..., 3:], max=1.0), "accumulation": alpha, "raw": img, "depth": depth,
            "depth_raw": depth_raw, "depth_fill": fill, "xys": pj["xys"], "projection": pj, "flag_pixels": flag_pix,
            "flag_gaussians": flag_g | (pj["near_clamp"] & pj["ok"]) | (near_sh & pj["ok"]), "pair_used": pair_used,
            "contributors_per_tile": pair_used.sum(0), "stopped": st["stopped"], "stopped_fraction": float(st["stopped"].float().mean())}


def scene(num: int, seed: int, sh_degree: int, extent: float = 1.0, scale_range=(-3.6, -2.2)) -> Dict[str, Tensor]:
    """synth_gaussians with the higher-order coefficients cut to `sh_degree` (config.sh_degree; 0 = none, the sigmoid colours)."""
    p = so.synth_gaussians(num, seed=seed, extent=extent, scale_range=scale_range)
    k = (sh_degree + 1) ** 2 - 1
    p["features_rest"], p["features_rest_thermal"] = p["features_rest"][:, :k].contiguous(), p["features_rest_thermal"][:, :k].contiguous()
    return p


def separate_depths(means: Tensor, c2w: Tensor, min_gap: float = 2.5e-5, fixed: Optional[Tensor] = None) -> Tensor:
    """`means` (float32) moved along the camera's optical axis until every float64 view-space depth exceeds its predecessor's, in sorted
    order, by at least `min_gap`: about a hundred float32 ulps of a depth near 2, so that float32 and float64 composite in the same order.
    fixed [N] bool: Gaussians that stay where they are (bit-equal means: tied depths); the others also keep `min_gap` from those.  The
    rounding of the moved means to float32 costs a few 1e-7 of depth, which is why tests ask the result for 2e-5 only."""
    viewmat, _ = so.camera_matrices(c2w, 1.0, 1.0, 2, 2)
    Rv, tv = viewmat[:3, :3].double(), viewmat[:3, 3].double()
    m = means.double()
    d = (m @ Rv.T + tv)[:, 2]
    fixed = torch.zeros(d.shape[0], dtype=torch.bool) if fixed is None else fixed
    walls = sorted(d[fixed].tolist())
    new, prev = d.clone(), -math.inf
    for i in torch.argsort(d, stable=True).tolist():
        if bool(fixed[i]):
            prev = max(prev, float(d[i]))
            continue
        t = max(float(d[i]), prev + min_gap)
        for f in walls:  # ascending, and t only grows: one pass
            if abs(t - f) < min_gap:
                t = f + min_gap
        new[i] = prev = t
    return (m + (new - d)[:, None] * Rv[2]).float()


def fov_focal(W: int, fov_deg: float = 60.0) -> float:
    return 0.5 * W / math.tan(math.radians(0.5 * fov_deg))
