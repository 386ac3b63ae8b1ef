"""Functional torch restatement of splatfacto's refinement (SplatfactoModel.after_train / refinement_after, nerfstudio/models/splatfacto.py:
346-498), written from its rules: the reference the HIP refinement (tn_splat_grad_stats, tn_splat_refine_plan / tn_splat_refine_apply) is
tested against, on the same device tensors, as splat_functional.py is for the render.

Parameters are a dict name -> tensor with rows = Gaussians, keyed by the model's gauss_params names ("means", "scales" (log), "quats",
"opacities", the SH coefficients ...); moments a dict name -> (exp_avg, exp_avg_sq) for the names that have Adam state.  Every function
returns new tensors and leaves its inputs alone."""
from typing import Callable, Dict, Optional, Tuple

import torch
from torch import Tensor

Stats = Optional[Tuple[Tensor, Tensor, Tensor]]  # (grad_norm_sum, vis_counts, max_2d_size), None = reset


def quat_to_rotmat(q: Tensor) -> Tensor:
    """[..., 4] quaternions (w, x, y, z) -> [..., 3, 3] rotation matrices of the normalised quaternions."""
    w, x, y, z = torch.unbind(q / q.norm(dim=-1, keepdim=True), dim=-1)
    m = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1)
    return m.reshape(q.shape[:-1] + (3, 3))


def after_train(stats: Stats, xys_grad: Tensor, radii: Tensor, size: Tuple[int, int], step: int, cfg) -> Stats:
    """One training frame's statistics: |xys_grad| summed and counted over the frames a Gaussian was visible in (radii > 0), and the
    largest radius seen as a fraction of max(H, W).  The first call after a reset takes every Gaussian, visible or not."""
    if step >= cfg.stop_split_at:
        return stats
    g = xys_grad.norm(dim=-1)
    vis = (radii > 0).flatten()
    if stats is None:
        gsum, cnt, m2d = g.clone(), torch.ones_like(g), torch.zeros(radii.shape, dtype=torch.float32, device=g.device)
    else:
        gsum, cnt, m2d = (t.clone() for t in stats)
        cnt[vis] = cnt[vis] + 1
        gsum[vis] = g[vis] + gsum[vis]
    m2d[vis] = torch.maximum(m2d[vis], radii[vis] / float(max(size[0], size[1])))
    return gsum, cnt, m2d


def _max_scale(scales: Tensor) -> Tensor:
    return torch.exp(scales).max(dim=-1).values


def _cull_mask(p: Dict[str, Tensor], m2d: Optional[Tensor], extra: Optional[Tensor], step: int, cfg) -> Tensor:
    culls = (torch.sigmoid(p["opacities"]) < cfg.cull_alpha_thresh).reshape(-1)
    if extra is not None:
        culls = culls | extra
    if step > cfg.refine_every * cfg.reset_alpha_every:
        big = _max_scale(p["scales"]) > cfg.cull_scale_thresh
        if step < cfg.stop_screen_size_at:
            big = big | (m2d > cfg.cull_screen_size)
        culls = culls | big
    return culls


def refine(params: Dict[str, Tensor], moments: Dict[str, Tuple[Tensor, Tensor]], stats: Stats, size: Tuple[int, int], step: int, cfg,
           num_train_data: int, noise: Callable[[int], Tensor]):
    """One refinement_after.  noise(n) returns the [n, 3] standard-normal draw of the split (n = n_split_samples * number of splits,
    sample-major).  Returns (params, moments, info); info holds the masks and counts (None when nothing ran)."""
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
        split = _max_scale(p["scales"]) > cfg.densify_size_thresh
        if step < cfg.stop_screen_size_at:
            split = split | (m2d > cfg.split_screen_size)
        split = split & high
        S, ns = cfg.n_split_samples, int(split.sum())
        z = noise(S * ns)
        # children: the parent's original log-scale places them; every other tensor is copied (the quaternion unnormalised)
        sc = p["scales"][split]
        rots = quat_to_rotmat(p["quats"][split].repeat(S, 1))
        offs = torch.bmm(rots, (torch.exp(sc.repeat(S, 1)) * z)[..., None])[..., 0]
        shrunk = torch.log(torch.exp(sc) / 1.6)
        child = {k: v[split].repeat(S, *([1] * (v.dim() - 1))) for k, v in p.items()}
        child["means"] = offs + p["means"][split].repeat(S, 1)
        child["scales"] = shrunk.repeat(S, 1)
        p["scales"][split] = shrunk
        # duplicates: decided on the updated scales, copy the updated values
        dup = (_max_scale(p["scales"]) <= cfg.densify_size_thresh) & high
        dups = {k: v[dup] for k, v in p.items()}
        nd = int(dup.sum())
        p = {k: torch.cat([p[k], child[k], dups[k]]) for k in p}
        m = {k: (torch.cat([a, torch.zeros_like(child[k]), torch.zeros_like(dups[k])]), torch.cat([b, torch.zeros_like(child[k]), torch.zeros_like(dups[k])]))
             for k, (a, b) in m.items()}
        new = S * ns + nd
        m2d_all = torch.cat([m2d, torch.zeros(new, device=m2d.device)])
        cull = _cull_mask(p, m2d_all, torch.cat([split, torch.zeros(new, dtype=torch.bool, device=split.device)]), step, cfg)
        info.update(split=split, dup=dup, num_split=ns, num_dup=nd)
    elif step >= cfg.stop_split_at and cfg.continue_cull_post_densification:
        cull = _cull_mask(p, stats[2] if stats is not None else None, None, step, cfg)
    if cull is not None:
        keep = ~cull
        p = {k: v[keep] for k, v in p.items()}
        m = {k: (a[keep], b[keep]) for k, (a, b) in m.items()}
        info["culled"] = cull
    if step < cfg.stop_split_at and step % R == cfg.refine_every:
        reset = torch.logit(torch.tensor(cfg.cull_alpha_thresh * 2.0, device=p["opacities"].device)).item()
        p["opacities"] = torch.clamp(p["opacities"], max=reset)
        if "opacities" in m:
            m["opacities"] = (torch.zeros_like(m["opacities"][0]), torch.zeros_like(m["opacities"][1]))
        info["reset"] = True
    return p, m, info
