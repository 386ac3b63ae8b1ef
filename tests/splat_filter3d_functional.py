"""Mip-Splatting's 3D smoothing filter restated in float64 torch (csrc/tn_splat_filter3d.hip computes the same expressions in the same order, in
double, and rounds once): the filter value per Gaussian from a camera table, its application to log-scales and opacity logits, and the closed-form
backward with the sum of its absolute terms (the yardstick of the backward tolerance).  Host only; inputs are float32 values widened."""
import torch

F64 = torch.float64
MARGIN = 0.15  # beyond each image side, as a share of the side, a Gaussian still counts as seen


def _camera_space(means: torch.Tensor, table: torch.Tensor):
    """(x, y, z) [N,C] of every Gaussian in every camera, each ((m0 px + m1 py) + m2 pz) + m3, and the table's columns [1,C]"""
    p, t = means.to(F64), table.to(F64)
    px, py, pz = (p[:, i:i + 1] for i in range(3))
    m = [t[:, j].unsqueeze(0) for j in range(18)]
    row = lambda r: ((m[4 * r] * px + m[4 * r + 1] * py) + m[4 * r + 2] * pz) + m[4 * r + 3]  # noqa: E731
    return row(0), row(1), row(2), m


def visibility(means: torch.Tensor, table: torch.Tensor, near: float):
    """(seen [N,C] bool, in_frame [N,C] bool: seen without the margin, nu [N,C]: max(fx, fy) / z where seen, else 0)"""
    x, y, z, m = _camera_space(means, table)
    fx, fy, cx, cy, W, H = m[12:18]
    front = z > near
    zs = torch.where(front, z, torch.ones_like(z))
    u, v = fx * x / zs + cx, fy * y / zs + cy
    seen = front & (u >= -MARGIN * W) & (u <= (1.0 + MARGIN) * W) & (v >= -MARGIN * H) & (v <= (1.0 + MARGIN) * H)
    in_frame = front & (u >= 0) & (u <= W) & (v >= 0) & (v <= H)
    nu = torch.where(seen, torch.maximum(fx, fy) / zs, torch.zeros_like(z))
    return seen, in_frame, nu


def compute_filter(means: torch.Tensor, table: torch.Tensor, near: float, variance: float) -> torch.Tensor:
    """filter_3D [N] float64: sqrt(variance) / nu_k; unseen Gaussians take the smallest nu of the seen ones; nothing seen (or no camera): zeros"""
    N = means.shape[0]
    if table.shape[0] == 0:
        return torch.zeros(N, dtype=F64)
    _, _, nu = visibility(means, table, near)
    nu = nu.max(dim=1).values
    seen = nu > 0
    if not bool(seen.any()):
        return torch.zeros(N, dtype=F64)
    sv = torch.tensor(float(variance), dtype=F64).sqrt()
    nu = torch.where(seen, nu, nu[seen].min())
    return sv / nu


def boundary_distance(means: torch.Tensor, table: torch.Tensor, near: float) -> torch.Tensor:
    """[N]: each Gaussian's smallest relative distance to a visibility boundary over all cameras -- |z - near| / near for the near plane and, in
    front of it, |u - edge| / W and |v - edge| / H for the four margins (edges at -0.15 and 1.15 of the side)"""
    x, y, z, m = _camera_space(means, table)
    fx, fy, cx, cy, W, H = m[12:18]
    d = (z - near).abs() / near
    front = z > near
    zs = torch.where(front, z, torch.ones_like(z))
    u, v = fx * x / zs + cx, fy * y / zs + cy
    big = torch.full_like(z, float("inf"))
    for val, side in ((u, W), (v, H)):
        for edge in (-MARGIN, 1.0 + MARGIN):
            d = torch.minimum(d, torch.where(front, (val - edge * side).abs() / side, big))
    return d.min(dim=1).values


def _row(scales: torch.Tensor, f: torch.Tensor):
    s2 = torch.exp(2.0 * scales.to(F64))
    f2 = (f.to(F64) * f.to(F64)).unsqueeze(-1)
    d = s2 + f2
    r, q = s2 / d, f2 / d
    lg = torch.log1p(f2 / s2)  # -log r_i
    log_c = -0.5 * ((lg[:, 0] + lg[:, 1]) + lg[:, 2])
    return d, r, q, (log_c, -torch.expm1(log_c))  # log c and 1 - c of c = sqrt(r_0 r_1 r_2)


def _logit(o: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    od = o.to(F64).reshape(-1)
    return ((od + c[0]) - torch.log1p(torch.exp(od) * c[1])).reshape(o.shape)


def apply_forward(scales, opacities, f, opacities_thermal=None):
    """(scales', opacities'[, opacities_thermal']) float64; rows with f == 0 are the inputs themselves"""
    d, _, _, c = _row(scales, f)
    on = (f != 0)
    out = [torch.where(on.unsqueeze(-1), 0.5 * torch.log(d), scales.to(F64))]
    for o in (opacities, opacities_thermal):
        if o is not None:
            out.append(torch.where(on.reshape(o.shape[0], *([1] * (o.dim() - 1))), _logit(o, c), o.to(F64)))
    return tuple(out)


def _complements(o, c):
    od = o.to(F64).reshape(-1)
    omp = 1.0 / (1.0 + torch.exp(od))
    p = 1.0 / (1.0 + torch.exp(-od))
    return omp, omp + p * c[1]


def apply_backward(scales, opacities, f, g_scales, g_opacities, opacities_thermal=None, g_opacities_thermal=None):
    """The closed form: ((g_scales, g_opacities[, g_opacities_thermal]) float64, (the same tuple's sums of absolute terms)).  Rows with f == 0
    pass the upstream gradients through."""
    _, r, q, c = _row(scales, f)
    on = (f != 0)
    gs, go = g_scales.to(F64), g_opacities.to(F64).reshape(-1)
    omp, ompp = _complements(opacities, c)
    A, A_abs = go / ompp, (go / ompp).abs()
    out_o = [go * omp / ompp]
    if opacities_thermal is not None:
        gth = g_opacities_thermal.to(F64).reshape(-1)
        omp_t, ompp_t = _complements(opacities_thermal, c)
        A, A_abs = A + gth / ompp_t, A_abs + (gth / ompp_t).abs()
        out_o.append(gth * omp_t / ompp_t)
    g_ls = gs * r + A.unsqueeze(-1) * q
    g_ls_abs = (gs * r).abs() + A_abs.unsqueeze(-1) * q
    g_ls = torch.where(on.unsqueeze(-1), g_ls, gs)
    g_ls_abs = torch.where(on.unsqueeze(-1), g_ls_abs, gs.abs())
    ups = [go] + ([g_opacities_thermal.to(F64).reshape(-1)] if opacities_thermal is not None else [])
    outs = [torch.where(on, v, u) for v, u in zip(out_o, ups)]
    shapes = [opacities.shape] + ([opacities_thermal.shape] if opacities_thermal is not None else [])
    grads = (g_ls,) + tuple(v.reshape(s) for v, s in zip(outs, shapes))
    abs_terms = (g_ls_abs,) + tuple(v.abs().reshape(s) for v, s in zip(outs, shapes))
    return grads, abs_terms
