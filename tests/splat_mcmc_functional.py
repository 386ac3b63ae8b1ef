"""The MCMC densification strategy restated in float64 numpy: the specification tn_splat_mcmc_relocate / tn_splat_mcmc_noise and
ThermalSplatfactoModel's strategy "mcmc" are tested against ("3D Gaussian Splatting as Markov Chain Monte Carlo", gsplat's MCMCStrategy, with
this project's second opacity chain).

Notation: o = sigmoid(opacities), o_th = sigmoid(opacities_thermal) (separate mode), s = exp(scales), o_vis = o (shared) or max(o, o_th)
(separate), eps = float32 machine epsilon, n_max = 51.

Relocation value of a source with ratio r (an integer clamped to [1, n_max]): every opacity chain c becomes c' = 1 - (1 - c)^(1/r), clamped to
[min_opacity, 1 - eps], stored as log(c' / (1 - c')).  The scale follows the dominant chain p (shared: o; separate: the larger of o and o_th, a
tie going to o): p' = 1 - (1 - p)^(1/r) unclamped, denom = sum_{i=1..r} sum_{k=0..i-1} binom(i-1, k) (-1)^k p'^(k+1) / sqrt(k+1),
s' = (p / denom) s on all three axes, stored as log s'.

`relocate` applies M draws src[j] -> dst[j] to tensors of one row count: ratio = 1 + how often a source was drawn; every drawn source takes its
relocation value once, from its values before the call, and both its Adam moments become zero in every tensor; every destination row becomes a
copy of its source's row, in every tensor, with the new opacity and scale; destination moments and rows not named stay.

`noise`: means += Sigma (z g scaler), g = 1 / (1 + exp(-100 ((1 - o_vis) - 0.995))), Sigma = R diag(s^2) R^T, R the rotation of quats / |quats|
(w x y z, gsplat's quat_to_rotmat: the projection's and the split's convention).  `noise_torch` is the same formula in plain torch at the dtype of
its inputs: the float32 yardstick of the kernel's tolerance.
"""
import math

import numpy as np

N_MAX = 51
EPS32 = float(np.finfo(np.float32).eps)
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest", "features_dc_thermal", "features_rest_thermal")
NAMES_SEP = NAMES + ("opacities_thermal",)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def num_added(n: int, max_gs_num: int, grow_factor: float) -> int:
    """n_add = max(0, min(max_gs_num, int(grow_factor * N)) - N)"""
    return max(0, min(int(max_gs_num), int(grow_factor * n)) - n)


def new_opacity(c: float, r: int, min_opacity: float) -> float:
    """c' of one chain, clamped"""
    return min(max(1.0 - (1.0 - c) ** (1.0 / r), min_opacity), 1.0 - EPS32)


def denominator(p_new: float, r: int) -> float:
    """sum_{i=1..r} sum_{k=0..i-1} binom(i-1, k) (-1)^k p'^(k+1) / sqrt(k+1), binomials as exact integers"""
    total = 0.0
    for i in range(1, r + 1):
        for k in range(i):
            total += float(math.comb(i - 1, k)) * (-1.0) ** k * p_new ** (k + 1) / math.sqrt(k + 1)
    return total


def relocation_value(opacity_logit: float, scale_logs, ratio: int, min_opacity: float, opacity_thermal_logit=None):
    """(new opacity logit, new thermal opacity logit or None, new log-scales [3]) of one source, all float64"""
    r = min(max(int(ratio), 1), N_MAX)
    o = float(sigmoid(opacity_logit))
    p = o
    logit = lambda c: math.log(c / (1.0 - c))  # noqa: E731
    new_o = logit(new_opacity(o, r, min_opacity))
    new_th = None
    if opacity_thermal_logit is not None:
        o_th = float(sigmoid(opacity_thermal_logit))
        new_th = logit(new_opacity(o_th, r, min_opacity))
        if o_th > o:
            p = o_th
    p_new = 1.0 - (1.0 - p) ** (1.0 / r)
    gain = p / denominator(p_new, r)
    s = np.exp(np.asarray(scale_logs, dtype=np.float64))
    return new_o, new_th, np.log(gain * s)


def relocate(params: dict, exp_avg: dict, exp_avg_sq: dict, src, dst, min_opacity: float):
    """params / exp_avg / exp_avg_sq: name -> array with one row count (moment dicts may lack names: no Adam state).  Returns new
    (params, exp_avg, exp_avg_sq) as float64 copies of float32-valued inputs; `src`, `dst`: integer sequences of one length."""
    sep = "opacities_thermal" in params
    out = {k: np.array(v, dtype=np.float64) for k, v in params.items()}
    m1 = {k: np.array(v, dtype=np.float64) for k, v in exp_avg.items()}
    m2 = {k: np.array(v, dtype=np.float64) for k, v in exp_avg_sq.items()}
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    drawn, counts = np.unique(src, return_counts=True)
    value = {}
    for s, c in zip(drawn.tolist(), counts.tolist()):  # from the values BEFORE the call
        value[s] = relocation_value(float(params["opacities"][s, 0]), params["scales"][s], c + 1, min_opacity,
                                    float(params["opacities_thermal"][s, 0]) if sep else None)
    for s, (new_o, new_th, new_s) in value.items():
        out["opacities"][s, 0] = new_o
        out["scales"][s] = new_s
        if sep:
            out["opacities_thermal"][s, 0] = new_th
        for k in m1:
            m1[k][s] = 0.0
            m2[k][s] = 0.0
    for s, d in zip(src.tolist(), dst.tolist()):
        for k in out:
            out[k][d] = out[k][s]
    return out, m1, m2


def rotation(quats):
    """[N,3,3] of quats [N,4] (w x y z), normalised first"""
    q = np.asarray(quats, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def visible_opacity(opacities, opacities_thermal=None):
    o = sigmoid(opacities).reshape(-1)
    return o if opacities_thermal is None else np.maximum(o, sigmoid(opacities_thermal).reshape(-1))


def noise_delta(scales, quats, opacities, z, scaler: float, opacities_thermal=None):
    """Sigma (z g scaler) [N,3] in float64"""
    g = 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - visible_opacity(opacities, opacities_thermal)) - 0.995)))
    R = rotation(quats)
    s2 = np.exp(np.asarray(scales, dtype=np.float64)) ** 2
    cov = np.einsum("nij,nj,nkj->nik", R, s2, R)
    v = np.asarray(z, dtype=np.float64) * g[:, None] * scaler
    return np.einsum("nij,nj->ni", cov, v)


def noise(means, scales, quats, opacities, z, scaler: float, opacities_thermal=None):
    return np.asarray(means, dtype=np.float64) + noise_delta(scales, quats, opacities, z, scaler, opacities_thermal)


def noise_delta_torch(scales, quats, opacities, z, scaler: float, opacities_thermal=None):
    """the same formula as plain torch ops at the inputs' dtype and device (gsplat's inject_noise_to_position: covariance [N,3,3], then bmm)"""
    import torch

    o = torch.sigmoid(opacities).reshape(-1)
    if opacities_thermal is not None:
        o = torch.maximum(o, torch.sigmoid(opacities_thermal).reshape(-1))
    g = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - o) - 0.995)))
    q = quats / quats.norm(dim=-1, keepdim=True)
    w, x, y, zq = q.unbind(-1)
    R = torch.stack([torch.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - w * zq), 2 * (x * zq + w * y)], -1),
                     torch.stack([2 * (x * y + w * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - w * x)], -1),
                     torch.stack([2 * (x * zq - w * y), 2 * (y * zq + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    M = R * torch.exp(scales)[:, None, :]
    cov = torch.bmm(M, M.transpose(1, 2))
    v = z * g[:, None] * scaler
    return torch.bmm(cov, v[:, :, None]).squeeze(-1)
