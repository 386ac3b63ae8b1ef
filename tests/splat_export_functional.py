"""Torch-CPU restatement of tn_export_splat_pack (csrc/tn_splat_export.hip) and the inputs of the splat-export tests.  Plain torch, no import
of the package.

pack_ref builds the rows of include/thermal_nerf_hip.h's layout by indexing alone (no float arithmetic, so the rows are exact) except under
colour_mode 1, whose map f = (sigmoid(dc) - 0.5) / C0 is evaluated in float64 and rounded once; and it keeps a Gaussian by the same float
compares as the kernel: isfinite on the parameters the row is made of, `logit >= threshold` on float32 values, and the crop box in the kernel's
seven fp32 operations (the test scenes hold no mean in the rounding band of a face, so a float64 evaluation would decide the same)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

import splat_crop_functional as scf

SH_C0 = 0.28209479177387814
SPECTRA = {"rgb": 0, "thermal": 1, "both": 2}
ATTRIBUTES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest", "features_dc_thermal", "features_rest_thermal",
              "opacities_thermal")
THERMAL_ONLY = ("features_dc_thermal", "features_rest_thermal", "opacities_thermal")
RGB_ONLY = ("features_dc", "features_rest")  # (opacities is the thermal row's opacity too in shared mode)


def properties(spectrum: str, K: int, separate: bool, colour_mode: int = 0):
    """The property lists, spelled out independently of splat_io.ply_properties (the layout of include/thermal_nerf_hip.h)."""
    R = 0 if colour_mode == 1 else K - 1
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    names += [f"f_rest_{i}" for i in range(3 * R)]
    names += ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    if spectrum == "both":
        names.append("f_dc_thermal")
        names += [f"f_rest_thermal_{i}" for i in range(R)]
        if separate:
            names.append("opacity_thermal")
    return names


def dc_colour64(dc: Tensor) -> Tensor:
    """colour_mode 1: (sigmoid(dc) - 0.5) / C0 in float64, rounded once to float32."""
    x = dc.double()
    return ((1.0 / (1.0 + torch.exp(-x)) - 0.5) / SH_C0).float()


def in_box_fp32(box, means: Tensor) -> Tensor:
    """The kernel's box test: q_i = ((m_i0 x + m_i1 y) + m_i2 z) + m_i3 in fp32, every operation rounded on its own; |q_i| < S_i / 2."""
    m = scf.world_to_box(box)
    h = 0.5 * box.S.float()
    x, y, z = means[:, 0], means[:, 1], means[:, 2]
    inside = torch.ones(means.shape[0], dtype=torch.bool)
    for i in range(3):
        q = ((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3]
        inside &= q.abs() < h[i]
    return inside


def pack_ref(params: Dict[str, Tensor], spectrum: str, colour_mode: int = 0, min_opacity_logit: float = -math.inf, crop=None) -> Tuple[Tensor, Tensor]:
    """(rows [kept, W] float32, kept_index [kept] int64) of float32 host `params` (with opacities_thermal: separate mode)."""
    p = {k: v.detach().float() for k, v in params.items()}
    n, R = p["means"].shape[0], p["features_rest"].shape[1]
    sep = "opacities_thermal" in p
    assert colour_mode in (0, 1) and (colour_mode == 0 or R == 0)
    dc_map = dc_colour64 if colour_mode == 1 else (lambda t: t)
    th = spectrum == "thermal"
    op_row = p["opacities_thermal"] if (th and sep) else p["opacities"]
    if th:
        f_dc = dc_map(p["features_dc_thermal"]).expand(n, 3)
        f_rest = p["features_rest_thermal"].reshape(n, 1, R).expand(n, 3, R).reshape(n, 3 * R)
    else:
        f_dc = dc_map(p["features_dc"])
        f_rest = p["features_rest"].transpose(1, 2).reshape(n, 3 * R)  # f_rest_{c R + k} = features_rest[g, k, c]
    cols = [p["means"], torch.zeros(n, 3), f_dc, f_rest, op_row.reshape(n, 1), p["scales"], p["quats"]]
    if spectrum == "both":
        cols += [dc_map(p["features_dc_thermal"]).reshape(n, 1), p["features_rest_thermal"].reshape(n, R)]
        if sep:
            cols.append(p["opacities_thermal"].reshape(n, 1))
    rows = torch.cat([c.reshape(n, -1) for c in cols], 1).contiguous()
    # the parameters the row is made of
    used = ["means", "scales", "quats"]
    if spectrum != "thermal":
        used += ["opacities", "features_dc", "features_rest"]
    if spectrum != "rgb":
        used += ["features_dc_thermal", "features_rest_thermal"]
        if sep:
            used.append("opacities_thermal")
        elif th:
            used.append("opacities")
    keep = torch.ones(n, dtype=torch.bool)
    for k in used:
        keep &= torch.isfinite(p[k].reshape(n, -1)).all(1)
    if spectrum == "both" and sep:
        logit = torch.maximum(p["opacities"], p["opacities_thermal"]).reshape(n)
    else:
        logit = op_row.reshape(n)
    keep &= logit >= torch.tensor(min_opacity_logit, dtype=torch.float32)
    if crop is not None:
        keep &= in_box_fp32(crop, p["means"])
    idx = keep.nonzero().reshape(-1)
    return rows[idx].contiguous(), idx


def random_params(n: int, K: int, separate: bool, seed: int) -> Dict[str, Tensor]:
    """n Gaussians with K coefficients per channel: finite normal draws (no two attributes share a value pattern, so a misplaced column shows)."""
    g = torch.Generator().manual_seed(7000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    p = {"means": r(n, 3), "scales": r(n, 3) - 3.0, "quats": r(n, 4), "opacities": 2.0 * r(n, 1), "features_dc": r(n, 3),
         "features_rest": 0.1 * r(n, K - 1, 3), "features_dc_thermal": r(n, 1), "features_rest_thermal": 0.1 * r(n, K - 1, 1)}
    if separate:
        p["opacities_thermal"] = 2.0 * r(n, 1)
    return p


DEFECTS = (float("nan"), float("inf"), float("-inf"))


def plant_defects(params: Dict[str, Tensor], seed: int) -> Dict[str, Tensor]:
    """A copy of `params` with one value that is not finite in each attribute class in turn: Gaussian 5 i + 2 (mod n) takes the defect of class i,
    NaN, +Inf and -Inf in rotation, at a seeded position inside the attribute's row."""
    p = {k: v.clone() for k, v in params.items()}
    n = p["means"].shape[0]
    g = torch.Generator().manual_seed(7100 + seed)
    for i, name in enumerate(a for a in ATTRIBUTES if a in p):
        flat = p[name].reshape(n, -1)
        if flat.shape[1] == 0:
            continue
        flat[(5 * i + 2) % n, int(torch.randint(flat.shape[1], (1,), generator=g))] = DEFECTS[(i + seed) % 3]
    return p


def ulp32(x: Tensor) -> Tensor:
    """The spacing of float32 at |x| (the distance to the next float32 away from zero)."""
    a = x.detach().float().abs()
    return (torch.nextafter(a, torch.tensor(float("inf"))) - a).double()
