"""tn_transform_splat restated in torch float64 on the CPU, op for op, from the entry point's contract (include/thermal_nerf_hip.h), and the scene
the render-invariance tests share.

`transform_ref` takes the TnSplatTransform fields as float64 tensors -- A [3,3] (= s R), t [3], log_scale (a float), q [4] (w, x, y, z of R), sh1
[3,3], sh2 [5,5], sh3 [7,7] -- and float32 parameters; every output value is evaluated in float64 from the float32 inputs widened, every product
and sum rounded on its own (torch evaluates each operator separately: nothing is contracted), in the contract's order, and rounded once to
float32.  A tensor-by-scalar product in float64 is the same IEEE operation as the kernel's, so the results are bit-equal.
"""
import functools
import math
from typing import Dict, Tuple

import torch
from torch import Tensor

import splat_oracle as so

F64 = torch.float64
MOVED = ("means", "scales", "quats", "features_rest", "features_rest_thermal")
BANDS = ((0, 3, "sh1"), (3, 8, "sh2"), (8, 15, "sh3"))  # rest coefficients k0..k1 of band 1, 2, 3 and the field that moves them


def fields(scale: float, R: Tensor, t: Tensor, q: Tensor, mats: Tuple[Tensor, Tensor, Tensor]) -> Dict[str, object]:
    """The TnSplatTransform fields of x' = scale R x + t, float64."""
    return {"A": scale * R.to(F64), "t": t.to(F64), "log_scale": math.log(scale), "q": q.to(F64), "sh1": mats[0].to(F64), "sh2": mats[1].to(F64),
            "sh3": mats[2].to(F64)}


def _band(M: Tensor, c: Tensor) -> Tensor:
    """c [N,D,C] float64 -> sum_j M[k][j] c[:,j], j ascending, starting from the first product."""
    out = []
    for k in range(M.shape[0]):
        acc = float(M[k, 0]) * c[:, 0]
        for j in range(1, M.shape[1]):
            acc = acc + float(M[k, j]) * c[:, j]
        out.append(acc)
    return torch.stack(out, 1)


def rotate_rest(f: Dict[str, object], rest: Tensor) -> Tensor:
    """rest [N,R,C] (R in 0, 3, 8, 15) -> the moved coefficients, float32."""
    R = rest.shape[1]
    if R not in (0, 3, 8, 15):
        raise ValueError(f"{R} rest coefficients")
    c = rest.to(F64)
    out = c.clone()
    for k0, k1, name in BANDS:
        if R >= k1:
            out[:, k0:k1] = _band(f[name], c[:, k0:k1])
    return out.float()


def transform_ref(f: Dict[str, object], p: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """The five moved tensors of the parameters `p` (float32, host)."""
    A, t = f["A"].tolist(), f["t"].tolist()
    m = p["means"].to(F64)
    x, y, z = m[:, 0], m[:, 1], m[:, 2]
    means = torch.stack([((A[i][0] * x + A[i][1] * y) + A[i][2] * z) + t[i] for i in range(3)], -1).float()
    scales = (p["scales"].to(F64) + float(f["log_scale"])).float()
    w1, x1, y1, z1 = f["q"].tolist()
    q = p["quats"].to(F64)
    w2, x2, y2, z2 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    quats = torch.stack([((w1 * w2 - x1 * x2) - y1 * y2) - z1 * z2, ((w1 * x2 + x1 * w2) + y1 * z2) - z1 * y2,
                         ((w1 * y2 - x1 * z2) + y1 * w2) + z1 * x2, ((w1 * z2 + x1 * y2) - y1 * x2) + z1 * w2], -1).float()
    return {"means": means, "scales": scales, "quats": quats, "features_rest": rotate_rest(f, p["features_rest"]),
            "features_rest_thermal": rotate_rest(f, p["features_rest_thermal"])}


def moved_params(f: Dict[str, object], p: Dict[str, Tensor]) -> Dict[str, Tensor]:
    return {**p, **transform_ref(f, p)}


def bits(t: Tensor) -> Tensor:
    return t.detach().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- the invariance scene
W, H, FX = 96, 72, 80.0
EYE = (2.4, 0.5, 0.7)
T_VEC = (0.7, -1.3, 0.4)
SCALES = (1.0, 2.5, 0.4)
N_SCENE = 300


def seeded_rotation(seed: int = 5) -> Tuple[Tensor, Tensor]:
    """(R [3,3], q [4] with w >= 0) float64 of a seeded unit quaternion: a rotation with no special axis."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(4, generator=g, dtype=F64)
    q = q / q.norm()
    if float(q[0]) < 0:
        q = -q
    return so.quat_to_rotmat(q[None])[0], q


@functools.lru_cache(maxsize=None)
def scene(sh_degree: int = 3) -> Dict[str, Tensor]:
    """synth_gaussians(300, seed=3, extent=0.6, scale_range=(-3.5, -2.0)) with thermal opacities of their own (a seeded draw, for the separate
    mode; shared-mode users drop the entry); sh_degree 0 keeps no rest coefficients."""
    p = so.synth_gaussians(N_SCENE, seed=3, extent=0.6, scale_range=(-3.5, -2.0))
    g = torch.Generator().manual_seed(31)
    p["opacities_thermal"] = (torch.rand(N_SCENE, 1, generator=g) * 6.0 - 2.0)
    if sh_degree == 0:
        p["features_rest"], p["features_rest_thermal"] = p["features_rest"][:, :0].contiguous(), p["features_rest_thermal"][:, :0].contiguous()
    return p


def camera_c2w() -> Tensor:
    return so.look_at_camera(EYE)


def moved_c2w(scale: float, R: Tensor, t: Tensor, c2w: Tensor) -> Tensor:
    """rotation R c2w_R, position scale R c2w_t + t, float64, rounded once."""
    c = c2w.to(F64)
    return torch.cat([R @ c[:, :3], (scale * (R @ c[:, 3]) + t)[:, None]], 1).float()


def _render(p, c2w, deg, mode):
    return so.render(p, c2w, FX, FX, W / 2, H / 2, W, H, sh_degree_to_use=deg, rasterize_mode=mode)


def image_differences(a: Dict[str, Tensor], b: Dict[str, Tensor], scale: float) -> Dict[str, float]:
    """The largest differences of two renders of one frame, b in the frame moved by `scale`: rgb, thermal, accumulation, and depth relative to
    scale * depth where a's accumulation > 0.5."""
    solid = a["accumulation"] > 0.5
    rel = ((b["depth"] - scale * a["depth"]).abs() / (scale * a["depth"]).abs())[solid]
    return {"rgb": float((a["rgb"] - b["rgb"]).abs().max()), "thermal": float((a["thermal"] - b["thermal"]).abs().max()),
            "accumulation": float((a["accumulation"] - b["accumulation"]).abs().max()), "depth": float(rel.max()) if rel.numel() else 0.0}


@functools.lru_cache(maxsize=None)
def oracle_pair(scale: float, deg: int, mode: str, thermal_chain: bool, make_fields) -> Tuple[Dict[str, Tensor], Dict[str, Tensor]]:
    """(the oracle's float32 render of the scene, its render of the restatement-moved scene from the moved camera) with `deg` active SH degrees
    (-1: the sh_degree == 0 model).  thermal_chain: the separate mode's thermal chain, the same renderer with the thermal opacities.
    make_fields(scale, R, t) -> the TnSplatTransform fields (the package's band matrices and quaternion, which the CPU tests check on their own)."""
    p = dict(scene(0 if deg < 0 else 3))
    if thermal_chain:
        p["opacities"] = p["opacities_thermal"]
    del p["opacities_thermal"]
    R, _ = seeded_rotation()
    t = torch.tensor(T_VEC, dtype=F64)
    c2w = camera_c2w()
    return _render(p, c2w, deg, mode), _render(moved_params(make_fields(scale, R, t), p), moved_c2w(scale, R, t, c2w), deg, mode)


def oracle_floor(scale: float, deg: int, mode: str, separate: bool, make_fields) -> Dict[str, float]:
    """The oracle's own float32 difference between the two frames: {"image": the largest of rgb, thermal and accumulation -- one number, because
    the three are blends with the same alphas and transmittances and all of order one, "depth": the relative one}.  In separate mode the larger of
    the two chains'."""
    out = {"image": 0.0, "depth": 0.0}
    for chain in ((False, True) if separate else (False,)):
        a, b = oracle_pair(scale, deg, mode, chain, make_fields)
        d = image_differences(a, b, scale)
        out = {"image": max(out["image"], d["rgb"], d["thermal"], d["accumulation"]), "depth": max(out["depth"], d["depth"])}
    return out
