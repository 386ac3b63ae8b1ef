"""Pose refinement of the splat render restated in torch, any dtype, differentiable by autograd: the reference of tests/test_splat_pose_cpu.py and
tests/test_splat_pose_gpu.py.  Not a test module.

A pose row p = (t, w): A(p) = [R(w) | t] is exp_map_SO3xR3 (cameras/lie_groups.py:24-58, theta = sqrt(clamp(|w|^2, 1e-4))), applied as
c2w' = c2w [A(p); 0 0 0 1] (CameraOptimizer.apply_to_camera, cameras/camera_optimizers.py:178-186).  View and projection matrices follow from
c2w' as splat_oracle.camera_matrices builds them, but in the dtype of c2w' (nothing here calls .float()); the render is splat_functional's
projection and front-to-back walk (two walks in separate mode, as splat_sep_functional.render arranges them) with those matrices, the SH view
directions taken from the corrected position as a value (splatfacto.py:770).  Scenes and cameras are those of tests/splat_backward_cases.py; for a
non-zero row the scene is depth-separated again for the corrected camera (a moved camera can bring two depths closer than float32 orders, which
would inflate the float32 floor)."""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional

import torch
from torch import Tensor

import splat_backward_cases as bc
import splat_functional as sf
import splat_oracle as so
import test_splat_forward_cpu as fc

POSES = {
    "zero": (0.0, 0.0, 0.0, 0.0, 0.0, 0.0),  # identity
    "small": (1e-3, 0.0, 0.0, 2e-3, -1e-3, 3e-3),  # |w|^2 = 1.4e-5: below the theta clamp, the theta derivative is 0
    "moved": (0.02, -0.015, 0.01, 0.012, -0.02, 0.015),  # |w|^2 = 7.7e-4: above the clamp
}


def pose_row(name: str, dtype=torch.float64) -> Tensor:
    return torch.tensor(POSES[name], dtype=dtype)


def exp_map(p: Tensor):
    """A(p) = (R [3,3], t [3]) in p's dtype."""
    t, w = p[:3], p[3:]
    theta = torch.sqrt(torch.clamp((w * w).sum(), min=1e-4))
    f1 = torch.sin(theta) / theta
    f2 = (1.0 - torch.cos(theta)) / (theta * theta)
    z = torch.zeros((), dtype=p.dtype)
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    return torch.eye(3, dtype=p.dtype) + f1 * K + f2 * (K @ K), t


def apply_pose(c2w: Tensor, p: Tensor) -> Tensor:
    """c2w [3,4] . [A(p); 0 0 0 1] in p's dtype."""
    R, t = exp_map(p)
    Rc, Tc = c2w[:3, :3].to(p.dtype), c2w[:3, 3].to(p.dtype)
    return torch.cat([Rc @ R, (Rc @ t + Tc)[:, None]], 1)


def camera_matrices(c2w: Tensor, fx: float, fy: float, W: int, H: int):
    """so.camera_matrices in c2w's dtype: (view [4,4], projection [4,4])."""
    dt = c2w.dtype
    R = c2w[:3, :3] @ torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=dt))
    R_inv = R.T
    T_inv = -R_inv @ c2w[:3, 3:4]
    view = torch.cat([torch.cat([R_inv, T_inv], 1), torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=dt)], 0)
    P = so.projection_matrix(0.001, 1000, 2 * math.atan(W / (2 * fx)), 2 * math.atan(H / (2 * fy))).to(dt)
    return view, P @ view


def render(params: Dict[str, Tensor], cam, pose: Tensor, mode: str, deg: int, viewdir_position: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """The training render of `params` (dtype of params["means"]) through the camera `cam` = (c2w, fx, fy, cx, cy, W, H) corrected by `pose`
    [6].  deg: the config's SH degree (0: sigmoid colours).  With opacities_thermal among the parameters the thermal channel walks with its own
    opacity.  viewdir_position [3]: where the SH view directions are taken from (default: the corrected position, detached); finite differences
    in the pose pass the unperturbed one, since the view directions carry no gradient.  Returns rgb, thermal (clamped), accumulation
    (+ accumulation_thermal), xys, view (the corrected [4,4] view matrix, a node of the graph), projection, flag_pixels, flag_gaussians."""
    c2w, fx, fy, cx, cy, W, H = cam
    dt = params["means"].dtype
    sep = "opacities_thermal" in params
    c2w2 = apply_pose(c2w.to(dt), pose.to(dt))
    view, proj = camera_matrices(c2w2, fx, fy, W, H)
    means = params["means"]
    quats = params["quats"] / params["quats"].norm(dim=-1, keepdim=True)
    pj = sf.project(means, torch.exp(params["scales"]), quats, view, proj, fx, fy, cx, cy, H, W, flag_tol=fc.FLAG_TOL)
    viewdirs = means.detach() - (c2w2[:3, 3].detach() if viewdir_position is None else viewdir_position.to(dt))
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    col = torch.cat([params["features_dc"][:, None, :], params["features_rest"]], 1)
    col_t = torch.cat([params["features_dc_thermal"][:, None, :], params["features_rest_thermal"]], 1)
    near_sh = torch.zeros(means.shape[0], dtype=torch.bool)
    if deg > 0 and col.shape[1] > 1:
        sh = torch.cat([so.spherical_harmonics(deg, viewdirs, col), so.spherical_harmonics(deg, viewdirs, col_t)], -1) + 0.5
        near_sh = (sh.detach().abs() < fc.FLAG_TOL).any(-1)
        colors = torch.clamp(sh, min=0.0)
    else:
        colors = torch.sigmoid(torch.cat([col[:, 0], col_t[:, 0]], -1))
    scale = pj["compensation"] if mode == "antialiased" else 1.0
    op = torch.sigmoid(params["opacities"])[:, 0] * scale
    bg, bgt = fc.background()
    bg4 = torch.cat([bg, torch.tensor([bgt])]).to(dt)
    geom = (pj["xys"], pj["depths"], pj["radii"], pj["conics"], pj["tile_min"], pj["tile_max"])
    if sep:
        op_t = torch.sigmoid(params["opacities_thermal"])[:, 0] * scale
        img, alpha, flag_pix, flag_g = sf.rasterize(*geom, colors[:, :3], op, H, W, bg4[:3], flag_tol=fc.FLAG_TOL)
        img_t, alpha_t, fp_t, fg_t = sf.rasterize(*geom, colors[:, 3:], op_t, H, W, bg4[3:], flag_tol=fc.FLAG_TOL)
        raw, flag_pix, flag_g = torch.cat([img, img_t], -1), flag_pix | fp_t, flag_g | fg_t
    else:
        raw, alpha, flag_pix, flag_g = sf.rasterize(*geom, colors, op, H, W, bg4, flag_tol=fc.FLAG_TOL)
    out = {"rgb": torch.clamp(raw[..., :3], max=1.0), "thermal": torch.clamp(raw[..., 3:], max=1.0), "accumulation": alpha[..., None], "xys": pj["xys"],
           "view": view, "projection": pj, "flag_pixels": flag_pix, "flag_gaussians": flag_g | (pj["near_clamp"] & pj["ok"]) | (near_sh & pj["ok"])}
    if sep:
        out["accumulation_thermal"] = alpha_t[..., None]
    return out


def scene(case: str, deg: int, sep: Optional[str], pose_name: str) -> Dict[str, Tensor]:
    """bc.scene, depth-separated once more for the corrected camera when the row is not zero."""
    p = bc.scene(case, deg, sep)
    if pose_name == "zero":
        return p
    c2w2 = apply_pose(bc.case_camera(case)[0].double(), pose_row(pose_name)).float()
    return fc._with(p, means=sf.separate_depths(p["means"], c2w2, bc.MIN_GAP))


def grads(p: Dict[str, Tensor], case: str, mode: str, deg: int, pose: Tensor, w: Optional[Dict[str, Tensor]], dt):
    """d sum(output * w) / d (every parameter, xys, the pose row, the corrected view matrix's three rows) as float64 tensors, by autograd in
    `dt`; w None: drawn here (bc.upstream), zero on the pixels this render flags.  Returns (gradients, the render detached, w)."""
    leaves = {k: v.to(dt).requires_grad_(True) for k, v in p.items()}
    row = pose.to(dt).requires_grad_(True)
    out = render(leaves, bc.case_camera(case), row, mode, deg)
    if w is None:
        w = bc.upstream(case, "sep" if "opacities_thermal" in p else None, out["flag_pixels"])
    loss = sum((out[k] * w[k].to(dt)).sum() for k in w)
    g = torch.autograd.grad(loss, list(leaves.values()) + [out["xys"], row, out["view"]], allow_unused=True)
    named = {k: (torch.zeros_like(v) if gi is None else gi).detach().double() for (k, v), gi in zip(leaves.items(), g)}
    named["xys"], named["pose"], named["dview"] = g[-3].detach().double(), g[-2].detach().double(), g[-1].detach().double()[:3]
    return named, {k: (v.detach() if isinstance(v, Tensor) else {a: b.detach() for a, b in v.items()}) for k, v in out.items()}, w


@functools.lru_cache(maxsize=None)
def reference(case: str, mode: str, deg: int, sep: Optional[str], pose_name: str):
    """What the tests of one configuration and pose row share, computed once and never modified: the scene `p`, the row `pose`, the float64
    render `out64` and the float32 one `out32`, the upstream images `w` (bc.upstream: zero on the pixels float64 flags), the gradients `g64`
    and `g32`, and `flagged`, the share of flagged pixels.  One forward and one backward per dtype."""
    p = scene(case, deg, sep, pose_name)
    pose = pose_row(pose_name)
    g64, out64, w = grads(p, case, mode, deg, pose, None, torch.float64)
    g32, out32, _ = grads(p, case, mode, deg, pose, w, torch.float32)
    return {"p": p, "pose": pose, "out64": out64, "out32": out32, "w": w, "g64": g64, "g32": g32, "flagged": float(out64["flag_pixels"].float().mean())}


def vec_err(a: Tensor, b: Tensor) -> float:
    """max |a - b| relative to b's largest entry (inf when b is all zero and a is not)."""
    scale = bc.amax(b)
    if scale == 0.0:
        return 0.0 if bc.amax(a) == 0.0 else math.inf
    return bc.amax(a.double() - b.double()) / scale


def floor(ref, key: str = "pose") -> float:
    """The float32 floor of a whole-frame gradient: the float32 restatement's own distance from float64, never below 2^-23."""
    return max(vec_err(ref["g32"][key], ref["g64"][key]), bc.EPS)
