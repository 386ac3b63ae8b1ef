"""Float64 restatement of the crop box of the splat eval render (OrientedBox / tn_splat_project's crop / tn_splat_crop_mask), and the scenes of
the crop tests.  Plain torch, no import of the package: a box is anything with R [3,3], T [3] and S [3] (`Box` here, OrientedBox there).

The rule (nerfstudio/data/scene_box.py:82-114): box -> world is p = R q + T; a point is inside iff -S_i/2 < q_i < S_i/2 on all three axes,
strictly.  The kernel evaluates q from the world -> box matrix M = inverse([R|T]) [3,4], inverted in float64 and ROUNDED TO FP32 -- that matrix is
part of the definition, so the restatement starts from the same fp32 matrix (`world_to_box`) and only the evaluation of q differs: float64 here,

    fl(q_i) = ((M_i0 x (*) + M_i1 y) (+) M_i2 z) (+) M_i3        seven fp32 operations, each rounded to nearest, none fused

in the kernel (csrc/tn_splat.hip, splat_in_crop) and in OrientedBox.within's torch path on fp32 tensors.

`near_boundary`: where may the two disagree?  With u = 2^-24 the unit roundoff, every operation returns its exact result times (1 + d), |d| <= u.
A product passes through its own rounding and up to three sums, M_i3 through one: |fl(q_i) - q_i| <= ((1 + u)^4 - 1) A_i <= 4.0001 u A_i with
A_i = |M_i0 x| + |M_i1 y| + |M_i2 z| + |M_i3|, the "magnitude of the points" in box axes (the standard bound of a 4-term dot product).  The
inputs are exact in both (fp32 points, fp32 matrix, S_i / 2 exact in fp32 and float64), and the comparison itself is exact.  So the decisions can
differ only where | |q_i| - S_i/2 | <= 4.0001 u A_i.  The band the tests use adds 8 fp32 ulps of max(|q_i|, S_i/2, 1) (8 * 2^-23 of it) on top as
room -- eps_i = 2^-20 max(|q_i|, S_i/2, 1) + 4.0001 * 2^-24 A_i -- and the scenes are REQUIRED to have no point in it (tests/test_splat_crop_cpu.py),
so the GPU tests may demand exact keep sets."""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

import splat_sep_functional as ssf

U = 2.0 ** -24  # fp32 unit roundoff
N_SCENE, W, H = 300, 96, 72  # blocks of 128, 128 and 44 Gaussians; 6 x 4.5 tiles
THR = 0.05  # removal_min_opacity_diff of the separate-mode cases


class Box(NamedTuple):
    R: Tensor
    T: Tensor
    S: Tensor


def rotation_rpy(roll: float, pitch: float, yaw: float) -> Tensor:
    """Rz(yaw) Ry(pitch) Rx(roll), the float64 matrix product."""
    def rot(a, i, j):
        m = torch.eye(3, dtype=torch.float64)
        m[i, i] = m[j, j] = math.cos(a)
        m[i, j], m[j, i] = -math.sin(a), math.sin(a)
        return m
    return rot(yaw, 0, 1) @ rot(pitch, 2, 0) @ rot(roll, 1, 2)


def box_from_params(pos, rpy, scale) -> Box:
    return Box(rotation_rpy(*rpy).float(), torch.tensor(pos, dtype=torch.float32), torch.tensor(scale, dtype=torch.float32))


def world_to_box(box) -> Tensor:
    """[3,4] fp32: inverse([R|T]) by float64 inverse, rounded to fp32."""
    R, T = box.R.detach().cpu().double(), box.T.detach().cpu().double()
    Rinv = torch.linalg.inv(R)
    return torch.cat([Rinv, -(Rinv @ T)[:, None]], 1).float()


def _q64(box, pts: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """q [n,3] in float64 from the fp32 matrix, A [n,3] (sum of the magnitudes of the four terms), h [3] = S / 2."""
    M = world_to_box(box).double()
    p = pts.detach().cpu().double()
    terms = torch.cat([M[None, :, :3] * p[:, None, :], M[None, :, 3:].expand(p.shape[0], 3, 1)], -1)  # [n,3,4]
    return terms.sum(-1), terms.abs().sum(-1), 0.5 * box.S.detach().cpu().float().double()


def within64(box, pts: Tensor) -> Tensor:
    q, _, h = _q64(box, pts)
    return ((q > -h) & (q < h)).all(-1)


def near_boundary(box, pts: Tensor, eps: Optional[Tensor] = None) -> Tensor:
    """bool [n]: any | |q_i| - S_i/2 | < eps_i; eps_i as derived in the module docstring unless given."""
    q, A, h = _q64(box, pts)
    if eps is None:
        eps = 8 * 2.0 ** -23 * torch.maximum(torch.maximum(q.abs(), h.expand_as(q)), torch.ones_like(q)) + 4.0001 * U * A
    return ((q.abs() - h).abs() < eps).any(-1)


# ---- the boxes and the scene of the GPU tests
_S = (0.8, 1.0, 0.9)
_RPY = (0.2, -0.3, 0.5)
_T = (0.1, -0.05, 0.05)
MAIN_BOX = box_from_params(_T, _RPY, _S)
# the same orientation, centred 1.1 S_x down the box's x axis: it holds block 0, and none of block 2
SECOND_BOX = box_from_params(tuple((torch.tensor(_T, dtype=torch.float64) + rotation_rpy(*_RPY) @ torch.tensor([-1.1 * _S[0], 0.0, 0.0], dtype=torch.float64)).tolist()),
                             _RPY, (1.1 * _S[0], _S[1], _S[2]))
EVERYTHING_BOX = box_from_params((0.0, 0.0, 0.0), (0.0, 0.0, 0.4), (50.0, 50.0, 50.0))
NOTHING_BOX = box_from_params((30.0, 30.0, 30.0), (0.1, 0.2, 0.3), (1.0, 1.0, 1.0))
BLOCKS = (slice(0, 128), slice(128, 256), slice(256, 300))  # the projection kernel's blocks of 128 Gaussians

# the edge cases of `within`: the identity box with S = 2, points on and next to its faces
EDGE_BOX = Box(torch.eye(3), torch.zeros(3), torch.full((3,), 2.0))
_IN1_F32 = 1.0 - 2.0 ** -24  # the fp32 number below 1
EDGE_POINTS = torch.tensor([[1.0, 0.0, 0.0], [_IN1_F32, 0.0, 0.0], [-1.0, 0.0, 0.0], [-_IN1_F32, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0],
                            [0.0, _IN1_F32, -_IN1_F32], [0.0, 0.0, 0.0], [_IN1_F32, _IN1_F32, 1.0]], dtype=torch.float32)
EDGE_INSIDE = torch.tensor([False, True, False, True, False, False, True, True, False])


def crop_scene(seed: int, sh_degree: int) -> Dict[str, Tensor]:
    """300 Gaussians (separate-mode parameters; ssf.shared_params drops the thermal opacity): everything but the means from
    ssf.awkward_scene, shuffled; the means laid out in MAIN_BOX's axes q (p = R q + T), block by block of the projection kernel:
      block 0 (128): q_x in (-1.6, -0.6) S_x, q_y, q_z within 0.45 S  -- all outside MAIN_BOX, all inside SECOND_BOX;
      block 1 (128): q_x in (-1.0, 0.4) S_x, q_y, q_z within 0.7 S    -- some in, some out, of either box;
      block 2 (44):  q within 0.45 S                                   -- all inside MAIN_BOX, all outside SECOND_BOX."""
    g = torch.Generator().manual_seed(4000 + seed)
    p = ssf.awkward_scene(N_SCENE, seed, sh_degree)
    assert p["means"].shape[0] == N_SCENE
    perm = torch.randperm(N_SCENE, generator=g)
    p = {k: v[perm].contiguous() for k, v in p.items()}
    S = torch.tensor(_S, dtype=torch.float64)

    def draw(n, x_lo, x_hi, yz):
        u = torch.rand(n, 3, generator=g, dtype=torch.float64)
        q = (2.0 * u - 1.0) * yz
        q[:, 0] = x_lo + (x_hi - x_lo) * u[:, 0]
        return q * S

    q = torch.cat([draw(128, -1.6, -0.6, 0.45), draw(128, -1.0, 0.4, 0.7), draw(44, -0.45, 0.45, 0.45)])
    p["means"] = (q @ rotation_rpy(*_RPY).T + torch.tensor(_T, dtype=torch.float64)).float().contiguous()
    return p


def subset(params: Dict[str, Tensor], keep: Tensor) -> Dict[str, Tensor]:
    return {k: v[keep].contiguous() for k, v in params.items()}
