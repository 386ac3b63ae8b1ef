"""Restatement of the shared (rig) pose correction of thermal-nerfacto, written from the oracle's exp map and per-camera apply
(oracle.thermal_nerfacto_oracle.exp_map_so3xr3 / apply_pose_adjustment) with the one row expanded to every camera:

    o1 = o0 + t_s, d1 = R_s d0     [R_s | t_s] = exp_map_SO3xR3(row), the identity on frozen cameras   (shared row, training and evaluation)
    o2 = o1 + t_c, d2 = R_c d1     the per-camera correction on top, training only                      (same frozen mask)

Everything follows the dtype of its inputs: float64 tensors give the reference, float32 tensors "the same expressions in fp32 torch" that
the GPU tests take their error bound from.  The row's gradient is autograd's.
"""
import torch

import thermal_nerfacto_oracle as orc


def shared_apply(row, frozen_cam, cam, origins, directions):
    """row [1,6], frozen_cam bool [C], cam int64 [N], rays [N,3] -> (o1, d1)."""
    return orc.apply_pose_adjustment(row.expand(frozen_cam.shape[0], 6), frozen_cam, cam, origins, directions)


def composed_apply(row, pose, frozen_cam, cam, origins, directions):
    """The rays the render sees: the shared correction, then (pose [C,6] not None) the per-camera one on top of it."""
    o, d = shared_apply(row, frozen_cam, cam, origins, directions)
    if pose is not None:
        o, d = orc.apply_pose_adjustment(pose, frozen_cam, cam, o, d)
    return o, d


def row_gradient(row, pose, frozen_cam, cam, origins, directions, g_o, g_d):
    """d/d row of <g_o, o2> + <g_d, d2>: what tn_pose_shared_bwd adds to the row's gradient."""
    r = row.detach().clone().requires_grad_(True)
    o, d = composed_apply(r, pose, frozen_cam, cam, origins, directions)
    ((o * g_o).sum() + (d * g_d).sum()).backward()
    return r.grad


def regularizer(row, trans_pen, rot_pen, scale):
    """CameraOptimizer.get_loss_dict over the one row (cameras/camera_optimizers.py:189-195)."""
    return orc.camera_opt_regularizer(row, orc.OracleConfig(trans_l2_penalty=trans_pen, rot_l2_penalty=rot_pen), scale)


def rows(dtype=torch.float64):
    """The three rows of the tests: exactly 0 (the exp map's clamped small-angle branch), |w| = 1e-6, |w| ~ 0.3 with a translation."""
    w = torch.tensor([0.6, -0.3, 0.74], dtype=torch.float64)
    w = w / w.norm()
    return {
        "zero": torch.zeros(1, 6, dtype=dtype),
        "tiny": torch.cat([torch.zeros(3, dtype=torch.float64), 1e-6 * w])[None].to(dtype),
        "rig": torch.cat([torch.tensor([0.04, -0.02, 0.03], dtype=torch.float64), 0.3 * w])[None].to(dtype),
    }


def rays(n, seed=5, frozen_block=None, frozen_cams=(4, 5, 6, 7), num_cameras=8):
    """n rays (float32, as the kernels take them) over `num_cameras` cameras of both spectra; frozen_block = (lo, hi): those rays all come from
    frozen cameras (a whole reduction block that contributes nothing)."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    cam = torch.randint(0, num_cameras, (n,), generator=g)
    if frozen_block is not None and n > frozen_block[0]:
        lo, hi = frozen_block[0], min(frozen_block[1], n)
        cam[lo:hi] = torch.tensor(frozen_cams)[torch.randint(0, len(frozen_cams), (hi - lo,), generator=g)]
    return o, d, cam
