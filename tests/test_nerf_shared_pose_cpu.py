"""Shared (rig) pose corrections of thermal-nerfacto, what can be checked without a GPU: the configuration gate, the arena layout, the
host-side argument validation of the two new entry points, and the float64 restatement the GPU tests compare against
(tests/nerf_shared_pose_functional.py) against finite differences."""
import ctypes as C
import os

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
import nerf_shared_pose_functional as fn
from nerfstudio_thermal_amd import _lib
from nerfstudio_thermal_amd.arena import ParamArena
from nerfstudio_thermal_amd.config import CameraOptimizerConfig, ThermalNerfactoModelConfig

SHARED_KEYS = ["shared_camera_optimizer.pose_adjustment", "shared_camera_optimizer_thermal.pose_adjustment"]


def small_cfg(mode="separate", shared=True, **kw):
    c = ThermalNerfactoModelConfig(density_mode=mode, log2_hashmap_size=12, **kw)
    for a in c.proposal_net_args_list:
        a["log2_hashmap_size"] = 10
    if shared:
        c.shared_camera_optimizer = CameraOptimizerConfig(mode="shared_SO3xR3", penalty_scale=1.0)
        c.shared_camera_optimizer_thermal = CameraOptimizerConfig(mode="shared_SO3xR3", penalty_scale=10.0)
    return c


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ configuration gate
def test_validate_for_hip_accepts_the_shared_optimisers():
    small_cfg("separate").validate_for_hip()
    small_cfg("shared").validate_for_hip()
    ThermalNerfactoModelConfig().validate_for_hip()  # the default: both switched off by penalty_scale = -1
    c = small_cfg("separate")
    c.shared_camera_optimizer = CameraOptimizerConfig(mode="off")
    c.validate_for_hip()


@pytest.mark.parametrize("name", ["shared_camera_optimizer", "shared_camera_optimizer_thermal"])
@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_other_modes_on_the_shared_optimisers_stay_refused(name, mode):
    c = small_cfg("separate")
    setattr(c, name, CameraOptimizerConfig(mode=mode, penalty_scale=1.0))
    with pytest.raises(NotImplementedError, match=name):
        c.validate_for_hip()


# ------------------------------------------------------------------------------------------------ arena layout
@pytest.mark.parametrize("mode", ["separate", "shared"])
def test_arena_layout_keeps_every_offset_and_appends_the_rows(mode):
    off = ParamArena(small_cfg(mode, shared=False), 8, "cpu")
    on = ParamArena(small_cfg(mode), 8, "cpu")
    new = SHARED_KEYS if mode == "separate" else SHARED_KEYS[:1]
    assert not any(k in off.layout for k in SHARED_KEYS)
    assert list(on.layout)[: len(off.layout)] == list(off.layout) and list(on.layout)[len(off.layout):] == new
    for k, v in off.layout.items():
        assert on.layout[k] == v, k
    assert all(on.layout[k][1] == (1, 6) and on.layout[k][0] >= off.total for k in new)
    groups = ["shared_camera_opt", "shared_camera_opt_thermal"][: len(new)]
    assert on.optimised_groups == off.optimised_groups + groups
    assert off.group_range == {g: r for g, r in on.group_range.items() if g not in groups}
    for g, k in zip(groups, new):
        assert on.group_keys[g] == [k]
    assert on.live_range == (off.live_range[0], on.total)


def test_default_config_arena_layout_is_unchanged():
    """the default configuration (shared optimisers off): the groups, their order and the six-group live range of separate mode"""
    a = ParamArena(small_cfg("separate", shared=False), 8, "cpu")
    assert a.optimised_groups == ["proposal_networks", "fields", "camera_opt", "proposal_networks_thermal", "fields_thermal", "camera_opt_thermal"]
    assert list(a.group_range) == a.optimised_groups and a.live_range == (0, a.total)
    assert list(a.layout)[-1] == "camera_optimizer_thermal.pose_adjustment"


def test_optimiser_table_has_the_two_groups_at_the_camera_rates():
    from nerfstudio_thermal_amd.engine import OPTIMIZERS

    assert OPTIMIZERS["shared_camera_opt"] == OPTIMIZERS["shared_camera_opt_thermal"] == (1e-3, 1e-4, 5000)


# ------------------------------------------------------------------------------------------------ groups, loss keys, metric keys
# (ThermalNerfactoModel itself refuses to be built without a HIP device; its get_param_groups / get_loss_dict / get_metrics_dict are
# checked in tests/test_nerf_shared_pose_gpu.py.  Here: the engine's records on a host arena, which the model's dicts are read from, and the
# CameraOptimizer component.)
@pytest.mark.parametrize("mode", ["separate", "shared"])
def test_engine_records_and_loss_keys(mode):
    from nerfstudio_thermal_amd.engine import RenderEngine

    th = [0, 0, 0, 0, 1, 1, 1, 1]
    cfg = small_cfg(mode)
    arena = ParamArena(cfg, 8, "cpu")
    eng = RenderEngine(cfg, arena, 8, th)
    assert eng.shared_on
    want = {"": ("shared_camera_opt", 13), "_thermal": ("shared_camera_opt_thermal", 14)} if mode == "separate" else {"": ("shared_camera_opt", 13)}
    for sfx, (group, slot) in want.items():
        bn = eng.nets[sfx]
        assert bn.shared.shape == (1, 6) and bn.shared_grad.shape == (1, 6) and bn.g_shared == group and bn.shared_slot == slot
        assert bn.shared.data_ptr() == arena.view(f"shared_camera_optimizer{sfx}.pose_adjustment").data_ptr()
        # the same mask as the per-camera optimiser's: the RGB branch's row is frozen on thermal cameras, the thermal branch's on RGB cameras
        assert bn.frozen.tolist() == ([1 - x for x in th] if sfx else th)
    keys = set(eng._loss_dict(torch.arange(16.0)))
    assert {"camera_opt_regularizer_shared" + sfx for sfx in want} <= keys
    assert ("camera_opt_regularizer_shared_thermal" in keys) == (mode == "separate")
    off = RenderEngine(small_cfg(mode, shared=False), ParamArena(small_cfg(mode, shared=False), 8, "cpu"), 8, th)
    assert not off.shared_on and all(bn.shared is None for bn in off.nets.values())
    assert not any("shared" in k for k in off._loss_dict(torch.arange(16.0)))


def test_camera_optimizer_component_in_shared_mode():
    from nerfstudio_thermal_amd.model_components import CameraOptimizer

    p = torch.nn.Parameter(torch.tensor([[3.0, 0.0, 4.0, 0.0, 0.0, 2.0]]))
    co = CameraOptimizer(CameraOptimizerConfig(mode="shared_SO3xR3", penalty_scale=1.0), 8, "cpu", torch.tensor([4, 5, 6, 7]), pose_param=p,
                         suffix="_shared_thermal")
    assert co.shared and co.pose_adjustment is p and co._frozen.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    groups, metrics = {}, {}
    co.get_param_groups(groups, name="shared_camera_opt_thermal")
    co.get_metrics_dict(metrics)
    assert groups == {"shared_camera_opt_thermal": [p]}
    assert float(metrics["camera_opt_translation_shared_thermal"]) == 5.0 and float(metrics["camera_opt_rotation_shared_thermal"]) == 2.0
    assert dict(co.state_dict()).keys() == {"pose_adjustment"}
    with pytest.raises(AssertionError):  # a shared optimiser owns ONE row
        CameraOptimizer(CameraOptimizerConfig(mode="shared_SO3xR3", penalty_scale=1.0), 8, "cpu", pose_param=torch.nn.Parameter(torch.zeros(8, 6)))
    off = CameraOptimizer(CameraOptimizerConfig(mode="shared_SO3xR3", penalty_scale=-1), 8, "cpu", suffix="_shared")
    groups, metrics = {}, {}
    off.get_param_groups(groups, name="shared_camera_opt")
    off.get_metrics_dict(metrics)
    assert groups == {} and metrics == {} and not hasattr(off, "pose_adjustment")


# ------------------------------------------------------------------------------------------------ host-side validation of the entry points
def test_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    # tn_pose_shared_apply(row, frozen, cam, o_in, d_in, N, C, o_out, d_out, stream)
    assert lib.tn_pose_shared_apply(None, None, None, None, None, 0, 8, None, None, None) == 0  # an empty batch touches nothing
    assert lib.tn_pose_shared_apply(None, None, p, p, p, 4, 8, p, p, None) == -22
    assert b"null pointer" in lib.tn_last_error()
    for bad in [dict(cam=None), dict(o=None), dict(d=None), dict(oo=None), dict(do=None)]:
        a = dict(cam=p, o=p, d=p, oo=p, do=p)
        a.update(bad)
        assert lib.tn_pose_shared_apply(p, None, a["cam"], a["o"], a["d"], 4, 8, a["oo"], a["do"], None) == -22, bad
    for n, c in [(-1, 8), (2**32 + 1, 8), (4, 0), (4, -3), (4, 2**20 + 1)]:
        assert lib.tn_pose_shared_apply(p, None, p, p, p, n, c, p, p, None) == -22, (n, c)
        assert b"bad N" in lib.tn_last_error()
    # tn_pose_shared_bwd(row, frozen, cam, d_in, g_o, g_d, pose, N, C, workspace, workspace_bytes, grad_row, stream)
    need = lib.tn_pose_shared_bwd_workspace_bytes(1027)
    assert need == 5 * 6 * 8 and lib.tn_pose_shared_bwd_workspace_bytes(0) > 0 and lib.tn_pose_shared_bwd_workspace_bytes(-1) == -22
    assert lib.tn_pose_shared_bwd(None, None, None, None, None, None, None, 0, 8, None, 0, None, None) == 0
    assert lib.tn_pose_shared_bwd(None, None, p, p, p, p, None, 4, 8, p, 256, p, None) == -22
    assert b"null pointer" in lib.tn_last_error()
    assert lib.tn_pose_shared_bwd(p, None, p, p, p, p, None, 4, 8, p, 256, None, None) == -22
    assert lib.tn_pose_shared_bwd(p, None, p, p, p, p, None, 4, 8, None, 256, p, None) == -22
    for n, c in [(-1, 8), (2**32 + 1, 8), (4, 0), (4, 2**20 + 1)]:
        assert lib.tn_pose_shared_bwd(p, None, p, p, p, p, None, n, c, p, 1 << 20, p, None) == -22, (n, c)
    assert lib.tn_pose_shared_bwd(p, None, p, p, p, p, None, 1027, 8, p, need - 1, p, None) == -22
    assert b"workspace of" in lib.tn_last_error()


# ------------------------------------------------------------------------------------------------ the restatement
FROZEN = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1], dtype=torch.bool)


def _case(n=37):
    o, d, cam = fn.rays(n, seed=9)
    g = torch.Generator().manual_seed(3)
    return o.double(), d.double(), cam, torch.randn(n, 3, generator=g, dtype=torch.float64), torch.randn(n, 3, generator=g, dtype=torch.float64)


def test_restatement_leaves_frozen_cameras_alone_and_corrects_the_rest():
    o, d, cam, _, _ = _case()
    row = fn.rows()["rig"]
    o1, d1 = fn.shared_apply(row, FROZEN, cam, o, d)
    fz = FROZEN[cam]
    assert torch.equal(o1[fz], o[fz]) and torch.equal(d1[fz], d[fz])
    m = fn.orc.exp_map_so3xr3(row)[0]
    assert torch.allclose(o1[~fz], o[~fz] + m[:, 3]) and torch.allclose(d1[~fz], d[~fz] @ m[:, :3].T)
    assert torch.allclose(d1.norm(dim=-1), d.norm(dim=-1), atol=1e-12)  # a rotation
    z0, z1 = fn.shared_apply(fn.rows()["zero"], FROZEN, cam, o, d)
    assert torch.equal(z0, o) and torch.equal(z1, d)  # the zero row is the identity exactly


@pytest.mark.parametrize("row_name", ["zero", "tiny", "rig"])
@pytest.mark.parametrize("with_pose", [False, True])
def test_restatement_gradient_agrees_with_finite_differences(row_name, with_pose):
    o, d, cam, g_o, g_d = _case()
    row = fn.rows()[row_name]
    pose = 0.2 * torch.randn(8, 6, generator=torch.Generator().manual_seed(1), dtype=torch.float64) if with_pose else None
    grad = fn.row_gradient(row, pose, FROZEN, cam, o, d, g_o, g_d)

    def f(r):
        o2, d2 = fn.composed_apply(r, pose, FROZEN, cam, o, d)
        return float((o2 * g_o).sum() + (d2 * g_d).sum())

    # (theta^2 is clamped at 1e-4, cameras/lie_groups.py:24-58: below it the map is R = I + f1 K + f2 K^2 with constant factors, a quadratic
    # in w, whose central difference is exact up to rounding; above it the step's truncation error is ~h^2)
    h = 1e-6
    for q in range(6):
        e = torch.zeros(1, 6, dtype=torch.float64)
        e[0, q] = h
        num = (f(row + e) - f(row - e)) / (2 * h)
        assert abs(num - float(grad[0, q])) <= 1e-6 * max(1.0, abs(num)), (q, num, float(grad[0, q]))
    fz = FROZEN[cam]
    assert torch.allclose(grad[0, :3], g_o[~fz].sum(0))  # g_t = sum of g_o over the rays that are not frozen


def test_restatement_gradient_pulls_back_through_the_per_camera_rotation():
    """g_w = sum J(row; d0)^T (R_c^T g_d2): the row's gradient with a per-camera pose equals the one without it when g_d is replaced by R_c^T g_d"""
    o, d, cam, g_o, g_d = _case()
    row = fn.rows()["rig"]
    pose = 0.2 * torch.randn(8, 6, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    Rc = fn.orc.exp_map_so3xr3(pose)[cam][:, :, :3]
    pulled = torch.einsum("nij,ni->nj", Rc, g_d)
    a = fn.row_gradient(row, pose, FROZEN, cam, o, d, g_o, g_d)
    b = fn.row_gradient(row, None, FROZEN, cam, o, d, g_o, pulled)
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)


def test_restatement_regulariser_and_its_gradient():
    row = fn.rows()["rig"].clone().requires_grad_(True)
    r = fn.regularizer(row, 1e-2, 1e-3, 10.0)
    want = (row[0, :3].norm() * 1e-2 + row[0, 3:].norm() * 1e-3) * 10.0
    assert torch.allclose(r, want)
    r.backward()
    g = torch.cat([row[0, :3] / row[0, :3].norm() * 1e-2, row[0, 3:] / row[0, 3:].norm() * 1e-3]) * 10.0
    assert torch.allclose(row.grad[0], g.detach())
    assert float(fn.regularizer(fn.rows()["zero"], 1e-2, 1e-3, 10.0)) == 0.0
