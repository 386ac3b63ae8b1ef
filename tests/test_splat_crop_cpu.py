"""The crop box of the splat eval render without a GPU: OrientedBox (from_params, within on CPU tensors, the singular and empty cases), the
C ABI of the box (the projection's nullable crop argument, tn_splat_crop_mask), the model's crop API, and the conditions the GPU tests' scene has to meet so that they may demand exact
keep sets (tests/splat_crop_functional.py)."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import splat_abi
import splat_crop_functional as scf

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib
from nerfstudio_thermal_amd.splat import OrientedBox, ThermalSplatfactoModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_PI = 0.5 * math.pi
# hand-checked: rpy -> R = Rz(yaw) Ry(pitch) Rx(roll)
HAND = [
    ((0.0, 0.0, HALF_PI), [[0, -1, 0], [1, 0, 0], [0, 0, 1]]),      # pure yaw: the box's x axis is world y
    ((0.0, HALF_PI, 0.0), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]),      # pure pitch: the box's x axis is world -z
    ((HALF_PI, 0.0, HALF_PI), [[0, 0, 1], [1, 0, 0], [0, 1, 0]]),   # roll, THEN yaw (Rz Rx; Rx Rz would be [[0,-1,0],[0,0,-1],[1,0,0]])
]


def test_the_package_exports_the_box():
    assert nerfstudio_thermal_amd.OrientedBox is OrientedBox


@pytest.mark.parametrize("rpy,want", HAND, ids=["yaw", "pitch", "roll-then-yaw"])
def test_from_params_hand_checked(rpy, want):
    box = OrientedBox.from_params((1.0, 2.0, 3.0), rpy, (2.0, 4.0, 6.0))
    assert box.R.dtype == torch.float32 and box.R.shape == (3, 3)
    assert float((box.R.double() - torch.tensor(want, dtype=torch.float64)).abs().max()) <= 2.0 ** -24
    assert float((scf.rotation_rpy(*rpy) - torch.tensor(want, dtype=torch.float64)).abs().max()) <= 1e-15
    assert box.T.tolist() == [1.0, 2.0, 3.0] and box.S.tolist() == [2.0, 4.0, 6.0]
    if rpy == HAND[0][0]:  # the box's x axis maps to world y: 1.9 along world y is inside (S_x = 2 would not reach, S_y = 4 is box y = world -x)
        pts = torch.tensor([[1.0, 2.9, 3.0], [1.0, 3.1, 3.0], [2.9, 2.0, 3.0], [-0.9, 2.0, 3.0], [3.1, 2.0, 3.0]])
        assert box.within(pts).tolist() == [True, False, True, True, False]


def test_from_params_random_against_the_float64_product():
    g = torch.Generator().manual_seed(7)
    for _ in range(8):
        rpy = ((torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 2 * math.pi).tolist()
        box = OrientedBox.from_params((0.0, 0.0, 0.0), rpy, (1.0, 1.0, 1.0))
        want = scf.rotation_rpy(*rpy)
        assert float((box.R.double() - want).abs().max()) <= 2.0 ** -24 + 1e-15  # the float64 product rounded to fp32
        assert float((want @ want.T - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-14


def test_within_is_strict_on_both_faces():
    box = OrientedBox(R=scf.EDGE_BOX.R, T=scf.EDGE_BOX.T, S=scf.EDGE_BOX.S)
    assert box.within(scf.EDGE_POINTS).tolist() == scf.EDGE_INSIDE.tolist()
    assert scf.within64(scf.EDGE_BOX, scf.EDGE_POINTS).tolist() == scf.EDGE_INSIDE.tolist()
    x = torch.tensor([[1.0, 0.0, 0.0], [float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))), 0.0, 0.0], [-1.0, 0.0, 0.0]])
    assert box.within(x).tolist() == [False, True, False]
    # float64 points take the same rule in their own precision
    x64 = torch.tensor([[1.0, 0.0, 0.0], [math.nextafter(1.0, 0.0), 0.0, 0.0], [-1.0, 0.0, 0.0]], dtype=torch.float64)
    assert box.within(x64).tolist() == [False, True, False]
    assert box.within(torch.zeros(0, 3)).shape == (0,)
    with pytest.raises(ValueError):
        box.within(torch.zeros(4, 2))


@pytest.mark.parametrize("name", ["rotated", "sheared"])
def test_within_on_rotated_translated_and_sheared_boxes(name):
    g = torch.Generator().manual_seed(11)
    if name == "rotated":
        box = OrientedBox.from_params((0.3, -0.2, 0.5), (0.4, -0.7, 1.1), (1.0, 0.6, 1.4))
    else:  # an invertible R that is no rotation: sheared and scaled columns
        box = OrientedBox(R=torch.tensor([[1.0, 0.4, 0.0], [0.0, 1.3, -0.5], [0.2, 0.0, 0.8]]), T=torch.tensor([-0.1, 0.2, 0.0]), S=torch.tensor([1.0, 0.7, 1.2]))
    pts = ((torch.rand(4000, 3, generator=g) - 0.5) * 2.0).contiguous()
    ref = scf.within64(box, pts)
    near = scf.near_boundary(box, pts)
    got = box.within(pts)
    assert got.dtype == torch.bool and got.shape == (4000,)
    assert 200 < int(ref.sum()) < 3800  # both sides of the box are exercised
    assert torch.equal(got[~near], ref[~near]) and int(near.sum()) < 8
    # the definition itself: a point inside is R q + T with |q_i| < S_i / 2
    q = (torch.rand(500, 3, generator=g, dtype=torch.float64) - 0.5) * box.S.double() * 0.999
    assert bool(box.within((q @ box.R.double().T + box.T.double()).float()).all())
    q_out = q.clone()
    q_out[:, 1] = 0.5 * float(box.S[1]) * 1.001
    assert not bool(box.within((q_out @ box.R.double().T + box.T.double()).float()).any())


def test_a_singular_box_is_refused_and_an_empty_one_keeps_nothing():
    pts = torch.zeros(5, 3)
    for R in (torch.zeros(3, 3), torch.tensor([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 1.0, 0.0]])):
        with pytest.raises(ValueError, match="singular"):
            OrientedBox(R=R, T=torch.zeros(3), S=torch.ones(3)).within(pts)
        with pytest.raises(ValueError, match="singular"):
            OrientedBox(R=R, T=torch.zeros(3), S=torch.ones(3)).crop_struct()
    for S in ([1.0, 0.0, 1.0], [1.0, 1.0, -2.0], [0.0, 0.0, 0.0]):
        assert not bool(OrientedBox(R=torch.eye(3), T=torch.zeros(3), S=torch.tensor(S)).within(pts).any())
        assert not bool(scf.within64(scf.Box(torch.eye(3), torch.zeros(3), torch.tensor(S)), pts).any())
    assert bool(OrientedBox(R=torch.eye(3), T=torch.zeros(3), S=torch.ones(3)).within(pts).all())


def test_the_world_to_box_matrix_is_the_float64_inverse_rounded_once():
    box = OrientedBox.from_params((0.3, -0.2, 0.5), (0.4, -0.7, 1.1), (1.0, 0.6, 1.4))
    m = box.world_to_box()
    assert m.dtype == torch.float32 and m.shape == (3, 4) and torch.equal(m, scf.world_to_box(box))
    c = box.crop_struct()
    assert list(c.world_to_box) == m.reshape(-1).tolist() and list(c.half_extent) == [0.5, 0.30000001192092896, 0.699999988079071]


def _declaration(hdr: str, name: str) -> str:
    m = re.search(r"TN_API\s+int\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m, name
    return m.group(1)


def test_the_header_declares_the_crop_entry_points_and_the_binding_matches():
    hdr = open(os.path.join(ROOT, "include", "thermal_nerf_hip.h")).read()
    args = [" ".join(a.split()) for a in _declaration(hdr, "tn_splat_project").split(",")]
    # the box is the projection's last argument before the stream, and the binding's type there is the struct pointer
    assert args[-2:] == ["const TnSplatCrop* crop", "tn_stream_t stream"] and args[:2] == ["const TnSplatCamera* camera", "const float* pose_camera"]
    res, argtypes = _lib.SIGNATURES["tn_splat_project"]
    assert res is C.c_int and len(argtypes) == len(args) and argtypes[-2] is C.POINTER(_lib.TnSplatCrop)
    for name in splat_abi.RETIRED:
        assert not re.search(r"\b%s\s*\(" % name, hdr) and name not in _lib.SIGNATURES, name
    mask_args = _declaration(hdr, "tn_splat_crop_mask").split(",")
    assert [" ".join(a.split()) for a in mask_args] == ["const TnSplatCrop* crop", "const float* means", "int64_t n", "uint8_t* mask", "tn_stream_t stream"]
    assert len(_lib.SIGNATURES["tn_splat_crop_mask"][1]) == 5 and _lib.SIGNATURES["tn_splat_crop_mask"][1][2] is C.c_int64
    assert _lib.ABI_VERSION == 314
    body = hdr[hdr.index("typedef struct TnSplatCrop {"):hdr.index("} TnSplatCrop;")]
    assert re.findall(r"float\s+(\w+)\[(\d+)\]", body) == [("world_to_box", "12"), ("half_extent", "3")]
    assert [(n, t._length_) for n, t in _lib.TnSplatCrop._fields_] == [("world_to_box", 12), ("half_extent", 3)] and C.sizeof(_lib.TnSplatCrop) == 60


def test_the_library_refuses_bad_crop_arguments_before_any_launch():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    lib = _lib.load()
    crop = OrientedBox.from_params((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)).crop_struct()
    assert lib.tn_splat_crop_mask(None, None, 4, None, None) == -22 and b"null crop box" in lib.tn_last_error()
    assert lib.tn_splat_crop_mask(C.byref(crop), None, 4, None, None) == -22 and b"null pointer" in lib.tn_last_error()
    assert lib.tn_splat_crop_mask(C.byref(crop), None, -1, None, None) == -22
    assert lib.tn_splat_crop_mask(C.byref(crop), None, 0, None, None) == 0
    cam = _lib.TnSplatCamera(fx=10.0, fy=10.0, width=16, height=16)
    # (a null box of the projection is no refusal any more: it is the uncropped frame)
    none = [None] * 8
    for oth in (None, C.c_void_p(256)):
        assert lib.tn_splat_project(C.byref(cam), None, *none, oth, 4, 0, 0, 0, *[None] * 8, 0, C.byref(crop), None) == -22
        assert b"tn_splat_project: null pointer" in lib.tn_last_error()
    assert lib.tn_version() == 314


class _Bare(ThermalSplatfactoModel):
    """The model's crop API without a device: no Gaussians, and get_outputs reports the box it would crop to."""

    def __init__(self):
        torch.nn.Module.__init__(self)
        self.crop_box = None

    def get_outputs(self, camera):
        return {"camera": camera, "box": self.crop_box, "struct": self._crop()}


def test_the_model_has_the_reference_crop_api():
    m = _Bare()
    box = OrientedBox.from_params((0.0, 0.1, 0.2), (0.1, 0.2, 0.3), (1.0, 2.0, 3.0))
    assert m.crop_box is None and m._crop() is None
    out = m.get_outputs_for_camera("cam", box)
    assert out["camera"] == "cam" and out["box"] is box and list(out["struct"].half_extent) == [0.5, 1.0, 1.5]
    assert m.crop_box is box
    out = m.get_outputs_for_camera("cam", None)  # as in the reference, None clears an earlier crop
    assert out["box"] is None and out["struct"] is None and m.crop_box is None
    m.set_crop(box)
    assert m.get_outputs_for_camera("cam")["box"] is None
    m.crop_box = box  # assigned directly, as the reference's viewer does
    assert list(m._crop().world_to_box) == box.world_to_box().reshape(-1).tolist()
    first = m._crop()
    box.S.mul_(2.0)  # written in place: the next frame reads the box anew
    assert list(m._crop().half_extent) == [1.0, 2.0, 3.0] and list(first.half_extent) == [0.5, 1.0, 1.5]
    box.T = torch.tensor([1.0, 0.0, 0.0])  # a new tensor
    assert list(m._crop().world_to_box) == box.world_to_box().reshape(-1).tolist() and m._crop().world_to_box[3] != first.world_to_box[3]
    box.R = [[2.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]  # a list, as OrientedBox accepts; changed in place below
    assert m._crop().world_to_box[0] == 0.5
    box.R[0][0] = 4.0
    assert m._crop().world_to_box[0] == 0.25
    assert "crop_box" not in m.state_dict() and not list(m.parameters()) and not list(m.buffers())
    with pytest.raises(TypeError):
        m.set_crop("box")
    m.set_crop(OrientedBox(R=torch.zeros(3, 3), T=torch.zeros(3), S=torch.ones(3)))
    with pytest.raises(ValueError, match="singular"):  # the frame's error, before any launch
        m.get_outputs_for_camera("cam", m.crop_box)


@pytest.mark.parametrize("sh", [0, 3])
def test_the_gpu_scene_meets_its_conditions(sh):
    """Nothing near a face of any box the GPU tests use (so fp32 and float64 keep the same Gaussians), and the block layout the kernel's
    block-wide vote is tested on."""
    p = scf.crop_scene(0, sh)
    means = p["means"]
    assert means.shape == (scf.N_SCENE, 3) and means.dtype == torch.float32 and p["features_rest"].shape[1] == (sh + 1) ** 2 - 1
    for box in (scf.MAIN_BOX, scf.SECOND_BOX, scf.EVERYTHING_BOX, scf.NOTHING_BOX):
        assert int(scf.near_boundary(box, means).sum()) == 0
        obox = OrientedBox(R=box.R, T=box.T, S=box.S)
        assert torch.equal(obox.within(means), scf.within64(box, means))
    b0, b1, b2 = scf.BLOCKS
    main, second = scf.within64(scf.MAIN_BOX, means), scf.within64(scf.SECOND_BOX, means)
    assert not bool(main[b0].any()) and bool(main[b2].all()) and 20 < int(main[b1].sum()) < 108
    assert bool(second[b0].all()) and not bool(second[b2].any()) and 10 < int(second[b1].sum()) < 118
    assert bool(scf.within64(scf.EVERYTHING_BOX, means).all()) and not bool(scf.within64(scf.NOTHING_BOX, means).any())
    assert int(scf.near_boundary(scf.EDGE_BOX, scf.EDGE_POINTS).sum()) >= 6  # the edge points ARE on the faces: exactness there is by construction
