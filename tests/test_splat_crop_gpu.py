"""The crop box of the splat eval render on the GPU: tn_splat_crop_mask, OrientedBox.within on device tensors and the cropped
ThermalSplatfactoModel.get_outputs (tn_splat_project with its crop box; under a shared pose row with the pose record too).

Everything here is exact.  The scene (scf.crop_scene: 300 Gaussians = projection blocks of 128, 128 and 44; frame 96 x 72 = 6 x 4.5 tiles) has no
mean within the rounding band of a face of any box used (tests/test_splat_crop_cpu.py checks that on the inputs), so the kernel must keep exactly
the Gaussians the float64 restatement keeps; and a kept Gaussian goes through the same arithmetic as without the box, a dropped one leaves like
one behind the camera, so the cropped frame must equal, bit for bit and on every output key, the frame of a model that holds only the kept
Gaussians and runs the entry points without a box.  For MAIN_BOX block 0 is entirely outside (its SH slab is never staged), block 1 mixed,
block 2 (the ragged one) entirely inside; SECOND_BOX is the reverse."""
import ctypes as C
import functools

import pytest
import torch

import splat_crop_functional as scf
import splat_functional as sf
import splat_oracle as so
import splat_pose_functional as spf
import splat_sep_functional as ssf

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOXES = {"main": scf.MAIN_BOX, "second": scf.SECOND_BOX}
SHARED_KEYS = {"rgb", "thermal", "depth", "accumulation", "background", "background_thermal"}
SEP_KEYS = SHARED_KEYS | {"accumulation_thermal"}
REMOVAL_KEYS = {"removal", "removal_thermal"}


def _splat():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import splat

    return splat


def _obox(box):
    return _splat().OrientedBox(R=box.R, T=box.T, S=box.S)


@functools.lru_cache(maxsize=None)
def _scene(sh_degree):
    return scf.crop_scene(0, sh_degree)


def _params(sh_degree, mode):
    p = _scene(sh_degree)
    return p if mode == "separate" else ssf.shared_params(p)


def _model(params, mode, raster, sh_degree, step, thr=None, **kw):
    splat = _splat()
    cfg = splat.ThermalSplatfactoModelConfig(sh_degree=sh_degree, sh_degree_interval=1, rasterize_mode=raster, background_thermal=0.3,
                                             thermal_opacity_mode=mode, removal_min_opacity_diff=thr, **kw)
    m = splat.ThermalSplatfactoModel(cfg, num_points=4, device=DEV)
    m.load_gaussians(params)
    m.step = step
    m.eval()
    return m


def _camera():
    c2w, fx = so.look_at_camera((2.3, 0.4, 0.6)), sf.fov_focal(scf.W)
    return _splat().PinholeCamera(c2w, fx, fx, scf.W / 2 - 0.5, scf.H / 2 + 0.25, scf.W, scf.H)


def _keys(mode, thr):
    return (SEP_KEYS if mode == "separate" else SHARED_KEYS) | (REMOVAL_KEYS if thr is not None else set())


def _assert_same_frame(got, want, keys):
    assert set(got) == set(want) == keys, (set(got) ^ keys, set(want) ^ keys)
    for k in sorted(keys):
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))


def _mask(box, pts):
    """tn_splat_crop_mask through the C ABI."""
    from nerfstudio_thermal_amd import _lib

    crop = _obox(box).crop_struct()
    out = torch.full((pts.shape[0],), 7, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().tn_splat_crop_mask(C.byref(crop), C.c_void_p(pts.data_ptr()), pts.shape[0], C.c_void_p(out.data_ptr()), None), "tn_splat_crop_mask")
    torch.cuda.synchronize()
    return out.cpu()


def test_crop_mask_equals_the_float64_restatement_exactly():
    means = _scene(3)["means"]
    for box in (scf.MAIN_BOX, scf.SECOND_BOX, scf.EVERYTHING_BOX, scf.NOTHING_BOX):
        got = _mask(box, means.to(DEV))
        assert set(got.unique().tolist()) <= {0, 1}
        assert torch.equal(got.bool(), scf.within64(box, means))
    # on a face is out, one ulp inside is in
    assert _mask(scf.EDGE_BOX, scf.EDGE_POINTS.to(DEV)).bool().tolist() == scf.EDGE_INSIDE.tolist()
    # more than one block of 256, ragged, against the band-free part of a random cloud
    g = torch.Generator().manual_seed(5)
    pts = ((torch.rand(1000, 3, generator=g) - 0.5) * 3.0).contiguous()
    near = scf.near_boundary(scf.MAIN_BOX, pts)
    got = _mask(scf.MAIN_BOX, pts.to(DEV)).bool()
    assert torch.equal(got[~near], scf.within64(scf.MAIN_BOX, pts)[~near]) and int(near.sum()) < 4 and 10 < int(got.sum()) < 990


def test_within_on_a_device_tensor_is_the_same_mask():
    means = _scene(3)["means"]
    for box in (scf.MAIN_BOX, scf.SECOND_BOX, scf.NOTHING_BOX):
        got = _obox(box).within(means.to(DEV))
        assert got.dtype == torch.bool and got.is_cuda and got.shape == (scf.N_SCENE,)
        assert torch.equal(got.cpu(), scf.within64(box, means)) and torch.equal(got.cpu(), _mask(box, means.to(DEV)).bool())
        assert torch.equal(_obox(box).within(means.to(DEV).double()).cpu(), scf.within64(box, means))  # not fp32: the torch rule, on the device
    assert _obox(scf.EDGE_BOX).within(scf.EDGE_POINTS.to(DEV)).cpu().tolist() == scf.EDGE_INSIDE.tolist()
    assert _obox(scf.MAIN_BOX).within(torch.zeros(0, 3, device=DEV)).shape == (0,)
    # a strided view is made contiguous, not misread
    wide = torch.cat([means, torch.full((scf.N_SCENE, 1), 9.0)], 1).to(DEV)
    assert torch.equal(_obox(scf.MAIN_BOX).within(wide[:, :3]).cpu(), scf.within64(scf.MAIN_BOX, means))


# (thermal_opacity_mode, removal threshold): separate mode runs with and without the removal renders
MODES = [("shared", None), ("separate", None), ("separate", scf.THR)]
# (config.sh_degree, step) -> degree evaluated: -1 (sigmoid colours, no higher-order coefficients), 0 (coefficients present, none evaluated, none staged), 3
DEGREES = [(0, 10**6), (3, 0), (3, 10**6)]


@pytest.mark.parametrize("box_name", ["main", "second"])
@pytest.mark.parametrize("sh_degree,step", DEGREES, ids=["deg-1", "deg0", "deg3"])
@pytest.mark.parametrize("raster", ["classic", "antialiased"])
@pytest.mark.parametrize("mode,thr", MODES, ids=["shared", "separate", "separate-removal"])
def test_cropped_render_is_the_render_of_the_kept_gaussians(mode, thr, raster, sh_degree, step, box_name):
    box = BOXES[box_name]
    p = _params(sh_degree, mode)
    keep = scf.within64(box, p["means"])
    cam = _camera()
    m = _model(p, mode, raster, sh_degree, step, thr)
    assert m._frame_settings()[1] == {(0, 10**6): -1, (3, 0): 0, (3, 10**6): 3}[(sh_degree, step)]
    got = m.get_outputs_for_camera(cam, _obox(box))
    sub = _model(scf.subset(p, keep), mode, raster, sh_degree, step, thr)
    want = sub.get_outputs(cam)
    assert sub.crop_box is None and 40 < int(keep.sum()) < 260
    _assert_same_frame(got, want, _keys(mode, thr))
    assert m.last_num_intersections == sub.last_num_intersections > 0
    assert float(got["accumulation"].max()) > 0.5 and float((got["rgb"] - got["background"]).abs().max()) > 0.1  # a frame, not the background
    # the projection: radius 0 exactly at the cropped-out Gaussians, the kept ones as the subset model projected them
    for k, v in m.last_projection.items():
        assert torch.equal(v[keep.to(DEV)], sub.last_projection[k]), k
        assert not bool(v[~keep.to(DEV)].any()), k
    assert bool((m.last_projection["radii"][keep.to(DEV)] > 0).any())


@pytest.mark.parametrize("mode,thr", [("shared", None), ("separate", scf.THR)], ids=["shared", "separate-removal"])
def test_cropped_render_under_a_shared_pose_row(mode, thr):
    """The pose instantiation of the projection with a non-null box (tn_splat_project with pose_camera and crop): an eval render under a shared pose row
    with the crop set equals, bit for bit, the render of the kept Gaussians under the same row.  The box test is on world-space means, so the
    pose does not change which Gaussians are kept."""
    from nerfstudio_thermal_amd.config import CameraOptimizerConfig

    p = _params(3, mode)
    keep = scf.within64(scf.MAIN_BOX, p["means"])
    cam = _camera()

    def posed(params, row):
        m = _model(params, mode, "classic", 3, 10**6, thr, camera_optimizer=CameraOptimizerConfig(mode="shared_SO3xR3"))
        with torch.no_grad():
            m.camera_optimizer.pose_adjustment[0] = row.float().to(DEV)
        return m

    m = posed(p, spf.pose_row("moved"))
    got = m.get_outputs_for_camera(cam, _obox(scf.MAIN_BOX))
    sub = posed(scf.subset(p, keep), spf.pose_row("moved"))
    want = sub.get_outputs(cam)
    assert sub.crop_box is None and 40 < int(keep.sum()) < 260
    _assert_same_frame(got, want, _keys(mode, thr))
    assert m.last_num_intersections == sub.last_num_intersections > 0
    for k, v in m.last_projection.items():
        assert torch.equal(v[keep.to(DEV)], sub.last_projection[k]), k
        assert not bool(v[~keep.to(DEV)].any()), k
    still = posed(p, torch.zeros(6)).get_outputs_for_camera(cam, _obox(scf.MAIN_BOX))  # a zero row: the uncorrected camera, another frame
    assert not torch.equal(still["rgb"], got["rgb"]) and not torch.equal(still["thermal"], got["thermal"])


@pytest.mark.parametrize("mode,thr", MODES, ids=["shared", "separate", "separate-removal"])
@pytest.mark.parametrize("raster", ["classic", "antialiased"])
def test_radii_against_the_uncropped_projection(mode, thr, raster):
    p = _params(3, mode)
    cam = _camera()
    m = _model(p, mode, raster, 3, 10**6, thr)
    full = m.get_outputs(cam)
    full_proj = {k: v.clone() for k, v in m.last_projection.items()}
    keep = scf.within64(scf.MAIN_BOX, p["means"]).to(DEV)
    m.get_outputs_for_camera(cam, _obox(scf.MAIN_BOX))
    radii = m.last_projection["radii"]
    assert not bool(radii[~keep].any()) and torch.equal(radii[keep], full_proj["radii"][keep]) and bool((full_proj["radii"][~keep] > 0).any())
    for k in ("xys", "depths", "conics", "compensation", "num_tiles_hit", "tile_box"):
        assert torch.equal(m.last_projection[k][keep], full_proj[k][keep]), k
    # and get_outputs_for_camera without a box clears the crop: the uncropped frame again
    again = m.get_outputs_for_camera(cam)
    assert m.crop_box is None
    _assert_same_frame(again, full, _keys(mode, thr))
    assert torch.equal(m.last_projection["radii"], full_proj["radii"])


@pytest.mark.parametrize("mode,thr", MODES, ids=["shared", "separate", "separate-removal"])
@pytest.mark.parametrize("raster", ["classic", "antialiased"])
def test_a_box_of_everything_and_a_box_of_nothing(mode, thr, raster):
    p = _params(3, mode)
    cam = _camera()
    m = _model(p, mode, raster, 3, 10**6, thr, background_color="white")
    full = m.get_outputs(cam)
    _assert_same_frame(m.get_outputs_for_camera(cam, _obox(scf.EVERYTHING_BOX)), full, _keys(mode, thr))
    nothing = m.get_outputs_for_camera(cam, _obox(scf.NOTHING_BOX))
    assert set(nothing) == _keys(mode, thr) and m.last_num_intersections == 0
    assert not bool(m.last_projection["radii"].any())
    H, W = scf.H, scf.W
    assert torch.equal(nothing["rgb"], nothing["background"].expand(H, W, 3)) and torch.equal(nothing["thermal"], nothing["background_thermal"].expand(H, W, 1))
    assert torch.equal(nothing["accumulation"], torch.zeros(H, W, 1, device=DEV)) and torch.equal(nothing["depth"], torch.full((H, W, 1), 10.0, device=DEV))
    if mode == "separate":
        assert torch.equal(nothing["accumulation_thermal"], torch.zeros(H, W, 1, device=DEV))
    if thr is not None:
        assert torch.equal(nothing["removal"], nothing["rgb"]) and torch.equal(nothing["removal_thermal"], nothing["thermal"])
    # an S with a zero keeps nothing either
    flat = _splat().OrientedBox(R=scf.MAIN_BOX.R, T=scf.MAIN_BOX.T, S=torch.tensor([0.8, 0.0, 0.9]))
    _assert_same_frame(m.get_outputs_for_camera(cam, flat), nothing, _keys(mode, thr))


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_the_training_render_never_crops(mode):
    p = _params(3, mode)
    cam = _camera()
    weight = torch.rand(scf.H, scf.W, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(3))

    def run(box):
        m = _model(p, mode, "classic", 3, 10**6)
        m.train()
        m.set_crop(box)
        out = m.get_train_outputs(cam)
        loss = (out["rgb"] * weight).sum() + (out["thermal"] ** 2).sum() + out["accumulation"].sum()
        if mode == "separate":
            loss = loss + 0.5 * out["accumulation_thermal"].sum()
        loss.backward()
        return out, {k: v.grad.clone() for k, v in m.gauss_params.items()}, m.last_radii.clone(), m.last_xys_grad.clone()

    out_c, grads_c, radii_c, xg_c = run(_obox(scf.MAIN_BOX))
    out_n, grads_n, radii_n, xg_n = run(None)
    assert set(out_c) == set(out_n)
    for k in out_n:
        assert torch.equal(out_c[k].detach(), out_n[k].detach()), k
    assert set(grads_c) == set(grads_n) == set(p)
    for k in grads_n:
        assert torch.equal(grads_c[k], grads_n[k]), k
    keep = scf.within64(scf.MAIN_BOX, p["means"]).to(DEV)
    assert torch.equal(radii_c, radii_n) and torch.equal(xg_c, xg_n) and bool((radii_c[~keep] > 0).any())
    assert float(grads_c["means"][~keep].abs().max()) > 0.0  # the Gaussians outside the box do take gradient


@pytest.mark.parametrize("mode,thr", MODES, ids=["shared", "separate", "separate-removal"])
def test_no_gaussians_with_a_crop_is_the_background(mode, thr):
    p = scf.subset(_params(3, mode), torch.zeros(scf.N_SCENE, dtype=torch.bool))
    m = _model(p, mode, "classic", 3, 10**6, thr)
    assert m.num_points == 0
    out = m.get_outputs_for_camera(_camera(), _obox(scf.MAIN_BOX))
    assert set(out) == _keys(mode, thr)
    assert torch.equal(out["rgb"], out["background"].expand(scf.H, scf.W, 3)) and torch.equal(out["thermal"], out["background_thermal"].expand(scf.H, scf.W, 1))
    assert not bool(out["accumulation"].any())
    assert _obox(scf.MAIN_BOX).within(m.means).shape == (0,)
