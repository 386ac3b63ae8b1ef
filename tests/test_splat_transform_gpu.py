"""Moving thermal splats by a similarity on the GPU: tn_transform_splat against its float64 restatement (tests/splat_transform_functional.py) bit
for bit, `transform_gaussians` / `transform_model`, the render invariance of ThermalSplatfactoModel under a move of model and camera, and the
export / import of splat files in a moved frame.

The render bound is 8 x the CPU oracle's own float32 difference between the two frames of the same scene and move (stf.oracle_floor, computed here
and shared between the cases): 8 x is the project's margin over a float32 floor.  A blend that sits on the 1/255 cut-off or on the 1e-4 stop may
fall differently in the two frames, so at most 7 of the 6 912 pixels (0.1 %) may exceed the bound, and those by no more than 2/255."""
import ctypes as C

import pytest
import torch

import splat_export_functional as sxf
import splat_transform_functional as stf

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 12345.0
F64 = torch.float64
CROP = ((-0.04, 0.06, 0.0), (0.3, -0.2, 0.5), (0.8, 0.7, 0.9))  # every mean of stf.scene() is 2e-3 or more from its faces (asserted below)


def _pkg():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import splat, splat_calls, splat_io, splat_transform

    return splat, splat_calls, splat_io, splat_transform


def make_fields(scale, R, t):
    st = _pkg()[3]
    return stf.fields(scale, R, t, st.rotation_quaternion(R), st.sh_rotation_matrices(R))


def _similarity(scale=0.4):
    return _pkg()[3].Similarity(scale, stf.seeded_rotation()[0], torch.tensor(stf.T_VEC, dtype=F64))


def _fields_of(T):
    return make_fields(T.scale, T.R, T.t)


def _padded(t, shift):
    """`t` on the device with GUARD rows behind it; shift = 1 puts it one float off the allocation's alignment (the kernel's one-float-a-lane path)."""
    flat = torch.full((t.numel() + 64 + shift,), GUARD, device=DEV)
    view = flat[shift:shift + t.numel()].view(t.shape)
    view.copy_(t)
    return flat, view


def _run(p, T, in_place=False, shift=0):
    """transform_call of the host parameters `p` -> (the five outputs on the host, whether every guard word survived)."""
    _, splat_calls, _, st = _pkg()
    src = [_padded(p[k], shift) for k in stf.MOVED]
    dst = src if in_place else [_padded(torch.full_like(p[k], GUARD), shift) for k in stf.MOVED]
    splat_calls.transform_call(st.transform_struct(T), *[v for _, v in src], *[v for _, v in dst])
    torch.cuda.synchronize()
    guards = all(bool((f[:shift] == GUARD).all()) and bool((f[shift + v.numel():] == GUARD).all()) for f, v in src + dst)
    if not in_place:  # the inputs are left alone
        guards = guards and all(torch.equal(stf.bits(v.cpu()), stf.bits(p[k])) for (_, v), k in zip(src, stf.MOVED))
    return {k: v.cpu() for k, (_, v) in zip(stf.MOVED, dst)}, guards


def _assert_bits(got, want, what):
    """Bit-equal, except that a NaN matches any NaN: the sign and payload of a NaN that arithmetic produced are not defined by IEEE 754 (the host's
    and the device's differ), every other value -- the infinities included -- has one encoding."""
    for k in stf.MOVED:
        assert got[k].shape == want[k].shape, (what, k)
        same = (stf.bits(got[k]) == stf.bits(want[k])) | (torch.isnan(got[k]) & torch.isnan(want[k]))
        assert bool(same.all()), (what, k, int((~same).sum()))


# ---------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("R", [0, 3, 8, 15])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 255, 256, 257, 1000])
def test_the_kernel_equals_the_restatement_bit_for_bit(n, R):
    """One Gaussian, a partial tile, an exact tile, a tile plus one (a tile is 128 Gaussians; 255 / 256 / 257 are two tiles' edges), several tiles;
    out of place, in place, a second run, and pointers one float off 16-byte alignment."""
    T = _similarity(0.4)
    p = sxf.random_params(n, R + 1, False, seed=n + R)
    want = stf.transform_ref(_fields_of(T), p)
    got, guards = _run(p, T)
    assert guards
    _assert_bits(got, want, "out of place")
    again, _ = _run(p, T)
    _assert_bits(again, got, "second run")
    inp, guards = _run(p, T, in_place=True)
    assert guards
    _assert_bits(inp, want, "in place")
    off, guards = _run(p, T, shift=1)
    assert guards
    _assert_bits(off, want, "unaligned")
    off, guards = _run(p, T, in_place=True, shift=1)
    assert guards
    _assert_bits(off, want, "unaligned, in place")


def test_no_gaussians_and_refused_arguments_launch_nothing():
    _, splat_calls, _, st = _pkg()
    from nerfstudio_thermal_amd import _lib

    lib = _lib.load()
    T = _similarity()
    s = st.transform_struct(T)
    p = sxf.random_params(4, 16, False, seed=1)
    bufs = [_padded(p[k], 0) for k in stf.MOVED]
    ptrs = [C.c_void_p(v.data_ptr()) for _, v in bufs]
    call = lambda tr, ins, n, R, outs: lib.tn_transform_splat(tr, *ins, n, R, *outs, None)  # noqa: E731
    assert call(None, ptrs, 4, 15, ptrs) == -22
    assert call(C.byref(s), ptrs, -1, 15, ptrs) == -22
    for R in (1, 7, 16, 24):
        assert call(C.byref(s), ptrs, 4, R, ptrs) == -22
    assert call(C.byref(s), [None] + ptrs[1:], 4, 15, ptrs) == -22
    assert call(C.byref(s), ptrs, 4, 15, ptrs[:3] + [None, ptrs[4]]) == -22
    assert call(C.byref(s), ptrs, 0, 15, ptrs) == 0
    torch.cuda.synchronize()
    for (flat, v), k in zip(bufs, stf.MOVED):  # nothing was written
        assert torch.equal(stf.bits(v.cpu()), stf.bits(p[k])) and bool((flat[v.numel():] == GUARD).all())
    empty = {k: v[:0] for k, v in p.items()}
    got, _ = _run(empty, T)
    assert all(got[k].shape == empty[k].shape for k in stf.MOVED)
    moved = st.transform_gaussians({k: v.to(DEV) for k, v in empty.items()}, T)
    assert moved["means"].shape == (0, 3) and moved["features_dc"].shape == (0, 3)


def test_a_value_that_is_not_finite_stays_in_its_gaussian_and_its_group():
    n = 300
    T = _similarity(0.4)
    clean = sxf.random_params(n, 16, False, seed=9)
    base, _ = _run(clean, T)
    p = {k: v.clone() for k, v in clean.items()}
    p["means"][5, 1] = float("nan")
    p["features_rest"][140, 9, 1] = float("inf")  # band 3, channel 1
    p["features_rest_thermal"][140, 1, 0] = float("-inf")  # band 1
    p["quats"][299, 2] = float("nan")
    want = stf.transform_ref(_fields_of(T), p)
    for in_place in (False, True):
        got, _ = _run(p, T, in_place=in_place)
        _assert_bits(got, want, in_place)
        assert not bool(torch.isfinite(got["means"][5]).any()) and not bool(torch.isfinite(got["quats"][299]).any())
        assert not bool(torch.isfinite(got["features_rest"][140, 8:15, 1]).any()) and not bool(torch.isfinite(got["features_rest_thermal"][140, 0:3, 0]).any())
        for k in stf.MOVED:  # every other value is what the clean run gave
            same = stf.bits(got[k]) == stf.bits(base[k])
            flat = same.reshape(n, -1)
            touched = {"means": [5], "quats": [299], "features_rest": [140], "features_rest_thermal": [140], "scales": []}[k]
            keep = torch.ones(n, dtype=torch.bool)
            keep[touched] = False
            assert bool(flat[keep].all()), k
            assert bool(torch.isfinite(got[k].reshape(n, -1)[keep]).all()), k
        assert bool(torch.isfinite(got["features_rest"][140, :8]).all()) and bool(torch.isfinite(got["features_rest"][140, 8:, 0]).all())
        assert bool(torch.isfinite(got["features_rest_thermal"][140, 3:]).all())


# ---------------------------------------------------------------------------------------------------- 2. the package layer
def _model(params, mode="shared", sh_degree=3, step=10**6, raster="classic"):
    splat = _pkg()[0]
    cfg = splat.ThermalSplatfactoModelConfig(sh_degree=sh_degree, sh_degree_interval=1, rasterize_mode=raster, background_thermal=0.0,
                                             background_color="black", thermal_opacity_mode=mode)
    m = splat.ThermalSplatfactoModel(cfg, num_points=4, device=DEV)
    m.load_gaussians(params)
    m.step = step
    m.eval()
    return m


def _params(sh_degree=3, mode="shared"):
    p = stf.scene(sh_degree)
    return dict(p) if mode == "separate" else {k: v for k, v in p.items() if k != "opacities_thermal"}


def _camera():
    return _pkg()[0].PinholeCamera(stf.camera_c2w(), stf.FX, stf.FX, stf.W / 2, stf.H / 2, stf.W, stf.H)


def test_transform_gaussians_returns_new_moved_tensors_and_the_others_as_they_are():
    st = _pkg()[3]
    T = _similarity(2.5)
    host = _params(3, "separate")
    p = {k: v.to(DEV) for k, v in host.items()}
    same = st.transform_gaussians(p, st.Similarity.identity())
    assert set(same) == set(p) and all(same[k] is p[k] for k in p)  # no launch, the inputs themselves
    out = st.transform_gaussians(p, T)
    want = stf.transform_ref(_fields_of(T), host)
    assert set(out) == set(p)
    for k in p:
        if k in stf.MOVED:
            assert out[k] is not p[k] and torch.equal(stf.bits(out[k].cpu()), stf.bits(want[k])) and torch.equal(p[k].cpu(), host[k]), k
        else:
            assert out[k] is p[k], k
    assert torch.equal(stf.bits(out["means"]), stf.bits(T.apply_points(p["means"])))  # apply_points evaluates the means' rule
    q = {k: v.clone() for k, v in p.items()}
    back = st.transform_gaussians(q, T, out=q)  # in place
    assert all(back[k] is q[k] for k in q)
    for k in stf.MOVED:
        assert torch.equal(stf.bits(q[k].cpu()), stf.bits(want[k])), k


def test_identity_and_no_transform_write_the_same_file(tmp_path):
    _, _, splat_io, st = _pkg()
    m = _model(_params(3, "separate"), "separate")
    a = splat_io.export_gaussian_ply(m, str(tmp_path / "a.ply"))
    b = splat_io.export_gaussian_ply(m, str(tmp_path / "b.ply"), transform=st.Similarity.identity())
    assert a["frame"] == "model" and b["frame"] == "transformed" and a["exported"] == b["exported"] == stf.N_SCENE
    assert open(a["path"], "rb").read() == open(b["path"], "rb").read()


# ---------------------------------------------------------------------------------------------------- 3. render invariance on the device
IMAGES = ("rgb", "thermal", "accumulation", "accumulation_thermal")


def _compare_frames(want, got, scale, floor, what):
    """`got` (moved model, moved camera) against `want`: the images within 8 x floor["image"], depth within 8 x floor["depth"] of scale * depth
    where accumulation > 0.5; at most 7 pixels over, by no more than 2 / 255."""
    H, W = want["rgb"].shape[:2]
    over = torch.zeros((H, W), dtype=torch.bool, device=want["rgb"].device)
    worst = {}
    for k in IMAGES:
        if k not in want:
            continue
        d = (got[k] - want[k]).abs().amax(-1)
        worst[k] = float(d.max())
        over |= d > 8 * floor["image"]
        assert float(d.max()) <= 8 * floor["image"] + 2 / 255, (what, k, float(d.max()))
    solid = want["accumulation"][..., 0] > 0.5
    rel = ((got["depth"] - scale * want["depth"]).abs() / (scale * want["depth"]).abs())[..., 0]
    rel = torch.where(solid, rel, torch.zeros_like(rel))
    worst["depth"] = float(rel.max())
    over |= rel > 8 * floor["depth"]
    assert float(rel.max()) <= 8 * floor["depth"] + 2 / 255, (what, "depth", float(rel.max()))
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; bounds {8 * floor['image']:.2e} / {8 * floor['depth']:.2e}; "
          f"{int(over.sum())} pixels over")
    assert int(over.sum()) <= 7, (what, int(over.sum()), worst)
    assert float(solid.float().mean()) > 0.2


@pytest.mark.parametrize("raster", ["classic", "antialiased"])
@pytest.mark.parametrize("mode", ["shared", "separate"])
@pytest.mark.parametrize("sh_degree,step", [(3, 10**6), (3, 1), (0, 10**6)], ids=["degree3", "degree1_of_3", "degree0"])
def test_the_moved_model_from_the_moved_camera_renders_the_same_frame(sh_degree, step, mode, raster):
    st = _pkg()[3]
    deg = -1 if sh_degree == 0 else min(step, sh_degree)
    p = _params(sh_degree, mode)
    cam = _camera()
    want = _model(p, mode, sh_degree, step, raster).get_outputs(cam)
    assert ("accumulation_thermal" in want) == (mode == "separate")
    for scale in stf.SCALES:
        T = _similarity(scale)
        m = _model(p, mode, sh_degree, step, raster)
        st.transform_model(m, T)
        assert set(m.gauss_params.keys()) == set(p)
        got = m.get_outputs(T.apply_camera(cam))
        _compare_frames(want, got, scale, stf.oracle_floor(scale, deg, raster, mode == "separate", make_fields), (sh_degree, step, mode, raster, scale))


def test_a_moved_crop_box_keeps_the_same_gaussians():
    splat, _, _, st = _pkg()
    p = _params(3, "shared")
    box = splat.OrientedBox.from_params(*CROP)
    w2b = box.world_to_box().double()
    q = (w2b[:, :3] @ p["means"].double().T).T + w2b[:, 3]
    assert float((q.abs() - 0.5 * box.S.double()).abs().min()) >= 1e-3  # no mean within 1e-3 of a face
    inside = box.within(p["means"])
    assert 50 < int(inside.sum()) < 150
    cam = _camera()
    m = _model(p)
    m.set_crop(box)
    want = m.get_outputs(cam)
    radii = m.last_projection["radii"].cpu()
    assert bool((radii[~inside] == 0).all()) and int((radii[inside] > 0).sum()) > 40
    T = _similarity(0.4)
    st.transform_model(m, T)
    assert m.crop_box is not box and torch.equal(m.crop_box.S, (0.4 * box.S.double()).float())
    got = m.get_outputs(T.apply_camera(cam))
    assert torch.equal(m.last_projection["radii"].cpu() == 0, radii == 0)
    floor = stf.oracle_floor(0.4, 3, "classic", False, make_fields)
    for k in ("rgb", "thermal", "accumulation"):  # fewer Gaussians than the full scene: the full scene's floor is the yardstick, the pixel rule the same
        d = (got[k] - want[k]).abs().amax(-1)
        assert int((d > 8 * floor["image"]).sum()) <= 7 and float(d.max()) <= 8 * floor["image"] + 2 / 255, (k, float(d.max()))


# ---------------------------------------------------------------------------------------------------- 4. files in a moved frame
@pytest.mark.parametrize("spectrum", ["both", "rgb", "thermal"])
def test_a_moved_export_holds_the_moved_gaussians_that_were_kept(tmp_path, spectrum):
    _, _, splat_io, st = _pkg()
    T = _similarity(0.4)
    host = {k: v.clone() for k, v in _params(3, "shared").items()}
    host["features_dc"][7, 1] = float("nan")
    host["features_dc_thermal"][11, 0] = float("inf")
    host["scales"][13, 0] = float("nan")
    m = _model(host)
    out = splat_io.export_gaussian_ply(m, str(tmp_path / "moved.ply"), spectrum=spectrum, min_opacity=0.3, transform=T)
    keep = host["opacities"].reshape(-1) >= torch.tensor(splat_io.opacity_logit(0.3))
    keep[13] = False
    if spectrum != "thermal":
        keep[7] = False
    if spectrum != "rgb":
        keep[11] = False
    assert out["frame"] == "transformed" and out["exported"] == int(keep.sum()) and 100 < out["exported"] < stf.N_SCENE - 3
    assert torch.equal(stf.bits(m.gauss_params["means"].detach().cpu()), stf.bits(host["means"]))  # the model itself is not moved
    moved = st.transform_gaussians({k: v.detach() for k, v in m.gauss_params.items()}, T)
    got, info = splat_io.read_gaussian_ply(out["path"])
    assert info["num_gaussians"] == out["exported"]
    for k in ("means", "scales", "quats"):
        assert torch.equal(stf.bits(got[k]), stf.bits(moved[k].cpu()[keep])), k
    assert torch.equal(stf.bits(got["means"]), stf.bits(T.apply_points(m.gauss_params["means"].detach())[keep.to(DEV)].cpu()))
    if spectrum == "thermal":  # the thermal coefficients under the Inria names, the same in the three channels
        assert torch.equal(stf.bits(got["features_rest"]), stf.bits(moved["features_rest_thermal"].cpu()[keep].expand(-1, -1, 3).contiguous()))
    else:
        assert torch.equal(stf.bits(got["features_rest"]), stf.bits(moved["features_rest"].cpu()[keep]))
    if spectrum == "both":
        assert torch.equal(stf.bits(got["features_rest_thermal"]), stf.bits(moved["features_rest_thermal"].cpu()[keep]))
        assert torch.equal(stf.bits(got["features_dc"]), stf.bits(host["features_dc"][keep])) and torch.equal(got["opacities"], host["opacities"][keep])


def test_a_moved_file_loaded_with_the_inverse_renders_the_original_frame(tmp_path):
    _, _, splat_io, st = _pkg()
    p = _params(3, "separate")
    cam = _camera()
    m = _model(p, "separate")
    want = m.get_outputs(cam)
    for scale in stf.SCALES:
        T = _similarity(scale)
        out = splat_io.export_gaussian_ply(m, str(tmp_path / f"moved_{scale}.ply"), transform=T)
        assert out["exported"] == stf.N_SCENE
        # in its own frame the file is the moved scene ...
        there = _model(_params(3, "separate"), "separate")
        splat_io.load_gaussian_ply(there, out["path"])
        floor = stf.oracle_floor(scale, 3, "classic", True, make_fields)
        _compare_frames(want, there.get_outputs(T.apply_camera(cam)), scale, floor, ("file", scale))
        # ... and the inverse brings it home
        home = _model(_params(3, "separate"), "separate")
        info = splat_io.load_gaussian_ply(home, out["path"], transform=T.inverse())
        assert info["num_gaussians"] == stf.N_SCENE and info["separate"]
        for k in ("features_dc", "features_dc_thermal", "opacities", "opacities_thermal"):
            assert torch.equal(home.gauss_params[k].detach().cpu(), p[k]), k
        assert float((home.gauss_params["means"].detach().cpu() - p["means"]).abs().max()) <= 4 * 2.0 ** -24 * (1 + 2 / scale)
        _compare_frames(want, home.get_outputs(cam), 1.0, floor, ("home", scale))


def test_a_crop_is_given_in_the_models_frame(tmp_path):
    splat, _, splat_io, _ = _pkg()
    T = _similarity(2.5)
    p = _params(3, "shared")
    box = splat.OrientedBox.from_params(*CROP)
    inside = box.within(p["means"])
    m = _model(p)
    out = splat_io.export_gaussian_ply(m, str(tmp_path / "crop.ply"), crop=box, transform=T)
    assert out["exported"] == int(inside.sum())
    got, _ = splat_io.read_gaussian_ply(out["path"])
    assert torch.equal(stf.bits(got["means"]), stf.bits(T.apply_points(p["means"])[inside]))
    with pytest.raises(ValueError, match="OrientedBox"):
        splat_io.export_gaussian_ply(m, str(tmp_path / "no.ply"), crop=box.crop_struct(), transform=T)
