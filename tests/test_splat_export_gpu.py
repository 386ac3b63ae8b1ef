"""The Gaussian-splat PLY export on the GPU: tn_export_splat_pack against its torch restatement (tests/splat_export_functional.py), and
export_gaussian_ply / load_gaussian_ply end to end on ThermalSplatfactoModel.

Everything but the degree-0 colour map is exact: the rows are copies of parameters, the keep rule is float compares, the order is the Gaussians'
own.  The box tests run on scf.crop_scene, which has no mean in the rounding band of a face (tests/test_splat_export_cpu.py asserts it), so the
kept sets are exact too."""
import functools
import math

import pytest
import torch

import splat_crop_functional as scf
import splat_export_functional as sxf
import splat_functional as sf
import splat_oracle as so
import splat_sep_functional as ssf

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 12345.0
U = 2.0 ** -24  # fp32 unit roundoff


def _pkg():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import splat, splat_calls, splat_io

    return splat, splat_calls, splat_io


def _obox(box):
    return _pkg()[0].OrientedBox(R=box.R, T=box.T, S=box.S)


def _pack(p, spectrum, colour_mode=0, thr=-math.inf, box=None):
    """pack_call of host params -> (out_rows on the host, guard included; count)."""
    _, splat_calls, splat_io = _pkg()
    sep = "opacities_thermal" in p
    tensors = [p[k].to(DEV).contiguous() for k in splat_calls.param_names("separate" if sep else "shared")]
    n, K = p["means"].shape[0], p["features_rest"].shape[1] + 1
    W = len(sxf.properties(spectrum, K, sep, colour_mode))
    out = torch.full((n, W), GUARD, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    splat_io.pack_call(tensors, sxf.SPECTRA[spectrum], colour_mode, thr, None if box is None else _obox(box).crop_struct(), out, count)
    torch.cuda.synchronize()
    return out.cpu(), int(count.item())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_rows(got, count, want_rows, what):
    assert count == want_rows.shape[0], (what, count, want_rows.shape[0])
    assert got.shape[1] == want_rows.shape[1], what
    assert torch.equal(_bits(got[:count]), _bits(want_rows)), what
    assert bool((got[count:] == GUARD).all()), what  # rows at and beyond count are not written


# ---------------------------------------------------------------------------------------------------- 1. the pack against its restatement
@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 3 * 256 + 17])
def test_pack_equals_the_restatement_bit_for_bit(n, K):
    """One lane, a wave's edge, a block's edge, a ragged last block; W is never a multiple of 64, so a block's flat run straddles rows.  Inputs:
    random, with a NaN / +Inf / -Inf planted in each attribute class in turn (Gaussians 2, 7, 12, ... mod n)."""
    for separate in (False, True):
        clean = sxf.random_params(n, K, separate, seed=n + K)
        p = sxf.plant_defects(clean, seed=n + K)
        for spectrum in ("rgb", "thermal", "both"):
            want, kept = sxf.pack_ref(p, spectrum)
            got, count = _pack(p, spectrum)
            _assert_rows(got, count, want, (n, K, separate, spectrum))
            if n >= 63:
                assert 0 < count < n
            # and without defects everything is kept, in order
            got, count = _pack(clean, spectrum)
            _assert_rows(got, count, sxf.pack_ref(clean, spectrum)[0], (n, K, separate, spectrum, "clean"))
            assert count == n


@pytest.mark.parametrize("separate", [False, True], ids=["shared", "separate"])
def test_a_defect_drops_the_gaussian_from_the_rows_that_carry_it(separate):
    """Each attribute class in turn: a defect in a thermal-only attribute leaves the rgb export alone and drops the Gaussian from thermal and
    both; an RGB-only one the other way round; a shared one drops it everywhere."""
    n, K = 70, 4
    base = sxf.random_params(n, K, separate, seed=3)
    every = set(range(n))
    for a, name in enumerate(k for k in sxf.ATTRIBUTES if k in base):
        for d, bad in enumerate(sxf.DEFECTS):
            p = {k: v.clone() for k, v in base.items()}
            g = (7 * a + 3 * d + 1) % n
            p[name].reshape(n, -1)[g, -1] = bad
            in_rgb = name not in sxf.THERMAL_ONLY
            in_thermal = name not in sxf.RGB_ONLY and not (name == "opacities" and separate)
            for spectrum, dropped in (("rgb", in_rgb), ("thermal", in_thermal), ("both", True)):
                want, kept = sxf.pack_ref(p, spectrum)
                assert set(kept.tolist()) == (every - {g} if dropped else every), (name, spectrum)
                got, count = _pack(p, spectrum)
                _assert_rows(got, count, want, (name, bad, spectrum))


def test_blocks_with_nothing_kept_with_everything_kept_and_nothing_at_all():
    n, K = 3 * 256 + 17, 4
    p = sxf.random_params(n, K, True, seed=11)
    p["means"][256:512, 1] = float("nan")  # block 1: nothing kept; block 0: everything; blocks 2 and 3: some
    p["scales"][512::3, 2] = float("inf")
    for spectrum in ("rgb", "thermal", "both"):
        want, kept = sxf.pack_ref(p, spectrum)
        assert kept[:256].tolist() == list(range(256)) and int(((kept >= 256) & (kept < 512)).sum()) == 0 and 100 < int((kept >= 512).sum()) < 200
        got, count = _pack(p, spectrum)
        _assert_rows(got, count, want, spectrum)
        got, count = _pack(p, spectrum, thr=50.0)  # every logit is below: all n dropped, nothing written
        assert count == 0 and bool((got == GUARD).all())
    p["quats"][:, 0] = float("-inf")
    got, count = _pack(p, "both")
    assert count == 0 and bool((got == GUARD).all())
    # no Gaussians at all: TN_OK, and count is set
    got, count = _pack({k: v[:0] for k, v in p.items()}, "both")
    assert count == 0 and got.shape == (0, len(sxf.properties("both", K, True)))


# ---------------------------------------------------------------------------------------------------- 2. the opacity threshold
def test_min_opacity_is_an_exact_float_compare():
    """Logits exactly at the threshold (kept), one ulp below (dropped), one ulp above (kept); `both` in separate mode keeps by the larger."""
    _, _, splat_io = _pkg()
    thr = splat_io.opacity_logit(0.005)
    t = torch.tensor(thr, dtype=torch.float32)
    below, above = torch.nextafter(t, torch.tensor(-math.inf)), torch.nextafter(t, torch.tensor(math.inf))
    assert float(below) < thr < float(above)
    op = torch.stack([t, below, above, below, t, below, above, below])[:, None]
    oth = torch.stack([t, below, above, t, below, above, below, below])[:, None]
    p = sxf.random_params(8, 4, True, seed=5)
    p["opacities"], p["opacities_thermal"] = op.clone(), oth.clone()
    expect = {"rgb": [0, 2, 4, 6], "thermal": [0, 2, 3, 5], "both": [0, 2, 3, 4, 5, 6]}
    for spectrum, kept_want in expect.items():
        want, kept = sxf.pack_ref(p, spectrum, 0, thr)
        assert kept.tolist() == kept_want, spectrum
        got, count = _pack(p, spectrum, thr=thr)
        _assert_rows(got, count, want, spectrum)
    shared = ssf.shared_params(p)
    for spectrum in ("rgb", "thermal", "both"):  # one logit: the thermal row carries it too
        want, kept = sxf.pack_ref(shared, spectrum, 0, thr)
        assert kept.tolist() == [0, 2, 4, 6], spectrum
        got, count = _pack(shared, spectrum, thr=thr)
        _assert_rows(got, count, want, spectrum)
    got, count = _pack(p, "both", thr=-math.inf)  # off
    assert count == 8


# ---------------------------------------------------------------------------------------------------- 3. the box
@functools.lru_cache(maxsize=None)
def _scene(sh_degree):
    return scf.crop_scene(0, sh_degree)


def _params(sh_degree, mode):
    p = _scene(sh_degree)
    return p if mode == "separate" else ssf.shared_params(p)


@pytest.mark.parametrize("box_name", ["main", "second"])
@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_the_box_keeps_what_the_crop_mask_keeps(mode, box_name):
    box = {"main": scf.MAIN_BOX, "second": scf.SECOND_BOX}[box_name]
    p = _params(3, mode)
    mask = _obox(box).within(p["means"].to(DEV)).cpu()  # tn_splat_crop_mask
    assert torch.equal(mask, scf.within64(box, p["means"])) and 40 < int(mask.sum()) < 260
    for spectrum in ("rgb", "thermal", "both"):
        want, kept = sxf.pack_ref(p, spectrum, crop=box)
        assert torch.equal(kept, mask.nonzero().reshape(-1))
        got, count = _pack(p, spectrum, box=box)
        _assert_rows(got, count, want, spectrum)
        assert torch.equal(got[:count, :3], p["means"][mask])


def test_export_reports_what_it_dropped_and_writes_an_empty_file(tmp_path):
    _, _, splat_io = _pkg()
    p = {k: v.clone() for k, v in _params(3, "separate").items()}
    p["features_dc_thermal"][5, 0] = float("nan")
    m = _model(p, "separate", 3)
    keep = scf.within64(scf.MAIN_BOX, p["means"])
    keep[5] = False
    keep &= torch.maximum(p["opacities"], p["opacities_thermal"]).reshape(-1) >= torch.tensor(splat_io.opacity_logit(0.3))
    out = splat_io.export_gaussian_ply(m, str(tmp_path / "a.ply"), min_opacity=0.3, crop=_obox(scf.MAIN_BOX))
    assert out["exported"] == int(keep.sum()) and out["dropped"] == scf.N_SCENE - out["exported"] and 5 < out["exported"] < 200
    got, info = splat_io.read_gaussian_ply(out["path"])
    assert info["num_gaussians"] == out["exported"] and torch.equal(got["means"], p["means"][keep])
    out = splat_io.export_gaussian_ply(m, str(tmp_path / "none.ply"), crop=_obox(scf.NOTHING_BOX))
    assert out["exported"] == 0 and out["dropped"] == scf.N_SCENE
    got, info = splat_io.read_gaussian_ply(out["path"])
    assert info["num_gaussians"] == 0 and info["K"] == 16 and got["features_rest"].shape == (0, 15, 3)
    empty = _model(scf.subset(p, torch.zeros(scf.N_SCENE, dtype=torch.bool)), "separate", 3)  # a model without Gaussians
    out = splat_io.export_gaussian_ply(empty, str(tmp_path / "empty.ply"))
    assert out["exported"] == 0 and out["dropped"] == 0 and splat_io.read_gaussian_ply(out["path"])[1]["num_gaussians"] == 0


# ---------------------------------------------------------------------------------------------------- 4. the degree-0 colours
@pytest.mark.parametrize("separate", [False, True], ids=["shared", "separate"])
def test_colour_mode_1_against_the_float64_restatement(separate):
    """f = (sigmoid(dc) - 0.5) / C0, evaluated in double and rounded once to float32 on both sides.  The two double results F_dev and F_host differ
    by a few double ulps at most (the device's and the host's exp may differ in the last place, the three operations after it each add half an
    ulp): |F_dev - F_host| <= ~8 * 2^-53 |F|, some 2^-27 of a float32 ulp.  Two doubles that close round to the same float32 unless a rounding
    boundary lies between them, and then to the two float32 neighbours of that boundary: the float32 results differ by at most ONE float32 ulp
    (and almost never do).  Every other column is a copy and bit-exact."""
    n = 3 * 256 + 17
    p = sxf.random_params(n, 1, separate, seed=21)
    p["features_dc"] *= 3.0  # colours from ~0.0001 to ~0.9999
    p = sxf.plant_defects(p, seed=21)
    worst = 0.0
    for spectrum in ("rgb", "thermal", "both"):
        want, kept = sxf.pack_ref(p, spectrum, colour_mode=1)
        got, count = _pack(p, spectrum, colour_mode=1)
        assert count == want.shape[0] and 0 < count < n and bool((got[count:] == GUARD).all())
        got = got[:count]
        mapped = [6, 7, 8] + ([17] if spectrum == "both" else [])
        exact = [c for c in range(want.shape[1]) if c not in mapped]
        assert want.shape[1] == 17 + (spectrum == "both") * (1 + separate)
        assert torch.equal(_bits(got[:, exact]), _bits(want[:, exact])), spectrum
        diff = (got[:, mapped].double() - want[:, mapped].double()).abs()
        ulps = diff / sxf.ulp32(want[:, mapped])
        worst = max(worst, float(ulps.max()))
        assert bool((diff <= sxf.ulp32(want[:, mapped])).all()), (spectrum, float(ulps.max()))
    print(f"colour_mode 1, separate={separate}: largest difference to the float64 restatement {worst:.3g} float32 ulp")


# ---------------------------------------------------------------------------------------------------- 5.-8. end to end on the model
def _model(params, mode, sh_degree, step=10**6):
    splat = _pkg()[0]
    cfg = splat.ThermalSplatfactoModelConfig(sh_degree=sh_degree, sh_degree_interval=1, rasterize_mode="classic", background_thermal=0.3,
                                             thermal_opacity_mode=mode)
    m = splat.ThermalSplatfactoModel(cfg, num_points=4, device=DEV)
    if params is not None:
        m.load_gaussians(params)
    m.step = step
    m.eval()
    return m


def _camera():
    c2w, fx = so.look_at_camera((2.3, 0.4, 0.6)), sf.fov_focal(scf.W)
    return _pkg()[0].PinholeCamera(c2w, fx, fx, scf.W / 2 - 0.5, scf.H / 2 + 0.25, scf.W, scf.H)


KEYS = {"shared": {"rgb", "thermal", "depth", "accumulation", "background", "background_thermal"}}
KEYS["separate"] = KEYS["shared"] | {"accumulation_thermal"}


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_export_then_load_gives_the_same_model_and_the_same_frame(tmp_path, mode):
    _, _, splat_io = _pkg()
    p = _params(3, mode)
    m = _model(p, mode, 3)
    out = splat_io.export_gaussian_ply(m, str(tmp_path / "splat.ply"), spectrum="both")
    assert out["exported"] == scf.N_SCENE and out["dropped"] == 0
    assert out["properties"] == sxf.properties("both", 16, mode == "separate")
    fresh = _model(None, mode, 3)
    info = splat_io.load_gaussian_ply(fresh, out["path"])
    assert info["separate"] == (mode == "separate") and info["has_thermal"] and info["K"] == 16
    assert set(fresh.gauss_params.keys()) == set(m.gauss_params.keys()) == set(p)
    for k in p:
        assert fresh.gauss_params[k].shape == m.gauss_params[k].shape and torch.equal(_bits(fresh.gauss_params[k].detach()), _bits(m.gauss_params[k].detach())), k
    cam = _camera()
    want, got = m.get_outputs_for_camera(cam), fresh.get_outputs_for_camera(cam)
    assert set(got) == set(want) == KEYS[mode]
    for k in sorted(want):
        assert torch.equal(got[k], want[k]), k
    assert float(want["accumulation"].max()) > 0.5
    # an rgb file into a separate model: the thermal logits start as a copy of the opacities, the thermal features at mid-grey
    out = splat_io.export_gaussian_ply(m, str(tmp_path / "rgb.ply"), spectrum="rgb")
    other = _model(None, "separate", 3)
    info = splat_io.load_gaussian_ply(other, out["path"])
    assert not info["has_thermal"] and torch.equal(other.gauss_params["opacities_thermal"], other.gauss_params["opacities"])
    assert torch.equal(other.gauss_params["features_rest"], m.gauss_params["features_rest"]) and not bool(other.gauss_params["features_dc_thermal"].any())
    if mode == "separate":  # and a file with opacity_thermal is not for a shared model
        with pytest.raises(ValueError, match="opacity_thermal"):
            splat_io.load_gaussian_ply(_model(None, "shared", 3), str(tmp_path / "splat.ply"))


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_a_thermal_export_is_a_grey_inria_scene(tmp_path, mode):
    _, _, splat_io = _pkg()
    p = _params(3, mode)
    m = _model(p, mode, 3)
    out = splat_io.export_gaussian_ply(m, str(tmp_path / "thermal.ply"), spectrum="thermal")
    assert out["properties"] == sxf.properties("rgb", 16, False)  # the Inria names
    viewer = _model(None, "shared", 3)
    info = splat_io.load_gaussian_ply(viewer, out["path"])
    assert not info["has_thermal"] and not info["separate"]
    gp = viewer.gauss_params
    want_op = p["opacities_thermal"] if mode == "separate" else p["opacities"]
    assert torch.equal(gp["opacities"].cpu(), want_op) and torch.equal(gp["features_dc"].cpu(), p["features_dc_thermal"].expand(-1, 3))
    assert torch.equal(gp["features_rest"].cpu(), p["features_rest_thermal"].expand(-1, -1, 3))
    rgb = viewer.get_outputs_for_camera(_camera())["rgb"]
    assert torch.equal(rgb[..., 0], rgb[..., 1]) and torch.equal(rgb[..., 1], rgb[..., 2])
    assert float(rgb[..., 0].max() - rgb[..., 0].min()) > 0.1  # a scene, not a flat frame


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_degree_0_export_then_load(tmp_path, mode):
    """A degree-0 model keeps x = logit(colour) in features_dc; the file carries f = fl((c - 0.5) / C0), the loader x' = fl(logit(0.5 + C0 f)), both
    maps evaluated in double and rounded once (fl: to float32, relative error u = 2^-24; one float32 ulp is at most 2 u relative).  For colours c =
    sigmoid(x) in [0.02, 0.98] (asserted on this scene in tests/test_splat_export_cpu.py):
      the device may round f one ulp away from the host's restatement (test_colour_mode_1_...): |f - F| <= 2 u |F|, so p = 0.5 + C0 f has
      |p - c| <= 2 u |c - 0.5| <= 0.96 u;
      x' = fl(logit p): |x' - logit p| <= u |logit p|, and sigmoid has the slope p (1 - p), so this moves the colour by at most
      u max p (1 - p) |logit p| = 0.2240 u (the maximum is at p = 0.176);
      together |sigmoid(x') - c| <= 1.2 u in exact arithmetic.                                                              (colour bound)
    The parameters: against the float64 restatement x'_ref (f and x' rounded on the host), a one-ulp flip of f moves p by C0 ulp(f) and logit p by
    that over p (1 - p), and the rounding of x' may then land on the neighbour: |x' - x'_ref| <= 1.01 C0 ulp(f_ref) / (p (1 - p)) + ulp(x'_ref).
    The frame: a pixel is sum_i w_i colour_i + T background with weights w_i, T that depend on nothing the round trip changed (every other
    parameter is bit-equal, so depth and accumulation must be bit-equal); sum_i w_i + T <= 1.  The rasteriser's colour is its fp32 sigmoid of x,
    accurate to 4 u absolute (an expf and a division on values <= 1), so the colours of the two frames differ by at most 1.2 u + 2 * 4 u; and each
    frame's fp32 sum of m + 1 <= N + 1 terms is within (N + 1) u / (1 - (N + 1) u) of its exact value.  Hence
      |pixel' - pixel| <= 9.2 u + 2.02 (N + 1) u  = 617.3 u = 3.7e-5  for the N = 300 Gaussians of the scene.                (frame bound)
    The blending term dominates and is a worst case over tile depth; the observed difference is recorded in profiles/splat_export.md."""
    _, _, splat_io = _pkg()
    p = _params(0, mode)
    m = _model(p, mode, 0)
    assert m._frame_settings()[1] == -1
    out = splat_io.export_gaussian_ply(m, str(tmp_path / "deg0.ply"), spectrum="both")
    assert out["exported"] == scf.N_SCENE and out["properties"] == sxf.properties("both", 1, mode == "separate", 1)
    fresh = _model(None, mode, 0)
    info = splat_io.load_gaussian_ply(fresh, out["path"])
    assert info["colour_mode"] == 1 and info["K"] == 1
    for k in p:
        if k in ("features_dc", "features_dc_thermal"):
            x = p[k].double()
            c = torch.sigmoid(x)
            assert 0.02 <= float(c.min()) and float(c.max()) <= 0.98
            f_ref = ((c - 0.5) / sxf.SH_C0).float()  # float64, rounded once
            pr = 0.5 + sxf.SH_C0 * f_ref.double()
            x_ref = torch.log(pr / (1.0 - pr)).float()
            colour_err = float((torch.sigmoid(x_ref.double()) - c).abs().max())
            assert colour_err <= 1.2 * U, colour_err  # the colour bound, on the restatement
            bound = 1.01 * sxf.SH_C0 * sxf.ulp32(f_ref) / (pr * (1.0 - pr)) + sxf.ulp32(x_ref)
            got = fresh.gauss_params[k].detach().cpu().double()
            err = (got - x_ref.double()).abs()
            assert bool((err <= bound).all()), (k, float((err / bound).max()))
            print(f"degree 0 {mode} {k}: round-trip colour error of the restatement {colour_err / U:.3f} u; loaded vs restated parameters, "
                  f"largest error / bound {float((err / bound).max()):.3g}, not bit-equal at {int((err > 0).sum())} of {err.numel()}")
        else:
            assert torch.equal(_bits(fresh.gauss_params[k].detach().cpu()), _bits(p[k])), k
    cam = _camera()
    want, got = m.get_outputs_for_camera(cam), fresh.get_outputs_for_camera(cam)
    assert set(got) == set(want) == KEYS[mode]
    tol = (9.2 + 2.02 * (scf.N_SCENE + 1)) * U
    for k in sorted(want):
        if k in ("rgb", "thermal"):
            d = float((got[k] - want[k]).abs().max())
            print(f"degree 0 {mode} frame {k}: max |loaded - original| = {d:.3e} ({d / U:.2f} u), bound {tol:.3e}")
            assert d <= tol, (k, d)
        else:
            assert torch.equal(got[k], want[k]), k
    assert float(want["accumulation"].max()) > 0.5


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_two_exports_are_the_same_bytes(tmp_path, mode):
    _, _, splat_io = _pkg()
    p = {k: v.clone() for k, v in _params(3, mode).items()}
    p["features_rest"][17, 3, 1] = float("nan")
    m = _model(p, mode, 3)
    files = []
    for i in range(2):
        out = splat_io.export_gaussian_ply(m, str(tmp_path / f"e{i}.ply"), spectrum="both", min_opacity=0.05, crop=_obox(scf.SECOND_BOX))
        assert 10 < out["exported"] < scf.N_SCENE
        files.append(open(out["path"], "rb").read())
    assert files[0] == files[1] and len(files[0]) > 1000
