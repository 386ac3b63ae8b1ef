"""The absgrad densification statistic on the GPU (ThermalSplatfactoModelConfig.use_absgrad: the ABS instantiations of k_splat_raster_bwd and
k_splat_pair_fold behind tn_splat_raster_backward with v_xys_abs, through ThermalSplatfactoModel.get_train_outputs and .backward()) against the
float64 walk of tests/splat_absgrad_functional.py, on scenes of tests/splat_backward_cases.py:

  deep-classic-3                  four 256-record batches with a partial front batch
  opaque-antialiased-3            stopped and running pixels in one wave, compensated opacity
  ragged-classic-1                image edges inside tiles
  clamped-classic-3               blends on the 0.999 clamp, which contribute zero
  single-classic-3                N = 1
  faint-antialiased-3             the 1/255 gate
  deep-classic-3-sep-noise        both chains carry upstream gradient on the same pixels
  faint-classic-3-sep-mirror      Gaussians gated in one chain only
  opaque-classic-3-sep-thermal_low  chains that stop in different batches

Bound of the parity test: err <= 8 x floor and err <= 2e-4 of the largest entry, the project's rule (tests/test_splat_backward_cases_gpu.py).
The floor is the largest of the float32 walk's error on v_xys_abs, the configuration's bc.floors(...)["xys"] floor and 2^-23.  The second term is
there because the absolute sum does not cancel: its float32 walk error sits at about one rounding, which measures summation luck and not the
arithmetic the factor 8 is the margin for (v_exp_f32, the log2-domain opacity, T rebuilt by division); the signed floor of the same per-pixel
products does measure that arithmetic.  A lost or extra per-pixel term, or a misplaced absolute value, moves entries by tens of per cent
(the CPU module holds the median |abs| / |signed| above 2).  Nothing is calibrated on the kernels' output; every figure is printed before it
is asserted, and profiles/splat_absgrad.md holds the measured ones."""
import dataclasses

import pytest
import torch

import splat_absgrad_functional as af
import splat_backward_cases as bc
import splat_pose_functional as pf
import test_splat_forward_cpu as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
FIXED_BOUND = 2e-4
TRAIN_FRAMES = 4
ROW = 2


def _model(p, mode, deg, sep, absgrad=True, rgb_mode="off", **kw):
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd.config import CameraOptimizerConfig
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

    cfg = ThermalSplatfactoModelConfig(sh_degree=deg, sh_degree_interval=1, rasterize_mode=mode, thermal_opacity_mode="separate" if sep else "shared",
                                       use_absgrad=absgrad, camera_optimizer=CameraOptimizerConfig(mode=rgb_mode), **kw)
    m = ThermalSplatfactoModel(cfg, num_points=4, device=DEV, num_train_data=TRAIN_FRAMES)
    m.load_gaussians(p)
    m.step = 10**6
    bg, bgt = fc.background()
    m._background4 = lambda training: bg.tolist() + [bgt]  # the frame's background: the test's RGB + thermal colour
    return m


def _camera(case, cam_idx=ROW):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    return PinholeCamera(*bc.case_camera(case), cam_idx=cam_idx)


def _backward(m, cam, w):
    m.zero_grad(set_to_none=True)
    out = m.get_train_outputs(cam)
    sum((out[k] * w[k].float().to(DEV)).sum() for k in w).backward()
    g = {k: m.gauss_params[k].grad.detach().cpu().clone() for k in m.param_names}
    g["xys"] = m.last_xys_grad.detach().cpu().clone()
    if m.last_xys_absgrad is not None:
        g["xys_abs"] = m.last_xys_absgrad.detach().cpu().clone()
    return g


def _excluded(m, st):
    """tests/test_splat_backward_cases_gpu.py's: on the frustum clamp, or with a radius that is zero on one side only; at most 1 %."""
    radii_hip = m.last_projection["radii"].cpu()
    excl = bc.cpu_excluded(st) | ((radii_hip > 0) != (st["projection"]["radii"] > 0))
    assert int(excl.sum()) <= bc.MAX_EXCLUDED_GAUSSIANS * excl.numel(), int(excl.sum())
    return excl, radii_hip


@pytest.mark.parametrize("cfg", af.CONFIGS, ids=af.IDS)
def test_absgrad_matches_float64(cfg):
    case, mode, deg, sep = cfg
    ref = af.reference(*cfg)
    m = _model(ref["bc"]["p"], mode, deg, sep)
    hip = _backward(m, _camera(case), ref["bc"]["w"])
    excl, radii_hip = _excluded(m, ref["bc"]["st"])
    walk = bc.rel_err(ref["abs32"], ref["abs64"], ~excl)
    signed = bc.floors(ref["bc"], excl, sep)["xys"][0]
    floor = max(walk, signed, bc.EPS)
    err = bc.rel_err(hip["xys_abs"], ref["abs64"], ~excl)
    print(f"{bc.config_id(cfg)}: {int(excl.sum())} of {excl.numel()} Gaussians left out; v_xys_abs err {err:.2e}, floor {floor:.2e} (float32 walk on abs {walk:.2e}, "
          f"signed xys floor {signed:.2e}), ratio {err / floor:.2f}, bound {min(TOL_FACTOR * floor, FIXED_BOUND):.2e}")
    assert hip["xys_abs"].shape == ref["abs64"].shape and bool(torch.isfinite(hip["xys_abs"]).all())
    assert err <= TOL_FACTOR * floor, (err, floor)
    assert err <= FIXED_BOUND, err
    assert bc.amax(hip["xys_abs"][radii_hip == 0]) == 0.0  # culled Gaussians get exactly zero
    assert float(hip["xys_abs"].min()) >= 0.0 and bc.amax(hip["xys_abs"]) > 0


@pytest.mark.parametrize("cfg", [("deep", "classic", 3, None), ("deep", "classic", 3, "noise")], ids=["deep-classic-3", "deep-classic-3-sep-noise"])
def test_the_flag_changes_nothing_else(cfg):
    case, mode, deg, sep = cfg
    ref = bc.reference(*cfg)
    on = _model(ref["p"], mode, deg, sep, absgrad=True)
    off = _model(ref["p"], mode, deg, sep, absgrad=False)
    g_on, g_off = _backward(on, _camera(case), ref["w"]), _backward(off, _camera(case), ref["w"])
    assert off.last_xys_absgrad is None and "xys_abs" in g_on
    for k in list(off.param_names) + ["xys"]:
        assert bc.amax(g_off[k]) > 0 and torch.equal(g_on[k], g_off[k]), k


def _plain_upstream(case, sep=None):
    _, W, H = bc.case_camera(case)[4:]
    return bc.upstream(case, sep, torch.zeros(H, W, dtype=torch.bool))


@pytest.mark.parametrize("sep", [None, "noise"], ids=["shared", "separate"])
def test_absgrad_is_bit_reproducible_and_zero_where_culled(sep):
    """`ragged` (94 of its 600 Gaussians are off screen): two backwards of one frame, and the culled rows."""
    p, w = bc.scene("ragged", 1, sep), _plain_upstream("ragged", sep)
    m = _model(p, "classic", 1, sep)
    a = _backward(m, _camera("ragged"), w)
    radii = m.last_radii.cpu()
    b = _backward(m, _camera("ragged"), w)
    assert bc.amax(a["xys_abs"]) > 0 and torch.equal(a["xys_abs"], b["xys_abs"])
    assert int((radii == 0).sum()) > 0 and bc.amax(a["xys_abs"][radii == 0]) == 0.0


def test_one_pixel_gives_the_absolute_value_of_the_signed_gradient():
    """Upstream gradient on a single pixel's thermal value: one term per Gaussian, so abs = |signed| on every Gaussian the pixel blends (1e-5
    relative: the two leave the kernel by different roundings -- plain conic after the sum, scaled conic before it) and exactly zero elsewhere."""
    cfg = ("opaque", "classic", 3, None)
    ref = bc.reference(*cfg)
    pixels, pj, op = bc.probe_pixels(*cfg)
    m = _model(ref["p"], cfg[1], cfg[2], cfg[3])
    m.get_outputs(_camera(cfg[0]))
    excl, _ = _excluded(m, ref["st"])
    assert pixels
    for label, ix, iy in pixels:
        w = {k: torch.zeros_like(v) for k, v in ref["w"].items()}
        w["thermal"][iy, ix, 0] = 1.0
        g = _backward(m, _camera(cfg[0]), w)
        got, want = g["xys_abs"].double(), g["xys"].double().abs()
        pp = bc.probe_pixel(pj, op, ix, iy)
        keep = ~(excl | pp["flagged"])  # a decision within flag_tol of its threshold may fall either way in float32
        blends = keep & (pp["weight"] > 0)
        big = blends[:, None] & (want > 0)
        rel = float(((got - want).abs() / want)[big].max()) if bool(big.any()) else 0.0
        stray = int(((got != 0) & (keep & (pp["weight"] == 0))[:, None]).sum())
        print(f"opaque ({ix}, {iy}) {label}: {int(blends.sum())} blends, {int(big.sum())} entries compared, largest relative difference {rel:.2e}, "
              f"{stray} nonzero where the pixel blends nothing")
        assert int(big.sum()) > 0 and rel <= 1e-5, (label, rel)
        assert stray == 0, label


def test_pose_path_gives_the_same_statistic():
    """`ragged` through the pose instantiations (mode "SO3xR3", a non-zero row) against a model with the pose off that is given the corrected
    camera directly: bit-equal last_xys_absgrad (and last_xys_grad).  The corrected camera is the one the frame used -- the device record of
    tn_splat_pose_camera, copied number by number into the comparison frame's camera struct: a host restatement of exp_map in another precision
    gives a camera some ulps away, and with it another frame."""
    from nerfstudio_thermal_amd import splat

    case = "ragged"
    p, w = pf.scene(case, 3, None, "moved"), _plain_upstream(case)
    cam = _camera(case)
    posed = _model(p, "classic", 3, None, rgb_mode="SO3xR3")
    with torch.no_grad():
        posed.camera_optimizer.pose_adjustment[ROW] = pf.pose_row("moved").float().to(DEV)
    g_pose = _backward(posed, cam, w)
    assert posed.camera_optimizer.pose_adjustment.grad is not None and bc.amax(posed.camera_optimizer.pose_adjustment.grad[ROW].cpu()) > 0
    s = splat.camera_struct(cam)
    rec = splat.pose_camera_record(cam, s, posed.camera_optimizer.pose_adjustment.detach(), ROW).cpu().tolist()
    for i in range(12):
        s.viewmat[i] = rec[i]
    for i in range(16):
        s.projmat[i] = rec[12 + i]
    for i in range(3):
        s.position[i] = rec[28 + i]
    plain = _model(p, "classic", 3, None)
    real = splat.camera_struct
    splat.camera_struct = lambda camera, *a, **k: s
    try:
        g_plain = _backward(plain, cam, w)
    finally:
        splat.camera_struct = real
    moved = _backward(_model(p, "classic", 3, None), cam, w)  # the uncorrected camera: another frame
    assert not torch.equal(moved["xys_abs"], g_pose["xys_abs"])
    assert bc.amax(g_pose["xys_abs"]) > 0
    assert torch.equal(g_pose["xys"], g_plain["xys"])
    assert torch.equal(g_pose["xys_abs"], g_plain["xys_abs"])


def test_absgrad_reaches_the_densification_decision():
    """`single` under the reference's upstream images, one training frame + after_train + refinement_after at step 600 (densification runs, big
    Gaussians are not culled yet).  k_refine_classify compares norm / frames x half the frame's larger side with densify_grad_thresh, so the
    threshold between the two statistics -- the geometric mean of the float64 norms n_s (signed) and n_a (absolute), which the CPU module holds
    at least a factor 4 apart -- is sqrt(n_s n_a) in those units.  With the flag off the model keeps its Gaussian; with it on, it splits."""
    cfg = ("single", "classic", 3, None)
    ref = af.reference(*cfg)
    n_s, n_a = float(ref["signed64"][0].norm()), float(ref["abs64"][0].norm())
    _, W, H = bc.case_camera("single")[4:]
    thresh = (n_s * n_a) ** 0.5 * 0.5 * max(W, H)
    counts = {}
    for flag in (False, True):
        m = _model(ref["bc"]["p"], cfg[1], cfg[2], None, absgrad=flag, densify_grad_thresh=thresh)
        m.step = 600
        _backward(m, _camera("single"), ref["bc"]["w"])
        m.after_train(600)
        stat = float(m.xys_grad_norm[0])
        m.refinement_after(None, 600)
        counts[flag] = m.num_points
        print(f"single, use_absgrad={flag}: accumulated norm {stat:.4e} (float64: signed {n_s:.4e}, absolute {n_a:.4e}), threshold in its units "
              f"{(n_s * n_a) ** 0.5:.4e}; {m.num_points} Gaussians after the refinement, counts {m.last_refine_counts}")
        assert abs(stat - (n_a if flag else n_s)) <= 1e-3 * (n_a if flag else n_s)
    assert counts[False] == 1 and counts[True] > 1, counts


def test_empty_frame_leaves_zeros():
    from nerfstudio_thermal_amd.synth import look_at_camera

    ref = bc.reference("single", "classic", 3, None)
    m = _model(ref["p"], "classic", 3, None)
    m.step = 600
    cam = _camera("single")
    away = dataclasses.replace(cam, camera_to_world=look_at_camera((2.5, 0.0, 0.0), target=(5.0, 0.0, 0.0)))  # the Gaussian is behind the camera
    out = m.get_train_outputs(away)
    assert m.last_num_intersections == 0
    (out["rgb"].sum() + out["thermal"].sum()).backward()
    assert m.last_xys_absgrad.shape == (1, 2) and float(m.last_xys_absgrad.abs().max()) == 0.0
    m.after_train(600)
    assert float(m.xys_grad_norm[0]) == 0.0
