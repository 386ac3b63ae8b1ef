"""The HIP splat backward (k_splat_raster_bwd -> k_splat_pair_fold -> k_splat_project_bwd, both instantiations, through
ThermalSplatfactoModel.get_train_outputs and .backward()) against float64 on the scenes of tests/splat_backward_cases.py: tile lists of three
and more 256-record batches with a partial front batch, tiles where some pixels hit the 1e-4 stop and others run on, blends on the 0.999
clamp, ragged image edges, an image inside one tile, Gaussians over every tile, opacities around 1/255, equal depths, N = 1; in separate mode
two chains that stop in different batches and Gaussians gated in one chain only.  tests/test_splat_backward_cases_cpu.py proves on the CPU
that the scenes have these properties.

Bounds.  (a) Every gradient: err <= 8 x floor, the floor being the float32 restatements' own distance from float64 on the same case
(bc.floors: float32 autograd and the float32 statement of the published backward walk, never below 2^-23; the CPU module holds it under 2e-5),
the factor 8 the project's margin for v_exp_f32, the log2-domain opacity and a differently fused quadratic form; and, independently,
err <= 2e-4 of the largest entry, which tests/test_splat_backward_gpu.py has always held.  (b) One pixel's thermal upstream gradient gives
d features_dc_thermal[g] = 0.28209479 alpha_g T_g at that pixel: relative error <= 1e-3 (one lost, extra or misordered blend in front of g
moves T_g by at least 1 / (1 - 1/255), 3.9e-3), and exactly zero for every Gaussian the pixel does not blend.  Nothing here is calibrated on
the kernels' output; every figure is printed before it is asserted, and profiles/splat_backward_parity.md holds the measured ones."""
import pytest
import torch

import splat_backward_cases as bc
import test_splat_forward_cpu as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
FIXED_BOUND = 2e-4
PROBE_BOUND = 1e-3
IDS = [bc.config_id(c) for c in bc.ALL_CONFIGS]


def _model(p, mode, deg, sep):
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

    cfg = ThermalSplatfactoModelConfig(sh_degree=deg, sh_degree_interval=1, rasterize_mode=mode, thermal_opacity_mode="separate" if sep else "shared")
    m = ThermalSplatfactoModel(cfg, num_points=4, device=DEV)
    m.load_gaussians(p)
    m.step = 10**6
    bg, bgt = fc.background()
    m._background4 = lambda training: bg.tolist() + [bgt]  # the frame's background: the test's RGB + thermal colour on both paths
    return m


def _camera(case):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    return PinholeCamera(*bc.case_camera(case))


def _grads(m, cam, w):
    m.zero_grad(set_to_none=True)
    out = m.get_train_outputs(cam)
    sum((out[k] * w[k].float().to(DEV)).sum() for k in w).backward()
    g = {k: m.gauss_params[k].grad.detach().cpu().clone() for k in m.param_names}
    g["xys"] = m.last_xys_grad.detach().cpu().clone()
    return g, out


def _excluded(m, st):
    """Gaussians left out for a decision of their own: on the frustum clamp, or with a radius that is zero on one side only."""
    radii_hip = m.last_projection["radii"].cpu()
    excl = bc.cpu_excluded(st) | ((radii_hip > 0) != (st["projection"]["radii"] > 0))
    assert int(excl.sum()) <= bc.MAX_EXCLUDED_GAUSSIANS * excl.numel(), int(excl.sum())
    return excl, radii_hip


def _check_gradients(name, hip, ref, excl, sep):
    worst = 0.0
    for k, (floor, _, _) in bc.floors(ref, excl, sep).items():
        assert hip[k].shape == ref["g64"][k].shape and bool(torch.isfinite(hip[k]).all()), k
        err = bc.rel_err(hip[k], ref["g64"][k], ~excl)
        print(f"{name} d {k}: err {err:.2e}, floor {floor:.2e}, ratio {err / floor:.2f}")
        assert err <= TOL_FACTOR * floor, (k, err, floor)
        assert err <= FIXED_BOUND, (k, err)
        worst = max(worst, err / floor)
    return worst


@pytest.mark.parametrize("cfg", bc.ALL_CONFIGS, ids=IDS)
def test_gradients_match_float64(cfg):
    case, mode, deg, sep = cfg
    ref = bc.reference(*cfg)
    cam = _camera(case)
    m = _model(ref["p"], mode, deg, sep)
    hip, tr = _grads(m, cam, ref["w"])
    ev = m.get_outputs(cam)
    for k in [k for k, _ in bc.images(sep)] + ["depth"]:
        assert torch.equal(tr[k].detach(), ev[k]), k  # the training render is the eval render, bit for bit
    excl, radii_hip = _excluded(m, ref["st"])
    print(f"{bc.config_id(cfg)}: {int(excl.sum())} of {excl.numel()} Gaussians left out, {100 * float(ref['st']['flag_pixels'].float().mean()):.2f} % of the pixels "
          f"without upstream gradient, {m.last_num_intersections} pairs")
    worst = _check_gradients(bc.config_id(cfg), hip, ref, excl, sep)
    print(f"{bc.config_id(cfg)}: largest err / floor {worst:.2f}")
    for k in bc.param_names(sep):
        assert bc.amax(hip[k][radii_hip == 0]) == 0.0, k  # culled Gaussians get exactly zero
    assert bc.amax(hip["means"]) > 0 and bc.amax(hip["opacities"]) > 0


@pytest.mark.parametrize("cfg", bc.PROBE_CONFIGS, ids=[bc.config_id(c) for c in bc.PROBE_CONFIGS])
def test_single_pixel_probes(cfg):
    """One backward per probe pixel with the upstream gradient 1 on that pixel's thermal value and 0 everywhere else."""
    case, mode, deg, sep = cfg
    ref = bc.reference(*cfg)
    pixels, pj, op = bc.probe_pixels(*cfg)
    cam = _camera(case)
    m = _model(ref["p"], mode, deg, sep)
    m.get_outputs(cam)
    excl, _ = _excluded(m, ref["st"])
    lit = pj["colors"][:, 3] > 0  # the thermal SH colour passes its clamp at zero
    skip = excl | pj["near_sh"]
    for label, ix, iy in pixels:
        w = {k: torch.zeros_like(v) for k, v in ref["w"].items()}
        w["thermal"][iy, ix, 0] = 1.0
        hip, _ = _grads(m, cam, w)
        got = hip["features_dc_thermal"][:, 0].double()
        pp = bc.probe_pixel(pj, op, ix, iy)
        want = torch.where(lit, bc.SH_C0 * pp["weight"], torch.zeros_like(pp["weight"]))
        keep = ~(skip | pp["flagged"])
        big = keep & (want > bc.EPS * float(want.max()))
        rel = float(((got - want).abs() / want)[big].max()) if bool(big.any()) else 0.0
        stray = int((keep & (want == 0) & (got != 0)).sum())
        print(f"{bc.config_id(cfg)} {label} ({ix}, {iy}): {int((pp['weight'] > 0).sum())} blends, T {pp['T']:.2e}, {'stopped' if pp['stopped'] else 'running'}, "
              f"{int(big.sum())} entries compared, largest relative error {rel:.2e}, {stray} nonzero where the pixel blends nothing")
        assert bool(torch.isfinite(got).all())
        assert rel <= PROBE_BOUND, (label, rel)
        assert stray == 0, (label, stray)


@pytest.mark.parametrize("sep", [None, ("noise", "thermal_low")], ids=["shared", "separate"])
def test_no_residue_in_a_reused_workspace(sep):
    """`deep` with upstream gradients x 1000, then `opaque` on the same model: the gradients of `opaque` are those of a fresh model, bit
    for bit.  (`opaque` leaves most pair records behind its pixels' last contributors unwritten; k_splat_pair_fold sums them all the same.)"""
    first = ("deep", "classic", 3, sep[0] if sep else None)
    second = ("opaque", "classic", 3, sep[1] if sep else None)
    a, b = bc.reference(*first), bc.reference(*second)
    fresh, _ = _grads(_model(b["p"], "classic", 3, sep), _camera("opaque"), b["w"])
    m = _model(a["p"], "classic", 3, sep)
    dirty, _ = _grads(m, _camera("deep"), {k: 1e3 * v for k, v in a["w"].items()})
    assert bc.amax(dirty["means"]) > 0
    m.load_gaussians(b["p"])
    again, _ = _grads(m, _camera("opaque"), b["w"])
    for k in fresh:
        assert torch.equal(again[k], fresh[k]), k


def test_equal_depths_keep_the_order_of_the_gaussians():
    """`ties`: the gradients are those of the float64 reference with the smaller index of each pair in front (to 8 x floor in
    test_gradients_match_float64; here, under the upstream image both references share, to the fixed bound) and NOT those with the pairs
    swapped, which differ by more than 1e-3 (asserted by the CPU module too)."""
    cfg = [c for c in bc.CONFIGS if c[0] == "ties"][0]
    case, mode, deg, sep = cfg
    ref, sw = bc.reference(*cfg), bc.swapped_reference(*cfg)
    m = _model(ref["p"], mode, deg, sep)
    hip, _ = _grads(m, _camera(case), sw["w"])
    m.get_outputs(_camera(case))
    excl, _ = _excluded(m, ref["st"])
    own = {k: bc.rel_err(hip[k], sw["own"][k], ~excl) for k in hip}
    other = {k: bc.rel_err(hip[k], sw["other"][k], ~excl) for k in hip}
    print("ties, against index order: " + ", ".join(f"{k} {v:.2e}" for k, v in own.items()))
    print("ties, against the swapped pairs: " + ", ".join(f"{k} {v:.2e}" for k, v in other.items()))
    for k, v in own.items():
        assert v <= FIXED_BOUND, (k, v)
    assert max(other.values()) > 1e-3
