"""The HIP splat forward (tn_splat_project -> tn_splat_bin -> tn_splat_raster / tn_splat_raster_chains) against the float64 restatement
tests/splat_functional.py, on the scenes of tests/test_splat_forward_cpu.py: ragged image sizes, an image inside one tile, lists longer than
two 256-record batches, frames where most pixels stop early, opacities around 1/255, Gaussians that cover every tile, equal depths; both
raster modes, a non-zero RGB and thermal background, through get_outputs and get_train_outputs.

Tolerances: TOL_FACTOR x FLOOR[case][config][output], FLOOR being the float32 oracle's own distance from float64 (measured and asserted by the
CPU module) -- the margin because the kernel evaluates exp2(l2op - power) with v_exp_f32 and a log2-domain opacity (about 1 ulp each on an
exponent of magnitude up to 8) and fuses the quadratic form differently from torch.  On top, two ceilings that hold whatever was measured:
one lost or extra blend moves T by a factor 1 / (1 - alpha) with alpha >= 1/255, i.e. by >= 3.9e-3 relative, so T must agree to 1e-3; and
the images to 1e-4.  Pixels and Gaussians the float64 walk flags (a decision within 1e-4 of its threshold) are left out.  Every figure is
printed before it is asserted; profiles/splat_forward_parity.md holds the measured ones."""
import functools

import pytest
import torch

import test_splat_forward_cpu as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
T_CEILING, IMAGE_CEILING = 1e-3, 1e-4
PATHS = ("eval", "train")


def tol(case, mode, deg, key):
    return TOL_FACTOR * fc.FLOOR[case][fc.config_id(mode, deg)][key]


def _model(params, mode, deg):
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

    cfg = ThermalSplatfactoModelConfig(sh_degree=deg, sh_degree_interval=1, rasterize_mode=mode)
    m = ThermalSplatfactoModel(cfg, num_points=4, device=DEV)
    m.load_gaussians(params)
    m.step = 10**6
    bg, bgt = fc.background()
    m._background4 = lambda training: bg.tolist() + [bgt]  # the frame's background: the test's RGB + thermal colour on both paths
    return m


def _render(params, case, mode, deg):
    """eval render, a second eval render, training render (CPU tensors), the projection of the eval render and its intersection count."""
    from nerfstudio_thermal_amd.splat import PinholeCamera

    cam = PinholeCamera(*fc.case_camera(case))
    m = _model(params, mode, deg)
    keys = ("rgb", "thermal", "accumulation", "depth")
    a = m.get_outputs(cam)
    ev = {k: a[k].detach().cpu().clone() for k in keys}
    pj = {k: v.detach().cpu().clone() for k, v in m.last_projection.items()}
    n_isect = m.last_num_intersections
    b = m.get_outputs(cam)
    ev2 = {k: b[k].detach().cpu().clone() for k in keys}
    t = m.get_train_outputs(cam)
    tr = {k: t[k].detach().cpu().clone() for k in keys}
    return {"eval": ev, "eval2": ev2, "train": tr, "projection": pj, "intersections": n_isect, "train_intersections": m.last_num_intersections}


@functools.lru_cache(maxsize=None)
def rendered(case, mode, deg):
    return _render(fc.references(case, mode, deg)[0], case, mode, deg)


def _fill(out):
    """The depth fill value as the frame shows it: the depth of the pixels without accumulation (all the same number), or None."""
    empty = out["accumulation"] == 0
    if not bool(empty.any()):
        return None
    v = out["depth"][empty]
    assert bool((v == v[0]).all()), "pixels without accumulation carry different depths"
    return float(v[0])


def _check_images(case, mode, deg, path, ref, out):
    e = fc.image_errors(ref, out, _fill(out))
    rec = fc.FLOOR[case][fc.config_id(mode, deg)]
    print(f"{case} {fc.config_id(mode, deg)} {path}: " + ", ".join(
        f"{k} {e[k]:.2e} ({e[k] / rec[k]:.1f}x floor)" if rec.get(k) else f"{k} {e[k]:.2e}" for k in e))
    assert e["zero_mismatch"] == 0
    for k in ("rgb", "thermal", "accumulation"):
        assert e[k] <= tol(case, mode, deg, k), (k, e[k])
        assert e[k] < IMAGE_CEILING, (k, e[k])
    assert e["T"] <= tol(case, mode, deg, "T") and e["T"] < T_CEILING, e["T"]
    assert e["depth"] <= tol(case, mode, deg, "depth"), e["depth"]
    assert e["depth_fill"] <= tol(case, mode, deg, "depth"), e["depth_fill"]  # the fill value: to the depth tolerance
    # nothing blended in the reference (and no decision nearby): exactly nothing blended here -- accumulation 0 (zero_mismatch above), the
    # background bit for bit, the fill value in the depth
    bg, bgt = fc.background()
    empty = ~ref["flag_pixels"] & (ref["accumulation"][..., 0] == 0)
    if bool(empty.any()):
        assert torch.equal(out["rgb"][empty], bg.expand(int(empty.sum()), 3))
        assert torch.equal(out["thermal"][empty], torch.full((int(empty.sum()), 1), bgt))
        assert bool((out["depth"][empty] == _fill(out)).all())
    return e


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case,mode,deg", fc.CONFIGS)
def test_images_match_float64(case, mode, deg, path):
    _, ref, _ = fc.references(case, mode, deg)
    _check_images(case, mode, deg, path, ref, rendered(case, mode, deg)[path])


@pytest.mark.parametrize("case,mode,deg", fc.CONFIGS)
def test_training_render_equals_eval_render_bit_for_bit(case, mode, deg):
    r = rendered(case, mode, deg)
    for k in ("rgb", "thermal", "accumulation", "depth"):
        assert torch.equal(r["eval"][k], r["eval2"][k]), k  # deterministic
        assert torch.equal(r["eval"][k], r["train"][k]), k
    assert r["intersections"] == r["train_intersections"]


@pytest.mark.parametrize("case,mode,deg", fc.CONFIGS)
def test_projection_matches_float64(case, mode, deg):
    _, ref, _ = fc.references(case, mode, deg)
    pj, rp = rendered(case, mode, deg)["projection"], ref["projection"]
    e = fc.projection_errors(ref, pj)
    rec = fc.FLOOR[case][fc.config_id(mode, deg)]
    print(f"{case} {fc.config_id(mode, deg)}: " + ", ".join(f"{k} {v:.2e} ({v / rec[k]:.1f}x floor)" for k, v in e.items()))
    for k, v in e.items():
        assert v <= tol(case, mode, deg, k), (k, v)
    exc = fc.radius_exceptions(ref)
    assert int(exc.sum()) <= 0.01 * exc.numel()
    hits = torch.where(rp["ok"], (rp["tile_max"] - rp["tile_min"]).prod(-1), torch.zeros(()).int()).int()
    assert torch.equal(pj["radii"][~exc], rp["radii"][~exc])
    assert torch.equal(pj["num_tiles_hit"][~exc], hits[~exc])


@pytest.mark.parametrize("case,mode,deg", fc.CONFIGS)
def test_binning_keeps_every_pair_that_contributes(case, mode, deg):
    """The tight tile boxes may keep more (Gaussian, tile) pairs than contribute, never fewer, and never more than the 3-sigma boxes."""
    _, ref, _ = fc.references(case, mode, deg)
    r = rendered(case, mode, deg)
    lo, hi = int(ref["pair_used"].sum()), int(r["projection"]["num_tiles_hit"].sum())
    print(f"{case} {fc.config_id(mode, deg)}: {lo} contributing pairs <= {r['intersections']} binned <= {hi} in 3-sigma boxes")
    assert lo <= r["intersections"] <= hi


@pytest.mark.parametrize("mode", fc.MODES)
def test_equal_depths_keep_the_order_of_the_gaussians(mode):
    """`ties`: the frame is the float64 frame with the smaller index of each pair in front (test_images_match_float64) and NOT the one with
    the pairs swapped, which differs by more than 1e-3 (asserted by the CPU module)."""
    p, ref, _ = fc.references("ties", mode, 3)
    out = rendered("ties", mode, 3)["eval"]
    swapped = fc.reference64(fc.swap_ties(p), "ties", mode, 3)
    keep = ~(ref["flag_pixels"] | swapped["flag_pixels"])
    own = float((out["rgb"].double() - ref["rgb"]).abs()[keep].max())
    other = float((out["rgb"].double() - swapped["rgb"]).abs()[keep].max())
    print(f"ties {mode}: rgb error {own:.2e} against index order, {other:.2e} against the swapped pairs")
    assert own <= tol("ties", mode, 3, "rgb") and other > 1e-3
