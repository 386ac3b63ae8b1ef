"""Ray-contribution scoring and pruning without a GPU: the float64 restatement (splat_contrib_functional.py) against the forward walk and the
single-pixel probes of splat_backward_cases.py, the conditions on the scenes the GPU test scores, `prune_mask`'s rules, the config's refusals and
the host-side validation of the new entry points."""
import ctypes as C
import math

import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
import splat_backward_cases as bc
import splat_contrib_functional as cf
from nerfstudio_thermal_amd import _lib, splat_calls
from nerfstudio_thermal_amd.splat import ThermalSplatfactoModelConfig
from nerfstudio_thermal_amd.splat_prune import GaussianScores, prune_gaussians, prune_mask, score_gaussians  # noqa: F401

# a small scene per property: batches with a partial front batch, stopping pixels, both chains of separate mode
WALK_SCENES = [(("single", "classic", 3, None), 0), (("subtile", "classic", 3, None), 0), (("opaque", "classic", 3, None), 0),
               (("faint", "classic", 3, "mirror"), 0), (("faint", "classic", 3, "mirror"), 1)]
PROBES = [("opaque", "classic", 3, None), ("opaque", "classic", 3, "rgb_low")]
assert all(c in bc.PROBE_CONFIGS for c in PROBES)


def _weight_image(case):
    _, W, H = bc.case_camera(case)[4:]
    g = torch.Generator().manual_seed(7)
    w = torch.rand(H, W, generator=g, dtype=torch.float64)
    w[::3, ::2] = 0.0  # pixels that count for nothing
    return w


@pytest.mark.parametrize("sc", WALK_SCENES, ids=[cf.scene_id(s) for s in WALK_SCENES])
def test_the_scores_sum_to_the_weighted_accumulation_of_the_forward_walk(sc):
    """sum_g sum[g] = sum_p weight_p (1 - T_p) with T from bc.raster_forward_walk, and the walk's other outputs agree with it."""
    (case, mode, deg, sep), chain = sc
    p = bc.scene(case, deg, sep)
    pw = _weight_image(case)
    c = cf.contributions(p, case, mode, deg, sep, chain, torch.float64, pw)
    pj, fw = bc.walk_stats(p, case, mode, deg, sep, "op_t" if chain else "op")
    assert torch.equal(c["T"], fw["T"]) and torch.equal(c["stopped"], fw["stopped"])
    want = float((pw * (1.0 - fw["T"])).sum())
    assert want > 0
    assert abs(float(c["sum"].sum()) - want) <= 1e-12 * want
    assert cf.conservation_error(c, pw) <= 1e-12
    # a Gaussian scores iff some pixel with a positive weight blends it; the maximum is a blend weight: at most the clamp
    assert float(c["max"].max()) <= 0.999 and bool((c["max"] <= c["sum"] + 1e-300).all())
    assert torch.equal(c["hits"] > 0, c["max"] > 0) and torch.equal(c["hits"] > 0, c["sum"] > 0)
    assert not bool((c["hits"] > 0)[~fw["used"]].any())
    ones = cf.contributions(p, case, mode, deg, sep, chain, torch.float64)
    assert torch.equal(ones["hits"] > 0, fw["used"]) and int(ones["hits"].sum()) == int(fw["count"].sum())
    if case == "opaque":  # pixels stop here: the Gaussian a pixel stops at takes nothing from it
        assert bool(fw["stopped"].any())


@pytest.mark.parametrize("cfg", PROBES, ids=[bc.config_id(c) for c in PROBES])
def test_per_pixel_weights_are_those_of_the_single_pixel_probes(cfg):
    case, mode, deg, sep = cfg
    pixels, pj, op = bc.probe_pixels(*cfg)
    assert len(pixels) >= 3
    p = bc.scene(case, deg, sep)
    c = cf.contributions(p, case, mode, deg, sep, 1 if sep else 0, torch.float64, probes=[(ix, iy) for _, ix, iy in pixels])
    for j, (label, ix, iy) in enumerate(pixels):
        want = bc.probe_pixel(pj, op, ix, iy)["weight"]
        assert int((want > 0).sum()) > 0, label
        assert torch.equal(c["probe_weight"][j] > 0, want > 0), label
        assert bc.amax(c["probe_weight"][j] - want) <= 1e-12 * bc.amax(want), label  # (a cumulative product against a running one)


@pytest.mark.parametrize("cfg", sorted({s[0] for s in cf.SCENES}, key=bc.config_id), ids=bc.config_id)
def test_the_scored_scenes_meet_the_conditions_on_flags_and_exclusions(cfg):
    """Conditions on the scenes, not measurements: at most MAX_FLAGGED_PIXELS of the pixels carry weight 0, at most MAX_EXCLUDED_GAUSSIANS of
    the Gaussians are left out on the CPU's side."""
    _, st = cf.scene_stats(*cfg)
    assert float(st["flag_pixels"].float().mean()) <= bc.MAX_FLAGGED_PIXELS
    excl = bc.cpu_excluded(st)
    assert int(excl.sum()) <= bc.MAX_EXCLUDED_GAUSSIANS * excl.numel()


def test_the_scenes_are_the_ones_the_issue_names():
    assert len(cf.SCENES) == 9 + 2 * len(bc.SEP_CONFIGS) and len(set(cf.SCENES)) == len(cf.SCENES)
    with pytest.raises(ValueError):
        cf.chain_opacity({"op": torch.zeros(1)}, None, 1)


def _scores(max_rgb, max_thermal=None):
    s = GaussianScores.zeros(len(max_rgb), "cpu")
    s.max_rgb = torch.tensor(max_rgb, dtype=torch.float32)
    if max_thermal is not None:
        s.max_thermal = torch.tensor(max_thermal, dtype=torch.float32)
    return s


def test_prune_mask_rules():
    s = _scores([0.5, 0.01, 0.0, 0.2, 0.009], [0.0, 0.0, 0.3, 0.2, 0.0])
    assert s.importance().tolist() == pytest.approx([0.5, 0.01, 0.3, 0.2, 0.009])
    # the threshold is inclusive; a Gaussian only the thermal frames see survives
    assert prune_mask(s, min_contribution=0.01).tolist() == [True, True, True, True, False]
    assert prune_mask(s, min_contribution=0.0).tolist() == [True] * 5
    assert prune_mask(s, keep_ratio=0.4).tolist() == [True, False, True, False, False]
    assert prune_mask(s, keep_ratio=0.41).tolist() == [True, False, True, True, False]  # ceil(2.05) = 3
    assert prune_mask(s, keep_ratio=0.0).tolist() == [False] * 5 and prune_mask(s, keep_ratio=1.0).tolist() == [True] * 5
    tied = _scores([0.2, 0.7, 0.2, 0.2, 0.2])
    assert prune_mask(tied, keep_ratio=0.6).tolist() == [True, True, True, False, False]  # ties go to the lower index
    thirty = _scores([float(i) for i in range(30)])
    assert int(prune_mask(thirty, keep_ratio=0.1).sum()) == 3  # 0.1 * 30 = 3.0000000000000004 keeps 3
    for kw in ({}, {"min_contribution": 0.01, "keep_ratio": 0.5}, {"min_contribution": -1.0}, {"keep_ratio": 1.5}, {"keep_ratio": -0.1},
               {"min_contribution": float("nan")}):
        with pytest.raises(ValueError):
            prune_mask(s, **kw)
    both = s.combined(_scores([0.1, 0.9, 0.0, 0.0, 0.0]))
    assert both.max_rgb.tolist() == pytest.approx([0.5, 0.9, 0.0, 0.2, 0.009]) and both.hits_rgb.dtype == torch.int64


def test_config_refusals():
    ok = ThermalSplatfactoModelConfig(prune_at_steps=[16000, 24000])
    assert ok.prune_at_steps == (16000, 24000) and ok.prune_min_contribution == 0.01
    assert ThermalSplatfactoModelConfig().prune_at_steps == ()
    assert ThermalSplatfactoModelConfig(stop_split_at=10, refine_every=1, prune_at_steps=(11,)).prune_at_steps == (11,)
    for kw in ({"prune_min_contribution": -0.01}, {"prune_min_contribution": float("nan")},
               {"prune_at_steps": (24000, 16000)}, {"prune_at_steps": (16000, 16000)}, {"prune_at_steps": (16000.0,)}, {"prune_at_steps": (True,)},
               {"prune_at_steps": 16000}, {"prune_at_steps": (15000,)}, {"prune_at_steps": (100, 16000)},
               {"prune_at_steps": (16000,), "stop_split_at": 16000}, {"prune_at_steps": (16000,), "strategy": "mcmc"},
               {"prune_at_steps": (16050,)}):  # not a refinement step: the callback would never see it
        with pytest.raises(ValueError):
            ThermalSplatfactoModelConfig(**kw)
    ThermalSplatfactoModelConfig(strategy="mcmc")  # without steps MCMC is untouched


def test_entry_points_validate_on_the_host():
    """A short scratch answers TN_EINVAL before any launch, as every workspace-writing entry point does; so do bad sizes, flags and null pointers."""
    lib = _lib.load()
    assert _lib.ABI_VERSION == 314 and lib.tn_version() == 314  # additions only: the version stays
    assert {"tn_splat_raster_contrib", "tn_splat_contrib_workspace_bytes"} <= set(_lib.SIGNATURES)
    wb = lib.tn_splat_contrib_workspace_bytes
    assert wb(-1, 10) == -1 and wb(10, -1) == -1 and wb(1 << 31, 10) == -1
    need = wb(1000, 5000)
    assert need >= 5000 * 3 * 4 + 1000 * 4 and wb(0, 0) > 0
    cam = _lib.TnSplatCamera()
    cam.width, cam.height, cam.fx, cam.fy = 64, 48, 50.0, 50.0
    fake = C.c_void_p(256 * 4096)  # never dereferenced
    call = lambda *a: lib.tn_splat_raster_contrib(*a, None)  # noqa: E731
    good = [C.byref(cam), 1000, fake, 5000, 0, 0, None, fake, need, fake, fake, fake, fake]
    assert call(C.byref(cam), 0, None, 0, 0, 0, None, None, 0, None, None, None, None) == 0  # no Gaussians: nothing to do
    for i, bad in ((8, need - 1), (4, 2), (5, 2), (5, -1), (1, -1), (3, -1), (2, None), (7, None), (9, None), (10, None), (11, None), (12, None), (0, None)):
        args = list(good)
        args[i] = bad
        assert call(*args) == -22, i
    assert call(*good[:8], need - 1, *good[9:]) == -22 and b"tn_splat_contrib_workspace_bytes" in lib.tn_last_error()
    assert math.isfinite(need)


def test_the_call_layer_checks_shapes_before_the_library():
    cam = _lib.TnSplatCamera()
    cam.width, cam.height = 8, 4
    acc = [torch.zeros(5), torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.int64), torch.zeros(5, dtype=torch.int32)]
    with pytest.raises(ValueError, match="pixel_weight"):
        splat_calls.raster_contrib(cam, 5, None, 10, 0, 0, torch.zeros(8, 4), *acc)
    with pytest.raises(ValueError, match="sum_acc"):
        splat_calls.raster_contrib(cam, 5, None, 10, 0, 0, None, acc[0], torch.zeros(4, dtype=torch.float64), *acc[2:])
    with pytest.raises(ValueError):
        prune_gaussians(type("M", (), {"num_points": 3})(), torch.ones(3))  # not a bool mask
    with pytest.raises(ValueError):
        prune_gaussians(type("M", (), {"num_points": 3})(), torch.ones(4, dtype=torch.bool))
