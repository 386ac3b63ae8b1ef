"""Ray-contribution scoring (tn_splat_raster_contrib: k_splat_raster_contrib -> k_splat_contrib_fold, through splat_prune.score_gaussians) and
pruning on the GPU, on the backward-parity scenes of tests/splat_backward_cases.py: lists of three and more 256-record batches with a partial front
batch, stopped and running pixels in one wave, ragged edges, a sub-tile image, opacities on the 1/255 gate, blends on the 0.999 clamp, N = 1; in
separate mode both chains.  tests/test_splat_contrib_cpu.py holds the conditions on the scenes.

The pixel weight is 1, and 0 on the pixels the float64 render flags (a decision within FLAG_TOL of its threshold): the device the backward tests
use for their upstream images.  Bounds: `sum` and `max` per Gaussian against the float64 restatement over the Gaussians not excluded
(bc.cpu_excluded, plus those whose integer radius is zero on one side only), relative to the largest kept entry, within TOL_FACTOR = 8 (the factor
of tests/test_splat_forward_gpu.py) times the float32 restatement's own error, at least 2^-23; `hits` exactly; the frame's total against the
eval render's accumulation within 8 times what the float32 restatement shows for the same identity (at least 2^-23: one rounding of the total).
Every figure is printed before it is asserted; profiles/splat_prune.md holds the measured ones.

There is deliberately no test that removing the Gaussians with a zero score leaves the frame unchanged: it is not true.  A Gaussian at which a
pixel stops (its blend would take the transmittance to 1e-4 or below) is not blended there and scores nothing there, yet it ends that pixel's
list; without it the pixel goes on to what lies behind."""
import functools
import math

import pytest
import torch

import splat_backward_cases as bc
import splat_contrib_functional as cf
import splat_oracle as so
import test_splat_forward_cpu as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
FIELDS = ("max", "sum", "hits", "views")


def _mods():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import optim, splat, splat_prune

    return splat, splat_prune, optim


def _model(p, mode="classic", deg=3, sep=None, **kw):
    splat = _mods()[0]
    cfg = splat.ThermalSplatfactoModelConfig(sh_degree=deg, sh_degree_interval=1, rasterize_mode=mode, thermal_opacity_mode="separate" if sep else "shared", **kw)
    m = splat.ThermalSplatfactoModel(cfg, num_points=4, device=DEV, num_train_data=3)
    m.load_gaussians(p)
    m.step = 10**6
    bg, bgt = fc.background()
    m._background4 = lambda training: bg.tolist() + [bgt]
    return m


def _camera(case, thermal=False):
    return _mods()[0].PinholeCamera(*bc.case_camera(case), is_thermal=thermal)


def _cpu(scores, thermal):
    return dict(zip(FIELDS, (t.cpu() for t in scores.spectrum(thermal))))


def _score(m, cam, pw=None):
    return _mods()[1].score_gaussians(m, [cam], None if pw is None else [pw.float()])


def _kept(m, st):
    radii_hip = m.last_projection["radii"].cpu()
    excl = bc.cpu_excluded(st) | ((radii_hip > 0) != (st["projection"]["radii"] > 0))
    assert int(excl.sum()) <= bc.MAX_EXCLUDED_GAUSSIANS * excl.numel(), int(excl.sum())
    return ~excl, radii_hip


@pytest.mark.parametrize("sc", cf.SCENES, ids=[cf.scene_id(s) for s in cf.SCENES])
def test_scores_match_float64(sc):
    cfg, chain = sc
    case, mode, deg, sep = cfg
    name = cf.scene_id(sc)
    ref = cf.reference(cfg, chain)
    thermal = chain == 1
    cam = _camera(case, thermal)
    m = _model(ref["p"], mode, deg, sep)
    scores = _score(m, cam, ref["pw"])
    got, other = _cpu(scores, thermal), _cpu(scores, not thermal)
    keep, radii_hip = _kept(m, ref["st"])
    c64 = ref["c64"]
    print(f"{name}: {int((~keep).sum())} of {keep.numel()} Gaussians left out, {100 * float(1 - ref['pw'].mean()):.2f} % of the pixels without weight, "
          f"{m.last_num_intersections} pairs, {int((c64['hits'] > 0).sum())} Gaussians score")
    for k in ("sum", "max"):
        err, floor = bc.rel_err(got[k], c64[k], keep), cf.floor(ref, k, keep)
        print(f"{name} {k}: err {err:.2e}, floor {floor:.2e}, ratio {err / floor:.2f}")
        assert bool(torch.isfinite(got[k]).all()) and err <= TOL_FACTOR * floor, (k, err, floor)
    differ = keep & (got["hits"] != c64["hits"])
    print(f"{name} hits: {int(differ.sum())} kept Gaussians with another count, {int(c64['hits'].sum())} hits in all")
    assert int(differ.sum()) == 0, differ.nonzero().reshape(-1).tolist()[:8]
    assert torch.equal(got["views"] > 0, got["max"] > 0) and int(got["views"].max()) <= 1
    # conservation: the frame's total is the eval render's accumulation of that chain over the weighted pixels
    out = m.get_outputs(cam)
    acc = out["accumulation_thermal" if thermal else "accumulation"][..., 0].double().cpu()
    want = float((ref["pw"] * acc).sum())
    err = abs(float(got["sum"].sum()) - want) / want
    floor = max(cf.conservation_error(ref["c32"], ref["pw"]), bc.EPS)
    print(f"{name} conservation: err {err:.2e}, floor {floor:.2e}")
    assert err <= TOL_FACTOR * floor, (err, floor)
    # bounds and exact zeros
    assert bool((got["max"] <= torch.tensor(0.999)).all()) and bool((got["max"] >= 0).all()) and bool((got["sum"] >= got["max"].double()).all())
    off = radii_hip == 0
    for k in FIELDS:
        assert not bool(got[k][off].any()), k  # not on screen: exactly zero
        assert not bool(other[k].any()), k  # the other spectrum's fields are untouched
    assert float(got["max"].max()) > 0


def test_an_all_zero_pixel_weight_leaves_zeros():
    cfg = ("opaque", "classic", 3, None)
    p, st = cf.scene_stats(*cfg)
    m = _model(p)
    got = _cpu(_score(m, _camera("opaque"), torch.zeros_like(st["flag_pixels"], dtype=torch.float32)), False)
    assert m.last_num_intersections > 0
    assert not bool(got["max"].view(torch.int32).any()) and not bool(got["sum"].view(torch.int64).any())  # bit for bit
    assert not bool(got["hits"].any()) and not bool(got["views"].any())


def test_frames_accumulate_and_the_bits_repeat():
    """[c1, c2, c3] in one call = the three scored one by one and combined (max of the maxima, sums of the rest), bit for bit, in both
    spectra; the same call twice gives the same bits."""
    sp = _mods()[1]
    cfg = ("deep", "classic", 3, "noise")
    p, _ = cf.scene_stats(*cfg)
    m = _model(p, sep="noise")
    cams = [_camera("deep"), _camera("opaque", thermal=True), _camera("ragged"), _camera("deep", thermal=True)]
    g = torch.Generator().manual_seed(5)
    pws = [None, torch.rand(cams[1].height, cams[1].width, generator=g), torch.rand(cams[2].height, cams[2].width, generator=g), None]
    together, again = sp.score_gaussians(m, cams, pws), sp.score_gaussians(m, cams, pws)
    singles = [sp.score_gaussians(m, [c], [w]) for c, w in zip(cams, pws)]
    combined = functools.reduce(lambda a, b: a.combined(b), singles)
    for thermal in (False, True):
        a, b, c = _cpu(together, thermal), _cpu(again, thermal), _cpu(combined, thermal)
        for k in FIELDS:
            assert a[k].dtype == c[k].dtype and torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), (thermal, k)
        assert int(a["views"].max()) == 2 and float(a["max"].max()) > 0
    assert together.max_rgb.dtype == torch.float32 and together.sum_rgb.dtype == torch.float64
    assert together.hits_rgb.dtype == torch.int64 and together.views_rgb.dtype == torch.int32 and together.max_rgb.is_cuda
    assert torch.equal(together.importance(), torch.maximum(together.max_rgb, together.max_thermal))
    with pytest.raises(ValueError):
        sp.score_gaussians(m, cams, pws[:2])
    with pytest.raises(ValueError):
        sp.score_gaussians(m, cams[:1], [torch.zeros(3, 3)])


def test_spectra_are_routed_to_their_chains():
    """("opaque", "rgb_low"): RGB opacities sigmoid(-1) = 0.27, thermal opacities sigmoid(3) = 0.95.  An RGB camera fills only *_rgb from chain 0, a
    thermal camera at the same pose only *_thermal from chain 1, and the importances differ as the opacities do."""
    cfg = ("opaque", "classic", 3, "rgb_low")
    p, st = cf.scene_stats(*cfg)
    pw = cf.reference(cfg, 0)["pw"]
    m = _model(p, sep="rgb_low")
    rgb, th = _score(m, _camera("opaque"), pw), _score(m, _camera("opaque", thermal=True), pw)
    keep, _ = _kept(m, st)
    for s, thermal in ((rgb, False), (th, True)):
        assert not any(bool(t.any()) for t in s.spectrum(not thermal))
        want = cf.reference(cfg, int(thermal))["c64"]
        dist = float((_cpu(s, thermal)["max"].double() - want["max"]).abs()[keep].max())
        print(f"rgb_low, {'thermal' if thermal else 'RGB'} camera: largest importance {float(s.importance().max()):.4f}, against float64 {dist:.2e}")
        assert dist <= 1e-4  # (the chain is the right one: the other's maxima are tenths away; the parity test holds the tight bound)
    assert float(rgb.importance().max()) <= 1.0 / (1.0 + math.e) + 1e-6 < 0.5 < float(th.importance().max())
    shared = _model({k: v for k, v in p.items() if k != "opacities_thermal"})  # shared mode: a thermal camera walks chain 0, into *_thermal
    s = _score(shared, _camera("opaque", thermal=True), pw)
    assert torch.equal(s.hits_thermal, rgb.hits_rgb) and torch.allclose(s.max_thermal, rgb.max_rgb, rtol=1e-5, atol=0) and not bool(s.max_rgb.any())


def _train_steps(m, opts, cams, gts, steps, cbs=None):
    from nerfstudio_thermal_amd.model import TrainingCallbackLocation as L

    for step in steps:
        for cb in cbs or []:
            cb.run_callback_at_location(step, L.BEFORE_TRAIN_ITERATION)
        opts.zero_grad_all()
        i = step % len(cams)
        loss = m.get_loss_dict(m.get_train_outputs(cams[i]), {"image": gts[i], "is_thermal": bool(cams[i].is_thermal)})
        functools.reduce(torch.add, loss.values()).backward()
        opts.optimizer_step_all()
        opts.scheduler_step_all()
        for cb in cbs or []:
            cb.run_callback_at_location(step, L.AFTER_TRAIN_ITERATION)


def _gaussians(n, seed, sep):
    p = so.synth_gaussians(n, seed=seed, extent=1.0, scale_range=(-4.5, -2.0))
    if sep:
        p["opacities_thermal"] = p["opacities"].flip(0).clone()
    return p


def _rig():
    splat = _mods()[0]
    import splat_functional as sf

    def cam(eye, thermal=False, idx=None):
        w, h = (48, 36) if thermal else (96, 72)
        fx = sf.fov_focal(w)
        return splat.PinholeCamera(so.look_at_camera(eye), fx, fx, w / 2, h / 2, w, h, cam_idx=idx, is_thermal=thermal)

    return [cam((2.4, 0.5, 0.7), idx=0), cam((-0.6, 2.3, 0.5), idx=1), cam((2.2, -0.8, 0.4), True, idx=2)]


def _targets(cams, sep):
    teacher = _model(_gaussians(400, 31, sep), sep=sep)
    return [(lambda o, c: (o["thermal"].expand(-1, -1, 3) if c.is_thermal else o["rgb"]).clone())(teacher.get_outputs(c), c) for c in cams]


def test_prune_gaussians_carries_parameters_moments_and_optimisers():
    splat, sp, optim = _mods()
    cams = _rig()
    gts = _targets(cams, True)
    n = 300
    m = _model(_gaussians(n, 32, True), sep=True)
    m.step = 0
    opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=optim.HipAdam)
    _train_steps(m, opts, cams, gts, range(3))
    before = {k: m.gauss_params[k].detach().clone() for k in m.param_names}
    group_of = {v: g for g, v in m.group_params.items()}
    state = {k: {a: b.clone() for a, b in opts.optimizers[group_of[k]].state[m.gauss_params[k]].items()} for k in m.param_names}
    keep = torch.rand(n, generator=torch.Generator().manual_seed(9)) < 0.6
    for bad in (keep[:-1], keep.float(), keep.tolist()):
        with pytest.raises(ValueError):
            sp.prune_gaussians(m, bad, opts)
    removed = sp.prune_gaussians(m, keep.to(DEV), opts)
    assert removed == n - int(keep.sum()) > 0 and m.num_points == int(keep.sum())
    assert m.xys_grad_norm is None and m.vis_counts is None and m.max_2Dsize is None and m._filter_stale
    fresh = _model({k: v[keep.to(DEV)] for k, v in before.items()}, sep=True)
    fresh.step = m.step
    for cam in cams:
        a, b = m.get_outputs(cam), fresh.get_outputs(cam)
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    for k in m.param_names:
        o, p = opts.optimizers[group_of[k]], m.gauss_params[k]
        assert torch.equal(p.detach(), before[k][keep.to(DEV)]), k
        assert len(o.param_groups) == 1 and len(o.param_groups[0]["params"]) == 1 and o.param_groups[0]["params"][0] is p, k
        assert opts.parameters[group_of[k]][0] is p and len(o.state) == 1 and p in o.state, k
        st = o.state[p]
        assert set(st) == set(state[k]) and float(st["step"]) == float(state[k]["step"]) == 3.0, k
        for a in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[a], state[k][a][keep.to(st[a].device)]), (k, a)
        assert bool(state[k]["exp_avg"].any()) or k.startswith("features_rest"), k
    assert sp.prune_gaussians(m, torch.ones(m.num_points, dtype=torch.bool), opts) == 0
    _train_steps(m, opts, cams, gts, range(3, 5))  # training goes on, on the new N
    assert m.gauss_params["means"].grad.shape == (m.num_points, 3)
    left = m.num_points
    assert sp.prune_gaussians(m, torch.zeros(left, dtype=torch.bool), opts) == left and m.num_points == 0
    out = m.get_outputs(cams[0])  # no Gaussians: the background
    assert not bool(out["accumulation"].any())
    assert int(sp.score_gaussians(m, cams).max_rgb.numel()) == 0


def test_the_refinement_callback_prunes_at_its_step(monkeypatch):
    """20 steps with stop_split_at = 10 and prune_at_steps = (11,): the pass runs once, after step 11, and step 12's backward runs on the new N."""
    splat, sp, optim = _mods()
    cams = _rig()
    gts = _targets(cams, False)
    p = _gaussians(300, 33, False)
    p["opacities"][:40] = -6.0  # sigmoid = 0.0025 < 1/255: never blended, so they score nothing
    kw = dict(warmup_length=100, refine_every=1, stop_split_at=10, prune_at_steps=(11,))
    m = _model(p, **kw)
    m.step = 0
    opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=optim.HipAdam)
    cbs = m.get_training_callbacks(opts)
    calls = []
    real = sp.score_gaussians
    monkeypatch.setattr(sp, "score_gaussians", lambda model, cameras, *a, **k: (calls.append((model.step, len(cameras))), real(model, cameras, *a, **k))[1])
    _train_steps(m, opts, cams, gts, range(11), cbs)
    assert m.last_prune_counts is None and m.num_points == 300 and not calls
    with pytest.raises(RuntimeError, match="set_prune_cameras"):
        _train_steps(m, opts, cams, gts, [11], cbs)  # the step arrives without cameras
    m.set_prune_cameras(cams)
    _train_steps(m, opts, cams, gts, [11], cbs)
    before, removed = m.last_prune_counts
    print(f"prune at step 11: {before} Gaussians, {removed} removed")
    assert calls == [(11, 3)] and before == 300 and 40 <= removed < 300 and m.num_points == before - removed
    assert float(torch.sigmoid(m.gauss_params["opacities"].detach()).min()) >= 1.0 / 255.0
    _train_steps(m, opts, cams, gts, range(12, 20), cbs)
    assert calls == [(11, 3)] and m.last_prune_counts == (before, removed)
    for k in m.param_names:
        assert m.gauss_params[k].grad.shape[0] == m.num_points, k
    assert all(math.isfinite(float(v)) for v in m.get_loss_dict(m.get_train_outputs(cams[0]), {"image": gts[0], "is_thermal": False}).values())
    off = _model(p, warmup_length=100, refine_every=1, stop_split_at=10)  # the switch off: the pass is never called
    off.step = 11
    off.refinement_after(None, 11)
    assert calls == [(11, 3)] and off.last_prune_counts is None
