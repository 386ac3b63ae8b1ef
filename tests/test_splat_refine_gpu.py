"""Splat refinement on the GPU: tn_splat_grad_stats / tn_splat_refine_plan / tn_splat_refine_apply through ThermalSplatfactoModel.after_train /
refinement_after against the functional restatement (splat_refine_functional.py) on the same device tensors, the optimiser bookkeeping,
determinism, edge cases, checkpoints, an end-to-end fit with refinement and a 1080p / 1 M-Gaussian smoke."""
import math

import pytest
import torch

import splat_functional as sf
import splat_oracle as so
import splat_refine_functional as rf

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest", "features_dc_thermal", "features_rest_thermal")
SIZE = (480, 640)
NUM_TRAIN_DATA = 10
MARGIN = 1e-5


def _mods():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import optim, splat

    return splat, optim


def _camera(c2w, fx, cx, cy, W, H):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    return PinholeCamera(c2w, fx, fx, cx, cy, W, H)


def _model(params, seed=0, **cfg_kw):
    splat, _ = _mods()
    cfg = splat.ThermalSplatfactoModelConfig(**cfg_kw)
    m = splat.ThermalSplatfactoModel(cfg, num_points=4, device=DEV, seed=seed, num_train_data=NUM_TRAIN_DATA)
    m.load_gaussians(params)
    return m


def _away(q, thresholds):
    """True where q is more than MARGIN (relative) away from every threshold"""
    ok = torch.ones_like(q, dtype=torch.bool)
    for t in thresholds:
        ok &= (q - t).abs() > MARGIN * abs(t)
    return ok


def _random_state(n, seed, cfg):
    """n Gaussians at sh_degree 3 with statistics, every thresholded quantity more than MARGIN away from its threshold."""
    g = torch.Generator().manual_seed(seed)
    p = so.synth_gaussians(n, seed=seed, extent=1.0)
    p["scales"] = torch.empty((n, 3)).uniform_(math.log(0.002), math.log(1.0), generator=g)
    p["opacities"] = torch.empty((n, 1)).uniform_(-4.0, 4.0, generator=g)
    M = max(SIZE)
    cnt = torch.randint(1, 6, (n,), generator=g).float()
    avg = torch.empty(n).uniform_(0.0, 2.0 * cfg.densify_grad_thresh, generator=g)
    gsum = avg * cnt / (0.5 * M)
    m2d = torch.empty(n).uniform_(0.0, 0.3, generator=g)
    for _ in range(20):  # nudge the few values that sit within the margin of a threshold (on the device, as the decisions are taken there)
        s = p["scales"].to(DEV)
        e = torch.exp(s).max(dim=-1).values
        e_new = torch.exp(torch.log(torch.exp(s) / 1.6)).max(dim=-1).values
        sc_ok = _away(e, (cfg.densify_size_thresh, cfg.cull_scale_thresh)) & _away(e_new, (cfg.densify_size_thresh, cfg.cull_scale_thresh))
        op_ok = _away(torch.sigmoid(p["opacities"].to(DEV)).reshape(-1), (cfg.cull_alpha_thresh,))
        gr_ok = _away((gsum.to(DEV) / cnt.to(DEV)) * 0.5 * M, (cfg.densify_grad_thresh,))
        m2_ok = _away(m2d.to(DEV), (cfg.split_screen_size, cfg.cull_screen_size))
        if bool((sc_ok & op_ok & gr_ok & m2_ok).all()):
            break
        p["scales"][~sc_ok.cpu()] += 1e-3
        p["opacities"][~op_ok.cpu()] += 1e-3
        gsum[~gr_ok.cpu()] *= 1.001
        m2d[~m2_ok.cpu()] += 1e-3
    else:
        raise AssertionError("could not keep the inputs away from the thresholds")
    return p, (gsum.to(DEV), cnt.to(DEV), m2d.to(DEV))


def _optimizers(m, cls=None, steps=2, seed=1):
    _, optim = _mods()
    opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=cls or optim.HipAdam)
    g = torch.Generator(device=DEV).manual_seed(seed)
    for _ in range(steps):
        for ps in m.get_param_groups().values():
            ps[0].grad = torch.randn(ps[0].shape, device=DEV, generator=g) * 1e-2
        opts.optimizer_step_all()
        opts.zero_grad_all()
    return opts


def _moments(m, opts):
    splat, _ = _mods()
    out = {}
    for grp, k in splat.GROUP_PARAMS.items():
        o = opts.optimizers[grp]
        st = o.state[o.param_groups[0]["params"][0]]
        out[k] = (st["exp_avg"], st["exp_avg_sq"])
    return out


def _steps(opts):
    return {grp: float(o.state[o.param_groups[0]["params"][0]]["step"]) for grp, o in opts.optimizers.items()}


def _run_both(n, seed, step, cls=None, **cfg_kw):
    """one refinement by the model (HIP) and by the restatement, from the same state and noise"""
    splat, _ = _mods()
    cfg = splat.ThermalSplatfactoModelConfig(**cfg_kw)
    p, stats = _random_state(n, seed, cfg)
    m = _model(p, seed=seed, **cfg_kw)
    opts = _optimizers(m, cls)
    params_in = {k: m.gauss_params[k].detach().clone() for k in NAMES}
    mom_in = {k: (a.clone(), b.clone()) for k, (a, b) in _moments(m, opts).items()}
    steps_in = _steps(opts)
    m.xys_grad_norm, m.vis_counts, m.max_2Dsize = (t.clone() for t in stats)
    m.last_size = SIZE
    m.step = step
    gen = torch.Generator(device=DEV)
    gen.set_state(m.noise_generator.get_state())
    m.refinement_after(opts, step)
    out, mom, info = rf.refine(params_in, mom_in, stats, SIZE, step, cfg, NUM_TRAIN_DATA,
                               lambda k: torch.randn((k, 3), device=DEV, generator=gen))
    return m, opts, out, mom, info, params_in, steps_in


def _assert_same(m, opts, out, mom):
    got_m = _moments(m, opts)
    for k in NAMES:
        got, ref = m.gauss_params[k].detach(), out[k]
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        if k in ("means", "scales"):  # child means and log-scales: 1e-6 relative (to the tensor's scale near 0); the copied rows bit for bit
            torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-6 * float(ref.abs().max()) if ref.numel() else 0.0)
        else:
            assert torch.equal(got, ref), k
        assert torch.equal(got_m[k][0], mom[k][0]) and torch.equal(got_m[k][1], mom[k][1]), k


def test_grad_stats_match_the_restatement():
    splat, _ = _mods()
    n = 50_000
    p = so.synth_gaussians(n, seed=1)
    m = _model(p, stop_split_at=15000)
    g = torch.Generator(device=DEV).manual_seed(2)
    stats = None
    m.step = 700
    for f in range(4):
        radii = torch.randint(0, 40, (n,), device=DEV, generator=g, dtype=torch.int32)
        radii[torch.rand(n, device=DEV, generator=g) < 0.3] = 0
        grad = torch.randn((n, 2), device=DEV, generator=g) * 1e-4
        size = (480, 640) if f % 2 else (1080, 1920)
        m.last_xys_grad, m.last_radii, m.last_size = grad, radii, size
        m.after_train(700)
        stats = rf.after_train(stats, grad, radii, size, 700, m.config)
        assert torch.equal(m.vis_counts, stats[1]) and torch.equal(m.max_2Dsize, stats[2]), f
        ulp = stats[0].abs() * 2.0**-23
        assert bool(((m.xys_grad_norm - stats[0]).abs() <= 2 * ulp).all()), f
        if f == 0:  # the first call: every Gaussian, visible or not
            assert torch.equal(m.vis_counts, torch.ones(n, device=DEV))
    m.step = 15000  # nothing after stop_split_at
    before = [t.clone() for t in (m.xys_grad_norm, m.vis_counts, m.max_2Dsize)]
    m.after_train(15000)
    assert all(torch.equal(a, b) for a, b in zip(before, (m.xys_grad_norm, m.vis_counts, m.max_2Dsize)))


@pytest.mark.parametrize("branch,step,kw", [
    ("densify", 600, {}),
    ("huge_and_screen", 3500, {}),
    ("after_screen_size", 4500, {}),
    ("cull_only", 15100, {}),
    ("opacity_reset", 3100, {}),
    ("no_cull_after_split", 15100, {"continue_cull_post_densification": False}),
    ("warmup", 500, {}),
])
def test_refinement_matches_the_restatement(branch, step, kw):
    m, opts, out, mom, info, params_in, steps_in = _run_both(100_000, 7, step, **kw)
    _assert_same(m, opts, out, mom)
    n_in, n_out = params_in["means"].shape[0], m.num_points
    if branch in ("densify", "huge_and_screen", "after_screen_size"):
        assert info["num_split"] > 0 and info["num_dup"] > 0 and bool((info["split"] & info["dup"]).any())
        assert m.last_refine_counts == (info["num_split"], int((~info["culled"][:n_in]).sum()),
                                        int((~info["culled"][n_in:n_in + m.config.n_split_samples * info["num_split"]]).sum()),
                                        int((~info["culled"][n_in + m.config.n_split_samples * info["num_split"]:]).sum()))
    if branch == "cull_only":
        assert n_out < n_in
    if branch in ("opacity_reset", "no_cull_after_split", "warmup"):
        assert n_out == n_in
    assert _steps(opts) == steps_in  # Adam step counts are kept
    assert m.xys_grad_norm is None or branch == "warmup"


@pytest.mark.parametrize("cls_name", ["HipAdam", "torch"])
def test_optimisers_follow_the_refinement(cls_name):
    _, optim = _mods()
    cls = optim.HipAdam if cls_name == "HipAdam" else torch.optim.Adam
    m, opts, out, mom, info, params_in, steps_in = _run_both(20_000, 9, 600, cls=cls)
    _assert_same(m, opts, out, mom)
    assert m.num_points != params_in["means"].shape[0]
    splat, _ = _mods()
    for grp, k in splat.GROUP_PARAMS.items():
        o = opts.optimizers[grp]
        p = o.param_groups[0]["params"][0]
        assert p is m.gauss_params[k] and opts.parameters[grp][0] is p
        st = o.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert len(o.state) == 1
    assert _steps(opts) == steps_in
    for ps in m.get_param_groups().values():
        ps[0].grad = torch.ones_like(ps[0]) * 1e-3
    opts.optimizer_step_all()
    assert all(v == steps_in[g] + 1 for g, v in _steps(opts).items())
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_hip_adam_matches_torch_adam_after_a_refinement():
    _, optim = _mods()
    runs = []
    for cls in (optim.HipAdam, torch.optim.Adam):
        m, opts, *_ = _run_both(20_000, 11, 600, cls=cls)
        g = torch.Generator(device=DEV).manual_seed(3)
        for ps in m.get_param_groups().values():
            ps[0].grad = torch.randn(ps[0].shape, device=DEV, generator=g) * 1e-2
        opts.optimizer_step_all()
        runs.append(m)
    for k in NAMES:
        a, b = runs[0].gauss_params[k].detach(), runs[1].gauss_params[k].detach()
        assert a.shape == b.shape
        assert float((a - b).abs().max()) <= 2e-6, k


def test_refinement_is_deterministic():
    a = _run_both(50_000, 13, 3500)
    b = _run_both(50_000, 13, 3500)
    for k in NAMES:
        assert torch.equal(a[0].gauss_params[k], b[0].gauss_params[k]), k
    ma, mb = _moments(a[0], a[1]), _moments(b[0], b[1])
    assert all(torch.equal(ma[k][0], mb[k][0]) and torch.equal(ma[k][1], mb[k][1]) for k in NAMES)


def test_nothing_qualifies_leaves_everything_bit_identical():
    splat, _ = _mods()
    n = 10_000
    p = so.synth_gaussians(n, seed=15)
    p["scales"] = torch.full((n, 3), math.log(0.02))  # large enough to split, small enough to keep
    p["opacities"] = torch.full((n, 1), 3.0)
    m = _model(p)
    opts = _optimizers(m)
    before = {k: m.gauss_params[k].detach().clone() for k in NAMES}
    mom = {k: (a.clone(), b.clone()) for k, (a, b) in _moments(m, opts).items()}
    m.xys_grad_norm, m.vis_counts, m.max_2Dsize = torch.zeros(n, device=DEV), torch.ones(n, device=DEV), torch.zeros(n, device=DEV)
    m.last_size, m.step = SIZE, 600
    m.refinement_after(opts, 600)
    assert m.last_refine_counts == (0, n, 0, 0)
    got = _moments(m, opts)
    for k in NAMES:
        assert torch.equal(m.gauss_params[k], before[k]) and torch.equal(got[k][0], mom[k][0]) and torch.equal(got[k][1], mom[k][1]), k


def test_everything_culled_leaves_a_renderable_empty_model():
    n = 5_000
    p = so.synth_gaussians(n, seed=16)
    p["opacities"] = torch.full((n, 1), -6.0)  # all transparent
    m = _model(p, background_color="white", background_thermal=0.25)
    opts = _optimizers(m)
    m.xys_grad_norm, m.vis_counts, m.max_2Dsize = torch.zeros(n, device=DEV), torch.ones(n, device=DEV), torch.zeros(n, device=DEV)
    m.last_size, m.step = SIZE, 600
    m.refinement_after(opts, 600)
    assert m.num_points == 0 and all(m.gauss_params[k].shape[0] == 0 for k in NAMES)
    cam = _camera(so.look_at_camera((2.5, 0.3, 0.6)), 60.0, 32.0, 24.0, 64, 48)
    out = m.get_outputs(cam)
    assert torch.equal(out["rgb"], torch.ones((48, 64, 3), device=DEV)) and torch.equal(out["thermal"], torch.full((48, 64, 1), 0.25, device=DEV))
    assert float(out["accumulation"].abs().max()) == 0.0
    tr = m.get_train_outputs(cam)
    (tr["rgb"].sum() + tr["thermal"].sum()).backward()
    assert m.last_xys_grad.shape == (0, 2)
    opts.optimizer_step_all()  # the optimisers step over empty parameters


def test_eval_render_between_backward_and_after_train_leaves_the_statistics_alone():
    p = so.synth_gaussians(3000, seed=17, extent=1.0)
    m = _model(p)
    m.step = 700
    W, H = 128, 96
    cam = _camera(so.look_at_camera((2.4, 0.5, 0.7)), sf.fov_focal(W), 64.0, 48.0, W, H)
    other = _camera(so.look_at_camera((-0.6, 2.3, 0.5)), 300.0, 160.0, 120.0, 320, 240)
    out = m.get_train_outputs(cam)
    (out["rgb"].mean() + out["thermal"].mean()).backward()
    grad, radii = m.last_xys_grad.clone(), m.last_radii.clone()
    m.get_outputs(other)  # a different camera and size
    m.after_train(700)
    ref = rf.after_train(None, grad, radii, (H, W), 700, m.config)
    assert torch.equal(m.vis_counts, ref[1]) and torch.equal(m.max_2Dsize, ref[2])
    assert bool(((m.xys_grad_norm - ref[0]).abs() <= 2 * ref[0].abs() * 2.0**-23).all())
    assert bool((m.max_2Dsize > 0).any())


def test_checkpoint_of_a_refined_model_loads_into_a_fresh_one():
    m, opts, *_ = _run_both(20_000, 19, 600)
    n = m.num_points
    assert n != 20_000
    fresh = _model(so.synth_gaussians(10, seed=1))
    fresh.load_state_dict(m.state_dict())
    assert fresh.num_points == n and fresh.step == 30000
    m.step = fresh.step
    cam = _camera(so.look_at_camera((2.4, 0.5, 0.7)), 110.0, 64.0, 48.0, 128, 96)
    a, b = m.get_outputs(cam), fresh.get_outputs(cam)
    for k in ("rgb", "thermal", "depth", "accumulation"):
        assert torch.equal(a[k], b[k]), k


def _fit(refine: bool, steps: int = 1000):
    """A few hundred Gaussians fitted to a synthetic RGB+T scene from three cameras through the training callbacks, L1 loss"""
    splat, optim = _mods()
    from nerfstudio_thermal_amd.model import TrainingCallbackLocation

    target = so.synth_gaussians(3000, seed=21, extent=1.0, scale_range=(-4.5, -3.0))
    W, H = 128, 96
    fx = sf.fov_focal(W)
    cams = [_camera(so.look_at_camera(e), fx, 64.0, 48.0, W, H) for e in ((2.4, 0.5, 0.7), (-0.6, 2.3, 0.5), (0.4, -2.2, 1.0))]
    tm = _model(target, sh_degree=3)
    tm.step = 10**6
    gts = [tm.get_outputs(c) for c in cams]
    n0 = 300
    g = torch.Generator().manual_seed(22)
    init = {"means": (torch.rand((n0, 3), generator=g) - 0.5) * 2.0, "scales": torch.full((n0, 3), math.log(0.08)),
            "quats": torch.nn.functional.normalize(torch.randn((n0, 4), generator=g), dim=-1), "opacities": torch.zeros((n0, 1)),
            "features_dc": torch.rand((n0, 3), generator=g) - 0.5, "features_rest": torch.zeros((n0, 15, 3)),
            "features_dc_thermal": torch.rand((n0, 1), generator=g) - 0.5, "features_rest_thermal": torch.zeros((n0, 15, 1))}
    m = _model(init, seed=23, sh_degree=3, sh_degree_interval=300, refine_every=50, warmup_length=100)
    m.num_train_data = len(cams)
    opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=optim.HipAdam)
    cbs = m.get_training_callbacks(opts)
    if not refine:
        cbs = cbs[:1]
    for step in range(steps):
        for cb in cbs:
            cb.run_callback_at_location(step, TrainingCallbackLocation.BEFORE_TRAIN_ITERATION)
        opts.zero_grad_all()
        i = step % len(cams)
        o = m.get_train_outputs(cams[i])
        loss = (o["rgb"] - gts[i]["rgb"]).abs().mean() + (o["thermal"] - gts[i]["thermal"]).abs().mean()
        loss.backward()
        opts.optimizer_step_all()
        opts.scheduler_step_all()
        for cb in cbs:
            cb.run_callback_at_location(step, TrainingCallbackLocation.AFTER_TRAIN_ITERATION)
    with torch.no_grad():
        final = sum(float((m.get_outputs(c)["rgb"] - gt["rgb"]).abs().mean() + (m.get_outputs(c)["thermal"] - gt["thermal"]).abs().mean())
                    for c, gt in zip(cams, gts)) / len(cams)
    return final, m.num_points


def test_training_with_refinement_beats_training_without():
    l_ref, n_ref = _fit(True)
    l_plain, n_plain = _fit(False)
    print(f"end to end: L1 with refinement {l_ref:.4f} ({n_ref} Gaussians), without {l_plain:.4f} ({n_plain} Gaussians)")
    assert n_plain == 300 and n_ref != 300
    assert math.isfinite(l_ref) and l_ref < 0.9 * l_plain, (l_ref, l_plain)


def test_1080p_one_million_gaussians_refinement_smoke():
    from nerfstudio_thermal_amd import synth

    n = 1_000_000
    p = synth.synth_gaussians(n, seed=11, extent=1.5, scale_range=(-5.5, -3.5))
    m = _model(p)
    opts = _optimizers(m, steps=1)
    cam = _camera(synth.look_at_camera((3.2, 0.5, 0.8)), 1400.0, 960.0, 540.0, 1920, 1080)
    m.step = 600
    out = m.get_train_outputs(cam)
    (out["rgb"].mean() + out["thermal"].mean()).backward()
    m.after_train(600)
    assert m.last_size == (1080, 1920) and bool(torch.isfinite(m.xys_grad_norm).all())
    # then statistics of which about 10 % split and 10 % are duplicated
    g = torch.Generator(device=DEV).manual_seed(4)
    high = torch.rand(n, device=DEV, generator=g) < 0.2
    small = torch.rand(n, device=DEV, generator=g) < 0.5
    with torch.no_grad():
        m.gauss_params["scales"][small] = math.log(0.005)
        m.gauss_params["scales"][~small] = math.log(0.03)
    m.xys_grad_norm = torch.where(high, 1e-3, 1e-8).float()
    m.vis_counts = torch.ones(n, device=DEV)
    m.refinement_after(opts, 600)
    ns, no, nc, nd = m.last_refine_counts
    print(f"1080p / 1M: {ns} split, {no} originals, {nc} children, {nd} duplicates kept -> {m.num_points}")
    assert m.num_points == no + nc + nd and 0.08 * n < ns < 0.12 * n and 0.08 * n < nd < 0.12 * n
    for k in NAMES:
        assert m.gauss_params[k].shape[0] == m.num_points and bool(torch.isfinite(m.gauss_params[k]).all()), k
    for (a, b) in _moments(m, opts).values():
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
