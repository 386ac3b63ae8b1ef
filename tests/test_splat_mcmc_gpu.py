"""The MCMC densification strategy on the GPU: tn_splat_mcmc_relocate / tn_splat_mcmc_noise against the float64 restatement
(splat_mcmc_functional.py), and ThermalSplatfactoModel's strategy "mcmc" through its training callbacks.

Tolerances.  Relocation values: 1 float32 ulp of the float64 restatement rounded to float32 -- the kernel evaluates in double and rounds once, so
only a rounding tie flipped by the last bit of a device pow / log can differ.  Noise: 8 x the largest error of the same formula in plain-torch
float32 against the float64 restatement on the same inputs, both relative to the case's largest |delta means| (printed; recorded in
profiles/splat_mcmc.md)."""
import functools
import math

import numpy as np
import pytest
import torch

import splat_functional as sf
import splat_mcmc_functional as mf
import splat_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIN_OPACITY = 0.005
MULTS = (1, 2, 3, 51, 52, 70)  # how often the hand-picked sources are drawn: ratios 2, 3, 4, 52, 53, 71 -- the clamp at 51 is crossed
MULT_ROWS = (1, 2, 3, 4, 6, 0)  # ... and their rows (row 6: opacity 1 - 1e-6, row 0: 1e-4)
OPACITIES = (1e-4, 0.004, 0.05, 0.3, 0.7, 0.99, 1 - 1e-6)


def _mods():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import optim, splat

    return splat, optim


def _logit(o):
    return math.log(o / (1.0 - o))


def _tensors(rows: int, K: int, sep: bool, seed: int):
    """rows random Gaussians as float32 numpy arrays (opacities cycling through OPACITIES; separate: o > o_th, o < o_th and exact ties) and
    random Adam moments"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    i = np.arange(rows)
    p = {"means": f(rows, 3), "scales": rng.uniform(-6.0, 0.5, (rows, 3)).astype(np.float32), "quats": f(rows, 4),
         "opacities": np.array([_logit(OPACITIES[j % 7]) for j in i], dtype=np.float32).reshape(rows, 1), "features_dc": f(rows, 3),
         "features_rest": f(rows, K, 3), "features_dc_thermal": f(rows, 1), "features_rest_thermal": f(rows, K, 1)}
    if sep:
        th = np.array([_logit(OPACITIES[(3 * j + 1) % 7]) for j in i], dtype=np.float32).reshape(rows, 1)
        tie = i % 5 == 2
        th[tie] = p["opacities"][tie]
        p["opacities_thermal"] = th
    m1 = {k: f(*v.shape) for k, v in p.items()}
    m2 = {k: f(*v.shape) ** 2 for k, v in p.items()}
    return p, m1, m2


def _draws(N: int, grown: bool):
    """(src, dst, number of rows of the tensors).  grown (the add phase): N draws into rows appended behind the N Gaussians.  Otherwise (the
    relocate phase): draws into the last rows of the N Gaussians themselves, which are no sources."""
    if N == 1:
        assert grown
        return np.array([0]), np.array([1]), 2
    M = N if grown else (479 if N >= 1000 else 209)
    src = [r for m, r in zip(MULTS, MULT_ROWS) for _ in range(m)]
    src += list(range(7, 7 + M - len(src)))  # single draws of further sources
    rng = np.random.default_rng(N)
    src = rng.permutation(np.array(src, dtype=np.int64))
    rows = N + M if grown else N
    dst = np.arange(rows - M, rows, dtype=np.int64)
    assert src.max() < dst.min() and len(src) == len(dst) == M
    return src, dst, rows


def _ulp_ok(got32: np.ndarray, ref64: np.ndarray) -> bool:
    ref32 = ref64.astype(np.float32)
    return bool(np.all(np.abs(got32.astype(np.float64) - ref32.astype(np.float64)) <= np.spacing(np.abs(ref32)).astype(np.float64)))


CASES = [(N, K, sep, grown) for N in (1, 255, 257, 1000) for K in (0, 15) for sep in (False, True) for grown in (True, False) if grown or N > 1]


@pytest.mark.parametrize("N,K,sep,grown", CASES)
def test_relocation_matches_the_restatement(N, K, sep, grown):
    splat, _ = _mods()
    src, dst, rows = _draws(N, grown)
    p, m1, m2 = _tensors(rows, K, sep, seed=7 * N + K + sep)
    if grown:  # rows appended by the caller: zero values, zero moments
        for d in (p, m1, m2):
            for v in d.values():
                v[N:] = 0.0
    names = mf.NAMES_SEP if sep else mf.NAMES
    ref, ref1, ref2 = mf.relocate(p, m1, m2, src, dst, MIN_OPACITY)

    def run():
        t = [torch.from_numpy(p[k]).to(DEV) for k in names]
        a = [torch.from_numpy(m1[k]).to(DEV) for k in names]
        b = [torch.from_numpy(m2[k]).to(DEV) for k in names]
        splat.mcmc_relocate(t, a, b, torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV), MIN_OPACITY)
        torch.cuda.synchronize()
        return [{k: v.cpu().numpy() for k, v in zip(names, ts)} for ts in (t, a, b)]

    got, got1, got2 = run()
    drawn = np.unique(src)
    named = np.zeros(rows, dtype=bool)
    named[drawn] = named[dst] = True
    fresh = ("scales", "opacities", "opacities_thermal")
    for k in names:
        if got[k].size == 0:
            continue
        if k in fresh:  # the relocation values, on the sources and on their copies
            assert _ulp_ok(got[k][drawn], ref[k][drawn]), k
        else:  # sources keep every other value
            assert np.array_equal(got[k][drawn], p[k][drawn]), k
        assert np.array_equal(got[k][dst], got[k][src]), k  # every destination row is bitwise its source's row
        assert np.array_equal(got[k][~named], p[k][~named]), k  # rows not named: untouched
        for g, r, m in ((got1, ref1, m1), (got2, ref2, m2)):
            assert not g[k][drawn].any(), k  # source moments: exactly 0
            assert np.array_equal(g[k][dst], m[k][dst]), k  # destination moments stay (the add phase's appended rows: zero)
            assert np.array_equal(g[k][~named], m[k][~named]), k
            assert np.array_equal(g[k], r[k].astype(np.float32)), k
        if grown:
            assert not got1[k][N:].any() and not got2[k][N:].any(), k
    again = run()
    for a, b in zip((got, got1, got2), again):
        for k in names:
            assert np.array_equal(a[k], b[k]), k  # bit-reproducible


def test_relocation_without_adam_state_and_with_no_draws():
    splat, _ = _mods()
    src, dst, rows = _draws(255, False)
    p, _, _ = _tensors(rows, 15, True, seed=3)
    ref, _, _ = mf.relocate(p, {}, {}, src, dst, MIN_OPACITY)
    t = [torch.from_numpy(p[k]).to(DEV) for k in mf.NAMES_SEP]
    none = [None] * 9
    splat.mcmc_relocate(t, none, none, torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV), MIN_OPACITY)
    for k, v in zip(mf.NAMES_SEP, t):
        assert _ulp_ok(v.cpu().numpy(), ref[k]), k
    before = [v.clone() for v in t]
    empty = torch.empty(0, dtype=torch.int64, device=DEV)
    splat.mcmc_relocate(t, none, none, empty, empty, MIN_OPACITY)
    assert all(torch.equal(a, b) for a, b in zip(before, t))
    with pytest.raises(ValueError):
        splat.mcmc_relocate(t[:7], none[:7], none[:7], empty, empty, MIN_OPACITY)
    with pytest.raises(ValueError):
        splat.mcmc_relocate([v.cpu() for v in t], none, none, torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int64), MIN_OPACITY)


# ------------------------------------------------------------------------------------------------ noise
def _noise_inputs(N: int, sep: bool):
    rng = np.random.default_rng(100 + N + sep)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    i = np.arange(N)
    scales = np.log(10.0 ** rng.uniform(-3.0, 0.0, (N, 3))).astype(np.float32)  # exp(scales) spread over three decades
    quats = (f(N, 4) * rng.uniform(0.2, 5.0, (N, 1))).astype(np.float32)  # unnormalised
    # row 0 and every third row: dead (o < 0.005, g about 0.5); then o_vis >= 0.5 (g < 1e-21: must not move); then in between
    kinds = i % 3
    op = np.where(kinds == 0, rng.uniform(-9.0, -5.4, N), np.where(kinds == 1, rng.uniform(0.0, 6.0, N), rng.uniform(-5.0, -0.5, N)))
    op = op.astype(np.float32).reshape(N, 1)
    th = None
    if sep:  # the thermal opacity is the visible one on half of the visible rows, and both are low on the dead rows
        th = np.where(kinds == 0, rng.uniform(-9.0, -5.4, N), rng.uniform(-8.0, -0.5, N)).astype(np.float32).reshape(N, 1)
        swap = (kinds == 1) & (i % 2 == 0)
        op[swap], th[swap] = th[swap], op[swap].copy()
    return {"means": f(N, 3), "scales": scales, "quats": quats, "opacities": op, "opacities_thermal": th, "z": f(N, 3)}


@pytest.mark.parametrize("sep", [False, True])
@pytest.mark.parametrize("N", [1, 255, 257, 1000])
def test_noise_matches_the_restatement(N, sep):
    splat, _ = _mods()
    scaler = 5e5 * 1.6e-4  # the defaults: noise_lr x the means' initial learning rate
    x = _noise_inputs(N, sep)
    d = {k: (torch.from_numpy(v).to(DEV) if v is not None else None) for k, v in x.items()}
    ref = mf.noise_delta(x["scales"], x["quats"], x["opacities"], x["z"], scaler, x["opacities_thermal"])
    scale = np.abs(ref).max()
    assert scale > 0
    yard = mf.noise_delta_torch(d["scales"], d["quats"], d["opacities"], d["z"], scaler, d["opacities_thermal"]).cpu().numpy()
    err_torch = np.abs(yard.astype(np.float64) - ref).max() / scale
    keep = {k: d[k].clone() for k in ("scales", "quats", "opacities", "z")}
    zero = torch.zeros((N, 3), device=DEV)  # from zero means the result IS the kernel's delta
    splat.mcmc_noise(zero, d["scales"], d["quats"], d["opacities"], d["z"], scaler, d["opacities_thermal"])
    err = np.abs(zero.cpu().numpy().astype(np.float64) - ref).max() / scale
    print(f"noise N={N} {'separate' if sep else 'shared'}: kernel error {err:.3e}, plain-torch float32 error {err_torch:.3e} (relative to max |delta| {scale:.3e})")
    assert err <= 8 * err_torch, (err, err_torch)
    means = d["means"].clone()
    splat.mcmc_noise(means, d["scales"], d["quats"], d["opacities"], d["z"], scaler, d["opacities_thermal"])
    got = means.cpu().numpy()
    visible = mf.visible_opacity(x["opacities"], x["opacities_thermal"]) >= 0.5
    assert np.array_equal(got[visible], x["means"][visible])  # g < 1e-21: bit-identical
    if N > 1:
        assert visible.any() and (got[~visible] != x["means"][~visible]).any()
    np.testing.assert_allclose(got, mf.noise(x["means"], x["scales"], x["quats"], x["opacities"], x["z"], scaler, x["opacities_thermal"]),
                               rtol=0, atol=2.0 ** -23 * (np.abs(x["means"]).max() + scale) + 8 * err_torch * scale)  # + the sum's one rounding
    for k, v in keep.items():
        assert torch.equal(v, d[k]), k
    if sep:
        assert torch.equal(d["opacities_thermal"], torch.from_numpy(x["opacities_thermal"]).to(DEV))


# ------------------------------------------------------------------------------------------------ the model
W, H = 96, 72


def _camera(eye):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    fx = sf.fov_focal(W)
    return PinholeCamera(so.look_at_camera(eye), fx, fx, W / 2, H / 2, W, H)


def _model(params, seed=0, **cfg_kw):
    splat, _ = _mods()
    m = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(**cfg_kw), num_points=4, device=DEV, seed=seed, num_train_data=3)
    m.load_gaussians(params)
    return m


@functools.lru_cache(maxsize=None)
def _scene():
    cams = [_camera(e) for e in ((2.4, 0.5, 0.7), (-0.6, 2.3, 0.5), (0.4, -2.2, 1.0))]
    tm = _model(so.synth_gaussians(400, seed=31, extent=1.0, scale_range=(-3.5, -2.0)), sh_degree=3)
    tm.step = 10 ** 6
    gts = [tm.get_outputs(c)["rgb"].clone() for c in cams]
    return cams, gts


def _iteration(m, opts, cbs, step, cam, gt, after_cb=None):
    from nerfstudio_thermal_amd.model import TrainingCallbackLocation as L

    for cb in cbs:
        cb.run_callback_at_location(step, L.BEFORE_TRAIN_ITERATION)
    opts.zero_grad_all()
    loss = m.get_loss_dict(m.get_train_outputs(cam), {"image": gt, "is_thermal": False})
    functools.reduce(torch.add, loss.values()).backward()
    opts.optimizer_step_all()
    opts.scheduler_step_all()
    for i, cb in enumerate(cbs):
        cb.run_callback_at_location(step, L.AFTER_TRAIN_ITERATION)
        if after_cb is not None:
            after_cb(i)
    return loss


def _check_optimizers(m, opts, splat):
    n = m.num_points
    for grp, k in m.group_params.items():
        p = m.gauss_params[k]
        o = opts.optimizers[grp]
        assert p.shape[0] == n, k
        assert o.param_groups[0]["params"][0] is p and opts.parameters[grp][0] is p, k
        assert len(o.state) == 1 and p in o.state, k
        st = o.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape, k


@functools.lru_cache(maxsize=None)
def _train(mode: str, run: int):
    """8 training steps of a 300-Gaussian scene through the callbacks (run: a cache key, so that a second, identical run exists)"""
    splat, optim = _mods()
    cams, gts = _scene()
    m = _model(so.synth_gaussians(300, seed=32, extent=1.0, scale_range=(-3.5, -2.0)), seed=5, strategy="mcmc", warmup_length=0, refine_every=2,
               max_gs_num=340, thermal_opacity_mode=mode, sh_degree=3)
    opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=optim.HipAdam)
    cbs = m.get_training_callbacks(opts)
    assert len(cbs) == 4
    rec = {"counts": [], "refine_counts": [], "dead_row_ok": None, "losses": []}
    for step in range(8):
        if step == 2:  # a Gaussian forced dead before a refine step
            with torch.no_grad():
                m.gauss_params["opacities"][5] = -10.0
                if mode == "separate":
                    m.gauss_params["opacities_thermal"][5] = -10.0

        def after_cb(i, step=step):
            if i == 2 and step in (2, 4, 6):  # straight after the refinement callback, before the noise
                _check_optimizers(m, opts, splat)
                rec["refine_counts"].append(m.last_refine_counts)
                assert m.last_radii is None and m.xys_grad_norm is None
                if step == 2:
                    gp = m.gauss_params
                    twin = ((gp["means"] == gp["means"][5]).all(dim=1)).nonzero().reshape(-1).tolist()
                    others = [j for j in twin if j != 5]
                    # (the growth that follows the relocation may have drawn one of the twins again: opacity and scale are compared below, in
                    # test_a_dead_gaussian_is_relocated_onto_a_live_one, where nothing grows)
                    carried = [k for k in m.param_names if k not in ("scales", "opacities", "opacities_thermal")]
                    same = [j for j in others if all(torch.equal(gp[k][j], gp[k][5]) for k in carried)]
                    rec["dead_row_ok"] = bool(same) and all(float(m._visible_opacity()[j]) > MIN_OPACITY for j in same + [5])

        loss = _iteration(m, opts, cbs, step, cams[step % 3], gts[step % 3], after_cb)
        assert m.last_xys_grad is None or m.last_xys_grad.shape[0] in (300, 315, 330, 340)
        rec["counts"].append(m.num_points)
        rec["losses"].append({k: float(v.detach()) for k, v in loss.items()})
    m.step_cb(8)
    m.refinement_after(opts, 8)  # one more refinement at the cap: nothing is added
    rec["counts"].append(m.num_points)
    rec["final"] = {k: m.gauss_params[k].detach().clone() for k in m.param_names}
    rec["moments"] = {g: (o.state[o.param_groups[0]["params"][0]]["exp_avg"].clone(), o.state[o.param_groups[0]["params"][0]]["exp_avg_sq"].clone())
                      for g, o in opts.optimizers.items()}
    return rec


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_training_grows_to_the_budget_and_stays(mode):
    rec = _train(mode, 0)
    assert rec["counts"] == [300, 300, 315, 315, 330, 330, 340, 340, 340]
    assert max(rec["counts"]) <= 340
    assert [c[2] for c in rec["refine_counts"]] == [15, 15, 10]
    assert rec["refine_counts"][0][0] >= 1 and rec["refine_counts"][0][1] == rec["refine_counts"][0][0]  # the forced-dead row was relocated
    assert rec["dead_row_ok"] is True
    for losses in rec["losses"]:
        assert {"main_loss", "scale_reg", "mcmc_opacity_reg", "mcmc_scale_reg"} <= set(losses)
        assert all(math.isfinite(v) for v in losses.values()), losses
    assert all(bool(torch.isfinite(v).all()) for v in rec["final"].values())


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_two_runs_with_one_seed_are_bit_identical(mode):
    a, b = _train(mode, 0), _train(mode, 1)
    assert a is not b and a["counts"] == b["counts"]
    for k in a["final"]:
        assert torch.equal(a["final"][k], b["final"][k]), k
    for g in a["moments"]:
        assert torch.equal(a["moments"][g][0], b["moments"][g][0]) and torch.equal(a["moments"][g][1], b["moments"][g][1]), g


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_loss_regularisers_reach_opacities_and_scales(mode):
    cams, gts = _scene()
    m = _model(so.synth_gaussians(300, seed=32, extent=1.0, scale_range=(-3.5, -2.0)), strategy="mcmc", thermal_opacity_mode=mode, sh_degree=3)
    gp = m.gauss_params
    loss = m.get_loss_dict(m.get_train_outputs(cams[0]), {"image": gts[0], "is_thermal": False})
    o, s = torch.sigmoid(gp["opacities"]).mean(), torch.exp(gp["scales"]).mean()
    if mode == "separate":
        o = o + torch.sigmoid(gp["opacities_thermal"]).mean()
    torch.testing.assert_close(loss["mcmc_opacity_reg"], 0.01 * o)
    torch.testing.assert_close(loss["mcmc_scale_reg"], 0.01 * s)
    g_o = torch.autograd.grad(loss["mcmc_opacity_reg"], [gp[k] for k in (("opacities", "opacities_thermal") if mode == "separate" else ("opacities",))],
                              retain_graph=True)
    (g_s,) = torch.autograd.grad(loss["mcmc_scale_reg"], [gp["scales"]], retain_graph=True)
    assert all(bool(torch.isfinite(g).all()) and bool((g > 0).all()) for g in g_o) and bool(torch.isfinite(g_s).all()) and bool((g_s > 0).all())


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_a_dead_gaussian_is_relocated_onto_a_live_one(mode):
    _, optim = _mods()
    m = _model(so.synth_gaussians(300, seed=34, extent=1.0), seed=2, strategy="mcmc", warmup_length=0, refine_every=2, max_gs_num=300,
               thermal_opacity_mode=mode, sh_degree=3)
    opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=optim.HipAdam)
    g = torch.Generator(device=DEV).manual_seed(1)
    for ps in m.get_param_groups().values():
        ps[0].grad = torch.randn(ps[0].shape, device=DEV, generator=g) * 1e-2
    opts.optimizer_step_all()
    opts.zero_grad_all()
    with torch.no_grad():
        m.gauss_params["opacities"][5] = -10.0
        if mode == "separate":
            m.gauss_params["opacities_thermal"][5] = -10.0
            m.gauss_params["opacities"][6] = -10.0  # dead in RGB alone: visible in thermal, so it stays
    before = {k: m.gauss_params[k].detach().clone() for k in m.param_names}
    params = {k: m.gauss_params[k] for k in m.param_names}
    m.step_cb(2)
    m.refinement_after(opts, 2)
    assert m.last_refine_counts == (1, 1, 0) and m.num_points == 300
    gp = m.gauss_params
    assert all(gp[k] is params[k] for k in m.param_names)  # relocation alone works in place: the optimisers keep their parameters
    twins = [j for j in range(300) if j != 5 and all(torch.equal(gp[k][j], gp[k][5]) for k in m.param_names)]
    assert len(twins) == 1
    j = twins[0]
    assert float(m._visible_opacity()[j]) > MIN_OPACITY
    ref = mf.relocation_value(float(before["opacities"][j]), before["scales"][j].cpu().numpy(), 2, MIN_OPACITY,
                              float(before["opacities_thermal"][j]) if mode == "separate" else None)
    assert _ulp_ok(gp["opacities"][j].detach().cpu().numpy(), np.array([ref[0]])) and _ulp_ok(gp["scales"][j].detach().cpu().numpy(), ref[2])
    rest = [i for i in range(300) if i not in (5, j)]
    for k in m.param_names:
        assert torch.equal(gp[k].detach()[rest], before[k][rest]), k
        o = opts.optimizers[{v: g_ for g_, v in m.group_params.items()}[k]]
        st = o.state[gp[k]]
        assert not st["exp_avg"][j].any() and not st["exp_avg_sq"][j].any() and st["exp_avg"][rest].any(), k
        assert float(st["step"]) == 1.0


def test_without_noise_a_step_moves_the_means_as_the_default_strategy_does():
    _, optim = _mods()
    cams, gts = _scene()
    ends = []
    for kw in ({"strategy": "mcmc", "noise_lr": 0.0}, {"strategy": "default"}):
        m = _model(so.synth_gaussians(300, seed=32, extent=1.0, scale_range=(-3.5, -2.0)), seed=5, warmup_length=0, refine_every=2, sh_degree=3, **kw)
        opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=optim.HipAdam)
        start = m.means.detach().clone()
        _iteration(m, opts, m.get_training_callbacks(opts), 1, cams[0], gts[0])  # step 1: no refinement under either strategy
        assert m.num_points == 300 and not torch.equal(start, m.means.detach())
        ends.append(m.means.detach().clone())
    assert torch.equal(ends[0], ends[1])


def test_the_noise_moves_only_faint_gaussians_and_stops_at_stop_split_at():
    _, optim = _mods()
    p = so.synth_gaussians(300, seed=33, extent=1.0)
    p["opacities"][:150] = -8.0
    p["opacities"][150:] = 2.0
    m = _model(p, seed=1, strategy="mcmc", stop_split_at=10)
    opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=optim.HipAdam)
    start = m.means.detach().clone()
    m.step_cb(3)
    m.mcmc_noise_after(opts, 3)
    end = m.means.detach()
    assert torch.equal(end[150:], start[150:]) and bool((end[:150] != start[:150]).any(dim=1).all())
    assert not opts.optimizers["xyz"].state  # Adam state untouched
    m.step_cb(10)
    before = m.means.detach().clone()
    m.mcmc_noise_after(opts, 10)
    assert torch.equal(before, m.means.detach())


def test_the_budget_is_checked_at_construction():
    splat, _ = _mods()
    cfg = splat.ThermalSplatfactoModelConfig(strategy="mcmc", max_gs_num=10)
    with pytest.raises(ValueError):
        splat.ThermalSplatfactoModel(cfg, num_points=11, device=DEV)
    xyz = torch.rand((11, 3))
    with pytest.raises(ValueError):
        splat.ThermalSplatfactoModel(cfg, device=DEV, seed_points=(xyz, torch.zeros((11, 3), dtype=torch.uint8)))
    assert splat.ThermalSplatfactoModel(cfg, num_points=10, device=DEV).num_points == 10
    assert splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(max_gs_num=10), num_points=11, device=DEV).num_points == 11  # "default": no budget


def test_the_default_strategy_is_unchanged():
    _, optim = _mods()
    cams, gts = _scene()
    m = _model(so.synth_gaussians(300, seed=32, extent=1.0), sh_degree=3)
    assert m.config.strategy == "default" and not m.mcmc
    opts = optim.Optimizers(m.get_param_groups(), optim.SPLAT_OPTIMIZERS, optimizer_cls=optim.HipAdam)
    cbs = m.get_training_callbacks(opts)
    assert len(cbs) == 3 and cbs[1].func == m.after_train and cbs[2].update_every_num_iters == m.config.refine_every
    loss = m.get_loss_dict(m.get_train_outputs(cams[0]), {"image": gts[0], "is_thermal": False})
    assert set(loss) == {"main_loss", "scale_reg"}
    m.step_cb(3)
    m.mcmc_noise_after(opts, 3)  # not the strategy: nothing happens
