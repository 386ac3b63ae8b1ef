"""The separate thermal opacity on the GPU (thermal_opacity_mode "separate": the thermal groups of the entry points of tn_splat.hip through
ThermalSplatfactoModel) against the float64 restatement tests/splat_sep_functional.py.

Scenes (ssf.awkward_scene, ~300 Gaussians, frames of 40 x 24 and 33 x 17: partial tiles and quadrants): a tile whose list is longer than one
256-record batch, an opaque stack on which the RGB chain hits its 1e-4 stop while the thermal chain runs on (and the reverse), Gaussians below
1/255 in one spectrum and ~0.99 in the other (present only through the larger opacity's box); both raster modes, sigmoid colours and degree 3.
tests/test_splat_separate_cpu.py checks on the restatement that the scenes do have these properties.

Tolerance rule (the splat forward test's, tests/test_splat_forward_gpu.py): the kernel's error against float64 is at most TOL_FACTOR = 8 times
the float32 restatement's own error against float64 on the same pixels / entries -- measured here on the case itself, and never less than one
float32 epsilon of the output's scale, below which neither float32 computation can be told from the other.  Pixels and Gaussians the float64
walk flags (a decision within 1e-4 of the 1/255 gate, the 0.999 clamp, the 1e-4 stop or an output clamp) are left out; at most 1 % of them."""
import ctypes as C
import functools

import pytest
import torch

import splat_functional as sf
import splat_oracle as so
import splat_refine_functional as rf  # noqa: F401
import splat_sep_functional as ssf

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FACTOR = 8.0
EPS = 2.0 ** -23
CASES = ssf.CASES
IMAGES = (("rgb", 3), ("thermal", 1), ("accumulation", 1), ("accumulation_thermal", 1))


def _model(params, sh_degree, mode="classic", sep="separate", **kw):
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

    cfg = ThermalSplatfactoModelConfig(sh_degree=sh_degree, sh_degree_interval=1, rasterize_mode=mode, background_thermal=0.3, thermal_opacity_mode=sep, **kw)
    m = ThermalSplatfactoModel(cfg, num_points=4, device=DEV)
    m.load_gaussians(params)
    m.step = 10**6
    return m


def _view(W, H):
    from nerfstudio_thermal_amd.splat import PinholeCamera

    c2w, fx, cx, cy = so.look_at_camera((2.3, 0.4, 0.6)), sf.fov_focal(W), W / 2 - 0.5, H / 2 + 0.25
    return (c2w, fx, fx, cx, cy, W, H), PinholeCamera(c2w, fx, fx, cx, cy, W, H)


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


@functools.lru_cache(maxsize=None)
def reference(case):
    """Float64 and float32 restatement of one case, computed once: images, gradients under one random upstream image per output, flags."""
    W, H, mode, sh, rev, seed = case
    p = ssf.awkward_scene(300, seed, sh, reverse=rev)
    view, _ = _view(W, H)
    deg = sh if sh > 0 else -1
    gen = torch.Generator().manual_seed(seed)
    w = {k: torch.randn(H, W, c, generator=gen, dtype=torch.float64) for k, c in IMAGES}
    res = {}
    for dt in (torch.float64, torch.float32):
        leaves = {k: v.to(dt).requires_grad_(True) for k, v in p.items()}
        out = ssf.render(leaves, *view, sh_degree_to_use=deg, rasterize_mode=mode, background_thermal=0.3, with_depth=True)
        out["xys"].retain_grad()
        if dt == torch.float64:
            keep = (~out["flag_pixels"])[..., None]
            w = {k: v * keep for k, v in w.items()}
        sum((out[k] * w[k].to(dt)).sum() for k in w).backward()
        grads = {k: leaves[k].grad.double() for k in ssf.PARAM_NAMES}
        grads["xys"] = out["xys"].grad.double()
        res[dt] = ({k: v.detach().double() for k, v in out.items() if k in dict(IMAGES) or k == "depth"}, grads, out)
    return p, w, res[torch.float64], res[torch.float32]


def _grads(m, cam, w):
    m.zero_grad(set_to_none=True)
    out = m.get_train_outputs(cam)
    sum((out[k] * w[k].float().to(DEV)).sum() for k in w).backward()
    g = {k: m.gauss_params[k].grad.detach().cpu().clone() for k in m.param_names}
    g["xys"] = m.last_xys_grad.detach().cpu().clone()
    return g, out


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-sh{c[3]}-{'rev' if c[4] else 'fwd'}")
def test_forward_and_backward_match_the_float64_restatement(case):
    W, H, mode, sh, rev, seed = case
    p, w, (img64, g64, out64), (img32, g32, _) = reference(case)
    _, cam = _view(W, H)
    m = _model(p, sh, mode)
    hip, tr = _grads(m, cam, w)
    ev = m.get_outputs(cam)
    flag = out64["flag_pixels"]
    share = float(flag.float().mean())
    print(f"near-threshold pixels left out: {int(flag.sum())} of {flag.numel()} ({100 * share:.2f} %); tile lists up to {int(out64['contributors_per_tile'].max())}")
    assert share <= 0.01
    assert m.last_num_intersections > 256 and float(img64["accumulation"].max()) > 0.9 and float(img64["accumulation_thermal"].max()) > 0.9
    ok = ~flag
    for k in ("rgb", "thermal", "accumulation", "accumulation_thermal", "depth"):
        ref, f32 = img64[k][ok], img32[k][ok]
        floor = max(_amax(f32 - ref), EPS * _amax(ref))
        for name, out in (("eval", ev), ("train", tr)):
            err = _amax(out[k].detach().cpu().double()[ok] - ref)
            print(f"{k} {name}: err {err:.2e}, float32 restatement {floor:.2e} ({err / floor:.1f}x)")
            assert err <= TOL_FACTOR * floor, (k, name, err, floor)
        assert torch.equal(tr[k].detach(), ev[k]), k  # the training render is the eval render, bit for bit
    radii_hip = m.last_projection["radii"].cpu()
    # flagged pixels carry no upstream gradient, so a decision float32 takes the other way there moves nothing; Gaussians are left out only for
    # decisions of their own: a view-space position on the frustum clamp, a knife-edge radius
    pj = out64["projection"]
    excl = (pj["near_clamp"] & pj["ok"]) | ((radii_hip > 0) != (pj["radii"] > 0))
    print(f"near-threshold Gaussians left out: {int(excl.sum())} of {excl.numel()}")
    assert int(excl.sum()) <= 0.01 * excl.numel()
    for k in list(ssf.PARAM_NAMES) + ["xys"]:
        a, b, c = hip[k].double()[~excl], g64[k][~excl], g32[k][~excl]
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), k
        scale = _amax(b)
        if scale == 0.0:
            assert _amax(a) == 0.0, k
            continue
        floor = max(_amax(c - b), EPS * scale)
        err = _amax(a - b)
        print(f"d {k}: err {err:.2e}, float32 restatement {floor:.2e} ({err / floor:.1f}x), scale {scale:.2e}")
        assert err <= TOL_FACTOR * floor, (k, err, floor)
    assert _amax(hip["opacities_thermal"]) > 0 and _amax(hip["opacities"]) > 0
    for k in ssf.PARAM_NAMES:
        assert _amax(hip[k][radii_hip == 0]) == 0.0, k


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_equal_opacities_are_bit_equal_to_shared_mode(mode):
    W, H, _, sh, rev, seed = CASES[0]
    p = ssf.shared_params(ssf.awkward_scene(300, seed, sh, reverse=rev))
    view, cam = _view(W, H)
    shared, sep = _model(p, sh, mode, sep="shared"), _model(p, sh, mode)  # load_gaussians starts opacities_thermal as a copy of opacities
    assert torch.equal(sep.gauss_params["opacities_thermal"], sep.gauss_params["opacities"])
    gen = torch.Generator().manual_seed(7)
    w = {k: torch.randn(H, W, c, generator=gen, dtype=torch.float64) for k, c in IMAGES[:3]}
    gs, outs = _grads(shared, cam, w)
    w_sep = {**w, "accumulation": 0.25 * w["accumulation"], "accumulation_thermal": 0.75 * w["accumulation"]}  # the same total on equal images
    gp, outp = _grads(sep, cam, w_sep)
    for a, b in ((outs, outp), (shared.get_outputs(cam), sep.get_outputs(cam))):
        for k in ("rgb", "thermal", "accumulation", "depth"):
            assert torch.equal(a[k].detach(), b[k].detach()), k
        assert torch.equal(b["accumulation_thermal"].detach(), b["accumulation"].detach())
        assert "accumulation_thermal" not in a
    # the two opacity gradients add up to the shared one; the bound: 8 x the float32 restatement's error on the shared gradient (never below eps)
    res = {}
    for dt in (torch.float64, torch.float32):
        leaves = {k: v.to(dt).requires_grad_(True) for k, v in p.items()}
        o = sf.render(leaves, *view, sh_degree_to_use=sh if sh > 0 else -1, rasterize_mode=mode, background_thermal=0.3)
        sum((o[k] * w[k].to(dt)).sum() for k in w).backward()
        res[dt] = leaves["opacities"].grad.double()
    floor = max(_amax(res[torch.float32] - res[torch.float64]), EPS * _amax(res[torch.float64]))
    err = _amax((gp["opacities"] + gp["opacities_thermal"]).double() - gs["opacities"].double())
    print(f"d opacities + d opacities_thermal vs shared: {err:.2e}, float32 restatement {floor:.2e} ({err / floor:.1f}x)")
    assert err <= TOL_FACTOR * floor


def test_backward_is_bit_reproducible():
    W, H, mode, sh, rev, seed = CASES[1]
    p, w, _, _ = reference(CASES[1])
    _, cam = _view(W, H)
    m = _model(p, sh, mode)
    g1, _ = _grads(m, cam, w)
    g2, _ = _grads(m, cam, w)
    for k in g1:
        assert torch.equal(g1[k], g2[k]) and bool(torch.isfinite(g1[k]).all()), k
    assert _amax(g1["opacities_thermal"]) > 0


def test_key_sets_of_both_modes():
    p = ssf.shared_params(ssf.awkward_scene(300, 1, 0))
    shared, sep = _model(p, 0, sep="shared"), _model(p, 0)
    assert set(shared.gauss_params.keys()) == set(sf.PARAM_NAMES) and set(shared.state_dict()) == {f"gauss_params.{k}" for k in sf.PARAM_NAMES}
    assert set(shared.get_param_groups()) == {"xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation", "features_dc_thermal", "features_rest_thermal"}
    assert set(sep.gauss_params.keys()) == set(ssf.PARAM_NAMES) and set(sep.state_dict()) == {f"gauss_params.{k}" for k in ssf.PARAM_NAMES}
    assert set(sep.get_param_groups()) == set(shared.get_param_groups()) | {"opacities_thermal"}
    with pytest.raises(ValueError, match="opacities_thermal"):
        shared.load_gaussians({**p, "opacities_thermal": p["opacities"]})
    fresh = _model(p, 0)
    fresh.load_state_dict({k: torch.zeros(7, *v.shape[1:]) for k, v in sep.state_dict().items()})
    assert fresh.gauss_params["opacities_thermal"].shape == (7, 1)
    from nerfstudio_thermal_amd.splat import ThermalSplatfactoModel, ThermalSplatfactoModelConfig

    init = ThermalSplatfactoModel(ThermalSplatfactoModelConfig(thermal_opacity_mode="separate"), num_points=5, device=DEV)
    assert torch.equal(init.gauss_params["opacities_thermal"], init.gauss_params["opacities"]) and init.gauss_params["opacities_thermal"].shape == (5, 1)


def _adam_with_state(m, seed):
    g = torch.Generator().manual_seed(seed)
    opts = {}
    for group, (p,) in m.get_param_groups().items():
        o = torch.optim.Adam([p], lr=1e-3)
        o.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.randn(p.shape, generator=g).to(DEV), "exp_avg_sq": torch.rand(p.shape, generator=g).to(DEV)}
        opts[group] = o
    return opts


def _state(m, opts):
    from nerfstudio_thermal_amd.splat import GROUP_PARAMS_SEP

    params = {k: m.gauss_params[k].detach().clone() for k in m.param_names}
    moments = {k: (opts[g].state[m.gauss_params[k]]["exp_avg"].clone(), opts[g].state[m.gauss_params[k]]["exp_avg_sq"].clone()) for g, k in GROUP_PARAMS_SEP.items()}
    return params, moments


def test_refinement_matches_the_restatement():
    """One densify-and-cull step (split, duplicate, both-below cull) and one opacity reset against ssf.refine on the same device tensors."""
    g = torch.Generator().manual_seed(11)
    p = ssf.awkward_scene(300, 2, 0)
    n = p["means"].shape[0]
    p["scales"] = p["scales"] + torch.where(torch.rand(n, 1, generator=g) < 0.3, 1.5, -1.5)  # some above densify_size_thresh, most below
    lo, hi = -3.0, 1.0
    pick = torch.randint(0, 4, (n, 1), generator=g)
    p["opacities"] = torch.where(pick < 2, lo, hi) + 0.01 * torch.rand(n, 1, generator=g)
    p["opacities_thermal"] = torch.where(pick % 2 == 0, lo, hi) + 0.01 * torch.rand(n, 1, generator=g)
    m = _model(p, 0)
    m.num_train_data = 0
    m.step = 600
    m.last_size = (24, 40)
    m.xys_grad_norm = (torch.rand(n, generator=g) * 4e-5).to(DEV)
    m.vis_counts = torch.ones(n, device=DEV)
    m.max_2Dsize = (torch.rand(n, generator=g) * 0.04).to(DEV)
    opts = _adam_with_state(m, 3)
    params, moments = _state(m, opts)
    stats = (m.xys_grad_norm.clone(), m.vis_counts.clone(), m.max_2Dsize.clone())
    gen = torch.Generator(device=DEV)
    gen.set_state(m.noise_generator.get_state())
    want, want_m, info = ssf.refine(params, moments, stats, (24, 40), 600, m.config, 0, lambda k: torch.randn((k, 3), device=DEV, generator=gen))
    m.refinement_after(opts, 600)
    got, got_m = _state(m, opts)
    both_low = ((torch.sigmoid(params["opacities"]) < 0.1) & (torch.sigmoid(params["opacities_thermal"]) < 0.1)).reshape(-1)
    one_low = ((torch.sigmoid(params["opacities"]) < 0.1) ^ (torch.sigmoid(params["opacities_thermal"]) < 0.1)).reshape(-1)
    assert info["densify"] and info["num_split"] > 5 and info["num_dup"] > 5 and int(both_low.sum()) > 20 and int(one_low.sum()) > 50
    assert bool(info["culled"][:n][both_low].all()) and not bool(info["culled"][:n][one_low & ~info["split"]].any())
    print(f"refine: {n} -> {want['means'].shape[0]} rows ({info['num_split']} split, {info['num_dup']} duplicated, {int(info['culled'].sum())} culled)")
    for k in ssf.PARAM_NAMES:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)  # row counts are exact
        if k in ("means", "scales"):
            assert torch.allclose(got[k], want[k], rtol=1e-5, atol=1e-6), k
        else:
            assert torch.equal(got[k], want[k]), k  # copies: the kept, split and duplicated sets are exactly the restatement's
        assert torch.equal(got_m[k][0], want_m[k][0]) and torch.equal(got_m[k][1], want_m[k][1]), k
    # the opacity reset (step % (reset_alpha_every * refine_every) == refine_every): both logit tensors clamped, both groups' moments zeroed
    m.step = 3100
    params, moments = got, got_m
    want, want_m, info = ssf.refine(params, moments, None, (24, 40), 3100, m.config, 0, lambda k: torch.zeros((k, 3), device=DEV))
    m.refinement_after(opts, 3100)
    got, got_m = _state(m, opts)
    reset = torch.logit(torch.tensor(0.2)).item()
    assert info["reset"] and info["culled"] is None
    for k in ssf.PARAM_NAMES:
        assert torch.equal(got[k], want[k]), k
        assert torch.equal(got_m[k][0], want_m[k][0]) and torch.equal(got_m[k][1], want_m[k][1]), k
    for k in ("opacities", "opacities_thermal"):
        assert float(got[k].max()) == reset and float(params[k].max()) > reset
        assert _amax(got_m[k][0]) == 0.0 and _amax(got_m[k][1]) == 0.0
    assert _amax(got_m["means"][0]) > 0


def _two_plane_scene(seed=0):
    """A back plane seen in both spectra and a front plane, between it and the cameras, that only thermal frames see: Gaussians on two grids."""
    g = torch.Generator().manual_seed(seed)
    ys, zs = torch.meshgrid(torch.linspace(-0.6, 0.6, 9), torch.linspace(-0.4, 0.4, 7), indexing="ij")
    grid = torch.stack([torch.zeros_like(ys), ys, zs], -1).reshape(-1, 3)
    n = grid.shape[0]
    means = torch.cat([grid + torch.tensor([0.6, 0.0, 0.0]), grid * 0.8 + torch.tensor([1.2, 0.0, 0.0])])  # cameras look down -x from x ~ 2.5
    front = torch.cat([torch.zeros(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool)])
    p = {"means": means, "scales": torch.full((2 * n, 3), -2.3), "quats": torch.nn.functional.normalize(torch.randn(2 * n, 4, generator=g), dim=-1),
         "opacities": torch.full((2 * n, 1), 3.0), "features_dc": torch.where(front[:, None], 2.0, -1.0) * torch.ones(2 * n, 3),
         "features_rest": torch.zeros(2 * n, 0, 3), "features_dc_thermal": torch.where(front[:, None], 2.5, -2.0), "features_rest_thermal": torch.zeros(2 * n, 0, 1)}
    return p, front


def test_training_separates_a_plane_that_only_thermal_frames_see():
    """60 Adam steps on a two-plane scene whose front plane is opaque in the thermal frames and absent from the RGB frames.  A direction check:
    separate mode ends with the front plane's thermal opacity above its RGB opacity, and a lower thermal loss than shared mode, which has to draw
    the plane in both spectra or in neither."""
    W, H = 40, 24
    _, cam = _view(W, H)
    p, front = _two_plane_scene()
    truth = _model({**p, "opacities_thermal": p["opacities"].clone(), "opacities": torch.where(front[:, None], -9.0, 3.0)}, 0)
    gt = truth.get_outputs(cam)
    gt_rgb, gt_th = gt["rgb"].clone(), gt["thermal"].clone()
    assert float((gt_th - truth.get_outputs(cam)["rgb"].mean(-1, keepdim=True)).abs().max()) > 0.3  # the spectra do differ
    start = {**p, "opacities": torch.zeros_like(p["opacities"])}
    final = {}
    for sep in ("shared", "separate"):
        m = _model(start, 0, sep=sep)
        opt = torch.optim.Adam([{"params": [m.gauss_params[k]], "lr": 0.1} for k in m.param_names if k.startswith("opacities")])
        for it in range(60):
            opt.zero_grad(set_to_none=True)
            o = m.get_train_outputs(cam)
            loss_th = (o["thermal"] - gt_th).abs().mean()
            ((o["rgb"] - gt_rgb).abs().mean() + loss_th).backward()
            opt.step()
        with torch.no_grad():
            o = m.get_outputs(cam)
            final[sep] = (float((o["thermal"] - gt_th).abs().mean()), float((o["rgb"] - gt_rgb).abs().mean()), m)
    m = final["separate"][2]
    gap = float((torch.sigmoid(m.gauss_params["opacities_thermal"]) - torch.sigmoid(m.gauss_params["opacities"]))[front.to(DEV)].mean())
    print(f"front plane: mean s(o_th) - s(o) = {gap:.3f}; thermal L1 separate {final['separate'][0]:.4f} / shared {final['shared'][0]:.4f}; "
          f"RGB L1 separate {final['separate'][1]:.4f} / shared {final['shared'][1]:.4f}")
    assert gap > 0
    assert final["separate"][0] < final["shared"][0]


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from nerfstudio_thermal_amd import _lib
    from nerfstudio_thermal_amd.splat import camera_struct

    lib = _lib.load()
    _, cam = _view(40, 24)
    c = C.byref(camera_struct(cam))
    buf = torch.zeros(1 << 16, device=DEV)
    d = C.c_void_p(buf.data_ptr())
    EINVAL = -22
    torch.cuda.synchronize()
    # (a null opacities_thermal of the projection and a null out_alpha_thermal of the eval raster are the shared mode now, not refusals)
    assert lib.tn_splat_project(c, None, d, d, d, d, d, d, d, d, d, 1 << 31, 0, 0, 0, d, d, d, d, d, d, d, d, 100, None, None) == EINVAL
    assert lib.tn_splat_raster_chains(c, 10, d, -1, d, 0, d, d, d, d, d, d, d, d, None) == EINVAL
    assert lib.tn_splat_raster_chains(c, 10, d, 100, d, 0, d, d, d, d, d, d, None, d, None) == EINVAL
    assert lib.tn_splat_raster_chains(c, 10, d, 100, d, 0, d, d, d, None, d, d, d, d, None) == EINVAL
    need = lib.tn_splat_backward_workspace_bytes(10, 100, 1, 0, 0)
    bw = lambda total, tth, nbytes: lib.tn_splat_raster_backward(c, 10, d, 100, total, d, 0, d, d, tth, d, d, d, d, d, d, nbytes, d, None, d, d, d, d, None, None, None, None)  # noqa: E731
    assert bw(50, d, need - 1) == EINVAL
    assert bw(50, None, need) == EINVAL
    assert bw(101, d, need) == EINVAL
    assert lib.tn_splat_project_backward(c, None, None, d, d, d, d, d, d, d, d, None, 10, 0, 0, 0, d, d, d, d, d, d, None, d, d, d, d, d, d, d, d, d, None, 0, None, None,
                                         None) == EINVAL
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0  # nothing ran
