"""Seeding thermal splats from a point cloud on the GPU: tn_knn against the float32 brute force (knn_functional.py) bit for bit, determinism
and streams, the seeded model's initial parameters (splatfacto's populate_modules), training from seeds, the seeded start against the random
one on the cube scene, and a 1 M-point / 1080p smoke."""
import json
import math
import os
import sys

import pytest
import torch

import knn_functional as kf

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOUDS = ("uniform", "plane", "line", "identical", "lattice", "duplicates", "clusters")


def _splat():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import splat

    return splat


def _knn(p, k):
    d, i = _splat().knn_distances(p.to(DEV), k, return_index=True)
    torch.cuda.synchronize()
    return d.cpu(), i.cpu()


def _exact(d, i, rd, ri, what):
    assert d.dtype == torch.float32 and d.shape == rd.shape, what
    assert torch.equal(d.view(torch.int32), rd.float().view(torch.int32)), (what, int((d != rd).sum()))
    assert torch.equal(i, ri), (what, int((i != ri).sum()))


@pytest.mark.parametrize("kind", CLOUDS)
@pytest.mark.parametrize("n", [2, 4, 5, 9, 1000, 4097, 50_000])
def test_knn_bit_identical_to_brute_force(kind, n):
    p = kf.cloud(kind, n, seed=n)
    ks = [k for k in (1, 3, 8) if k + 1 <= n]
    kmax = max(ks)
    rd, ri = kf.knn_brute(p.to(DEV), kmax)  # brute force on the device: separate elementwise fp32 ops, sqrt on the host
    for k in ks:
        d, i = _knn(p, k)
        _exact(d, i, rd[:, :k], ri[:, :k], f"{kind} n={n} k={k}")


@pytest.mark.parametrize("kind", ["uniform", "surface"])
@pytest.mark.parametrize("n", [1_000_000, 4_000_000])
def test_knn_large_clouds_on_sampled_rows(kind, n):
    p = kf.cloud(kind, n, seed=7)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:4096]
    d, i = _knn(p, 3)
    rd, ri = kf.knn_brute(p.to(DEV), 3, rows=rows, max_elems=1 << 26)
    _exact(d[rows], i[rows], rd, ri, f"{kind} n={n}")


def test_knn_runs_are_identical_and_follow_the_stream():
    splat = _splat()
    p = kf.cloud("surface", 300_000, seed=3).to(DEV)
    a, ia = splat.knn_distances(p, 3, return_index=True)
    b, ib = splat.knn_distances(p, 3, return_index=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c, ic = splat.knn_distances(p, 3, return_index=True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for x, y in ((a, b), (a, c), (ia, ib), (ia, ic)):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert torch.equal(splat.knn_distances(p, 3), a)


def test_knn_refuses_bad_input():
    splat = _splat()
    with pytest.raises(ValueError):
        splat.knn_distances(torch.zeros((3, 3), device=DEV), 3)
    bad = torch.rand((100, 3), device=DEV)
    bad[17, 1] = float("nan")
    with pytest.raises(ValueError):
        splat.knn_distances(bad, 3)
    bad[17, 1] = float("inf")
    with pytest.raises(ValueError):
        splat.knn_distances(bad, 3)
    with pytest.raises(ValueError):
        splat.knn_distances(torch.rand((100, 3)), 3)  # host tensor


def _seeds(n=2000, seed=0, colours=True):
    from nerfstudio_thermal_amd import synth

    xyz, rgb = synth.cube_surface_points(n, seed=seed)
    rgb = torch.from_numpy(rgb) if colours else torch.zeros((0, 3), dtype=torch.uint8)
    return torch.from_numpy(xyz), rgb


@pytest.mark.parametrize("sh_degree", [3, 0])
def test_seeded_parameters_follow_populate_modules(sh_degree):
    splat = _splat()
    xyz, rgb = _seeds()
    rgb[0] = torch.tensor([0, 255, 128], dtype=torch.uint8)
    m = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(sh_degree=sh_degree), device=DEV, seed=5, seed_points=(xyz, rgb))
    gp = {k: v.detach().cpu() for k, v in m.gauss_params.items()}
    n, dim_sh = xyz.shape[0], (sh_degree + 1) ** 2
    assert m.num_points == n
    assert torch.equal(gp["means"], xyz)
    dist, _ = kf.knn_brute(xyz, 3)  # exact on the host; the reference's torch ops after it run where the model runs them
    assert torch.equal(gp["scales"], torch.log(dist.to(DEV).mean(dim=-1, keepdim=True).repeat(1, 3)).cpu())
    g = torch.Generator().manual_seed(5)
    assert torch.equal(gp["quats"], torch.nn.functional.normalize(torch.randn((n, 4), generator=g), dim=-1))
    assert torch.equal(gp["opacities"], torch.logit(0.1 * torch.ones(n, 1)))
    if sh_degree > 0:
        assert torch.equal(gp["features_dc"], ((rgb.to(DEV) / 255 - 0.5) / 0.28209479177387814).cpu())
    else:
        want = torch.logit(rgb.to(DEV).double() / 255, eps=1e-10).float().cpu()
        assert torch.equal(gp["features_dc"], want)
        assert bool(torch.isfinite(gp["features_dc"]).all())
        assert abs(float(gp["features_dc"][0, 0]) + 23.0259) < 1e-3 and abs(float(gp["features_dc"][0, 1]) - 23.0259) < 1e-3
    assert gp["features_rest"].shape == (n, dim_sh - 1, 3) and not gp["features_rest"].any()
    assert gp["features_dc_thermal"].shape == (n, 1) and not gp["features_dc_thermal"].any()
    assert gp["features_rest_thermal"].shape == (n, dim_sh - 1, 1) and not gp["features_rest_thermal"].any()
    assert all(v.is_cuda and v.dtype == torch.float32 for v in m.gauss_params.values())


def test_seeds_without_colours_random_init_and_too_few_points():
    splat = _splat()
    xyz, _ = _seeds(500, colours=False)
    cfg = splat.ThermalSplatfactoModelConfig()
    m = splat.ThermalSplatfactoModel(cfg, device=DEV, seed=2, seed_points=(xyz.to(DEV), torch.zeros((0, 3), dtype=torch.uint8)))
    g = torch.Generator().manual_seed(2)
    torch.randn((500, 4), generator=g)  # the quats' draw comes first
    assert torch.equal(m.gauss_params["features_dc"].cpu(), torch.rand((500, 3), generator=g))
    assert torch.equal(m.gauss_params["means"].cpu(), xyz)
    # random_init ignores the seeds: the random cube of a model built without them
    r = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(random_init=True, num_random=300), device=DEV, seed=4, seed_points=_seeds(500))
    plain = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(num_random=300), device=DEV, seed=4)
    assert r.num_points == 300 and all(torch.equal(r.gauss_params[k], plain.gauss_params[k]) for k in plain.gauss_params)
    for n in (0, 3):
        with pytest.raises(ValueError):
            splat.ThermalSplatfactoModel(cfg, device=DEV, seed_points=(torch.rand((n, 3)), torch.zeros((n, 3), dtype=torch.uint8)))


def test_construction_without_seeds_is_unchanged():
    """The random start as it was before seeding existed, restated."""
    splat = _splat()
    for cfg_kw, n in (({}, None), ({"sh_degree": 0, "random_scale": 2.0}, 1234)):
        cfg = splat.ThermalSplatfactoModelConfig(**cfg_kw)
        m = splat.ThermalSplatfactoModel(cfg, num_points=n, device=DEV, seed=9)
        n = cfg.num_random if n is None else n
        g = torch.Generator().manual_seed(9)
        dim_sh = (cfg.sh_degree + 1) ** 2
        want = {"means": (torch.rand((n, 3), generator=g) - 0.5) * cfg.random_scale,
                "scales": torch.full((n, 3), math.log(0.01 * cfg.random_scale)),
                "quats": torch.nn.functional.normalize(torch.randn((n, 4), generator=g), dim=-1),
                "opacities": torch.logit(0.1 * torch.ones(n, 1)), "features_dc": torch.rand((n, 3), generator=g),
                "features_rest": torch.zeros((n, dim_sh - 1, 3)), "features_dc_thermal": torch.rand((n, 1), generator=g),
                "features_rest_thermal": torch.zeros((n, dim_sh - 1, 1))}
        assert sorted(m.gauss_params.keys()) == sorted(want.keys())
        for k, v in want.items():
            assert torch.equal(m.gauss_params[k].cpu(), v), k


def _cube_scene(tmp_path, num_seed_points):
    """the cube scene of scripts/train_splat_scene.py (4 frames per spectrum) with its PLY, through the dataparser"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train_splat_scene as tss
    from train_eval_scene import write_cube_scene

    from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig

    d = str(tmp_path / "cube")
    write_cube_scene(d, 4, torch.device(DEV))
    tss.add_seed_points(d, num_seed_points, 0)
    with open(os.path.join(d, "transforms.json"), encoding="utf-8") as f:
        assert json.load(f)["ply_file_path"] == "sparse_pc.ply"
    out = ThermalNerfDataParserConfig(data=d, load_3D_points=True, train_split_fraction=1.0).setup().get_dataparser_outputs("train")
    return tss.frames_of(out, torch.device(DEV)), (out.metadata["points3D_xyz"], out.metadata["points3D_rgb"])


def _train(frames, steps, seed_points=None, num=0, refine_every=100):
    splat = _splat()
    from nerfstudio_thermal_amd.model import TrainingCallbackLocation
    from nerfstudio_thermal_amd.optim import SPLAT_OPTIMIZERS, HipAdam, Optimizers

    cfg = splat.ThermalSplatfactoModelConfig(num_random=num, random_scale=1.0, refine_every=refine_every, warmup_length=refine_every,
                                             sh_degree_interval=steps)
    m = splat.ThermalSplatfactoModel(cfg, device=DEV, seed=0, num_train_data=len(frames), seed_points=seed_points)
    n0 = m.num_points
    opts = Optimizers(m.get_param_groups(), SPLAT_OPTIMIZERS, optimizer_cls=HipAdam)
    cbs = m.get_training_callbacks(opts)
    losses = []
    for step in range(steps):
        for cb in cbs:
            cb.run_callback_at_location(step, TrainingCallbackLocation.BEFORE_TRAIN_ITERATION)
        opts.zero_grad_all()
        cam, batch = frames[step % len(frames)]
        loss = m.get_loss_dict(m.get_train_outputs(cam), batch)
        (loss["main_loss"] + loss["scale_reg"]).backward()
        opts.optimizer_step_all()
        opts.scheduler_step_all()
        for cb in cbs:
            cb.run_callback_at_location(step, TrainingCallbackLocation.AFTER_TRAIN_ITERATION)
        losses.append(loss["main_loss"].detach())
    torch.cuda.synchronize()
    return [float(x) for x in losses], n0, m.num_points


def test_seeded_model_trains_with_refinement(tmp_path):
    frames, seeds = _cube_scene(tmp_path, 3000)
    assert seeds[0].shape == (3000, 3) and seeds[1].dtype == torch.uint8
    losses, n0, n1 = _train(frames, 260, seed_points=seeds, refine_every=50)
    assert n0 == 3000 and all(math.isfinite(v) for v in losses)
    assert n1 != n0  # densification / culling ran on the seeded Gaussians


def test_seeded_start_beats_random_start(tmp_path):
    """Same step budget and initial Gaussian count (5000) on the cube scene, trained frame by frame through get_loss_dict, HipAdam and
    refinement.  Mean main_loss over the last 50 of 300 steps, measured on an MI355X: 0.0370 from the seeds, 0.1990 from the random cube
    (a ratio of 0.19); the assertion asks for a ratio below 0.5."""
    frames, seeds = _cube_scene(tmp_path, 5000)
    seeded, _, _ = _train(frames, 300, seed_points=seeds)
    rand, _, _ = _train(frames, 300, num=5000)
    s, r = sum(seeded[-50:]) / 50, sum(rand[-50:]) / 50
    print(f"seeded start: main_loss {s:.4f}, random start: {r:.4f}")
    assert s < 0.5 * r, (s, r)


def test_one_million_seed_points_then_a_1080p_frame():
    splat = _splat()
    p = kf.cloud("surface", 1_000_000, seed=12) * 0.5
    rgb = torch.randint(0, 256, (1_000_000, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    m = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(), device=DEV, seed=1, seed_points=(p, rgb))
    assert m.num_points == 1_000_000
    cam = splat.PinholeCamera(_look_at((3.2, 0.5, 0.8)), 1400.0, 1400.0, 960.0, 540.0, 1920, 1080)
    out = m.get_outputs(cam)
    torch.cuda.synchronize()
    assert out["rgb"].shape == (1080, 1920, 3) and bool(torch.isfinite(out["rgb"]).all()) and bool(torch.isfinite(out["thermal"]).all())
    assert float(out["accumulation"].max()) > 0.5


def _look_at(eye):
    from nerfstudio_thermal_amd import synth

    return synth.look_at_camera(eye)
