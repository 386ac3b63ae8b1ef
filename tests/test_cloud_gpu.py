"""The point-cloud export on the GPU: tn_cloud_append bit for bit against the float32 restatement (cloud_functional.py), the neighbour means and
the outlier rule of tn_cloud_remove_outliers against the brute force, generate_point_cloud on a small trained model in both density modes, and the
thermal seeds of ThermalSplatfactoModel."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import cloud_functional as cf
import knn_functional as kf
from nerfstudio_thermal_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -12345.0


def _cloud():
    from nerfstudio_thermal_amd import cloud

    return cloud


# ---------------------------------------------------------------------------------------------------- 1. append
def _rays(R, seed=0):
    """R rays around the unit box: about half are opaque, most points land inside (-1, 1)^3."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(s, generator=g)  # noqa: E731
    o = u(R, 3) - 0.5
    d = torch.nn.functional.normalize(torch.randn((R, 3), generator=g), dim=-1)
    return {"o": o, "d": d, "depth": u(R) * 1.2, "acc": u(R), "rgbt": u(R, 4).contiguous()}


def _append(r, alpha=0.5, box=None, cap=None, views=True, buffers=None, count=None):
    """One tn_cloud_append call on the device.  -> (buffers with a guard row behind cap, count tensor)."""
    cloud = _cloud()
    R = r["o"].shape[0]
    cap = R if cap is None else cap
    if buffers is None:
        buffers = [torch.full((cap + 1, w), GUARD, device=DEV) for w in (3, 3, 1)]
        count = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = cloud.PointCloud(*(b[:cap] for b in buffers))
    rgbt = r["rgbt"].to(DEV)
    rgb, th = (rgbt[:, :3], rgbt[:, 3:]) if views else (rgbt[:, :3].contiguous(), rgbt[:, 3:].contiguous())
    assert rgb.is_contiguous() != views or R == 1
    crop = box.crop_struct() if box is not None else None
    cloud.append_call(r["o"].to(DEV), r["d"].to(DEV), r["depth"].to(DEV), r["acc"].to(DEV), rgb, th, alpha, crop, out, count)
    return buffers, count


def _ref(r, alpha=0.5, box=None):
    return cf.append_ref(r["o"], r["d"], r["depth"], r["acc"], r["rgbt"][:, :3], r["rgbt"][:, 3:], alpha, box.crop_struct() if box is not None else None)


def _check(buffers, count, want, cap):
    """The first min(K, cap) kept rays, bit for bit; the counter; untouched rows (the guard row included) still hold the fill value."""
    xyz, rgb, th = want[:3]
    k = min(xyz.shape[0], cap)
    assert int(count.item()) == k
    for b, w in zip(buffers, (xyz, rgb, th)):
        got = b.cpu()
        assert torch.equal(got[:k].view(torch.int32), w[:k].contiguous().view(torch.int32))
        assert bool((got[k:] == GUARD).all())


def _box():
    return _cloud().default_box()


@pytest.mark.parametrize("R", [1, 63, 64, 65, 256, 257, 3 * 256 + 17])
@pytest.mark.parametrize("boxed", [False, True])
def test_append_matches_the_restatement_bit_for_bit(R, boxed):
    r = _rays(R, seed=R)
    box = _box() if boxed else None
    want = _ref(r, box=box)
    if R > 60:
        assert 0.25 * R < int(want[3].sum()) < 0.75 * R  # about half the rays are kept
    b, c = _append(r, box=box)
    _check(b, c, want, R)
    b2, c2 = _append(r, box=box, views=False)  # contiguous copies instead of views of the [R,4] buffer: the same bytes
    assert all(torch.equal(x, y) for x, y in zip(b, b2)) and torch.equal(c, c2)
    b3, c3 = _append(r, box=box)  # and a second run
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(b, b3)) and torch.equal(c, c3)


def test_append_all_kept_none_kept_and_the_edge_values():
    R = 300
    r = _rays(R, seed=3)
    r["acc"] = torch.ones(R)
    r["depth"] = torch.rand(R, generator=torch.Generator().manual_seed(1)) * 0.4
    want = _ref(r, box=_box())
    assert int(want[3].sum()) == R
    _check(*_append(r, box=_box()), want, R)
    r["acc"] = torch.zeros(R)
    want = _ref(r)
    assert int(want[3].sum()) == 0
    _check(*_append(r), want, R)
    # one ray per edge: NaN depth, inf depth, accumulation exactly at the threshold, just above it, a point exactly on a box face, one just inside
    o = torch.zeros(6, 3)
    d = torch.tensor([[1.0, 0, 0]]).repeat(6, 1)
    depth = torch.tensor([float("nan"), float("inf"), 0.5, 0.5, 1.0, float(np.nextafter(np.float32(1.0), np.float32(0.0)))])
    acc = torch.tensor([1.0, 1.0, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1.0))), 1.0, 1.0])
    e = {"o": o, "d": d, "depth": depth, "acc": acc, "rgbt": torch.rand(6, 4, generator=torch.Generator().manual_seed(2))}
    want = _ref(e, box=_box())
    assert want[3].tolist() == [False, False, False, True, False, True]
    _check(*_append(e, box=_box()), want, 6)
    want = _ref(e)  # without a box the point on the face stays; NaN, inf and the threshold itself still go
    assert want[3].tolist() == [False, False, False, True, True, True]
    _check(*_append(e), want, 6)
    d[1] = torch.tensor([0.0, 1.0, 0.0])  # inf * 0 in two coordinates: NaN there, inf in the third
    _check(*_append(e), _ref(e), 6)


def test_append_twice_in_order_and_capacity():
    a, b = _rays(257, seed=10), _rays(3 * 256 + 17, seed=11)
    wa, wb = _ref(a, box=_box()), _ref(b, box=_box())
    both = [torch.cat([x, y]) for x, y in zip(wa[:3], wb[:3])]
    total = both[0].shape[0]
    cap = total + 5
    buf, cnt = _append(a, box=_box(), cap=cap)
    buf, cnt = _append(b, box=_box(), cap=cap, buffers=buf, count=cnt)
    _check(buf, cnt, both, cap)
    # a capacity below the kept number: the first `cap` kept rays, count == cap, nothing behind the buffers
    for cap in (total - 1, wa[0].shape[0] + 1, wa[0].shape[0], 7, 0):
        buf, cnt = _append(a, box=_box(), cap=cap)
        buf, cnt = _append(b, box=_box(), cap=cap, buffers=buf, count=cnt)
        _check(buf, cnt, both, cap)
        assert int(cnt.item()) == cap


def test_append_points_reads_the_model_outputs_and_refuses_host_tensors():
    from nerfstudio_thermal_amd.rays import RayBundle

    cloud = _cloud()
    r = _rays(500, seed=21)
    rgbt = r["rgbt"].to(DEV)
    out = {"rgb": rgbt[:, :3], "rgb_thermal": rgbt[:, 3:], "depth": r["depth"].to(DEV)[:, None], "accumulation": r["acc"].to(DEV)[:, None]}
    rb = RayBundle(origins=r["o"].to(DEV), directions=r["d"].to(DEV), pixel_area=torch.ones(500, 1, device=DEV))
    buf = cloud.PointCloud.empty(500, DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    cloud.append_points(out, rb, buf, cnt, _box())
    want = _ref(r, box=_box())
    k = int(cnt.item())
    assert k == want[0].shape[0]
    assert torch.equal(buf.xyz[:k].cpu(), want[0]) and torch.equal(buf.rgb[:k].cpu(), want[1]) and torch.equal(buf.thermal[:k].cpu(), want[2])
    with pytest.raises(ValueError, match="no CPU fallback"):
        cloud.append_points({k_: v.cpu() for k_, v in out.items()}, rb, buf, cnt, None)


# ---------------------------------------------------------------------------------------------------- 2. neighbour means
def _means(points, nb, ratio=10.0):
    cloud = _cloud()
    n = points.shape[0]
    p = points.to(DEV).contiguous()
    src = cloud.PointCloud(p, torch.rand(n, 3, device=DEV), torch.rand(n, 1, device=DEV))
    out = cloud.PointCloud.empty(n, DEV)
    cnt, stats = torch.zeros(1, dtype=torch.int64, device=DEV), torch.empty(3, dtype=torch.float64, device=DEV)
    mean, keep = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    cloud.remove_outliers_call(src, nb, ratio, out, cnt, stats, mean, keep)
    return src, out, int(cnt.item()), stats.cpu().numpy(), mean.cpu().numpy(), keep.cpu().numpy().astype(bool)


@pytest.mark.parametrize("kind", ["uniform", "duplicates", "lattice", "plane"])
@pytest.mark.parametrize("n,nbs", [(20, (2, 9, 20)), (21, (2, 9, 20)), (33, (2, 9, 20, 32)), (1000, (2, 9, 20, 32))])
def test_neighbour_means_equal_the_brute_force(kind, n, nbs):
    """uniform; exact duplicates (heavy ties at distance 0); a lattice (mass ties at equal distances); a coplanar cloud (one zero extent)."""
    p = kf.cloud(kind, n, seed=n)
    for nb in nbs:
        got = _means(p, nb)[4]
        want = cf.neighbor_means(p, nb)
        assert np.array_equal(got, want), (kind, n, nb, np.abs(got - want).max())


# ---------------------------------------------------------------------------------------------------- 3. outlier removal
def _cube_with_far_points(seed):
    xyz, _ = synth.cube_surface_points(2000, seed=seed)
    g = np.random.default_rng(100 + seed)
    far = torch.nn.functional.normalize(torch.from_numpy(g.standard_normal((10, 3))), dim=-1) * torch.from_numpy(g.uniform(30.0, 60.0, (10, 1)))
    p = torch.cat([torch.from_numpy(xyz), far.float()])
    perm = torch.from_numpy(np.random.default_rng(200 + seed).permutation(p.shape[0]))
    is_far = torch.zeros(p.shape[0], dtype=torch.bool)
    is_far[2000:] = True
    return p[perm].contiguous(), is_far[perm].numpy()


@pytest.mark.parametrize("std_ratio", [1.0, 10.0])
@pytest.mark.parametrize("seed", [0, 1])
def test_outlier_removal_matches_the_rule(std_ratio, seed):
    p, is_far = _cube_with_far_points(seed)
    mean, (m, s, thr), keep = cf.outliers_ref(p, 20, std_ratio)
    assert not bool((np.abs(mean - thr) <= 1e-9 * thr).any())  # no point sits on the threshold: the mask does not hang on the sums' last bits
    src, out, k, stats, got_mean, got_keep = _means(p, 20, std_ratio)
    assert np.array_equal(got_mean, mean)
    for got, want in zip(stats, (m, s, thr)):
        assert abs(got - want) <= 1e-12 * abs(want), (stats, (m, s, thr))
    assert np.array_equal(got_keep, keep) and k == int(keep.sum())
    sel = torch.from_numpy(keep)
    for a, b in ((out.xyz, src.xyz), (out.rgb, src.rgb), (out.thermal, src.thermal)):  # compacted in the original order
        assert torch.equal(a[:k].cpu(), b.cpu()[sel])
    assert int((~keep & is_far).sum()) >= 1
    if std_ratio == 10.0:
        assert not bool((~keep & ~is_far).any())  # no surface point goes at the reference's ratio
    # the public wrapper hands back exactly the kept rows, and the same bytes on a second run
    cloud = _cloud()
    a, b = cloud.remove_outliers(src, 20, std_ratio), cloud.remove_outliers(src, 20, std_ratio)
    assert len(a) == k and torch.equal(a.xyz, out.xyz[:k]) and torch.equal(a.xyz, b.xyz) and torch.equal(a.thermal, b.thermal)


def test_identical_points_keep_nothing_and_small_clouds_come_back_unchanged(capsys):
    cloud = _cloud()
    p = kf.cloud("identical", 50)
    src, out, k, stats, mean, keep = _means(p, 20)
    assert k == 0 and not keep.any() and bool((mean == 0).all())
    assert len(cloud.remove_outliers(src)) == 0
    small = cloud.PointCloud(torch.rand(19, 3, device=DEV), torch.rand(19, 3, device=DEV), torch.rand(19, 1, device=DEV))
    capsys.readouterr()
    back = cloud.remove_outliers(small, nb_neighbors=20)
    assert back is small and "returned unchanged" in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------- 4. generate_point_cloud
NUM_POINTS, RAYS, BUNDLES, STEPS = 20_000, 4096, 12, 300
_TRAINED = {}


def _trained(mode):
    """The small model of test_model_api_gpu.build_model, trained for 300 iterations on the cube scene's analytic pixels, and BUNDLES fixed
    ray bundles of its cameras.  Built once per density mode."""
    if mode in _TRAINED:
        return _TRAINED[mode]
    from nerfstudio_thermal_amd import ops
    from nerfstudio_thermal_amd.rays import RayBundle
    from test_model_api_gpu import build_model

    _, _, model = build_model(mode)
    cams = synth.synth_cameras()
    t = lambda k: torch.from_numpy(cams[k]).to(DEV)  # noqa: E731

    def batch(seed):
        idx = torch.from_numpy(synth.synth_ray_indices(cams, RAYS, seed=seed)).to(DEV)
        o, d, area, _ = ops.raygen(idx, t("c2w"), t("fx"), t("fy"), t("cx"), t("cy"), t("distortion"))
        return idx, RayBundle(origins=o, directions=d, pixel_area=area, camera_indices=idx[:, 0:1].contiguous())

    model.train()
    pool = []
    for s in range(8):  # eight fixed training batches, cycled
        idx, rb = batch(1000 + s)
        is_th = torch.from_numpy(cams["is_thermal"][idx[:, 0].cpu().numpy()].astype(np.float32))
        img = np.stack([synth.cube_scene_images(rb.origins.cpu().numpy(), rb.directions.cpu().numpy(), th) for th in (False, True)])
        img = torch.from_numpy(np.where(is_th.numpy()[:, None] > 0, img[1], img[0]).astype(np.float32))
        pool.append((rb, {"image": img.to(DEV).contiguous(), "is_thermal": is_th.to(DEV)}))
    for step in range(STEPS):
        rb, b = pool[step % len(pool)]
        model.train_iteration(rb, b, step)
    bundles = [batch(2000 + s)[1] for s in range(BUNDLES)]
    _TRAINED[mode] = (model, bundles)
    return _TRAINED[mode]


class _Replay:
    def __init__(self, bundles):
        self.bundles, self.calls = bundles, 0

    def __call__(self):
        self.calls += 1
        return self.bundles[(self.calls - 1) % len(self.bundles)]


@pytest.mark.parametrize("mode", ["shared", "separate"])
def test_generate_point_cloud_equals_the_restatement_on_the_models_outputs(mode):
    cloud = _cloud()
    model, bundles = _trained(mode)
    model.train()
    replay = _Replay(bundles)
    got = cloud.generate_point_cloud(model, replay, num_points=NUM_POINTS, remove_outliers=False)
    assert model.training  # the mode is restored
    assert len(got) == NUM_POINTS and replay.calls % 8 == 0  # the counter is read every eighth batch
    # the restatement on the model's own outputs, bundle by bundle in the order they were served
    crop = cloud.default_box().crop_struct()
    parts, have = [], 0
    model.eval()
    with torch.no_grad():
        for c in range(replay.calls):
            rb = bundles[c % len(bundles)]
            out = model(rb)
            xyz, rgb, th, _ = cf.append_ref(rb.origins.cpu(), rb.directions.cpu(), out["depth"].cpu(), out["accumulation"].cpu(), out["rgb"].cpu(),
                                            out["rgb_thermal"].cpu(), 0.5, crop)
            parts.append((xyz, rgb, th))
            have += xyz.shape[0]
    model.train()
    assert have >= NUM_POINTS
    want = [torch.cat([p[i] for p in parts])[:NUM_POINTS] for i in range(3)]
    assert torch.equal(got.xyz.cpu(), want[0]) and torch.equal(got.rgb.cpu(), want[1]) and torch.equal(got.thermal.cpu(), want[2])
    assert bool((got.xyz.abs() < 1).all()) and bool(cloud.default_box().within(got.xyz).all())
    assert 0 <= float(got.thermal.min()) and float(got.thermal.max()) <= 1
    again = cloud.generate_point_cloud(model, _Replay(bundles), num_points=NUM_POINTS, remove_outliers=False)
    assert all(torch.equal(a, b) for a, b in zip((got.xyz, got.rgb, got.thermal), (again.xyz, again.rgb, again.thermal)))
    cleaned = cloud.generate_point_cloud(model, _Replay(bundles), num_points=NUM_POINTS)  # with the outlier rule: a subset, in order
    assert 0 < len(cleaned) <= NUM_POINTS


def test_generate_point_cloud_gives_up_on_a_model_that_is_never_opaque():
    from test_model_api_gpu import build_model

    cloud = _cloud()
    _, _, model = build_model("shared")
    _, bundles = _trained("shared")
    replay = _Replay(bundles)
    with pytest.raises(RuntimeError, match="of the rays are opaque"):
        cloud.generate_point_cloud(model, replay, num_points=NUM_POINTS, remove_outliers=False, alpha_thresh=0.999, max_batches=4)
    assert replay.calls == 4


# ---------------------------------------------------------------------------------------------------- 5. seeding
def test_thermal_seeds_become_the_thermal_dc_features():
    from nerfstudio_thermal_amd import splat

    xyz, rgb = synth.cube_surface_points(2000, seed=0)
    th = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (2000, 1)).astype(np.uint8))
    th[:2, 0] = torch.tensor([0, 255], dtype=torch.uint8)
    seeds = (torch.from_numpy(xyz), torch.from_numpy(rgb), th)
    m = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(), device=DEV, seed=0, seed_points=seeds)
    want = splat.RGB2SH(th.to(DEV) / 255)
    assert m.gauss_params["features_dc_thermal"].shape == (2000, 1) and torch.equal(m.gauss_params["features_dc_thermal"].detach(), want)
    assert not bool(m.gauss_params["features_rest_thermal"].any()) and m.gauss_params["features_rest_thermal"].shape == (2000, 15, 1)
    flat = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(), device=DEV, seed=0, seed_points=(seeds[0], seeds[1], th[:, 0]))
    assert torch.equal(flat.gauss_params["features_dc_thermal"], m.gauss_params["features_dc_thermal"])
    two = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(), device=DEV, seed=0, seed_points=seeds[:2])
    assert not bool(two.gauss_params["features_dc_thermal"].any())  # a 2-tuple still starts mid-grey
    for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest"):
        assert torch.equal(two.gauss_params[k], m.gauss_params[k]), k
    deg0 = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(sh_degree=0), device=DEV, seed=0, seed_points=seeds)
    assert torch.equal(deg0.gauss_params["features_dc_thermal"].detach(), torch.logit(th.to(DEV).double() / 255, eps=1e-10).float())
    with pytest.raises(ValueError, match="thermal values for 2000 points"):
        splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(), device=DEV, seed=0, seed_points=(seeds[0], seeds[1], th[:-1]))
    with pytest.raises(ValueError, match="thermal must be"):
        splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(), device=DEV, seed=0, seed_points=(seeds[0], seeds[1], th.repeat(1, 3)))


def test_datamanager_hands_out_the_thermal_seeds_and_the_model_renders(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from train_eval_scene import write_cube_scene

    from nerfstudio_thermal_amd import splat
    from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig, write_ply
    from nerfstudio_thermal_amd.splat_datamanager import ThermalFullImageDatamanagerConfig

    d = str(tmp_path / "cube")
    write_cube_scene(d, 2, torch.device(DEV))
    xyz, rgb = synth.cube_surface_points(1500, seed=1)
    th = np.random.default_rng(5).integers(0, 256, (1500, 1)).astype(np.uint8)
    path = os.path.join(d, "transforms.json")
    meta = json.load(open(path, encoding="utf-8"))
    meta["ply_file_path"] = "cloud.ply"
    json.dump(meta, open(path, "w", encoding="utf-8"))
    write_ply(os.path.join(d, "cloud.ply"), xyz, rgb)
    pc = lambda: ThermalNerfDataParserConfig(data=d, load_3D_points=True, train_split_fraction=1.0)  # noqa: E731
    plain = ThermalFullImageDatamanagerConfig(dataparser=pc()).setup(device=DEV).seed_points
    assert len(plain) == 2  # a cloud without the property: the 2-tuple, as before
    write_ply(os.path.join(d, "cloud.ply"), xyz, rgb, thermal=th)
    dm = ThermalFullImageDatamanagerConfig(dataparser=pc()).setup(device=DEV)
    seeds = dm.seed_points
    assert len(seeds) == 3 and torch.equal(seeds[2], torch.from_numpy(th)) and torch.equal(seeds[0], plain[0]) and torch.equal(seeds[1], plain[1])
    m = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(), device=DEV, seed=0, num_train_data=dm.num_train_data, seed_points=seeds,
                                     train_is_thermal=dm.train_is_thermal)
    assert torch.equal(m.gauss_params["features_dc_thermal"].detach(), splat.RGB2SH(torch.from_numpy(th).to(DEV) / 255))
    cam, _ = dm.next_train(0)
    m.eval()
    with torch.no_grad():
        out = m.get_outputs(cam)
    assert all(bool(torch.isfinite(v).all()) for v in out.values() if isinstance(v, torch.Tensor))
    assert float(out["accumulation"].max()) > 0
