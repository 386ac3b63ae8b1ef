"""The TSDF mesh export on the GPU: tn_tsdf_integrate against the reference's recorded volumes and the float64 restatement (tsdf_functional.py), its
invariants (any split of the frames gives the same bits, unobserved voxels keep theirs), tn_mesh_count / tn_mesh_emit bit for bit against the float32
restatement, and export_tsdf_mesh end to end on a small splat model and on the small thermal-nerfacto model of the point-cloud tests."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import tsdf_functional as tf

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tsdf_reference.npz")
F32, F64 = torch.float32, torch.float64
DIMS = (23, 19, 17)  # no multiple of anything: 7429 voxels, 30 blocks of 256
GUARD = -12345.0
MAX_EXCLUDED = 0.01


def _mesh():
    from nerfstudio_thermal_amd import mesh

    return mesh


# ---------------------------------------------------------------------------------------------------- 1. integration
_SCENES = {}


def _scene(B, H, W, depth_kind, with_acc, dims=DIMS):
    """The sphere scene of tsdf_functional at this size, built once.  with_acc: the frames look like a splat render -- pixels off the sphere hold
    the image's largest depth and accumulation 0, and the accumulation on the sphere is random, about a third of it below the threshold."""
    key = (B, H, W, depth_kind, with_acc, dims)
    if key not in _SCENES:
        origin, voxel = tf.box_grid(dims)
        c2w, intr = tf.scene_cameras(B, H, W, seed=B)
        c2w, intr = c2w.float(), intr.float()
        depth, rgbt, hit = tf.sphere_frames(c2w.double(), intr.double(), H, W, seed=B, depth_kind=depth_kind)
        acc = None
        if with_acc:
            g = torch.Generator().manual_seed(100 + B)
            acc = hit * (0.25 + 0.75 * torch.rand(hit.shape, generator=g))
            depth = torch.where(hit > 0, depth, depth.amax(dim=(1, 2), keepdim=True))
        _SCENES[key] = {"dims": dims, "origin": origin, "voxel": voxel, "records": tf.camera_records(c2w, intr), "depth": depth, "rgbt": rgbt,
                        "acc": acc, "truncation": float(voxel[0]) * 5.0, "kind": depth_kind}
    return _SCENES[key]


def _ref(s, dtype, max_weight, vol=None, details=None, frames=slice(None)):
    vol = tf.fresh_volume(s["dims"]) if vol is None else vol
    return tf.integrate_ref(*vol, s["origin"], s["voxel"], s["truncation"], max_weight, s["records"][frames], s["depth"][frames], s["rgbt"][frames],
                            None if s["acc"] is None else s["acc"][frames], 0.5, s["kind"], dtype=dtype, details=details)


def _gpu(s, max_weight, vol=None, frames=slice(None)):
    """tn_tsdf_integrate of the scene's frames into a copy of `vol` on the device -> (values, weights, rgbt) back on the host."""
    vol = tf.fresh_volume(s["dims"]) if vol is None else vol
    v, w, c = (t.to(DEV).contiguous() for t in vol)
    acc = None if s["acc"] is None else s["acc"][frames].to(DEV).contiguous()
    _mesh().integrate_call(v, w, c, s["origin"].tolist(), s["voxel"].tolist(), s["truncation"], max_weight, s["depth"][frames].to(DEV).contiguous(),
                           s["rgbt"][frames].to(DEV).contiguous(), acc, 0.5, s["records"][frames].to(DEV).contiguous(), s["kind"] == "ray")
    return v.cpu(), w.cpu(), c.cpu()


def _compare(got, s, max_weight, label):
    """The convention: outside the voxels on a discontinuity the weights are exact and values and RGB+T miss float64 by at most 8 x what the
    float32 restatement misses it by on the same inputs."""
    details = {}
    want = _ref(s, F64, max_weight, details=details)
    keep = ~details["near"]
    excluded = 1.0 - float(keep.float().mean())
    assert excluded <= MAX_EXCLUDED, excluded
    assert 0.02 < float(details["touched"].float().mean()) < 0.98
    floor32 = _ref(s, F32, max_weight)
    floor = [float((a.double() - b)[keep].abs().max()) for a, b in zip(floor32, want)]
    err = [float((a.double() - b)[keep].abs().max()) for a, b in zip(got, want)]
    print(f"{label}: values {err[0]:.3g} (floor {floor[0]:.3g}), weights {err[1]:.3g}, rgbt {err[2]:.3g} (floor {floor[2]:.3g}), excluded {excluded:.3%}")
    assert err[1] == 0.0
    assert err[0] <= 8 * floor[0] and err[2] <= 8 * floor[2]
    un = ~details["touched"] & keep  # not observed: still the initial volume, bit for bit
    assert bool((got[0][un] == -1.0).all()) and not bool(got[1][un].any()) and not bool(got[2][un].any())


@pytest.mark.parametrize("max_weight", [1.0, 4.0])
@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("depth_kind", ["ray", "z"])
@pytest.mark.parametrize("B", [1, 5, 17])
@pytest.mark.parametrize("H,W", [(48, 64), (29, 37)])
def test_integrate_matches_the_float64_restatement(H, W, B, depth_kind, with_acc, max_weight):
    s = _scene(B, H, W, depth_kind, with_acc)
    _compare(_gpu(s, max_weight), s, max_weight, f"{W}x{H} B={B} {depth_kind} acc={with_acc} max_weight={max_weight}")


def test_integrate_matches_the_references_recorded_volumes():
    """tests/golden/tsdf_reference.npz: the reference's own float32 volumes.  The kernel and the reference both miss the float64 restatement by a few
    float32 roundings, so they may differ by the sum of the two bounds; the thermal channel, which the reference lacks, is held to the restatement."""
    z = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(z[k])  # noqa: E731
    s = {"dims": tuple(int(v) for v in z["dims"]), "origin": t("origin"), "voxel": t("voxel"), "records": tf.camera_records(t("c2w"), t("intr")),
         "depth": t("depth"), "rgbt": t("rgbt"), "acc": None, "truncation": float(z["truncation"]), "kind": "ray"}
    got = _gpu(s, 1.0)
    _compare(got, s, 1.0, "golden scene")
    details = {}
    want = _ref(s, F64, 1.0, details=details)
    keep = ~details["near"]
    floor = [float((a.double() - b)[keep].abs().max()) for a, b in zip(_ref(s, F32, 1.0), want)]
    assert torch.equal(got[1][keep], t("weights")[keep])
    assert float((got[0] - t("values"))[keep].abs().max()) <= 16 * floor[0]
    assert float((got[2][..., :3] - t("colors"))[keep].abs().max()) <= 16 * floor[2]


def _guard_volume(dims):
    g = torch.Generator().manual_seed(9)
    return (torch.full(dims, GUARD), torch.zeros(dims), torch.rand(tuple(dims) + (4,), generator=g) + 7.0)


@pytest.mark.parametrize("max_weight", [1.0, 4.0])
def test_integrate_in_batches_is_bit_equal_and_untouched_voxels_keep_their_bits(max_weight):
    s = _scene(17, 29, 37, "ray", True)
    guard = _guard_volume(s["dims"])
    whole = _gpu(s, max_weight, guard)
    for step in (1, 3):
        vol = guard
        for b0 in range(0, 17, step):
            vol = _gpu(s, max_weight, vol, slice(b0, b0 + step))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(whole, vol)), step
    details = {}
    _ref(s, F64, max_weight, guard, details)
    un = ~details["touched"] & ~details["near"]
    assert 0 < int(un.sum()) < un.numel()
    for got, was in zip(whole, guard):
        assert torch.equal(got[un].view(torch.int32), was[un].view(torch.int32))
    seen = details["touched"] & ~details["near"]
    assert bool((whole[1][seen] > 0).all()) and bool((whole[0][seen] != GUARD).all())
    again = _gpu(s, max_weight, guard)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(whole, again))


@pytest.mark.parametrize("depth_kind", ["ray", "z"])
def test_voxels_behind_a_camera_inside_the_box_are_untouched(depth_kind):
    """The reference divides by the camera z of a voxel behind the camera and mirrors it into the image; here such a voxel is skipped."""
    dims = DIMS
    origin, voxel = tf.box_grid(dims)
    c2w = tf.look_at((0.11, -0.07, 0.05), (0.9, 0.35, 0.2))[None].float()
    intr = torch.tensor([[30.0, 29.0, 32.5, 23.5]])
    s = {"dims": dims, "origin": origin, "voxel": voxel, "records": tf.camera_records(c2w, intr), "depth": torch.full((1, 48, 64), 0.5),
         "rgbt": torch.rand((1, 48, 64, 4), generator=torch.Generator().manual_seed(4)), "acc": None, "truncation": float(voxel[0]) * 5.0, "kind": depth_kind}
    guard = _guard_volume(dims)
    got = _gpu(s, 1.0, guard)
    i, j, k = torch.meshgrid(*(torch.arange(d, dtype=F64) for d in dims), indexing="ij")
    p = torch.stack([origin[0].double() + i * voxel[0].double(), origin[1].double() + j * voxel[1].double(), origin[2].double() + k * voxel[2].double()], -1)
    m = s["records"][0].double()
    z = -(p @ m[8:11] + m[11])
    behind = z < -1e-6
    assert 0.2 < float(behind.float().mean()) < 0.8
    for g, was in zip(got, guard):
        assert torch.equal(g[behind].view(torch.int32), was[behind].view(torch.int32))
    assert bool((got[1][~behind] > 0).any())  # and the camera does see voxels in front of it
    _compare(_gpu(s, 1.0), s, 1.0, f"camera inside the box, {depth_kind}")


# ---------------------------------------------------------------------------------------------------- 2. extraction
def _extract(values, weights, rgbt, origin, voxel, observed_only=False):
    """tn_mesh_count + tn_mesh_emit with one guard row behind the vertices and the faces -> (totals, vertices, normals, rgbt, faces) on the host,
    guard rows included."""
    mesh = _mesh()
    v, w, c = values.to(DEV).contiguous(), weights.to(DEV).contiguous(), rgbt.to(DEV).contiguous()
    ws = mesh.mesh_workspace(tuple(values.shape), DEV)
    totals = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    mesh.mesh_count_call(v, w, observed_only, totals, ws)
    V, Fn = (int(x) for x in totals.tolist())
    bufs = [torch.full((V + 1, 3), GUARD, device=DEV), torch.full((V + 1, 3), GUARD, device=DEV), torch.full((V + 1, 4), GUARD, device=DEV),
            torch.full((Fn + 1, 3), -7, dtype=torch.int32, device=DEV)]
    mesh.mesh_emit_call(v, w, c, observed_only, origin.tolist(), voxel.tolist(), bufs[0][:V], bufs[1][:V], bufs[2][:V], bufs[3][:Fn], ws)
    return (V, Fn), [b.cpu() for b in bufs]


def _check_extraction(values, weights, rgbt, origin, voxel, observed_only=False):
    want = tf.extract_ref(values, weights, rgbt, origin, voxel, observed_only)
    (V, Fn), (vertices, normals, out, faces) = _extract(values, weights, rgbt, origin, voxel, observed_only)
    assert (V, Fn) == (want["vertices"].shape[0], want["faces"].shape[0])
    for got, w in ((vertices, want["vertices"]), (normals, want["normals"]), (out, want["rgbt"])):
        assert torch.equal(got[:V].view(torch.int32), w.contiguous().view(torch.int32))
        assert bool((got[V:] == GUARD).all())
    assert torch.equal(faces[:Fn], want["faces"]) and bool((faces[Fn:] == -7).all())
    return want


_FUSED = {}


def _fused_sphere():
    """The sphere scene fused on the device (a running mean of 9 frames): a volume with observed and unobserved voxels."""
    if not _FUSED:
        s = _scene(9, 48, 64, "ray", True)
        _FUSED["vol"] = _gpu(s, 16.0)
        _FUSED["grid"] = (s["origin"], s["voxel"])
    return _FUSED["vol"], _FUSED["grid"]


@pytest.mark.parametrize("observed_only", [False, True])
def test_mesh_of_a_fused_volume_matches_the_restatement_bit_for_bit(observed_only):
    (values, weights, rgbt), (origin, voxel) = _fused_sphere()  # 30 blocks of lattice points
    assert 0.1 < float((weights > 0).float().mean()) < 0.9
    want = _check_extraction(values, weights, rgbt, origin, voxel, observed_only)
    assert want["faces"].shape[0] > 500
    if observed_only:  # what is left is the sphere alone: every vertex within the truncation distance of it
        r = want["vertices"].norm(dim=-1)
        assert float((r - 0.6).abs().max()) <= float(voxel[0]) * 5.0
        assert bool((want["rgbt"] >= 0).all()) and bool((want["rgbt"] <= 1).all())


@pytest.mark.parametrize("dims", [(9, 8, 7), (2, 2, 2), (3, 2, 5), (1, 6, 5), (6, 5, 1), (40, 3, 33)])
def test_mesh_of_random_signs_matches_the_restatement_bit_for_bit(dims):
    g = torch.Generator().manual_seed(sum(dims))
    values = torch.rand(dims, generator=g) * 2.4 - 1.2  # some beyond the clamp
    values.view(-1)[::11] = 0.0  # and exact zeros, which count as outside
    weights = (torch.rand(dims, generator=g) > 0.2).float()
    rgbt = torch.rand(tuple(dims) + (4,), generator=g)
    origin, voxel = torch.tensor([0.3, -1.7, 0.9]), torch.tensor([0.11, 0.07, 0.13])
    for observed_only in (False, True):
        want = _check_extraction(values, weights, rgbt, origin, voxel, observed_only)
        if dims == (9, 8, 7) and not observed_only:
            assert want["cases"] == set(range(16)) and set(want["edge_kind"].tolist()) == set(range(7))  # every sign case, every edge kind
        if min(dims) == 1:
            assert want["vertices"].shape[0] == 0 and want["faces"].shape[0] == 0


def test_mesh_of_uniform_volumes_is_empty():
    for fill in (-1.0, 1.0, 0.0):
        dims = (7, 6, 5)
        (V, Fn), _ = _extract(torch.full(dims, fill), torch.ones(dims), torch.zeros(tuple(dims) + (4,)), torch.zeros(3), torch.ones(3))
        assert (V, Fn) == (0, 0)


# ---------------------------------------------------------------------------------------------------- 3. the export, end to end
def _rendered_band(mesh_mod, model, cams, volume):
    """bool [X,Y,Z]: the lattice points some camera renders within the truncation distance BEHIND its surface (an opaque pixel, sampled as the
    fusion samples it) -- the only points whose fused value can be negative -- and the range of the thermal values rendered on opaque pixels."""
    X, Y, Z = volume.dims
    o, s = volume.origin.double(), volume.voxel_size.double()
    i, j, k = torch.meshgrid(torch.arange(X, dtype=F64), torch.arange(Y, dtype=F64), torch.arange(Z, dtype=F64), indexing="ij")
    p = torch.stack([o[0] + i * s[0], o[1] + j * s[1], o[2] + k * s[2]], dim=-1)
    rec = mesh_mod.camera_records(cams, "cpu").double()
    band = torch.zeros((X, Y, Z), dtype=torch.bool)
    lo, hi = math.inf, -math.inf
    model.eval()
    with torch.no_grad():
        for b, cam in enumerate(cams):
            depth, acc, rgbt, kind = (t.cpu() if isinstance(t, torch.Tensor) else t for t in mesh_mod.render_frame(model, cam))
            m = rec[b]
            x, y, z = p @ m[0:3] + m[3], -(p @ m[4:7] + m[7]), -(p @ m[8:11] + m[11])
            zs = torch.where(z > 0, z, torch.ones_like(z))
            ru, rv = m[12] * x / zs + m[14] - 0.5, m[13] * y / zs + m[15] - 0.5
            H, W = depth.shape
            vd = torch.sqrt(x * x + y * y + z * z) if kind == "ray" else z
            for du in (-1e-3, 1e-3):  # a projection within 1e-3 pixel of a rounding boundary may take either pixel in float32
                for dv in (-1e-3, 1e-3):
                    fu, fv = torch.round(ru + du), torch.round(rv + dv)
                    inb = (z > 0) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
                    iu, iv = fu.clamp(0, W - 1).long(), fv.clamp(0, H - 1).long()
                    dist = depth.double()[iv, iu] - vd
                    band |= inb & (acc[iv, iu] >= 0.5) & (depth[iv, iu] > 0) & (dist > -1.001 * volume.truncation) & (dist < 1e-3 * volume.truncation)
            if bool((acc >= 0.5).any()):
                th = rgbt[..., 3][acc >= 0.5]
                lo, hi = min(lo, float(th.min())), max(hi, float(th.max()))
    return band, p, lo, hi


def _check_export(model, cams, resolution, box, downscale_factor):
    mesh_mod = _mesh()
    was_training = model.training
    kw = dict(resolution=resolution, downscale_factor=downscale_factor, batch_size=3, bounding_box_min=[-box] * 3, bounding_box_max=[box] * 3)
    full = mesh_mod.export_tsdf_mesh(model, cams, **kw)
    obs, volume = mesh_mod.export_tsdf_mesh(model, cams, observed_only=True, return_volume=True, **kw)
    assert model.training == was_training
    assert volume.dims == ((resolution,) * 3 if isinstance(resolution, int) else tuple(resolution))
    for m in (full, obs):
        V, Fn = m.vertices.shape[0], m.faces.shape[0]
        assert V > 100 and Fn > 100
        assert m.colors.shape == (V, 3) and m.thermal.shape == (V, 1) and m.normals.shape == (V, 3) and m.faces.dtype == torch.int32
        assert int(m.faces.min()) >= 0 and int(m.faces.max()) < V
        assert bool(torch.isfinite(m.vertices).all()) and bool((m.vertices.abs() <= box).all())
    assert obs.faces.shape[0] <= full.faces.shape[0]
    rescaled = [mesh_mod.rescaled_camera(c, downscale_factor) for c in cams]
    band, points, lo, hi = _rendered_band(mesh_mod, model, rescaled, volume)
    assert bool(band.any()) and lo <= hi
    # every vertex sits on a lattice edge whose inside end some camera rendered within the truncation distance behind its surface: it lies within
    # the longest edge, |voxel_size|, of such a point -- and so within truncation + |voxel_size| of the rendered surface
    reach = float(volume.voxel_size.double().norm()) * (1 + 1e-6)
    near = torch.cdist(obs.vertices.double().cpu(), points[band]).min(dim=1).values
    print(f"export: V {obs.vertices.shape[0]} F {obs.faces.shape[0]} (whole volume: F {full.faces.shape[0]}), farthest vertex from the rendered band "
          f"{float(near.max()):.4f} (edge {reach:.4f}), thermal {float(obs.thermal.min()):.3f}..{float(obs.thermal.max()):.3f} (rendered {lo:.3f}..{hi:.3f})")
    assert float(near.max()) <= reach
    # a fused thermal value is a convex combination of rendered ones
    assert lo - 1e-6 <= float(obs.thermal.min()) and float(obs.thermal.max()) <= hi + 1e-6
    assert min(lo, 0.0) - 1e-6 <= float(full.thermal.min()) and float(full.thermal.max()) <= hi + 1e-6  # (a never-observed voxel holds 0)
    return obs, volume


def test_export_tsdf_mesh_of_a_splat_model():
    from nerfstudio_thermal_amd import splat
    from nerfstudio_thermal_amd.splat_camera import OrientedBox, PinholeCamera

    g = torch.Generator().manual_seed(0)
    n = 6000
    xyz = torch.nn.functional.normalize(torch.randn((n, 3), generator=g), dim=-1) * 0.5
    rgb = (torch.rand((n, 3), generator=g) * 255).to(torch.uint8)
    th = (64 + 128 * (0.5 + 0.5 * xyz[:, 2:3] / 0.5)).to(torch.uint8)  # the temperature rises with z
    model = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(background_color="black"), device=DEV, seed=0, seed_points=(xyz, rgb, th))
    with torch.no_grad():
        model.gauss_params["opacities"].fill_(4.0)  # opaque: the render's accumulation passes the threshold on the sphere
    c2w, intr = tf.scene_cameras(7, 96, 128, radius=1.9, seed=1)
    cams = [PinholeCamera(c2w[b].float().to(DEV), *(float(v) for v in intr[b]), 128, 96) for b in range(7)]
    crop = OrientedBox.from_params((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (3.0, 3.0, 3.0))
    model.set_crop(crop)
    obs, volume = _check_export(model, cams, (26, 24, 22), 0.8, 2)
    assert model.crop_box is crop  # left as found
    r = obs.vertices.norm(dim=-1)
    print(f"splat sphere: vertex radius {float(r.min()):.3f}..{float(r.max()):.3f}")
    reach = volume.truncation + float(volume.voxel_size.norm())  # of a vertex from the rendered surface, which is the sphere the Gaussians sit on
    assert 0.5 - reach < float(r.min()) and float(r.max()) < 0.5 + reach
    top, bottom = obs.thermal[obs.vertices[:, 2] > 0.3], obs.thermal[obs.vertices[:, 2] < -0.3]
    assert float(top.mean()) > float(bottom.mean()) + 0.2  # the temperature went with the surface


def test_export_tsdf_mesh_of_the_nerf_model():
    from nerfstudio_thermal_amd import synth
    from nerfstudio_thermal_amd.splat_camera import PinholeCamera
    from test_cloud_gpu import _trained

    model, _ = _trained("shared")
    cams_np = synth.synth_cameras()
    cams = [PinholeCamera(torch.from_numpy(cams_np["c2w"][i]), 150.0, 150.0, 80.0, 60.0, 160, 120, cam_idx=i) for i in range(len(cams_np["c2w"]))]
    _check_export(model, cams, 24, 0.6, 2)


def test_export_script_writes_a_ply_that_reads_back(tmp_path, capsys):
    import json

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import export_tsdf_mesh as script

    from nerfstudio_thermal_amd.dataparser import read_ply_thermal

    out = str(tmp_path / "mesh")
    assert script.main(["--model", "nerf", "--iterations", "150", "--frames", "3", "--resolution", "24", "--downscale-factor", "4", "--output-dir", out]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["ply"] == os.path.join(out, "tsdf_mesh.ply") and os.path.exists(line["ply"])
    xyz, rgb, thermal = read_ply_thermal(line["ply"])
    faces = _mesh().read_mesh_ply_faces(line["ply"])
    assert xyz.shape[0] == line["vertices"] and faces.shape == (line["faces"], 3) and rgb.shape == (xyz.shape[0], 3) and thermal.shape == (xyz.shape[0], 1)
    assert faces.shape[0] == 0 or (int(faces.min()) >= 0 and int(faces.max()) < xyz.shape[0])
