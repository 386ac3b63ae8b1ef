"""The Poisson mesh export without a GPU: the float64 restatement (poisson_functional.py) on its own -- the operator's symmetry, the sphere -- the
host-side argument checks of every tn_poisson_* entry point, header and binding, the wrapper's refusals, the trim rule and the script's --help."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import poisson_functional as pf
import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib, poisson
from nerfstudio_thermal_amd.cloud import PointCloud
from nerfstudio_thermal_amd.mesh import Mesh

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE_SEED = 0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


# ---- the restatement
def test_restated_operator_is_symmetric():
    """<A x, y> = <x, A y> to float64 round-off on a (5, 4, 6) grid with anisotropic voxels, with and without screening: the stencil with its
    Dirichlet boundary is a symmetric matrix.  Each side is a sum of 120 products of magnitude up to |A x| |y|: 1e-12 relative is ample."""
    grid = pf.Grid((5, 4, 6), np.float32([0, 0, 0]), np.float32([0.11, 0.07, 0.05]))
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(grid.dims, generator=g, dtype=torch.float64), torch.randn(grid.dims, generator=g, dtype=torch.float64)
    for s in (None, torch.rand(grid.dims, generator=g, dtype=torch.float64) * 50):
        a, b = float((pf.apply_ref(x, grid, s)[0] * y).sum()), float((x * pf.apply_ref(y, grid, s)[0]).sum())
        scale = float((pf.apply_ref(x, grid, s)[1] * y.abs()).sum())
        assert abs(a - b) <= 1e-12 * scale, (a, b)
        assert float((pf.apply_ref(x, grid, s)[0] * x).sum()) > 0  # and positive definite along x


def test_restatement_reconstructs_the_sphere_within_an_eighth_of_a_voxel():
    """8000 points on the sphere of radius 0.5 with exact outward normals (seed 0), 32^3 over [-1, 1]^3, tol 1e-3, density weighting on: every
    sign change along a lattice edge crosses within 0.125 voxel of the sphere (measured with this seed: 0.080 voxel), and the sign is the
    extractor's: negative at the centre, positive at the corner."""
    pts, nrm = pf.sphere_cloud(8000, 0.5, SPHERE_SEED)
    rec = pf.reconstruct_ref(pts, nrm, 32, ((-1, -1, -1), (1, 1, 1)), tol=1e-3)
    assert 0 < rec["iterations"] < 128 and rec["rr"] <= 1e-6 * rec["bb"]
    cross = pf.edge_crossings(rec["values"], rec["grid"])
    voxel = 2.0 / 31.0
    err = float((cross.norm(dim=1) - 0.5).abs().max()) / voxel
    print(f"sphere, 32^3: {cross.shape[0]} crossings, worst distance from the sphere {err:.4f} voxel, {rec['iterations']} iterations, iso {rec['iso']:.4e}")
    assert cross.shape[0] > 1000 and err <= 0.125
    v = rec["values"]
    assert v.dtype == torch.float32 and float(v.abs().max()) == 1.0
    assert float(v[15, 15, 15]) < 0 and float(v[16, 16, 16]) < 0 and float(v[0, 0, 0]) > 0 and float(v[31, 31, 31]) > 0


def test_restated_projection_puts_the_diagonal_crossings_back_on_the_sphere():
    """The same sphere.  The extractor's tetrahedra also have face and body diagonals; the linear zero along those misses the sphere by up to
    0.2967 voxel (measured with this seed; the solution is an S-curve across the surface and the chord is 1.7 voxels long), more than the 0.25 the
    mesh is held to.  Two Newton steps onto the zero level of the trilinear interpolant (project_ref) bring every crossing within the 0.125 voxel
    the axis crossings are held to (measured: 0.079)."""
    pts, nrm = pf.sphere_cloud(8000, 0.5, SPHERE_SEED)
    rec = pf.reconstruct_ref(pts, nrm, 32, ((-1, -1, -1), (1, 1, 1)), tol=1e-3)
    cross = pf.edge_crossings(rec["values"], rec["grid"], diagonals=True)
    voxel = 2.0 / 31.0
    raw = float((cross.norm(dim=1) - 0.5).abs().max()) / voxel
    moved = pf.project_ref(cross.float(), rec["values"], rec["grid"], 2).double()
    err = float((moved.norm(dim=1) - 0.5).abs().max()) / voxel
    print(f"sphere, 32^3, all seven edge kinds: {cross.shape[0]} crossings, worst distance {raw:.4f} voxel as chords, {err:.4f} after the projection")
    assert cross.shape[0] > 3000 and raw > 0.25 and err <= 0.125
    assert torch.equal(pf.project_ref(cross.float(), rec["values"], rec["grid"], 0), cross.float())


def test_restated_splat_partitions_unity_and_skips_what_the_rule_skips():
    grid = pf.Grid((4, 3, 5), np.float32([-1, 0, 1]), np.float32([0.5, 0.25, 0.125]))
    pts = torch.tensor([[-0.9, 0.1, 1.3], [-1.0, 0.0, 1.0], [0.5, 0.5, 1.5], [0.49, 0.49, 1.49], [float("nan"), 0.1, 1.1], [-1.1, 0.1, 1.1]])
    out, mag, den = pf.splat_ref(pts, grid)
    kept = pf.bin_ref(pts, grid)[0]
    assert kept.tolist() == [True, True, False, True, False, False]  # the upper outer faces, a NaN and a point below the grid are skipped
    assert abs(float(out.sum()) - 3.0) <= 1e-12 and float(out[0, 0, 0, 0]) >= 1.0  # each kept point spreads a weight of 1; one sits on a lattice point
    w = torch.tensor([1.0, 2.0, 1.0, float("inf"), 1.0, 1.0])
    assert abs(float(pf.splat_ref(pts, grid, None, w)[0].sum()) - 3.0) <= 1e-12  # the infinite weight is skipped: 1 + 2
    nrm = pf.splat_ref(pts, grid, torch.full((6, 2), 0.25), None, normalize=True)[0]
    assert bool(((nrm == 0) | ((nrm - 0.25).abs() <= 1e-15)).all()) and bool((nrm[den <= 0] == 0).all())


# ---- the entry points refuse bad arguments on the host
def test_every_entry_point_refuses_bad_arguments_before_any_launch(lib):
    fake, n = C.c_void_p(256 * 4096), 1000
    dims, org, vox = (17, 9, 33), (0.0, 0.0, 0.0), (0.11, 0.07, 0.05)
    need = lib.tn_poisson_workspace_bytes(n, *dims)
    assert need > 0 and lib.tn_poisson_workspace_bytes(0, *dims) == 0
    for bad in ((n, 1, 9, 33), (n, 17, 9, 0), (n, 2048, 1024, 1024), (2**31, *dims), (-1, *dims)):
        assert lib.tn_poisson_workspace_bytes(*bad) == -1, bad
    sneed = lib.tn_poisson_solve_workspace_bytes(*dims)
    assert sneed >= 3 * 4 * 17 * 9 * 33 and lib.tn_poisson_solve_workspace_bytes(1, 9, 33) == -1 and lib.tn_poisson_solve_workspace_bytes(2048, 1024, 1024) == -1
    bad_dims = ((1, 9, 33), (17, 9, 1), (2048, 1024, 1024))
    bad_vox = ((0.0, 0.07, 0.05), (0.11, -1.0, 0.05), (0.11, 0.07, float("inf")), (float("nan"), 0.07, 0.05))

    def bin_(points=fake, n=n, dims=dims, org=org, vox=vox, ws=fake, ws_bytes=need):
        return lib.tn_poisson_bin(points, n, *dims, *org, *vox, ws, ws_bytes, None)

    def splat(points=fake, n=n, values=fake, ch=3, weights=fake, normalize=0, dims=dims, org=org, vox=vox, out=fake, ws=fake, ws_bytes=need):
        return lib.tn_poisson_splat(points, n, values, ch, weights, normalize, *dims, *org, *vox, out, ws, ws_bytes, None)

    def sample(points=fake, n=n, volume=fake, dims=dims, org=org, vox=vox, out=fake):
        return lib.tn_poisson_sample(points, n, volume, *dims, *org, *vox, out, None)

    def div(field=fake, dims=dims, vox=vox, out=fake):
        return lib.tn_poisson_divergence(field, *dims, *vox, out, None)

    def apply(x=fake, s=None, dims=dims, vox=vox, out=C.c_void_p(512 * 4096)):
        return lib.tn_poisson_apply(x, s, *dims, *vox, out, None)

    record = (C.c_double * 3)()

    def solve(b=fake, s=None, x=fake, dims=dims, vox=vox, tol=1e-3, max_it=10, every=5, rec=record, ws=fake, ws_bytes=sneed):
        return lib.tn_poisson_solve(b, s, x, *dims, *vox, tol, max_it, every, rec, ws, ws_bytes, None)

    for call in (bin_, splat, sample, div, apply, solve):
        for d in bad_dims:
            assert call(dims=d) == EINVAL and b"lattice" in lib.tn_last_error(), (call.__name__, d)
        for v in bad_vox:
            assert call(vox=v) == EINVAL and b"voxel" in lib.tn_last_error(), (call.__name__, v)
    for call in (bin_, splat, sample):
        assert call(n=2**31) == EINVAL and call(n=-1) == EINVAL, call.__name__
        assert call(org=(float("nan"), 0.0, 0.0)) == EINVAL and b"origin" in lib.tn_last_error()
        assert call(points=None) == EINVAL and b"null pointer" in lib.tn_last_error()
    for call, names in ((bin_, ("ws",)), (splat, ("out", "ws")), (sample, ("volume", "out")), (div, ("field", "out")), (apply, ("x", "out")),
                        (solve, ("b", "x", "rec", "ws"))):
        for name in names:
            assert call(**{name: None}) == EINVAL and b"null pointer" in lib.tn_last_error(), (call.__name__, name)
    for ch in (0, 5, -1):
        assert splat(ch=ch) == EINVAL and b"C =" in lib.tn_last_error()
    assert splat(values=None, ch=3) == EINVAL  # no values: the density, one channel
    assert splat(normalize=2) == EINVAL
    assert bin_(ws_bytes=need - 1) == EINVAL and b"workspace of" in lib.tn_last_error()
    assert splat(ws_bytes=need - 1) == EINVAL and b"workspace of" in lib.tn_last_error()
    assert solve(ws_bytes=sneed - 1) == EINVAL and b"workspace of" in lib.tn_last_error()
    assert bin_(ws=C.c_void_p(256 * 4096 + 64)) == EINVAL and solve(ws=C.c_void_p(256 * 4096 + 64)) == EINVAL
    assert solve(tol=-1e-3) == EINVAL and b"tol" in lib.tn_last_error()
    assert solve(tol=float("nan")) == EINVAL
    assert solve(max_it=-1) == EINVAL and b"max_iterations" in lib.tn_last_error()
    assert solve(every=0) == EINVAL and b"check_every" in lib.tn_last_error()
    assert apply(x=fake, out=fake) == EINVAL  # in place
    # n == 0 is TN_OK and touches nothing
    assert lib.tn_poisson_bin(None, 0, *dims, *org, *vox, None, 0, None) == 0
    assert lib.tn_poisson_sample(None, 0, None, *dims, *org, *vox, None, None) == 0


def test_header_binding_and_kernel_constants_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "thermal_nerf_hip.h"), encoding="utf-8").read()
    src = open(os.path.join(ROOT, "nerfstudio-thermal_amd", "csrc", "tn_poisson.hip"), encoding="utf-8").read()
    assert _lib.ABI_VERSION == 314 and lib.tn_version() == 314  # additions only: the version stays
    names = ("tn_poisson_workspace_bytes", "tn_poisson_bin", "tn_poisson_splat", "tn_poisson_sample", "tn_poisson_divergence", "tn_poisson_apply",
             "tn_poisson_solve_workspace_bytes", "tn_poisson_solve")
    for name in names:
        decl = re.search(r"TN_API\s+\w+\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert decl is not None, name
        res, argtypes = _lib.SIGNATURES[name]
        assert len(decl.group(1).split(",")) == len(argtypes), name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res
    assert int(re.search(r"#define POISSON_BLOCK (\d+)", src).group(1)) == poisson.SOLVE_BLOCK
    assert int(re.search(r"#define POISSON_MAX_BLOCKS (\d+)", src).group(1)) == poisson.SOLVE_MAX_BLOCKS
    build = open(os.path.join(ROOT, "nerfstudio-thermal_amd", "csrc", "build.sh"), encoding="utf-8").read()
    assert build.count("tn_poisson") == 2  # compiled and linked


# ---- the wrapper
def test_poisson_reconstruct_refuses_a_cloud_without_normals_and_host_tensors():
    pc = PointCloud(torch.zeros(40, 3), torch.zeros(40, 3), torch.zeros(40, 1))
    with pytest.raises(ValueError, match="estimate_normals"):
        poisson.poisson_reconstruct(pc)
    pc.normals = torch.zeros(40, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        poisson.poisson_reconstruct(pc, resolution=16)
    with pytest.raises(ValueError, match="lattice"):
        poisson.Grid.over_box(((-1, -1, -1), (1, 1, 1)), 1)
    with pytest.raises(ValueError, match="box"):
        poisson.Grid.over_box(((-1, -1, -1), (1, -1, 1)), 8)
    g = poisson.Grid.over_box(((-1, -1, -1), (1, 1, 1)), (32, 16, 8))
    r = pf.grid_over_box(((-1, -1, -1), (1, 1, 1)), (32, 16, 8))
    assert g.dims == r.dims and np.array_equal(g.origin, r.origin) and np.array_equal(g.voxel, r.voxel) and g.voxel.dtype == np.float32
    assert poisson.DENSITY_FLOOR == pf.DENSITY_FLOOR


def _six_vertex_mesh():
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [1, 1, 0], [2, 1, 0]])
    f = torch.tensor([[0, 1, 3], [1, 4, 3], [1, 2, 4], [2, 5, 4]], dtype=torch.int32)
    return Mesh(v, f, torch.tensor([[0.0, 0, 1]]).repeat(6, 1), torch.arange(24, dtype=torch.float32).reshape(6, 4))


def test_trim_rule_on_a_hand_made_mesh():
    m = _six_vertex_mesh()
    d = torch.tensor([5.0, 4.0, 0.5, 6.0, 3.0, 1.0], dtype=torch.float64)
    # q = 0.3: pos = 1.5 between the sorted 1.0 and 3.0 -> 2.0; the vertices 2 (0.5) and 5 (1.0) go, and with them the faces 2 and 3
    assert abs(poisson.quantile_threshold(d, 0.3) - 2.0) <= 1e-15 and abs(pf.quantile_ref(d.numpy(), 0.3) - 2.0) <= 1e-15
    t = poisson.trim_mesh(m, d, 0.3)
    assert t.vertices.tolist() == m.vertices[[0, 1, 3, 4]].tolist() and t.faces.dtype == torch.int32
    assert t.faces.tolist() == [[0, 1, 2], [1, 3, 2]]
    assert t.rgbt.tolist() == m.rgbt[[0, 1, 3, 4]].tolist() and t.normals.shape == (4, 3)
    keep, faces = pf.trim_ref(6, m.faces.numpy(), d.numpy(), 0.3)
    assert keep.tolist() == [True, True, False, True, True, False] and faces.tolist() == t.faces.tolist()
    # a vertex AT the threshold stays (strictly below goes); q = 0 returns the mesh itself; q = 1 keeps the maximum only, and no face
    assert poisson.trim_mesh(m, d, 0.0) is m
    t1 = poisson.trim_mesh(m, d, 1.0)
    assert t1.vertices.tolist() == [[0.0, 1.0, 0.0]] and t1.faces.shape == (0, 3)
    at = poisson.trim_mesh(m, torch.tensor([1.0, 1, 1, 1, 1, 1], dtype=torch.float64), 0.5)
    assert at.vertices.shape == (6, 3) and at.faces.tolist() == m.faces.tolist()
    with pytest.raises(ValueError, match="trim_quantile"):
        poisson.trim_mesh(m, d, 1.5)
    with pytest.raises(ValueError, match="densities"):
        poisson.trim_mesh(m, d[:5], 0.3)


def test_level_volume_matches_the_restatement():
    g = torch.Generator().manual_seed(3)
    phi = torch.randn((4, 5, 6), generator=g)
    at = torch.randn(50, generator=g, dtype=torch.float64)
    w = torch.rand(50, generator=g)
    kept = torch.rand(50, generator=g) > 0.2
    w[3], at[7] = float("nan"), float("nan")
    a, iso_a = poisson.level_volume(phi, at, w, kept)
    b, iso_b = pf.level_ref(phi, at, w, kept)
    assert abs(iso_a - iso_b) <= 1e-14 and float((a - b).abs().max()) <= 2.0**-23 and float(a.abs().max()) == 1.0


def test_export_script_help_names_the_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "export_poisson_mesh.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--resolution", "--num-points", "--trim-quantile", "--screening", "--target-num-faces", "--texture", "--save-point-cloud", "--from-ply"):
        assert flag in r.stdout, flag
