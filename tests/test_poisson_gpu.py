"""The Poisson mesh export on the GPU: every tn_poisson_* entry point against the float64 restatement (poisson_functional.py), the solve's
determinism and stop rule, and the pipeline end to end on an analytic sphere, closed and open.

The bounds are derived, not tuned.  An fp32 output is one rounding of a double-precision sum: 2^-24 relative to the sum, which is at most the sum
of the absolute values of its terms; the project's factor 8 gives 2^-21 times that sum, which the restatement returns.  The double-precision
sample repeats the restatement's operations in its order, so 2^-50 (8 x 2^-53) times the same kind of sum is ample.  A solve is compared with the
float64 restatement within 8 x the deviation of the restatement run with fp32 storage -- the project's "8 x the float32 oracle's own error"."""
import os
import warnings

import numpy as np
import pytest
import torch

import poisson_functional as pf

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32_BOUND, F64_BOUND = 2.0**-21, 2.0**-50
MAIN = ((17, 9, 33), (-0.5, 0.1, -0.3), (0.11, 0.07, 0.05))
UNIT_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
_CACHE = {}


def _poisson():
    from nerfstudio_thermal_amd import poisson

    return poisson


def _grid(dims, origin=(0.0, 0.0, 0.0), voxel=(0.11, 0.07, 0.05)):
    return _poisson().Grid(tuple(dims), np.float32(origin), np.float32(voxel))


def main_cloud():
    """On the MAIN grid: 3000 uniform points inside it, 500 copies of one point, 30 points on lattice points (as exactly as fp32 has them), 40 on the
    grid's outer faces (lower and upper), 50 outside, 5 rows with a NaN or an infinity -> (points [3625,3] fp32, values [n,4], weights [n]); the
    values carry one NaN row and the weights one NaN and one infinity, on kept points."""
    if "cloud" in _CACHE:
        return _CACHE["cloud"]
    dims, origin, voxel = MAIN
    g = torch.Generator().manual_seed(11)
    o, h, d = torch.tensor(origin, dtype=torch.float64), torch.tensor(np.float32(voxel)).double(), torch.tensor(dims, dtype=torch.float64)
    ext = (d - 1) * h
    uniform = o + torch.rand((3000, 3), generator=g, dtype=torch.float64) * ext
    dup = (o + torch.tensor([0.37, 0.61, 0.23], dtype=torch.float64) * ext).repeat(500, 1)
    ijk = torch.stack([torch.randint(0, int(k), (30,), generator=g) for k in dims], 1).double()
    lattice = o + ijk * h
    faces = o + torch.rand((40, 3), generator=g, dtype=torch.float64) * ext
    for r in range(40):
        faces[r, r % 3] = o[r % 3] if (r // 3) % 2 == 0 else o[r % 3] + ext[r % 3]
    outside = o + (torch.rand((50, 3), generator=g, dtype=torch.float64) * 3 - 1) * ext
    axis = torch.arange(50) % 3
    outside[torch.arange(50), axis] = torch.where(torch.arange(50) % 2 == 0, o[axis] - 0.3 * ext[axis], o[axis] + 1.3 * ext[axis])
    bad = uniform[:5].clone()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4] = float("nan"), float("inf"), -float("inf"), float("nan"), float("nan")
    pts = torch.cat([uniform, dup, lattice, faces, outside, bad]).float()
    n = pts.shape[0]
    assert n == 3625
    values = torch.randn((n, 4), generator=g)
    weights = 0.5 + 1.5 * torch.rand(n, generator=g)
    values[17, 2], weights[23], weights[3001] = float("nan"), float("inf"), float("nan")
    _CACHE["cloud"] = (pts, values, weights)
    return _CACHE["cloud"]


def run_splat(points, grid, values=None, weights=None, normalize=False):
    po = _poisson()
    p = points.to(DEV).contiguous()
    ws = po.plan_workspace(p.shape[0], grid, DEV)
    po.bin_call(p, grid, ws)
    ch = 1 if values is None else values.shape[1]
    out = torch.full((*grid.dims, ch), float("nan"), device=DEV)
    po.splat_call(p, None if values is None else values.to(DEV).contiguous(), None if weights is None else weights.to(DEV).contiguous(), normalize, grid,
                  out, ws)
    return out.cpu()


def check(got, ref, mag, bound, what):
    err = (got.double() - ref).abs()
    worst = float((err / mag.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max |got - ref| {float(err.max()) if err.numel() else 0.0:.3e}, worst error over its bound's scale {worst:.3e} (bound {bound:.3e})")
    assert bool(torch.isfinite(got).all()), what
    assert bool((err <= bound * mag).all()), what


# ---------------------------------------------------------------------------------------------------- splat
@pytest.mark.parametrize("with_weights", [False, True])
@pytest.mark.parametrize("channels", [1, 3, 4])
def test_splat_matches_the_restatement(channels, with_weights):
    pts, values, weights = main_cloud()
    grid = _grid(*MAIN)
    v = None if channels == 1 else values[:, :channels].contiguous()
    w = weights if with_weights else None
    ref, mag, _ = pf.splat_ref(pts, grid, v, w)
    got = run_splat(pts, grid, v, w)
    check(got, ref, mag, F32_BOUND, f"splat C = {channels}, weights {with_weights}")
    assert bool((got[mag == 0] == 0).all())  # where nothing lands the output is exactly zero
    assert torch.equal(got.view(torch.int32), run_splat(pts, grid, v, w).view(torch.int32))  # the same bits every run
    if channels == 1 and not with_weights:  # every kept point spreads a weight of exactly 1: the 50 outside and the 5 non-finite rows add nothing
        kept = int(pf.bin_ref(pts, grid)[0].sum())
        assert 3500 < kept < 3625 - 55 + 1 and abs(float(got.double().sum()) - kept) <= F32_BOUND * kept


def test_splat_normalised_form_is_zero_where_the_density_is_zero():
    pts, values, weights = main_cloud()
    grid = _grid(*MAIN)
    ref, mag, den = pf.splat_ref(pts, grid, values, weights, normalize=True)
    got = run_splat(pts, grid, values, weights, normalize=True)
    check(got, ref, mag, F32_BOUND, "normalised splat")
    assert int((den <= 0).sum()) > 0 and bool((got[den <= 0] == 0).all())


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_splat_block_edges_and_the_empty_cloud(n):
    pts, values, _ = main_cloud()
    grid = _grid(*MAIN)
    p, v = pts[:n].contiguous(), values[:n, :3].contiguous()
    ref, mag, _ = pf.splat_ref(p, grid, v)
    got = run_splat(p, grid, v)
    check(got, ref, mag, F32_BOUND, f"splat n = {n}")
    if n == 0:
        assert bool((got == 0).all()) and bool((run_splat(p, grid) == 0).all())


def test_splat_on_the_smallest_grid():
    grid = _grid((2, 2, 2), (0.25, -0.5, 1.0), (0.11, 0.07, 0.05))
    g = torch.Generator().manual_seed(2)
    pts = (torch.tensor([0.25, -0.5, 1.0]) + (torch.rand((300, 3), generator=g) * 1.4 - 0.2) * torch.tensor([0.11, 0.07, 0.05])).float()
    v = torch.randn((300, 4), generator=g)
    ref, mag, _ = pf.splat_ref(pts, grid, v)
    assert 50 < int(pf.bin_ref(pts, grid)[0].sum()) < 300
    check(run_splat(pts, grid, v), ref, mag, F32_BOUND, "splat (2, 2, 2)")


# ---------------------------------------------------------------------------------------------------- sample
def test_sample_matches_the_restatement_and_gives_nan_for_nan():
    po = _poisson()
    pts, _, _ = main_cloud()
    grid = _grid(*MAIN)
    vol = torch.randn(grid.dims, generator=torch.Generator().manual_seed(4))
    ref, mag = pf.sample_ref(pts, vol, grid)
    got = po.sample(pts.to(DEV), vol.to(DEV), grid).cpu()
    assert got.dtype == torch.float64
    bad = torch.isnan(ref)
    assert int(bad.sum()) == 5 and torch.equal(torch.isnan(got), bad)
    err = (got[~bad] - ref[~bad]).abs()
    print(f"sample: max error {float(err.max()):.3e}, worst over scale {float((err / mag[~bad].clamp_min(1e-300)).max()):.3e} (bound {F64_BOUND:.3e})")
    assert bool((err <= F64_BOUND * mag[~bad]).all())
    small = _grid((2, 2, 2))
    v2 = torch.arange(8, dtype=torch.float32).reshape(2, 2, 2)
    p2 = torch.tensor([[0.0, 0.0, 0.0], [0.11, 0.07, 0.05], [0.055, 0.035, 0.025], [5.0, -3.0, 0.01]])
    r2, m2 = pf.sample_ref(p2, v2, small)
    assert bool(((po.sample(p2.to(DEV), v2.to(DEV), small).cpu() - r2).abs() <= F64_BOUND * m2).all())


# ---------------------------------------------------------------------------------------------------- divergence and operator
GRIDS = [(2, 2, 2), (17, 9, 33), (5, 64, 65), (3, 3, 129)]


@pytest.mark.parametrize("dims", GRIDS)
def test_divergence_matches_the_restatement(dims):
    po = _poisson()
    grid = _grid(dims)
    V = torch.randn((*dims, 3), generator=torch.Generator().manual_seed(sum(dims)))
    ref, mag = pf.divergence_ref(V, grid)
    out = torch.full(dims, float("nan"), device=DEV)
    po.divergence_call(V.to(DEV), grid, out)
    check(out.cpu(), ref, mag, F32_BOUND, f"divergence {dims}")


@pytest.mark.parametrize("screened", [False, True])
@pytest.mark.parametrize("dims", GRIDS)
def test_operator_matches_the_restatement(dims, screened):
    po = _poisson()
    grid = _grid(dims)
    g = torch.Generator().manual_seed(sum(dims) + 1)
    x = torch.randn(dims, generator=g)
    s = torch.rand(dims, generator=g) * 300 if screened else None
    ref, mag = pf.apply_ref(x, grid, s)
    out = torch.full(dims, float("nan"), device=DEV)
    po.apply_call(x.to(DEV), None if s is None else s.to(DEV), grid, out)
    check(out.cpu(), ref, mag, F32_BOUND, f"operator {dims}, screening {screened}")


# ---------------------------------------------------------------------------------------------------- solve
def run_solve(b, grid, s=None, x0=None, tol=1e-3, max_iterations=100, check_every=25):
    po = _poisson()
    x = torch.zeros(grid.dims, device=DEV) if x0 is None else x0.to(DEV).clone()
    rec = po.solve_call(b.to(DEV), None if s is None else s.to(DEV), x, grid, tol, max_iterations, check_every, po.solve_workspace(grid, DEV))
    return x.cpu(), rec


def check_fixed_length(dims, iterations, screened, what):
    grid = _grid(dims)
    g = torch.Generator().manual_seed(sum(dims) + 2)
    b = torch.randn(dims, generator=g)
    s = torch.rand(dims, generator=g) * 300 if screened else None
    x64, it64, _, _ = pf.cg_ref(b, grid, s, None, 0.0, iterations, fp32_storage=False)
    x32, it32, rr32, bb32 = pf.cg_ref(b, grid, s, None, 0.0, iterations, fp32_storage=True)
    x, (it, rr, bb) = run_solve(b, grid, s, tol=0.0, max_iterations=iterations, check_every=2)
    own = float((x32 - x64).abs().max())
    err = float((x.double() - x64).abs().max())
    print(f"{what}: max |x - x64| {err:.3e}, the fp32-storage restatement's own {own:.3e} (bound 8 x); r.r {rr:.6e} (restated {rr32:.6e})")
    assert it == it64 == it32 == iterations
    assert own > 0 and err <= 8 * own
    assert abs(bb - bb32) <= 1e-12 * bb32 and abs(rr - rr32) <= 1e-3 * rr32
    return x


@pytest.mark.parametrize("screened", [False, True])
def test_solve_of_fixed_length_matches_the_restatement(screened):
    """tol = 0, max_iterations = 5 on (17, 9, 33) with a random right-hand side"""
    check_fixed_length((17, 9, 33), 5, screened, f"5 iterations, screening {screened}")


@pytest.mark.parametrize("dims", [(41, 41, 41), (65, 64, 65)])
def test_solve_where_the_partials_exceed_one_fold_pass(dims):
    """A dot product is one partial per block of SOLVE_BLOCK lattice points, folded by blocks of SOLVE_BLOCK threads: above SOLVE_BLOCK^2 points a
    thread folds more than one partial ((41, 41, 41): 270 partials); above SOLVE_BLOCK x SOLVE_MAX_BLOCKS points the launches are grid-stride
    ((65, 64, 65): 1024 partials, some threads take a second element).  3 iterations, the same 8 x bound."""
    po = _poisson()
    total = dims[0] * dims[1] * dims[2]
    assert total > po.SOLVE_BLOCK ** 2 and (dims[0] < 65 or total > po.SOLVE_BLOCK * po.SOLVE_MAX_BLOCKS)
    check_fixed_length(dims, 3, False, f"3 iterations on {dims}")


def sphere_refs():
    """The restatement of the pipeline on the sphere (8000 points, radius 0.5, seed 0, 32^3 over [-1, 1]^3, tol 1e-3), in float64 and with fp32 storage"""
    if "sphere" not in _CACHE:
        pts, nrm = pf.sphere_cloud(8000, 0.5, 0)
        _CACHE["sphere"] = (pts, nrm, pf.reconstruct_ref(pts, nrm, 32, UNIT_BOX, tol=1e-3), pf.reconstruct_ref(pts, nrm, 32, UNIT_BOX, tol=1e-3, fp32_storage=True))
    return _CACHE["sphere"]


def test_solve_converges_on_the_sphere_and_its_bits_do_not_depend_on_the_read_backs():
    """32^3, the sphere's right-hand side, tol 1e-3.  The true residual |b - A x| / |b|, in float64 on the host, is at most 2e-3: fp32 CG's floor
    here is kappa 2^-24 ~ 3e-5 (kappa ~ 4 33^2 / pi^2), so the recursive residual drifts from the true one by a few percent of tol."""
    _, _, _, r32 = sphere_refs()
    grid, b = _poisson().Grid(r32["grid"].dims, r32["grid"].origin, r32["grid"].voxel), r32["b"].float()
    x, (it, rr, bb) = run_solve(b, grid, tol=1e-3, max_iterations=128, check_every=25)
    true = float((b.double() - pf.apply_ref(x, grid)[0]).norm() / b.double().norm())
    print(f"converged solve: {it} iterations (fp32-storage restatement: {r32['iterations']}), recursive |r|/|b| {(rr / bb) ** 0.5:.3e}, true {true:.3e}")
    assert rr <= 1e-6 * bb and true <= 2e-3
    assert abs(it - r32["iterations"]) <= 2
    for every in (1, 7, 1000):
        x2, rec2 = run_solve(b, grid, tol=1e-3, max_iterations=128, check_every=every)
        assert rec2 == (it, rr, bb) and torch.equal(x2.view(torch.int32), x.view(torch.int32)), every
    x3, (it3, rr3, _) = run_solve(b, grid, tol=1e-3, max_iterations=3, check_every=25)
    assert it3 == 3 and rr3 > 1e-6 * bb
    x0, (it0, _, _) = run_solve(b, grid, tol=1e-3, max_iterations=0)
    assert it0 == 0 and bool((x0 == 0).all())
    # the solution is a starting guess that already satisfies the stop rule (a little slack for the residual recomputed from x): no iteration
    again, (it_again, _, _) = run_solve(b, grid, x0=x, tol=3e-3, max_iterations=128)
    assert it_again == 0 and torch.equal(again, x)


# ---------------------------------------------------------------------------------------------------- end to end
def sphere_cloud_on_device(rows=None):
    from nerfstudio_thermal_amd.cloud import PointCloud

    pts, nrm, _, _ = sphere_refs()
    if rows is not None:
        pts, nrm = pts[rows], nrm[rows]
    return PointCloud(pts.to(DEV), (pts + 0.5).clamp(0, 1).to(DEV), (pts[:, 2:] + 0.5).clamp(0, 1).to(DEV), None, nrm.to(DEV))


def edge_use(faces):
    f = faces.long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = torch.sort(e, dim=1).values
    return torch.unique(e, dim=0, return_counts=True)[1]


def sphere_mesh():
    """poisson_reconstruct on the sphere cloud, closed (trim_quantile 0), once for the tests that look at it -> (Mesh, TSDFVolume)"""
    if "sphere mesh" not in _CACHE:
        _CACHE["sphere mesh"] = _poisson().poisson_reconstruct(sphere_cloud_on_device(), resolution=32, box=UNIT_BOX, tol=1e-3, trim_quantile=0.0,
                                                               return_volume=True)
    return _CACHE["sphere mesh"]


def test_sphere_end_to_end_is_closed_oriented_and_coloured():
    _, _, r64, r32 = sphere_refs()
    mesh, volume = sphere_mesh()
    v, f, nrm, rgbt = mesh.vertices.cpu().double(), mesh.faces.cpu(), mesh.normals.cpu().double(), mesh.rgbt.cpu().double()
    voxel = 2.0 / 31.0
    assert v.shape[0] > 1000 and f.shape[0] > 2000 and bool((edge_use(f) == 2).all())  # closed: every edge is shared by exactly two faces
    radial = v / v.norm(dim=1, keepdim=True)
    ndot = float((nrm * radial).sum(1).min())
    a, b, c = (v[f[:, k].long()] for k in range(3))
    wound = float((torch.cross(b - a, c - a, dim=1) * (a + b + c)).sum(1).min())
    colour = float((rgbt - torch.cat([v + 0.5, v[:, 2:] + 0.5], 1)).abs().max()) / voxel
    own = float((r32["values"].double() - r64["values"].double()).abs().max())
    dev = float((volume.values.cpu().double() - r64["values"].double()).abs().max())
    print(f"sphere end to end: {v.shape[0]} vertices, {f.shape[0]} faces, {volume.solve_record[0]} iterations; min n . radial {ndot:.4f}, colour off by "
          f"{colour:.3f} voxel; values deviate {dev:.3e} (fp32-storage restatement: {own:.3e})")
    assert ndot > 0.9 and wound > 0 and colour <= 2.0
    assert float(volume.values.abs().max()) == 1.0
    assert own > 0 and dev <= 8 * own


def test_sphere_end_to_end_every_vertex_within_a_quarter_voxel():
    """Every vertex of the closed mesh within 0.25 voxel of the sphere: twice the 0.125 voxel the restatement is held to along lattice edges.

    As extracted (project_iterations 0) the mesh does not meet this, and no implementation of the stated rules can: the extractor (marching
    tetrahedra on the Freudenthal split, reused unchanged) also puts vertices on face and body diagonals, and the LINEAR zero of the restatement's
    own float64 volume along those lies up to 0.169 and 0.2967 voxel from the sphere (0.079 along axis edges) -- across the surface the solution
    is an S-curve some two voxels wide, and a chord over 1.7 voxels that straddles it unevenly misses by that much.  The pipeline therefore
    projects the vertices onto the zero level of the volume's trilinear interpolant (poisson.project_vertices, two Newton steps), which is within
    0.079 voxel of the sphere everywhere the restatement was evaluated; the raw figure is printed beside the projected one."""
    mesh, volume = sphere_mesh()
    voxel = 2.0 / 31.0
    off = float((mesh.vertices.cpu().double().norm(dim=1) - 0.5).abs().max()) / voxel
    raw = volume.get_mesh().vertices.cpu().double()
    print(f"sphere end to end: worst distance of a vertex from the sphere {off:.4f} voxel (bound 0.25); as extracted, before the projection: "
          f"{float((raw.norm(dim=1) - 0.5).abs().max()) / voxel:.4f}")
    assert off <= 0.25


def test_projection_matches_the_restatement_and_keeps_the_faces():
    """project_vertices against project_ref on the extracted sphere mesh.  The samples are the restatement's bit for bit and a step is float64
    arithmetic rounded once to fp32, so a coordinate (|c| <= 1) differs by a flipped rounding at the most, and a flip in the first step moves the
    second step's input by one ulp: 8 x 2^-24 covers both.  After two steps the vertices lie on the level set: |values(v)| is second order in a step
    of under 0.03 voxel against a gradient of about 0.5 per voxel -- 1e-2 is two orders above that."""
    po = _poisson()
    mesh, volume = sphere_mesh()
    grid = po.Grid(volume.dims, volume.origin.numpy(), volume.voxel_size.numpy())
    raw = volume.get_mesh()
    assert torch.equal(raw.faces, mesh.faces) and torch.equal(raw.rgbt, mesh.rgbt) and torch.equal(raw.normals, mesh.normals)
    got = po.project_vertices(raw.vertices, volume.values, grid, 2)
    assert torch.equal(got, mesh.vertices)  # what the pipeline did
    ref = pf.project_ref(raw.vertices.cpu(), volume.values.cpu(), grid, 2)
    err = float((got.cpu().double() - ref.double()).abs().max())
    moved = float(((got - raw.vertices).cpu().double() / torch.from_numpy(grid.voxel).double()).norm(dim=1).max())
    left = float(po.sample(got, volume.values, grid).abs().max())
    print(f"projection: max |got - ref| {err:.3e} (bound {8 * 2.0**-24:.3e}), largest move {moved:.4f} voxel, |values| left {left:.3e}")
    assert err <= 8 * 2.0**-24 and 0.1 < moved <= 1.0 and left <= 1e-2
    assert torch.equal(po.project_vertices(raw.vertices, volume.values, grid, 0), raw.vertices)
    same = po.poisson_reconstruct(sphere_cloud_on_device(), resolution=32, box=UNIT_BOX, tol=1e-3, trim_quantile=0.0, project_iterations=0)
    assert torch.equal(same.vertices, raw.vertices)


def test_open_surface_is_trimmed_as_the_restatement_trims_it():
    po = _poisson()
    pts = sphere_refs()[0]
    rows = pts[:, 2] > -0.1
    cloud = sphere_cloud_on_device(rows)
    closed, volume = po.poisson_reconstruct(cloud, resolution=32, box=UNIT_BOX, tol=1e-3, trim_quantile=0.0, return_volume=True)
    dens = po.sample(closed.vertices, volume.density, volume.density_grid).cpu().numpy()
    keep, faces = pf.trim_ref(closed.vertices.shape[0], closed.faces.cpu().numpy(), dens, 0.1)
    trimmed = po.poisson_reconstruct(cloud, resolution=32, box=UNIT_BOX, tol=1e-3, trim_quantile=0.1)
    V, Vt = closed.vertices.shape[0], trimmed.vertices.shape[0]
    print(f"open surface: {V} vertices and {closed.faces.shape[0]} faces closed, {Vt} and {trimmed.faces.shape[0]} trimmed")
    assert 0 < V - Vt == int((~keep).sum()) and Vt == int(keep.sum())
    assert np.array_equal(trimmed.faces.cpu().numpy().astype(np.int64), faces)
    assert torch.equal(trimmed.vertices.cpu(), closed.vertices.cpu()[torch.from_numpy(keep)])
    assert int(trimmed.faces.min()) >= 0 and int(trimmed.faces.max()) < Vt  # every face names a kept vertex
    # the trim is not vacuous: what it removes is the cap Poisson closed the hole with, below the lowest points of the cloud
    removed = closed.vertices.cpu()[torch.from_numpy(~keep)]
    assert float(removed[:, 2].max()) < -0.1 + 4 * 2.0 / 31.0 and bool((edge_use(trimmed.faces.cpu()) == 1).any())


class _SphereModel:
    """Renders the sphere |p| = 0.5 analytically: depth = the first hit of the ray, accumulation 1 on a hit and 0 on a miss, colours from the hit."""

    device = torch.device(DEV)
    training = True

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode

    def __call__(self, bundle):
        o, d = bundle.origins, bundle.directions
        b, c = (o * d).sum(-1), (o * o).sum(-1) - 0.25
        disc = b * b - c
        hit = disc > 0
        t = torch.where(hit, -b - torch.sqrt(disc.clamp_min(0)), torch.zeros_like(b))
        p = o + d * t[:, None]
        return {"rgb": (p + 0.5).clamp(0, 1), "rgb_thermal": (p[:, 2:] + 0.5).clamp(0, 1), "depth": t[:, None], "accumulation": hit.float()[:, None]}


def _sphere_bundles():
    from nerfstudio_thermal_amd.rays import RayBundle

    g = torch.Generator().manual_seed(17)
    origins = torch.tensor([[2.0, 0.0, 0.3], [-1.2, 1.6, 0.2], [-0.9, -1.7, -0.5], [0.1, 0.3, 2.0], [0.2, -0.1, -2.0], [-2.0, 0.1, 0.0]])
    bundles = []
    for b in range(12):
        target = (torch.rand((1024, 3), generator=g) - 0.5) * 1.3  # most rays hit the sphere, some pass it
        o = origins[b % 6].repeat(1024, 1)
        d = torch.nn.functional.normalize(target - o, dim=-1)
        bundles.append(RayBundle(origins=o.to(DEV), directions=d.to(DEV), pixel_area=torch.ones(1024, 1, device=DEV)))
    return bundles


class _Replay:
    def __init__(self, bundles):
        self.bundles, self.calls = bundles, 0

    def __call__(self):
        self.calls += 1
        return self.bundles[(self.calls - 1) % len(self.bundles)]


def test_export_poisson_mesh_from_a_model(tmp_path):
    po = _poisson()
    from nerfstudio_thermal_amd import mesh as mesh_mod

    model = _SphereModel()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        full, volume, cloud = po.export_poisson_mesh(model, _Replay(_sphere_bundles()), num_points=4000, resolution=32, trim_quantile=0.0,
                                                     return_volume=True, return_cloud=True)
    assert not any("stopped at the cap" in str(w.message) for w in caught)  # the solve converges
    assert model.training and cloud.normals is not None and 30 <= len(cloud) <= 4000
    assert full.faces.shape[0] > 2000 and float((full.vertices.norm(dim=1) - 0.5).abs().max()) <= 2 * 2.0 / 31.0
    assert tuple(volume.dims) == (32, 32, 32) and volume.solve_record[0] > 0
    small = po.export_poisson_mesh(model, _Replay(_sphere_bundles()), num_points=4000, resolution=32, trim_quantile=0.0, target_num_faces=500)
    assert model.training and 0 < small.faces.shape[0] <= 500 and small.vertices.shape[0] < full.vertices.shape[0]
    path = mesh_mod.write_mesh_ply(str(tmp_path / "poisson_mesh.ply"), small)
    assert os.path.getsize(path) > 0 and mesh_mod.read_mesh_ply_faces(path).shape == (small.faces.shape[0], 3)
    with pytest.warns(UserWarning, match="stopped at the cap"):
        po.poisson_reconstruct(cloud, resolution=32, box=UNIT_BOX, max_iterations=2, trim_quantile=0.0)
