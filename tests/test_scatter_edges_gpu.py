"""tn_hash_scatter against the float64 reference of tests/scatter_cases.py at its run and bucket edges, on every path: TN_SCATTER_MODE 2
(segmented), 1 (binned), 0 (atomics with dense replicas) and without a workspace; into a zeroed table gradient with the table_grad_is_zero
promise, and adding into a prefilled one.  tests/test_scatter_cases_cpu.py asserts that each case reaches the edge it is named for.

Per slot, with u = 2^-24:  |got - (prefill + ref)| <= (8 + R + F) u A + u |prefill + ref|  (terms: scatter_cases); slots with A == 0 hold the
prefill bit for bit; everything is finite.  The worst err / (u A) of every case and path is printed.

The ray cases add d origins / d directions (the three reductions of the d-position variant: a wave inside one group of 4 rays, waves that
straddle two groups, a last group of 3 rays) against float64 autograd through orc.unit_cube_positions and orc.hash_encode, at 2e-4 of the
largest entry -- the bound of test_hash_scatter_matches_autograd_of_hash_encode.  The sharper reference does not extend to d position: on G16
autograd forms the positions and p * res in float64 where the kernel forms them in float32, and d position is a sum of cell-wise constant
slopes -- a sample that the two precisions put on different sides of a lattice plane gets the slope of another cell (measured with the first
ray seed on G16: 3.5e-2 of the largest entry, the same on all four paths).  The ray cases therefore take the first seed of synth_rays_simple
whose samples fall into the same cells in both precisions (scatter_cases.cells_agree, asserted in tests/test_scatter_cases_cpu.py): a condition
on the inputs, not on what the kernel returns.  Measured then: at most 1.7e-4 (d directions on G16, where the far samples weigh in with
their distance), equal on all four paths to three digits -- the float32 positions, not the order of the reduction's atomics."""
import pytest
import torch

import scatter_cases as sc
import thermal_nerfacto_oracle as orc
from nerfstudio_thermal_amd import ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATHS = ("2", "1", "0", "nows")
_DEVICE = {}


def _on_device(name):
    if name not in _DEVICE:
        c = sc.case(name)
        T = 1 << c.log2T
        table = torch.from_numpy(synth.uniform("sc_table_" + c.grid, (c.L * T, 2), seed=3)) * 0.5
        _DEVICE[name] = dict(table=table, d_table=table.to(DEV), o=c.origins.to(DEV), d=c.directions.to(DEV), e=c.e_bins.to(DEV).contiguous(),
                             g=c.g_enc().to(DEV))
    return _DEVICE[name]


def _run(name, path, monkeypatch, pre, zero):
    c, t = sc.case(name), _on_device(name)
    monkeypatch.setenv("TN_SCATTER_MODE", "2" if path == "nows" else path)
    tg = pre.to(DEV).clone()
    d_o = torch.zeros((c.N, 3), device=DEV) if c.want_dpos else None
    d_d = torch.zeros((c.N, 3), device=DEV) if c.want_dpos else None
    ops.hash_scatter(t["d_table"], tg, c.L, c.log2T, c.res.tolist(), t["o"], t["d"], t["e"], t["g"], d_o, d_d, use_workspace=path != "nows",
                     grad_is_zero=zero)
    torch.cuda.synchronize()
    return tg.cpu(), (d_o.cpu() if c.want_dpos else None), (d_d.cpu() if c.want_dpos else None)


def _check_table(name, path, got, pre, what):
    c, cen = sc.case(name), sc.case_census(name)
    ref, A, count = sc.case_reference(name)
    R, F = sc.addends(c, cen, count, path)
    want = pre.double() + ref
    err = (got.double() - want).abs()
    bound = (8.0 + R + F)[:, None] * sc.U * A + sc.U * want.abs()
    live = A > 0
    ratios = err[live] / (sc.U * A[live])
    at = int(ratios.argmax())
    ratio = float(ratios[at])
    print(f"{name} path {path} {what}: worst err / (u A) = {ratio:.2f} where {float((bound[live] / (sc.U * A[live]))[at]):.1f} is allowed; "
          f"R = {R}, largest F = {float(F[live.any(dim=1)].max()):.0f}")
    assert torch.isfinite(got).all()
    assert torch.equal(got[~live], pre[~live]), "a slot nothing is added to changed"
    worst = float((err - bound).max())
    assert worst <= 0.0, (name, path, what, worst, ratio)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(sc.POINT_CASES))
def test_point_cases_table_gradient(name, path, monkeypatch):
    ref, A, count = sc.case_reference(name)
    zeros = torch.zeros(A.shape, dtype=torch.float32)
    got, _, _ = _run(name, path, monkeypatch, zeros, True)
    _check_table(name, path, got, zeros, "store")
    pre = sc.prefill(sc.case(name), A, count)
    got, _, _ = _run(name, path, monkeypatch, pre, False)
    _check_table(name, path, got, pre, "add")


_DPOS = {}


def _dpos_reference(name):
    if name not in _DPOS:
        c, t = sc.case(name), _on_device(name)
        o = c.origins.double().requires_grad_(True)
        d = c.directions.double().requires_grad_(True)
        smp = orc.Samples(s_bins=c.e_bins.double(), e_bins=c.e_bins.double())  # (the cells these positions fall into: scatter_cases.cells_agree)
        p, _ = orc.unit_cube_positions(smp.positions(o, d))
        enc = orc.hash_encode(p.view(-1, 3), t["table"].double(), c.res.double(), c.log2T)
        (enc * c.g.double().reshape(c.P, 2 * c.L)).sum().backward()
        _DPOS[name] = (o.grad, d.grad)
    return _DPOS[name]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(sc.RAY_CASES))
def test_ray_cases_table_gradient_and_d_position(name, path, monkeypatch):
    ref, A, count = sc.case_reference(name)
    ref_o, ref_d = _dpos_reference(name)
    for what, pre, zero in (("store", torch.zeros(A.shape, dtype=torch.float32), True), ("add", sc.prefill(sc.case(name), A, count), False)):
        got, d_o, d_d = _run(name, path, monkeypatch, pre, zero)
        _check_table(name, path, got, pre, what)
        for tag, g_, r_ in (("d_origins", d_o, ref_o), ("d_directions", d_d, ref_d)):
            scale = float(r_.abs().max())
            err = float((g_.double() - r_).abs().max())
            print(f"{name} path {path} {what} {tag}: err {err:.3e} scale {scale:.3e} ratio {err / scale:.2e}")
            assert torch.isfinite(g_).all() and scale > 0
            assert err <= 2e-4 * scale, (tag, err, scale)
