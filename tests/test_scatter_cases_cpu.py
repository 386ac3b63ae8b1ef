"""The scatter cases (tests/scatter_cases.py) without a GPU: the float64 reference against float64 autograd of the oracle's hash encoding
where the two must agree (power-of-two resolutions), and every case's census claims -- a case that no longer reaches the edge it is named for
fails here, not silently on the GPU."""
import numpy as np
import pytest
import torch

import scatter_cases as sc
import thermal_nerfacto_oracle as orc


def _lengths(cen, level):
    return set(int(n) for n in cen["runs"][level][:, 2])


def _starts(cen, level):
    return set(int(n) for n in cen["runs"][level][:, 1])


def test_grids_are_what_the_cases_assume():
    assert sc.grid_res("G5").tolist() == [16.0, 32.0, 64.0, 128.0, 256.0]
    assert sc.grid_res("G20").tolist() == [16.0, 32.0]
    r16 = sc.grid_res("G16")
    assert r16[0] == 16 and r16[-1] == 2047 and any(int(r) & (int(r) - 1) for r in r16)  # non-integral growth: resolutions that are no powers of two
    assert [sc.seg_plan(*sc.GRIDS[g][:2], 1000)["nslices"] for g in ("G5", "G16", "G20")] == [1, 4, 256]


@pytest.mark.parametrize("name", ["lattice", "spread_runs_G5", "rays_7x16_G5_rows"])
def test_reference_equals_float64_autograd_on_power_of_two_grid(name):
    c = sc.case(name)
    ref, A, count = sc.case_reference(name)
    T = 1 << c.log2T
    table = torch.zeros((c.L * T, 2), dtype=torch.float64, requires_grad=True)
    enc = orc.hash_encode(c.p32.double(), table, c.res.double(), c.log2T)
    (enc * c.g.double().reshape(c.P, 2 * c.L)).sum().backward()
    scale = float(ref.abs().max())
    assert scale > 0
    assert float((table.grad - ref).abs().max()) <= 1e-12 * scale
    assert torch.equal(table.grad == 0, ref == 0)
    assert bool((A >= ref.abs() - 1e-12 * scale).all()) and bool(((A == 0) <= (ref == 0)).all())
    assert int(count.sum()) == 8 * c.P * c.L


def test_reference_places_a_selector_zero_point_and_a_lattice_wave():
    c = sc.case("lattice")
    ref, A, count = sc.case_reference("lattice")
    T = 1 << c.log2T
    sel0 = (c.p32 == 0).all(dim=1)
    assert int(sel0.sum()) == 65
    # p = 0: the floor corner with weight 1 and seven corners with weight 0, all in slot hash(0, 0, 0) = 0 of every level
    for l in range(c.L):
        assert int(count[l * T]) >= 8 * 65
    on = c.marks["on_wave"]
    f, cc, o = sc.level_geometry(c.p32[on:on + 64], c.res)
    assert bool((o == 0).all()) and bool((f == cc).all())


@pytest.mark.parametrize("name", ["runs_G5", "runs_G16"])
def test_runs_cases_hold_every_listed_run(name):
    c, cen = sc.case(name), sc.case_census(name)
    assert c.P == sc.RUNS_P and cen["seg"]["NB"] == 3
    for l in range(c.L):  # every level merges, and every run is one cell of every level
        lengths, runs = _lengths(cen, l), cen["runs"][l]
        assert set(sc.RUN_LENGTHS) <= lengths, (l, sorted(set(sc.RUN_LENGTHS) - lengths))
        assert set(sc.RUN_STARTS) <= _starts(cen, l), l
        rows = {(int(w), int(s), int(n)) for w, s, n in runs}
        assert (0, 60, 4) in rows and (1, 0, 4) in rows          # 60..67, cut by the wave boundary
        assert (7, 60, 4) in rows and (8, 0, 4) in rows          # 508..515, cut by the block boundary
        assert (8, 4, 48) in rows                                # over the row boundaries at 16, 32 and 48
        assert (16, 20, 17) in rows                              # ends on the last live lane; the clamped lanes behind it are heads of their own
        assert bool(cen["heads"][l][sc.RUNS_P:].all())
        # the maxlen ladder: waves whose longest run is 1, 2, 3..4, 5..8, 9 and more
        longest = {int(w): int(runs[runs[:, 0] == w][:, 2].max()) for w in np.unique(runs[:, 0])}
        ladder = {1 if n == 1 else 2 if n == 2 else 4 if n <= 4 else 8 if n <= 8 else 16 for n in longest.values()}
        assert ladder == {1, 2, 4, 8, 16}, (l, ladder)
    assert cen["max_run"] == 64


def test_lattice_case_splits_runs_on_the_flags():
    c, cen = sc.case("lattice"), sc.case_census("lattice")
    m = c.marks
    f, cc, o = sc.level_geometry(c.p32, c.res)
    for tag, n_on in (("on1", 1), ("on2", 2), ("on3", 3)):
        i = m[tag]
        for l in range(c.L):
            assert int((o[i, l] == 0).sum()) == n_on and int((o[i + 1, l] == 0).sum()) == 0
            assert torch.equal(f[i, l], f[i + 1, l])  # the same floor cell ...
            assert bool(cen["heads"][l][i + 1])       # ... and still a run of its own
    for l in range(c.L):
        rows = {(int(w), int(s), int(n)) for w, s, n in cen["runs"][l]}
        assert (0, 0, 64) in rows and (2, 0, 64) in rows  # the selector-0 wave and the wave on one lattice point
        i = m["sel0_single"]
        assert (i // 64, i % 64, 1) in rows and bool(cen["heads"][l][i + 1])
        i = m["on_run3"]
        assert (i // 64, i % 64, 3) in rows


def test_hot_slot_and_spread_cases_reach_their_fold_classes():
    classes = {}
    for name in ("hot_slot_G5", "one_cell_G5", "spread_runs_G5", "spread_G5", "spread_G16", "hot_slot_G20"):
        gw = sc.case_census(name)["gw_log2"]
        classes[name] = set(int(x) for x in gw[gw >= 0])
    assert classes["hot_slot_G5"] == {6} and classes["one_cell_G5"] == {4} and classes["spread_runs_G5"] == {5}, classes
    hot = sc.case_census("hot_slot_G5")
    assert hot["max_run"] == 1 and bool((hot["records"] == 4096).all())
    assert bool((sc.case_census("one_cell_G5")["records"] == 64).all()) and sc.case_census("one_cell_G5")["max_run"] == 64
    rec = sc.case_census("spread_runs_G5")["records"]
    assert 96 <= int(rec[:, :-1].min()) and int(rec.max()) <= 255


def test_spread_cases_reach_chunks_odd_and_empty_segments():
    big = sc.case_census("spread_G5")
    assert big["seg"]["NB"] == 65 and big["seg"]["segc"] == 33 and big["seg"]["chunks"] == 2
    assert sc.case_census("spread_G16")["seg"]["chunks"] == 1 and sc.case_census("hot_slot_G20")["seg"]["nslices"] == 256
    cen = sc.case_census("spread_G16")
    assert cen["empty_first"] > 0 and cen["empty_mid"] > 0 and cen["empty_last"] > 0, (cen["empty_first"], cen["empty_mid"], cen["empty_last"])
    # odd record counts need an x corner pair that straddles two buckets: resolution 4096 and more (scatter_cases.GRIDS)
    assert all(sc.case_census(n)["odd_segments"] == 0 for n in sc.POINT_CASES if n != "odd_G8k")
    odd = sc.case_census("odd_G8k")
    assert odd["odd_segments"] > 0 and odd["seg"]["nslices"] == 8
    f, c, _ = sc.level_geometry(sc.case("odd_G8k").p32, sc.case("odd_G8k").res)
    assert bool((f[:, 1, 0] == 4095).all()) and bool((c[:, 1, 0] == 4096).all())
    assert {sc.case_census(n)["seg"]["level_groups"] for n in sc.POINT_CASES} >= {2, 5, 16}


def test_binned_overflow_and_replica_plans():
    cen = sc.case_census("hot_slot_G20")
    assert cen["bin"]["cap"] == 8192 // 16 + 1032
    assert bool(cen["overflow"].any()) and not bool(cen["overflow"].all())
    _, _, count = sc.case_reference("hot_slot_G20")
    assert int(count.max()) >= 4096 > cen["bin"]["cap"]
    for name in sc.POINT_CASES:
        if name != "hot_slot_G20":
            assert not bool(sc.case_census(name)["overflow"].any()), name
    assert int(sc.case_census("spread_G5")["nfold"].max()) > 1  # the binned fold split into chunks that flush with float atomics
    rep = sc.case_census("spread_G16")["replicas"]
    assert rep[0] and not all(rep)                                  # level 0 through dense replicas, the fine levels direct
    assert rep == [True, True] + [False] * 14
    assert not any(sc.case_census("runs_G16")["replicas"])          # P too small for a replica to pay
    assert not any(sc.case_census("spread_G5")["replicas"])         # table smaller than level 0's 17^3 cells
    assert sc.case_census("hot_slot_G20")["replicas"] == [True, False]


@pytest.mark.parametrize("N,S", sc.RAY_SHAPES)
def test_ray_cases_reach_the_three_reductions_of_d_position(N, S):
    """a wave wholly inside one group of 4 rays (the shuffle reduction), waves that straddle two groups, a last group of fewer than 4 rays"""
    i = np.arange(-(-N * S // 64) * 64)
    ray, s = sc.patch_order(np.minimum(i, N * S - 1), N, S)
    assert sorted(set(zip(ray[: N * S].tolist(), s[: N * S].tolist()))) == [(r, k) for r in range(N) for k in range(S)]  # a permutation
    uniform = [bool((ray[w:w + 64] == np.tile(ray[w:w + 4], 16)).all()) for w in range(0, len(i), 64)]
    if (N, S) == (8, 16):
        assert all(uniform)
    elif (N, S) == (8, 24):
        assert uniform == [True, False, True]
    else:
        assert uniform == [True, False] and int(ray[64:112].max()) == 6 and len(set(ray[64:67].tolist())) == 3


@pytest.mark.parametrize("name", list(sc.RAY_CASES))
def test_ray_cases_sit_in_the_same_cells_in_float32_and_float64(name):
    c = sc.case(name)
    assert sc.cells_agree(c) and c.want_dpos and bool(((c.p32 > 0) & (c.p32 < 1)).all())
    print(name, "seed", c.marks["seed"])


def test_prefill_is_non_zero_in_about_half_of_the_slots_and_small_against_the_bound():
    for name in ("runs_G16", "hot_slot_G5"):
        c = sc.case(name)
        ref, A, count = sc.case_reference(name)
        pre = sc.prefill(c, A, count).double()
        frac = float((pre != 0).any(dim=1).double().mean())
        assert 0.45 < frac < 0.55
        assert bool((((A == 0) & (pre != 0)).any())) and bool(((A > 0) & (pre != 0)).any())
        assert bool((count.double()[:, None] * pre.abs() <= 2.0 * A * (1 + 1e-6))[A > 0].all())
