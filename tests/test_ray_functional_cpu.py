"""The float64 restatement of the per-ray kernels (ray_functional.py) against the fp32 oracle, on the inputs the GPU edge test uses.

(a) the oracle stays within ORACLE_DISTANCE of the restatement on every generic and every edge input;
(b) the lo / hi tables of the two small dyadic interlevel cases, written out by hand, are the restatement's and the oracle's;
(c) a wrong searchsorted side, or a ray that loses its last sample, leaves the tolerance the GPU test applies: those assertions can fail;
(d) the builders' rows contain what they claim to contain, and no ray is near a median tie or a clip tie.

`PYTHONPATH=oracle:tests python tests/test_ray_functional_cpu.py` prints the measured distances (the source of ORACLE_DISTANCE).
"""
import functools

import pytest
import torch

import ray_functional as rf
import thermal_nerfacto_oracle as orc


def _smp(s, e=None):
    return orc.Samples(s_bins=s, e_bins=s if e is None else e)


def _gen(tag: int):
    return torch.Generator().manual_seed(4242 + tag)


def oracle_interlevel(c, w, cp, wp):
    wp = wp.clone().requires_grad_(True)
    loss = orc.interlevel_loss([wp[..., None], w[..., None]], [_smp(cp), _smp(c)])
    loss.backward()
    return loss.detach(), wp.grad


def oracle_tables(c, cp):
    """lo / hi of the oracle's _outer, read off its result for one-hot proposal weights: w_outer_i = [lo_i <= k <= hi_i]."""
    Sp = cp.shape[-1] - 1
    cover = torch.stack([orc._outer(c[:, :-1], c[:, 1:], cp[:, :-1], cp[:, 1:], torch.eye(Sp)[k].expand(c.shape[0], Sp)) for k in range(Sp)], -1)
    assert ((cover == 0) | (cover == 1)).all() and (cover.sum(-1) >= 1).all()
    k = torch.arange(Sp)
    lo = torch.where(cover == 1, k, Sp).min(-1).values
    hi = torch.where(cover == 1, k, -1).max(-1).values
    assert torch.equal(cover.sum(-1).long(), hi - lo + 1)  # one run
    return lo, hi


@functools.lru_cache(maxsize=None)
def measure():
    """{quantity: (abs, rel)}: the largest distance of the fp32 oracle from the restatement over every input of the GPU edge test."""
    worst = {q: (0.0, 0.0) for q in rf.ORACLE_DISTANCE}

    def see(q, got, ref):
        d = rf.distance(q, got, ref)
        worst[q] = (max(worst[q][0], d[0]), max(worst[q][1], d[1]))

    for S in rf.SWEEP:
        b = rf.edge_batch(S)
        s, e = b["s_bins"], b["e_bins"]
        N = e.shape[0]
        smp = _smp(s, e)
        gw = torch.rand((N, S), generator=_gen(S)) * 2 - 1
        dens = b["density"].clone().requires_grad_(True)
        w32 = orc.get_weights(smp.deltas, dens[..., None])
        (w32[..., 0] * gw).sum().backward()
        w64, dd64 = rf.weights_grad(e, b["density"], gw)
        see("weights", w32[..., 0], w64)
        see("d_density", dens.grad, dd64)
        w = rf.edge_weights(S)
        for C in (1, 3, 4):
            for training in (True, False):
                rgb = rf.edge_rgb(S, C)
                if not training:
                    rgb = rgb.clone()
                    rgb[3, S // 2, 0] = float("nan")
                    rgb[4, 0, C - 1] = 3.0
                comp64, acc64 = rf.composite(rgb, w, training)
                see("composite", orc.composite_rgb(rgb, w[..., None], training), comp64)
                see("accumulation", orc.accumulation(w[..., None]), acc64)
            gc = torch.rand((N, C), generator=_gen(S + C)) - 0.5
            r32, w32_ = rf.edge_rgb(S, C).clone().requires_grad_(True), w.clone().requires_grad_(True)
            (orc.composite_rgb(r32, w32_[..., None], True) * gc).sum().backward()
            drgb64, dw64 = rf.composite_grad(rf.edge_rgb(S, C), w, gc)
            see("d_rgb", r32.grad, drgb64)
            see("d_weights", w32_.grad, dw64)
        see("expected_depth", orc.depth_expected(w[..., None], smp), rf.expected_depth(w, e)[1])
        w32_ = w.clone().requires_grad_(True)
        loss = 0.002 * orc.distortion_loss([w32_[..., None]], [smp])
        loss.backward()
        loss64, dw64 = rf.distortion(s, w, 0.002)
        see("distortion", loss.detach(), loss64)
        see("distortion_d_weights", w32_.grad, dw64)
    for unsorted_row in (False, True):
        for c, w, cp, wp in rf.interlevel_cases(unsorted_row):
            loss32, g32 = oracle_interlevel(c, w, cp, wp)
            loss64, g64, _, _ = rf.interlevel(c, w, cp, wp)
            see("interlevel", loss32, loss64)
            see("interlevel_d_weights", g32, g64)
    for Sp, S in rf.pdf_cases():
        p = rf.pdf_case(Sp, S)
        for anneal in rf.PDF_ANNEALS:
            for jit in p["jitters"].values():
                s32 = orc.pdf_resample(p["s_bins"], torch.pow(p["weights"], anneal)[..., None], S, jit)
                s64, e64 = rf.pdf_resample(p["s_bins"], p["weights"], S, anneal, p["nears"], p["fars"], jit)
                see("pdf_s", s32, s64)
                see("pdf_e", orc.s_to_euclidean(s32, p["nears"], p["fars"]), e64)
    return worst


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("quantity", sorted(rf.ORACLE_DISTANCE))
def test_oracle_stays_within_its_recorded_distance(quantity):
    a, r = measure()[quantity]
    rec = rf.ORACLE_DISTANCE[quantity]
    assert a <= rec["abs"] and r <= rec["rel"], (quantity, a, r, rec)
    # the record is a measurement, not a budget: the asserted entry is the measured one rounded up, not something far above it
    mode = rf.TOL_MODE[quantity]
    assert rec[mode] <= 4.0 * max((a, r)[mode == "rel"], 1e-12), (quantity, a, r, rec)


def test_oracle_median_is_the_midpoint_at_the_float64_index():
    for S in rf.SWEEP:
        b = rf.edge_batch(S)
        e = b["e_bins"]
        idx, _ = rf.median_index(rf.weights(e, b["density"]))
        w32 = orc.get_weights(_smp(b["s_bins"], e).deltas, b["density"][..., None])
        mid = (e[:, :-1] + e[:, 1:]) / 2
        assert torch.equal(orc.depth_median(w32, _smp(b["s_bins"], e)), torch.gather(mid, -1, idx[:, None])), S
        assert torch.equal(rf.median_depth(rf.weights(e, b["density"]), e)[0].float(), torch.gather(mid, -1, idx[:, None])), S


@pytest.mark.parametrize("unsorted_row", [False, True])
@pytest.mark.parametrize("pair", rf.INTERLEVEL_PAIRS)
def test_interlevel_gradient_written_out_is_autograds(pair, unsorted_row):
    """same values to float64 rounding; the written-out sum has an exact zero wherever no fine interval with a non-zero g covers the bin,
    autograd (back through the cumulative sum) a residue in some of those places."""
    case = rf.interlevel_case(*pair, unsorted_row)
    loss, grad, _, _ = rf.interlevel(*case)
    loss_a, grad_a = rf.interlevel_autograd(*case)
    assert float(loss) == float(loss_a)
    assert float((grad - grad_a).abs().max()) <= 1e-14 * float(grad_a.abs().max())
    assert bool((grad[grad_a == 0] == 0).all())
    assert float(grad_a[grad == 0].abs().max()) <= 1e-14 * float(grad_a.abs().max())


# ------------------------------------------------------------------------------------------------ (b)
HAND_TABLES = {
    # fine edges k/4 in proposal bins of width 1/8: the start search lands ON the coinciding start, the end search one bin PAST the
    # coinciding end (side="right" counts the tie)
    (4, 8): ([0, 2, 4, 6], [2, 4, 6, 7]),
    # fine edges k/8 in proposal bins of width 1/4
    (8, 4): ([0, 0, 1, 1, 2, 2, 3, 3], [0, 1, 1, 2, 2, 3, 3, 3]),
}


@pytest.mark.parametrize("pair", sorted(HAND_TABLES))
def test_hand_written_tables_of_the_small_dyadic_cases(pair):
    c, w, cp, wp = rf.interlevel_case(*pair)
    lo_hand, hi_hand = (torch.tensor(t) for t in HAND_TABLES[pair])
    _, _, lo, hi = rf.interlevel(c, w, cp, wp)
    o_lo, o_hi = oracle_tables(c, cp)
    for r in (0, 1, 2, 4, 5, 6):  # every ray on the plain linspace edges (ray 3 carries the duplicated edges)
        assert torch.equal(lo[r], lo_hand) and torch.equal(hi[r], hi_hand), (pair, r, lo[r], hi[r])
        assert torch.equal(o_lo[r], lo_hand) and torch.equal(o_hi[r], hi_hand), (pair, r, o_lo[r], o_hi[r])
    assert torch.equal(lo, o_lo) and torch.equal(hi, o_hi)  # the duplicated-edge ray too


@pytest.mark.parametrize("pair", rf.INTERLEVEL_PAIRS)
def test_tables_equal_the_oracles_in_every_case(pair):
    c, w, cp, wp = rf.interlevel_case(*pair)
    _, _, lo, hi = rf.interlevel(c, w, cp, wp)
    o_lo, o_hi = oracle_tables(c, cp)
    assert torch.equal(lo, o_lo) and torch.equal(hi, o_hi)


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("pair", rf.INTERLEVEL_DYADIC)
@pytest.mark.parametrize("which", ["side_lo", "side_hi"])
def test_a_wrong_side_moves_the_dyadic_losses_far_out_of_tolerance(pair, which):
    c, w, cp, wp = rf.interlevel_case(*pair)
    loss, grad, lo, hi = rf.interlevel(c, w, cp, wp)
    loss_l, grad_l, lo_l, hi_l = rf.interlevel(c, w, cp, wp, **{which: "left"})
    assert not (torch.equal(lo, lo_l) and torch.equal(hi, hi_l))
    assert abs(float(loss_l - loss)) > 100.0 * rf.tolerance("interlevel") * abs(float(loss)), (pair, which, float(loss), float(loss_l))
    assert rf.distance("interlevel_d_weights", grad_l, grad)[1] > 100.0 * rf.tolerance("interlevel_d_weights")


def test_random_bins_do_not_fix_the_side():
    """what the dyadic cases are for: on jittered bins the two sides give the same tables, a wrong side passes unnoticed."""
    for pair in ((65, 64), (63, 129)):
        c, w, cp, wp = rf.interlevel_case(*pair)
        rows = [r for r in range(c.shape[0]) if r != 3]  # (the duplicated edges tie among themselves)
        _, _, lo, hi = rf.interlevel(c[rows], w[rows], cp[rows], wp[rows])
        _, _, lo_l, hi_l = rf.interlevel(c[rows], w[rows], cp[rows], wp[rows], side_lo="left", side_hi="left")
        assert torch.equal(lo, lo_l) and torch.equal(hi, hi_l)


@pytest.mark.parametrize("S", [65, 129])
def test_a_dropped_last_sample_leaves_the_tolerance(S):
    """a ray treated as if it had S - 1 samples (the ragged tail of a lane layout lost)."""
    b = rf.edge_batch(S)
    s, e, dens = b["s_bins"], b["e_bins"], b["density"]
    N = e.shape[0]
    zero = torch.zeros((N, 1), dtype=rf.F64)
    w = rf.weights(e, dens)
    w_drop = torch.cat([rf.weights(e[:, :S], dens[:, :S - 1]), zero], -1)
    assert not rf.within("weights", w_drop, w)
    wf = rf.edge_weights(S)
    for C in (1, 3, 4):
        rgb = rf.edge_rgb(S, C)
        comp, acc = rf.composite(rgb, wf, True)
        comp_d, acc_d = rf.composite(rgb[:, :S - 1], wf[:, :S - 1], True)
        assert not rf.within("composite", comp_d, comp)
        assert not rf.within("accumulation", acc_d, acc)
    loss, dw = rf.distortion(s, wf, 0.002)
    loss_d, dw_d = rf.distortion(s[:, :S], wf[:, :S - 1], 0.002)
    assert not rf.within("distortion", loss_d, loss)
    assert not rf.within("distortion_d_weights", torch.cat([dw_d, zero], -1), dw)


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("S", rf.SWEEP)
def test_edge_batch_rows_are_what_they_claim(S):
    b = rf.edge_batch(S)
    s, e, dens, kinds = b["s_bins"], b["e_bins"], b["density"], b["kinds"]
    assert e.shape == (rf.EDGE_N, S + 1) and dens.shape == (rf.EDGE_N, S) and e.dtype == torch.float32 and dens.dtype == torch.float32
    assert set(kinds) == {k for k in rf.EDGE_KINDS if S >= rf.EDGE_MIN_S[k]}
    if S >= 4:
        assert set(kinds) == set(rf.EDGE_KINDS)
    w64 = rf.weights(e, dens)
    w32 = orc.get_weights(_smp(s, e).deltas, dens[..., None])[..., 0]
    _, margin = rf.median_index(w64)
    assert float(margin.min()) > rf.MEDIAN_MARGIN
    assert float(rf.median_index(w32)[1].min()) > rf.MEDIAN_MARGIN / 2  # and the fp32 weights are nowhere near one either
    assert bool((e[:, 1:] >= e[:, :-1]).all()) and bool((s[:, 1:] >= s[:, :-1]).all())
    delta = e[:, 1:] - e[:, :-1]
    h = S // 2
    for k, r in kinds.items():
        if k == "empty":
            assert bool((dens[r] == 0).all()) and bool((w64[r] == 0).all()) and bool((delta[r] > 0).all())
        elif k == "opaque_first":
            assert float(dens[r, 0]) == 1e6 and float(w32[r, 0]) == 1.0 and float(w64[r, 1:].sum()) < 1e-300
        elif k == "opaque_last":
            assert bool((w32[r, :-1] == 0).all()) and float(w32[r, -1]) == 1.0
        elif k == "underflow":
            dd = delta[r] * dens[r]
            trans = torch.exp(-torch.cumsum(dd[:-1], 0))  # fp32
            assert float(torch.cumsum(dd, 0)[h - 1]) > 104.0 and float(dd[0]) < 104.0
            assert bool((trans[h - 1:] == 0).all()) and float(trans[0]) > 0
            assert bool((w32[r, h:] == 0).all()) and float(w64[r, h]) > 0.0  # float64 still resolves the sample where fp32 gives up
        elif k == "zero_second_half":
            assert bool((dens[r, h:] == 0).all()) and bool((w64[r, h:] == 0).all()) and bool((dens[r, :h] > 0).all())
        elif k == "near_eq_far":
            assert bool((e[r] == e[r, 0]).all()) and bool((delta[r] == 0).all()) and bool((w64[r] == 0).all())
            assert float(e[r, 0]) < float(e[torch.arange(e.shape[0]) != r].min())  # it sets the lower end of the depth clip
        elif k == "duplicate_edge":
            assert float(delta[r, h]) == 0.0 and float(s[r, h + 1] - s[r, h]) == 0.0 and float(dens[r, h]) > 0.0
            assert int((delta[r] == 0).sum()) == 1 and float(w64[r, h]) == 0.0
        elif k == "tiny_density":
            assert bool((w32[r] == 0).all()) and bool((w64[r] > 0).all())  # 1 - expf(-x) cancels, 1 - exp(-x) does not
    # the expected depth of the empty ray is the near == far ray's depth: the clip is batch-wide
    clipped = rf.expected_depth(rf.edge_weights(S), e)[1]
    assert float(clipped[kinds["empty"], 0]) == pytest.approx(rf.NEAR_EQ_FAR_DEPTH, rel=1e-6)


def test_edge_batch_is_deterministic_and_sized_by_its_arguments():
    a, b = rf.edge_batch(65), rf.edge_batch.__wrapped__(65)
    assert all(torch.equal(a[k], b[k]) for k in ("s_bins", "e_bins", "density"))
    c = rf.edge_batch(65, 36)
    assert c["density"].shape == (36, 65) and float(rf.median_index(rf.weights(c["e_bins"], c["density"]))[1].min()) > rf.MEDIAN_MARGIN


@pytest.mark.parametrize("pair", rf.INTERLEVEL_PAIRS)
@pytest.mark.parametrize("unsorted_row", [False, True])
def test_interlevel_cases_are_what_they_claim(pair, unsorted_row):
    Sf, Sp = pair
    c, w, cp, wp = rf.interlevel_case(Sf, Sp, unsorted_row)
    N = len(rf.INTERLEVEL_ROWS)
    assert c.shape == (N, Sf + 1) and w.shape == (N, Sf) and cp.shape == (N, Sp + 1) and wp.shape == (N, Sp)
    d = rf.interlevel_excess(c, w, cp, wp)
    assert float(d.abs().min()) > rf.CLIP_MARGIN  # the clip takes the same branch in float32 and in float64
    _, grad, lo, hi = rf.interlevel(c, w, cp, wp)
    assert bool((w[0] == 0).all()) and bool((grad[0] == 0).all())
    assert bool((d[1] < 0).all()) and bool((grad[1] == 0).all())
    assert float((d[2] > 0).double().mean()) >= 0.5 and bool((grad[2] < 0).any())
    assert bool((cp[:, 1:] >= cp[:, :-1]).all())
    sorted_rows = slice(0, N - 1) if unsorted_row else slice(0, N)
    assert bool((c[sorted_rows, 1:] >= c[sorted_rows, :-1]).all())
    if unsorted_row and Sf >= 2:
        assert bool((c[N - 1, 1:] < c[N - 1, :-1]).any())
    if Sf >= 2 and Sp >= 2:
        assert float(c[3, Sf // 2 + 1]) == float(c[3, Sf // 2]) and float(cp[3, Sp // 2 + 1]) == float(cp[3, Sp // 2])
    if pair in rf.INTERLEVEL_DYADIC:  # interior ties on both searches
        ties_lo = (c[4, 1:-1, None] == cp[4, None, 1:-1]).any(-1)
        assert int(ties_lo.sum()) >= min(Sf, Sp) - 1


@pytest.mark.parametrize("pair", rf.PDF_PAIRS)
def test_pdf_cases_are_what_they_claim(pair):
    Sp, S = pair
    p = rf.pdf_case(Sp, S)
    N = len(rf.PDF_ROWS)
    w, s = p["weights"], p["s_bins"]
    assert w.shape == (N, Sp) and s.shape == (N, Sp + 1) and p["e_bins"].shape == (N, Sp + 1)
    assert bool((w[0] == 0).all())
    assert float(w[1].sum()) == 1.0 and int((w[1] != 0).sum()) == 1
    assert bool((w[2] == 1).all())
    if Sp >= 2:
        assert float(s[3, Sp // 2 + 1]) == float(s[3, Sp // 2])
    assert bool((s[:, 1:] >= s[:, :-1]).all())
    assert p["jitters"]["none"] is None and float(p["jitters"]["zero"].abs().max()) == 0.0
    jm = p["jitters"]["max"]
    assert jm.dtype == torch.float32 and float(jm.max()) < 1.0 and float(torch.nextafter(jm.max(), torch.tensor(2.0))) == 1.0
    for anneal in rf.PDF_ANNEALS:
        for jit in p["jitters"].values():
            sn, en = rf.pdf_resample(s, w, S, anneal, p["nears"], p["fars"], jit)
            assert sn.shape == (N, S + 1) and bool((sn[:, 1:] >= sn[:, :-1]).all()) and float(sn.min()) >= 0.0 and float(sn.max()) <= 1.0
            assert bool((en[:, 1:] >= en[:, :-1]).all())


if __name__ == "__main__":
    for q, (a, r) in sorted(measure().items()):
        print(f"{q:24s} abs {a:.3e}  rel {r:.3e}")
