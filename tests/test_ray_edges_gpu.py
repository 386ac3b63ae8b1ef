"""The per-ray kernels (one wave per ray: weights, depths, PDF resampling, renderers, distortion and interlevel loss, and their fused launches)
against the float64 restatement of ray_functional.py, at the sample counts next to 64 / 128 / 256 where the two lane layouts have ragged
tails, and on degenerate rays (empty, opaque at one end, underflowing transmittance, zero-width interval, near == far, cancelling alphas).

Every ray is checked, no outlier share: the bound of a quantity is ray_functional.tolerance() = 4 x the fp32 oracle's own distance from the
restatement, never looser than test_hip_ops_gpu.py's.  A dropped, doubled or misplaced sample is ~1e-3 and a wrong searchsorted side moves the
dyadic interlevel cases by far more (test_ray_functional_cpu.py shows both without a GPU).  Each comparison prints its figure
(`FIGURE quantity distance bound where`) before the test asserts.
"""
import pytest
import torch

import ray_functional as rf
from nerfstudio_thermal_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

FUSED_FINE = (1, 63, 64, 65, 128, 129, 256)
FUSED_PROPS = ((256, 96), (65, 64), (1, 1))


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_error():
    """a kernel error ends the session: nothing more is started on a device that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"GPU error: {err}", returncode=3)


def g(x):
    return x.to(DEV).contiguous()


def eq(a, b):
    """bit for bit (NaNs in the same places count as equal)."""
    return a.shape == b.shape and torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0))


class Figures:
    """prints every figure, fails at the end: one run shows all of a test's distances."""

    def __init__(self):
        self.bad = []

    def __call__(self, quantity, got, ref, where=""):
        d = rf.asserted_distance(quantity, got, ref)
        tol = rf.tolerance(quantity)
        print(f"FIGURE {quantity} {d:.3e} {tol:.3e} {where}")
        if not d <= tol:
            self.bad.append((quantity, where, d, tol))

    def that(self, cond, what):
        if not cond:
            self.bad.append(what)

    def done(self):
        assert not self.bad, self.bad


def _gen(tag):
    return torch.Generator().manual_seed(99 + tag)


def _mid32(e):
    return (e[:, :-1] + e[:, 1:]) / 2


def _assert_median(fig, med, w_for_index, e, where):
    """the median depth is, bit for bit, the float32 midpoint at the float64 index -- on rays that are provably not at a tie."""
    idx, margin = rf.median_index(w_for_index)
    assert float(margin.min()) > rf.MEDIAN_MARGIN
    fig.that(torch.equal(med.cpu(), torch.gather(_mid32(e), -1, idx[:, None])), ("median", where))


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("S", rf.SWEEP)
def test_weights_fwd_bwd(S):
    fig = Figures()
    b = rf.edge_batch(S)
    e, dens = b["e_bins"], b["density"]
    gw = torch.rand(dens.shape, generator=_gen(S)) * 2 - 1
    w64, dd64 = rf.weights_grad(e, dens, gw)
    w, med = ops.weights_fwd(g(e), g(dens), want_median=True)
    fig("weights", w, w64, f"S={S}")
    _assert_median(fig, med, w64, e, f"S={S}")
    w2, none = ops.weights_fwd(g(e), g(dens))
    fig.that(none is None and eq(w, w2), "weights without the median")
    dd = ops.weights_bwd(g(e), g(dens), w, g(gw))
    fig("d_density", dd, dd64, f"S={S}")
    for k in ("near_eq_far",):  # delta = 0: an exact zero gradient
        fig.that(bool((dd[b["kinds"][k]] == 0).all()), k)
    fig.done()


# ------------------------------------------------------------------------------------------------ renderers
def _eval_rgb(rgb, S, C):
    rgb = rgb.clone()
    rgb[3, S // 2, 0] = float("nan")
    rgb[4, 0, C - 1] = 3.0  # out of range: row 4 keeps its first half, the composite leaves [0,1] before the clamp
    return rgb


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("S", rf.SWEEP)
def test_composite_fwd_bwd(S, C):
    fig = Figures()
    b = rf.edge_batch(S)
    e, w = b["e_bins"], rf.edge_weights(S)
    N = e.shape[0]
    for training in (True, False):
        rgb = rf.edge_rgb(S, C) if training else _eval_rgb(rf.edge_rgb(S, C), S, C)
        where = f"S={S} C={C} training={training}"
        comp, acc, med, exp = ops.composite_fwd(g(rgb), g(w), g(e), training)
        comp64, acc64 = rf.composite(rgb, w, training)
        fig("composite", comp, comp64, where)
        fig("accumulation", acc, acc64, where)
        fig("expected_depth", exp, rf.expected_depth(w, e)[1], where)
        _assert_median(fig, med, w, e, where)
        comp2, acc2, m2, x2 = ops.composite_fwd(g(rgb), g(w), g(e), training, want_depth=False)
        fig.that(m2 is None and x2 is None and eq(comp, comp2) and eq(acc, acc2), ("no depths", where))
    rgb = rf.edge_rgb(S, C)
    gc = torch.rand((N, C), generator=_gen(S + C)) - 0.5
    incoming = 0.05 * (torch.rand((N, S), generator=_gen(S + C + 1)) - 0.5)
    drgb64, dw64 = rf.composite_grad(rgb, w, gc)
    dw = g(incoming)
    drgb = ops.composite_bwd(g(rgb), g(w), g(gc), dw)
    fig("d_rgb", drgb, drgb64, f"S={S} C={C}")
    fig("d_weights", dw, incoming.double() + dw64, f"S={S} C={C}")
    fig.done()


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("S", rf.SWEEP)
def test_render_fwd_bwd(S, C):
    """tn_render_fwd / tn_render_bwd: the restatement's values, and the bits of the separate launches.  The composite half is compared at the
    weights the launch itself returned (the expected depth of a ray with sum w ~ 1e-10 amplifies any weight error without bound)."""
    fig = Figures()
    b = rf.edge_batch(S)
    e, dens, kinds = b["e_bins"], b["density"], b["kinds"]
    N = e.shape[0]
    he, hd = g(e), g(dens)
    for training in (True, False):
        rgb = rf.edge_rgb(S, C) if training else _eval_rgb(rf.edge_rgb(S, C), S, C)
        where = f"S={S} C={C} training={training}"
        hr = g(rgb)
        w_ref, _ = ops.weights_fwd(he, hd)
        c_ref, a_ref, m_ref, x_ref = ops.composite_fwd(hr, w_ref, he, training)
        for rep in range(2):  # the second call finds the scratch as the first one left it
            w, c, a, m, x = ops.render_fwd(he, hd, hr, training)
            for name, got, ref in (("w", w, w_ref), ("comp", c, c_ref), ("acc", a, a_ref), ("median", m, m_ref), ("expected", x, x_ref)):
                fig.that(eq(got, ref), ("render_fwd != separate launches", name, where, rep))
        w64 = rf.weights(e, dens)
        fig("weights", w, w64, where)
        comp64, acc64 = rf.composite(rgb, w.cpu(), training)
        fig("composite", c, comp64, where)
        fig("accumulation", a, acc64, where)
        fig("expected_depth", x, rf.expected_depth(w.cpu(), e)[1], where)
        _assert_median(fig, m, w64, e, where)
        # the clip is batch-wide: the empty ray's depth is the smallest midpoint of the batch, which only the near == far ray has
        lo = torch.tensor(rf.NEAR_EQ_FAR_DEPTH, dtype=torch.float32)
        fig.that(float(_mid32(e).min()) == float(lo) and float(x[kinds["empty"]]) == float(lo) and float(x[kinds["near_eq_far"]]) == float(lo),
                 ("batch-wide clip", where, float(x[kinds["empty"]])))
    rgb = rf.edge_rgb(S, C)
    hr = g(rgb)
    gc = torch.rand((N, C), generator=_gen(S + C)) - 0.5
    dw_loss = 0.05 * (torch.rand((N, S), generator=_gen(S + C + 1)) - 0.5)
    h_dw = g(dw_loss)
    dw = h_dw.clone()
    drgb_ref = ops.composite_bwd(hr, w_ref, g(gc), dw)
    dd_ref = ops.weights_bwd(he, hd, w_ref, dw)
    drgb, dd = ops.render_bwd(he, hd, hr, w_ref, g(gc), h_dw)
    fig.that(eq(drgb, drgb_ref) and eq(dd, dd_ref), ("render_bwd != separate launches", S, C))
    fig.that(torch.equal(h_dw.cpu(), dw_loss), "d_weights_in is read only")
    sigma, rgb64 = dens.double().requires_grad_(True), rgb.double().requires_grad_(True)
    w64 = rf._weights(e.double(), sigma)
    comp64, _ = rf._composite(rgb64, w64, True)
    ((comp64 * gc.double()).sum() + (w64 * dw_loss.double()).sum()).backward()
    fig("d_rgb", drgb, rgb64.grad, f"S={S} C={C}")
    fig("d_density", dd, sigma.grad, f"S={S} C={C}")
    fig.done()


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("S", rf.SWEEP)
def test_distortion_loss(S):
    fig = Figures()
    b = rf.edge_batch(S)
    s, w = b["s_bins"], rf.edge_weights(S)
    loss64, dw64 = rf.distortion(s, w, 0.002)
    incoming = 0.1 * float(dw64.abs().max()) * (torch.rand(w.shape, generator=_gen(S)) - 0.5)  # result = incoming + gradient
    loss, dw = torch.zeros(1, device=DEV), g(incoming)
    ops.distortion_loss(g(s), g(w), 0.002, loss, dw)
    fig("distortion", loss[0], loss64, f"S={S}")
    fig("distortion_d_weights", dw, incoming.double() + dw64, f"S={S}")
    loss2 = torch.zeros(1, device=DEV)
    ops.distortion_loss(g(s), g(w), 0.002, loss2, None)  # the gradient is optional
    fig("distortion", loss2[0], loss64, f"S={S} no gradient")
    fig.done()


@pytest.mark.parametrize("unsorted_row", [False, True])
@pytest.mark.parametrize("pair", rf.INTERLEVEL_PAIRS)
def test_interlevel_loss(pair, unsorted_row):
    fig = Figures()
    c, w, cp, wp = rf.interlevel_case(*pair, unsorted_row)
    loss64, g64, _, _ = rf.interlevel(c, w, cp, wp)
    incoming = 0.1 * float(g64.abs().max()) * (torch.rand(wp.shape, generator=_gen(pair[0] + pair[1])) + 0.5)  # non-zero everywhere
    loss, dw = torch.zeros(1, device=DEV), g(incoming)
    ops.interlevel_loss(g(c), g(w), g(cp), g(wp), 1.0, loss, dw)
    where = f"Sf={pair[0]} Sp={pair[1]} unsorted_row={unsorted_row}"
    fig("interlevel", loss[0], loss64, where)
    fig("interlevel_d_weights", dw, incoming.double() + g64, where)
    zero = g64 == 0
    assert bool(zero[0].all()) and bool(zero[1].all())  # zero fine weights; proposal weights that dominate
    fig.that(torch.equal(dw.cpu()[zero], incoming[zero]), ("an exact zero gradient changed the incoming bits", where))
    fig.that(bool((dw.cpu()[~zero] != incoming[~zero]).all()), ("a non-zero gradient left the incoming bits", where))
    fig.done()


# ------------------------------------------------------------------------------------------------ PDF resampling
@pytest.mark.parametrize("pair", rf.PDF_PAIRS)
def test_pdf_resample_and_weights_resample(pair):
    fig = Figures()
    Sp, S = pair
    p = rf.pdf_case(Sp, S)
    s_prev, e_prev, w_prev, dens, nears, fars = (p[k] for k in ("s_bins", "e_bins", "weights", "density", "nears", "fars"))
    hs, he, hw, hd, hn, hf = (g(t) for t in (s_prev, e_prev, w_prev, dens, nears, fars))
    w_a, med_a = ops.weights_fwd(he, hd, want_median=True)
    fig("weights", w_a, rf.weights(e_prev, dens), f"Sp={Sp}")
    for anneal in rf.PDF_ANNEALS:
        for name, jit in p["jitters"].items():
            where = f"Sp={Sp} S={S} anneal={anneal} jitter={name}"
            hj = None if jit is None else g(jit)
            s, e = ops.pdf_resample(hs, hw, S, anneal, hn, hf, hj)
            s64, e64 = rf.pdf_resample(s_prev, w_prev, S, anneal, nears, fars, jit)
            fig("pdf_s", s, s64, where)
            fig("pdf_e", e, e64, where)
            for t, what in ((s, "s"), (e, "e")):
                fig.that(bool((t[:, 1:] >= t[:, :-1]).all()), (what + " bins decrease", where))
            fig.that(float(s.min()) >= 0.0 and float(s.max()) <= 1.0, ("s bins leave [0,1]", where))
            # the fused launch: the two calls' bits, weights and median included
            s_a, e_a = ops.pdf_resample(hs, w_a, S, anneal, hn, hf, hj)
            w_b, med_b, s_b, e_b = ops.weights_resample(he, hd, hs, S, anneal, hn, hf, hj)
            fig.that(eq(w_a, w_b) and eq(med_a, med_b) and eq(s_a, s_b) and eq(e_a, e_b), ("weights_resample != the two calls", where))
            s64, e64 = rf.pdf_resample(s_prev, w_a.cpu(), S, anneal, nears, fars, jit)
            fig("pdf_s", s_b, s64, where + " fused")
            fig("pdf_e", e_b, e64, where + " fused")
    w_c, none, s_c, _ = ops.weights_resample(he, hd, hs, S, 1.0, hn, hf, None, want_median=False)
    fig.that(none is None and eq(w_c, w_a), "median optional")
    fig.done()


# ------------------------------------------------------------------------------------------------ fused loss launches
def _levels(S, props, N):
    """fine level S and the proposal levels `props` of N rays each: (s bins, e bins, density, weights) on the device, edge rows included."""
    out = []
    for seed, Sl in enumerate((*props, S)):
        b = rf.edge_batch(Sl, N, seed + 1)
        out.append((g(b["s_bins"]), g(b["e_bins"]), g(b["density"]), g(rf.edge_weights(Sl, N, seed + 1))))
    return out[:-1], out[-1]


def _pixels(N, tag):
    gen = _gen(tag)
    img = torch.rand((N, 3), generator=gen)
    is_th = (torch.rand((N // 4, 1), generator=gen) < 0.4).float().repeat(1, 4).reshape(N)  # 2x2 patches are of one camera
    return g(img), g(is_th)


def _sums_agree(a, b):
    """the order of the additions is free: 2e-6 relative, term by term."""
    return bool(((a - b).abs() <= 2e-6 * a.abs()).all())


@pytest.mark.parametrize("props", FUSED_PROPS)
@pytest.mark.parametrize("S", FUSED_FINE)
def test_proposal_losses_is_the_separate_launches(S, props):
    N = rf.EDGE_N
    prop_lv, (s_f, _, _, w_f) = _levels(S, props, N)
    gen = _gen(S + props[0])
    acc0 = [g(torch.rand((N, Sl), generator=gen) * 1e-3) for Sl in (*props, S)]

    def run(fused):
        L = torch.zeros(2, device=DEV)
        d = [a.clone() for a in acc0]
        if fused:
            ops.proposal_losses(s_f, w_f, [(lv[0], lv[3], d[i]) for i, lv in enumerate(prop_lv)], 0.002, 1.0, L[0:1], L[1:2], d[2])
        else:
            ops.distortion_loss(s_f, w_f, 0.002, L[0:1], d[2])
            for i, lv in enumerate(prop_lv):
                ops.interlevel_loss(s_f, w_f, lv[0], lv[3], 1.0, L[1:2], d[i])
        return L, d

    La, da = run(False)
    Lb, db = run(True)
    for i, (a, b) in enumerate(zip(da, db)):
        assert torch.equal(a, b), (S, props, i, float((a - b).abs().max()))
    assert _sums_agree(La, Lb), (La, Lb)
    assert float(La[0]) > 0 and float(La[1]) > 0 and float((da[2] - acc0[2]).abs().max()) > 0 and float((da[0] - acc0[0]).abs().max()) > 0


@pytest.mark.parametrize("props", FUSED_PROPS)
@pytest.mark.parametrize("S", FUSED_FINE)
def test_train_losses_is_the_separate_launches(S, props):
    for N in (rf.EDGE_N, rf.EDGE_N - 1):  # 37 rays without the pixel terms; 36 with them (2x2 patches)
        prop_lv, (s_f, _, _, w_f) = _levels(S, props, N)
        gen = _gen(S + props[0] + N)
        acc0 = [g(torch.rand((N, Sl), generator=gen) * 1e-3) for Sl in (*props, S)]
        pred = g(torch.rand((N, 4), generator=gen))
        with_pixels = N % 4 == 0
        img, is_th = _pixels(N, S + props[0]) if with_pixels else (None, None)

        def run(fused):
            L = torch.zeros(16, device=DEV)
            Lp = torch.zeros((ops.LOSS_LINES, 16), device=DEV)
            d, dp = [a.clone() for a in acc0], torch.zeros_like(pred)
            pl = [(lv[0], lv[3], d[i]) for i, lv in enumerate(prop_lv)]
            pixel = (pred[:, :3], pred[:, 3:], img, is_th, 100.0, 1e-3, 1e-3, dp[:, :3], dp[:, 3:]) if with_pixels else None
            if fused:
                ops.train_losses(s_f, w_f, pl, 0.002, 1.0, d[2], Lp, pixel=pixel)
                ops.losses_finish(Lp, L)
            else:
                if with_pixels:
                    ops.pixel_losses(pred[:, :3], pred[:, 3:], img, is_th, 100.0, 1e-3, 1e-3, L[0:8], dp[:, :3], dp[:, 3:])
                ops.proposal_losses(s_f, w_f, pl, 0.002, 1.0, L[9:10], L[8:9], d[2])
            return L, d + [dp]

        La, da = run(False)
        Lb, db = run(True)
        for i, (a, b) in enumerate(zip(da, db)):
            assert torch.equal(a, b), (S, props, N, i, float((a - b).abs().max()))
        assert _sums_agree(La, Lb), (N, La, Lb)
        assert float(La[8]) > 0 and float(La[9]) > 0
        if with_pixels:
            assert float(Lb[4]) + float(Lb[5]) == N and float(La[0]) > 0 and float(da[3].abs().max()) > 0


@pytest.mark.parametrize("props", FUSED_PROPS)
@pytest.mark.parametrize("S", FUSED_FINE)
def test_render_losses_bwd_is_the_three_launches(S, props):
    """every rendered output and every gradient bit for bit, the batch-wide depth clip included; the loss sums up to their order."""
    N = rf.EDGE_N - 1
    prop_lv, (s_f, e_f, dens, _) = _levels(S, props, N)
    gen = _gen(S + props[0])
    rgb = g(torch.rand((N, S, 4), generator=gen))
    img, is_th = _pixels(N, S + props[0])
    acc0 = [g(torch.rand(shape, generator=gen) * 1e-3) for shape in ((N, props[0]), (N, props[1]), (N, S), (N, 4))]

    def run(fused):
        L = torch.zeros(16, device=DEV)
        Lp = torch.zeros((ops.LOSS_LINES, 16), device=DEV)
        d0, d1, d2, dc = (a.clone() for a in acc0)
        pl = [(prop_lv[0][0], prop_lv[0][3], d0), (prop_lv[1][0], prop_lv[1][3], d1)]
        if fused:
            w, c, a, m, x, d_rgb, dd = ops.render_losses_bwd(e_f, dens, rgb, s_f, pl, 0.002, 1.0, d2, img, is_th, 100.0, 1e-3, 1e-3, dc, Lp)
        else:
            w, c, a, m, x = ops.render_fwd(e_f, dens, rgb, True)
            ops.train_losses(s_f, w, pl, 0.002, 1.0, d2, Lp, pixel=(c[:, :3], c[:, 3:], img, is_th, 100.0, 1e-3, 1e-3, dc[:, :3], dc[:, 3:]))
            d_rgb, dd = ops.render_bwd(e_f, dens, rgb, w, dc, d2)
        ops.losses_finish(Lp, L)
        torch.cuda.synchronize()
        return L, dict(w=w, comp=c, acc=a, median=m, expected=x, d0=d0, d1=d1, d2=d2, d_comp=dc, d_rgb=d_rgb, d_density=dd)

    La, A = run(False)
    Lb, B = run(True)
    for k in A:
        assert torch.equal(A[k], B[k]), (S, props, k, float((A[k] - B[k]).abs().max()))
    assert _sums_agree(La, Lb), (La, Lb)
    assert float(A["d_density"].abs().max()) > 0 and float((A["d2"] - acc0[2]).abs().max()) > 0 and float((A["d0"] - acc0[0]).abs().max()) > 0
    assert float(Lb[4]) + float(Lb[5]) == N and all(float(Lb[k]) > 0 for k in (0, 8, 9))
    fig = Figures()  # and the fused launch's weights are the restatement's
    b = rf.edge_batch(S, N, 3)
    fig("weights", A["w"], rf.weights(b["e_bins"], b["density"]), f"S={S}")
    fig.done()
