"""A float64 restatement of the per-ray sampler, renderer and loss kernels (csrc/tn_sampler.hip, csrc/tn_sampler_ray.h), the reference the
edge tests hold them to, plus the builders of the inputs those tests share.

Written from oracle/thermal_nerfacto_oracle.py and the formulas in the kernel comments.  Every function takes the float32 tensors the kernels
take, upcasts them once and works in float64 from there on (no float32 constructor inside); gradients come from plain float64 autograd.
Shapes are the kernels': bins [N,S+1], weights / density [N,S], colours [N,S,C], per-ray scalars [N,1].

    weights / weights_grad            RaySamples.get_weights (with nan_to_num)
    median_index / median_depth       first sample whose cumulative weight reaches 0.5, and how far every ray is from a tie
    expected_depth                    unclipped and with the batch-wide clip
    composite / composite_grad        last-sample background; training and eval form
    pdf_resample                      PDFSampler as tn_pdf_resample runs it (anneal, padding, single jitter, right-side search)
    distortion / interlevel           loss values, d weights / d proposal weights, the interlevel lo / hi tables

ORACLE_DISTANCE records how far the fp32 oracle is from this restatement on the inputs below (test_ray_functional_cpu.py keeps it true);
tolerance() turns it into the bound the GPU test applies to the kernels.
"""
import functools

import torch

import thermal_nerfacto_oracle as orc

F64 = torch.float64

SWEEP = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)
EDGE_N = 37             # not a multiple of the 4 rays per block
NEAR, FAR = 0.05, 1000.0
MEDIAN_MARGIN = 1e-4    # no ray of edge_batch() has a cumulative weight this close to 0.5
CLIP_MARGIN = 1e-6      # no fine interval of interlevel_cases() has |w - w_outer| below this: the clip's branch is the same in every precision
HIST_PAD = 0.01
PDF_EPS = 1e-5
LOSS_EPS = 1e-7

# Largest distance between the fp32 oracle and the float64 restatement over SWEEP, interlevel_cases() and pdf_cases(), measured on the CPU
# (rounded up to two digits; the largest of torch's default / avx2 / avx512 code paths).  "abs": max |a - b|; "rel": the same divided by
# the quantity's largest magnitude (pdf_e: element-wise |a / b - 1|).  TOL_MODE names the entry the tests assert.
ORACLE_DISTANCE = {
    "weights": {"abs": 6.5e-08, "rel": 6.5e-08},
    "d_density": {"abs": 1.5e-05, "rel": 7.0e-08},
    "composite": {"abs": 2.5e-07, "rel": 2.6e-07},
    "accumulation": {"abs": 1.8e-07, "rel": 1.8e-07},
    "expected_depth": {"abs": 1.3e-05, "rel": 8.3e-08},
    "d_rgb": {"abs": 8.7e-08, "rel": 1.9e-07},
    "d_weights": {"abs": 1.7e-07, "rel": 1.9e-07},
    "pdf_s": {"abs": 5.8e-07, "rel": 5.9e-07},
    "pdf_e": {"abs": 8.5e-02, "rel": 9.6e-05},
    "distortion": {"abs": 8.6e-12, "rel": 1.3e-07},
    "distortion_d_weights": {"abs": 2.6e-11, "rel": 2.4e-07},
    "interlevel": {"abs": 5.3e-07, "rel": 3.1e-07},
    "interlevel_d_weights": {"abs": 1.2e-06, "rel": 8.1e-06},
}
TOL_MODE = {
    "weights": "abs", "composite": "abs", "accumulation": "abs", "d_rgb": "abs", "d_weights": "abs", "pdf_s": "abs",
    "d_density": "rel", "expected_depth": "rel", "pdf_e": "rel", "distortion": "rel", "distortion_d_weights": "rel", "interlevel": "rel",
    "interlevel_d_weights": "rel",
}
# what test_hip_ops_gpu.py asserts for the same quantity: the GPU bound is never looser.  (It has no bound on the worst PDF bin, only outlier
# shares: pdf_s / pdf_e stand on 4 x the oracle's distance alone.  For pdf_e that is ~3 ulps of the s-space value in front of
# e = 1 / (2 - 2 v): at e = 1000 one ulp of v, 6e-8, is already 1.2e-4 of e.)
TOL_CAP = {
    "weights": 2e-6, "composite": 2e-6, "accumulation": 2e-6, "d_rgb": 1e-6, "d_weights": 1e-5, "pdf_s": float("inf"),
    "d_density": 1e-5, "expected_depth": 1e-5, "pdf_e": float("inf"), "distortion": 1e-5, "distortion_d_weights": 1e-5, "interlevel": 1e-4,
    "interlevel_d_weights": 1e-4,
}
TOL_FACTOR = 4.0  # kernel and oracle are two fp32 evaluations of one formula (other reduction order, other expf): errors of the same order


def tolerance(quantity: str) -> float:
    """The bound of the GPU test: 4 x the oracle's own distance, never looser than the existing per-op tests."""
    return min(TOL_FACTOR * ORACLE_DISTANCE[quantity][TOL_MODE[quantity]], TOL_CAP[quantity])


def distance(quantity: str, got, ref):
    """(abs, rel) distance of `got` from the float64 `ref`, as ORACLE_DISTANCE defines them."""
    got, ref = torch.as_tensor(got).detach().cpu().to(F64), torch.as_tensor(ref).detach().cpu().to(F64)
    assert got.shape == ref.shape, (quantity, got.shape, ref.shape)
    a = float((got - ref).abs().max())
    if quantity == "pdf_e":
        return a, float((got / ref - 1.0).abs().max())
    m = float(ref.abs().max())
    return a, (a / m if m > 0.0 else (0.0 if a == 0.0 else float("inf")))


def asserted_distance(quantity: str, got, ref) -> float:
    """the entry of distance() that TOL_MODE names."""
    return distance(quantity, got, ref)[0 if TOL_MODE[quantity] == "abs" else 1]


def within(quantity: str, got, ref) -> bool:
    return asserted_distance(quantity, got, ref) <= tolerance(quantity)


def _d(x):
    return x.detach().to(F64)


# ------------------------------------------------------------------------------------------------ weights and depths
def _weights(e, sigma):
    dd = (e[:, 1:] - e[:, :-1]) * sigma
    alpha = 1.0 - torch.exp(-dd)
    trans = torch.cat([torch.zeros_like(dd[:, :1]), torch.cumsum(dd[:, :-1], dim=-1)], dim=-1)
    return torch.nan_to_num(alpha * torch.exp(-trans))


def weights(e_bins, density):
    """w_i = (1 - exp(-delta_i sigma_i)) exp(-sum_{k<i} delta_k sigma_k), nan_to_num'd.  [N,S] float64."""
    return _weights(_d(e_bins), _d(density))


def weights_grad(e_bins, density, d_weights):
    """-> weights, d density of sum(weights * d_weights)."""
    sigma = _d(density).requires_grad_(True)
    w = _weights(_d(e_bins), sigma)
    (w * _d(d_weights)).sum().backward()
    return w.detach(), sigma.grad


def median_index(w):
    """-> index [N] of the first sample whose cumulative weight is >= 0.5 (clamped to S-1), margin [N] = the ray's smallest |cum - 0.5|."""
    cum = torch.cumsum(_d(w), dim=-1)
    idx = (cum < 0.5).sum(dim=-1).clamp(max=w.shape[-1] - 1)
    return idx, (cum - 0.5).abs().min(dim=-1).values


def median_depth(w, e_bins):
    """-> depth [N,1] (the midpoint at median_index), index [N], margin [N]."""
    e = _d(e_bins)
    idx, margin = median_index(w)
    mid = (e[:, :-1] + e[:, 1:]) / 2.0
    return torch.gather(mid, -1, idx[:, None]), idx, margin


def expected_depth(w, e_bins):
    """-> (sum w mid / (sum w + 1e-10)) [N,1], and the same clipped to the batch's smallest / largest midpoint."""
    w, e = _d(w), _d(e_bins)
    mid = (e[:, :-1] + e[:, 1:]) / 2.0
    depth = (w * mid).sum(-1, keepdim=True) / (w.sum(-1, keepdim=True) + 1e-10)
    return depth, torch.clip(depth, mid.min(), mid.max())


# ------------------------------------------------------------------------------------------------ renderers
def _composite(rgb, w, training):
    if not training:
        rgb = torch.nan_to_num(rgb)
    acc = w.sum(-1, keepdim=True)
    comp = (w[..., None] * rgb).sum(-2) + rgb[:, -1, :] * (1.0 - acc)
    if not training:
        comp = torch.clamp(comp, min=0.0, max=1.0)
    return comp, acc


def composite(rgb, w, training: bool):
    """-> composite [N,C] over the last sample's colour as background, accumulation [N,1].  Eval: nan_to_num on the colours, clamp to [0,1]."""
    return _composite(_d(rgb), _d(w), training)


def composite_grad(rgb, w, d_comp):
    """training form -> d rgb [N,S,C], d weights [N,S] of sum(composite * d_comp)."""
    rgb, w = _d(rgb).requires_grad_(True), _d(w).requires_grad_(True)
    comp, _ = _composite(rgb, w, True)
    (comp * _d(d_comp)).sum().backward()
    return rgb.grad, w.grad


# ------------------------------------------------------------------------------------------------ PDF resampling
def spacing(x):
    return torch.where(x < 1, x / 2, 1 - 1 / (2 * x))


def spacing_inv(x):
    return torch.where(x < 0.5, 2 * x, 1 / (2 - 2 * x))


def s_to_euclidean(s_bins, nears, fars):
    s, s_near, s_far = _d(s_bins), spacing(_d(nears)), spacing(_d(fars))
    return spacing_inv(s * s_far + (1 - s) * s_near)


def pdf_resample(s_bins_prev, weights_prev, S: int, anneal: float, nears, fars, jitter=None):
    """-> s bins [N,S+1], e bins [N,S+1] of the next level.  jitter: None (eval: bin centres) or [N,1] (one jitter per ray)."""
    b, w = _d(s_bins_prev), _d(weights_prev)
    Sp, nb = w.shape[-1], S + 1
    w = torch.pow(w, anneal) + HIST_PAD
    w_sum = w.sum(-1, keepdim=True)
    padding = torch.relu(PDF_EPS - w_sum)
    w = w + padding / Sp
    w_sum = w_sum + padding
    cdf = torch.minimum(torch.ones_like(w), torch.cumsum(w / w_sum, dim=-1))
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], dim=-1)
    u = torch.arange(nb, dtype=F64) / nb  # linspace(0, 1 - 1/nb, nb)
    if jitter is not None:
        u = u[None, :] + _d(jitter).reshape(-1, 1) / nb
    else:
        u = (u + 1.0 / (2 * nb))[None, :].expand(w.shape[0], nb)
    u = u.contiguous()
    inds = torch.searchsorted(cdf, u, side="right")
    below, above = torch.clamp(inds - 1, 0, Sp), torch.clamp(inds, 0, Sp)
    c0, c1 = torch.gather(cdf, -1, below), torch.gather(cdf, -1, above)
    b0, b1 = torch.gather(b, -1, below), torch.gather(b, -1, above)
    t = torch.clip(torch.nan_to_num((u - c0) / (c1 - c0), 0), 0, 1)
    s = b0 + t * (b1 - b0)
    return s, s_to_euclidean(s, nears, fars)


# ------------------------------------------------------------------------------------------------ losses
def distortion(s_bins, w, mult: float = 1.0):
    """-> mult * mean over rays of sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 (t_{i+1} - t_i), and its d weights [N,S]."""
    t, w = _d(s_bins), _d(w).requires_grad_(True)
    m = (t[:, 1:] + t[:, :-1]) / 2.0
    dm = (m[:, :, None] - m[:, None, :]).abs()
    inter = (w * (w[:, None, :] * dm).sum(-1)).sum(-1)
    intra = (w ** 2 * (t[:, 1:] - t[:, :-1])).sum(-1) / 3.0
    loss = mult * (inter + intra).mean()
    loss.backward()
    return loss.detach(), w.grad


def _interlevel_terms(c, w, cp, wp, side_lo="right", side_hi="right"):
    """-> w - w_outer [N,Sf], lo, hi (float64 tensors in)."""
    Sp = wp.shape[-1]
    cy = torch.cat([torch.zeros_like(wp[:, :1]), torch.cumsum(wp, dim=-1)], dim=-1)
    lo = torch.searchsorted(cp[:, :-1].contiguous(), c[:, :-1].contiguous(), side=side_lo) - 1
    lo = torch.clamp(lo, 0, Sp - 1)
    hi = torch.searchsorted(cp[:, 1:].contiguous(), c[:, 1:].contiguous(), side=side_hi)
    hi = torch.clamp(hi, 0, Sp - 1)
    return w - (torch.gather(cy[:, 1:], -1, hi) - torch.gather(cy[:, :-1], -1, lo)), lo, hi


def interlevel(c, w, cp, wp, mult: float = 1.0, side_lo: str = "right", side_hi: str = "right"):
    """c / w: the fine level's s bins and weights (constants), cp / wp: the proposal level's.
    -> mult * mean over rays and fine samples of clip(w - w_outer, 0)^2 / (w + 1e-7), d proposal weights [N,Sp], lo [N,Sf], hi [N,Sf] with
    w_outer_i = cy[hi_i + 1] - cy[lo_i], cy = [0, cumsum(wp)].  The gradient is autograd's, written out: d wp_k = sum over the fine intervals
    that cover k ([lo_i <= k <= hi_i], minus the inverted ones [hi_i < k < lo_i]) of g_i = -2 clip_i / (w_i + 1e-7) * mult / (N Sf).  Autograd
    itself goes back through the cumulative sum and leaves residues of 1e-19 where nothing covers k (interlevel_autograd, and the CPU test
    that holds the two together); summed directly, a zero gradient is an exact zero.
    side_lo / side_hi exist for the tests that show what a wrong side would do."""
    c, w, cp, wp = _d(c), _d(w), _d(cp), _d(wp)
    d, lo, hi = _interlevel_terms(c, w, cp, wp, side_lo, side_hi)
    d = torch.clip(d, min=0)
    loss = mult * (d ** 2 / (w + LOSS_EPS)).mean()
    g = -2.0 * d / (w + LOSS_EPS) * (mult / w.numel())
    k = torch.arange(wp.shape[-1])
    cover = ((lo[..., None] <= k) & (k <= hi[..., None])).to(F64) - ((hi[..., None] < k) & (k < lo[..., None])).to(F64)
    return loss, (cover * g[..., None]).sum(1), lo, hi


def interlevel_autograd(c, w, cp, wp, mult: float = 1.0):
    """-> loss, d proposal weights by float64 autograd."""
    c, w, cp, wp = _d(c), _d(w), _d(cp), _d(wp).requires_grad_(True)
    d = torch.clip(_interlevel_terms(c, w, cp, wp)[0], min=0)
    loss = mult * (d ** 2 / (w + LOSS_EPS)).mean()
    loss.backward()
    return loss.detach(), wp.grad


def interlevel_excess(c, w, cp, wp):
    """w - w_outer [N,Sf] before the clip (the builders' and the tests' clip-margin check)."""
    return _interlevel_terms(_d(c), _d(w), _d(cp), _d(wp))[0]


# ------------------------------------------------------------------------------------------------ inputs
def _bins(N: int, S: int, gen):
    """the oracle's jittered spaced bins between NEAR and FAR -> s bins, e bins, nears, fars (float32)."""
    nears, fars = torch.full((N, 1), NEAR), torch.full((N, 1), FAR)
    s = orc.spaced_bins(N, S, torch.rand((N, 1), generator=gen)).contiguous()
    return s, orc.s_to_euclidean(s, nears, fars).contiguous(), nears, fars


def _random_density(rows: int, S: int, gen):
    return (6.0 * torch.rand((rows, S), generator=gen)) ** 2


EDGE_KINDS = ("empty", "opaque_first", "opaque_last", "underflow", "zero_second_half", "near_eq_far", "duplicate_edge", "tiny_density")
EDGE_MIN_S = {"empty": 1, "opaque_first": 1, "opaque_last": 2, "underflow": 4, "zero_second_half": 2, "near_eq_far": 1, "duplicate_edge": 2,
              "tiny_density": 1}
NEAR_EQ_FAR_DEPTH = 0.02  # below NEAR: this ray alone sets the lower end of the batch-wide depth clip


@functools.lru_cache(maxsize=None)
def edge_batch(S: int, N: int = EDGE_N, seed: int = 0):
    """One level of N rays with S samples: rows 0-7 are EDGE_KINDS (a kind S is too small for stays a random row), the others random
    ((6 U)^2 densities, as the existing tests draw them).  -> dict of float32 tensors s_bins, e_bins [N,S+1], density [N,S], nears, fars [N,1],
    and kinds {name: row}.  Shared between tests: never modified in place."""
    gen = torch.Generator().manual_seed(1000 * seed + S)
    s, e, nears, fars = _bins(N, S, gen)
    dens = _random_density(N, S, gen)
    kinds = {k: r for r, k in enumerate(EDGE_KINDS) if S >= EDGE_MIN_S[k] and r < N}
    for k, r in kinds.items():
        if k == "empty":
            dens[r] = 0.0
        elif k == "opaque_first":
            dens[r, 0] = 1e6
        elif k == "opaque_last":
            dens[r] = 0.0
            dens[r, -1] = 1e6
        elif k == "underflow":  # sum delta sigma reaches 120 at the middle edge: expf(-trans) is 0 for the second half
            dens[r] = 120.0 / float(e[r, S // 2] - e[r, 0])
        elif k == "zero_second_half":
            dens[r, S // 2:] = 0.0
        elif k == "near_eq_far":
            e[r] = NEAR_EQ_FAR_DEPTH
            nears[r] = fars[r] = NEAR_EQ_FAR_DEPTH
        elif k == "duplicate_edge":  # interval S // 2 has width zero, in both spaces
            s[r, S // 2 + 1] = s[r, S // 2]
            e[r, S // 2 + 1] = e[r, S // 2]
        elif k == "tiny_density":
            dens[r] = 1e-12
    fixed = set(kinds.values())
    for _ in range(50):  # no median ties: redraw the random rows that come near one
        tie = (median_index(weights(e, dens))[1] <= MEDIAN_MARGIN).nonzero().flatten().tolist()
        if not tie:
            break
        assert not fixed.intersection(tie), ("a fixed row ties", S, seed, tie)
        dens[tie] = _random_density(len(tie), S, gen)
    else:
        raise AssertionError("edge_batch: median ties survive the redraws")
    return {"s_bins": s, "e_bins": e, "density": dens, "nears": nears, "fars": fars, "kinds": kinds}


@functools.lru_cache(maxsize=None)
def edge_weights(S: int, N: int = EDGE_N, seed: int = 0):
    """the batch's float64 weights rounded to float32: the weights input of the ops that take one."""
    b = edge_batch(S, N, seed)
    return weights(b["e_bins"], b["density"]).float()


@functools.lru_cache(maxsize=None)
def edge_rgb(S: int, C: int, N: int = EDGE_N, seed: int = 0):
    gen = torch.Generator().manual_seed(1000 * seed + 10 * S + C + 7)
    return torch.rand((N, S, C), generator=gen)


def _normalised(rows: int, S: int, total: float, gen, floor: float = 1e-3):
    w = torch.rand((rows, S), generator=gen) ** 2 + floor
    return w * (total / w.sum(-1, keepdim=True))


INTERLEVEL_PAIRS = ((4, 8), (8, 4), (64, 128), (128, 64), (256, 256), (1, 1), (1, 256), (256, 1), (65, 64), (63, 129))
INTERLEVEL_DYADIC = INTERLEVEL_PAIRS[:5]
INTERLEVEL_ROWS = ("zero_fine", "proposal_dominates", "fine_dominates", "duplicate_edges", "generic0", "generic1", "generic2")


@functools.lru_cache(maxsize=None)
def interlevel_case(Sf: int, Sp: int, unsorted_row: bool = False):
    """-> fine bins [N,Sf+1], fine weights [N,Sf], proposal bins [N,Sp+1], proposal weights [N,Sp] (float32), N = len(INTERLEVEL_ROWS).
    The dyadic pairs use linspace(0, 1, S+1) on every ray: edges that coincide do so exactly, interior ties on both searches.
    unsorted_row: the last ray's fine edges are shuffled (the gradient's walk over every interval instead of the sorted fast path)."""
    N = len(INTERLEVEL_ROWS)
    gen = torch.Generator().manual_seed(7000 + 300 * Sf + Sp)
    if (Sf, Sp) in INTERLEVEL_DYADIC:
        c = torch.linspace(0.0, 1.0, Sf + 1)[None, :].repeat(N, 1)
        cp = torch.linspace(0.0, 1.0, Sp + 1)[None, :].repeat(N, 1)
    else:
        c = orc.spaced_bins(N, Sf, torch.rand((N, 1), generator=gen)).clone()
        cp = orc.spaced_bins(N, Sp, torch.rand((N, 1), generator=gen)).clone()
    # d = w - (cy[hi + 1] - cy[lo]) carries the rounding of the fp32 cumulative sums (half an ulp of ~0.7 each) into g = -2 d / (w + eps): an
    # error of ~6e-8 / w_i relative to the largest gradient.  A floor under the weights (every w_i above a sixth of the mean) keeps that below
    # the 1e-4 the loss is held to at 256 samples; weights a thousand times below the mean would measure fp32 itself, not the kernel.
    if Sf >= 2:
        c[3, Sf // 2 + 1] = c[3, Sf // 2]
    if Sp >= 2:
        cp[3, Sp // 2 + 1] = cp[3, Sp // 2]
    if unsorted_row:
        c[N - 1] = c[N - 1][torch.randperm(Sf + 1, generator=gen)]
    for _ in range(50):  # no clip ties: draw the weights again if some w_i comes within CLIP_MARGIN of its w_outer_i
        w = _normalised(N, Sf, 0.8, gen, floor=0.1)
        wp = _normalised(N, Sp, 0.7, gen, floor=0.1)  # (another total than the fine level's: one-sample levels do not tie)
        w[0] = 0.0                                   # g = 0
        wp[1] = 0.9 / Sp                             # every proposal bin outweighs ...
        w[1] = _normalised(1, Sf, 1e-3, gen)[0]      # ... the whole fine ray: d = 0
        wp[2] = _normalised(1, Sp, 1e-3, gen)[0]     # fine weights dominate
        if float(interlevel_excess(c, w, cp, wp).abs().min()) > 2.0 * CLIP_MARGIN:
            break
    else:
        raise AssertionError("interlevel_case: clip ties survive the redraws")
    return c.contiguous(), w.contiguous(), cp.contiguous(), wp.contiguous()


def interlevel_cases(unsorted_row: bool = False):
    return [interlevel_case(Sf, Sp, unsorted_row) for Sf, Sp in INTERLEVEL_PAIRS]


PDF_PAIRS = ((1, 1), (1, 256), (256, 1), (64, 64), (65, 48), (128, 129), (129, 256), (256, 256), (256, 96), (96, 48))
PDF_ROWS = ("zero", "spike", "uniform_one", "duplicate_edge", "generic0", "generic1", "generic2", "generic3", "generic4")
PDF_ANNEALS = (1.0, 0.37)
JITTER_MAX = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))  # the largest float32 below 1


def pdf_cases():
    return PDF_PAIRS


@functools.lru_cache(maxsize=None)
def pdf_case(Sp: int, S: int):
    """The previous level of one PDF case -> dict of float32 s_bins, e_bins [N,Sp+1], weights, density [N,Sp], nears, fars [N,1] and
    jitters {name: None or [N,1]}; N = len(PDF_ROWS).  `density` gives positive weights on the same bins for the fused weights + resample
    launch (its rows: empty, opaque at the spike's sample, then random)."""
    N = len(PDF_ROWS)
    gen = torch.Generator().manual_seed(9000 + 300 * Sp + S)
    s, e, nears, fars = _bins(N, Sp, gen)
    w = _normalised(N, Sp, 0.9, gen)
    w[0] = 0.0
    w[1] = 0.0
    w[1, Sp // 2] = 1.0
    w[2] = 1.0  # an unnormalised sum
    if Sp >= 2:
        s[3, Sp // 2 + 1] = s[3, Sp // 2]
        e[3, Sp // 2 + 1] = e[3, Sp // 2]
    dens = _random_density(N, Sp, gen)
    dens[0] = 0.0
    dens[1] = 0.0
    dens[1, Sp // 2] = 1e6
    jitters = {"none": None, "zero": torch.zeros((N, 1)), "max": torch.full((N, 1), JITTER_MAX)}
    return {"s_bins": s, "e_bins": e, "weights": w.contiguous(), "density": dens, "nears": nears, "fars": fars, "jitters": jitters}
