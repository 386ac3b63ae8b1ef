"""Cases, workspace access and float64 restatements of the main field's forward stages and of its d position pass
(tests/test_field_stage_cases_cpu.py, tests/test_field_fwd_stages_gpu.py).  Not a test module; nothing in it touches a GPU.

Stages (csrc/tn_field.hip, csrc/tn_field_dpos.h):  k_field_prep -> k_field_encode_xcd -> k_field_mlp_fwd / k_field_density_only, and k_field_dpos,
the consumer of the saved Jacobian planes.  Every restatement is fed with the kernel's own fp32 output of the stage before (read from the
workspace), evaluates its stage in float64 and returns the value AND a worst-case bound per entry.  The bounds are counted from the kernel source,
u = 2^-24 (round to nearest), gamma(K) = K u / (1 - K u) bounds (1 + d_1) ... (1 + d_K) - 1; the library is built with -ffp-contract=off, so every
multiply and add of the scalar code rounds once, and an fp32 MFMA is a k-ordered fmaf chain with one rounding per product
(v_mfma_f32_32x32x2_f32).  No bound here was read off a run of the kernel.

prep (ref_prep; tn_contract in tn_common.h, sh16 in tn_field.hip).
  world w = o + (d * (st + en)) / 2: three roundings (st + en, d * se, o + .; / 2 is exact)           -> e_w = gamma(3) (|o| + |d se / 2|)
  mag < 1: c = w.  Else c = (2 - 1 / mag) * (w / mag): four roundings of its own (1 / mag, 2 - ., w / mag, the product) -> gamma(4) |c|, plus e_w
  through the contraction, whose rows have |d c_i / d w|_1 <= s + |w_i| |t| <= 4 / mag (s = 2/m - 1/m^2 <= 2/m, |t| = |-2/m^2 + 2/m^3| <= 2/m^2,
  |w_i| <= m); the second-order terms are below 2^-20 of the first-order ones and covered by a factor (1 + 2^-10).
  p = (c + 2) / 4: one rounding (the division by 4 is exact)                                             -> e_p = (e_c + u |c + 2|) / 4
  p * m with m in {0, 1} is exact.  The selector of the reference is taken on fp32(fp32(c64) + 2) / 4 (the kernel's last two roundings; fp32(p64)
  would not do: below the lower face p64 ~ 1e-13 is a positive fp32 number, while the kernel's c rounds to -2 and its p to 0).  It equals the
  kernel's wherever no coordinate is within e_p of a face (asserted on the reference by the tests); the dead sample's coordinate is within e_p of
  a face AND rounds onto it (asserted).
  SH16: x = (d + 1) / 2 is one rounding (the sum; the halving is exact).  The longest terms are c * y * (3 xx - yy) and c * z * (5 zz - 3): c * y
  carries 3 (the rounded constant, y's own, the product), xx 3 (x twice, the product), 3 * xx 1, the subtraction 1, the last product 1: 9
  -> gamma(9) * (the same polynomial on absolute values with every subtraction turned into an addition).

encode (ref_encode; k_field_encode_xcd).  s32 = fp32(pos) * fp32(res) in fp32 is the model's definition (the oracle and the reference project
  form it in fp32 as well) and s - floor(s) is exact in fp32, so cells, corners and offsets of the restatement ARE the kernel's; everything after
  is float64 with the oracle's corner order and x-then-y-then-z interpolation.  Per corner term w_i f_i the kernel rounds 1 - o (1), the product
  with the x weight (1) and the x sum (1), then product, sum and 1 - o again for y and for z: 9             -> gamma(9) sum_i w_i |f_i|
  Jacobian planes: a corner difference (1), then the y and z lerps (3 each) and the multiply by res (1) for d/dx; the x lerp (3), a difference (1),
  the z lerp (3) and res (1) for d/dy; x and y lerps (6), the difference (1) and res (1) for d/dz: 8        -> gamma(8) res sum (2-D weights) |f_i|

MLP chain (ref_chain; k_field_mlp_fwd).  A layer y = W x + b as an fmaf chain that starts from the bias: a term passes at most K roundings with
  K = (products of the chain) + 1: 33 for Linear(32, 64), 65 for the three 64-slot layers.  Head layer 0 in training starts from
  bias + camhead[cam] (camhead: a 32-term fmaf chain from zero, one more rounding for the sum) and then runs 32 products: 32 + 1 + 32 = 65 as
  well; in eval it runs 64 products on [sh | base outputs | mean embedding].  The last layer sums two 32-term fmaf chains from zero, adds the halves
  and the bias: 34, K = 35.  Any summation order of the same products (the fp32 oracle's) is inside the same K.  Running bound, with e_0 = 0
  because the chain is fed with the kernel's own encoding, selector and SH table:
      e_{l+1} = |W| e_l + gamma(K) (|W| (|x| + e_l) + |b|),   unchanged through ReLU (1-Lipschitz, exact).
  The mean embedding (eval) is a sequential sum of num_images rows and one division: e = gamma(num_images) mean|emb| on its 32 slots.
  expf: ROCm's documentation of the device function's error is not among the files of this project, so 2 ulp (= 4 u relative) is ASSUMED.
  density = expf(pre) * sel (the product with 0 / 1 is exact): exp(pre) (expm1(e_pre) + 5 u); exactly 0 where sel = 0.
  y = 1 / (1 + expf(-e)): expf 4 u, the sum 1 u, the division 1 u, second-order 1 u: 7 u y, plus e_in / 4 (the sigmoid is 1/4-Lipschitz).
  The running bound is a worst case through five layers and grows with every |W| it passes (about 4e-6 on h1, 4e-5 on the logit, 2e-3 on the
  sigmoid outputs with the synthetic weights).  So in training every layer is ALSO restated from the kernel's own saved input of that layer
  (`fed`: h1 -> base outputs, [sh | base outputs | embedding] -> hh1, hh1 -> hh2, hh2 -> y) and, in both modes, the density from the kernel's own
  logit: one layer's gamma(K) (about 1e-5 of sum |w x|) and expf's allowance alone.

d position (ref_dpos; field_dpos_body), fed with the kernel's d enc and Jacobian planes.  dp = sum over 16 levels x 2 features of g * jac, the
  backward of the contraction (tn_contract_bwd: 14 operations on its longest path: t (6), dot (5), dot * t * sign (2), the final add (1)), the
  multiply by tm = (st + en) / 2 for d directions (2), the S samples of the ray and the `pieces` atomics a ray is cut into by tile boundaries:
      |got - ref| <= 2 (n - 1) u A + Q,   n = 32 + 14 + 2 + S + pieces,
  A the same sums formed on absolute values (as the fused backward's test does for its atomic sums).  Q: the kernel evaluates the contraction's
  backward at ITS fp32 world position, e_w away from the restatement's; with |s'| <= 2/m^2 + 2/m^3, |t'| <= 6/m^3 the first-order effect is
  e_w (t_a |g_i| + [i = argmax] (t_a |g|_1 + 6/m^3 sum |g_j w_j|)), t_a = 2/m^2 + 2/m^3 (zero where mag < 1: the backward is g / 4 there).
  Two runs, or the pass as a launch of its own and as co-work of the bin launch, add the same per-tile pieces in another order:
      |a - b| <= 2 (pieces - 1) u A  (bit-identical where a ray lies in one tile).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

import thermal_nerfacto_oracle as orc
from helpers import SEED, tiny_cfg
from nerfstudio_thermal_amd import _lib, synth

U = 2.0 ** -24
EXPF_ULPS = 2  # assumed (see the module docstring)

# name -> (rays, samples per ray)
SHAPES = {
    "one_sample": (1, 1),       # P = 1: every clamp p >= P -> P - 1 of the encode, the chain and d position
    "one_tile": (4, 8),         # P = 32, no partial tile
    "tile_plus_one": (33, 1),   # S = 1: every lane its own ray segment in d position; the last tile holds one sample
    "sub_chunk": (43, 3),       # P = 129: the second u slot of an encode lane pair holds one sample
    "chunk_edge": (27, 19),     # P = 513: a second encode chunk with one sample; rays straddle tile boundaries
    "second_trip": (2431, 27),  # P = 32 * 2051 + 5: 2052 tiles on the chain's 2048 waves, the last tile partial; 129 encode chunks
    "default_table": (5, 8),    # default config: log2_hashmap_size 19, top resolution 2047 (the uint32 hash)
}
FWD_MAX_BLOCKS, FWD_WAVES_PER_BLOCK = 512, 4  # tn_field_fwd_ex: grid = min(cdiv(cdiv(P, 32), 4), 512) blocks of 256 threads
ENC_CHUNK = 512                               # ENC_PER * 128

LATTICE_ORIGIN = (0.25, -0.5, 0.75)          # unit cube (9/16, 6/16, 11/16): a lattice point of level 0 (res 16) on all three axes
FACE_ORIGIN = (4194304.0, 1000.0, -2000.0)   # mag = 2^22: k = 2 - 2^-22, (k + 2) / 4 = 1 - 2^-24, the largest fp32 below the upper face (exact)
MAG1_ORIGIN = (1.0, 0.25, -0.5)              # |x|_inf = 1 exactly: the !(mag < 1) branch with k = 1


def gamma(k):
    return k * U / (1.0 - k * U)


def oracle_cfg(name):
    return orc.OracleConfig(density_mode="shared") if name == "default_table" else tiny_cfg("shared")


def field_param_tensors(ocfg):
    """the main field's synthetic parameters (the tensors of make_params that belong to it)"""
    shapes = {k: v for k, v in orc.param_shapes(ocfg).items() if k.startswith("field.")}
    return {k: torch.from_numpy(v) for k, v in synth.synth_params(shapes, seed=SEED).items()}


# ---------------------------------------------------------------------------------------------------------------- inputs
def _world(o: Tensor, d: Tensor, e: Tensor):
    """float64 world positions [N, S, 3] of the sample midpoints, |d se / 2| and tm"""
    o, d, e = o.double(), d.double(), e.double()
    se = e[:, :-1] + e[:, 1:]
    half = d[:, None, :] * se[..., None] / 2.0
    return o[:, None, :] + half, half.abs(), se / 2.0


def _conditions(w: Tensor):
    """per sample: distance of mag from 1, and the gap between the two largest |coordinates|"""
    a = w.abs().sort(dim=-1, descending=True).values
    return (a[..., 0] - 1.0).abs(), a[..., 0] - a[..., 1]


def make_inputs(name):
    """The inputs of shape `name`: synth.synth_rays_simple with three cameras cycling per ray, camera indices -1 and num_images on the last two rays
    (N >= 3), one dead sample (the last bin edge of ray N // 2 pushed to 2e12: the contracted position rounds onto the cube's face), and where
    N >= 4 three placed rays with direction 0 (lattice, face, mag = 1).  A drawn ray with a sample within 1e-4 of mag = 1 or of a tie of its two
    largest |coordinates| is replaced by the ray of the same index drawn with the next seed (the branch of the contraction and the arg max of its
    backward must not depend on the precision they are evaluated in)."""
    N, S = SHAPES[name]
    ocfg = oracle_cfg(name)
    s = orc.spaced_bins(N, S, None)
    e = orc.s_to_euclidean(s, torch.ones(N, 1) * 0.05, torch.ones(N, 1) * 1000.0).clone()
    dead_ray = N // 2
    e[dead_ray, S] = 2e12
    r = synth.synth_rays_simple(N, 11)
    o, d = torch.from_numpy(r["origins"]).clone(), torch.from_numpy(r["directions"]).clone()
    placed = {}
    if N >= 4:
        free = [i for i in range(N) if i != dead_ray][:3]
        for kind, ray, org in zip(("lattice", "face", "mag1"), free, (LATTICE_ORIGIN, FACE_ORIGIN, MAG1_ORIGIN)):
            placed[kind] = ray
            o[ray] = torch.tensor(org)
            d[ray] = 0.0
    is_placed = torch.zeros(N, dtype=torch.bool)
    is_placed[list(placed.values())] = True
    for seed in range(12, 24):
        near1, tie = _conditions(_world(o, d, e)[0])
        bad = (((near1 < 1e-4) | (tie < 1e-4)).any(dim=1)) & ~is_placed
        if not bool(bad.any()):
            break
        rr = synth.synth_rays_simple(N, seed)
        o[bad], d[bad] = torch.from_numpy(rr["origins"])[bad], torch.from_numpy(rr["directions"])[bad]
    cam = (torch.arange(N) % 3).to(torch.int64)
    bad_cams = []
    if N >= 3:
        cam[N - 1], cam[N - 2] = -1, ocfg.num_images
        bad_cams = [N - 1, N - 2]
    zero_ray = None if N < 4 else (N // 2 + 1 if N >= 8 else placed["lattice"])  # d density = d rgb = 0 on this ray (never the last ray)
    C = ocfg.num_channels
    g_dens = torch.from_numpy(synth.uniform("stage_gd_" + name, (N, S), seed=SEED)).clone()
    g_rgb = torch.from_numpy(synth.uniform("stage_gc_" + name, (N, S, C), seed=SEED)).clone()
    if zero_ray is not None:
        g_dens[zero_ray] = 0.0
        g_rgb[zero_ray] = 0.0
    return dict(name=name, N=N, S=S, P=N * S, ocfg=ocfg, origins=o, directions=d, e_bins=e, cam=cam, bad_cams=bad_cams, dead=dead_ray * S + S - 1,
                dead_ray=dead_ray, placed=placed, zero_ray=zero_ray, g_dens=g_dens, g_rgb=g_rgb)


def fwd_tiles_and_waves(P):
    """(tiles, waves) of k_field_mlp_fwd's launch (the grid formula of tn_field_fwd_ex)"""
    tiles = -(-P // 32)
    return tiles, FWD_WAVES_PER_BLOCK * max(1, min(-(-tiles // FWD_WAVES_PER_BLOCK), FWD_MAX_BLOCKS))


# ---------------------------------------------------------------------------------------------------------------- workspace
_TRAIN_REGIONS = ("pos", "enc", "sel", "sh", "h1", "hin", "hh1", "hh2", "y", "g_enc", "jac")
_EVAL_REGIONS = ("pos", "enc", "sel", "sh")


def region_floats(P, training=True):
    """name -> floats RESERVED for the region (ws_layout in csrc/tn_field.hip), in layout order, the packed weights first"""
    PT = (P + 31) // 32 * 32
    size = {"pos": P * 4, "enc": PT * 32, "sel": P, "sh": P * 16, "h1": PT * 64, "hin": PT * 16, "hh1": PT * 64, "hh2": PT * 64, "y": P * 4,
            "g_enc": P * 32, "jac": PT * 96}
    return {k: size[k] for k in (_TRAIN_REGIONS if training else _EVAL_REGIONS)}


def _ws_float_offsets(P, training=True):
    """float offsets of the workspace regions the tests look at (ws_layout in csrc/tn_field.hip: every region rounded up to 256 bytes); "end" is
    the first float behind the last of them (training: behind jac, where cam_bias and the scatter's scratch follow; eval: the end of the workspace)"""
    lib = _lib.load()
    r = lambda floats: ((floats * 4 + 255) // 256) * 256  # noqa: E731
    off = int(lib.tn_field_workspace_bytes(0, 0))  # the packed weights: every other region is empty at 0 points
    regions = {"pack": 0}
    for name, floats in region_floats(P, training).items():
        regions[name] = off // 4
        off += r(floats)
    total = int(lib.tn_field_workspace_bytes(P, 1 if training else 0))
    assert off < total if training else off == total, (off, total)
    regions["end"] = off // 4
    return regions


def written_floats(N, S, training=True):
    """name -> floats from the start of the region that the FORWARD writes densely (enc and jac are written by rows: see level_major_rows); what
    lies between this and the next region's start must keep its poison.  sh is sized for S = 1 and holds one row per ray; g_enc is the backward's."""
    P = N * S
    w = region_floats(P, training)
    w["sh"] = N * 16
    if training:
        w["g_enc"] = 0
    return w


def frag_decode(flat: Tensor, tiles: int, M: int) -> Tensor:
    """fragment order [tile][m][g][lane] float4 -> [tiles * 32 samples, 32 M features]: lane (j = lane & 31, h = lane >> 5) of group g holds features
    32 m + 8 g + 4 h + {0..3} of sample 32 tile + j (store_frag / store_bo; M = 2 for h1, hh1, hh2; the 16 base outputs are groups 0, 1 of M = 1)"""
    G = flat.numel() // (tiles * M * 64 * 4)
    v = flat.reshape(tiles, M, G, 2, 32, 4)          # [tile][m][g][h][j][q]
    return v.permute(0, 4, 1, 2, 3, 5).reshape(tiles * 32, M * G * 8)  # feature = 32 m + 8 g + 4 h + q (G = 4), 8 g + 4 h + q (G = 2, M = 1)


def frag_encode(x: Tensor, M: int) -> Tensor:
    """inverse of frag_decode for x [tiles * 32, F] with F = 32 M (G = 4) or F = 16 (M = 1, G = 2)"""
    tiles, G = x.shape[0] // 32, x.shape[1] // (8 * M)
    return x.reshape(tiles, 32, M, G, 2, 4).permute(0, 2, 3, 4, 1, 5).reshape(-1)


_SHTAB = torch.tensor([(r & 3) + 8 * (r >> 2) + 4 * h for h in range(2) for r in range(8)])


def shtab_decode(tab: Tensor) -> Tensor:
    """[rays][h][r] = sh[(r & 3) + 8 (r >> 2) + 4 h]  ->  sh [rays, 16]"""
    out = torch.empty_like(tab.reshape(-1, 16))
    out[:, _SHTAB] = tab.reshape(-1, 16)
    return out


def shtab_encode(sh: Tensor) -> Tensor:
    return sh.reshape(-1, 16)[:, _SHTAB].contiguous()


def level_major_rows(flat: Tensor, planes: int, P: int):
    """[planes][PT] float2 (enc: 16 planes; jac: 48 = [16 levels][3 axes]) -> (rows [planes, P, 2], padding rows [planes, PT - P, 2])"""
    PT = (P + 31) // 32 * 32
    v = flat[:planes * PT * 2].reshape(planes, PT, 2)
    return v[:, :P], v[:, P:]


# ---------------------------------------------------------------------------------------------------------------- comparison
def check(stage, got: Tensor, ref: Tensor, bound: Tensor):
    """worst |got - ref| / bound over the entries and where it occurs: (ratio, index tuple).  0 / 0 counts as 0, a non-zero error on a zero bound and a
    non-finite entry as inf.  A ratio above 1 is a finding."""
    got, ref, bound = got.detach().double().cpu(), ref.detach().double().cpu(), bound.detach().double().cpu()
    assert got.shape == ref.shape == bound.shape, (stage, got.shape, ref.shape, bound.shape)
    if got.numel() == 0:
        return 0.0, ()
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isfinite(got) & ~torch.isnan(ratio), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.reshape(-1).argmax())
    return float(ratio.reshape(-1)[i]), tuple(int(x) for x in np.unravel_index(i, tuple(ratio.shape)))


# ---------------------------------------------------------------------------------------------------------------- prep
def _sh16_abs(x: Tensor) -> Tensor:
    """orc.sh16 on absolute values with every subtraction turned into an addition"""
    x, y, z = x[..., 0].abs(), x[..., 1].abs(), x[..., 2].abs()
    xx, yy, zz = x * x, y * y, z * z
    c = torch.zeros((*x.shape, 16), dtype=x.dtype)
    c[..., 0] = 0.28209479177387814
    c[..., 1] = 0.4886025119029199 * y
    c[..., 2] = 0.4886025119029199 * z
    c[..., 3] = 0.4886025119029199 * x
    c[..., 4] = 1.0925484305920792 * x * y
    c[..., 5] = 1.0925484305920792 * y * z
    c[..., 6] = 0.9461746957575601 * zz + 0.31539156525251999
    c[..., 7] = 1.0925484305920792 * x * z
    c[..., 8] = 0.5462742152960396 * (xx + yy)
    c[..., 9] = 0.5900435899266435 * y * (3 * xx + yy)
    c[..., 10] = 2.890611442640554 * x * y * z
    c[..., 11] = 0.4570457994644658 * y * (5 * zz + 1)
    c[..., 12] = 0.3731763325901154 * z * (5 * zz + 3)
    c[..., 13] = 0.4570457994644658 * x * (5 * zz + 1)
    c[..., 14] = 1.445305721320277 * z * (xx + yy)
    c[..., 15] = 0.5900435899266435 * x * (xx + 3 * yy)
    return c


def ref_prep(origins: Tensor, directions: Tensor, e_bins: Tensor):
    """position, selector and SH16 from the fp32 inputs in float64.  Returns dict(pos [P, 3], pos_bound, unmasked [P, 3] (before the selector), sel [P]
    (float64 0 / 1), rounded [P, 3] (what the selector is taken on), sh [N, 16], sh_bound, mag [P], e_w [P] (the bound of the world position, max over the axes), w [P, 3], tm [P])."""
    w, ahalf, tm = _world(origins, directions, e_bins)
    e_w3 = gamma(3) * (origins.double().abs()[:, None, :] + ahalf)
    mag = w.abs().amax(dim=-1, keepdim=True)
    far = ~(mag < 1.0)
    msafe = torch.where(far, mag, torch.ones_like(mag))
    c = torch.where(far, (2.0 - 1.0 / msafe) * (w / msafe), w)
    e_wmax = e_w3.amax(dim=-1, keepdim=True)
    e_c = torch.where(far, (4.0 / msafe) * e_wmax * (1.0 + 2.0 ** -10) + gamma(4) * c.abs(), e_w3)
    p = (c + 2.0) / 4.0
    e_p = (e_c + U * (c + 2.0).abs()) / 4.0
    p32 = (c.float() + 2.0) / 4.0  # the kernel's last two roundings: c to fp32, then the sum (the division by 4 is exact)
    sel = ((p32 > 0.0) & (p32 < 1.0)).all(dim=-1)
    x = (directions.double() + 1.0) / 2.0
    P = p.shape[0] * p.shape[1]
    return dict(pos=(p * sel[..., None]).reshape(P, 3), pos_bound=e_p.reshape(P, 3), unmasked=p.reshape(P, 3), rounded=p32.reshape(P, 3), sel=sel.reshape(P).double(), sh=orc.sh16(x),
                sh_bound=gamma(9) * _sh16_abs(x), mag=mag.reshape(P), e_w=e_wmax.reshape(P), w=w.reshape(P, 3), tm=tm.reshape(P))


def prep_conditions(inp, ref):
    """What the inputs must satisfy, from the reference alone: min over the unplaced, live samples of (distance of a coordinate from a cube face) /
    (its position bound), the dead sample's facts, min |mag - 1| and min arg-max gap over the samples outside the placed rays."""
    P, S = inp["P"], inp["S"]
    ray = torch.arange(P) // S
    placed = torch.zeros(P, dtype=torch.bool)
    for r_ in inp["placed"].values():
        placed |= ray == r_
    keep = ~placed
    keep[inp["dead"]] = False
    un, b = ref["unmasked"], ref["pos_bound"]
    margin = (torch.minimum(un, 1.0 - un) / b)[keep]
    near1, tie = _conditions(ref["w"])
    return dict(face_margin=float(margin.min()) if margin.numel() else float("inf"),
                dead_on_face=bool(((ref["rounded"][inp["dead"]] == 1.0) | (ref["rounded"][inp["dead"]] == 0.0)).any()),
                dead_within_bound=bool((torch.minimum(un[inp["dead"]], 1.0 - un[inp["dead"]]) <= b[inp["dead"]]).any()),
                dead_count=int((ref["sel"] == 0).sum()), dead_is_dead=bool(ref["sel"][inp["dead"]] == 0),
                mag1_gap=float(near1.reshape(P)[~placed].min()) if bool((~placed).any()) else float("inf"),
                tie_gap=float(tie.reshape(P)[~placed].min()) if bool((~placed).any()) else float("inf"))


# ---------------------------------------------------------------------------------------------------------------- encode
_PY, _PZ = 2654435761, 805459861


def encode_model(pos32: Tensor, table: Tensor, res32: Tensor, log2T: int, dtype=torch.float64, corners="ceil", swap_x=False):
    """One evaluation of the encode in `dtype` on the fp32 cells: (enc [P, 2L], jac [L, 3, P, 2], the same two on absolute values).  dtype float64 is
    the restatement; float32 is the kernel's own operation order (the stand-in of the CPU tests).  corners / swap_x seed wrong variants."""
    L, T = res32.shape[0], 2 ** log2T
    s32 = pos32.float()[:, None, :] * res32.float().view(-1, 1)  # [P, L, 3] in fp32: the model's definition
    s = s32.double()
    fl = torch.floor(s)
    f = fl.to(torch.int64)
    c = (f + 1) if corners == "floor+1" else torch.ceil(s).to(torch.int64)
    o = (s - fl).to(dtype)
    lvl = torch.arange(L) * T
    tab = table.to(dtype)
    g = lambda a, b, d_: tab[((a ^ (b * _PY) ^ (d_ * _PZ)) % T) + lvl]  # noqa: E731  [P, L, 2]
    cx, cy, cz, fx, fy, fz = c[..., 0], c[..., 1], c[..., 2], f[..., 0], f[..., 1], f[..., 2]
    f0, f1, f2, f3 = g(cx, cy, cz), g(cx, fy, cz), g(fx, fy, cz), g(fx, cy, cz)
    f4, f5, f6, f7 = g(cx, cy, fz), g(cx, fy, fz), g(fx, fy, fz), g(fx, cy, fz)
    if swap_x:
        f0, f3 = f3, f0
    ox, oy, oz = o[..., 0:1], o[..., 1:2], o[..., 2:3]
    ux, uy, uz = 1 - ox, 1 - oy, 1 - oz
    r = res32.to(dtype).view(1, -1, 1)

    def run(f0, f1, f2, f3, f4, f5, f6, f7, sub):
        f03, f12, f56, f47 = f0 * ox + f3 * ux, f1 * ox + f2 * ux, f5 * ox + f6 * ux, f4 * ox + f7 * ux
        f0312, f4756 = f03 * oy + f12 * uy, f47 * oy + f56 * uy
        enc = f0312 * oz + f4756 * uz
        dx = (sub(f0, f3) * oy + sub(f1, f2) * uy) * oz + (sub(f4, f7) * oy + sub(f5, f6) * uy) * uz
        dy = sub(f03, f12) * oz + sub(f47, f56) * uz
        dz = sub(f0312, f4756)
        return enc, torch.stack([dx * r, dy * r, dz * r], dim=0)  # [P, L, 2], [3, P, L, 2]

    enc, jac = run(f0, f1, f2, f3, f4, f5, f6, f7, lambda a, b: a - b)
    aenc, ajac = run(*[t.abs() for t in (f0, f1, f2, f3, f4, f5, f6, f7)], lambda a, b: a + b)
    P = pos32.shape[0]
    return enc.reshape(P, 2 * L), jac.permute(2, 0, 1, 3).contiguous(), aenc.reshape(P, 2 * L), ajac.permute(2, 0, 1, 3).contiguous()


def ref_encode(pos32: Tensor, table: Tensor, res32: Tensor, log2T: int):
    """(enc [P, 2L], its bound, jac [L, 3, P, 2] = res * d enc / d offset, its bound) in float64 from the kernel's fp32 positions"""
    enc, jac, aenc, ajac = encode_model(pos32, table, res32, log2T)
    return enc, gamma(9) * aenc, jac, gamma(8) * ajac


# ---------------------------------------------------------------------------------------------------------------- MLP chain
K_BASE0, K_64, K_HEAD2 = 33, 65, 35


def _layer(W, b, x, e, K):
    y = x @ W.T + b
    return y, e @ W.abs().T + gamma(K) * ((x.abs() + e) @ W.abs().T + b.abs())


def ref_chain(p64, k, enc32: Tensor, sel: Tensor, sh32: Tensor, cam, S: int, num_images: int, training: bool, fed=None):
    """The five layers in float64 on the kernel's fp32 encoding [P, 32], selector [P] and SH rows [N, 16] with the running bound of the module
    docstring.  cam [N] int64 (training: out-of-range indices read camera 0; eval: ignored, the mean embedding is used).  Returns (values, bounds):
    dicts with h1, bo (the 16 base outputs), hh1, hh2, y, pre, density.
    fed: the kernel's own fp32 h1, bo, hh1, hh2 (saved activations, [P, .]) and / or pre [P]: every layer then starts from the kernel's input of THAT
    layer with no inherited error (one layer's gamma(K) alone, no growth through the |W| of the layers behind it), and the density from the kernel's
    own logit (expf's allowance alone)."""
    W0, b0, W1, b1 = p64[k["w0"]], p64[k["b0"]], p64[k["w1"]], p64[k["b1"]]
    H0, c0, H1, c1, H2, c2, E = p64[k["hw0"]], p64[k["hb0"]], p64[k["hw1"]], p64[k["hb1"]], p64[k["hw2"]], p64[k["hb2"]], p64[k["emb"]]
    x0 = enc32.double()
    P = x0.shape[0]
    fed = fed or {}
    own = lambda nm, x, e_: (fed[nm].double(), torch.zeros_like(e_)) if nm in fed else (x, e_)  # noqa: E731  what the next layer starts from
    a1, e1 = _layer(W0, b0, x0, torch.zeros_like(x0), K_BASE0)
    h1 = a1.clamp_min(0)
    bo, ebo = _layer(W1, b1, *own("h1", h1, e1), K_64)
    if training:
        camc = torch.where((cam < 0) | (cam >= num_images), torch.zeros_like(cam), cam)
        emb_in = E[camc].repeat_interleave(S, dim=0)
        e_emb = torch.zeros_like(emb_in)
    else:
        emb_in = E.mean(dim=0)[None, :].expand(P, 32)
        e_emb = (gamma(num_images) * E.abs().mean(dim=0))[None, :].expand(P, 32)
    bo_in, ebo_in = own("bo", bo, ebo)
    hin = torch.cat([sh32.double().repeat_interleave(S, dim=0), bo_in[:, 1:16], emb_in], dim=1)
    ehin = torch.cat([torch.zeros(P, 16, dtype=torch.float64), ebo_in[:, 1:16], e_emb], dim=1)
    a2, e2 = _layer(H0, c0, hin, ehin, K_64)
    hh1 = a2.clamp_min(0)
    a3, e3 = _layer(H1, c1, *own("hh1", hh1, e2), K_64)
    hh2 = a3.clamp_min(0)
    a4, e4 = _layer(H2, c2, *own("hh2", hh2, e3), K_HEAD2)
    y = torch.sigmoid(a4)
    ulp = 2.0 * EXPF_ULPS * U
    pre, epre = bo[:, 0], ebo[:, 0]
    pre_in, epre_in = own("pre", pre, epre)
    sel = sel.double()
    val = dict(h1=h1, bo=bo, hh1=hh1, hh2=hh2, y=y, pre=pre, density=torch.exp(pre_in) * sel)
    bnd = dict(h1=e1, bo=ebo, hh1=e2, hh2=e3, y=0.25 * e4 + (ulp + 3.0 * U) * y, pre=epre,
               density=torch.exp(pre_in) * (torch.expm1(epre_in) + ulp + U) * sel)
    return val, bnd


# ---------------------------------------------------------------------------------------------------------------- d position
N_DPOS_FIXED = 32 + 14 + 2  # products, tn_contract_bwd's longest path, (st + en) / 2 and the product with it


def ray_pieces(N, S):
    """tiles every ray's samples fall into (the atomics its sums are cut into)"""
    first = torch.arange(N) * S
    return (first + S - 1) // 32 - first // 32 + 1


def ref_dpos(origins: Tensor, directions: Tensor, e_bins: Tensor, g_enc: Tensor, jac: Tensor, sel: Tensor):
    """d origins / d directions in float64 from the kernel's d enc g_enc [L, P, 2] and Jacobian planes jac [L, 3, P, 2] and the reference selector
    [P].  Returns dict(d_o [N, 3], d_d, bound_o, bound_d, order_o, order_d (the bound between two orders of the per-tile atomics), abs_o, abs_d)."""
    N, S = e_bins.shape[0], e_bins.shape[1] - 1
    pr = ref_prep(origins, directions, e_bins)
    w, m, tm, e_w = pr["w"], pr["mag"][:, None], pr["tm"][:, None], pr["e_w"][:, None]
    g = torch.einsum("lpf,lkpf->pk", g_enc.double(), jac.double()) * 0.25
    ga = torch.einsum("lpf,lkpf->pk", g_enc.double().abs(), jac.double().abs()) * 0.25
    far = ~(m < 1.0)
    ms = torch.where(far, m, torch.ones_like(m))
    s_, t_ = 2.0 / ms - 1.0 / (ms * ms), -2.0 / (ms * ms) + 2.0 / (ms * ms * ms)
    sa, ta = 2.0 / ms + 1.0 / (ms * ms), 2.0 / (ms * ms) + 2.0 / (ms * ms * ms)
    amax = torch.nn.functional.one_hot(w.abs().argmax(dim=1), 3).double()
    sign = torch.where((w * amax).sum(dim=1, keepdim=True) >= 0, 1.0, -1.0)
    dot, dota = (g * w).sum(dim=1, keepdim=True), (ga * w.abs()).sum(dim=1, keepdim=True)
    wg = torch.where(far, s_ * g + amax * dot * t_ * sign, g) * sel[:, None]
    wga = torch.where(far, sa * ga + amax * dota * ta, ga) * sel[:, None]
    q = torch.where(far, e_w * (ta * ga + amax * (ta * ga.sum(dim=1, keepdim=True) + 6.0 / (ms * ms * ms) * dota)), torch.zeros_like(ga)) * sel[:, None]
    per_ray = lambda x: x.reshape(N, S, 3).sum(dim=1)  # noqa: E731
    pieces = ray_pieces(N, S).double()[:, None]
    n = N_DPOS_FIXED + S + pieces
    abs_o, abs_d = per_ray(wga), per_ray(wga * tm.abs())
    return dict(d_o=per_ray(wg), d_d=per_ray(wg * tm), abs_o=abs_o, abs_d=abs_d,
                bound_o=2.0 * (n - 1) * U * abs_o + per_ray(q), bound_d=2.0 * (n - 1) * U * abs_d + per_ray(q * tm.abs()),
                order_o=2.0 * (pieces - 1) * U * abs_o, order_d=2.0 * (pieces - 1) * U * abs_d)
