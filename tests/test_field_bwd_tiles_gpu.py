"""k_field_bwd_fused (the TN_BWD_MLP launch of tn_field_bwd) at the tile counts where its tile loop, its prefetch of the next tile and its block
sum take another path: one tile, a tile and a quarter, one block whose waves walk several tiles and end in a partial one
(tn_field_bwd_max_blocks(1)), and a batch whose blocks differ in tile count.

Every shape has three cameras whose samples interleave inside a tile (rays shorter than a tile, the camera changes from ray to ray), and one
sample with selector 0 (its last bin edge pushed out until the contracted position is exactly on the cube's face).

Reference: the five layers restated here in float64 (base MLP 32 -> 64 -> 16 with ReLU, trunc_exp on output 0, colour head
63 -> 64 -> 64 -> C with ReLU / sigmoid on [SH16 | 15 geo features | 32 appearance-embedding entries]), forward and backward written out, fed with
the oracle's fp32 hash encoding.  Tolerance: 3e-4 of the reference tensor's largest magnitude, the bound tests/test_hip_ops_gpu.py::
test_field_fwd_bwd uses for the same quantities.

Poison: the whole workspace is NaN before the forward writes what it writes, so whatever the backward reads that the forward did not
write for this batch (behind the last tile of an activation array, alignment gaps, rows [P, PT) of the level-major arrays) is NaN and would
show in the outputs.  (The padding lanes of the last tile are NOT poisoned: the forward fills them with copies of the last sample, and the
weight-gradient products multiply them by exact zeros by design.)  Each shape runs twice.  d enc has no cross-block sum and must agree bit
for bit.  The weight, bias and embedding gradients are sums of per-block partial sums added with float atomics, in an order that changes from
run to run: two orders of a sum of n fp32 terms differ by at most 2 (n - 1) u sum|x_i| (u = 2^-24), with n <= 256 blocks + the (per-camera)
flushes of the embedding path (one per ray at most); sum|x_i| is bounded per entry by the same product formed on absolute values in the
float64 restatement.  With one block (the first three shapes) the block's atomics land on zeros and the gradients are bit-identical too, which
is asserted -- except the two that come from the per-camera sums (emb, hw0), which the waves of a block flush with atomics of their own: those
are bit-identical only where one wave does all the work (one tile).
"""
import numpy as np
import pytest
import torch

import thermal_nerfacto_oracle as orc
from field_stage_cases import _ws_float_offsets
from helpers import make_params, tiny_cfg, SEED
from nerfstudio_thermal_amd import _lib, ops, synth
from nerfstudio_thermal_amd.arena import ParamArena
from nerfstudio_thermal_amd.config import ThermalNerfactoModelConfig
from nerfstudio_thermal_amd.netparams import field_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 3e-4  # tests/test_hip_ops_gpu.py::test_field_fwd_bwd
U = 2.0 ** -24

# name -> (rays, samples per ray, block cap of the launch (0 = default))
SHAPES = {
    "one_tile": (4, 8, 0),                   # P = 32: one tile, no prefetch partner
    "tile_and_quarter": (5, 8, 0),           # P = 40: a full tile followed by a quarter tile
    "one_block_partial_end": (229, 1, 1),    # P = 32 * 7 + 5 in ONE block: every wave walks two tiles, the last wave ends in a partial one
    "uneven_blocks": (2054, 16, 0),          # P = 32 * (4 * 256 + 3): 1027 tiles on 1024 waves -> blocks with 8, 3 and 0 tiles
}
GRADS = ("w0", "b0", "w1", "b1", "hw0", "hb0", "hw1", "hb1", "hw2", "hb2", "emb")


def _restatement(p64, k, enc, sel, sh, cam, g_dens, g_rgb, num_images):
    """the five layers in float64, forward and backward; returns the gradients, d enc and the absolute-value bounds of the gradient sums"""
    W0, b0, W1, b1 = p64[k["w0"]], p64[k["b0"]], p64[k["w1"]], p64[k["b1"]]
    H0, c0, H1, c1, H2, c2, E = p64[k["hw0"]], p64[k["hb0"]], p64[k["hw1"]], p64[k["hb1"]], p64[k["hw2"]], p64[k["hb2"]], p64[k["emb"]]
    a1 = enc @ W0.T + b0
    h1 = a1.clamp_min(0)
    bo = h1 @ W1.T + b1
    hin = torch.cat([sh, bo[:, 1:16], E[cam]], dim=1)  # [P, 63]
    a2 = hin @ H0.T + c0
    hh1 = a2.clamp_min(0)
    a3 = hh1 @ H1.T + c1
    hh2 = a3.clamp_min(0)
    y = torch.sigmoid(hh2 @ H2.T + c2)
    g4 = g_rgb * y * (1 - y)
    g3 = (g4 @ H2) * (a3 > 0)
    g2 = (g3 @ H1) * (a2 > 0)
    dhin = g2 @ H0
    dbo = torch.cat([(g_dens * torch.exp(bo[:, 0].clamp(-15, 15)) * sel)[:, None], dhin[:, 16:31]], dim=1)
    g1 = (dbo @ W1) * (a1 > 0)
    onehot = torch.zeros((num_images, enc.shape[0]), dtype=torch.float64)
    onehot[cam, torch.arange(enc.shape[0])] = 1.0
    grads = {"w0": g1.T @ enc, "b0": g1.sum(0), "w1": dbo.T @ h1, "b1": dbo.sum(0), "hw0": g2.T @ hin, "hb0": g2.sum(0), "hw1": g3.T @ hh1,
             "hb1": g3.sum(0), "hw2": g4.T @ hh2, "hb2": g4.sum(0), "emb": onehot @ dhin[:, 31:63]}
    # what the same sums come to on absolute values (the bound on sum|x_i| of every entry)
    ab = torch.abs
    a_g2cam = onehot @ ab(g2)  # [cameras, 64]
    bounds = {"w0": ab(g1).T @ ab(enc), "b0": ab(g1).sum(0), "w1": ab(dbo).T @ ab(h1), "b1": ab(dbo).sum(0),
              "hw0": torch.cat([ab(g2).T @ ab(hin[:, :31]), a_g2cam.T @ ab(E)], dim=1), "hb0": ab(g2).sum(0), "hw1": ab(g3).T @ ab(hh1),
              "hb1": ab(g3).sum(0), "hw2": ab(g4).T @ ab(hh2), "hb2": ab(g4).sum(0), "emb": a_g2cam @ ab(H0[:, 31:63])}
    return grads, g1 @ W0, bounds


_CASES = {}


def _case(name):
    """inputs, the float64 reference (computed once per shape) and the two poisoned runs of the kernel"""
    if name in _CASES:
        return _CASES[name]
    N, S, cap = SHAPES[name]
    P = N * S
    ocfg = tiny_cfg("shared")
    params = make_params(ocfg)
    cfg = ThermalNerfactoModelConfig(density_mode="shared", log2_hashmap_size=ocfg.log2_hashmap_size)
    for a in cfg.proposal_net_args_list:
        a["log2_hashmap_size"] = ocfg.prop_log2_hashmap_size
    arena = ParamArena(cfg, ocfg.num_images, DEV)
    arena.load(params)
    fld = field_params(arena, "field", cfg, with_grads=True)
    C = fld.num_channels
    r = {kk: torch.from_numpy(v) for kk, v in synth.synth_rays_simple(N, 11).items()}
    cam = (torch.arange(N) % 3).to(torch.int64)  # three cameras, changing from ray to ray: they interleave inside every tile
    s = orc.spaced_bins(N, S, None)
    e = orc.s_to_euclidean(s, torch.ones(N, 1) * 0.05, torch.ones(N, 1) * 1000.0).clone()
    dead_ray = N // 2
    e[dead_ray, S] = 2e12  # the ray's last sample lands on the face of the contracted cube (2 - 1e-12 rounds to 2 in fp32): selector 0
    dead = dead_ray * S + S - 1
    smp = orc.Samples(s_bins=s, e_bins=e)
    pos = smp.positions(r["origins"], r["directions"])
    with torch.no_grad():
        _, _, _, enc = orc.field_density(params, "field", ocfg, pos)
        _, sel = orc.unit_cube_positions(pos)
        sh = orc.sh16((r["directions"].double() + 1.0) / 2.0)
    assert float(sel.reshape(-1)[dead]) == 0.0 and int((sel.reshape(-1) == 0).sum()) == 1
    g_dens = torch.from_numpy(synth.uniform("tiles_gd_" + name, (N, S), seed=SEED))
    g_rgb = torch.from_numpy(synth.uniform("tiles_gc_" + name, (N, S, C), seed=SEED)).clone()
    g_rgb.view(P, C)[dead] = 0.0  # nothing reaches the dead sample's d enc but its selector-masked density gradient
    k = orc.field_keys("field")
    p64 = {kk: v.double() for kk, v in params.items()}
    ref, ref_denc, bounds = _restatement(p64, k, enc.double(), sel.reshape(-1).double(), sh.repeat_interleave(S, dim=0), cam.repeat_interleave(S),
                                         g_dens.reshape(-1).double(), g_rgb.reshape(P, C).double(), ocfg.num_images)
    off = _ws_float_offsets(P)
    lib = _lib.load()
    g = lambda x: x.to(DEV).contiguous()  # noqa: E731
    runs = []
    was = lib.tn_field_bwd_max_blocks(cap)
    try:
        for _ in range(2):
            ws = fld.workspace(P, True)
            ws.view(torch.float32).fill_(float("nan"))
            ops.field_fwd(fld, g(r["origins"]), g(r["directions"]), g(cam), g(e), True)
            arena.zero_grad()
            ops.field_bwd(fld, g(r["origins"]), g(r["directions"]), g(cam), g(e), g(g_dens), g(g_rgb))
            torch.cuda.synchronize()
            denc = ws.view(torch.float32)[off["g_enc"]:off["g_enc"] + 32 * P].view(16, P, 2).permute(1, 0, 2).reshape(P, 32).cpu().clone()
            runs.append(({short: arena.grad_view(k[short]).detach().cpu().clone() for short in GRADS}, denc))
    finally:
        lib.tn_field_bwd_max_blocks(was)
    nblocks = max(1, min(-(-(-(-P // 32)) // 4), cap if cap > 0 else 256))
    _CASES[name] = dict(ref=ref, ref_denc=ref_denc, bounds=bounds, runs=runs, dead=dead, nblocks=nblocks, P=P, N=N)
    return _CASES[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_gradients_and_d_enc_match_the_float64_restatement(name):
    c = _case(name)
    got, denc = c["runs"][0]
    for short in GRADS:
        ref = c["ref"][short]
        scale = float(ref.abs().max())
        err = float((got[short].double().reshape(ref.shape) - ref).abs().max())
        print(f"{name} {short}: max err {err:.3e} scale {scale:.3e} ratio {err / scale:.2e}")
        assert torch.isfinite(got[short]).all(), short
        assert err <= TOL * scale, (short, err, scale)
    scale = float(c["ref_denc"].abs().max())
    err = float((denc.double() - c["ref_denc"]).abs().max())
    print(f"{name} d enc: max err {err:.3e} scale {scale:.3e} ratio {err / scale:.2e}")
    assert torch.isfinite(denc).all()
    assert err <= TOL * scale, (err, scale)
    # exact zeros of the restatement (the selector-masked sample; rows whose 64 hidden units are all masked) are exact zeros of the kernel
    zero = c["ref_denc"] == 0
    assert bool(zero[c["dead"]].all())
    assert bool((denc[zero] == 0).all())


@pytest.mark.parametrize("name", list(SHAPES))
def test_two_poisoned_runs_agree(name):
    c = _case(name)
    (g0, d0), (g1, d1) = c["runs"]
    assert torch.equal(d0, d1)  # d enc: no sum across waves or blocks
    for short in GRADS:
        a, b = g0[short].double(), g1[short].double()
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), short
        per_camera = short in ("emb", "hw0")  # fed by the per-camera sums, which every wave flushes with atomics on a camera change
        if c["nblocks"] == 1 and (not per_camera or c["P"] <= 32):
            assert torch.equal(a, b), short  # one block (one wave for the per-camera sums): its atomics land on zeros
            continue
        n = c["nblocks"] + (c["N"] + 8 if per_camera else 0)  # blocks (+ at most one flush per ray)
        bound = 2.0 * (n - 1) * U * c["bounds"][short].reshape(a.shape)
        worst = float(((a - b).abs() - bound).max())
        print(f"{name} {short}: max run-to-run diff {float((a - b).abs().max()):.3e}, largest bound {float(bound.max()):.3e}")
        assert worst <= 0.0, (short, worst)
