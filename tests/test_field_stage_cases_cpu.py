"""The float64 restatements, the bounds and the comparison of tests/field_stage_cases.py, tested on their own (no GPU):
  * the restatements agree with the oracle in float64 and with float64 autograd where both are defined;
  * the fp32 oracle, standing in for the kernels, passes `check` at every stage and every shape with the derived bounds;
  * seeded wrong variants of that stand-in fail `check` at every shape they can affect;
  * the workspace offsets and the fragment / SH-table decoders round-trip against the library's sizes and the lane model of test_mfma_layout_model;
  * the inputs satisfy what the bounds assume (selector margin, distance from mag = 1 and from arg-max ties, exactly one dead sample).
"""
import numpy as np
import pytest
import torch

import field_stage_cases as fsc
import test_mfma_layout_model as lm
import thermal_nerfacto_oracle as orc
from helpers import SEED
from nerfstudio_thermal_amd import _lib, synth

F32, F64 = torch.float32, torch.float64
_CASES = {}


def _case(name):
    """inputs, parameters, every restatement and the fp32 stand-in's outputs of a shape, computed once"""
    if name in _CASES:
        return _CASES[name]
    inp = fsc.make_inputs(name)
    ocfg, N, S, P = inp["ocfg"], inp["N"], inp["S"], inp["P"]
    params = fsc.field_param_tensors(ocfg)
    k = orc.field_keys("field")
    p64 = {kk: v.double() for kk, v in params.items()}
    res = orc.level_resolutions(ocfg.num_levels, ocfg.base_res, ocfg.max_res)
    o, d, e = inp["origins"], inp["directions"], inp["e_bins"]
    prep = fsc.ref_prep(o, d, e)
    # the fp32 oracle as the kernel: positions, selector, SH rows
    with torch.no_grad():
        pos32, sel32 = orc.unit_cube_positions(orc.Samples(s_bins=e, e_bins=e).positions(o, d))
        pos32, sel32 = pos32.reshape(P, 3), sel32.reshape(P).float()
        sh32 = orc.sh16((d + 1.0) / 2.0)
        enc32 = orc.hash_encode(pos32, params[k["table"]], res, ocfg.log2_hashmap_size)
        _, jac32, _, _ = fsc.encode_model(pos32, params[k["table"]], res, ocfg.log2_hashmap_size, dtype=F32)
    enc = fsc.ref_encode(pos32, params[k["table"]], res, ocfg.log2_hashmap_size)
    g_enc = torch.from_numpy(synth.uniform("stage_genc_" + name, (ocfg.num_levels, P, 2), seed=SEED)) * 1e-3
    if inp["zero_ray"] is not None:
        g_enc[:, inp["zero_ray"] * S:(inp["zero_ray"] + 1) * S] = 0.0
    dpos = fsc.ref_dpos(o, d, e, g_enc, jac32, prep["sel"])
    c = dict(inp=inp, params=params, p64=p64, k=k, res=res, prep=prep, pos32=pos32, sel32=sel32, sh32=sh32, enc32=enc32, jac32=jac32, enc=enc,
             g_enc=g_enc, dpos=dpos, chain={t: fsc.ref_chain(p64, k, enc32, sel32, sh32, inp["cam"], S, ocfg.num_images, t) for t in (True, False)})
    _CASES[name] = c
    return c


# ------------------------------------------------------------------------------------------------ the fp32 stand-ins (and their wrong variants)
def _chain32(c, training, all_cam0=False, mean_is_cam0=False, last_is_neighbour=False):
    """the fp32 oracle's five layers (orc.field_density / orc.field_color: nn.Linear + ReLU, trunc_exp, sigmoid) with the intermediates kept"""
    p, k, inp = c["params"], c["k"], c["inp"]
    S, n_img = inp["S"], inp["ocfg"].num_images
    lin = torch.nn.functional.linear
    h1 = torch.relu(lin(c["enc32"], p[k["w0"]], p[k["b0"]]))
    bo = lin(h1, p[k["w1"]], p[k["b1"]])
    E = p[k["emb"]]
    if training:
        cam = inp["cam"]
        camc = torch.zeros_like(cam) if all_cam0 else torch.where((cam < 0) | (cam >= n_img), torch.zeros_like(cam), cam)
        emb = E[camc].repeat_interleave(S, dim=0)
    else:
        emb = (E[0] if mean_is_cam0 else E.mean(dim=0))[None, :].expand(bo.shape[0], 32)
    hin = torch.cat([c["sh32"].repeat_interleave(S, dim=0), bo[:, 1:], emb], dim=1)
    hh1 = torch.relu(lin(hin, p[k["hw0"]], p[k["hb0"]]))
    hh2 = torch.relu(lin(hh1, p[k["hw1"]], p[k["hb1"]]))
    y = torch.sigmoid(lin(hh2, p[k["hw2"]], p[k["hb2"]]))
    out = dict(h1=h1, bo=bo, hh1=hh1, hh2=hh2, y=y, pre=bo[:, 0], density=torch.exp(bo[:, 0]) * c["sel32"])
    if last_is_neighbour:
        out = {kk: torch.cat([v[:-1], v[-2:-1]], dim=0) for kk, v in out.items()}
    return out


def _dpos32(c, drop_partial_share=False):
    """field_dpos_body's arithmetic in fp32 (tn_contract, tn_contract_bwd, per-ray sums) on the stand-in's fp32 Jacobian planes"""
    inp = c["inp"]
    N, S, P = inp["N"], inp["S"], inp["P"]
    o, d, e = inp["origins"], inp["directions"], inp["e_bins"]
    se = e[:, :-1] + e[:, 1:]
    w = (o[:, None, :] + (d[:, None, :] * se[..., None]) / 2.0).reshape(P, 3)
    tm = (se / 2.0).reshape(P, 1)
    g = torch.einsum("lpf,lkpf->pk", c["g_enc"], c["jac32"]) * 0.25
    m = w.abs().amax(dim=1, keepdim=True)
    far = ~(m < 1.0)
    ms = torch.where(far, m, torch.ones_like(m))
    s_, t_ = 2.0 / ms - 1.0 / (ms * ms), -2.0 / (ms * ms) + 2.0 / (ms * ms * ms)
    amax = torch.nn.functional.one_hot(w.abs().argmax(dim=1), 3).float()
    sign = torch.where((w * amax).sum(dim=1, keepdim=True) >= 0, 1.0, -1.0)
    wg = torch.where(far, s_ * g + amax * ((g * w).sum(dim=1, keepdim=True) * t_ * sign), g) * c["sel32"][:, None]
    wd = wg * tm
    if drop_partial_share:  # the last ray's samples in the last, partial tile never reach d directions
        wd = wd.clone()
        wd[max((P // 32) * 32, (N - 1) * S):] = 0.0
    return wg.reshape(N, S, 3).sum(dim=1), wd.reshape(N, S, 3).sum(dim=1)


def _ratios(c, enc_kw=None, jac_sign=False, drop_top=False, chain_kw=None, dpos_kw=None):
    """worst err / bound of the stand-in per stage (a variant: of the stage group it changes alone)"""
    inp, k = c["inp"], c["k"]
    out = {}
    variant = bool(enc_kw or jac_sign or drop_top or chain_kw or dpos_kw)
    if not variant or enc_kw or jac_sign or drop_top:
        _ratios_prep_encode(c, out, enc_kw, jac_sign, drop_top)
    if not variant or chain_kw:
        _ratios_chain(c, out, chain_kw)
    if not variant or dpos_kw:
        _ratios_dpos(c, out, dpos_kw)
    return out


def _ratios_prep_encode(c, out, enc_kw, jac_sign, drop_top):
    inp, k = c["inp"], c["k"]
    out["pos"] = fsc.check("pos", c["pos32"], c["prep"]["pos"], c["prep"]["pos_bound"])[0]
    out["sel"] = 0.0 if torch.equal(c["sel32"].double(), c["prep"]["sel"]) else float("inf")
    out["sh"] = fsc.check("sh", c["sh32"], c["prep"]["sh"], c["prep"]["sh_bound"])[0]
    enc32, jac32 = c["enc32"], c["jac32"]
    if enc_kw:
        enc32, jac32, _, _ = fsc.encode_model(c["pos32"], c["params"][k["table"]], c["res"], inp["ocfg"].log2_hashmap_size, dtype=F32, **enc_kw)
    if drop_top:
        enc32 = enc32.clone()
        enc32[:, -2:] = 0.0
    if jac_sign:
        jac32 = jac32.clone()
        jac32[:, 1] *= -1.0
    renc, benc, rjac, bjac = c["enc"]
    out["enc"] = fsc.check("enc", enc32, renc, benc)[0]
    out["jac"] = fsc.check("jac", jac32, rjac, bjac)[0]


def _ratios_chain(c, out, chain_kw):
    inp, k = c["inp"], c["k"]
    for training in (True, False):
        got = _chain32(c, training, **(chain_kw or {}))
        val, bnd = c["chain"][training]
        for kk in val:
            out[f"{'train' if training else 'eval'}/{kk}"] = fsc.check(kk, got[kk], val[kk], bnd[kk])[0]
        # every layer from the stand-in's own input of that layer (training: the saved activations; eval: the logit alone)
        fed = {kk: got[kk] for kk in (("h1", "bo", "hh1", "hh2", "pre") if training else ("pre",))}
        val, bnd = fsc.ref_chain(c["p64"], k, c["enc32"], c["sel32"], c["sh32"], inp["cam"], inp["S"], inp["ocfg"].num_images, training, fed=fed)
        for kk in (("bo", "hh1", "hh2", "y", "density") if training else ("density",)):
            out[f"{'train' if training else 'eval'}/fed/{kk}"] = fsc.check(kk, got[kk], val[kk], bnd[kk])[0]


def _ratios_dpos(c, out, dpos_kw):
    inp = c["inp"]
    d_o, d_d = _dpos32(c, **(dpos_kw or {}))
    keep = torch.ones(inp["N"], dtype=torch.bool)
    if "mag1" in inp["placed"]:
        keep[inp["placed"]["mag1"]] = False
    out["d_o"] = fsc.check("d_o", d_o[keep], c["dpos"]["d_o"][keep], c["dpos"]["bound_o"][keep])[0]
    out["d_d"] = fsc.check("d_d", d_d[keep], c["dpos"]["d_d"][keep], c["dpos"]["bound_d"][keep])[0]


# ------------------------------------------------------------------------------------------------ the matrix: oracle passes, wrong variants fail
@pytest.mark.parametrize("name", list(fsc.SHAPES))
def test_fp32_oracle_passes_every_stage_with_the_derived_bounds(name):
    r = _ratios(_case(name))
    print(name, " ".join(f"{kk}={v:.3f}" for kk, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), {kk: v for kk, v in r.items() if v > 1.0}


def _partial(name):
    return fsc.SHAPES[name][0] * fsc.SHAPES[name][1] % 32 != 0


# variant -> (keyword arguments of _ratios, the stages that must fail, the shapes it can affect)
VARIANTS = {
    # with ceil == floor the ceil corner has weight 0 in the value: only the Jacobian sees it; every shape has the masked sample at (0, 0, 0)
    "floor_plus_1_for_ceil": (dict(enc_kw=dict(corners="floor+1")), ("jac",), lambda n: True),
    # (one_sample: the only sample is the masked one, all eight corners are one cell)
    "x_lerp_corners_swapped": (dict(enc_kw=dict(swap_x=True)), ("enc",), lambda n: n != "one_sample"),
    "top_level_dropped": (dict(drop_top=True), ("enc",), lambda n: True),
    "last_sample_is_its_neighbour": (dict(chain_kw=dict(last_is_neighbour=True)), ("train/pre", "eval/pre", "train/y", "eval/y"), lambda n: _partial(n) and n != "one_sample"),
    "all_cameras_read_as_0": (dict(chain_kw=dict(all_cam0=True)), ("train/hh1", "train/y", "train/fed/hh1"), lambda n: n != "one_sample"),
    "mean_embedding_is_camera_0": (dict(chain_kw=dict(mean_is_cam0=True)), ("eval/hh1", "eval/y"), lambda n: True),
    "jacobian_y_sign": (dict(jac_sign=True), ("jac",), lambda n: n != "one_sample"),
    # (one_sample: its only sample is masked, nothing reaches d directions)
    "partial_tile_share_dropped": (dict(dpos_kw=dict(drop_partial_share=True)), ("d_d",), lambda n: _partial(n) and n != "one_sample"),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_seeded_wrong_variant_fails_wherever_it_can(variant):
    kw, stages, affects = VARIANTS[variant]
    hit = 0
    for name in fsc.SHAPES:
        if not affects(name):
            continue
        r = _ratios(_case(name), **kw)
        for st in stages:
            assert r[st] > 1.0, (variant, name, st, r[st])
        hit += 1
    assert hit >= 4, (variant, hit)


# ------------------------------------------------------------------------------------------------ the restatements against the oracle / autograd
def _few_bit_positions(P):
    """[P, 3] in (0, 1) with 13 significant bits and odd numerators: p * res is exact in fp32 for every resolution below 2048 and never an integer"""
    kk = torch.from_numpy(synth.uniform("stage_pts", (P, 3), 0.0, 1.0, SEED)).double()
    return ((2.0 * torch.floor(kk * 4095.0) + 1.0) / 8192.0).float()


def test_encode_restatement_is_the_oracles_hash_encode_and_its_autograd_in_float64():
    c = _case("one_tile")
    table, res, log2T = c["params"][c["k"]["table"]], c["res"], c["inp"]["ocfg"].log2_hashmap_size
    pos = _few_bit_positions(37)
    enc, _, jac, _ = fsc.ref_encode(pos, table, res, log2T)
    x = pos.double().requires_grad_(True)
    ref = orc.hash_encode(x, table.double(), res.double(), log2T)
    assert float((enc - ref.detach()).abs().max()) <= 1e-13
    for j in range(ref.shape[1]):
        (gx,) = torch.autograd.grad(ref[:, j].sum(), x, retain_graph=True)
        assert float((jac[j // 2, :, :, j % 2].T - gx).abs().max()) <= 1e-9 * float(res[j // 2]), j


@pytest.mark.parametrize("training", [True, False])
def test_chain_restatement_is_the_oracles_field_in_float64(training):
    c = _case("chunk_edge")
    inp, p64, k = c["inp"], c["p64"], c["k"]
    N, S, ocfg = inp["N"], inp["S"], inp["ocfg"]
    cam = torch.arange(N) % ocfg.num_images
    o, d = inp["origins"].double(), inp["directions"].double()
    pos = orc.Samples(s_bins=inp["e_bins"].double(), e_bins=inp["e_bins"].double()).positions(o, d)
    with torch.no_grad():
        dens, geo, pre, enc = orc.field_density(p64, "field", ocfg, pos)
        rgb = orc.field_color(p64, "field", ocfg, d, geo, cam, training)
        _, sel = orc.unit_cube_positions(pos)
        val, _ = fsc.ref_chain(p64, k, enc, sel.reshape(-1), orc.sh16((d + 1.0) / 2.0), cam, S, ocfg.num_images, training)
    assert float((val["pre"] - pre.reshape(-1)).abs().max()) <= 1e-12
    assert float((val["density"] - dens.reshape(-1)).abs().max()) <= 1e-12 * float(dens.max())
    assert float((val["y"] - rgb.reshape(-1, rgb.shape[-1])).abs().max()) <= 1e-13
    assert float((val["bo"][:, 1:] - geo.reshape(-1, 15)).abs().max()) <= 1e-12


def test_dpos_restatement_is_autograd_through_the_oracles_contraction():
    c = _case("chunk_edge")
    inp = c["inp"]
    N, S, P = inp["N"], inp["S"], inp["P"]
    keep = torch.ones(N, dtype=torch.bool)
    keep[inp["placed"]["mag1"]] = False  # torch.where's gradient at mag == 1 is the test's business nowhere
    o = inp["origins"].double().requires_grad_(True)
    d = inp["directions"].double().requires_grad_(True)
    e = inp["e_bins"].double()
    up = torch.einsum("lpf,lkpf->pk", c["g_enc"].double(), c["jac32"].double())
    p, sel = orc.unit_cube_positions(orc.Samples(s_bins=e, e_bins=e).positions(o, d))
    (p.reshape(P, 3) * up).sum().backward()
    ref = c["dpos"]
    # (autograd sees the dead sample through the float64 selector, which is 1 there: the restatement masks it as the kernel does)
    dead_ray = inp["dead_ray"]
    keep[dead_ray] = False
    for got, want in ((ref["d_o"], o.grad), (ref["d_d"], d.grad)):
        assert float((got[keep] - want[keep]).abs().max()) <= 1e-12 * max(1.0, float(want[keep].abs().max()))
    assert int((ref["d_o"][keep].abs().sum(dim=1) > 0).sum()) >= N - 4


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("P", [1, 32, 33, 129, 513, 65637])
def test_workspace_offsets_add_up_to_the_librarys_sizes(P):
    lib = _lib.load()
    r = lambda nbytes: (nbytes + 255) // 256 * 256  # noqa: E731
    ev, tr = fsc._ws_float_offsets(P, False), fsc._ws_float_offsets(P, True)
    assert ev["end"] * 4 == int(lib.tn_field_workspace_bytes(P, 0))  # pack, pos, enc, sel, sh and nothing else
    for name in ("pack", "pos", "enc", "sel", "sh"):
        assert ev[name] == tr[name]
    # behind jac: the per-camera sums ((FIELD_MAX_IMAGES = 4096) * 64 + 64 floats) and the table scatter's scratch
    assert tr["end"] * 4 + r(4 * (4096 * 64 + 64)) + int(lib.tn_hash_scatter_workspace_bytes(P, 16)) == int(lib.tn_field_workspace_bytes(P, 1))
    PT = (P + 31) // 32 * 32
    assert tr["jac"] - tr["g_enc"] == r(P * 32 * 4) // 4 and tr["end"] - tr["jac"] == r(PT * 96 * 4) // 4
    order = ["pack", "pos", "enc", "sel", "sh", "h1", "hin", "hh1", "hh2", "y", "g_enc", "jac", "end"]
    assert all(tr[a] < tr[b] and tr[a] % 64 == 0 for a, b in zip(order, order[1:]))


def test_fragment_and_sh_table_decoders_round_trip_against_the_lane_model():
    rng = np.random.default_rng(3)
    tiles = 3
    for M, F in ((2, 64), (1, 16)):
        x = rng.uniform(-1, 1, (tiles * 32, F))
        # what the kernel's waves store: register r of lane l of feature tile m (lm.to_tile), as float4 groups [tile][m][g][lane]
        G = 4 if F == 64 else 2
        flat = np.zeros((tiles, M, G, 64, 4))
        for t in range(tiles):
            for m in range(M):
                xt = np.zeros((32, 32 * max(M, 1)))
                xt[:, :F] = x[32 * t:32 * t + 32]
                regs = lm.to_tile(xt, m)  # [64 lanes, 16 registers]
                for g in range(G):
                    flat[t, m, g] = regs[:, 4 * g:4 * g + 4]
        dec = fsc.frag_decode(torch.from_numpy(flat.reshape(-1)), tiles, M)
        assert np.array_equal(dec.numpy(), x)
        assert np.array_equal(fsc.frag_encode(torch.from_numpy(x), M).numpy(), flat.reshape(-1))
    sh = torch.from_numpy(rng.uniform(-1, 1, (5, 16)))
    tab = fsc.shtab_encode(sh)
    for h in range(2):
        for r_ in range(8):
            assert torch.equal(tab[:, 8 * h + r_], sh[:, lm.rrow(r_, h)])
    assert torch.equal(fsc.shtab_decode(tab), sh)
    # level-major rows
    P, PT = 33, 64
    flat = torch.arange(16 * PT * 2, dtype=torch.float64)
    rows, pad = fsc.level_major_rows(flat, 16, P)
    assert rows.shape == (16, P, 2) and pad.shape == (16, PT - P, 2) and float(rows[3, 5, 1]) == (3 * PT + 5) * 2 + 1


# ------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("name", list(fsc.SHAPES))
def test_inputs_satisfy_what_the_bounds_assume(name):
    c = _case(name)
    inp, prep = c["inp"], c["prep"]
    cond = fsc.prep_conditions(inp, prep)
    print(name, cond)
    assert cond["face_margin"] > 1.0         # no live, unplaced coordinate within its position bound of a cube face
    assert cond["dead_count"] == 1 and cond["dead_is_dead"] and cond["dead_on_face"] and cond["dead_within_bound"]
    assert cond["mag1_gap"] > 1e-4 and cond["tie_gap"] > 1e-4
    N, S, P = inp["N"], inp["S"], inp["P"]
    tiles, waves = fsc.fwd_tiles_and_waves(P)
    if name == "second_trip":
        assert tiles == 2052 and waves == 2048 and P % 32 == 5 and -(-P // fsc.ENC_CHUNK) == 129
    else:
        assert tiles <= waves
    if N >= 4:
        pl = inp["placed"]
        lat, face, mag1 = (prep["unmasked"][pl[kk] * S] for kk in ("lattice", "face", "mag1"))
        assert torch.equal(lat, torch.tensor([9.0, 6.0, 11.0], dtype=F64) / 16.0)
        assert float(face[0]) == 1.0 - 2.0 ** -24 and float(prep["sel"][pl["face"] * S]) == 1.0
        assert float(prep["mag"][pl["mag1"] * S]) == 1.0 and float(mag1[0]) == 0.75
        # the lattice ray's level-0 planes are exact zeros of the restatement (ceil == floor on all three axes)
        assert float(c["enc"][2][0, :, pl["lattice"] * S].abs().max()) == 0.0
    if N >= 3:
        cam = inp["cam"]
        assert int(cam[N - 1]) == -1 and int(cam[N - 2]) == inp["ocfg"].num_images and set(cam[:N - 2].tolist()) <= {0, 1, 2}
    assert inp["ocfg"].log2_hashmap_size == (19 if name == "default_table" else 12)
