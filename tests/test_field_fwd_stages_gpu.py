"""The main field's forward, stage by stage (k_field_prep -> k_field_encode_xcd -> k_field_mlp_fwd / k_field_density_only in csrc/tn_field.hip), and
k_field_dpos (csrc/tn_field_dpos.h), the consumer of the saved Jacobian planes, against the float64 restatements of tests/field_stage_cases.py at
the shapes where their loops change path (SHAPES there), in training and in eval.

Every stage's restatement is fed with the kernel's own fp32 output of the stage before, read from the workspace, and compared within the
worst-case bound derived in field_stage_cases' docstring (rounding counts from the kernel source; expf at an ASSUMED 2 ulp): a ratio
err / bound above 1 is a finding, never a reason to widen a bound.  The whole workspace is NaN before every forward and every shape runs twice:
what the forward must not write (rows [P, PT) of the level-major arrays, alignment gaps, in eval everything behind the SH table) still holds
the poison afterwards, and the two runs agree bit for bit (the forward has no atomics).  The worst ratio per stage is printed (-s).

Largest ratios seen on an MI355X over all shapes when the file was added, as recorded values (not thresholds): pos 0.96, sh 0.49, enc 0.46,
jac 0.54; running bound: h1 0.14, base outputs 0.014, hh1 0.019, hh2 0.001, logit 0.013, density 0.013, y below 0.001; one layer from the
kernel's own input: base outputs 0.066, hh1 0.075, hh2 0.062, y 0.069, density from the kernel's logit 0.27 (of 5 u: expf within the assumed
2 ulp); d origins 0.013, d directions 0.017 (own launch and co-work alike).
"""
import os

import pytest
import torch

import field_stage_cases as fsc
import thermal_nerfacto_oracle as orc
from nerfstudio_thermal_amd import ops
from nerfstudio_thermal_amd.arena import ParamArena
from nerfstudio_thermal_amd.config import ThermalNerfactoModelConfig
from nerfstudio_thermal_amd.netparams import field_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("train", "eval")
_SETUPS, _CASES = {}, {}


def _setup(name):
    """inputs, parameters (host float64 and device arena) of a shape"""
    if name in _SETUPS:
        return _SETUPS[name]
    inp = fsc.make_inputs(name)
    ocfg = inp["ocfg"]
    params = fsc.field_param_tensors(ocfg)
    cfg = ThermalNerfactoModelConfig(density_mode="shared", log2_hashmap_size=ocfg.log2_hashmap_size)
    for a in cfg.proposal_net_args_list:
        a["log2_hashmap_size"] = ocfg.prop_log2_hashmap_size
    arena = ParamArena(cfg, ocfg.num_images, DEV)
    arena.load(params)
    fld = field_params(arena, "field", cfg, with_grads=True)
    k = orc.field_keys("field")
    _SETUPS[name] = dict(inp=inp, params=params, p64={kk: v.double() for kk, v in params.items()}, k=k, arena=arena, fld=fld,
                         res=orc.level_resolutions(ocfg.num_levels, ocfg.base_res, ocfg.max_res), prep=fsc.ref_prep(inp["origins"], inp["directions"], inp["e_bins"]))
    return _SETUPS[name]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _region(snap, off, name, floats):
    return snap[off[name]:off[name] + floats]


def _case(name, mode):
    """the two poisoned runs of the forward (outputs, the workspace behind the packed weights, what kept its poison), the density-only forward
    beside each, and in training the backward's d position as a launch of its own and as co-work of the bin launch"""
    if (name, mode) in _CASES:
        return _CASES[(name, mode)]
    su = _setup(name)
    inp, fld, arena = su["inp"], su["fld"], su["arena"]
    training = mode == "train"
    N, S, P = inp["N"], inp["S"], inp["P"]
    PT = (P + 31) // 32 * 32
    off = fsc._ws_float_offsets(P, training)
    written = fsc.written_floats(N, S, training)
    g = lambda x: x.to(DEV).contiguous()  # noqa: E731
    o, d, cam, e = g(inp["origins"]), g(inp["directions"]), g(inp["cam"]), g(inp["e_bins"])
    names = list(fsc.region_floats(P, training))
    runs = []
    for _ in range(2):
        ws = fld.workspace(P, training)
        wsf = ws.view(torch.float32)
        wsf.fill_(float("nan"))
        dens, rgb, pre = ops.field_fwd(fld, o, d, cam, e, training, want_pre=True)
        torch.cuda.synchronize()
        poison = {}
        for i, nm in enumerate(names):  # the gap between what the forward writes of a region and the start of the next one
            nxt = off[names[i + 1]] if i + 1 < len(names) else off["end"]
            if nm in ("enc", "jac"):
                planes = 16 if nm == "enc" else 48
                body = wsf[off[nm]:off[nm] + planes * PT * 2].view(planes, PT, 2)
                poison[nm + " rows [P, PT)"] = bool(torch.isnan(body[:, P:]).all())
                poison[nm + " gap"] = bool(torch.isnan(wsf[off[nm] + planes * PT * 2:nxt]).all())
            else:
                poison[nm + " gap"] = bool(torch.isnan(wsf[off[nm] + written[nm]:nxt]).all())
        if not training:
            poison["behind sh"] = bool(torch.isnan(wsf[off["sh"] + written["sh"]:]).all())
        snap = wsf[:off["end"]].cpu().clone()
        wc = fld.workspace(P, training, "cross")
        wc.view(torch.float32).fill_(float("nan"))
        dcross = ops.field_density_fwd(fld, o, d, e, training=training, tag="cross")
        torch.cuda.synchronize()
        logit = None
        if training:
            hin = wc.view(torch.float32)[off["hin"]:off["hin"] + PT * 16].cpu()
            logit = fsc.frag_decode(hin, PT // 32, 1)[:P, 0]
        runs.append(dict(dens=dens.cpu().reshape(P), rgb=rgb.cpu().reshape(P, -1), pre=pre.cpu().reshape(P), snap=snap, poison=poison,
                         dcross=dcross.cpu().reshape(P), logit=logit))
    c = dict(su=su, off=off, runs=runs, P=P, PT=PT)
    if training:
        was = os.environ.get("TN_DPOS_COWORK")
        try:
            c["dpos"] = {}
            for cw in ("0", "1"):  # "0": k_field_dpos as a launch of its own; "1": in extra blocks of the table scatter's bin launch
                os.environ["TN_DPOS_COWORK"] = cw
                arena.zero_grad()
                d_o, d_d = torch.zeros((N, 3), device=DEV), torch.zeros((N, 3), device=DEV)
                ops.field_bwd(fld, o, d, cam, e, g(inp["g_dens"]), g(inp["g_rgb"]), d_o, d_d)
                torch.cuda.synchronize()
                wsf = fld.workspace(P, True).view(torch.float32)
                c["dpos"][cw] = dict(d_o=d_o.cpu(), d_d=d_d.cpu(), g_enc=wsf[off["g_enc"]:off["g_enc"] + 32 * P].cpu().clone().view(16, P, 2),
                                     jac=wsf[off["jac"]:off["jac"] + 96 * PT].cpu().clone())
        finally:
            if was is None:
                os.environ.pop("TN_DPOS_COWORK", None)
            else:
                os.environ["TN_DPOS_COWORK"] = was
    _CASES[(name, mode)] = c
    return c


def _report(name, mode, stage, ratio, where=()):
    print(f"RATIO {name:14s} {mode:5s} {stage:12s} {ratio:.4f} at {where}")


def _kernel_prep(c, run=0):
    """(pos [P, 3], selector of pos.w [P], sel [P], sh rows [N, 16]) as the kernel left them"""
    su, off, P = c["su"], c["off"], c["P"]
    snap, N = c["runs"][run]["snap"], su["inp"]["N"]
    pos4 = _region(snap, off, "pos", 4 * P).view(P, 4)
    return pos4[:, :3], pos4[:, 3], _region(snap, off, "sel", P), fsc.shtab_decode(_region(snap, off, "sh", 16 * N))


def _kernel_enc(c, run=0):
    rows, _ = fsc.level_major_rows(_region(c["runs"][run]["snap"], c["off"], "enc", 32 * c["PT"]), 16, c["P"])
    return rows.permute(1, 0, 2).reshape(c["P"], 32)


ALL = [(n, m) for n in fsc.SHAPES for m in MODES]


@pytest.mark.parametrize("name,mode", ALL)
def test_prep_matches_the_restatement(name, mode):
    c = _case(name, mode)
    prep, inp = c["su"]["prep"], c["su"]["inp"]
    pos, posw, sel, sh = _kernel_prep(c)
    assert torch.equal(sel.double(), prep["sel"]) and torch.equal(posw, sel)  # the selector matches exactly
    assert float(sel[inp["dead"]]) == 0.0 and bool((pos[inp["dead"]] == 0).all())  # a masked position is exactly (0, 0, 0)
    assert bool((pos[sel == 0] == 0).all())
    for stage, got, ref, bound in (("pos", pos, prep["pos"], prep["pos_bound"]), ("sh", sh, prep["sh"], prep["sh_bound"])):
        ratio, where = fsc.check(stage, got, ref, bound)
        _report(name, mode, stage, ratio, where)
        assert ratio <= 1.0, (stage, ratio, where)


@pytest.mark.parametrize("name,mode", ALL)
def test_encode_and_jacobian_planes_match_the_restatement(name, mode):
    c = _case(name, mode)
    su, P, PT = c["su"], c["P"], c["PT"]
    inp = su["inp"]
    pos = _kernel_prep(c)[0]
    enc, benc, jac, bjac = fsc.ref_encode(pos, su["params"][su["k"]["table"]], su["res"], inp["ocfg"].log2_hashmap_size)
    ratio, where = fsc.check("enc", _kernel_enc(c), enc, benc)
    _report(name, mode, "enc", ratio, where)
    assert ratio <= 1.0, ("enc", ratio, where)
    if mode != "train":
        return
    rows, _ = fsc.level_major_rows(_region(c["runs"][0]["snap"], c["off"], "jac", 96 * PT), 48, P)
    got = rows.reshape(16, 3, P, 2)
    ratio, where = fsc.check("jac", got, jac, bjac)
    _report(name, mode, "jac", ratio, where)
    assert ratio <= 1.0, ("jac", ratio, where)
    if "lattice" in inp["placed"]:  # ceil == floor on all three axes of level 0: the planes are exactly the restatement's (zeros)
        p = inp["placed"]["lattice"] * inp["S"]
        assert torch.equal(got[0, :, p].double(), jac[0, :, p]) and float(jac[0, :, p].abs().max()) == 0.0


@pytest.mark.parametrize("name,mode", ALL)
def test_chain_outputs_and_saved_activations_match_the_restatement(name, mode):
    c = _case(name, mode)
    su, off, P, PT = c["su"], c["off"], c["P"], c["PT"]
    inp, run = su["inp"], c["runs"][0]
    N, S, training = inp["N"], inp["S"], mode == "train"
    _, _, sel, sh = _kernel_prep(c)
    val, bnd = fsc.ref_chain(su["p64"], su["k"], _kernel_enc(c), sel, sh, inp["cam"], S, inp["ocfg"].num_images, training)
    got = dict(pre=run["pre"], density=run["dens"], y=run["rgb"])
    if training:
        snap, tiles = run["snap"], PT // 32
        for nm, M, floats in (("h1", 2, 64), ("hin", 1, 16), ("hh1", 2, 64), ("hh2", 2, 64)):
            full = fsc.frag_decode(_region(snap, off, nm, PT * floats), tiles, M)
            assert bool(torch.isfinite(full).all()), nm  # every lane of the last, partial tile is written
            got["bo" if nm == "hin" else nm] = full[:P]
        ysaved = _region(snap, off, "y", 4 * P).view(P, 4)
        assert torch.equal(_bits(ysaved[:, :run["rgb"].shape[1]]), _bits(run["rgb"]))  # the sigmoid outputs kept for the backward are the outputs
    for stage, gv in got.items():
        ratio, where = fsc.check(stage, gv, val[stage], bnd[stage])
        _report(name, mode, stage, ratio, where)
        assert ratio <= 1.0, (stage, ratio, where)
    # every layer again from the kernel's own input of that layer (training: the saved activations), the density from the kernel's own logit:
    # one layer's bound, not the running one
    fed = {kk: got[kk] for kk in (("h1", "bo", "hh1", "hh2", "pre") if training else ("pre",))}
    fval, fbnd = fsc.ref_chain(su["p64"], su["k"], _kernel_enc(c), sel, sh, inp["cam"], S, inp["ocfg"].num_images, training, fed=fed)
    for stage in (("bo", "hh1", "hh2", "y", "density") if training else ("density",)):
        ratio, where = fsc.check(stage, got[stage], fval[stage], fbnd[stage])
        _report(name, mode, "fed/" + stage, ratio, where)
        assert ratio <= 1.0, ("fed", stage, ratio, where)
    assert float(run["dens"][inp["dead"]]) == 0.0 and bool((run["dens"][sel == 0] == 0).all())  # exactly 0 where the selector is 0
    if training and inp["bad_cams"]:  # camera indices -1 and num_images read camera 0 (the restatement's clamp), compared on those rays alone
        for ray in inp["bad_cams"]:
            sl = slice(ray * S, (ray + 1) * S)
            ratio, where = fsc.check("y", run["rgb"][sl], val["y"][sl], bnd["y"][sl])
            assert ratio <= 1.0, ("bad camera", ray, ratio)
    # the density-only forward: bit-equal density, and in training its saved logit is the full forward's
    assert torch.equal(_bits(run["dcross"]), _bits(run["dens"]))
    if training:
        assert torch.equal(_bits(run["logit"]), _bits(run["pre"]))


@pytest.mark.parametrize("name,mode", ALL)
def test_forward_writes_nothing_else(name, mode):
    c = _case(name, mode)
    for i, run in enumerate(c["runs"]):
        lost = [kk for kk, ok in run["poison"].items() if not ok]
        assert not lost, (i, lost)
    assert ("behind sh" in c["runs"][0]["poison"]) == (mode == "eval")
    if mode == "train":  # d enc is the backward's: the forward leaves the whole region alone
        assert "g_enc gap" in c["runs"][0]["poison"] and fsc.written_floats(c["su"]["inp"]["N"], c["su"]["inp"]["S"])["g_enc"] == 0


@pytest.mark.parametrize("name,mode", ALL)
def test_two_poisoned_runs_agree_bit_for_bit(name, mode):
    a, b = _case(name, mode)["runs"]
    for kk in ("dens", "rgb", "pre", "dcross", "snap"):  # (snap: the workspace from the packed weights to the end of jac / of the eval layout)
        assert torch.equal(_bits(a[kk]), _bits(b[kk])), kk
    if mode == "train":
        assert torch.equal(_bits(a["logit"]), _bits(b["logit"]))


@pytest.mark.parametrize("name", list(fsc.SHAPES))
def test_d_position_matches_the_restatement_as_own_launch_and_as_co_work(name):
    c = _case(name, "train")
    su, P, PT = c["su"], c["P"], c["PT"]
    inp = su["inp"]
    N, S = inp["N"], inp["S"]
    own, cow = c["dpos"]["0"], c["dpos"]["1"]
    assert torch.equal(_bits(own["g_enc"]), _bits(cow["g_enc"])) and torch.equal(_bits(own["jac"]), _bits(cow["jac"]))
    # the backward reads the planes the forward saved and leaves them alone
    assert torch.equal(_bits(own["jac"]), _bits(_region(c["runs"][1]["snap"], c["off"], "jac", 96 * PT)))
    rows, _ = fsc.level_major_rows(own["jac"], 48, P)
    assert bool(torch.isfinite(own["g_enc"]).all())
    ref = fsc.ref_dpos(inp["origins"], inp["directions"], inp["e_bins"], own["g_enc"], rows.reshape(16, 3, P, 2), su["prep"]["sel"])
    keep = torch.ones(N, dtype=torch.bool)
    if "mag1" in inp["placed"]:
        keep[inp["placed"]["mag1"]] = False  # (the branch of the contraction's backward at mag == 1 exactly is not this test's business)
    for tag, run in (("own", own), ("cowork", cow)):
        for kk in ("d_o", "d_d"):
            ratio, where = fsc.check(kk, run[kk][keep], ref[kk][keep], ref["bound_" + kk[-1]][keep])
            _report(name, "train", f"{kk}/{tag}", ratio, where)
            assert ratio <= 1.0, (tag, kk, ratio, where)
    for kk in ("d_o", "d_d"):  # the two differ by the order of the per-tile atomics at most
        diff = (own[kk].double() - cow[kk].double()).abs()
        assert bool((diff <= ref["order_" + kk[-1]]).all()), (kk, float((diff - ref["order_" + kk[-1]]).max()))
    if inp["zero_ray"] is not None:  # a ray whose samples all have zero d enc keeps exactly-zero rows
        z = inp["zero_ray"]
        assert float(own["g_enc"][:, z * S:(z + 1) * S].abs().max()) == 0.0
        for run in (own, cow):
            assert float(run["d_o"][z].abs().max()) == 0.0 and float(run["d_d"][z].abs().max()) == 0.0
    # the dead sample's ray gets nothing from it: its selector masks the contraction's backward (restated the same way)
    assert bool(torch.isfinite(own["d_o"]).all() and torch.isfinite(own["d_d"]).all())


@pytest.mark.parametrize("name", list(fsc.SHAPES))
def test_eval_shares_the_training_forwards_density_path(name):
    """The eval launches (encode without the Jacobian planes, chain without the saved activations) run the same arithmetic up to the base MLP's
    outputs: positions, encoding, logit and density agree bit for bit with the training forward's.  That makes the training run's saved base
    outputs the eval chain's own input of the colour head: eval's colours are restated from them (three layers of running bound instead of five)."""
    tr, ev = _case(name, "train"), _case(name, "eval")
    su, P, PT = tr["su"], tr["P"], tr["PT"]
    inp = su["inp"]
    for a, b in zip(_kernel_prep(tr), _kernel_prep(ev)):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(_kernel_enc(tr)), _bits(_kernel_enc(ev)))
    for kk in ("pre", "dens"):
        assert torch.equal(_bits(tr["runs"][0][kk]), _bits(ev["runs"][0][kk])), kk
    snap = tr["runs"][0]["snap"]
    fed = {"h1": fsc.frag_decode(_region(snap, tr["off"], "h1", PT * 64), PT // 32, 2)[:P],
           "bo": fsc.frag_decode(_region(snap, tr["off"], "hin", PT * 16), PT // 32, 1)[:P]}
    _, _, sel, sh = _kernel_prep(ev)
    val, bnd = fsc.ref_chain(su["p64"], su["k"], _kernel_enc(ev), sel, sh, inp["cam"], inp["S"], inp["ocfg"].num_images, False, fed=fed)
    ratio, where = fsc.check("y", ev["runs"][0]["rgb"], val["y"], bnd["y"])
    _report(name, "eval", "fed/y", ratio, where)
    print(f"BOUND {name} eval y from the saved base outputs: largest {float(bnd['y'].max()):.2e}")
    assert ratio <= 1.0, ("eval y from the saved base outputs", ratio, where)
