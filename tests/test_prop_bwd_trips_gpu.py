"""k_prop_bwd_mlp (the MLP launch of tn_prop_density_bwd) where a wave makes a second trip: the next trip's inputs are requested before this
trip's MFMAs and the wave's LDS rows are reused behind a wave barrier, which happens only beyond 256 * 1024 points (256 blocks of 16 waves, 64
samples per wave and trip).  Level 0 of the tiny configuration:
  two_trips_partial_end  N = 1029, S = 255: P = 262395 = 256 * 1024 + 251 -- waves 0..3 of block 0 make a prefetched second trip and the
                         fourth of them ends with 59 live lanes;
  one_trip_and_a_lane    N = 5, S = 13: P = 65 -- one full trip and a wave with one live lane.

Reference: the 10 -> 16 -> 1 MLP restated in float64, forward and backward (trunc_exp backward exp(clamp(out, -15, 15))), fed with the oracle's
fp32 hash encoding, as tests/test_field_bwd_tiles_gpu.py does for the main field.
  w0, b0, w1, b1 gradients: 2e-4 of each tensor's largest entry (the bound of test_prop_density_fwd_bwd).
  d enc (the first 10 P floats of the workspace, level-major [5][P] float2), row by row.  Rows whose float64 pre-activations come within 1e-6 of
  a ReLU kink are left out: a condition on the inputs, capped at 2e-4 of the rows (measured on the CPU: 17 of 262395 rows, 6.5e-5).  Per entry
  the bound is C u sum_j |d_out w1_j w0_jk| with u = 2^-24.  C is not taken from the kernel: the same formulas are evaluated in torch float32
  on the CPU against the float64 restatement, the worst ratio over the case is taken (measured: 2.5 to 3.1 at P = 262395 depending on the summation order of the host's BLAS, 1.75 at P = 65: C = 10 to 12.6 and 7.0; the kernel itself comes to 2.5 and 0.9) and given
  a factor 4 for the MFMA's four-term k-steps and expf.
  The workspace is NaN before the call: every output must be finite, and the floats between the 10 P of d enc and the scatter's scratch must
  still be NaN.  Two runs give the same d enc bit for bit (no sum across lanes that depends on timing).
The saved_enc instantiation is reachable only through the one-call training entry points and is not covered here."""
import pytest
import torch

import thermal_nerfacto_oracle as orc
from helpers import make_params, tiny_cfg, SEED
from nerfstudio_thermal_amd import ops, synth
from nerfstudio_thermal_amd.arena import ParamArena
from nerfstudio_thermal_amd.config import ThermalNerfactoModelConfig
from nerfstudio_thermal_amd.netparams import prop_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
TOL = 2e-4  # tests/test_hip_ops_gpu.py::test_prop_density_fwd_bwd
KINK, MAX_KINK_ROWS = 1e-6, 2e-4
MARGIN = 4.0
SHAPES = {"two_trips_partial_end": (1029, 255), "one_trip_and_a_lane": (5, 13)}
GRADS = ("w0", "b0", "w1", "b1")
LVL = 0


def mlp_restatement(enc, W0, b0, w1, b1, g_dens, sel):
    """forward and backward of the proposal MLP in the dtype of its arguments -> (gradients, d enc [P, 10], pre-activations, d_out)"""
    a = enc @ W0.T + b0
    h = a.clamp_min(0)
    out = h @ w1.T + b1  # [P, 1]
    d_out = g_dens * torch.exp(out[:, 0].clamp(-15, 15)) * sel
    da = d_out[:, None] * w1 * (a > 0)
    grads = {"w0": da.T @ enc, "b0": da.sum(0), "w1": (d_out[:, None] * h).sum(0, keepdim=True), "b1": d_out.sum().reshape(1)}
    return grads, da @ W0, a, d_out


_CASES = {}


def _case(name):
    if name in _CASES:
        return _CASES[name]
    N, S = SHAPES[name]
    P = N * S
    ocfg = tiny_cfg("shared")
    params = make_params(ocfg)
    cfg = ThermalNerfactoModelConfig(density_mode="shared", log2_hashmap_size=ocfg.log2_hashmap_size)
    for a in cfg.proposal_net_args_list:
        a["log2_hashmap_size"] = ocfg.prop_log2_hashmap_size
    arena = ParamArena(cfg, ocfg.num_images, DEV)
    arena.load(params)
    net = prop_params(arena, "proposal_networks", LVL, cfg, with_grads=True)
    r = {kk: torch.from_numpy(v) for kk, v in synth.synth_rays_simple(N, 11).items()}
    s = orc.spaced_bins(N, S, None)
    e = orc.s_to_euclidean(s, torch.ones(N, 1) * 0.05, torch.ones(N, 1) * 1000.0).contiguous()
    k = orc.prop_keys("proposal_networks", LVL)
    with torch.no_grad():
        p, sel = orc.unit_cube_positions(orc.Samples(s_bins=s, e_bins=e).positions(r["origins"], r["directions"]))
        res = orc.level_resolutions(ocfg.prop_num_levels, ocfg.prop_base_res, ocfg.prop_max_res[LVL])
        enc = orc.hash_encode(p.view(-1, 3), params[k["table"]], res, ocfg.prop_log2_hashmap_size)  # fp32: what the kernel gathers
    g_dens = torch.from_numpy(synth.uniform("trips_gd_" + name, (P,), seed=SEED))
    args = lambda dt: (enc.to(dt), params[k["w0"]].to(dt), params[k["b0"]].to(dt), params[k["w1"]].to(dt), params[k["b1"]].to(dt),  # noqa: E731
                       g_dens.to(dt), sel.reshape(-1).to(dt))
    with torch.no_grad():
        ref, ref_denc, a64, d_out = mlp_restatement(*args(torch.float64))
        _, denc32, _, _ = mlp_restatement(*args(torch.float32))
    keep = a64.abs().min(dim=1).values >= KINK
    W0, w1 = params[k["w0"]].double(), params[k["w1"]].double()
    S_abs = d_out.abs()[:, None] * ((w1.abs().T * W0.abs()).sum(0))[None, :]  # [P, 10]: sum_j |d_out w1_j w0_jk|
    pos = keep[:, None] & (S_abs > 0)
    c_measured = float(((denc32.double() - ref_denc).abs()[pos] / (U * S_abs[pos])).max())
    g = lambda x: x.to(DEV).contiguous()  # noqa: E731
    o_d, d_d, e_d, gd_d = g(r["origins"]), g(r["directions"]), g(e), g(g_dens.view(N, S))
    ws = ops._prop_ws(o_d.device, P, "trips")
    gap = slice(10 * P, ((P * 64 + 1024 + 255) // 256) * 256 // 4)  # behind d enc, in front of the scatter's scratch (tn_prop.hip)
    runs = []
    for _ in range(2):
        ws.view(torch.float32).fill_(float("nan"))
        arena.zero_grad()
        ops.prop_density_bwd(net, o_d, d_d, e_d, gd_d, None, None, tag="trips")
        torch.cuda.synchronize()
        assert ops._prop_ws(o_d.device, P, "trips").data_ptr() == ws.data_ptr()
        wsf = ws.view(torch.float32)
        denc = wsf[: 10 * P].view(5, P, 2).permute(1, 0, 2).reshape(P, 10).cpu().clone()
        runs.append(dict(grads={sh: arena.grad_view(k[sh]).detach().cpu().clone() for sh in GRADS}, denc=denc,
                         table=arena.grad_view(k["table"]).detach().cpu().clone(), gap_untouched=bool(torch.isnan(wsf[gap]).all())))
    _CASES[name] = dict(ref=ref, ref_denc=ref_denc, keep=keep, S_abs=S_abs, c_measured=c_measured, runs=runs, P=P)
    return _CASES[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_weight_gradients_match_the_float64_restatement(name):
    c = _case(name)
    for sh in GRADS:
        ref, got = c["ref"][sh], c["runs"][0]["grads"][sh]
        scale = float(ref.abs().max())
        err = float((got.double().reshape(ref.shape) - ref).abs().max())
        print(f"{name} {sh}: err {err:.3e} scale {scale:.3e} ratio {err / scale:.2e}")
        assert torch.isfinite(got).all() and scale > 0
        assert err <= TOL * scale, (sh, err, scale)
    assert torch.isfinite(c["runs"][0]["table"]).all() and float(c["runs"][0]["table"].abs().max()) > 0


@pytest.mark.parametrize("name", list(SHAPES))
def test_d_enc_matches_the_float64_restatement_row_by_row(name):
    c = _case(name)
    denc, keep = c["runs"][0]["denc"], c["keep"]
    dropped = int((~keep).sum())
    C = MARGIN * c["c_measured"]
    print(f"{name}: {dropped} of {c['P']} rows within {KINK} of a ReLU kink; C measured in float32 on the CPU {c['c_measured']:.2f}, used {C:.2f}")
    assert dropped <= MAX_KINK_ROWS * c["P"]
    assert torch.isfinite(denc).all()
    err = (denc.double() - c["ref_denc"]).abs()
    bound = C * U * c["S_abs"]
    ratio = (err / (U * c["S_abs"]).clamp_min(1e-300))[keep]
    print(f"{name}: worst err / (u sum|.|) over the kept rows {float(ratio.max()):.2f}")
    assert bool((err[keep] <= bound[keep]).all()), float((err - bound)[keep].max())
    assert bool((denc[c["S_abs"] == 0] == 0).all())  # selector-masked and zero-gradient samples: exact zeros


@pytest.mark.parametrize("name", list(SHAPES))
def test_two_poisoned_runs_agree_and_leave_the_rest_of_the_workspace_alone(name):
    a, b = _case(name)["runs"]
    assert a["gap_untouched"] and b["gap_untouched"]
    assert torch.equal(a["denc"], b["denc"])
    for sh in GRADS:
        assert torch.isfinite(b["grads"][sh]).all(), sh
