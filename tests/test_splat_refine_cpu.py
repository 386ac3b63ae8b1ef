"""Splat refinement without a GPU: the functional restatement (splat_refine_functional.py) against the reference's own after_train /
refinement_after recorded in tests/golden/splat_refine_cases.npz, the configuration defaults, and the host-side argument checks of the
refinement entry points."""
import ctypes as C
import dataclasses
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import _lib
from nerfstudio_thermal_amd.splat import ThermalSplatfactoModelConfig

import splat_refine_functional as rf

EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "splat_refine_cases.npz")
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _cfg():
    return ThermalSplatfactoModelConfig(sh_degree=1)


def _t(a):
    return torch.from_numpy(np.asarray(a))


def test_config_defaults_are_the_reference_ones(gold):
    ref = json.loads(str(gold["config_defaults"]))
    mine = dataclasses.asdict(ThermalSplatfactoModelConfig())
    for k, v in ref.items():
        assert mine[k] == v, k


def test_after_train_statistics_match_the_reference(gold):
    cfg = _cfg()
    size = tuple(int(x) for x in gold["size"])
    checked = 0
    for case in gold["cases"]:
        pre = f"{case}__"
        stats = None
        for f in range(int(gold[pre + "frames"])):
            stats = rf.after_train(stats, _t(gold[pre + f"frame{f}__xys_grad"]), _t(gold[pre + f"frame{f}__radii"]), size, int(gold[pre + "step"]), cfg)
            for s, t in zip(("grad_norm_sum", "vis_counts", "max_2d_size"), stats):
                assert torch.equal(t, _t(gold[pre + f"frame{f}__{s}"])), (case, f, s)
            checked += 1
            if f:  # invisible Gaussians kept their sums and counts
                inv = _t(gold[pre + f"frame{f}__radii"]) == 0
                assert inv.any()
                assert torch.equal(stats[1][inv], _t(gold[pre + f"frame{f - 1}__vis_counts"])[inv])
    assert checked >= 10


@pytest.mark.parametrize("case", ["warmup", "densify", "huge", "late", "cull_only", "reset"])
def test_refinement_matches_the_reference(gold, case):
    cfg = _cfg()
    size = tuple(int(x) for x in gold["size"])
    pre = f"{case}__"
    step = int(gold[pre + "step"])
    stats = None
    for f in range(int(gold[pre + "frames"])):
        stats = rf.after_train(stats, _t(gold[pre + f"frame{f}__xys_grad"]), _t(gold[pre + f"frame{f}__radii"]), size, step, cfg)
    params = {k: _t(gold[pre + "in__" + k]) for k in NAMES}
    moments = {k: (_t(gold[pre + "m1_in__" + k]), _t(gold[pre + "m2_in__" + k])) for k in NAMES}
    noise = _t(gold[pre + "noise"])

    def draw(n):
        assert n == noise.shape[0]
        return noise

    out, mom, info = rf.refine(params, moments, stats, size, step, cfg, int(gold["num_train_data"]), draw)
    for k in NAMES:
        ref = _t(gold[pre + "out__" + k])
        assert out[k].shape == ref.shape, (k, out[k].shape, ref.shape)
        if k in ("means", "scales"):  # 1e-6 relative to the tensor's scale (a child mean near 0 carries the offset's absolute error)
            torch.testing.assert_close(out[k], ref, rtol=1e-6, atol=1e-6 * float(ref.abs().max()))
        else:
            assert torch.equal(out[k], ref), k
        assert torch.equal(mom[k][0], _t(gold[pre + "m1_out__" + k])), k
        assert torch.equal(mom[k][1], _t(gold[pre + "m2_out__" + k])), k
        assert float(gold[pre + "adam_step_out__" + k]) == float(gold[pre + "adam_step_in__" + k])
    n_in, n_out = params["means"].shape[0], out["means"].shape[0]
    if case == "warmup":
        assert info is None and n_out == n_in
    if case in ("densify", "huge", "late"):
        assert info["num_split"] > 0 and info["num_dup"] > 0 and bool(info["culled"].any())
        assert bool((info["split"] & info["dup"]).any())  # the split-and-duplicate quirk is covered
    if case == "cull_only":
        assert not info["densify"] and n_out < n_in
    if case == "reset":
        assert info["reset"] and n_out == n_in and bool((out["opacities"] < params["opacities"]).any())


def test_refine_workspace_size(lib):
    assert lib.tn_splat_refine_workspace_bytes(-1, 2) == -1
    assert lib.tn_splat_refine_workspace_bytes(10, 0) == -1
    assert lib.tn_splat_refine_workspace_bytes(10, 17) == -1
    small, big = lib.tn_splat_refine_workspace_bytes(1000, 2), lib.tn_splat_refine_workspace_bytes(2000, 2)
    assert 0 < small < big and big - small >= 1000 * (2 * 16 + 4 * 8) - 1024  # two 4-counter records + a 4-row map per Gaussian (256-byte aligned)
    assert lib.tn_splat_refine_workspace_bytes(0, 2) > 0


def _refine_struct(**kw):
    r = _lib.TnSplatRefine()
    cfg = ThermalSplatfactoModelConfig()
    for f, _ in r._fields_:
        if hasattr(cfg, f):
            setattr(r, f, getattr(cfg, f))
    r.max_size = 64
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_grad_stats_argument_validation(lib):
    d = C.c_void_p(256)  # never dereferenced: every call below is refused before anything is read or launched
    assert lib.tn_splat_grad_stats(d, d, -1, 64, 1, d, d, d, None) == EINVAL
    assert lib.tn_splat_grad_stats(d, d, 10, 0, 1, d, d, d, None) == EINVAL
    assert lib.tn_splat_grad_stats(d, None, 10, 64, 1, d, d, d, None) == EINVAL
    assert b"null pointer" in lib.tn_last_error()
    assert lib.tn_splat_grad_stats(d, d, 10, 64, 0, d, d, None, None) == EINVAL
    assert lib.tn_splat_grad_stats(None, None, 0, 64, 1, None, None, None, None) == 0  # N = 0: nothing to do, nothing launched


def test_refine_plan_argument_validation(lib):
    d = C.c_void_p(256)
    counts = (C.c_int64 * 4)()
    need = lib.tn_splat_refine_workspace_bytes(10, 2)

    def call(rs=None, step=600, n=10, ws_bytes=need, scales=d, out=counts):
        rs = rs or _refine_struct()
        return lib.tn_splat_refine_plan(C.byref(rs), step, scales, d, None, d, d, d, n, d, ws_bytes, out, None)

    assert lib.tn_splat_refine_plan(None, 600, d, d, None, d, d, d, 10, d, need, counts, None) == EINVAL
    assert call(n=-1) == EINVAL
    assert call(step=-1) == EINVAL
    assert call(rs=_refine_struct(refine_every=0)) == EINVAL
    assert call(rs=_refine_struct(n_split_samples=0)) == EINVAL
    assert call(rs=_refine_struct(max_size=0)) == EINVAL
    assert call(scales=None) == EINVAL
    assert b"null pointer" in lib.tn_last_error()
    assert call(out=None) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL
    assert b"workspace" in lib.tn_last_error()
    # nothing launched when there is nothing to refine: N = 0, or a step that neither densifies nor culls (counts = identity)
    assert call(n=0, scales=None) == 0 and list(counts) == [0, 0, 0, 0]
    assert call(step=3100, scales=None, ws_bytes=0) == 0 and list(counts) == [0, 10, 0, 0]


def test_refine_apply_argument_validation(lib):
    d = C.c_void_p(256)
    need = lib.tn_splat_refine_workspace_bytes(10, 2)
    ptrs = (C.c_void_p * 8)(*([256] * 8))
    nulls = (C.c_void_p * 8)()
    half = (C.c_void_p * 8)(*([256] * 4 + [None] * 4))

    def call(n=10, K=3, ws_bytes=need, counts=(2, 7, 4, 1), noise=d, params=ptrs, m1=ptrs, m2=ptrs, new_m1=ptrs, rs=None):
        rs = rs or _refine_struct()
        return lib.tn_splat_refine_apply(C.byref(rs), n, K, d, ws_bytes, (C.c_int64 * 4)(*counts), noise, 8, params, m1, m2, ptrs, new_m1, ptrs, None)

    assert call(n=-1) == EINVAL
    assert call(K=16) == EINVAL
    assert call(counts=(2, 11, 4, 1)) == EINVAL  # more survivors than Gaussians
    assert call(counts=(2, 7, 5, 1)) == EINVAL  # children not a multiple of n_split_samples
    assert call(counts=(-1, 7, 0, 1)) == EINVAL
    assert b"not a plan" in lib.tn_last_error()
    assert call(ws_bytes=need - 1) == EINVAL
    assert b"workspace" in lib.tn_last_error()
    assert call(noise=None) == EINVAL
    assert call(params=nulls) == EINVAL
    assert call(m1=half) == EINVAL  # a parameter's moments must be all set or all null
    assert b"partly null" in lib.tn_last_error()
    assert call(rs=_refine_struct(n_split_samples=17)) == EINVAL
    assert call(counts=(0, 0, 0, 0), params=nulls) == 0  # everything culled: nothing written, nothing launched


def test_refine_struct_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    hdr = os.path.join(ROOT, "include", "thermal_nerf_hip.h")
    names = [f[0] for f in _lib.TnSplatRefine._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n  printf("%%zu\\n", sizeof(TnSplatRefine));\n%s  return 0;\n}\n'
                   % (hdr, "".join('  printf("%s %%zu\\n", offsetof(TnSplatRefine, %s));\n' % (n, n) for n in names)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(_lib.TnSplatRefine)
    assert {ln.split()[0]: int(ln.split()[1]) for ln in out[1:] if ln} == {n: getattr(_lib.TnSplatRefine, n).offset for n in names}
    text = open(hdr).read()
    body = re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct TnSplatRefine {"):text.index("} TnSplatRefine;")], flags=re.S)
    assert set(re.findall(r"(\w+);", body)) == set(names)
