"""The scenes of the splat forward parity tests, checked on the two references alone (no GPU): tests/splat_functional.py in float64 against
the float32 oracle oracle/splat_oracle.py.  Every case is built to reach one thing the HIP forward does on top of the published algorithm
(tight tile box, quadrant cull, exponent skip, early exits around the prefetch of the next 256-record batch); the tests here assert that the
scene still HAS that property, that few enough pixels and Gaussians sit on a discrete decision (`flag_tol` = 1e-4, as in the backward
tests), and that the float32 restatement agrees with float64 no worse than the recorded FLOOR.  tests/test_splat_forward_gpu.py imports
CASES, CONFIGS, FLOOR and the helpers: its tolerances are 8 x FLOOR and nothing else.

FLOOR holds, per case, configuration ("<raster mode>-<SH degree>", degree 0 = sigmoid colours) and output, the float32-vs-float64 error measured
on an x86-64 host and rounded UP to one significant digit: the float32 oracle's last bits differ between hosts (profiles/r06_sampler_ulps.md
found that for the sampler), so the recorded value is a ceiling of the measurement, not the measurement.  rgb / thermal / accumulation:
max-abs; T: max relative error of 1 - accumulation where the float64 T > 2e-4; depth: max relative error where accumulation > 1e-3;
depth_fill: relative error of the fill value; xys / depths / conics / compensation: max of |a - b| / (|b| + 1) over the Gaussians both
references keep.  All on pixels the float64 walk does not flag."""
import functools
import math

import pytest
import torch

import splat_functional as sf
import splat_oracle as so

BG_RGB, BG_THERMAL = (0.2, 0.5, 0.9), 0.3
FLAG_TOL = 1e-4
MAX_FLAGGED_PIXELS, MAX_FLAGGED_GAUSSIANS = 0.10, 0.20  # conditions on the scenes, not measurements
IMAGE_OUTPUTS = ("rgb", "thermal", "accumulation", "T", "depth", "depth_fill")
PROJECTION_OUTPUTS = ("xys", "depths", "conics", "compensation")


def _with(p, **kw):
    p = dict(p)
    p.update(kw)
    return p


def _ragged(deg, num=1500):
    return sf.scene(num, 21, deg, scale_range=(-4.0, -2.6))


def _sliver(deg):
    return sf.scene(300, 22, deg, extent=0.5, scale_range=(-3.0, -2.0))


def _subtile(deg):
    return sf.scene(200, 23, deg, extent=0.4, scale_range=(-3.0, -2.0))


def _deep(deg, num=2500, extent=0.6):
    p = sf.scene(num, 24, deg, extent=extent, scale_range=(-2.2, -1.4))
    g = torch.Generator().manual_seed(24)
    return _with(p, opacities=torch.rand(p["opacities"].shape, generator=g) * 1.0 - 4.8)  # sigmoid: 0.008 .. 0.022, all above 1/255


def _opaque(deg, num=4500):
    p = sf.scene(num, 21, deg, extent=0.6, scale_range=(-2.6, -1.6))
    return _with(p, opacities=p["opacities"] * 0.0 + 3.0)


def _faint(deg):
    p = sf.scene(800, 25, deg, extent=0.8, scale_range=(-2.8, -1.8))
    g = torch.Generator().manual_seed(25)
    op = p["opacities"].clone()
    op[:500] = torch.rand((500, 1), generator=g) * 3.5 - 7.5  # logit(1/255) = -5.54: sigmoid from 5.5e-4 to 1.8e-2
    return _with(p, opacities=op)


def _huge(deg):
    p = sf.scene(500, 26, deg, extent=0.8)
    sc, mu, op = p["scales"].clone(), p["means"].clone(), p["opacities"].clone()
    sc[:6] = torch.tensor([-0.3, -0.1, 0.1])  # standard deviations of about one scene extent: the 3-sigma box covers the image
    mu[:6] = mu[:6] * 0.3
    op[:6] = torch.tensor([[-1.5], [-0.5], [0.5], [-3.0], [1.5], [-2.0]])
    return _with(p, scales=sc, means=mu, opacities=op)


TIE_PAIRS = 50


def _ties(deg):
    """Gaussians 0..49 and 50..99 share their means bit for bit (so depth and centre too); every other parameter differs."""
    p = sf.scene(300, 27, deg, extent=0.7, scale_range=(-3.2, -2.4))
    mu = p["means"].clone()
    mu[TIE_PAIRS:2 * TIE_PAIRS] = mu[:TIE_PAIRS]
    return _with(p, means=mu)


def swap_ties(p):
    """The same Gaussians with the members of every pair in the other order."""
    perm = torch.arange(p["means"].shape[0])
    perm[:TIE_PAIRS], perm[TIE_PAIRS:2 * TIE_PAIRS] = torch.arange(TIE_PAIRS, 2 * TIE_PAIRS), torch.arange(TIE_PAIRS)
    return {k: v[perm].contiguous() for k, v in p.items()}


# name -> (scene, W, H, fov in degrees (of W), (cx, cy), eye)
CASES = {
    "ragged": (_ragged, 150, 101, 60.0, (77.3, 48.9), (2.6, 0.4, 0.9)),
    "sliver": (_sliver, 17, 33, 40.0, (8.0, 17.2), (2.2, -0.3, 0.5)),
    "subtile": (_subtile, 13, 7, 30.0, (6.2, 3.7), (2.4, 0.2, 0.3)),
    "deep": (_deep, 64, 48, 50.0, (31.5, 24.5), (2.3, 0.3, 0.6)),
    "opaque": (_opaque, 75, 53, 60.0, (37.0, 27.0), (2.6, 0.4, 0.9)),
    "faint": (_faint, 64, 48, 60.0, (32.5, 23.0), (2.4, -0.4, 0.7)),
    "huge": (_huge, 64, 48, 60.0, (31.0, 24.5), (2.5, 0.5, 0.5)),
    "ties": (_ties, 64, 48, 60.0, (32.0, 24.0), (2.3, 0.2, 0.8)),
}
MODES = ("classic", "antialiased")
# (case, raster mode, SH degree): every case in both modes at degree 3; `ragged` also with sigmoid colours (0) and degree 1
CONFIGS = [(c, m, d) for c in CASES for m in MODES for d in ((0, 1, 3) if c == "ragged" else (3,))]

# float32 oracle vs float64 restatement, measured and rounded up to one significant digit (see the module docstring)
FLOOR = {
    "ragged": {
        "classic-0": {"rgb": 3e-06, "thermal": 2e-06, "accumulation": 3e-06, "T": 0.0002, "depth": 7e-06, "depth_fill": 9e-08, "xys": 7e-06, "depths": 7e-08, "conics": 3e-07, "compensation": 1e-07},
        "classic-1": {"rgb": 3e-06, "thermal": 2e-06, "accumulation": 3e-06, "T": 0.0002, "depth": 7e-06, "depth_fill": 9e-08, "xys": 7e-06, "depths": 7e-08, "conics": 3e-07, "compensation": 1e-07},
        "classic-3": {"rgb": 3e-06, "thermal": 3e-06, "accumulation": 3e-06, "T": 0.0002, "depth": 7e-06, "depth_fill": 9e-08, "xys": 7e-06, "depths": 7e-08, "conics": 3e-07, "compensation": 1e-07},
        "antialiased-0": {"rgb": 2e-06, "thermal": 2e-06, "accumulation": 3e-06, "T": 0.0002, "depth": 9e-06, "depth_fill": 9e-08, "xys": 7e-06, "depths": 7e-08, "conics": 3e-07, "compensation": 1e-07},
        "antialiased-1": {"rgb": 3e-06, "thermal": 2e-06, "accumulation": 3e-06, "T": 0.0002, "depth": 9e-06, "depth_fill": 9e-08, "xys": 7e-06, "depths": 7e-08, "conics": 3e-07, "compensation": 1e-07},
        "antialiased-3": {"rgb": 3e-06, "thermal": 3e-06, "accumulation": 3e-06, "T": 0.0002, "depth": 9e-06, "depth_fill": 9e-08, "xys": 7e-06, "depths": 7e-08, "conics": 3e-07, "compensation": 1e-07},
    },
    "sliver": {
        "classic-3": {"rgb": 5e-07, "thermal": 5e-07, "accumulation": 6e-07, "T": 0.0002, "depth": 5e-06, "depth_fill": 2e-08, "xys": 2e-07, "depths": 5e-08, "conics": 3e-07, "compensation": 1e-07},
        "antialiased-3": {"rgb": 5e-07, "thermal": 5e-07, "accumulation": 6e-07, "T": 9e-05, "depth": 6e-06, "depth_fill": 2e-08, "xys": 2e-07, "depths": 5e-08, "conics": 3e-07, "compensation": 1e-07},
    },
    "subtile": {
        "classic-3": {"rgb": 3e-07, "thermal": 4e-07, "accumulation": 4e-07, "T": 0.0002, "depth": 2e-06, "depth_fill": 0, "xys": 4e-07, "depths": 6e-08, "conics": 4e-07, "compensation": 9e-08},
        "antialiased-3": {"rgb": 4e-07, "thermal": 3e-07, "accumulation": 3e-07, "T": 0.0001, "depth": 6e-06, "depth_fill": 0, "xys": 4e-07, "depths": 6e-08, "conics": 4e-07, "compensation": 9e-08},
    },
    "deep": {
        "classic-3": {"rgb": 1e-05, "thermal": 4e-06, "accumulation": 5e-07, "T": 3e-06, "depth": 8e-06, "depth_fill": 2e-07, "xys": 5e-07, "depths": 5e-08, "conics": 1e-07, "compensation": 7e-08},
        "antialiased-3": {"rgb": 9e-06, "thermal": 4e-06, "accumulation": 5e-07, "T": 3e-06, "depth": 8e-06, "depth_fill": 2e-07, "xys": 5e-07, "depths": 5e-08, "conics": 1e-07, "compensation": 7e-08},
    },
    "opaque": {
        "classic-3": {"rgb": 8e-07, "thermal": 6e-07, "accumulation": 6e-07, "T": 0.0002, "depth": 8e-06, "depth_fill": 2e-07, "xys": 2e-07, "depths": 6e-08, "conics": 2e-07, "compensation": 7e-08},
        "antialiased-3": {"rgb": 7e-07, "thermal": 5e-07, "accumulation": 7e-07, "T": 0.0002, "depth": 7e-06, "depth_fill": 2e-07, "xys": 2e-07, "depths": 6e-08, "conics": 2e-07, "compensation": 7e-08},
    },
    "faint": {
        "classic-3": {"rgb": 5e-07, "thermal": 4e-07, "accumulation": 5e-07, "T": 0.0002, "depth": 6e-06, "depth_fill": 3e-08, "xys": 4e-07, "depths": 5e-08, "conics": 3e-07, "compensation": 8e-08},
        "antialiased-3": {"rgb": 5e-07, "thermal": 4e-07, "accumulation": 5e-07, "T": 0.0002, "depth": 8e-06, "depth_fill": 3e-08, "xys": 4e-07, "depths": 5e-08, "conics": 3e-07, "compensation": 8e-08},
    },
    "huge": {
        "classic-3": {"rgb": 9e-07, "thermal": 8e-07, "accumulation": 6e-07, "T": 0.0002, "depth": 7e-07, "depth_fill": 0, "xys": 5e-07, "depths": 5e-08, "conics": 3e-07, "compensation": 9e-08},
        "antialiased-3": {"rgb": 7e-07, "thermal": 7e-07, "accumulation": 5e-07, "T": 0.0002, "depth": 7e-07, "depth_fill": 0, "xys": 5e-07, "depths": 5e-08, "conics": 3e-07, "compensation": 9e-08},
    },
    "ties": {
        "classic-3": {"rgb": 9e-07, "thermal": 6e-07, "accumulation": 9e-07, "T": 0.0001, "depth": 6e-06, "depth_fill": 2e-07, "xys": 3e-07, "depths": 5e-08, "conics": 3e-07, "compensation": 9e-08},
        "antialiased-3": {"rgb": 7e-07, "thermal": 5e-07, "accumulation": 9e-07, "T": 5e-05, "depth": 7e-06, "depth_fill": 2e-07, "xys": 3e-07, "depths": 5e-08, "conics": 3e-07, "compensation": 9e-08},
    },
}


def config_id(mode, deg):
    return f"{mode}-{deg}"


def case_scene(case, deg):
    return CASES[case][0](deg)


def case_camera(case, cases=None):
    """c2w, fx, fy, cx, cy, W, H of a row of `cases` (default: CASES)"""
    _, W, H, fov, (cx, cy), eye = (CASES if cases is None else cases)[case]
    fx = sf.fov_focal(W, fov)
    return so.look_at_camera(eye), fx, fx * 0.97, cx, cy, W, H


def background():
    """The background as the model hands it to the kernel: float32 values (the float64 reference gets the same numbers)."""
    return torch.tensor(BG_RGB, dtype=torch.float32), float(torch.tensor(BG_THERMAL, dtype=torch.float32))


def reference64(p, case, mode, deg):
    c2w, fx, fy, cx, cy, W, H = case_camera(case)
    bg, bgt = background()
    with torch.no_grad():
        return sf.render({k: v.double() for k, v in p.items()}, c2w, fx, fy, cx, cy, W, H, sh_degree_to_use=deg if deg > 0 else -1, rasterize_mode=mode,
                         background=bg, background_thermal=bgt, flag_tol=FLAG_TOL, with_depth=True)


def reference32(p, case, mode, deg):
    c2w, fx, fy, cx, cy, W, H = case_camera(case)
    bg, bgt = background()
    with torch.no_grad():
        return so.render(p, c2w, fx, fy, cx, cy, W, H, sh_degree_to_use=deg if deg > 0 else -1, rasterize_mode=mode, background=bg, background_thermal=bgt)


@functools.lru_cache(maxsize=None)
def references(case, mode, deg):
    p = case_scene(case, deg)
    return p, reference64(p, case, mode, deg), reference32(p, case, mode, deg)


def image_errors(ref, out, fill):
    """Errors of float32 images `out` (rgb, thermal, accumulation, depth: [H,W,C]) and of the depth fill value `fill` (or None: not
    observable) against the float64 render `ref`, on the pixels `ref` does not flag.  Keys: IMAGE_OUTPUTS, plus `zero_mismatch`: pixels
    without any contribution in the reference whose accumulation is not exactly 0."""
    keep = ~ref["flag_pixels"]
    acc = ref["accumulation"][..., 0]
    o = {k: out[k].detach().cpu().double() for k in ("rgb", "thermal", "accumulation", "depth")}
    e = {k: float((o[k] - ref[k]).abs()[keep].max()) for k in ("rgb", "thermal", "accumulation")}
    T_ref, T_out = 1.0 - acc, 1.0 - o["accumulation"][..., 0]
    sel = keep & (T_ref > 2e-4)
    e["T"] = float(((T_out - T_ref).abs() / T_ref)[sel].max()) if bool(sel.any()) else 0.0
    sel = keep & (acc > 1e-3)
    d_ref, d_out = ref["depth"][..., 0], o["depth"][..., 0]
    e["depth"] = float(((d_out - d_ref).abs() / d_ref.abs())[sel].max()) if bool(sel.any()) else 0.0
    fill_ref = float(ref["depth_fill"])
    e["depth_fill"] = abs(float(fill) - fill_ref) / abs(fill_ref) if fill is not None else 0.0
    e["zero_mismatch"] = int((keep & (acc == 0) & (o["accumulation"][..., 0] != 0)).sum())
    return e


def projection_errors(ref, pj):
    """|a - b| / (|b| + 1) of xys, depths, conics, compensation over the Gaussians visible in both."""
    rp = ref["projection"]
    both = rp["ok"] & (pj["radii"].cpu() > 0)
    e = {}
    for k in PROJECTION_OUTPUTS:
        a, b = pj[k].detach().cpu().double()[both], rp[k][both]
        e[k] = float(((a - b).abs() / (b.abs() + 1.0)).max()) if bool(both.any()) else 0.0
    return e


def radius_exceptions(ref):
    """Gaussians whose integer radius / tile count may legitimately differ from the float64 one: on the frustum clamp, or with the float64
    3 sqrt(lambda_max) within 1e-4 of an integer."""
    c = ref["projection"]["conics"]
    det = c[:, 0] * c[:, 2] - c[:, 1] * c[:, 1]  # cov2d = conic^-1
    a, cc, det_cov = c[:, 2] / det, c[:, 0] / det, 1.0 / det
    mid = 0.5 * (a + cc)
    r = 3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp(mid * mid - det_cov, min=0.1)))
    knife = (r - torch.round(r)).abs() < 1e-4
    return ref["projection"]["near_clamp"] | (knife & ref["projection"]["ok"])


def oracle_fill(ref32):
    """The float32 oracle's fill value: the maximum of its un-normalised depth image = max(depth * accumulation) over hit pixels, which its
    `depth` no longer holds; an empty pixel shows it directly."""
    acc = ref32["accumulation"]
    empty = acc == 0
    if bool(empty.any()):
        return float(ref32["depth"][empty][0])
    return None


def measured_floor(case, mode, deg):
    _, r64, r32 = references(case, mode, deg)
    e = image_errors(r64, r32, oracle_fill(r32))
    e.update(projection_errors(r64, r32["projection"]))
    return e


def scene_stats(case, mode, deg):
    _, r64, _ = references(case, mode, deg)
    vis = r64["projection"]["ok"]
    return {"flagged_pixels": float(r64["flag_pixels"].float().mean()), "flagged_gaussians": float((r64["flag_gaussians"] & vis).sum()) / max(int(vis.sum()), 1),
            "visible": int(vis.sum()), "contributors_max": int(r64["contributors_per_tile"].max()), "stopped_fraction": r64["stopped_fraction"],
            "pairs": int(r64["pair_used"].sum())}


def quadrant_mix(stopped):
    """True when some 8x8 quadrant of some tile holds a stopped and a running pixel."""
    H, W = stopped.shape
    ph, pw = -H % 16, -W % 16
    inside = torch.nn.functional.pad(torch.ones(H, W, dtype=torch.bool), (0, pw, 0, ph))
    st = torch.nn.functional.pad(stopped, (0, pw, 0, ph))
    q = lambda m: m.view((H + ph) // 8, 8, (W + pw) // 8, 8).any(3).any(1)  # noqa: E731
    return bool((q(st) & q(inside & ~st)).any())


@pytest.mark.parametrize("case,mode,deg", CONFIGS)
def test_scene_keeps_its_property(case, mode, deg):
    p, r64, _ = references(case, mode, deg)
    _, W, H, _, _, _ = CASES[case]
    pj = r64["projection"]
    ok, acc = pj["ok"], r64["accumulation"][..., 0]
    tbx, tby = (W + 15) // 16, (H + 15) // 16
    assert max(W, H) <= 150 and p["means"].shape[0] <= 6000
    if case == "ragged":
        assert W % 16 != 0 and H % 16 != 0
        tc, tr = pj["xys"] / 16.0, pj["radii"].double() / 16.0
        for name, hit in (("left", tc[:, 0] - tr < 0), ("right", tc[:, 0] + tr + 1 > tbx), ("top", tc[:, 1] - tr < 0), ("bottom", tc[:, 1] + tr + 1 > tby)):
            assert bool((ok & hit).any()), name
    elif case == "sliver":
        assert W == 17 and float(acc[:, 16].max()) > 0.01
    elif case == "subtile":
        assert tbx * tby == 1 and float(acc.max()) > 0.5
    elif case == "deep":
        assert max(W, H) <= 96 and int(r64["contributors_per_tile"].max()) >= 3 * 256 and r64["stopped_fraction"] <= 0.2
    elif case == "opaque":
        assert max(W, H) <= 96 and 0.3 <= r64["stopped_fraction"] <= 0.9 and quadrant_mix(r64["stopped"])
    elif case == "faint":
        op = torch.sigmoid(p["opacities"][:, 0])[ok]
        assert float((op < 1.0 / 255.0).float().mean()) >= 0.2 and float((op > 1.0 / 255.0).float().mean()) >= 0.2
    elif case == "huge":
        full = ok & (pj["tile_min"] == 0).all(-1) & (pj["tile_max"] == torch.tensor([tbx, tby])).all(-1)
        assert bool(full.any()) and int(full.sum()) < 0.1 * int(ok.sum())
    elif case == "ties":
        d = pj["depths"]
        assert torch.equal(d[:TIE_PAIRS], d[TIE_PAIRS:2 * TIE_PAIRS]) and int(ok[:TIE_PAIRS].sum()) >= 40
        swapped = reference64(swap_ties(p), case, mode, deg)
        keep = ~(r64["flag_pixels"] | swapped["flag_pixels"])
        assert float((swapped["rgb"] - r64["rgb"]).abs()[keep].max()) > 1e-3  # the order inside a pair is observable


@pytest.mark.parametrize("case,mode,deg", CONFIGS)
def test_few_decisions_are_near_a_threshold(case, mode, deg):
    s = scene_stats(case, mode, deg)
    print(f"{case} {config_id(mode, deg)}: {s}")
    assert s["flagged_pixels"] <= MAX_FLAGGED_PIXELS, s
    assert s["flagged_gaussians"] <= MAX_FLAGGED_GAUSSIANS, s


@pytest.mark.parametrize("case,mode,deg", CONFIGS)
def test_float32_oracle_stays_within_the_recorded_floor(case, mode, deg):
    e = measured_floor(case, mode, deg)
    print(f"{case} {config_id(mode, deg)}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e.pop("zero_mismatch") == 0
    rec = FLOOR[case][config_id(mode, deg)]
    assert set(rec) == set(IMAGE_OUTPUTS + PROJECTION_OUTPUTS)
    for k, v in e.items():
        assert v <= rec[k], (k, v, rec[k])
    # integers of the projection: equal except on the knife edges
    _, r64, r32 = references(case, mode, deg)
    exc = radius_exceptions(r64)
    assert int(exc.sum()) <= 0.01 * exc.numel()
    assert torch.equal(r32["projection"]["radii"][~exc], r64["projection"]["radii"][~exc])


def test_floors_leave_room_under_the_ceilings():
    """8 x the image floors stays under the 1e-4 ceiling of the GPU test (a scene whose float32 noise comes near a lost blend is too hard for
    the method).  The T floor is the quantisation of 1 - T in float32 -- half an ulp of a number near 1, 3e-8, over T >= 2e-4: 1.5e-4 -- wherever
    a pixel ends just above the stop; there the GPU test's 1e-3 ceiling binds instead of 8 x FLOOR, which only makes it stricter."""
    for case, rows in FLOOR.items():
        for cid, rec in rows.items():
            for k in ("rgb", "thermal", "accumulation"):
                assert 8 * rec[k] < 1e-4, (case, cid, k)
            assert rec["T"] <= 2e-4, (case, cid)
    assert math.isclose(2.0 ** -25 / 2e-4, 1.5e-4, rel_tol=0.01)
