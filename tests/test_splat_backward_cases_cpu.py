"""The scenes and references of the splat backward parity tests, checked without a GPU (tests/splat_backward_cases.py): every case still has
the property it was built for, no two visible depths are closer than float32 can order, few enough pixels and Gaussians sit on a discrete
decision, the float64 statement of the published backward walk IS the derivative (equal to float64 autograd to 1e-9), and the float32 floor
of every gradient -- the larger of float32 autograd's and the float32 walk's distance from float64 -- is at most 2e-5 of the gradient's
largest entry.  tests/test_splat_backward_cases_gpu.py allows the kernels 8 x that floor; a scene whose own float32 noise were larger would
hide a lost blend.  Every figure is printed before it is asserted; profiles/splat_backward_parity.md holds the measured ones."""
import pytest
import torch

import splat_backward_cases as bc
import test_splat_forward_cpu as fc

IDS = [bc.config_id(c) for c in bc.ALL_CONFIGS]


def _tiles(case):
    _, W, H = bc.case_camera(case)[4:]
    return W, H, (W + 15) // 16, (H + 15) // 16


def _tile_share(mask, ty, tx):
    """Share of the tile's pixels inside the image for which `mask` holds."""
    t = mask[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16]
    return float(t.float().mean())


@pytest.mark.parametrize("cfg", bc.CONFIGS, ids=IDS[:len(bc.CONFIGS)])
def test_case_keeps_its_property(cfg):
    case, mode, deg, _ = cfg
    ref = bc.reference(*cfg)
    p, st = ref["p"], ref["st"]
    W, H, tbx, tby = _tiles(case)
    pj = st["projection"]
    ok, acc, per_tile = pj["ok"], st["accumulation"][..., 0], st["contributors_per_tile"]
    print(f"{bc.config_id(cfg)}: contributors per tile {per_tile.flatten().tolist()}, stopped {st['stopped_fraction']:.3f}, visible {int(ok.sum())}")
    if case == "deep":
        assert any(n >= 3 * 256 and n % 256 != 0 for n in per_tile.flatten().tolist())
    elif case == "opaque":
        shares = {(ty, tx): _tile_share(st["stopped"], ty, tx) for ty in range(tby) for tx in range(tbx)}
        print("stopped share per tile: " + ", ".join(f"{k}: {v:.2f} ({int(per_tile[k])})" for k, v in shares.items()))
        assert any(int(per_tile[k]) > 256 and 0.1 < v < 0.95 for k, v in shares.items())
        assert any(v == 0.0 for v in shares.values())
        assert fc.quadrant_mix(st["stopped"])
    elif case == "ragged":
        assert W % 16 != 0 and H % 16 != 0
        tc, tr = pj["xys"] / 16.0, pj["radii"].double() / 16.0
        for name, hit in (("left", tc[:, 0] - tr < 0), ("right", tc[:, 0] + tr + 1 > tbx), ("top", tc[:, 1] - tr < 0), ("bottom", tc[:, 1] + tr + 1 > tby)):
            assert bool((ok & hit).any()), name
    elif case == "sliver":
        assert W == 17 and float(acc[:, 16].max()) > 0.01
    elif case == "subtile":
        assert tbx * tby == 1 and float(acc.max()) > 0.5
    elif case == "faint":
        op = torch.sigmoid(p["opacities"][:, 0])[ok]
        assert float((op < 1.0 / 255.0).float().mean()) >= 0.2 and float((op > 1.0 / 255.0).float().mean()) >= 0.2
    elif case == "huge":
        full = ok & (pj["tile_min"] == 0).all(-1) & (pj["tile_max"] == torch.tensor([tbx, tby])).all(-1)
        assert bool(full.any()) and int(full.sum()) < 0.1 * int(ok.sum())
    elif case == "ties":
        d, n = pj["depths"], fc.TIE_PAIRS
        assert torch.equal(p["means"][:n], p["means"][n:2 * n]) and torch.equal(d[:n], d[n:2 * n]) and int(ok[:n].sum()) >= 40
    elif case == "single":
        assert p["means"].shape[0] == 1 and tuple(per_tile.shape) == (2, 3) and int(per_tile.sum()) == 6  # N = 1, a run of 3 x 2 pairs
    elif case == "clamped":
        # unflagged pixels that blend on the 0.999 clamp (no geometry or opacity gradient from that blend) and go on behind it
        pjd, fw = bc.walk_stats(p, case, mode, deg)
        n, inner = (t * ~st["flag_pixels"] for t in bc.clamped_blends(pjd, fw, pjd["op"], H, W))
        behind = inner > 0
        print(f"pixels with a blend on the clamp: {int((n > 0).sum())}, of them with a contributor behind it: {int(behind.sum())}")
        assert int((n > 0).sum()) >= 10 and int(behind.sum()) >= 10


@pytest.mark.parametrize("cfg", bc.SEP_CONFIGS, ids=IDS[len(bc.CONFIGS):])
def test_separate_case_keeps_its_property(cfg):
    case, mode, deg, sep = cfg
    ref = bc.reference(*cfg)
    p, st = ref["p"], ref["st"]
    per_tile = st["contributors_per_tile"]
    a, b = st["stopped"], st["stopped_thermal"]
    only_rgb, only_th = float((a & ~b).float().mean()), float((b & ~a).float().mean())
    _, rgb = bc.walk_stats(p, case, mode, deg, sep, "op")
    _, th = bc.walk_stats(p, case, mode, deg, sep, "op_t")
    one_chain = int((rgb["used"] ^ th["used"]).sum())
    print(f"{bc.config_id(cfg)}: contributors per tile {per_tile.flatten().tolist()}; stopped in RGB only {only_rgb:.3f}, in thermal only {only_th:.3f}; "
          f"Gaussians used by one chain only {one_chain}; last contributors differ on {float((rgb['last'] != th['last']).float().mean()):.3f} of the pixels")
    if case == "deep":
        assert any(n >= 3 * 256 and n % 256 != 0 for n in per_tile.flatten().tolist())
        assert float((rgb["last"] != th["last"]).float().mean()) > 0.1
    elif case == "opaque":
        assert int(per_tile.max()) > 256
        assert (only_rgb if sep == "thermal_low" else only_th) >= 0.10
        assert {"thermal_low", "rgb_low"} <= {c[3] for c in bc.SEP_CONFIGS if c[0] == "opaque"}  # each direction has its configuration
    elif case == "faint":
        assert one_chain >= 50


@pytest.mark.parametrize("cfg", bc.ALL_CONFIGS, ids=IDS)
def test_no_two_depths_are_closer_than_float32_can_order(cfg):
    """A condition on the scenes: a float32 ulp at these depths is about 2.4e-7, the smallest gap a hundred times that (`ties`: outside
    the tied pairs, whose depths are bit-equal and whose order is the index order in both precisions)."""
    case = cfg[0]
    st = bc.reference(*cfg)["st"]
    gap = bc.visible_depth_gap(st, fc.TIE_PAIRS if case == "ties" else None)
    print(f"{bc.config_id(cfg)}: smallest depth gap {gap:.3e}")
    assert gap >= bc.MIN_GAP_KEPT


@pytest.mark.parametrize("cfg", bc.ALL_CONFIGS, ids=IDS)
def test_few_decisions_are_near_a_threshold(cfg):
    st = bc.reference(*cfg)["st"]
    share, excl = float(st["flag_pixels"].float().mean()), bc.cpu_excluded(st)
    print(f"{bc.config_id(cfg)}: flagged pixels {100 * share:.2f} %, Gaussians on the frustum clamp {int(excl.sum())} of {excl.numel()}")
    assert share <= bc.MAX_FLAGGED_PIXELS
    assert int(excl.sum()) <= bc.MAX_EXCLUDED_GAUSSIANS * excl.numel()


WALK_CONFIGS = [("opaque", "classic", 3, None), ("deep", "antialiased", 3, None), ("faint", "antialiased", 3, None), ("single", "classic", 3, None),
                ("clamped", "classic", 3, None), ("opaque", "classic", 3, "thermal_low")]


@pytest.mark.parametrize("cfg", WALK_CONFIGS, ids=[bc.config_id(c) for c in WALK_CONFIGS])
def test_the_walk_is_the_derivative(cfg):
    """float64: raster_backward_walk chained through the projection equals autograd of the restatement."""
    case, mode, deg, sep = cfg
    ref = bc.reference(*cfg)
    walk = bc.walk_grads(ref["p"], case, mode, deg, sep, ref["w"], torch.float64)
    keep = torch.ones(ref["p"]["means"].shape[0], dtype=torch.bool)
    for k, g in ref["g64"].items():
        e = bc.rel_err(walk[k], g, keep)
        print(f"{bc.config_id(cfg)} d {k}: walk vs autograd {e:.2e} (largest entry {bc.amax(g):.2e})")
        assert e <= 1e-9, k
    assert bc.amax(ref["g64"]["means"]) > 0 and bc.amax(ref["g64"]["opacities"]) > 0


@pytest.mark.parametrize("cfg", bc.ALL_CONFIGS, ids=IDS)
def test_float32_floors_stay_small(cfg):
    ref = bc.reference(*cfg)
    fl = bc.floors(ref, bc.cpu_excluded(ref["st"]), cfg[3])
    print(f"{bc.config_id(cfg)} (references {ref['seconds']:.1f} s): " + ", ".join(f"{k} {f:.1e} (autograd {a:.1e}, walk {w:.1e})" for k, (f, a, w) in fl.items()))
    for k, (f, _, _) in fl.items():
        assert f <= bc.MAX_FLOOR, (k, f)


def test_the_order_inside_a_tied_pair_shows_in_the_gradients():
    """`ties`: the float64 gradients with each pair swapped differ from those in index order by more than 1e-3 of the largest entry on
    some parameter -- so the GPU test can tell which order the kernels used."""
    cfg = [c for c in bc.CONFIGS if c[0] == "ties"][0]
    sw = bc.swapped_reference(*cfg)
    keep = torch.ones(sw["own"]["xys"].shape[0], dtype=torch.bool)
    diffs = {k: bc.rel_err(sw["other"][k], sw["own"][k], keep) for k in sw["own"]}
    print("ties, swapped vs index order: " + ", ".join(f"{k} {v:.2e}" for k, v in diffs.items()))
    assert max(diffs.values()) > 1e-3


@pytest.mark.parametrize("cfg", bc.PROBE_CONFIGS, ids=[bc.config_id(c) for c in bc.PROBE_CONFIGS])
def test_probe_pixels_exist_and_the_one_pixel_walk_agrees_with_the_loop(cfg):
    """The pixels the GPU test probes: each kind the case calls for is found, and the vectorised one-pixel statement (bc.probe_pixel) gives
    the final transmittance and the stop of the looped float64 walk at that pixel."""
    case, mode, deg, sep = cfg
    pixels, pj, op = bc.probe_pixels(*cfg)
    _, fw = bc.walk_stats(bc.reference(*cfg)["p"], case, mode, deg, sep, "op_t" if sep else "op")
    labels = [l for l, _, _ in pixels]
    print(f"{bc.config_id(cfg)}: " + ", ".join(f"{l} ({x}, {y}): {int(fw['count'][y, x])} contributors" for l, x, y in pixels))
    assert "most contributors" in labels and len(pixels) <= 6
    if case == "opaque":
        assert "stopped, longest list" in labels and "running, same quadrant" in labels
    if case in ("ragged", "sliver"):
        assert "last column" in labels
    if case == "ragged":
        assert "last row" in labels
    if case == "huge":
        assert "corner tile" in labels
    if sep == "thermal_low":
        assert "thermal runs longer than RGB" in labels
    if sep == "rgb_low":
        assert "thermal stops earlier than RGB" in labels
    for _, x, y in pixels:
        pp = bc.probe_pixel(pj, op, x, y)
        assert abs(pp["T"] - float(fw["T"][y, x])) <= 1e-12 and pp["stopped"] == bool(fw["stopped"][y, x])
        assert int((pp["weight"] > 0).sum()) == int(fw["count"][y, x])
