"""The differentiable depth of the splat training render restated in torch, any dtype, and the references of tests/test_splat_depth_cpu.py and
tests/test_splat_depth_gpu.py.  Not a test module.

Classic mode.  depth = D / A where A = accumulation > 0, with D = sum alpha_i T_i z_i riding the RGB chain (the only chain in shared mode) as one more
colour channel without a background term, z_i the view-space depth of the mean; elsewhere depth is the frame's largest D, detached (the reference's
.detach().max()).  `render` builds that from bc.projected and sf.rasterize (sf.render's own depth is computed under no_grad); with a pose row the
projection is pf.render's (the corrected camera of tests/splat_pose_functional.py).

References per configuration, computed once (`reference`): the float64 gradients `g64` of sum(output * w) over every differentiable output --
rgb, thermal, accumulation(s) under bc.upstream's images and depth under one of two upstream images, both zero on the flagged pixels:
    "acc"   v_depth = w * accumulation    (the division by the accumulation cancels)
    "raw"   v_depth = w                   (divides by accumulations down to 1/255)
-- the same in float32 (`g32`), and the published backward walk in float32 (`walk32`: bc.raster_backward_walk fed five channels and
v_alpha_eff = v_alpha - vD * depth, vD = v_depth / A).  Errors are measured relative to `scale`: per gradient tensor the larger of the largest
entries of the two float64 PARTIAL gradients -- `gA`, the loss with A detached inside the quotient (the numerator's path, plus every other output's
term), and `gB`, the depth term with D detached (the normalisation's path); g64 = gA + gB.  On `single` the two cancel to ~1e-13 for the
geometry and the opacity under a depth-only upstream (one Gaussian's depth is its z whatever its alpha): float32 cannot reproduce that zero, and a
ratio against the sum would mean nothing."""
from __future__ import annotations

import functools

import torch

import splat_absgrad_functional as af
import splat_backward_cases as bc
import splat_functional as sf
import splat_oracle as so
import splat_pose_functional as pf
import test_splat_forward_cpu as fc

MODE = "classic"
UPSTREAMS = ("acc", "raw")
# (case, SH degree, separate-opacity variant, pose row of splat_pose_functional.POSES or None)
SHARED_CONFIGS = [("subtile", 3, None, None), ("opaque", 3, None, None), ("deep", 3, None, None), ("ragged", 1, None, None), ("clamped", 3, None, None),
                  ("single", 3, None, None)]
SEP_CONFIGS = [("opaque", 3, "thermal_low", None), ("opaque", 3, "rgb_low", None)]
POSE_CONFIG = ("subtile", 3, None, "moved")
ABS_CONFIG = ("ragged", 1, None, None)  # the configuration that also runs with use_absgrad
CONFIGS = SHARED_CONFIGS + SEP_CONFIGS + [POSE_CONFIG]
MAX_FLOOR_ACC = bc.MAX_FLOOR  # the suite's cap on a float32 floor: a condition on the scenes under the "acc" upstream
# The "raw" upstream divides by accumulations down to 1/255, which raises its float32 floor -- measured on the CPU over all configurations and
# gradients at 1.4e-6 to 3.5e-6 against 5e-7 to 1.8e-6 under "acc" (profiles/splat_depth_grad.md) -- but not past the suite's cap: it holds here too.
MAX_FLOOR_RAW = bc.MAX_FLOOR


def config_id(cfg):
    case, deg, sep, pose = cfg
    return f"{case}-{deg}" + (f"-sep-{sep}" if sep else "") + (f"-pose-{pose}" if pose else "")


def scene(cfg):
    case, deg, sep, pose = cfg
    return pf.scene(case, deg, sep, pose) if pose else bc.scene(case, deg, sep)


def projected(leaves, cfg, row=None):
    """What the rasteriser reads: bc.projected, or with a pose row the same through pf's corrected camera.  Returns (dict, corrected view or None)."""
    case, deg, _, pose = cfg
    if pose is None:
        return bc.projected(leaves, case, MODE, bc._deg_use(deg)), None
    c2w, fx, fy, cx, cy, W, H = bc.case_camera(case)
    dt = leaves["means"].dtype
    c2w2 = pf.apply_pose(c2w.to(dt), row.to(dt))
    view, proj = pf.camera_matrices(c2w2, fx, fy, W, H)
    quats = leaves["quats"] / leaves["quats"].norm(dim=-1, keepdim=True)
    pj = dict(sf.project(leaves["means"], torch.exp(leaves["scales"]), quats, view, proj, fx, fy, cx, cy, H, W, flag_tol=fc.FLAG_TOL))
    viewdirs = leaves["means"].detach() - c2w2[:3, 3].detach()
    viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    col = torch.cat([leaves["features_dc"][:, None, :], leaves["features_rest"]], 1)
    col_t = torch.cat([leaves["features_dc_thermal"][:, None, :], leaves["features_rest_thermal"]], 1)
    if deg > 0:
        sh = torch.cat([so.spherical_harmonics(deg, viewdirs, col), so.spherical_harmonics(deg, viewdirs, col_t)], -1) + 0.5
        pj["near_sh"] = (sh.detach().abs() < fc.FLAG_TOL).any(-1)
        pj["colors"] = torch.clamp(sh, min=0.0)
    else:
        pj["near_sh"] = torch.zeros(col.shape[0], dtype=torch.bool)
        pj["colors"] = torch.sigmoid(torch.cat([col[:, 0], col_t[:, 0]], -1))
    pj["op"] = torch.sigmoid(leaves["opacities"])[:, 0]
    if "opacities_thermal" in leaves:
        pj["op_t"] = torch.sigmoid(leaves["opacities_thermal"])[:, 0]
    return pj, view


def _background(dt):
    bg, bgt = fc.background()
    return torch.cat([bg, torch.tensor([bgt])]).to(dt)


def render(leaves, cfg, row=None, colors_from=None):
    """The training render with a differentiable depth, in the dtype of leaves["means"]: rgb, thermal (clamped), accumulation (+ accumulation_thermal),
    depth [H,W,1], its two partial forms depth_A (A detached) and depth_B (D detached), depth_raw (D), xys, view, projection, flag_pixels,
    flag_gaussians.  colors_from: parameters whose projection supplies the colours -- finite differences in the means pass the unperturbed ones, since
    the SH view directions carry no gradient."""
    case = cfg[0]
    _, W, H = bc.case_camera(case)[4:]
    pj, view = projected(leaves, cfg, row)
    if colors_from is not None:
        pj["colors"] = projected(colors_from, cfg, row)[0]["colors"]
    dt = leaves["means"].dtype
    bg4, zero1 = _background(dt), torch.zeros(1, dtype=dt)
    geom = (pj["xys"], pj["depths"], pj["radii"], pj["conics"], pj["tile_min"], pj["tile_max"])
    colors, z = pj["colors"], pj["depths"][:, None]
    out = {}
    if "op_t" in pj:  # separate mode: depth on chain 1, with RGB
        img, A, flag_pix, flag_g = sf.rasterize(*geom, torch.cat([colors[:, :3], z], -1), pj["op"], H, W, torch.cat([bg4[:3], zero1]), flag_tol=fc.FLAG_TOL,
                                                clamp_channels=3)
        img_t, A_t, fp_t, fg_t = sf.rasterize(*geom, colors[:, 3:], pj["op_t"], H, W, bg4[3:], flag_tol=fc.FLAG_TOL)
        raw, D, flag_pix, flag_g = torch.cat([img[..., :3], img_t], -1), img[..., 3:], flag_pix | fp_t, flag_g | fg_t
        out["accumulation_thermal"] = A_t[..., None]
    else:
        img, A, flag_pix, flag_g = sf.rasterize(*geom, torch.cat([colors, z], -1), pj["op"], H, W, torch.cat([bg4, zero1]), flag_tol=fc.FLAG_TOL, clamp_channels=4)
        raw, D = img[..., :4], img[..., 4:]
    A = A[..., None]
    covered = A > 0
    fill = D.detach().max()
    safe = torch.where(covered, A, torch.ones_like(A))  # (0 / 0 in the branch not taken would still poison the gradient)
    out.update({"rgb": torch.clamp(raw[..., :3], max=1.0), "thermal": torch.clamp(raw[..., 3:], max=1.0), "accumulation": A,
                "depth": torch.where(covered, D / safe, fill), "depth_A": torch.where(covered, D / safe.detach(), fill),
                "depth_B": torch.where(covered, D.detach() / safe, fill), "depth_raw": D, "xys": pj["xys"], "view": view, "projection": pj,
                "flag_pixels": flag_pix, "flag_gaussians": flag_g | (pj["near_clamp"] & pj["ok"]) | (pj["near_sh"] & pj["ok"])})
    return out


def images(sep):
    return [k for k, _ in bc.images(sep)]


def upstreams(cfg, out64):
    """bc.upstream's images for rgb, thermal and the accumulation(s), and the two depth upstreams, all zero on the pixels the float64 render flags."""
    case, _, sep, _ = cfg
    w = bc.upstream(case, sep, out64["flag_pixels"])
    gen = torch.Generator().manual_seed(7 + sum(map(ord, case)))
    wd = torch.randn(out64["depth"].shape, generator=gen, dtype=torch.float64) * (~out64["flag_pixels"])[..., None]
    return w, {"acc": wd * out64["accumulation"].detach().double(), "raw": wd}


def _wanted(leaves, out, row):
    return list(leaves.values()) + [out["xys"]] + ([row, out["view"]] if row is not None else [])


def _named(leaves, grads, row):
    named = {k: (torch.zeros_like(v) if g is None else g).detach().double() for (k, v), g in zip(leaves.items(), grads)}
    named["xys"] = grads[len(leaves)].detach().double()
    if row is not None:
        named["pose"], named["dview"] = grads[len(leaves) + 1].detach().double(), grads[len(leaves) + 2].detach().double()[:3]
    return named


def autograd_grads(p, cfg, w, v_depth, dt, parts=False):
    """{upstream name: gradients} of sum(output * w) + sum(depth * v_depth) over every parameter, xys and (pose configuration) the pose row and the
    corrected view, by autograd in `dt` through ONE forward graph.  parts: instead {name: (gA, gB)}, the two partial gradients (module docstring).
    Also returns the render, detached."""
    leaves = bc._leaves(p, dt)
    row = pf.pose_row(cfg[3]).to(dt).requires_grad_(True) if cfg[3] else None
    out = render(leaves, cfg, row)
    rest = sum((out[k] * w[k].to(dt)).sum() for k in w)
    res = {}
    for name, vd in v_depth.items():
        vd = vd.to(dt)
        if parts:
            gA = torch.autograd.grad(rest + (out["depth_A"] * vd).sum(), _wanted(leaves, out, row), allow_unused=True, retain_graph=True)
            gB = torch.autograd.grad((out["depth_B"] * vd).sum(), _wanted(leaves, out, row), allow_unused=True, retain_graph=True)
            zero = lambda g, like: [torch.zeros_like(t) if x is None else x for x, t in zip(g, like)]  # noqa: E731
            like = _wanted(leaves, out, row)
            res[name] = (_named(leaves, zero(gA, like), row), _named(leaves, zero(gB, like), row))
        else:
            g = torch.autograd.grad(rest + (out["depth"] * vd).sum(), _wanted(leaves, out, row), allow_unused=True, retain_graph=True)
            res[name] = _named(leaves, g, row)
    detached = {k: (v.detach() if isinstance(v, torch.Tensor) else {a: b.detach() for a, b in v.items()} if isinstance(v, dict) else v) for k, v in out.items()}
    return res, detached


def _walk_chains(pj, w, vd, sep, dt, H, W):
    """The chains of the frame as af.raster_backward_walk_abs takes them -- (colours, opacity, final T, last, upstream image, upstream accumulation,
    background) -- with the depth as chain 1's last channel and v_alpha_eff as its upstream accumulation; also `order` and the walk's depth image."""
    bg4, zero = _background(dt), torch.zeros((), dtype=dt)
    geom = [pj[k].detach() for k in ("xys", "depths", "radii", "conics", "tile_min", "tile_max")]
    col, z = pj["colors"].detach(), pj["depths"].detach()[:, None]
    nc = 3 if sep else 4  # colour channels of chain 1
    col1, bg1 = torch.cat([col[:, :nc], z], -1), torch.cat([bg4[:nc], torch.zeros(1, dtype=dt)])
    v1 = (w["rgb"] if sep else torch.cat([w["rgb"], w["thermal"]], -1)).to(dt)
    fw = bc.raster_forward_walk(*geom, col1, pj["op"].detach(), bg1, H, W)
    A, D = 1.0 - fw["T"], fw["img"][..., nc]
    safe = torch.where(A > 0, A, torch.ones_like(A))
    depth = torch.where(A > 0, D / safe, D.max())
    vD = torch.where(A > 0, vd.to(dt)[..., 0] / safe, zero)
    v_img = torch.cat([torch.where(fw["img"][..., :nc] <= 1.0, v1, zero), vD[..., None]], -1)  # the output clamp is the colours' alone
    chains = [(col1, pj["op"].detach(), fw["T"], fw["last"], v_img, w["accumulation"][..., 0].to(dt) - vD * depth, bg1)]
    if sep:
        fw_t = bc.raster_forward_walk(*geom, col[:, 3:], pj["op_t"].detach(), bg4[3:], H, W)
        v_t = torch.where(fw_t["img"] <= 1.0, w["thermal"].to(dt), zero)
        chains.append((col[:, 3:], pj["op_t"].detach(), fw_t["T"], fw_t["last"], v_t, w["accumulation_thermal"][..., 0].to(dt), bg4[3:]))
    return chains, fw["order"], depth


def walk_grads(p, cfg, w, v_depth, dt):
    """{upstream name: gradients} from bc.raster_backward_walk in `dt`, chained to the parameters (and the pose row) through `projected`; the entry
    "xys_abs" is af.raster_backward_walk_abs' statistic of the same chains."""
    case, _, sep, _ = cfg
    _, W, H = bc.case_camera(case)[4:]
    leaves = bc._leaves(p, dt)
    row = pf.pose_row(cfg[3]).to(dt).requires_grad_(True) if cfg[3] else None
    pj, view = projected(leaves, cfg, row)
    N = pj["xys"].shape[0]
    nc = 3 if sep else 4
    res = {}
    for name, vd in v_depth.items():
        with torch.no_grad():
            chains, order, _ = _walk_chains(pj, w, vd, sep, dt, H, W)
            d_xys, d_conics, d_colors = torch.zeros(N, 2, dtype=dt), torch.zeros(N, 3, dtype=dt), torch.zeros(N, 4, dtype=dt)
            d_z, d_ops = None, []
            for c, (col, op, T, last, v_img, v_acc, bg) in enumerate(chains):
                gx, gc, gcol, gop = bc.raster_backward_walk(pj["xys"].detach(), pj["conics"].detach(), col, op, pj["tile_min"], pj["tile_max"], order, T, last,
                                                            v_img, v_acc, bg)
                d_xys, d_conics = d_xys + gx, d_conics + gc
                if c == 0:
                    d_colors[:, :nc], d_z = gcol[:, :nc], gcol[:, nc]
                else:
                    d_colors[:, 3:] = gcol
                d_ops.append(gop)
            v_abs, _ = af.raster_backward_walk_abs(pj["xys"].detach(), pj["conics"].detach(), pj["tile_min"], pj["tile_max"], order, chains)
        outs = [pj["xys"], pj["conics"], pj["colors"], pj["depths"], pj["op"]] + ([pj["op_t"]] if sep else [])
        wanted = list(leaves.values()) + ([row, view] if row is not None else [])
        g = torch.autograd.grad(outs, wanted, grad_outputs=[d_xys, d_conics, d_colors, d_z] + d_ops, allow_unused=True, retain_graph=True)
        named = {k: (torch.zeros_like(v) if gi is None else gi).detach().double() for (k, v), gi in zip(leaves.items(), g)}
        named["xys"], named["xys_abs"] = d_xys.double(), v_abs.double()
        if row is not None:
            named["pose"], named["dview"] = g[len(leaves)].detach().double(), g[len(leaves) + 1].detach().double()[:3]
        res[name] = named
    return res


def grad_keys(cfg):
    return list(bc.param_names(cfg[2])) + ["xys"] + (["pose"] if cfg[3] else [])


@functools.lru_cache(maxsize=None)
def reference(cfg):
    """Everything the tests of one configuration share, computed once and never modified: the scene `p`, the float64 render `out64`, the upstream images
    `w` and `v_depth` {"acc", "raw"}, and per upstream name `gA`, `gB`, `g64` = gA + gB, `g32`, `walk32` (dicts of float64 tensors; the walk also holds
    "xys_abs"), `excl` (Gaussians on the frustum clamp) and `flagged`."""
    p = scene(cfg)
    with torch.no_grad():
        out64 = render({k: v.double() for k, v in p.items()}, cfg, pf.pose_row(cfg[3]) if cfg[3] else None)
    w, v_depth = upstreams(cfg, out64)
    parts, _ = autograd_grads(p, cfg, w, v_depth, torch.float64, parts=True)
    g64 = {n: {k: a[k] + b[k] for k in a} for n, (a, b) in parts.items()}  # (the product rule; test_splat_depth_cpu.py holds it to the undivided graph)
    g32, _ = autograd_grads(p, cfg, w, v_depth, torch.float32)
    walk32 = walk_grads(p, cfg, w, v_depth, torch.float32)
    pj = out64["projection"]
    return {"p": p, "out64": out64, "w": w, "v_depth": v_depth, "g64": g64, "gA": {n: a for n, (a, _) in parts.items()}, "gB": {n: b for n, (_, b) in parts.items()},
            "g32": g32, "walk32": walk32, "excl": pj["near_clamp"] & pj["ok"], "flagged": float(out64["flag_pixels"].float().mean())}


@functools.lru_cache(maxsize=None)
def walk64(cfg):
    """The float64 walk of the configuration ({upstream name: gradients, "xys_abs" among them}): the reference of last_xys_absgrad."""
    ref = reference(cfg)
    return walk_grads(ref["p"], cfg, ref["w"], ref["v_depth"], torch.float64)


def _rows(t, key, keep):
    return t if key in ("pose", "dview") else t[keep]


def scale(ref, name, key, excl):
    """The larger of the largest entries of the two float64 partial gradients over the kept Gaussians."""
    return max(bc.amax(_rows(ref["gA"][name][key], key, ~excl)), bc.amax(_rows(ref["gB"][name][key], key, ~excl)))


def err(g, ref, name, key, excl):
    """max |g - g64| over the kept Gaussians relative to `scale` (0 when both vanish)."""
    s = scale(ref, name, key, excl)
    d = bc.amax(_rows(g.double() - ref["g64"][name][key], key, ~excl))
    if s == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / s


def floors(ref, name, excl, cfg):
    """Per gradient: (floor, err of float32 autograd, err of the float32 walk), as bc.floors."""
    out = {}
    for k in grad_keys(cfg):
        ea, ew = err(ref["g32"][name][k], ref, name, k, excl), err(ref["walk32"][name][k], ref, name, k, excl)
        out[k] = (max(ea, ew, bc.EPS), ea, ew)
    return out


def max_floor(name):
    return MAX_FLOOR_ACC if name == "acc" else MAX_FLOOR_RAW


# ------------------------------------------------------------------------------------------------ the depth losses
def depth_losses(depth, accumulation, depth_image, depth_mult, tv_mult):
    """(depth_mult * depth_loss, tv_mult * depth_tv_loss) of tn_depth_loss in the dtype of `depth` [H,W,1], differentiable by autograd (sign(0) = 0):
    the mean |depth - depth_image| over the pixels with accumulation > 0 and a finite, positive depth_image (None, or no such pixel: 0), and
    thermal_reg_functional.tv's 0.25 * mean of the four absolute differences over the stride-1 2 x 2 windows whose four pixels all have
    accumulation > 0 (none: 0)."""
    d, cov = depth[..., 0], accumulation[..., 0] > 0
    zero = torch.zeros((), dtype=depth.dtype, device=depth.device)
    l_d = l_tv = zero
    if depth_mult and depth_image is not None:
        s = depth_image[..., 0].to(depth.dtype)
        valid = cov & torch.isfinite(s) & (s > 0)
        if bool(valid.any()):
            l_d = depth_mult * torch.where(valid, (d - torch.where(valid, s, zero)).abs(), zero).sum() / valid.sum()
    if tv_mult:
        win = cov[:-1, :-1] & cov[:-1, 1:] & cov[1:, :-1] & cov[1:, 1:]
        if bool(win.any()):
            p0, p1, p2, p3 = d[:-1, :-1], d[:-1, 1:], d[1:, :-1], d[1:, 1:]
            terms = (p0 - p1).abs() + (p0 - p2).abs() + (p1 - p3).abs() + (p2 - p3).abs()
            l_tv = tv_mult * 0.25 * torch.where(win, terms, zero).sum() / win.sum()
    return l_d, l_tv


def near_ties(depth, accumulation, depth_image, depth_mult, tv_mult, eps=1e-5):
    """[H,W] mask of the pixels one of whose live terms has an |argument| below eps (a sign decided in fp32 may differ there) and their share."""
    d, cov = depth[..., 0].double(), accumulation[..., 0] > 0
    mask = torch.zeros_like(cov)
    if depth_mult and depth_image is not None:
        s = depth_image[..., 0].double()
        valid = cov & torch.isfinite(s) & (s > 0)
        mask |= valid & ((d - torch.where(valid, s, torch.zeros_like(s))).abs() < eps)
    if tv_mult:
        win = cov[:-1, :-1] & cov[:-1, 1:] & cov[1:, :-1] & cov[1:, 1:]
        H, W = d.shape
        for (ay, ax), (by, bx) in (((0, 0), (0, 1)), ((0, 0), (1, 0)), ((0, 1), (1, 1)), ((1, 0), (1, 1))):
            a, b = d[ay:ay + H - 1, ax:ax + W - 1], d[by:by + H - 1, bx:bx + W - 1]
            near = win & ((a - b).abs() < eps)
            mask[ay:ay + H - 1, ax:ax + W - 1] |= near
            mask[by:by + H - 1, bx:bx + W - 1] |= near
    return mask, float(mask.float().mean())


def loss_frame(h, w, seed, border=0, holes=0.0):
    """(depth, accumulation, depth_image) [H,W,1] float32 for the loss tests: a smooth depth between 1 and 4 plus noise, an accumulation that is 0 on a
    `border`-wide frame edge and on a share `holes` of the pixels, and a sensor depth near the render's with invalid entries (0, negative, inf, NaN)."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    depth = 2.5 + 1.2 * torch.sin(3.0 * xx + 1.0) * torch.cos(2.0 * yy) + 0.05 * torch.rand(h, w, generator=gen)
    acc = 0.05 + 0.95 * torch.rand(h, w, generator=gen)
    if border:
        acc[:border], acc[-border:], acc[:, :border], acc[:, -border:] = 0.0, 0.0, 0.0, 0.0
    if holes:
        acc[torch.rand(h, w, generator=gen) < holes] = 0.0
    depth = torch.where(acc > 0, depth, torch.full_like(depth, float(depth.max())))  # uncovered pixels hold the fill value
    sensor = depth + 0.1 * torch.randn(h, w, generator=gen)
    bad = torch.rand(h, w, generator=gen)
    for lo, value in ((0.00, 0.0), (0.03, -1.0), (0.06, float("inf")), (0.09, float("nan"))):
        sensor[(bad >= lo) & (bad < lo + 0.03)] = value
    return depth[..., None].contiguous(), acc[..., None].contiguous(), sensor[..., None].contiguous()
