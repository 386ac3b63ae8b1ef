"""Frame rendering on the GPU: tn_frame_compose's bytes against the torch restatement (render_functional) at every position, with no tolerance;
tn_frame_minmax against the finite min and max; the float colours of tn_frame_colors; and render_trajectory end to end on both models -- the PNGs it
writes against compose_frame of the model's own frames, with and without a crop."""
import os

import numpy as np
import pytest
import torch

import render_functional as rf
import splat_functional as sf

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 77
SIZES = [(1, 1), (3, 5), (7, 64), (33, 19), (64, 65)]


def _render():
    import nerfstudio_thermal_amd  # noqa: F401
    from nerfstudio_thermal_amd import render

    return render


_LUT = {}


def _lut():
    if not _LUT:
        _LUT.update(rf.tables())
    return _LUT


def _values(H, W, seed, lo=-0.25, hi=1.25, bad=False):
    """[H,W,1]: random values in [lo, hi) with the edge values of render_functional in front (as many as fit), and with `bad` a NaN, +inf and -inf"""
    g = torch.Generator().manual_seed(seed)
    x = lo + (hi - lo) * torch.rand((H * W,), generator=g)
    e = rf.edge_values()[:H * W]
    x[:e.numel()] = e
    if bad and H * W >= 8:
        x[H * W // 2], x[H * W // 3], x[-1] = float("nan"), float("inf"), float("-inf")
    return x.view(H, W, 1).contiguous()


def _panel_specs(H, W):
    """Eight panels that mix three-channel, scalar and depth panels: each a dict of render_functional.colours' arguments."""
    acc = rf.accumulation(H, W)
    rgb = torch.cat([_values(H, W, 11 + k) for k in range(3)], dim=2).contiguous()
    rgb2 = torch.rand((H, W, 3), generator=torch.Generator().manual_seed(5))
    if H * W >= 4:
        rgb2[0, 0, 1], rgb2[-1, -1, 2] = float("nan"), float("inf")
    depth = 0.3 + 6.2 * torch.rand((H, W, 1), generator=torch.Generator().manual_seed(6))
    return [
        dict(image=rgb),
        dict(image=_values(H, W, 1), colormap="default", colormap_min=0.02, colormap_max=0.51),  # (a pair whose difference must be taken in double)
        dict(image=depth, colormap="turbo", depth=True, accumulation=acc),
        dict(image=_values(H, W, 2, -0.5, 1.5), colormap="inferno", normalize=True, invert=True, colormap_min=0.2, colormap_max=0.7),
        dict(image=depth, colormap="gray", depth=True, near_plane=0.0, far_plane=4.0, accumulation=acc),
        dict(image=depth, colormap="viridis", depth=True, near_plane=1.0, far_plane=5.0, normalize=True),
        dict(image=_values(H, W, 3, bad=True), colormap="magma", normalize=True),
        dict(image=rgb2),
    ]


def _records(render, specs):
    """the panel records of the specs (through render._panel: min / max launched where needed) and what they point to"""
    keep, records = [], []
    scratch = render._Scratch(DEV, len(specs))
    for s in specs:
        opts = render.ColormapOptions(s.get("colormap", "default"), s.get("normalize", False), s.get("colormap_min", 0), s.get("colormap_max", 1),
                                      s.get("invert", False))
        acc = s.get("accumulation")
        rec, _, _ = render._panel(s["image"].to(DEV), opts, scratch, depth=s.get("depth", False), accumulation=None if acc is None else acc.to(DEV),
                                  near_plane=s.get("near_plane"), far_plane=s.get("far_plane"), keep=keep)
        records.append(rec)
    return records, keep


# ---------------------------------------------------------------------------------------------------- 1. the frame
@pytest.mark.parametrize("H,W", SIZES)
def test_compose_bytes_equal_the_restatement(H, W):
    """1, 2, 3, 4 and 8 panels: every byte is the restatement's.  The frame sits between two guard rows (so its start is dword-aligned only where a
    row's bytes are a multiple of 4: both store paths run) and, a second time, at the start of its buffer (aligned; the last run of 4 pixels is short
    where H k W is no multiple of 4); the guard rows stay as they were."""
    render = _render()
    specs = _panel_specs(H, W)
    for k in (1, 2, 3, 4, 8):
        chosen = (specs[k - 1:] + specs[:k - 1])[:k] if k < 8 else specs  # another mix for every k
        want = rf.compose(chosen, _lut())
        assert want.shape == (H, k * W, 3) and want.dtype == torch.uint8
        records, keep = _records(render, chosen)
        for front in (1, 0):
            buf = torch.full((H + front + 1, k * W, 3), GUARD, dtype=torch.uint8, device=DEV)
            render.compose_call(records, H, W, buf[front:front + H])
            got = buf.cpu()
            assert torch.equal(got[front:front + H], want), (k, front, (got[front:front + H] != want).nonzero()[:5].tolist())
            assert bool((got[:front] == GUARD).all()) and bool((got[front + H:] == GUARD).all()), (k, front)
        del keep


def test_compose_frame_names_panels_and_float_colours():
    """compose_frame on an output dict: depth panels blend over accumulation, depth_thermal over accumulation_thermal; the float functions give the
    restatement's colours bit for bit; a wrong name is a KeyError that lists the keys."""
    render = _render()
    H, W = 33, 19
    acc, acc_th = rf.accumulation(H, W), rf.accumulation(W, H).reshape(H, W, 1).contiguous()
    depth = 0.3 + 6.2 * torch.rand((H, W, 1), generator=torch.Generator().manual_seed(8))
    outputs = {"rgb": torch.rand((H, W, 3), generator=torch.Generator().manual_seed(9)), "thermal": _values(H, W, 4), "depth": depth,
               "depth_thermal": depth * 0.5, "accumulation": acc, "accumulation_thermal": acc_th, "background": torch.zeros(3)}
    on_dev = {k: v.to(DEV) for k, v in outputs.items()}
    opts = render.ColormapOptions(colormap="inferno", colormap_min=0.1, colormap_max=0.9)
    kw = dict(colormap="inferno", colormap_min=0.1, colormap_max=0.9)
    got = render.compose_frame(on_dev, ["rgb", "thermal", "depth", "depth_thermal"], opts, depth_near_plane=0.0, depth_far_plane=5.0)
    want = rf.compose([dict(image=outputs["rgb"]), dict(image=outputs["thermal"], **kw),
                       dict(image=depth, depth=True, near_plane=0.0, far_plane=5.0, accumulation=acc, **kw),
                       dict(image=depth * 0.5, depth=True, near_plane=0.0, far_plane=5.0, accumulation=acc_th, **kw)], _lut())
    assert torch.equal(got.cpu(), want)
    no_th = {k: v for k, v in on_dev.items() if k != "accumulation_thermal"}  # a shared-opacity model: depth_thermal blends over accumulation
    got = render.compose_frame(no_th, ["depth_thermal"], opts)
    assert torch.equal(got.cpu(), rf.compose([dict(image=depth * 0.5, depth=True, accumulation=acc, **kw)], _lut()))
    with pytest.raises(KeyError, match="accumulation_thermal"):
        render.compose_frame(on_dev, ["rgb", "normals"])
    with pytest.raises(NotImplementedError):
        render.compose_frame(on_dev, ["rgb"], render.ColormapOptions(colormap="pca"))
    # the float functions
    x = _values(H, W, 12, -0.5, 1.5).to(DEV)
    for cmap in rf.COLORMAPS:
        o = render.ColormapOptions(colormap=cmap, normalize=True, invert=True, colormap_min=0.2, colormap_max=0.7)
        assert torch.equal(render.apply_colormap(x, o).cpu(), rf.colours(x.cpu(), cmap, normalize=True, invert=True, colormap_min=0.2, colormap_max=0.7,
                                                                          lut=_lut())), cmap
    assert torch.equal(render.apply_float_colormap(_values(H, W, 13, 0.0, 1.0).to(DEV)).cpu(), rf.colours(_values(H, W, 13, 0.0, 1.0), "viridis", lut=_lut()))
    d = render.apply_depth_colormap(on_dev["depth"], on_dev["accumulation"], far_plane=4.0)
    assert d.shape == (H, W, 3) and d.dtype == torch.float32
    assert torch.equal(d.cpu(), rf.colours(depth, "default", depth=True, far_plane=4.0, accumulation=acc, lut=_lut()))
    assert render.apply_colormap(on_dev["rgb"]) is on_dev["rgb"]


# ---------------------------------------------------------------------------------------------------- 2. min and max
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 33 * 19])
def test_minmax_is_the_finite_min_and_max(n):
    """Clean values, then NaN and +-inf sprinkled in, then nothing but NaN: the bits of the finite min and max ((0, 0) where there is none), the same
    bits on a second run, and a workspace and neighbours that the call leaves alone.  4097 values take three blocks and the final pass."""
    render = _render()
    g = torch.Generator().manual_seed(n)
    clean = torch.randn((n,), generator=g) * 3
    dirty = clean.clone()
    dirty[::7] = float("nan")
    dirty[3::11] = float("inf")
    dirty[5::13] = float("-inf")
    words = render._lib.TN_FRAME_MINMAX_WORKSPACE_BYTES // 4
    for x in (clean, dirty, torch.full((n,), float("nan"))):
        want = torch.stack(rf.finite_minmax(x))
        runs = []
        for _ in range(2):
            out = torch.full((4,), -7.0, device=DEV)
            ws = torch.full((words + 1,), -7.0, device=DEV)
            render.minmax_call(x.to(DEV), out[1:3], ws[:words])
            runs.append(out.cpu())
            assert float(ws[words]) == -7.0 and out[0] == -7.0 and out[3] == -7.0
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
        assert torch.equal(runs[0][1:3].view(torch.int32), want.view(torch.int32)), (n, runs[0][1:3].tolist(), want.tolist())


# ---------------------------------------------------------------------------------------------------- 3. end to end
def _splat_model():
    from nerfstudio_thermal_amd import splat

    cfg = splat.ThermalSplatfactoModelConfig(sh_degree=1, sh_degree_interval=1, background_thermal=0.3, thermal_opacity_mode="separate")
    m = splat.ThermalSplatfactoModel(cfg, num_points=4, device=DEV)
    m.load_gaussians(sf.scene(64, 0, 1))
    m.step = 10
    m.eval()
    return m


def _splat_cameras(render):
    from nerfstudio_thermal_amd.synth import look_at_camera

    W, H = 32, 24
    fx = sf.fov_focal(W)
    ends = [render.PinholeCamera(look_at_camera(eye), fx, fx, W / 2, H / 2, W, H) for eye in ((2.3, 0.4, 0.6), (1.2, 1.9, 0.9))]
    return render.interpolated_path(ends, 3)


def _read(paths):
    from nerfstudio_thermal_amd.texture import read_png

    return [torch.from_numpy(read_png(p)) for p in paths]


def test_render_trajectory_splat(tmp_path):
    """Three interpolated cameras over the 64-Gaussian scene of splat_functional: three PNGs whose pixels are compose_frame of the model's own frames
    -- without a crop, with the crop of the JSON (through both forms of `crop`), with two pinned buffers (the default) and with one."""
    render = _render()
    model = _splat_model()
    cams = _splat_cameras(render)
    assert len(cams) == 3
    names = ("rgb", "thermal", "depth")
    paths = render.render_trajectory(model, cams, str(tmp_path / "a"))
    assert [os.path.basename(p) for p in paths] == ["00000.png", "00001.png", "00002.png"] and sorted(os.listdir(tmp_path / "a")) == [os.path.basename(p) for p in paths]
    want = [render.compose_frame(model.get_outputs_for_camera(c), names).cpu() for c in cams]
    frames = _read(paths)
    assert all(f.shape == (24, 96, 3) and torch.equal(f, w) for f, w in zip(frames, want))
    assert not torch.equal(want[0], want[2]) and len(torch.unique(want[0][:, 32:64])) > 8  # the path moves and the thermal panel is coloured
    one = _read(render.render_trajectory(model, cams, str(tmp_path / "b"), pinned_buffers=1))
    assert all(torch.equal(f, w) for f, w in zip(one, want))
    crop = render.crop_from_json(rf.CAMERA_PATH_JSON)
    opts = render.ColormapOptions(colormap="inferno", normalize=True)
    all_names = ("rgb", "thermal", "depth", "accumulation", "accumulation_thermal")
    want_crop = [render.compose_frame(model.get_outputs_for_camera(c, crop[0]), all_names, opts, 0.5, 6.0).cpu() for c in cams]
    for form, sub in ((crop, "c"), (crop[0], "d")):
        got = _read(render.render_trajectory(model, cams, str(tmp_path / sub), all_names, crop=form, colormap_options=opts, depth_near_plane=0.5,
                                             depth_far_plane=6.0))
        assert all(torch.equal(f, w) for f, w in zip(got, want_crop))
    assert not torch.equal(want_crop[0][:, :96], want[0])  # the crop drops Gaussians
    half = _read(render.render_trajectory(model, cams[:1], str(tmp_path / "e"), rendered_resolution_scaling_factor=0.5))
    assert half[0].shape == (12, 48, 3)
    with pytest.raises(KeyError, match="rgb_thermal"):
        render.render_trajectory(model, cams[:1], str(tmp_path / "f"), ("rgb", "rgb_thermal"))


def test_render_trajectory_nerf(tmp_path):
    """A fresh thermal-nerfacto model (separate densities) at 16 x 12 with rgb, rgb_thermal, depth and depth_thermal; a crop raises the model's
    NotImplementedError, a wrong name a KeyError."""
    from test_model_api_gpu import build_model

    from nerfstudio_thermal_amd.synth import look_at_camera

    render = _render()
    _, _, model = build_model("separate")
    W, H = 16, 12
    fx = sf.fov_focal(W)
    cams = render.interpolated_path([render.PinholeCamera(look_at_camera(eye), fx, fx, W / 2, H / 2, W, H) for eye in ((0.9, 0.2, 0.3), (0.4, 0.8, 0.5))], 3)
    names = ("rgb", "rgb_thermal", "depth", "depth_thermal")
    model.train()
    paths = render.render_trajectory(model, cams, str(tmp_path / "n"), names)
    assert model.training is True
    model.eval()
    assert render.thermal_output_name(model) == "rgb_thermal" and len(paths) == 3
    for cam, frame in zip(cams, _read(paths)):
        outputs = render.model_outputs(model, cam)
        assert outputs["depth_thermal"].shape == (H, W, 1) and frame.shape == (H, 4 * W, 3)
        assert torch.equal(frame, render.compose_frame(outputs, names).cpu())
    default = _read(render.render_trajectory(model, cams[:1], str(tmp_path / "m")))
    assert torch.equal(default[0], render.compose_frame(render.model_outputs(model, cams[0]), ("rgb", "rgb_thermal", "depth")).cpu())
    with pytest.raises(NotImplementedError, match="obb_box"):
        render.render_trajectory(model, cams, str(tmp_path / "x"), names, crop=render.crop_from_json(rf.CAMERA_PATH_JSON))
    with pytest.raises(KeyError, match="depth_thermal"):
        render.render_trajectory(model, cams, str(tmp_path / "y"), ("rgb", "thermal"))


def test_render_dataset_writes_predictions_and_ground_truth(tmp_path):
    render = _render()
    model = _splat_model()
    cams = _splat_cameras(render)[:2]
    gt = torch.rand((24, 32, 3), generator=torch.Generator().manual_seed(3))
    pairs = [(cams[0], {"image": gt, "is_thermal": False}), (cams[1], {"image": gt, "is_thermal": True})]
    paths = render.render_dataset(model, pairs, str(tmp_path), ("rgb", "thermal", "depth"))
    rel = sorted(os.path.relpath(p, tmp_path) for p in paths)
    assert rel == sorted(["rgb/00000.png", "thermal/00000.png", "depth/00000.png", "gt-rgb/00000.png", "rgb/00001.png", "thermal/00001.png",
                          "depth/00001.png", "gt-thermal/00001.png"])
    read = {os.path.relpath(p, tmp_path): f for p, f in zip(paths, _read(paths))}
    out = model.get_outputs_for_camera(cams[1])
    assert torch.equal(read["thermal/00001.png"], render.compose_frame(out, ["thermal"]).cpu())
    assert torch.equal(read["gt-rgb/00000.png"], rf.to_bytes(gt))
    assert torch.equal(read["gt-thermal/00001.png"], rf.compose([dict(image=gt[..., :1].contiguous(), colormap="default")], _lut()))
