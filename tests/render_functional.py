"""A torch restatement of the frame rule of csrc/tn_render.hip (colour maps and bytes), runnable on the CPU: every operation is a torch operation of
its own on float32 tensors, so every product, sum and quotient is rounded on its own, in the order of the reference's expressions
(nerfstudio/utils/colormaps.py).  Scalars the reference computes in Python (far - near + 1e-10, colormap_max - colormap_min) are computed in Python
floats here too and rounded to float32 where torch rounds them: when they meet the tensor.

The one deliberate difference from the reference: min and max are over the FINITE values of the panel's source, (0, 0) where it has none, and the min
/ max a later step (normalize after the depth step) needs are that step's values at the source's min and max -- every step before it is monotone, so
on all-finite frames these are torch.min / torch.max of the step's output, which the comparison with the recorded reference outputs confirms bit for
bit (tests/test_render_cpu.py).  Also the cases of tests/golden/render_reference.npz, which scripts/make_golden_render.py runs the reference on."""
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT_PATH = os.path.join(ROOT, "nerfstudio-thermal_amd", "colormap_luts.json")
F32 = torch.float32
COLORMAPS = ("default", "turbo", "viridis", "magma", "inferno", "cividis", "gray")
SIZES = ((5, 7), (33, 19))


def tables() -> Dict[str, Tensor]:
    with open(LUT_PATH, encoding="utf-8") as f:
        g = json.load(f)
    return {str(n): torch.from_numpy(np.array(t, dtype=np.float64).astype(np.float32)) for n, t in zip(g["names"], g["luts"])}


def _s(v: float, like: Tensor) -> Tensor:
    """a Python scalar as torch rounds it when it meets a float32 tensor"""
    return torch.tensor(float(v), dtype=torch.float64).to(device=like.device, dtype=F32)


def finite_minmax(x: Tensor) -> Tuple[Tensor, Tensor]:
    v = x[torch.isfinite(x)]
    if v.numel() == 0:
        z = torch.zeros((), dtype=F32, device=x.device)
        return z, z.clone()
    return v.min(), v.max()


def _depth_step(x: Tensor, near_f: Tensor, den_f: Tensor) -> Tensor:
    return torch.clip((x - near_f) / den_f, 0, 1)


def scalar_value(x: Tensor, normalize: bool = False, colormap_min: float = 0, colormap_max: float = 1, invert: bool = False, depth: bool = False,
                 near_plane: Optional[float] = None, far_plane: Optional[float] = None) -> Tensor:
    """the value in [0, 1] a one-channel panel is coloured by"""
    x = x.to(F32)
    mn, mx = finite_minmax(x)
    a, b = mn, mx
    if depth:
        near = near_plane or float(mn)  # the reference's `or`: 0.0 counts as not given
        far = far_plane or float(mx)
        near_f, den_f = _s(near, x), _s(far - near + 1e-10, x)
        x = _depth_step(x, near_f, den_f)
        a, b = _depth_step(mn, near_f, den_f), _depth_step(mx, near_f, den_f)
    if normalize:
        lo, hi = (b, a) if bool(b < a) else (a, b)
        x = (x - lo) / ((hi - lo) + _s(1e-9, x))
    x = x * _s(float(colormap_max) - float(colormap_min), x) + _s(colormap_min, x)
    x = torch.clip(x, 0, 1)
    if invert:
        x = 1 - x
    return torch.where(torch.isnan(x), torch.zeros_like(x), x)


def colours(image: Tensor, colormap: str = "default", accumulation: Optional[Tensor] = None, lut: Optional[Dict[str, Tensor]] = None, **kw) -> Tensor:
    """float colours [H,W,3] of a panel [H,W,1] or [H,W,3] (kw: scalar_value's)"""
    if image.shape[-1] == 3:
        return image.to(F32)
    x = scalar_value(image, **kw)
    name = "turbo" if colormap == "default" else colormap
    if name == "gray":
        c = x.repeat(1, 1, 3)
    else:
        table = (lut if lut is not None else tables())[name].to(x.device)
        c = table[(x * 255).long()[..., 0]]
    if kw.get("depth") and accumulation is not None:
        acc = accumulation.to(F32).reshape(x.shape)
        c = c * acc + (1 - acc)
    return c


def to_bytes(c: Tensor) -> Tensor:
    v = torch.clip(c, 0, 1) * 255 + 0.5
    return torch.where(torch.isnan(v), torch.zeros_like(v), v).to(torch.uint8)  # [0.5, 255.5]: truncation


def compose(panels: Sequence[dict], lut: Optional[Dict[str, Tensor]] = None) -> Tensor:
    """uint8 [H, k W, 3]: panels are dicts of colours' arguments"""
    lut = lut if lut is not None else tables()
    return torch.cat([to_bytes(colours(lut=lut, **p)) for p in panels], dim=1)


# ---------------------------------------------------------------------------------------------------- the recorded cases
def edge_values() -> Tensor:
    """values exactly on k / 255, 0, 1, and just outside [0, 1]"""
    ks = torch.tensor([1, 2, 3, 64, 127, 128, 200, 254, 255], dtype=torch.float64) / 255
    one = torch.tensor(1.0, dtype=F32)
    return torch.cat([ks.to(F32), torch.tensor([0.0, 1.0, -0.0]), torch.nextafter(one, one * 2)[None], torch.nextafter(one, one * 0)[None],
                      torch.tensor([-1e-7, -0.25, 1.5, 1e-30])])


def frame(H: int, W: int, kind: str) -> Tensor:
    """[H,W,1] float32: "unit" values in [0, 1] with the edge values in front, "depth" values in [0.3, 6.5], "wide" values in [-0.5, 1.5],
    "const" one value, "inf" the unit frame with +inf and -inf in it."""
    g = torch.Generator().manual_seed(1000 * H + W + sum(map(ord, kind)))
    x = torch.rand((H * W,), generator=g)
    if kind in ("unit", "inf", "wide"):
        e = edge_values()
        x[:e.numel()] = e
        if kind == "wide":
            x = x * 2 - 0.5
        if kind == "inf":
            x[-1], x[-2] = float("inf"), float("-inf")
    elif kind == "depth":
        x = 0.3 + 6.2 * x
    elif kind == "const":
        x = torch.full((H * W,), 2.5)
    return x.view(H, W, 1).contiguous()


def accumulation(H: int, W: int) -> Tensor:
    """[H,W,1] in [0, 1] with exact zeros and ones"""
    a = torch.rand((H * W,), generator=torch.Generator().manual_seed(77 * H + W))
    a[::5], a[1::7] = 0.0, 1.0
    return a.view(H, W, 1).contiguous()


def colormap_cases() -> List[dict]:
    """apply_colormap cases: every colour map; normalize on and off; invert; colormap_min / max (0.2, 0.7); the unit, wide and inf frames"""
    cases = []
    for H, W in SIZES:
        for cmap in COLORMAPS:
            cases.append(dict(H=H, W=W, kind="unit", colormap=cmap, normalize=False, invert=False, cmin=0.0, cmax=1.0))
        for kind in ("unit", "wide"):
            for normalize in (False, True):
                for invert in (False, True):
                    for cmin, cmax in ((0.0, 1.0), (0.2, 0.7)):
                        cases.append(dict(H=H, W=W, kind=kind, colormap="inferno", normalize=normalize, invert=invert, cmin=cmin, cmax=cmax))
        cases.append(dict(H=H, W=W, kind="wide", colormap="gray", normalize=True, invert=True, cmin=0.2, cmax=0.7))
        # (0.51 - 0.02 rounds to another float32 when the two are rounded to float32 first: the difference is Python's, in double)
        cases.append(dict(H=H, W=W, kind="unit", colormap="turbo", normalize=False, invert=False, cmin=0.02, cmax=0.51))
        cases.append(dict(H=H, W=W, kind="inf", colormap="turbo", normalize=False, invert=False, cmin=0.0, cmax=1.0))
        cases.append(dict(H=H, W=W, kind="inf", colormap="gray", normalize=False, invert=True, cmin=0.2, cmax=0.7))
    return cases


def depth_cases() -> List[dict]:
    """apply_depth_colormap cases: near / far given, absent and near = 0.0; with and without accumulation; a constant frame; normalize and invert"""
    cases = []
    for H, W in SIZES:
        for near, far in ((None, None), (1.0, 5.0), (0.0, 4.0), (0.7, None), (None, 3.3)):
            for acc in (True, False):
                cases.append(dict(H=H, W=W, kind="depth", colormap="default", normalize=False, invert=False, cmin=0.0, cmax=1.0, near=near, far=far, acc=acc))
        cases.append(dict(H=H, W=W, kind="depth", colormap="viridis", normalize=True, invert=True, cmin=0.2, cmax=0.7, near=1.0, far=5.0, acc=True))
        cases.append(dict(H=H, W=W, kind="depth", colormap="gray", normalize=True, invert=False, cmin=0.0, cmax=1.0, near=None, far=None, acc=True))
        cases.append(dict(H=H, W=W, kind="const", colormap="magma", normalize=False, invert=False, cmin=0.0, cmax=1.0, near=None, far=None, acc=True))
        cases.append(dict(H=H, W=W, kind="inf", colormap="cividis", normalize=False, invert=False, cmin=0.0, cmax=1.0, near=0.25, far=0.75, acc=True))
    return cases


def case_key(prefix: str, i: int) -> str:
    return f"{prefix}{i:03d}"


def case_inputs(c: dict) -> Tuple[Tensor, Optional[Tensor]]:
    return frame(c["H"], c["W"], c["kind"]), (accumulation(c["H"], c["W"]) if c.get("acc") else None)


def case_colours(c: dict, lut=None) -> Tensor:
    """the restatement's colours of a recorded case"""
    image, acc = case_inputs(c)
    kw = dict(normalize=c["normalize"], colormap_min=c["cmin"], colormap_max=c["cmax"], invert=c["invert"])
    if "near" in c:
        kw.update(depth=True, near_plane=c["near"], far_plane=c["far"])
    return colours(image, c["colormap"], accumulation=acc, lut=lut, **kw)


# ---------------------------------------------------------------------------------------------------- camera path cases
def random_poses(n: int, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """n random poses [n,3,4] (a rotation from a QR factorisation, det +1; positions in [-2, 2]^3) and Ks [n,3,3], float64"""
    rng = np.random.default_rng(seed)
    poses, Ks = [], []
    for _ in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        poses.append(np.concatenate([q, rng.uniform(-2, 2, (3, 1))], 1))
        fx, fy = rng.uniform(300, 600, 2)
        Ks.append(np.array([[fx, 0.0, 320.0], [0.0, fy, 240.0], [0.0, 0.0, 1.0]]))
    return np.stack(poses), np.stack(Ks)


PATH_CASES = tuple((n, steps, order) for n in (3, 5) for steps in (1, 4) for order in (False, True))
SPIRAL_CASES = (dict(steps=7, radius=0.4, radiuses=None, rots=2, zrate=0.5), dict(steps=5, radius=None, radiuses=(0.3, 0.5, 0.2), rots=1, zrate=0.25))

CAMERA_PATH_JSON = {
    "render_height": 48, "render_width": 64, "fps": 24, "seconds": 1.0,
    "camera_path": [
        {"camera_to_world": [1.0, 0.0, 0.0, 0.1, 0.0, 1.0, 0.0, -0.2, 0.0, 0.0, 1.0, 2.5, 0.0, 0.0, 0.0, 1.0], "fov": 50.0, "aspect": 1.3333},
        {"camera_to_world": [0.8, 0.0, 0.6, 1.5, 0.0, 1.0, 0.0, 0.0, -0.6, 0.0, 0.8, 2.0, 0.0, 0.0, 0.0, 1.0], "fov": 62.5, "aspect": 1.3333},
        {"camera_to_world": [0.0, 0.0, 1.0, 2.5, 0.0, 1.0, 0.0, 0.3, -1.0, 0.0, 0.0, 0.125, 0.0, 0.0, 0.0, 1.0], "fov": 75.0, "aspect": 1.3333},
    ],
    "crop": {"crop_bg_color": {"r": 38, "g": 42, "b": 55}, "crop_center": [0.1, -0.05, 0.0], "crop_scale": [1.2, 0.9, 1.5], "crop_rot": [0.1, -0.2, 0.3]},
}
