"""Thermal splats as Gaussian-splat PLY files, out and in: the counterpart of `ns-export gaussian-splat` (nerfstudio/scripts/exporter.py:480-546,
ExportGaussianSplat) and the way back.

The file is the Inria layout every splat viewer reads: one `vertex` element of float properties, binary little-endian, per Gaussian
x y z, nx ny nz (zeros), f_dc_0..2, f_rest_* (channel-major), opacity (logit), scale_0..2 (logs), rot_0..3 (as stored).  Three spectra:
  "rgb"      the Inria file of the colour scene;
  "thermal"  the same properties filled from the thermal parameters (and the thermal opacity in separate mode): any viewer shows the thermal
             scene in grey;
  "both"     the rgb row followed by f_dc_thermal, f_rest_thermal_* and, in separate mode, opacity_thermal.  Viewers go by property name and ignore
             the extras; `read_gaussian_ply` reads them back, so this is the lossless form (bit for bit for sh_degree > 0).
The rows are assembled on the device by tn_export_splat_pack (csrc/tn_splat_export.hip): Gaussians with a parameter that is not finite (the
reference's filter), with an opacity below `min_opacity`, or outside a crop box are dropped, the others keep their order.  `pack_call` is the only
place that knows that entry point's argument order.  There is no CPU fallback for the pack; the file layer (`ply_properties`, `write_gaussian_ply`,
`read_gaussian_ply`) is host code.

Every stored SH coefficient is exported whatever degree the training step has activated, as in the reference.  A model with sh_degree == 0 keeps
sigmoid colours in features_dc; its file carries f_dc = (sigmoid(dc) - 0.5) / C0, which a viewer's 0.5 + C0 f_dc turns back into the colour, and no
f_rest.  The reference writes uint8 `colors` for such a model instead; that layout is not reproduced.

Without a `transform` the file is in the model's frame.  `export_gaussian_ply(..., transform=T)` writes the Gaussians moved by the Similarity `T`
(splat_transform.py: means, scales, quaternions and the SH bands 1 to 3 of both spectra, on the device by tn_transform_splat, then the same pack);
`T = dataset_frame(dataparser_outputs, applied_transform)` puts the file into the dataset's own frame, where the point-cloud and mesh exports put
theirs.  `load_gaussian_ply(..., transform=T)` moves the file's Gaussians before they are loaded: `dataset_frame(...).inverse()` brings a
dataset-frame file home.  The reference offers no world-frame export for splats.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .dataparser import _ply_header
from .ops import _stream
from .splat_calls import _param_ptrs, _ptr
from .splat_camera import OrientedBox
from .splat_transform import Similarity, transform_gaussians

SPECTRA = {"rgb": 0, "thermal": 1, "both": 2}
SH_C0 = 0.28209479177387814
Box = Union[OrientedBox, _lib.TnSplatCrop, None]


# ---------------------------------------------------------------------------------------------------- the file layer (host only)
def ply_properties(spectrum: str, K: int, separate: bool, colour_mode: int = 0) -> List[str]:
    """The float properties of a row, in order, for K SH coefficients per channel (K - 1 of them `rest`).  colour_mode 1 (sh_degree == 0) has no
    f_rest.  "rgb" and "thermal" have the same 14 + 3 K names; "both" adds the thermal ones."""
    if spectrum not in SPECTRA:
        raise ValueError(f"spectrum must be one of {sorted(SPECTRA)}, got {spectrum!r}")
    if K < 1 or colour_mode not in (0, 1) or (colour_mode == 1 and K != 1):
        raise ValueError(f"ply_properties: K = {K} with colour_mode {colour_mode} (colour_mode 1 is the degree-0 layout: K = 1)")
    R = K - 1
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(3 * R)]
    names += ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    if spectrum == "both":
        names += ["f_dc_thermal"] + [f"f_rest_thermal_{i}" for i in range(R)] + (["opacity_thermal"] if separate else [])
    return names


def write_gaussian_ply(path: str, rows: np.ndarray, properties: Sequence[str]) -> str:
    """rows [M, W] float32 under `properties` (W names) as a binary little-endian PLY with one vertex element of float properties."""
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != len(properties) or rows.dtype != np.float32:
        raise ValueError(f"write_gaussian_ply: rows must be float32 [M,{len(properties)}], got {rows.dtype} {rows.shape}")
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {rows.shape[0]}"] + [f"property float {p}" for p in properties] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        np.ascontiguousarray(rows).astype("<f4", copy=False).tofile(f)
    return path


_REQUIRED = ("x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3")


def _indexed(names: Sequence[str], prefix: str, path: str) -> int:
    """How many `prefix`<i> properties there are; they must be numbered 0..count-1."""
    idx = sorted(int(n[len(prefix):]) for n in names if n.startswith(prefix) and n[len(prefix):].isdigit())
    if idx != list(range(len(idx))):
        raise ValueError(f"{path}: the {prefix}* properties are not numbered 0..{len(idx) - 1}")
    return len(idx)


def read_gaussian_ply(path: str, sh_degree: Optional[int] = None) -> Tuple[Dict[str, Tensor], dict]:
    """A Gaussian-splat PLY -> (params, info).  params are float32 host tensors under the gauss_params names; info has num_gaussians, K, sh_degree,
    has_thermal, separate, colour_mode and properties.

    binary_little_endian only.  The float properties are found by name, in any order; other properties (nx ny nz, anything unknown, of any fixed
    type) are skipped.  K comes from the number of f_rest_*, which must be 3 (K - 1) with K a square; f_rest_{c (K-1) + k} is
    features_rest[g,k,c].  An Inria file fills the six RGB parameters, and the thermal ones by the project's rule for Gaussians without thermal
    values: zeros, mid-grey.  A file with f_dc_thermal (and then f_rest_thermal_0..K-2) fills those too, and opacities_thermal where it has
    opacity_thermal.  `sh_degree` == 0 asks for the parameters of a degree-0 model: the file must have no f_rest, and features_dc (and
    features_dc_thermal, where the file has it) = logit(0.5 + C0 f_dc) in float64, clamped to logit's 1e-10 .. 1 - 1e-10, rounded once.
    ValueError: ASCII or big-endian files, a missing required property or one that is not a float, a K that is not a square, thermal rest
    coefficients that do not match K, a payload shorter than the header promises."""
    with open(path, "rb") as f:
        data = f.read()
    fmt, elements, body = _ply_header(path, data)
    if fmt != "binary_little_endian":
        raise ValueError(f"{path}: a Gaussian-splat PLY must be binary_little_endian, this one is {fmt}")
    names = [e[0] for e in elements]
    if "vertex" not in names:
        raise ValueError(f"{path}: PLY without a vertex element")
    vi = names.index("vertex")
    for name, _, props in elements[:vi + 1]:
        if any(t == "list" for _, t in props):
            raise ValueError(f"{path}: list property in element {name!r} at or before the vertices")
    count, props = elements[vi][1], elements[vi][2]
    types = dict(props)
    missing = [p for p in _REQUIRED if p not in types]
    if missing:
        raise ValueError(f"{path}: the vertices lack the properties {missing}")
    pnames = [p for p, _ in props]
    n_rest_th, n_rest_rgb = _indexed(pnames, "f_rest_thermal_", path), _indexed(pnames, "f_rest_", path)  # (f_rest_thermal_<i> has no digit after f_rest_)
    K = n_rest_rgb // 3 + 1
    degree = math.isqrt(K) - 1
    if n_rest_rgb % 3 != 0 or (degree + 1) ** 2 != K:
        raise ValueError(f"{path}: {n_rest_rgb} f_rest properties are not 3 (K - 1) for a square K (0, 9, 24, 45, ...)")
    has_thermal = "f_dc_thermal" in types
    if (has_thermal and n_rest_th != K - 1) or (not has_thermal and (n_rest_th or "opacity_thermal" in types)):
        raise ValueError(f"{path}: thermal properties that do not fit K = {K} (f_dc_thermal {'present' if has_thermal else 'absent'}, "
                         f"{n_rest_th} f_rest_thermal, opacity_thermal {'present' if 'opacity_thermal' in types else 'absent'})")
    if sh_degree == 0 and K != 1:
        raise ValueError(f"{path}: {n_rest_rgb} f_rest properties, a degree-0 model has none")
    separate = "opacity_thermal" in types
    off = body + sum(e[1] * int(np.dtype([(p, "<" + t) for p, t in e[2]]).itemsize) for e in elements[:vi])
    dt = np.dtype([(p, "<" + t) for p, t in props])
    if len(data) < off + count * dt.itemsize:
        raise ValueError(f"{path}: truncated PLY body ({len(data) - off} bytes, {count} vertices need {count * dt.itemsize})")
    arr = np.frombuffer(data, dtype=dt, count=count, offset=off)

    def cols(*wanted: str) -> Tensor:
        for p in wanted:
            if types[p] != "f4":
                raise ValueError(f"{path}: property {p!r} is not a float")
        if not wanted:
            return torch.zeros((count, 0), dtype=torch.float32)
        return torch.from_numpy(np.stack([arr[p] for p in wanted], -1).astype(np.float32))

    R = K - 1
    colour_mode = 1 if sh_degree == 0 else 0

    def dc(t: Tensor) -> Tensor:
        if colour_mode == 0:
            return t
        return torch.logit(0.5 + SH_C0 * t.double(), eps=1e-10).float()

    params = {
        "means": cols("x", "y", "z"), "scales": cols("scale_0", "scale_1", "scale_2"), "quats": cols("rot_0", "rot_1", "rot_2", "rot_3"),
        "opacities": cols("opacity"), "features_dc": dc(cols("f_dc_0", "f_dc_1", "f_dc_2")),
        "features_rest": cols(*[f"f_rest_{i}" for i in range(3 * R)]).reshape(count, 3, R).transpose(1, 2).contiguous(),
    }
    if has_thermal:
        params["features_dc_thermal"] = dc(cols("f_dc_thermal"))
        params["features_rest_thermal"] = cols(*[f"f_rest_thermal_{i}" for i in range(R)]).reshape(count, R, 1)
    else:
        params["features_dc_thermal"] = torch.zeros((count, 1), dtype=torch.float32)
        params["features_rest_thermal"] = torch.zeros((count, R, 1), dtype=torch.float32)
    if separate:
        params["opacities_thermal"] = cols("opacity_thermal")
    info = {"num_gaussians": count, "K": K, "sh_degree": degree, "has_thermal": has_thermal, "separate": separate, "colour_mode": colour_mode,
            "properties": pnames}
    return params, info


# ---------------------------------------------------------------------------------------------------- the raw call
def _crop(box: Box) -> Optional[_lib.TnSplatCrop]:
    if box is None or isinstance(box, _lib.TnSplatCrop):
        return box
    if isinstance(box, OrientedBox):
        return box.crop_struct()
    raise ValueError(f"crop must be an OrientedBox, a TnSplatCrop or None, got {type(box).__name__}")


def opacity_logit(min_opacity: float) -> float:
    """The float32 logit tn_export_splat_pack compares with: log(p / (1 - p)) in float64, rounded once; 0 switches the threshold off (-inf)."""
    p = float(min_opacity)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"min_opacity must be in [0, 1), got {min_opacity}")
    if p == 0.0:
        return -math.inf
    return float(np.float32(math.log(p / (1.0 - p))))


def pack_call(params: Sequence[Tensor], spectrum: int, colour_mode: int, min_opacity_logit: float, crop: Optional[_lib.TnSplatCrop], out_rows: Tensor,
              count: Tensor, workspace: Optional[Tensor] = None) -> None:
    """tn_export_splat_pack of the 8 (separate mode: 9) gauss_params tensors, in param_names order, into `out_rows` [N, W] fp32 and `count`
    (device int64 [1]); the workspace is allocated here unless given."""
    if len(params) not in (8, 9):
        raise ValueError(f"pack_call takes the 8 or 9 gauss_params tensors, got {len(params)}")
    n, R = int(params[0].shape[0]), int(params[5].shape[1])
    W = 17 + 3 * R + ((1 + R + (len(params) == 9)) if spectrum == 2 else 0)
    lib = _lib.load()
    if workspace is None:
        need = int(lib.tn_export_splat_workspace_bytes(n))
        if need < 0:
            raise ValueError(f"tn_export_splat_workspace_bytes({n}): a size the library refuses")
        workspace = torch.empty(max(need, 8), dtype=torch.uint8, device=params[0].device)
    if out_rows.dim() != 2 or tuple(out_rows.shape) != (n, W) or tuple(count.shape) != (1,):
        raise ValueError(f"pack_call: out_rows must be [{n},{W}] and count [1], got {tuple(out_rows.shape)} and {tuple(count.shape)}")
    pp = _param_ptrs(list(params))
    rc = lib.tn_export_splat_pack(*pp, *([None] if len(params) == 8 else []), n, R, int(spectrum), int(colour_mode), float(min_opacity_logit),
                                  C.byref(crop) if crop is not None else None, _ptr(out_rows, torch.float32, "out_rows"),
                                  _ptr(count, torch.int64, "count"), _ptr(workspace, torch.uint8, "workspace"), workspace.numel(), _stream())
    _lib.check(rc, "tn_export_splat_pack")


# ---------------------------------------------------------------------------------------------------- export and import of a model
def export_gaussian_ply(model, path: str, spectrum: str = "both", min_opacity: float = 0.0, crop: Box = None,
                        transform: Optional[Similarity] = None, fuse_3d_filter: bool = True) -> dict:
    """`model`'s Gaussians as the splat file `path`.  Dropped: Gaussians with a parameter of the row that is not finite, with
    sigmoid(opacity) < min_opacity (the row's opacity; in a "both" file of a separate-mode model the larger of the two, the MCMC strategy's notion
    of a live Gaussian; 0 keeps every opacity), and, with `crop` (an OrientedBox), those whose mean is not strictly inside the box.  One read-back
    of the kept number, one device-to-host copy of the kept rows.  Returns {"path", "exported", "dropped", "spectrum", "properties", "frame"}; no
    kept Gaussian gives a valid file with `element vertex 0`.

    `transform` None writes the model's frame ("frame": "model").  With a Similarity the parameters are moved out of place on the device
    (transform_gaussians; the model is not touched) and then packed as before ("frame": "transformed").  `crop` is still given in the model's
    frame, as an OrientedBox: it is moved with `transform.apply_box` and tested on the moved means, so a mean within rounding of a face may fall
    either way.  A parameter that is not finite stays not finite through the move, so the same Gaussians are dropped; `min_opacity` is not affected.

    A model with use_3d_filter writes, by default, the scales and opacities its renders read -- the 3D filter fused in (model.filtered_gaussians;
    Mip-Splatting's save_fused_ply), so a viewer shows what was trained, and `min_opacity` then compares the filtered opacity;
    `fuse_3d_filter=False` writes the raw parameters.  A move by `transform` comes after the fusion."""
    if spectrum not in SPECTRA:
        raise ValueError(f"spectrum must be one of {sorted(SPECTRA)}, got {spectrum!r}")
    colour_mode = 1 if model.config.sh_degree == 0 else 0
    if fuse_3d_filter and getattr(model.config, "use_3d_filter", False):
        named = {k: v.contiguous() for k, v in model.filtered_gaussians().items()}
    else:
        named = {k: model.gauss_params[k].detach().contiguous() for k in model.param_names}
    if transform is not None:
        if crop is not None and not transform.is_identity:
            if not isinstance(crop, OrientedBox):
                raise ValueError(f"crop must be an OrientedBox to be moved with the Gaussians, got {type(crop).__name__}")
            crop = transform.apply_box(crop)
        named = transform_gaussians(named, transform)
    params = [named[k] for k in model.param_names]
    n, R = int(params[0].shape[0]), int(params[5].shape[1])
    props = ply_properties(spectrum, R + 1, model.separate, colour_mode)
    logit, box = opacity_logit(min_opacity), _crop(crop)
    dev = params[0].device
    kept = 0
    rows = np.zeros((0, len(props)), dtype=np.float32)
    if n > 0:
        out = torch.empty((n, len(props)), dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        pack_call(params, SPECTRA[spectrum], colour_mode, logit, box, out, count)
        kept = int(count.item())
        rows = out[:kept].cpu().numpy()
    write_gaussian_ply(path, rows, props)
    return {"path": path, "exported": kept, "dropped": n - kept, "spectrum": spectrum, "properties": props,
            "frame": "model" if transform is None else "transformed"}


def load_gaussian_ply(model, path: str, transform: Optional[Similarity] = None) -> dict:
    """Replace `model`'s Gaussians by the file's (read_gaussian_ply, then model.load_gaussians, whose shared / separate rules apply: a file
    without opacity_thermal starts a separate-mode model's thermal logits as a copy of the opacities, a file with it is refused by a shared-mode
    model).  The file's K must be the model's (sh_degree + 1)^2.  With `transform` the file's Gaussians are moved on the device before they are
    loaded (transform_gaussians): `dataset_frame(...).inverse()` for a file in the dataset's frame.  Returns read_gaussian_ply's info."""
    want = int(model.config.sh_degree)
    params, info = read_gaussian_ply(path, sh_degree=want)
    if info["K"] != (want + 1) ** 2:
        raise ValueError(f"{path}: {info['K']} SH coefficients per channel (degree {info['sh_degree']}), the model has sh_degree {want}")
    if info["separate"] and not model.separate:
        raise ValueError(f'{path}: the file has opacity_thermal, the model has thermal_opacity_mode "shared"')
    if transform is not None and not transform.is_identity:
        params = {k: v.to(model.means.device).contiguous() for k, v in params.items()}
        params = transform_gaussians(params, transform, out=params)
    model.load_gaussians(params)
    return info
