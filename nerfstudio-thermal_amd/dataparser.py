"""RGB+T `transforms.json` datasets on disk: reader, writer and loader.

Reader  = ThermalNerf dataparser (data/dataparsers/thermalnerf_dataparser.py:17-30 over nerfstudio_dataparser.py:67-466): frames sorted by
          file name, per-frame or global intrinsics and distortion, `is_thermal` per frame, "up" orientation + centring + auto scale of the
          poses (cameras/camera_utils.py:449-474,515-623), the thermal-aware train/eval split (data/utils/dataparsers_utils.py:23-73).
Writer  = the layout process_data/rgbt_to_nerfstudio_dataset.py:240-266 produces: RGB frames first, then the thermal frames, every frame with
          its own fl_x/fl_y/cx/cy/w/h/k1/k2/p1/p2 and `is_thermal`, images under images/ and images_thermal/ (8-bit PNG; thermal single channel).
Loader  = InputDataset.get_image_float32 (data/datasets/base_dataset.py:61-95): uint8 / 255, a single-channel image repeated to 3 channels.
Points  = load_3D_points (nerfstudio_dataparser.py:352-466): the sparse point cloud named by `ply_file_path`, read by `read_ply` (the
          subset of PLY that open3d's reader is used for there: ascii / binary little-endian vertices with optional colours), moved into the
          dataparser's frame and scale; `write_ply` writes such a file.

The outputs feed ops.ImageCache / DeviceDataManager (the per-step pixel sampling and ray generation run on the device) and
ThermalNerfactoModel.get_outputs_for_camera.  Host-side, one-off work: plain numpy / torch CPU; nothing here is on the per-ray path.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor


@dataclass
class ThermalNerfDataParserConfig:
    data: str = ""
    scale_factor: float = 1.0
    downscale_factor: Optional[int] = None
    scene_scale: float = 1.0
    orientation_method: str = "up"  # "up" | "none"
    center_method: str = "poses"  # "poses" | "none"
    auto_scale_poses: bool = True
    eval_mode: str = "fraction"  # "fraction" | "interval" | "all"
    train_split_fraction: float = 0.9
    eval_interval: int = 8
    load_3D_points: bool = False  # metadata points3D_xyz / points3D_rgb from transforms.json's ply_file_path (splatfacto's seed points)

    def setup(self) -> "ThermalNerf":
        return ThermalNerf(self)


@dataclass
class DataparserOutputs:
    image_filenames: List[str]
    cameras: Dict[str, Tensor]  # c2w [C,3,4], fx, fy, cx, cy [C] fp32, width, height [C] int32, distortion [C,6] (k1,k2,k3,k4,p1,p2)
    scene_box_aabb: Tensor  # [2,3]
    dataparser_scale: float
    dataparser_transform: Tensor  # [3,4]
    metadata: Dict[str, list] = field(default_factory=dict)  # "is_thermal": per image


def rotation_matrix(a: Tensor, b: Tensor) -> Tensor:
    """Rotation taking direction a to direction b (cameras/camera_utils.py:449-474; the exactly-opposite case is nudged deterministically)."""
    a = a / torch.linalg.norm(a)
    b = b / torch.linalg.norm(b)
    v = torch.linalg.cross(a, b)
    c = torch.dot(a, b)
    if c < -1 + 1e-8:
        return rotation_matrix(a + torch.tensor([1e-3, -2e-3, 1.5e-3]), b)
    s = torch.linalg.norm(v)
    k = torch.tensor([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return torch.eye(3) + k + k @ k * ((1 - c) / (s**2 + 1e-8))


def auto_orient_and_center_poses(poses: Tensor, method: str = "up", center_method: str = "poses") -> Tuple[Tensor, Tensor]:
    """cameras/camera_utils.py:515-623 for the methods the thermal pipeline uses.  poses [C,4,4] -> ([C,3,4], transform [3,4])."""
    origins = poses[..., :3, 3]
    mean_origin = torch.mean(origins, dim=0)
    if center_method == "poses":
        translation = mean_origin
    elif center_method == "none":
        translation = torch.zeros_like(mean_origin)
    else:
        raise NotImplementedError(f"center_method={center_method}")
    if method == "up":
        up = torch.mean(poses[:, :3, 1], dim=0)
        up = up / torch.linalg.norm(up)
        rot = rotation_matrix(up, torch.tensor([0.0, 0.0, 1.0]))
        transform = torch.cat([rot, rot @ -translation[..., None]], dim=-1)
    elif method == "none":
        transform = torch.eye(4)
        transform[:3, 3] = -translation
        transform = transform[:3, :]
    else:
        raise NotImplementedError(f"orientation_method={method}")
    return transform @ poses, transform


def train_eval_split_fraction(image_filenames: Sequence[str], train_split_fraction: float) -> Tuple[np.ndarray, np.ndarray]:
    """data/utils/dataparsers_utils.py:23-73: equally spaced training images; for a thermal dataset (file names under images_thermal/) the
    same frame numbers are chosen in both spectra (the list holds the RGB block first, then the thermal block, as the sort by name leaves it)."""
    total = len(image_filenames)
    num_thermal = sum("images_thermal" in str(f) for f in image_filenames)
    num_rgb = total - num_thermal
    n = min(num_rgb, num_thermal) if num_thermal > 0 else total
    n_train = math.ceil(n * train_split_fraction)
    i_train = np.linspace(0, n - 1, n_train, dtype=int)
    i_eval = np.setdiff1d(np.arange(n), i_train)
    if num_thermal > 0:
        rem = max(num_rgb, num_thermal) - n
        r_train = np.linspace(0, rem - 1, math.ceil(rem * train_split_fraction), dtype=int)
        r_eval = np.setdiff1d(np.arange(rem), r_train)
        r_train, r_eval = r_train + n, r_eval + n
        if n == num_rgb:
            i_train = np.concatenate((i_train, i_train + num_rgb, r_train + num_rgb))
            i_eval = np.concatenate((i_eval, i_eval + num_rgb, r_eval + num_rgb))
        else:
            i_train = np.concatenate((i_train, r_train, i_train + num_rgb))
            i_eval = np.concatenate((i_eval, r_eval, i_eval + num_rgb))
    assert total == len(i_train) + len(i_eval) and len(np.intersect1d(i_train, i_eval)) == 0
    return i_train, i_eval


def _distortion(src: dict) -> List[float]:
    if "distortion_params" in src:
        return [float(x) for x in src["distortion_params"]]
    return [float(src.get(k, 0.0)) for k in ("k1", "k2", "k3", "k4", "p1", "p2")]


class ThermalNerf:
    def __init__(self, config: ThermalNerfDataParserConfig):
        self.config = config
        self.downscale_factor = config.downscale_factor

    def _fname(self, file_path: str, data_dir: str) -> str:
        """_get_fname of both parsers: <folder>_<factor>/<name> when a downscale factor > 1 is in use (thermal frames use their own folder
        name as the prefix), auto factor = smallest power of two that brings the longer side under 1600 px and exists on disk."""
        folder, name = os.path.split(file_path)
        if self.downscale_factor is None:
            from PIL import Image

            w, h = Image.open(os.path.join(data_dir, file_path)).size
            df = 0
            while max(h, w) / 2**df > 1600 and os.path.exists(os.path.join(data_dir, f"{os.path.basename(folder)}_{2 ** (df + 1)}", name)):
                df += 1
            self.downscale_factor = 2**df
        if self.downscale_factor > 1:
            return os.path.join(data_dir, f"{os.path.basename(folder)}_{self.downscale_factor}", name)
        return os.path.join(data_dir, file_path)

    def get_dataparser_outputs(self, split: str = "train") -> DataparserOutputs:
        c = self.config
        path = c.data
        meta_path = path if path.endswith(".json") else os.path.join(path, "transforms.json")
        data_dir = os.path.dirname(meta_path)
        with open(meta_path, encoding="utf-8") as f:
            meta = json.load(f)
        fnames = [self._fname(fr["file_path"], data_dir) for fr in meta["frames"]]
        order = np.argsort(fnames)
        frames = [meta["frames"][i] for i in order]
        image_filenames = [fnames[i] for i in order]

        def per_frame(key, cast):
            return [cast(meta[key]) if key in meta else cast(fr[key]) for fr in frames]

        fx, fy = per_frame("fl_x", float), per_frame("fl_y", float)
        cx, cy = per_frame("cx", float), per_frame("cy", float)
        height, width = per_frame("h", int), per_frame("w", int)
        global_dist = any(k in meta for k in ("k1", "k2", "k3", "p1", "p2", "distortion_params"))
        dist = [_distortion(meta) if global_dist else _distortion(fr) for fr in frames]
        poses = torch.from_numpy(np.array([fr["transform_matrix"] for fr in frames]).astype(np.float32))
        if c.eval_mode == "fraction":
            i_train, i_eval = train_eval_split_fraction(image_filenames, c.train_split_fraction)
        elif c.eval_mode == "interval":
            allv = np.arange(len(image_filenames))
            i_train, i_eval = allv[allv % c.eval_interval != 0], allv[allv % c.eval_interval == 0]
        elif c.eval_mode == "all":
            i_train = i_eval = np.arange(len(image_filenames))
        else:
            raise NotImplementedError(f"eval_mode={c.eval_mode}")
        if split == "train":
            indices = i_train
        elif split in ("val", "test"):
            indices = i_eval
        else:
            raise ValueError(f"Unknown dataparser split {split}")
        poses, transform = auto_orient_and_center_poses(poses, method=meta.get("orientation_override", c.orientation_method), center_method=c.center_method)
        scale = 1.0
        if c.auto_scale_poses:
            scale /= float(torch.max(torch.abs(poses[:, :3, 3])))
        scale *= c.scale_factor
        poses[:, :3, 3] *= scale
        idx = torch.as_tensor(np.asarray(indices), dtype=torch.long)
        s = 1.0 / (self.downscale_factor or 1)  # Cameras.rescale_output_resolution (cameras/cameras.py:930-967)
        t = lambda v, dt=torch.float32: torch.tensor(v, dtype=dt)[idx]  # noqa: E731
        cams = {"c2w": poses[idx][:, :3, :4].contiguous(), "fx": t(fx) * s, "fy": t(fy) * s, "cx": t(cx) * s, "cy": t(cy) * s,
                "width": (t(width) * s).to(torch.int32), "height": (t(height) * s).to(torch.int32), "distortion": t(dist)}
        a = c.scene_scale
        dataparser_transform = transform
        if "applied_transform" in meta:
            at = torch.tensor(meta["applied_transform"], dtype=transform.dtype)
            dataparser_transform = transform @ torch.cat([at, torch.tensor([[0, 0, 0, 1]], dtype=transform.dtype)], 0)
        if "applied_scale" in meta:
            scale *= float(meta["applied_scale"])
        metadata = {"is_thermal": [frames[i]["is_thermal"] for i in indices]}
        if c.load_3D_points:
            if "ply_file_path" in meta:
                metadata.update(load_3D_points(os.path.join(data_dir, meta["ply_file_path"]), transform, scale))
            else:
                print("Warning: load_3D_points set to true but no point cloud found. splatfacto will use random point cloud initialization.")
        return DataparserOutputs(image_filenames=[image_filenames[i] for i in indices], cameras=cams,
                                 scene_box_aabb=torch.tensor([[-a, -a, -a], [a, a, a]], dtype=torch.float32), dataparser_scale=scale,
                                 dataparser_transform=dataparser_transform, metadata=metadata)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """The vertices of a PLY file -> (xyz [M,3] float32, rgb [M,3] uint8, or [0,3] when the file has no colours -- what
    np.asarray(pcd.colors) gives).  Formats ascii 1.0 and binary_little_endian 1.0; x y z of any numeric type (read as float64, as open3d
    does, then cast); red green blue as uchar (the bytes as stored) or float / double ((c * 255).astype(uint8), open3d's colours times 255 as
    nerfstudio_dataparser.py:461 computes them; clipped to 0..255 first).  Other vertex properties and the elements after `vertex` are
    ignored; fixed-size elements before it are skipped.  ValueError: big-endian or unknown formats, a missing x, y or z, a list property at or
    before the vertices, a truncated body."""
    return _read_ply_vertices(path)[:2]


def read_ply_thermal(path: str) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
    """read_ply plus the vertices' `thermal` property -> (xyz, rgb, thermal [M,1] uint8, or None when the file has no such property): the rendered
    temperature a NeRF point cloud carries (cloud.py).  uchar as stored; float / double as the colours are read, (t * 255).astype(uint8) after
    clipping to 0..255."""
    return _read_ply_vertices(path)[:3]


def read_ply_normals(path: str) -> Optional[np.ndarray]:
    """The vertices' normals -> [M,3] float32 (nx ny nz of any numeric type, cast), or None when the file lacks one of the three properties."""
    return _read_ply_vertices(path)[3]


def _ply_u8(path: str, values: np.ndarray, what: str) -> np.ndarray:
    if values.dtype == np.uint8:
        return values.copy()
    if values.dtype.kind == "f":
        return np.clip(values.astype(np.float64) * 255, 0, 255).astype(np.uint8)
    raise ValueError(f"{path}: {what} of type {values.dtype} (uchar, float or double are read)")


def _ply_header(path: str, data: bytes) -> Tuple[str, List[Tuple[str, int, List[Tuple[str, str]]]], int]:
    """The header of a PLY file's bytes -> (format, [(element, count, [(property, numpy type, or "list")])], offset of the body).  ValueError:
    no PLY header, unknown or big-endian formats, unknown property types.  (The header reader of _read_ply_vertices and of splat_io.)"""
    if not data.startswith(b"ply"):
        raise ValueError(f"{path}: not a PLY file")
    end = data.find(b"end_header")
    if end < 0:
        raise ValueError(f"{path}: PLY header without end_header")
    body = data.index(b"\n", end) + 1
    fmt = None
    elements: List[Tuple[str, int, List[Tuple[str, str]]]] = []  # (name, count, [(property, numpy type)])
    for raw in data[:end].decode("ascii", errors="replace").splitlines()[1:]:
        tok = raw.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            if len(tok) < 3 or tok[1] not in ("ascii", "binary_little_endian", "binary_big_endian"):
                raise ValueError(f"{path}: unknown PLY format {' '.join(tok[1:])!r}")
            if tok[1] == "binary_big_endian":
                raise ValueError(f"{path}: big-endian PLY is not supported (ascii 1.0 and binary_little_endian 1.0 are)")
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property outside an element")
            if tok[1] == "list":
                elements[-1][2].append((tok[-1], "list"))
            elif tok[1] in _PLY_TYPES:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
            else:
                raise ValueError(f"{path}: unknown PLY property type {tok[1]!r}")
    if fmt is None:
        raise ValueError(f"{path}: PLY header without a format line")
    return fmt, elements, body


def _read_ply_vertices(path: str) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
    """-> (xyz, rgb, thermal or None, normals or None) of the vertex element."""
    with open(path, "rb") as f:
        data = f.read()
    fmt, elements, body = _ply_header(path, data)
    names = [e[0] for e in elements]
    if "vertex" not in names:
        raise ValueError(f"{path}: PLY without a vertex element")
    vi = names.index("vertex")
    for name, _, props in elements[:vi + 1]:
        if any(t == "list" for _, t in props):
            raise ValueError(f"{path}: list property in element {name!r} at or before the vertices")
    count, props = elements[vi][1], elements[vi][2]
    pnames = [p for p, _ in props]
    for axis in ("x", "y", "z"):
        if axis not in pnames:
            raise ValueError(f"{path}: the vertices have no {axis!r} property")
    if fmt == "ascii":
        lines = data[body:].decode("ascii", errors="replace").splitlines()
        skip = sum(e[1] for e in elements[:vi])
        rows = [ln.split() for ln in lines[skip:skip + count]]
        if len(rows) < count or any(len(r) < len(props) for r in rows):
            raise ValueError(f"{path}: truncated PLY body ({len(rows)} of {count} vertices)")
        cols = {p: np.array([r[i] for r in rows], dtype=np.float64 if t[0] == "f" else np.int64).astype(t) for i, (p, t) in enumerate(props)}
    else:
        off = body + sum(e[1] * int(np.dtype([(p, "<" + t) for p, t in e[2]]).itemsize) for e in elements[:vi])
        dt = np.dtype([(p, "<" + t) for p, t in props])
        if len(data) < off + count * dt.itemsize:
            raise ValueError(f"{path}: truncated PLY body ({len(data) - off} bytes, {count} vertices need {count * dt.itemsize})")
        arr = np.frombuffer(data, dtype=dt, count=count, offset=off)
        cols = {p: arr[p] for p in pnames}
    xyz = np.stack([cols[a].astype(np.float64) for a in ("x", "y", "z")], -1).astype(np.float32)
    thermal = _ply_u8(path, np.asarray(cols["thermal"]), "vertex thermal values").reshape(-1, 1) if "thermal" in pnames else None
    normals = np.stack([cols[a].astype(np.float32) for a in ("nx", "ny", "nz")], -1) if all(a in pnames for a in ("nx", "ny", "nz")) else None
    if not all(c in pnames for c in ("red", "green", "blue")):
        return xyz, np.zeros((0, 3), dtype=np.uint8), thermal, normals
    return xyz, _ply_u8(path, np.stack([cols[c] for c in ("red", "green", "blue")], -1), "vertex colours"), thermal, normals


def write_ply(path: str, xyz: np.ndarray, rgb: Optional[np.ndarray] = None, binary: bool = True, thermal: Optional[np.ndarray] = None,
              normals: Optional[np.ndarray] = None) -> str:
    """xyz [M,3] (float32 or float64 -> float / double properties) and optional rgb [M,3] (uint8 -> uchar, float -> float / double) as one
    PLY vertex element, binary little-endian or ascii.  With `thermal` ([M] or [M,1] uint8) one more property, `uchar thermal`, follows; without
    it the file is byte for byte what it was before the property existed.  With `normals` ([M,3], written as float) nx ny nz follow x y z
    directly, Open3D's order and mesh.write_mesh_ply's; without them, again, the file is what it was."""
    xyz = np.asarray(xyz)
    if xyz.dtype not in (np.float32, np.float64):
        xyz = xyz.astype(np.float32)
    ptype = {np.dtype("u1"): "uchar", np.dtype("f4"): "float", np.dtype("f8"): "double"}
    fields = [(a, xyz.dtype) for a in ("x", "y", "z")]
    if normals is not None:
        normals = np.asarray(normals)
        if normals.shape != (xyz.shape[0], 3) or normals.dtype.kind != "f":
            raise ValueError(f"write_ply: normals must be [{xyz.shape[0]},3] floats, got {normals.shape} of type {normals.dtype}")
        normals = normals.astype(np.float32)
        fields += [(a, normals.dtype) for a in ("nx", "ny", "nz")]
    if rgb is not None:
        rgb = np.asarray(rgb)
        if rgb.dtype not in ptype:
            raise ValueError(f"write_ply: colours of type {rgb.dtype} (uint8, float32 or float64)")
        fields += [(c, rgb.dtype) for c in ("red", "green", "blue")]
    if thermal is not None:
        thermal = np.asarray(thermal).reshape(-1)
        if thermal.dtype != np.uint8 or thermal.shape[0] != xyz.shape[0]:
            raise ValueError(f"write_ply: thermal must be {xyz.shape[0]} uint8 values, got {thermal.shape[0]} of type {thermal.dtype}")
        fields.append(("thermal", thermal.dtype))
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", f"element vertex {xyz.shape[0]}"]
    head += [f"property {ptype[np.dtype(t)]} {n}" for n, t in fields] + ["end_header"]
    rec = np.empty(xyz.shape[0], dtype=[(n, np.dtype(t).newbyteorder("<")) for n, t in fields])
    for i, a in enumerate(("x", "y", "z")):
        rec[a] = xyz[:, i]
    if normals is not None:
        for i, a in enumerate(("nx", "ny", "nz")):
            rec[a] = normals[:, i]
    if rgb is not None:
        for i, c in enumerate(("red", "green", "blue")):
            rec[c] = rgb[:, i]
    if thermal is not None:
        rec["thermal"] = thermal
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if binary:
            f.write(rec.tobytes())
        else:
            for r in rec:
                f.write((" ".join(repr(float(r[n])) if np.dtype(t).kind == "f" else str(int(r[n])) for n, t in fields) + "\n").encode("ascii"))
    return path


def load_3D_points(ply_path: str, transform: Tensor, scale: float) -> Dict[str, Tensor]:
    """nerfstudio_dataparser.py:429-466: the cloud in the dataparser's frame, points3D_xyz = cat(xyz, 1) @ transform.T * scale (transform =
    auto_orient_and_center_poses' [3,4], scale = the final scale, applied_scale included), and points3D_rgb uint8.  A file with a `thermal` vertex property (a NeRF point cloud, cloud.py) adds points3D_thermal uint8 [M,1]; a
    file without it adds no such key.  A file with all of nx ny nz adds points3D_normals float32 [M,3] = n @ transform[:, :3].T: the normals
    turn with the points and are neither scaled nor translated.  No keys for an empty cloud."""
    xyz, rgb, thermal, normals = _read_ply_vertices(ply_path)
    if xyz.shape[0] == 0:
        return {}
    points = torch.from_numpy(xyz)
    points = torch.cat((points, torch.ones_like(points[..., :1])), -1) @ transform.T
    points *= scale
    out = {"points3D_xyz": points, "points3D_rgb": torch.from_numpy(rgb)}
    if thermal is not None:
        out["points3D_thermal"] = torch.from_numpy(thermal)
    if normals is not None:
        out["points3D_normals"] = torch.from_numpy(normals) @ transform[:, :3].T.to(torch.float32)
    return out


def load_image_uint8(path: str) -> Tensor:
    """[H,W,3] uint8 (base_dataset.py:61-77, get_numpy_image: a single-channel image is repeated to three channels; alpha dropped, as
    load_image_float32 drops it)."""
    from PIL import Image

    im = np.array(Image.open(path), dtype="uint8")
    if im.ndim == 2:
        im = im[:, :, None].repeat(3, axis=2)
    return torch.from_numpy(np.ascontiguousarray(im[:, :, :3]))


def load_image_float32(path: str) -> Tensor:
    """[H,W,3] fp32 in [0,1] (base_dataset.py:61-95: uint8 / 255; a single-channel image is repeated to three channels; alpha dropped)."""
    from PIL import Image

    im = np.array(Image.open(path), dtype="uint8")
    if im.ndim == 2:
        im = im[:, :, None].repeat(3, axis=2)
    return torch.from_numpy(im[:, :, :3].astype("float32") / 255.0)


def write_rgbt_dataset(out_dir: str, cams: Dict[str, np.ndarray], images: Sequence[np.ndarray]) -> str:
    """Write cameras + images as an RGB+T nerfstudio dataset (the layout of process_data/rgbt_to_nerfstudio_dataset.py:240-266).
    cams: c2w [C,3,4], fx, fy, cx, cy, width, height, distortion [C,6] (k1,k2,k3,k4,p1,p2), is_thermal [C]; images [H,W,3] fp32 in [0,1].
    RGB frames are written first, then the thermal frames; frame k of each spectrum is frame_{k+1:05d}.png."""
    from PIL import Image

    os.makedirs(os.path.join(out_dir, "images"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "images_thermal"), exist_ok=True)
    frames = []
    counters = {0: 0, 1: 0}
    order = [i for i in range(len(images)) if not cams["is_thermal"][i]] + [i for i in range(len(images)) if cams["is_thermal"][i]]
    for i in order:
        th = int(bool(cams["is_thermal"][i]))
        counters[th] += 1
        rel = os.path.join("images_thermal" if th else "images", f"frame_{counters[th]:05d}.png")
        u8 = np.clip(np.rint(np.asarray(images[i]) * 255.0), 0, 255).astype(np.uint8)
        Image.fromarray(u8[:, :, 0] if th else u8).save(os.path.join(out_dir, rel))
        m = np.eye(4)
        m[:3, :4] = cams["c2w"][i]
        d = cams["distortion"][i]
        frames.append({"file_path": rel.replace(os.sep, "/"), "transform_matrix": m.tolist(), "colmap_im_id": len(frames) + 1, "is_thermal": th,
                       "fl_x": float(cams["fx"][i]), "fl_y": float(cams["fy"][i]), "cx": float(cams["cx"][i]), "cy": float(cams["cy"][i]),
                       "w": int(cams["width"][i]), "h": int(cams["height"][i]), "k1": float(d[0]), "k2": float(d[1]), "p1": float(d[4]), "p2": float(d[5])})
    path = os.path.join(out_dir, "transforms.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump({"camera_model": "OPENCV", "frames": frames}, f, indent=4)
    return path
