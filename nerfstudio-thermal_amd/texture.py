"""RGB and thermal textures for an exported mesh, on the device: the counterpart of nerfstudio/exporter/texture_utils.py (export_textured_mesh with
unwrap_method "custom"; xatlas unwrapping is not built).

The mesh is unwrapped into the reference's regular atlas -- two faces per square of (px + 3) x px texels -- and every texel gets the value of the
surface point it stands for: rendered by the radiance field along the interpolated normal (source "nerf": tn_texture_rays emits the rays of one chunk
of texels, the model renders them, tn_texture_store writes the bytes; no more than one chunk of rays ever exists), or interpolated from the mesh's own
per-vertex colours and temperatures (source "vertex": tn_texture_vertex, no model, so meshes from thermal splats get a texture too).  Because the
reference puts the triangles' corners on texel centres its barycentric weights are small integers over px - 1, and the kernels compute them that way in
double (csrc/tn_texture.hip states the atlas and the weights); the reference evaluates them as ratios of float32 UV areas, which cancel as the atlas
grows.  The thermal channel becomes a second, grey texture and a second material of the same OBJ.

The raw calls are `layout_call`, `coords_call`, `rays_call`, `vertex_call`, `store_call` and `mean_edge_call`, the only places that know the argument
order of their entry points (include/thermal_nerf_hip.h).  Everything runs on torch's current stream; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .cloud import _contig, _dev, _rows
from .mesh import Mesh, _is_splat, mesh_to_dataset_frame
from .ops import _stream
from .rays import RayBundle

F32 = torch.float32
SOURCES = ("nerf", "vertex")
RAYLEN_METHODS = ("edge", "none")
MATERIALS = {"rgb": ("material_0", "material_0.png"), "thermal": ("material_thermal", "material_0_thermal.png")}  # usemtl -> (material, its map_Kd)


@dataclass
class Texture:
    """rgb uint8 [H,W,3] and thermal uint8 [H,W] (row 0 is the top of the image), texture_coordinates fp32 [F,3,2] (u to the right, v down, 0..1 over
    the image; the OBJ writer flips v), on the device; raylen, the length of the rendered rays (0 for source "vertex"); rgbt fp32 [H,W,4], the values
    before they became bytes, with return_float."""

    rgb: Tensor
    thermal: Tensor
    texture_coordinates: Tensor
    raylen: float
    rgbt: Optional[Tensor] = None


# ---------------------------------------------------------------------------------------------------- the raw calls
def layout_call(num_faces: int, px_per_uv_triangle: int) -> Tuple[int, int, int, int]:
    """tn_texture_layout (host only, no device) -> (W, H, squares_w, squares_h); ValueError for fewer than 1 face or fewer than 2 texels per triangle."""
    out = (C.c_int64 * 4)()
    F, px = int(num_faces), int(px_per_uv_triangle)
    if not -2 ** 31 <= px < 2 ** 31 or _lib.load().tn_texture_layout(F, px, out) != 0:
        raise ValueError(f"texture atlas: {F} faces (at least 1) at px_per_uv_triangle = {px} (at least 2; the reference's scale (px - 1) / px is 0 at 1)")
    return tuple(int(v) for v in out)


def coords_call(num_faces: int, px: int, texture_coordinates: Tensor) -> None:
    """tn_texture_coords into texture_coordinates [F,3,2]"""
    rc = _lib.load().tn_texture_coords(int(num_faces), int(px), _contig(texture_coordinates, "texture_coordinates", (num_faces, 3, 2)), _stream())
    _lib.check(rc, "tn_texture_coords")


def _mesh_args(vertices: Tensor, faces: Tensor):
    V, Fn = vertices.shape[0], faces.shape[0]
    return V, _contig(faces, "faces", (Fn, 3), torch.int32), Fn


def rays_call(vertices: Tensor, normals: Tensor, faces: Tensor, px: int, raylen: float, texel0: int, count: int, origins: Tensor,
              directions: Tensor) -> None:
    """tn_texture_rays of texels [texel0, texel0 + count) into origins / directions [count,3]"""
    V, p_faces, Fn = _mesh_args(vertices, faces)
    rc = _lib.load().tn_texture_rays(_contig(vertices, "vertices", (V, 3)), _contig(normals, "normals", (V, 3)), V, p_faces, Fn, int(px), float(raylen),
                                     int(texel0), int(count), _contig(origins, "origins", (count, 3)), _contig(directions, "directions", (count, 3)),
                                     _stream())
    _lib.check(rc, "tn_texture_rays")


def vertex_call(rgbt: Tensor, faces: Tensor, px: int, texel0: int, count: int, out: Tensor) -> None:
    """tn_texture_vertex of texels [texel0, texel0 + count) into out [count,4]"""
    V, p_faces, Fn = _mesh_args(rgbt, faces)
    rc = _lib.load().tn_texture_vertex(_contig(rgbt, "vertex rgbt", (V, 4)), V, p_faces, Fn, int(px), int(texel0), int(count),
                                       _contig(out, "texel rgbt", (count, 4)), _stream())
    _lib.check(rc, "tn_texture_vertex")


def store_call(rgb: Tensor, thermal: Tensor, texel0: int, rgb_image: Tensor, thermal_image: Tensor, float_image: Optional[Tensor]) -> None:
    """tn_texture_store of a chunk's rgb [n,3] and thermal [n,1] (strided views are read in place) into the images [H,W,3] / [H,W] uint8 and, unless
    None, [H,W,4] fp32, at texel0"""
    n = rgb.shape[0]
    H, W = thermal_image.shape
    rgb, p_rgb, s_rgb = _rows(rgb, "rgb", n, 3)  # (a copy _rows had to make is held here until the call is enqueued)
    thermal, p_th, s_th = _rows(thermal, "thermal", n, 1)
    rc = _lib.load().tn_texture_store(p_rgb, s_rgb, p_th, s_th, n, int(texel0), H * W, _contig(rgb_image, "rgb image", (H, W, 3), torch.uint8),
                                      _contig(thermal_image, "thermal image", (H, W), torch.uint8),
                                      None if float_image is None else _contig(float_image, "float image", (H, W, 4)), _stream())
    _lib.check(rc, "tn_texture_store")


def mean_edge_call(vertices: Tensor, faces: Tensor, mean: Tensor) -> None:
    """tn_mesh_mean_edge: the mean length of the first edge of every face into `mean` (device fp32 [1])"""
    V, p_faces, Fn = _mesh_args(vertices, faces)
    need = int(_lib.load().tn_mesh_mean_edge_workspace_bytes(Fn))
    if need < 0:
        raise ValueError(f"tn_mesh_mean_edge_workspace_bytes({Fn}): a size the library refuses")
    ws = torch.empty(need, dtype=torch.uint8, device=vertices.device)
    rc = _lib.load().tn_mesh_mean_edge(_contig(vertices, "vertices", (V, 3)), V, p_faces, Fn, _contig(mean, "mean", (1,)), C.c_void_p(ws.data_ptr()),
                                       ws.numel(), _stream())
    _lib.check(rc, "tn_mesh_mean_edge")


# ---------------------------------------------------------------------------------------------------- unwrap and bake
def atlas_layout(num_faces: int, px_per_uv_triangle: int) -> Tuple[int, int, int, int]:
    """(W, H, squares_w, squares_h) of the atlas of num_faces faces: squares = ceil(F / 2) of (px + 3) x px texels, squares_w = ceil(sqrt(squares)),
    squares_h = ceil(squares / squares_w)."""
    return layout_call(num_faces, px_per_uv_triangle)


def _checked(mesh: Mesh, px: int):
    Fn = int(mesh.faces.shape[0])
    W, H, _, _ = atlas_layout(Fn, px)
    _dev(mesh.vertices, "vertices"), _dev(mesh.faces, "faces", torch.int32)
    return Fn, W, H


def texture_coordinates(num_faces: int, px_per_uv_triangle: int, device="cuda") -> Tensor:
    """[F,3,2] fp32: the reference's texture coordinates, evaluated in double and rounded once."""
    atlas_layout(num_faces, px_per_uv_triangle)
    tc = torch.empty((int(num_faces), 3, 2), dtype=F32, device=device)
    coords_call(int(num_faces), px_per_uv_triangle, tc)
    return tc


def mesh_raylen(mesh: Mesh, raylen_method: str = "edge") -> float:
    """The length of the rays a texel is rendered with: "edge", the reference's default, twice the mean length of the first edge of every face (double
    sums in a fixed order, returned as fp32; one read-back); "none", 0."""
    if raylen_method not in RAYLEN_METHODS:
        raise ValueError(f"Ray length method {raylen_method} not supported.")
    if raylen_method == "none":
        return 0.0
    mean = torch.empty(1, dtype=F32, device=mesh.vertices.device)
    mean_edge_call(mesh.vertices, mesh.faces, mean)
    return 2.0 * float(mean.item())


def unwrap_mesh(mesh: Mesh, px_per_uv_triangle: int) -> Tuple[Tensor, Tensor, Tensor]:
    """unwrap_mesh_per_uv_triangle (texture_utils.py:78-209) -> (texture_coordinates [F,3,2], origins [H,W,3], directions [H,W,3]): per texel the
    surface point and the negated, normalised interpolated normal.  The whole image at once, for tests and parity with the reference's interface
    (raylen 0); bake_texture emits the same rays a chunk at a time.  Texels no face owns take the last face's plane: finite, and never sampled."""
    Fn, W, H = _checked(mesh, px_per_uv_triangle)
    dev = mesh.vertices.device
    origins, directions = torch.empty((H * W, 3), dtype=F32, device=dev), torch.empty((H * W, 3), dtype=F32, device=dev)
    rays_call(mesh.vertices, mesh.normals, mesh.faces, px_per_uv_triangle, 0.0, 0, H * W, origins, directions)
    return texture_coordinates(Fn, px_per_uv_triangle, dev), origins.view(H, W, 3), directions.view(H, W, 3)


def bake_texture(mesh: Mesh, model=None, px_per_uv_triangle: int = 4, source: str = "nerf", raylen_method: str = "edge", chunk: Optional[int] = None,
                 return_float: bool = False) -> Texture:
    """export_textured_mesh (texture_utils.py:323-411) up to the texture image, with the thermal channel beside the colours.

    source "nerf" (a ThermalNerfactoModel): per chunk of `chunk` texels (default: the model's eval_num_rays_per_chunk) tn_texture_rays emits the rays
    -- from the surface point, raylen / 2 back along the interpolated normal, looking at the surface --, the model renders them as its eval render does
    (pixel_area 1 and camera index 0, as the reference passes; eval mode under no_grad, the model's mode is restored) and tn_texture_store writes
    `rgb` and `rgb_thermal` into the images.  Near and far planes are the model's own at inference, 0 and far_plane: the reference sets nears = 0 and
    fars = raylen on its bundle, and its NearFarCollider then overwrites both (scene_colliders.py:186-190), so this is what the reference renders too.
    The ray starts raylen / 2 outside the surface and the first surface it meets is the mesh's.  The engine has no per-ray near / far path, and none is
    added.  Rays are rendered independently, so the chunk size does not change a byte.
    source "vertex": the mesh's own per-vertex RGB+T spread over the atlas (tn_texture_vertex); no model, no rays, raylen 0.
    A thermal splat model has no ray render: source "nerf" raises NotImplementedError for it; use "vertex"."""
    if source not in SOURCES:
        raise ValueError(f"bake_texture: source = {source!r}, one of {SOURCES}")
    if raylen_method not in RAYLEN_METHODS:
        raise ValueError(f"Ray length method {raylen_method} not supported.")
    px = int(px_per_uv_triangle)
    Fn, W, H = _checked(mesh, px)
    total = H * W
    if source == "nerf":
        if model is None:
            raise ValueError('bake_texture: source "nerf" needs the model')
        if _is_splat(model):
            raise NotImplementedError('bake_texture: source "nerf" renders rays through a radiance field, which a splat model does not have; use '
                                      'source="vertex" for meshes exported from thermal splats')
        chunk = int(model.config.eval_num_rays_per_chunk if chunk is None else chunk)
    else:
        chunk = total if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError(f"bake_texture: chunk = {chunk}")
    dev = mesh.vertices.device
    tex = Texture(torch.empty((H, W, 3), dtype=torch.uint8, device=dev), torch.empty((H, W), dtype=torch.uint8, device=dev),
                  texture_coordinates(Fn, px, dev), 0.0, torch.empty((H, W, 4), dtype=F32, device=dev) if return_float else None)
    if source == "vertex":
        _dev(mesh.rgbt, "vertex rgbt")
        rgbt = mesh.rgbt.contiguous()
        for t0 in range(0, total, chunk):
            n = min(chunk, total - t0)
            out = torch.empty((n, 4), dtype=F32, device=dev)
            vertex_call(rgbt, mesh.faces, px, t0, n, out)
            store_call(out[:, :3], out[:, 3:], t0, tex.rgb, tex.thermal, tex.rgbt)
        return tex
    tex.raylen = mesh_raylen(mesh, raylen_method)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for t0 in range(0, total, chunk):
                n = min(chunk, total - t0)
                origins, directions = torch.empty((n, 3), dtype=F32, device=dev), torch.empty((n, 3), dtype=F32, device=dev)
                rays_call(mesh.vertices, mesh.normals, mesh.faces, px, tex.raylen, t0, n, origins, directions)
                bundle = RayBundle(origins=origins, directions=directions, pixel_area=torch.ones((n, 1), dtype=F32, device=dev),
                                   camera_indices=torch.zeros((n, 1), dtype=torch.int64, device=dev))
                outputs = model(bundle)
                rgb, thermal = outputs["rgb"], outputs["rgb_thermal"]
                store_call(rgb if rgb.dim() == 2 else rgb.reshape(n, 3), thermal if thermal.dim() == 2 else thermal.reshape(n, 1), t0, tex.rgb,
                           tex.thermal, tex.rgbt)
    finally:
        model.train(was_training)
    return tex


# ---------------------------------------------------------------------------------------------------- files
def png_bytes(image: np.ndarray) -> bytes:
    """An 8-bit PNG of a uint8 image [H,W,3] (RGB) or [H,W] (grey), with the standard library only: rows unfiltered, one IDAT."""
    if image.dtype != np.uint8 or image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3):
        raise ValueError(f"png_bytes: a uint8 [H,W,3] or [H,W] image, got {image.dtype} {image.shape}")
    H, W = image.shape[:2]
    rows = np.zeros((H, 1 + W * (3 if image.ndim == 3 else 1)), dtype=np.uint8)  # a filter byte of 0 in front of every row
    rows[:, 1:] = image.reshape(H, -1)

    def chunk(kind: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    head = struct.pack(">IIBBBBB", W, H, 8, 2 if image.ndim == 3 else 0, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", head) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b"")


def read_png(path: str) -> np.ndarray:
    """The image of a PNG written by png_bytes -> uint8 [H,W,3] or [H,W] (8 bits, RGB or grey, unfiltered rows, not interlaced: nothing else)."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG")
    at, idat, head = 8, b"", None
    while at < len(data):
        (size,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + size]
        if struct.unpack(">I", data[at + 8 + size:at + 12 + size])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError(f"{path}: a {kind!r} chunk fails its checksum")
        head, idat = (body if kind == b"IHDR" else head), (idat + body if kind == b"IDAT" else idat)
        at += 12 + size
    W, H, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", head)
    if depth != 8 or colour not in (0, 2) or interlace != 0:
        raise ValueError(f"{path}: {depth} bits, colour type {colour}, interlace {interlace}")
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, -1)
    if rows[:, 0].any():
        raise ValueError(f"{path}: filtered rows")
    return rows[:, 1:].reshape((H, W, 3) if colour == 2 else (H, W)).copy()


def _lines(prefix: str, columns, sep: str = " ") -> str:
    """One line per row: prefix, then the columns (arrays of strings) joined by sep; built with numpy's string operations, no loop per line."""
    text = np.char.add(prefix, columns[0])
    for c in columns[1:]:
        text = np.char.add(np.char.add(text, sep), c)
    return "\n".join(text.tolist()) + ("\n" if len(text) else "")


def write_textured_obj(directory: str, mesh: Mesh, texture: Texture, dataparser_outputs=None, applied_transform=None, usemtl: str = "rgb") -> Dict[str, str]:
    """The files export_textured_mesh writes (texture_utils.py:409-482), plus the thermal texture: `mesh.obj` -- `v x y z` per vertex, `vt u (1 - v)`
    per face corner, `vn x y z` per vertex, `f v/vt/vn` three times per face with vt = 3 f + 1 .. 3 f + 3 and vn = v, all indices 1-based, in this
    order --, `material_0.mtl` with the reference's block `material_0` (map_Kd material_0.png) and a second block `material_thermal` (map_Kd
    material_0_thermal.png), and the two 8-bit PNGs, RGB and grey (png_bytes: zlib and struct only).  usemtl names the material the OBJ uses: "rgb" or
    "thermal".  With dataparser_outputs the mesh is written in the dataset's frame (mesh.mesh_to_dataset_frame; where that swaps the winding, the
    texture coordinates of the two swapped corners go with them).  Numbers are written in the shortest form that reads back to the same float32.
    -> the paths, by "obj", "mtl", "rgb", "thermal"."""
    if usemtl not in MATERIALS:
        raise ValueError(f"write_textured_obj: usemtl = {usemtl!r}, one of {tuple(MATERIALS)}")
    tc = texture.texture_coordinates
    if tuple(tc.shape) != (mesh.faces.shape[0], 3, 2):
        raise ValueError(f"write_textured_obj: texture coordinates {tuple(tc.shape)} for {mesh.faces.shape[0]} faces")
    if dataparser_outputs is not None:
        moved = mesh_to_dataset_frame(mesh, dataparser_outputs, applied_transform)
        if moved.faces is not mesh.faces:  # mirrored: corners 1 and 2 changed places
            tc = tc[:, [0, 2, 1]]
        mesh = moved
    os.makedirs(directory, exist_ok=True)
    paths = {"obj": os.path.join(directory, "mesh.obj"), "mtl": os.path.join(directory, "material_0.mtl"),
             "rgb": os.path.join(directory, MATERIALS["rgb"][1]), "thermal": os.path.join(directory, MATERIALS["thermal"][1])}
    with open(paths["rgb"], "wb") as f:
        f.write(png_bytes(texture.rgb.detach().cpu().numpy()))
    with open(paths["thermal"], "wb") as f:
        f.write(png_bytes(texture.thermal.detach().cpu().numpy()))
    block = ["Ka 1.000 1.000 1.000", "Kd 1.000 1.000 1.000", "Ks 0.000 0.000 0.000", "d 1.0", "illum 2", "Ns 1.00000000"]
    mtl = ["# Generated with nerfstudio-thermal_amd"]
    for name, image in MATERIALS.values():
        mtl += [f"newmtl {name}"] + block + [f"map_Kd {image}"]
    with open(paths["mtl"], "w", encoding="utf-8") as f:
        f.write("\n".join(mtl) + "\n")
    text = lambda a: np.ascontiguousarray(a).astype(str)  # noqa: E731  (float32 -> its shortest repr)
    v = text(mesh.vertices.detach().float().cpu().numpy())
    vn = text(mesh.normals.detach().float().cpu().numpy())
    uv = tc.detach().float().cpu().numpy().reshape(-1, 2)
    faces = mesh.faces.detach().cpu().numpy().astype(np.int64) + 1
    vt = np.arange(1, 3 * faces.shape[0] + 1, dtype=np.int64).reshape(-1, 3)
    corner = [np.char.add(np.char.add(np.char.add(np.char.add(text(faces[:, k]), "/"), text(vt[:, k])), "/"), text(faces[:, k])) for k in range(3)]
    with open(paths["obj"], "w", encoding="utf-8") as f:
        f.write(f"# Generated with nerfstudio-thermal_amd\nmtllib material_0.mtl\nusemtl {MATERIALS[usemtl][0]}\n")
        f.write(_lines("v ", [v[:, 0], v[:, 1], v[:, 2]]))
        f.write(_lines("vt ", [text(uv[:, 0]), text(np.float32(1.0) - uv[:, 1])]))
        f.write(_lines("vn ", [vn[:, 0], vn[:, 1], vn[:, 2]]))
        f.write(_lines("f ", corner))
    return paths


def read_textured_obj(directory: str) -> Dict[str, object]:
    """What write_textured_obj wrote -> vertices [V,3], normals [V,3], vt [3F,2] (as in the file: v counts from the bottom) fp32; faces, face_vt,
    face_vn [F,3] int64, 0-based; usemtl (the material's name); materials {name: map_Kd file}; rgb uint8 [H,W,3] and thermal uint8 [H,W]; order, the
    kinds of the OBJ's lines in the order they first appear."""
    with open(os.path.join(directory, "mesh.obj"), encoding="utf-8") as f:
        lines = [ln.split() for ln in f.read().splitlines() if ln and not ln.startswith("#")]
    order = []
    for ln in lines:
        if ln[0] not in order:
            order.append(ln[0])
    rows = lambda kind, width: np.array([ln[1:] for ln in lines if ln[0] == kind], dtype=np.float32).reshape(-1, width)  # noqa: E731
    corners = np.array([[c.split("/") for c in ln[1:]] for ln in lines if ln[0] == "f"], dtype=np.int64).reshape(-1, 3, 3) - 1
    materials, name = {}, None
    with open(os.path.join(directory, next(ln[1] for ln in lines if ln[0] == "mtllib")), encoding="utf-8") as f:
        for ln in f.read().splitlines():
            part = ln.split()
            if part[:1] == ["newmtl"]:
                name = part[1]
            elif part[:1] == ["map_Kd"]:
                materials[name] = part[1]
    return {"vertices": rows("v", 3), "normals": rows("vn", 3), "vt": rows("vt", 2), "faces": corners[:, :, 0], "face_vt": corners[:, :, 1],
            "face_vn": corners[:, :, 2], "usemtl": next(ln[1] for ln in lines if ln[0] == "usemtl"), "materials": materials, "order": order,
            "rgb": read_png(os.path.join(directory, materials[MATERIALS["rgb"][0]])),
            "thermal": read_png(os.path.join(directory, materials[MATERIALS["thermal"][0]]))}
