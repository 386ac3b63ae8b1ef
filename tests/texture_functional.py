"""The texture atlas of the mesh export restated in plain torch (nerfstudio/exporter/texture_utils.py, unwrap_method "custom", and the ray length and
origin offset of export_textured_mesh).

`unwrap_ref` follows the reference's formula operation by operation with a `dtype` argument: the texture coordinates from the scaled corner table and
the square offsets, the texel centres from linspace, barycentric weights as ratios of UV parallelogram areas.  In float32 every tensor has the dtype the
reference's own code gives it (its Python scalars stay doubles there as here), so the result is the reference's rounding; in float64 it is the formula
itself, UV areas included.  `integer_weights` is what the kernels compute instead: the corners lie on texel centres, so the weights are small integers
over px - 1.  `owned` marks the texels a texture coordinate can address.  `bilinear` samples a texture the way a renderer does."""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

F32, F64 = torch.float32, torch.float64
GAP = 3  # texels between the two triangles of a square
CASES = ((1, 2), (2, 2), (3, 2), (7, 4), (37, 4), (201, 3), (1000, 4), (5, 7))  # (faces, px_per_uv_triangle)


def layout(F: int, px: int):
    """-> (W, H, squares_w, squares_h)"""
    squares = -(-F // 2)
    sw = math.ceil(math.sqrt(squares))
    sh = math.ceil(squares / sw)
    return sw * (px + GAP), sh * px, sw, sh


def case_mesh(F: int, seed=None):
    """The test mesh of a case: vertices uniform in [-1, 1]^3, faces as random vertex triples, normals normalize(randn + (0, 0, 3)); seeded by F."""
    g = torch.Generator().manual_seed(F if seed is None else seed)
    V = max(4, F // 2 + 3)
    vertices = torch.rand((V, 3), generator=g) * 2.0 - 1.0
    faces = torch.randint(0, V, (F, 3), generator=g, dtype=torch.int64)
    normals = Fn.normalize(torch.randn((V, 3), generator=g) + torch.tensor([0.0, 0.0, 3.0]), dim=-1)
    return vertices, faces, normals


def texel_grid(F: int, px: int, device=None):
    """Integer images [H,W]: the unclamped face index 2 square + lower, the local offsets i and j, and whether the texel is in the lower-right triangle."""
    W, H, sw, _ = layout(F, px)
    x, y = torch.meshgrid(torch.arange(W, device=device), torch.arange(H, device=device), indexing="xy")
    i, j = x % (px + GAP), y % px
    lower = (i + j) >= (px + GAP - 2)
    square = torch.div(y, px, rounding_mode="floor") * sw + torch.div(x, px + GAP, rounding_mode="floor")
    return square * 2 + lower.long(), i, j, lower


def owned(F: int, px: int):
    """[H,W] bool: the texels whose own face exists."""
    return texel_grid(F, px)[0] < F


def owned_count(F: int, px: int) -> int:
    """The layout's own figure: every face owns half a square, (px + 3) px / 2 texels -- the diagonal rule i + j >= px + 1 splits the (px + 3) x px
    square into two halves of equal size (the map (i, j) -> (px + 2 - i, px - 1 - j) swaps them)."""
    return F * (px + GAP) * px // 2


def integer_weights(F: int, px: int):
    """-> (face [H,W] clamped to F - 1, w0, w1, w2 [H,W] float64): the weights as the kernels compute them."""
    face, i, j, lower = texel_grid(F, px)
    den = float(px - 1)
    w1 = torch.where(lower, px + 2 - i, i).double() / den
    w2 = torch.where(lower, px - 1 - j, j).double() / den
    return face.clamp(max=F - 1), (1.0 - w1) - w2, w1, w2


def _area2(p, a, b):
    """twice the signed area of (p, a, b) in the UV plane"""
    return (p[..., 0] - a[..., 0]) * (b[..., 1] - a[..., 1]) - (p[..., 1] - a[..., 1]) * (b[..., 0] - a[..., 0])


def texture_coordinates_ref(F: int, px: int, dtype=F64, device=None):
    """[F,3,2]: per square the upper-left triangle (0, 0), (e, 0), (0, e) and the lower-right one (far corner, its left neighbour on the bottom edge, its
    upper neighbour on the right edge), each pulled towards its right-angle corner by (px - 1) / px and moved half a texel inside, plus the square's
    offset."""
    W, H, sw, sh = layout(F, px)
    t = lambda v: torch.tensor(v, dtype=dtype, device=device)  # noqa: E731
    cell_w, cell_h, tx_w, tx_h = (px + GAP) / W, px / H, 1.0 / W, 1.0 / H
    cell, half = t([cell_w, cell_h]), t([tx_w, tx_h]) / 2
    shrink = (px - 1) / px
    upper = t([[0, 0], [px / W, 0], [0, px / H]]) * shrink + half
    far = t([cell_w, cell_h])
    lower = (t([[cell_w, cell_h], [GAP * tx_w, cell_h], [cell_w, 0]]) - far) * shrink + far - half
    six = torch.stack([upper, lower], dim=0).reshape(1, 1, 6, 2)
    offsets = torch.stack(torch.meshgrid(torch.arange(sw, device=device), torch.arange(sh, device=device), indexing="xy"), dim=-1) * cell
    return (six + offsets.view(sh, sw, 1, 2)).view(-1, 3, 2)[:F]


def reference_weights(F: int, px: int, dtype=F64, device=None):
    """-> (face [H,W] clamped, w0, w1, w2 [H,W]) by the reference's formula: ratios of UV areas at the texel centres."""
    W, H, _, _ = layout(F, px)
    tc = texture_coordinates_ref(F, px, dtype, device)
    tx_w, tx_h = 1.0 / W, 1.0 / H
    us = torch.linspace(tx_w / 2, 1 - tx_w / 2, W, dtype=dtype, device=device)
    vs = torch.linspace(tx_h / 2, 1 - tx_h / 2, H, dtype=dtype, device=device)
    p = torch.stack(torch.meshgrid(us, vs, indexing="xy"), dim=-1)
    face = texel_grid(F, px, device)[0].clamp(min=0, max=F - 1)
    uv = tc[face]
    a, b, c = uv[..., 0, :], uv[..., 1, :], uv[..., 2, :]
    area = _area2(c, a, b)
    return face, _area2(p, b, c) / area, _area2(p, c, a) / area, _area2(p, a, b) / area


def _blend(values, faces, face, w0, w1, w2):
    corner = values[faces[face]]  # [H,W,3,C]
    return corner[..., 0, :] * w0[..., None] + corner[..., 1, :] * w1[..., None] + corner[..., 2, :] * w2[..., None]


def unwrap_ref(vertices, faces, normals, px: int, dtype=F64, weights=None):
    """-> (texture_coordinates [F,3,2], origins [H,W,3], directions [H,W,3]) in `dtype`, on the device of `vertices`; weights: reference_weights
    (default) or integer_weights."""
    F, device = faces.shape[0], vertices.device
    face, w0, w1, w2 = (reference_weights(F, px, dtype, device) if weights is None else weights)
    w0, w1, w2 = w0.to(dtype), w1.to(dtype), w2.to(dtype)
    origins = _blend(vertices.to(dtype), faces.long(), face, w0, w1, w2)
    directions = Fn.normalize(-_blend(normals.to(dtype), faces.long(), face, w0, w1, w2), dim=-1)
    return texture_coordinates_ref(F, px, dtype, device), origins, directions


def normal_length(normals, faces, px: int):
    """[H,W] float64: the length of the interpolated normal before it is normalised (float64 formula)."""
    F = faces.shape[0]
    face, w0, w1, w2 = reference_weights(F, px, F64)
    return _blend(normals.double(), faces.long(), face, w0, w1, w2).norm(dim=-1)


def raylen_ref(vertices, faces, dtype=F64):
    """export_textured_mesh's raylen_method "edge": twice the mean length of the first edge of every face."""
    fv = vertices.to(dtype)[faces.long()]
    return 2.0 * torch.mean(torch.norm(fv[:, 1, :] - fv[:, 0, :], dim=-1))


def offset_origins(origins, directions, raylen: float):
    """The rays start raylen / 2 outside the surface."""
    return origins - 0.5 * raylen * directions


def vertex_texture_ref(rgbt, faces, px: int):
    """[H,W,C] float64: the per-vertex values spread over the atlas with the integer weights."""
    return _blend(rgbt.double(), faces.long(), *integer_weights(faces.shape[0], px))


def to_bytes(values):
    """rint(255 clamp(v, 0, 1)) as cloud.to_uint8 evaluates it, in float32"""
    return torch.clamp(values.float() * 255.0, 0.0, 255.0).round().to(torch.uint8)


def bilinear(image, uv):
    """image [H,W,C], uv [...,2] with u to the right and v down, both in 0..1 over the whole image (texel centres at (k + 0.5) / size) -> [...,C] in
    float64, indices clamped to the image."""
    H, W = image.shape[:2]
    img = image.double()
    x, y = uv[..., 0].double() * W - 0.5, uv[..., 1].double() * H - 0.5
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    xi = lambda v: v.long().clamp(0, W - 1)  # noqa: E731
    yi = lambda v: v.long().clamp(0, H - 1)  # noqa: E731
    top = img[yi(y0), xi(x0)] * (1 - fx) + img[yi(y0), xi(x0 + 1)] * fx
    bottom = img[yi(y0 + 1), xi(x0)] * (1 - fx) + img[yi(y0 + 1), xi(x0 + 1)] * fx
    return top * (1 - fy) + bottom * fy


def cube_mesh(half: float = 0.35, split: int = 3):
    """A cube of half-size `half`, each side split into split x split quads of two triangles, with its own vertices per side and flat outward normals:
    -> (vertices [V,3], faces [F,3] int64, normals [V,3]); 6 * split^2 * 2 faces, wound so that the face normal points out."""
    verts, faces, normals = [], [], []
    lin = np.linspace(-half, half, split + 1)
    for axis in range(3):
        for sign in (-1.0, 1.0):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            base = len(verts)
            for ia in range(split + 1):
                for ib in range(split + 1):
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[a], p[b] = sign * half, lin[ia], lin[ib]
                    n = [0.0, 0.0, 0.0]
                    n[axis] = sign
                    verts.append(p), normals.append(n)
            at = lambda ia, ib: base + ia * (split + 1) + ib  # noqa: E731
            for ia in range(split):
                for ib in range(split):
                    q = [at(ia, ib), at(ia + 1, ib), at(ia + 1, ib + 1), at(ia, ib + 1)]  # counter-clockwise seen from +axis
                    if sign < 0:
                        q = q[::-1]
                    faces.append([q[0], q[1], q[2]]), faces.append([q[0], q[2], q[3]])
    return (torch.tensor(verts, dtype=F32), torch.tensor(faces, dtype=torch.int64), torch.tensor(normals, dtype=F32))
