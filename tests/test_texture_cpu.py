"""Texture baking without a GPU: the float32 restatement of the reference's atlas unwrap (texture_functional.unwrap_ref) against the reference's
recorded outputs (tests/golden/texture_reference.npz, scripts/make_golden_texture.py) and, where its tree is present, the live reference; the integer
weights the kernels compute against the float64 formula; the layout arithmetic of the library's host entry point; the OBJ / MTL / PNG round trip; and
the host-side argument checks of the entry points."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest
import torch

import texture_functional as xf
from nerfstudio_thermal_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "texture_reference.npz")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

F32, F64 = torch.float32, torch.float64
# The float32 restatement against the reference's float32 outputs.  Measured here: 0 on all three outputs in all eight cases, against the golden
# file and against the live reference (bit-equal).  Texture coordinates and origins are element-wise products and sums, which IEEE arithmetic fixes: they
# are asserted bit-equal.  The directions go through F.normalize, whose 3-term sum of squares a library may order differently on another CPU: with
# |d| <= 1 two orders differ by at most 2 ulp of the squared length, 1 ulp of the length, and so 2 ulp of 1 in a component after the division; the bound
# is that, 2 * 2^-23.
DIRECTION_TOL = 2.0 * 2.0 ** -23


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def golden_case(F, px):
    g = np.load(GOLDEN)
    key = f"F{F}_px{px}"
    return {name: torch.from_numpy(g[f"{key}_{name}"]) for name in ("vertices", "faces", "normals", "texture_coordinates", "origins", "directions")}


def _texture():
    from nerfstudio_thermal_amd import texture

    return texture


# ---------------------------------------------------------------------------------------------------- 1. the restatement and the reference
def test_golden_file_holds_the_cases():
    g = np.load(GOLDEN)
    assert [tuple(c) for c in g["cases"].tolist()] == list(xf.CASES)
    assert os.path.getsize(GOLDEN) < 1 << 20
    for F, px in xf.CASES:
        c = golden_case(F, px)
        W, H, _, _ = xf.layout(F, px)
        assert c["origins"].shape == (H, W, 3) and c["directions"].shape == (H, W, 3) and c["texture_coordinates"].shape == (F, 3, 2)
        assert c["faces"].shape == (F, 3) and int(c["faces"].min()) >= 0 and int(c["faces"].max()) < c["vertices"].shape[0]


def _assert_restatement(c, tc, origins, directions, px, label):
    got = xf.unwrap_ref(c["vertices"], c["faces"], c["normals"], px, F32)
    err = [float((a.double() - b.double()).abs().max()) for a, b in zip(got, (tc, origins, directions))]
    print(f"{label}: float32 restatement misses the reference by {err[0]:.3g} (texture coordinates), {err[1]:.3g} (origins), {err[2]:.3g} (directions)")
    assert all(a.dtype == F32 for a in got)
    assert err[0] == 0.0 and err[1] == 0.0
    assert err[2] <= DIRECTION_TOL


@pytest.mark.parametrize("F,px", xf.CASES)
def test_float32_restatement_matches_the_recorded_reference(F, px):
    c = golden_case(F, px)
    _assert_restatement(c, c["texture_coordinates"], c["origins"], c["directions"], px, f"F={F} px={px} golden")


@pytest.mark.skipif(not ref_import.reference_available(), reason="reference tree not present")
@pytest.mark.parametrize("F,px", xf.CASES)
def test_float32_restatement_matches_the_live_reference(F, px):
    ref_import.install_extended_stubs()
    for name in ("mediapy", "xatlas", "pymeshlab"):
        if name not in sys.modules:
            ref_import._perm_mod(name)
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    from nerfstudio.exporter.texture_utils import unwrap_mesh_per_uv_triangle

    c = golden_case(F, px)
    tc, origins, directions = unwrap_mesh_per_uv_triangle(c["vertices"], c["faces"].long(), c["normals"], px)
    assert torch.equal(tc, c["texture_coordinates"]) and torch.equal(origins, c["origins"])  # the golden file is this reference's output
    _assert_restatement(c, tc, origins, directions, px, f"F={F} px={px} live")


@pytest.mark.parametrize("F,px", xf.CASES)
def test_case_inputs_are_the_seeded_ones_and_normals_stay_long(F, px):
    """The recorded inputs are case_mesh(F); over the owned texels the interpolated normal keeps a length of at least 0.25 (float64 formula), so the
    normalisation does not amplify rounding in the comparisons of directions."""
    c = golden_case(F, px)
    v, f, n = xf.case_mesh(F)
    assert torch.equal(v, c["vertices"]) and torch.equal(f.int(), c["faces"]) and torch.equal(n, c["normals"])
    shortest = float(xf.normal_length(c["normals"], c["faces"], px)[xf.owned(F, px)].min())
    print(f"F={F} px={px}: shortest interpolated normal over owned texels {shortest:.4f}")
    assert shortest >= 0.25


# ---------------------------------------------------------------------------------------------------- 2. the integer weights
@pytest.mark.parametrize("px", [2, 3, 4, 7])
@pytest.mark.parametrize("F", [1, 2, 3, 5, 7, 37, 201, 1000])
def test_integer_weights_are_the_reference_formula(F, px):
    face_i, *wi = xf.integer_weights(F, px)
    face_r, *wr = xf.reference_weights(F, px, F64)
    own = xf.owned(F, px)
    assert torch.equal(face_i, face_r)
    assert int(own.sum()) == xf.owned_count(F, px)
    err = max(float((a - b)[own].abs().max()) for a, b in zip(wi, wr))
    assert err <= 1e-12, err
    assert all(bool(torch.isfinite(w).all()) for w in wi)
    # corners lie on texel centres: sampling the integer-weight plane at a face's texture coordinates gives its three vertices
    W, H, _, _ = xf.layout(F, px)
    tc = xf.texture_coordinates_ref(F, px, F64)
    ids = torch.arange(F)
    for k in range(3):
        x, y = (tc[:, k, 0] * W - 0.5), (tc[:, k, 1] * H - 0.5)
        xi, yi = x.round().long(), y.round().long()
        assert float((x - xi).abs().max()) < 1e-9 and float((y - yi).abs().max()) < 1e-9
        assert torch.equal(face_i[yi, xi], ids)
        want = [1.0 if j == k else 0.0 for j in range(3)]
        assert all(float((wi[j][yi, xi] - want[j]).abs().max()) < 1e-12 for j in range(3))


# ---------------------------------------------------------------------------------------------------- 3. layout
def test_layout_arithmetic(lib):
    texture = _texture()
    assert texture.atlas_layout(1, 2) == (5, 2, 1, 1)
    assert texture.atlas_layout(2, 2) == (5, 2, 1, 1)
    assert texture.atlas_layout(3, 2) == (10, 2, 2, 1)
    assert texture.atlas_layout(7, 4) == (14, 8, 2, 2)
    assert texture.atlas_layout(201, 3) == (66, 30, 11, 10)
    for F in list(range(1, 70)) + [199, 200, 201, 1000, 2 * 49, 2 * 49 + 1, 100_003, 10 ** 6, 2 * 4097 ** 2, 2 * 4097 ** 2 + 1, (2 ** 31 - 1) // 3]:
        for px in (2, 3, 4, 7, 64):
            W, H, sw, sh = texture.atlas_layout(F, px)
            assert (W, H, sw, sh) == xf.layout(F, px), (F, px)
            squares = -(-F // 2)
            assert sw * sh >= squares > sw * (sh - 1) and (sw - 1) ** 2 < squares <= sw ** 2
    out = (C.c_int64 * 4)()
    assert lib.tn_texture_layout(4, 4, None) == -22 and b"null pointer" in lib.tn_last_error()
    assert lib.tn_texture_layout(0, 4, out) == -22 and lib.tn_texture_layout(4, 1, out) == -22 and b"texels per triangle" in lib.tn_last_error()
    assert lib.tn_texture_layout((2 ** 31 - 1) // 3 + 1, 4, out) == -22


def test_too_small_sizes_raise(lib):
    """px_per_uv_triangle = 1 (the reference's scale (px - 1) / px is 0 there and it returns NaN) and an empty mesh are a ValueError before any launch."""
    texture = _texture()
    from nerfstudio_thermal_amd.mesh import Mesh

    v, f, n = xf.cube_mesh()
    mesh = Mesh(v, f.int(), n, torch.zeros((v.shape[0], 4)))
    empty = Mesh(v, f.int()[:0], n, torch.zeros((v.shape[0], 4)))
    for fn in (lambda m, px: texture.atlas_layout(m.faces.shape[0], px), texture.unwrap_mesh,
               lambda m, px: texture.bake_texture(m, None, px, source="vertex"), lambda m, px: texture.texture_coordinates(m.faces.shape[0], px, "cpu")):
        for m, px in ((mesh, 1), (mesh, 0), (mesh, -3), (empty, 4)):
            with pytest.raises(ValueError, match="px_per_uv_triangle"):
                fn(m, px)
    with pytest.raises(ValueError, match="source"):
        texture.bake_texture(mesh, None, 4, source="xatlas")
    with pytest.raises(ValueError, match="not supported"):
        texture.bake_texture(mesh, None, 4, source="vertex", raylen_method="mean")
    with pytest.raises(ValueError, match="no CPU fallback"):
        texture.unwrap_mesh(mesh, 4)


# ---------------------------------------------------------------------------------------------------- 4. files
def _decode_png(path):
    """An independent decoder of the subset the writer produces: chunks by hand, zlib, filter type 0."""
    import struct

    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        size = struct.unpack(">I", data[at:at + 4])[0]
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + size]
        assert struct.unpack(">I", data[at + 8 + size:at + 12 + size])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        at += 12 + size
    assert [k for k, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, comp, filt, inter = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, inter) == (8, 0, 0, 0) and colour in (0, 2)
    raw = np.frombuffer(zlib.decompress(b"".join(b for k, b in chunks if k == b"IDAT")), dtype=np.uint8).reshape(H, 1 + W * (3 if colour == 2 else 1))
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape((H, W, 3) if colour == 2 else (H, W))


@pytest.mark.parametrize("usemtl", ["rgb", "thermal"])
def test_textured_obj_round_trip(tmp_path, usemtl):
    texture = _texture()
    from nerfstudio_thermal_amd.mesh import Mesh

    v, f, n = xf.cube_mesh()
    Fn, px = f.shape[0], 4
    mesh = Mesh(v, f.int(), n, torch.zeros((v.shape[0], 4)))
    W, H, _, _ = xf.layout(Fn, px)
    g = torch.Generator().manual_seed(3)
    tex = texture.Texture(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8), torch.randint(0, 256, (H, W), generator=g, dtype=torch.uint8),
                          xf.texture_coordinates_ref(Fn, px, F64).float(), 0.25)
    paths = texture.write_textured_obj(str(tmp_path), mesh, tex, usemtl=usemtl)
    assert sorted(os.path.basename(p) for p in paths.values()) == ["material_0.mtl", "material_0.png", "material_0_thermal.png", "mesh.obj"]
    # the raw text: the reference's line kinds in its order, 1-based indices, vt = 3 f + 1 .. 3 f + 3, vn = v
    lines = [ln for ln in open(paths["obj"]).read().splitlines() if not ln.startswith("#")]
    assert lines[0] == "mtllib material_0.mtl" and lines[1] == "usemtl " + {"rgb": "material_0", "thermal": "material_thermal"}[usemtl]
    kinds = [ln.split()[0] for ln in lines[2:]]
    V = v.shape[0]
    assert kinds == ["v"] * V + ["vt"] * (3 * Fn) + ["vn"] * V + ["f"] * Fn
    first, last = lines[2 + 2 * V + 3 * Fn], lines[-1]
    a, b, c = (int(t) + 1 for t in f[0])
    assert first == f"f {a}/1/{a} {b}/2/{b} {c}/3/{c}"
    a, b, c = (int(t) + 1 for t in f[-1])
    assert last == f"f {a}/{3 * Fn - 2}/{a} {b}/{3 * Fn - 1}/{b} {c}/{3 * Fn}/{c}"
    x, y, z = v.numpy()[0]
    assert lines[2] == f"v {str(x)} {str(y)} {str(z)}" == "v -0.35 -0.35 -0.35"  # the shortest text that reads back to the same float32
    back = texture.read_textured_obj(str(tmp_path))
    assert back["order"] == ["mtllib", "usemtl", "v", "vt", "vn", "f"]
    assert np.array_equal(back["vertices"], v.numpy()) and np.array_equal(back["normals"], n.numpy())
    assert np.array_equal(back["faces"], f.numpy()) and np.array_equal(back["face_vn"], f.numpy())
    assert np.array_equal(back["face_vt"], np.arange(3 * Fn).reshape(Fn, 3)) and int(back["faces"].min()) == 0
    tc = tex.texture_coordinates.numpy().reshape(-1, 2)
    assert np.array_equal(back["vt"][:, 0], tc[:, 0]) and np.array_equal(back["vt"][:, 1], np.float32(1.0) - tc[:, 1])  # v is flipped
    assert back["materials"] == {"material_0": "material_0.png", "material_thermal": "material_0_thermal.png"}
    mtl = open(paths["mtl"]).read()
    assert mtl.count("newmtl ") == 2 and "map_Kd material_0.png" in mtl and "map_Kd material_0_thermal.png" in mtl
    for key in ("rgb", "thermal"):
        want = getattr(tex, key).numpy()
        assert np.array_equal(_decode_png(paths[key]), want) and np.array_equal(back[key], want)
    with pytest.raises(ValueError, match="usemtl"):
        texture.write_textured_obj(str(tmp_path), mesh, tex, usemtl="infrared")


def test_mirroring_frame_swaps_the_texture_corners_with_the_winding(tmp_path):
    """In a dataset frame that mirrors, mesh_to_dataset_frame swaps corners 1 and 2 of every face; each corner keeps its own texture coordinate."""
    import types

    texture = _texture()
    from nerfstudio_thermal_amd.mesh import Mesh

    v, f, n = xf.cube_mesh()
    Fn, px = f.shape[0], 2
    W, H, _, _ = xf.layout(Fn, px)
    mesh = Mesh(v, f.int(), n, torch.zeros((v.shape[0], 4)))
    tex = texture.Texture(torch.zeros((H, W, 3), dtype=torch.uint8), torch.zeros((H, W), dtype=torch.uint8), xf.texture_coordinates_ref(Fn, px).float(), 0.0)
    T = torch.tensor([[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, 0.2], [0.0, 0.0, -1.0, 0.3]])
    outputs = types.SimpleNamespace(dataparser_transform=T, dataparser_scale=2.0)
    texture.write_textured_obj(str(tmp_path), mesh, tex, dataparser_outputs=outputs)
    back = texture.read_textured_obj(str(tmp_path))
    assert np.array_equal(back["faces"], f.numpy()[:, [0, 2, 1]])
    tc = tex.texture_coordinates.numpy()[:, [0, 2, 1]].reshape(-1, 2)
    assert np.array_equal(back["vt"][:, 0], tc[:, 0]) and np.array_equal(back["vt"][:, 1], np.float32(1.0) - tc[:, 1])
    fv = torch.from_numpy(back["vertices"])[torch.from_numpy(back["faces"])]
    face_normal = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=-1)
    assert bool(((face_normal * torch.from_numpy(back["normals"])[torch.from_numpy(back["faces"][:, 0])]).sum(-1) > 0).all())


# ---------------------------------------------------------------------------------------------------- 5. host-side validation
def test_entry_points_validate_on_the_host(lib):
    """Null pointers, px < 2, texel ranges that leave the image, bad strides and a short workspace are refused before any launch: no device needed; the
    pointers only have to be non-NULL."""
    fake = C.c_void_p(256 * 4096)  # aligned, never dereferenced
    V, Fn, px = 8, 7, 4
    total = 14 * 8
    err = lib.tn_last_error
    assert lib.tn_texture_rays(None, None, V, None, Fn, px, 0.0, 0, 1, None, None, None) == -22 and b"null" in err()
    assert lib.tn_texture_rays(fake, fake, V, fake, Fn, px, 0.0, 0, 1, None, fake, None) == -22 and b"null pointer" in err()
    assert lib.tn_texture_rays(fake, fake, V, fake, Fn, 1, 0.0, 0, 1, fake, fake, None) == -22 and b"texels per triangle" in err()
    assert lib.tn_texture_rays(fake, fake, V, fake, 0, px, 0.0, 0, 1, fake, fake, None) == -22
    assert lib.tn_texture_rays(fake, fake, 0, fake, Fn, px, 0.0, 0, 1, fake, fake, None) == -22 and b"vertices" in err()
    assert lib.tn_texture_rays(fake, fake, V, fake, Fn, px, 0.0, 0, total + 1, fake, fake, None) == -22 and b"outside the image of 14 x 8" in err()
    assert lib.tn_texture_rays(fake, fake, V, fake, Fn, px, 0.0, total, 1, fake, fake, None) == -22
    assert lib.tn_texture_rays(fake, fake, V, fake, Fn, px, 0.0, -1, 1, fake, fake, None) == -22
    assert lib.tn_texture_rays(fake, fake, V, fake, Fn, px, 0.0, 2, -1, fake, fake, None) == -22
    assert lib.tn_texture_rays(fake, fake, V, fake, Fn, px, -1.0, 0, 1, fake, fake, None) == -22 and b"raylen" in err()
    assert lib.tn_texture_rays(fake, fake, V, fake, Fn, px, float("nan"), 0, 1, fake, fake, None) == -22
    assert lib.tn_texture_rays(fake, fake, V, C.c_void_p(256 * 4096 + 2), Fn, px, 0.0, 0, 1, fake, fake, None) == -22 and b"misaligned" in err()
    assert lib.tn_texture_rays(fake, fake, V, fake, Fn, px, 0.5, total, 0, None, None, None) == 0  # an empty range at the end touches nothing
    assert lib.tn_texture_coords(Fn, px, None, None) == -22 and lib.tn_texture_coords(Fn, 1, fake, None) == -22
    assert lib.tn_texture_vertex(None, V, fake, Fn, px, 0, 1, fake, None) == -22 and b"null pointer" in err()
    assert lib.tn_texture_vertex(C.c_void_p(256 * 4096 + 4), V, fake, Fn, px, 0, 1, fake, None) == -22 and b"16-byte" in err()
    assert lib.tn_texture_vertex(fake, V, fake, Fn, px, total - 1, 2, fake, None) == -22 and b"outside the image" in err()
    assert lib.tn_texture_vertex(fake, V, fake, Fn, px, 0, 0, None, None) == 0
    assert lib.tn_texture_store(fake, 3, fake, 1, 4, 0, total, fake, None, None, None) == -22 and b"null pointer" in err()
    assert lib.tn_texture_store(fake, 2, fake, 1, 4, 0, total, fake, fake, None, None) == -22 and b"strides" in err()
    assert lib.tn_texture_store(fake, 3, fake, 0, 4, 0, total, fake, fake, None, None) == -22
    assert lib.tn_texture_store(fake, 3, fake, 1, 4, total - 3, total, fake, fake, None, None) == -22 and b"outside the image" in err()
    assert lib.tn_texture_store(fake, 4, fake, 4, 4, 0, total, fake, fake, C.c_void_p(256 * 4096 + 8), None) == -22 and b"16 bytes" in err()
    assert lib.tn_texture_store(None, 3, None, 1, 0, total, total, None, None, None, None) == 0
    need = lib.tn_mesh_mean_edge_workspace_bytes(Fn)
    assert need > 0 and lib.tn_mesh_mean_edge_workspace_bytes(0) == -1
    assert lib.tn_mesh_mean_edge(fake, V, fake, Fn, fake, fake, need - 1, None) == -22 and b"workspace of" in err()
    assert lib.tn_mesh_mean_edge(fake, V, fake, Fn, None, fake, need, None) == -22 and b"null pointer" in err()
    assert lib.tn_mesh_mean_edge(fake, V, fake, 0, fake, fake, need, None) == -22
