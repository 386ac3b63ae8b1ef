"""Texture baking on the GPU: tn_texture_rays and tn_texture_coords against the float64 restatement of the reference's atlas unwrap
(texture_functional.py) within the project's convention (8 x what the reference's recorded float32 output misses it by), texel ranges bit for bit
against the whole image, zero normals, tn_mesh_mean_edge, the vertex bake sampled bilinearly against the barycentric blend, the NeRF bake bit for bit
against the model's own eval render of the same rays, and the written files."""
import os

import numpy as np
import pytest
import torch

import texture_functional as xf

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "texture_reference.npz")
F32, F64 = torch.float32, torch.float64
GUARD = -12345.0


def _texture():
    from nerfstudio_thermal_amd import texture

    return texture


def _mesh(vertices, faces, normals, rgbt=None):
    from nerfstudio_thermal_amd.mesh import Mesh

    rgbt = torch.zeros((vertices.shape[0], 4)) if rgbt is None else rgbt
    return Mesh(vertices.to(DEV, F32).contiguous(), faces.to(DEV, torch.int32).contiguous(), normals.to(DEV, F32).contiguous(),
                rgbt.to(DEV, F32).contiguous())


_CASES = {}


def _case(F, px):
    """The recorded inputs and reference outputs of a case, the float64 restatement and the owned mask: computed once, never modified."""
    if (F, px) not in _CASES:
        g = np.load(GOLDEN)
        c = {name: torch.from_numpy(g[f"F{F}_px{px}_{name}"]) for name in ("vertices", "faces", "normals", "texture_coordinates", "origins", "directions")}
        c["want"] = xf.unwrap_ref(c["vertices"], c["faces"], c["normals"], px, F64)
        c["owned"] = xf.owned(F, px)
        _CASES[(F, px)] = c
    return _CASES[(F, px)]


def _ulp32(x):
    """the spacing of float32 at |x| (float64 tensor -> float64 tensor)"""
    return torch.from_numpy(np.spacing(np.abs(x.numpy()).astype(np.float32)).astype(np.float64))


# ---------------------------------------------------------------------------------------------------- 1. the whole image
@pytest.mark.parametrize("F,px", xf.CASES)
def test_rays_and_coordinates_match_the_float64_restatement(F, px):
    """The convention (test_tsdf_mesh_gpu._compare): on owned texels origins and directions miss the float64 restatement by at most 8 x what the
    reference's recorded float32 output misses it by in the same case.  Measured on an MI355X (error / floor):
        (1,2)  origins 3.3e-16 / 1.19e-07, directions 2.89e-08 / 1.03e-07        (37,4)   origins 3.97e-08 / 1.43e-06, directions 2.97e-08 / 4.12e-07
        (2,2)  origins 2.2e-16 / 1.49e-08, directions 2.57e-08 / 6.03e-08        (201,3)  origins 5.96e-08 / 5.54e-06, directions 2.98e-08 / 3.87e-06
        (3,2)  origins 1.19e-07 / 3.58e-07, directions 2.74e-08 / 6.39e-08 (1000,4) origins 3.97e-08 / 7.09e-06, directions 2.98e-08 / 1.33e-05
        (7,4)  origins 3.97e-08 / 3.58e-07, directions 2.93e-08 / 1.24e-07 (5,7)    origins 5.96e-08 / 4.37e-07, directions 2.97e-08 / 9.65e-08
    Unowned texels are finite; texture coordinates are within 1 fp32 ulp of the float64 restatement; the owned share is the layout's own figure, so
    the mask hides nothing."""
    texture = _texture()
    c = _case(F, px)
    own = c["owned"]
    W, H, _, _ = xf.layout(F, px)
    assert int(own.sum()) == xf.owned_count(F, px) and own.shape == (H, W)
    tc, origins, directions = texture.unwrap_mesh(_mesh(c["vertices"], c["faces"], c["normals"]), px)
    assert tc.shape == (F, 3, 2) and origins.shape == (H, W, 3) and directions.shape == (H, W, 3)
    tc, origins, directions = tc.cpu(), origins.cpu(), directions.cpu()
    want_tc, want_o, want_d = c["want"]
    assert float(xf.normal_length(c["normals"], c["faces"], px)[own].min()) >= 0.25
    miss = lambda a, b: float((a.double() - b)[own].abs().max())  # noqa: E731
    floor_o, floor_d = miss(c["origins"], want_o), miss(c["directions"], want_d)
    err_o, err_d = miss(origins, want_o), miss(directions, want_d)
    tc_ulps = float(((tc.double() - want_tc).abs() / _ulp32(want_tc)).max())
    print(f"F={F} px={px} ({W}x{H}): origins {err_o:.3g} (floor {floor_o:.3g}), directions {err_d:.3g} (floor {floor_d:.3g}), "
          f"texture coordinates {tc_ulps:.3f} ulp, owned {int(own.sum())} of {own.numel()}")
    assert err_o <= 8 * floor_o and err_d <= 8 * floor_d
    assert bool(torch.isfinite(origins).all()) and bool(torch.isfinite(directions).all())
    assert tc_ulps <= 1.0
    assert float((directions.double().norm(dim=-1) - 1).abs().max()) <= 2e-7  # unit length everywhere, unowned texels included


# ---------------------------------------------------------------------------------------------------- 2. ranges
@pytest.mark.parametrize("F,px", [(37, 4), (201, 3)])
def test_ranges_give_the_bits_of_the_whole_image(F, px):
    """The image emitted in ranges of 1, 63, 64, 257 and W + 1 texels (they cross rows and squares) is the one-range image bit for bit, for the rays,
    the vertex colours and the store; a guard row in front of and behind the outputs stays untouched."""
    texture = _texture()
    c = _case(F, px)
    mesh = _mesh(c["vertices"], c["faces"], c["normals"], torch.rand((c["vertices"].shape[0], 4), generator=torch.Generator().manual_seed(F)))
    W, H, _, _ = xf.layout(F, px)
    total, raylen = W * H, 0.37
    whole_o, whole_d, whole_c = torch.empty((total, 3), device=DEV), torch.empty((total, 3), device=DEV), torch.empty((total, 4), device=DEV)
    texture.rays_call(mesh.vertices, mesh.normals, mesh.faces, px, raylen, 0, total, whole_o, whole_d)
    texture.vertex_call(mesh.rgbt, mesh.faces, px, 0, total, whole_c)
    for step in (1, 63, 64, 257, W + 1):
        o, d = torch.full((total + 2, 3), GUARD, device=DEV), torch.full((total + 2, 3), GUARD, device=DEV)
        col = torch.full((total + 2, 4), GUARD, device=DEV)  # (a row is 16 bytes: every row of it is aligned as tn_texture_vertex asks)
        img_rgb, img_th = torch.full((H + 2, W, 3), 77, dtype=torch.uint8, device=DEV), torch.full((H + 2, W), 77, dtype=torch.uint8, device=DEV)
        img_f = torch.full((H + 2, W, 4), GUARD, device=DEV)
        for t0 in range(0, total, step):
            n = min(step, total - t0)
            texture.rays_call(mesh.vertices, mesh.normals, mesh.faces, px, raylen, t0, n, o[1 + t0:1 + t0 + n], d[1 + t0:1 + t0 + n])
            texture.vertex_call(mesh.rgbt, mesh.faces, px, t0, n, col[1 + t0:1 + t0 + n])
            texture.store_call(whole_c[t0:t0 + n, :3], whole_c[t0:t0 + n, 3:], t0, img_rgb[1:-1], img_th[1:-1], img_f[1:-1])
        assert torch.equal(o[1:-1], whole_o) and torch.equal(d[1:-1], whole_d) and torch.equal(col[1:-1], whole_c), step
        assert torch.equal(img_f[1:-1].view(-1, 4), whole_c), step
        assert torch.equal(img_rgb[1:-1].view(-1, 3), xf.to_bytes(whole_c[:, :3])) and torch.equal(img_th[1:-1].view(-1), xf.to_bytes(whole_c[:, 3]))
        for buf in (o, d, col, img_f):
            assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all()), step
        for buf in (img_rgb, img_th):
            assert bool((buf[0] == 77).all()) and bool((buf[-1] == 77).all()), step


def test_store_writes_only_its_range_and_rounds_half_to_even():
    texture = _texture()
    H, W = 4, 7
    rgb = torch.full((H, W, 3), 77, dtype=torch.uint8, device=DEV)
    th = torch.full((H, W), 77, dtype=torch.uint8, device=DEV)
    fl = torch.full((H, W, 4), GUARD, device=DEV)
    def half(x):  # a float32 whose float32 product with 255 is exactly x
        v = np.float32(x / 255.0)
        for c in (v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(1))):
            if np.float32(c * np.float32(255.0)) == np.float32(x):
                return float(c)
        raise AssertionError(x)

    vals = torch.tensor([[-0.5, 0.0, half(0.5), 1.0], [half(1.5), half(2.5), 1.0, 7.0], [float("nan"), 0.5, 0.999, 0.25]], device=DEV)
    texture.store_call(vals[:, :3], vals[:, 3:], 9, rgb, th, fl)
    torch.cuda.synchronize()
    assert torch.equal(fl.view(-1, 4)[9:12].nan_to_num(nan=-7.0), vals.nan_to_num(nan=-7.0))
    want = xf.to_bytes(vals.nan_to_num(nan=0.0).cpu()).to(DEV)  # a NaN gives 0
    assert torch.equal(rgb.view(-1, 3)[9:12], want[:, :3]) and torch.equal(th.view(-1)[9:12], want[:, 3])
    assert want[0].tolist() == [0, 0, 0, 255] and want[1].tolist() == [2, 2, 255, 255] and want[2].tolist() == [0, 128, 255, 64]  # halves go to even
    keep = torch.ones(H * W, dtype=torch.bool, device=DEV)
    keep[9:12] = False
    assert bool((rgb.view(-1, 3)[keep] == 77).all()) and bool((th.view(-1)[keep] == 77).all()) and bool((fl.view(-1, 4)[keep] == GUARD).all())


# ---------------------------------------------------------------------------------------------------- 3. zero normals
def test_zero_normals_give_a_zero_direction_on_the_face():
    texture = _texture()
    F, px = 7, 4
    c = _case(F, px)
    normals = c["normals"].clone()
    dead = c["faces"][2].long()
    normals[dead] = 0.0
    raylen = 0.5
    mesh = _mesh(c["vertices"], c["faces"], normals)
    W, H, _, _ = xf.layout(F, px)
    o, d = torch.empty((H * W, 3), device=DEV), torch.empty((H * W, 3), device=DEV)
    texture.rays_call(mesh.vertices, mesh.normals, mesh.faces, px, raylen, 0, H * W, o, d)
    o, d = o.cpu().view(H, W, 3), d.cpu().view(H, W, 3)
    face = xf.texel_grid(F, px)[0]
    sel = face == 2
    assert int(sel.sum()) == (px + 3) * px // 2
    assert bool((d[sel] == 0).all()) and bool(torch.isfinite(o[sel]).all())
    _, want_o, _ = xf.unwrap_ref(c["vertices"], c["faces"], normals, px, F64, weights=xf.integer_weights(F, px))
    assert torch.equal(o[sel], want_o[sel].float())  # on the face, not moved: the offset is raylen / 2 times a zero direction
    other = c["owned"] & ~sel & ~torch.isin(c["faces"].long()[face.clamp(max=F - 1)], dead).any(dim=-1)
    assert bool((d[other].norm(dim=-1) > 0.99).all())


# ---------------------------------------------------------------------------------------------------- 4. the mean edge
@pytest.mark.parametrize("F", [1, 255, 256, 257, 100_003])
def test_mean_edge_matches_float64_and_repeats(F):
    texture = _texture()
    vertices, faces, normals = xf.case_mesh(F)
    mesh = _mesh(vertices, faces, normals)
    want = float(xf.raylen_ref(vertices, faces, F64))
    got = [texture.mesh_raylen(mesh, "edge") for _ in range(2)]
    ulp = float(np.spacing(np.float32(want)))
    print(f"F={F}: raylen {got[0]!r}, float64 {want!r}, {abs(got[0] - want) / ulp:.3f} ulp")
    assert got[0] == got[1] and got[0] == float(np.float32(got[0]))
    assert abs(got[0] - want) <= ulp
    assert texture.mesh_raylen(mesh, "none") == 0.0
    with pytest.raises(ValueError, match="not supported"):
        texture.mesh_raylen(mesh, "mean")


# ---------------------------------------------------------------------------------------------------- 5. the vertex bake
@pytest.mark.parametrize("F,px", [(37, 4), (201, 3)])
def test_vertex_bake_samples_back_to_the_barycentric_blend(F, px):
    """Corners lie on texel centres and the gap texels extrapolate the face's plane, so a bilinear lookup at any point of a face returns the
    barycentric blend of its vertex values: any error in winding, the v-flip, the lower-right mapping or the face -> square order breaks this.
    The bound has two terms.  A texel is the exact blend rounded once to fp32, an error of at most 2^-24 of its size, and the bilinear weights are
    convex: 2^-24 M, M the largest texel of the exact texture (the gap texels extrapolate beyond 0..1).  The texture coordinates are fp32 as well: a
    coordinate below 1 is off by at most 2^-25, which moves the lookup by at most 2^-25 W texels across and 2^-25 H down, and along either axis the
    face's plane changes by at most R / (px - 1) per texel, R the range of the vertex values: 2^-25 (W + H) R / (px - 1).  Plus 1e-12 for the float64
    arithmetic of the lookup.  Measured on an MI355X: 2.16e-07 at (37,4) (bound 5.70e-07), 7.70e-07 at (201,3) (bound 1.51e-06)."""
    texture = _texture()
    c = _case(F, px)
    g = torch.Generator().manual_seed(1000 + F)
    rgbt = torch.rand((c["vertices"].shape[0], 4), generator=g)
    tex = texture.bake_texture(_mesh(c["vertices"], c["faces"], c["normals"], rgbt), None, px, source="vertex", return_float=True)
    W, H, _, _ = xf.layout(F, px)
    assert tex.rgbt.shape == (H, W, 4) and tex.rgb.shape == (H, W, 3) and tex.thermal.shape == (H, W) and tex.raylen == 0.0
    assert tex.rgb.dtype == torch.uint8 and tex.thermal.dtype == torch.uint8
    image = tex.rgbt.cpu()
    exact = xf.vertex_texture_ref(rgbt, c["faces"], px)
    M = float(exact.abs().max())
    bary = torch.rand((F, 16, 3), generator=g, dtype=F64)
    bary = bary / bary.sum(dim=-1, keepdim=True)
    tc = tex.texture_coordinates.cpu().double()
    uv = (bary[..., None] * tc[:, None, :, :]).sum(dim=-2)  # [F,16,2]
    got = xf.bilinear(image, uv)
    want = (bary[..., None] * rgbt.double()[c["faces"].long()][:, None, :, :]).sum(dim=-2)
    R = float(rgbt.max() - rgbt.min())
    err, bound = float((got - want).abs().max()), 2.0 ** -24 * M + 2.0 ** -25 * (W + H) * R / (px - 1) + 1e-12
    print(f"F={F} px={px}: bilinear lookup misses the barycentric blend by {err:.3g} (bound {bound:.3g}, largest texel {M:.3f}, value range {R:.3f})")
    assert err <= bound
    assert float((image.double() - exact).abs().max()) <= 2.0 ** -24 * M
    # the bytes are the float image's
    assert torch.equal(tex.rgb.cpu(), xf.to_bytes(image[..., :3])) and torch.equal(tex.thermal.cpu(), xf.to_bytes(image[..., 3]))
    # in chunks: the same bytes
    again = texture.bake_texture(_mesh(c["vertices"], c["faces"], c["normals"], rgbt), None, px, source="vertex", chunk=100, return_float=True)
    assert torch.equal(again.rgbt, tex.rgbt) and torch.equal(again.rgb, tex.rgb) and torch.equal(again.thermal, tex.thermal)
    assert texture.bake_texture(_mesh(c["vertices"], c["faces"], c["normals"], rgbt), None, px, source="vertex").rgbt is None


# ---------------------------------------------------------------------------------------------------- 6. the NeRF bake, 7. the files
_BAKED = {}


def _baked():
    """The trained model of test_cloud_gpu, the cube mesh and its bake in chunks of 1000 texels (once)."""
    if not _BAKED:
        from test_cloud_gpu import _trained

        texture = _texture()
        model, _ = _trained("shared")
        v, f, n = xf.cube_mesh(0.35, 3)
        assert f.shape[0] == 108
        mesh = _mesh(v, f, n, torch.rand((v.shape[0], 4), generator=torch.Generator().manual_seed(5)))
        model.train()
        tex = texture.bake_texture(mesh, model, 4, source="nerf", chunk=1000, return_float=True)
        _BAKED.update(model=model, mesh=mesh, tex=tex, training_after=model.training)
    return _BAKED


def test_nerf_bake_is_the_models_eval_render_of_the_unwrapped_rays():
    """Trained for 300 iterations, the colours prove nothing and are not asserted: the bake is the model's own render of the rays, bit for bit."""
    from nerfstudio_thermal_amd.rays import RayBundle

    texture = _texture()
    b = _baked()
    model, mesh, tex = b["model"], b["mesh"], b["tex"]
    assert b["training_after"] is True  # the mode the model was in is restored
    W, H, _, _ = xf.layout(108, 4)
    assert (W, H) == (56, 28) and tex.rgbt.shape == (H, W, 4)
    want_raylen = float(xf.raylen_ref(mesh.vertices.cpu(), mesh.faces.cpu(), F64))
    assert abs(tex.raylen - want_raylen) <= float(np.spacing(np.float32(want_raylen))) and tex.raylen > 0
    tc, origins, directions = texture.unwrap_mesh(mesh, 4)
    assert torch.equal(tc, tex.texture_coordinates)
    o = xf.offset_origins(origins, directions, tex.raylen).reshape(-1, 3).contiguous()
    d = directions.reshape(-1, 3).contiguous()
    n = o.shape[0]
    model.eval()
    try:
        with torch.no_grad():
            out = model(RayBundle(origins=o, directions=d, pixel_area=torch.ones((n, 1), device=DEV),
                                  camera_indices=torch.zeros((n, 1), dtype=torch.int64, device=DEV)))
            rgb, thermal = out["rgb"].reshape(n, 3).clone(), out["rgb_thermal"].reshape(n, 1).clone()
    finally:
        model.train()
    assert bool(torch.isfinite(tex.rgbt).all())
    assert torch.equal(tex.rgbt.view(-1, 4)[:, :3], rgb) and torch.equal(tex.rgbt.view(-1, 4)[:, 3:], thermal)
    assert torch.equal(tex.rgb.cpu(), xf.to_bytes(tex.rgbt[..., :3].cpu())) and torch.equal(tex.thermal.cpu(), xf.to_bytes(tex.rgbt[..., 3].cpu()))
    # another chunk size: the same bytes; an eval-mode model stays in eval mode
    model.eval()
    other = texture.bake_texture(mesh, model, 4, source="nerf", chunk=4096, return_float=True)
    assert model.training is False
    model.train()
    assert torch.equal(other.rgbt, tex.rgbt) and torch.equal(other.rgb, tex.rgb) and torch.equal(other.thermal, tex.thermal)
    assert other.raylen == tex.raylen
    # the flat cube: every direction is minus its side's normal; every surface point lies in its side's plane (gap texels beyond the side's edge
    # too), and every ray starts raylen / 2 outside it
    own = xf.owned(108, 4).to(DEV)
    normal = -directions[own]
    assert bool(((normal.abs().sum(dim=-1) - 1).abs() < 1e-6).all()) and bool((normal.abs().amax(dim=-1) == 1).all())
    assert bool((((origins[own] * normal).sum(dim=-1) - 0.35).abs() < 1e-6).all())
    assert bool((((o.view(H, W, 3)[own] * normal).sum(dim=-1) - (0.35 + 0.5 * tex.raylen)).abs() < 1e-6).all())


def test_nerf_source_refuses_a_splat_model():
    from nerfstudio_thermal_amd import splat

    texture = _texture()
    g = torch.Generator().manual_seed(0)
    xyz = torch.randn((200, 3), generator=g) * 0.3
    rgb, th = (torch.rand((200, 3), generator=g) * 255).to(torch.uint8), (torch.rand((200, 1), generator=g) * 255).to(torch.uint8)
    model = splat.ThermalSplatfactoModel(splat.ThermalSplatfactoModelConfig(background_color="black"), device=DEV, seed=0, seed_points=(xyz, rgb, th))
    v, f, n = xf.cube_mesh(0.35, 1)
    mesh = _mesh(v, f, n, torch.rand((v.shape[0], 4), generator=g))
    with pytest.raises(NotImplementedError, match="vertex"):
        texture.bake_texture(mesh, model, 4, source="nerf")
    with pytest.raises(ValueError, match="needs the model"):
        texture.bake_texture(mesh, None, 4, source="nerf")
    tex = texture.bake_texture(mesh, model, 4, source="vertex")  # the model is not needed, and not touched
    assert tex.rgb.shape == (2 * 4, 3 * 7, 3)  # 12 faces: 6 squares, 3 across and 2 down


@pytest.mark.parametrize("usemtl", ["rgb", "thermal"])
def test_file_export_of_the_bake_reads_back(tmp_path, usemtl):
    texture = _texture()
    b = _baked()
    mesh, tex = b["mesh"], b["tex"]
    paths = texture.write_textured_obj(str(tmp_path), mesh, tex, usemtl=usemtl)
    back = texture.read_textured_obj(str(tmp_path))
    assert np.array_equal(back["vertices"], mesh.vertices.cpu().numpy()) and np.array_equal(back["normals"], mesh.normals.cpu().numpy())
    assert np.array_equal(back["faces"], mesh.faces.cpu().numpy()) and np.array_equal(back["face_vn"], back["faces"])
    assert np.array_equal(back["face_vt"], np.arange(3 * 108).reshape(108, 3))
    tc = tex.texture_coordinates.cpu().numpy().reshape(-1, 2)
    assert np.array_equal(back["vt"][:, 0], tc[:, 0]) and np.array_equal(back["vt"][:, 1], np.float32(1.0) - tc[:, 1])
    assert np.array_equal(back["rgb"], tex.rgb.cpu().numpy()) and np.array_equal(back["thermal"], tex.thermal.cpu().numpy())
    assert back["usemtl"] == {"rgb": "material_0", "thermal": "material_thermal"}[usemtl]
    assert back["materials"] == {"material_0": "material_0.png", "material_thermal": "material_0_thermal.png"}
    assert all(os.path.getsize(p) > 0 for p in paths.values())
