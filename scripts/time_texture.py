"""Texture baking at export sizes (profiles/mesh_texture.md): a 50 000-face and a 1 000 000-face mesh at px_per_uv_triangle = 4 -- a triangulated
height field, so that neighbouring faces share vertices as an extracted mesh's do -- through `tn_texture_rays` over the whole image against the
float32 restatement of the reference's unwrap in plain torch on the same device (tests/texture_functional.unwrap_ref: the reference's way, whole-image
temporaries; not the code under test), through `bake_texture` by source (for "nerf" an untrained thermal-nerfacto of the default size: the render's
cost does not depend on what the field holds; the share of the render is measured with events around it, chunk by chunk), and through
`write_textured_obj` (host clock).

    python scripts/time_texture.py [--faces 50000 1000000] [--px 4] [--repeats 20] [--warmup 3] [--torch-repeats 5] [--no-torch] [--no-nerf] [--no-write]

Times are HIP events around one call after warm-up, the median of --repeats (the spread is reported too).  Peak temporary memory is torch's allocator
high-water mark above the inputs.  One JSON line.
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
import texture_functional as xf  # noqa: E402
from nerfstudio_thermal_amd import mesh, texture  # noqa: E402
from nerfstudio_thermal_amd.rays import RayBundle  # noqa: E402
from time_tsdf_mesh import timed  # noqa: E402


def height_field(num_faces: int, dev) -> mesh.Mesh:
    """The first num_faces triangles of an n x n grid over [-0.8, 0.8]^2 lifted to z = 0.2 sin(3 x) cos(2 y), with its analytic normals."""
    n = math.ceil(math.sqrt(num_faces / 2))
    lin = torch.linspace(-0.8, 0.8, n + 1, dtype=torch.float64)
    x, y = torch.meshgrid(lin, lin, indexing="ij")
    z = 0.2 * torch.sin(3 * x) * torch.cos(2 * y)
    normal = torch.nn.functional.normalize(torch.stack([-0.6 * torch.cos(3 * x) * torch.cos(2 * y), 0.4 * torch.sin(3 * x) * torch.sin(2 * y),
                                                        torch.ones_like(x)], dim=-1), dim=-1)
    at = (torch.arange(n)[:, None] * (n + 1) + torch.arange(n)[None, :]).reshape(-1)
    quads = torch.stack([at, at + n + 1, at + n + 2, at + 1], dim=-1)
    faces = torch.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], dim=1).reshape(-1, 3)[:num_faces]
    V = (n + 1) ** 2
    return mesh.Mesh(torch.stack([x, y, z], dim=-1).reshape(V, 3).float().to(dev), faces.int().contiguous().to(dev), normal.reshape(V, 3).float().to(dev),
                     torch.rand((V, 4), generator=torch.Generator().manual_seed(0)).to(dev))


def bake_parts(m, model, px, chunk):
    """bake_texture's "nerf" loop with events around the render of every chunk -> (total ms, render ms)"""
    dev = m.vertices.device
    Fn = int(m.faces.shape[0])
    W, H, _, _ = texture.atlas_layout(Fn, px)
    total = W * H
    rgb, th = torch.empty((H, W, 3), dtype=torch.uint8, device=dev), torch.empty((H, W), dtype=torch.uint8, device=dev)
    pairs = []
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    raylen = texture.mesh_raylen(m, "edge")
    with torch.no_grad():
        for t0 in range(0, total, chunk):
            n = min(chunk, total - t0)
            o, d = torch.empty((n, 3), device=dev), torch.empty((n, 3), device=dev)
            texture.rays_call(m.vertices, m.normals, m.faces, px, raylen, t0, n, o, d)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = model(RayBundle(origins=o, directions=d, pixel_area=torch.ones((n, 1), device=dev),
                                  camera_indices=torch.zeros((n, 1), dtype=torch.int64, device=dev)))
            b.record()
            pairs.append((a, b))
            texture.store_call(out["rgb"].reshape(n, 3), out["rgb_thermal"].reshape(n, 1), t0, rgb, th, None)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end), sum(a.elapsed_time(b) for a, b in pairs)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--faces", type=int, nargs="+", default=[50_000, 1_000_000])
    ap.add_argument("--px", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=1 << 15, help="texels per rendered chunk (the method's eval_num_rays_per_chunk)")
    ap.add_argument("--no-torch", action="store_true", help="skip the plain-torch restatement")
    ap.add_argument("--no-nerf", action="store_true", help="skip the NeRF bake")
    ap.add_argument("--no-write", action="store_true", help="skip the OBJ write")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "time_texture.py needs a GPU"
    dev = torch.device("cuda", 0)
    px = args.px
    model = None
    if not args.no_nerf:
        from nerfstudio_thermal_amd.config import ThermalNerfactoModelConfig
        from nerfstudio_thermal_amd.model import SceneBox

        model = ThermalNerfactoModelConfig(density_mode="shared", eval_num_rays_per_chunk=args.chunk).setup(
            scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1, -1], [1, 1, 1]])), num_train_data=8, metadata={"is_thermal": [False, True] * 4}, device=dev)
        model.eval()
    results = []
    for Fn in args.faces:
        m = height_field(Fn, dev)
        W, H, sw, sh = texture.atlas_layout(Fn, px)
        total = W * H
        r = {"faces": Fn, "vertices": int(m.vertices.shape[0]), "px": px, "atlas": [W, H], "squares": [sw, sh], "texels": total,
             "owned_share": xf.owned_count(Fn, px) / total}
        o, d = torch.empty((total, 3), device=dev), torch.empty((total, 3), device=dev)
        hip = timed(lambda: texture.rays_call(m.vertices, m.normals, m.faces, px, 0.0, 0, total, o, d), args.repeats, args.warmup)
        moved = total * 24 + Fn * 12 + int(m.vertices.shape[0]) * 24  # the rays written, the mesh read once
        r.update({"rays_hip_ms": hip[0], "rays_hip_ms_min_max": [hip[1], hip[2]], "rays_bytes": moved, "rays_hip_GBps": moved / hip[0] / 1e6,
                  "rays_output_bytes": total * 24})
        if not args.no_torch:
            try:
                fl = m.faces.long()
                tor = timed(lambda: xf.unwrap_ref(m.vertices, fl, m.normals, px, torch.float32), args.torch_repeats, 1)
                _, wo, wd = xf.unwrap_ref(m.vertices, fl, m.normals, px, torch.float32)
                own = (xf.texel_grid(Fn, px, dev)[0] < Fn).view(-1)  # texels without a face of their own differ by design
                _, eo, ed = xf.unwrap_ref(m.vertices, fl, m.normals, px, torch.float64)  # the formula in float64, on the device
                miss = lambda got, want: float((got.reshape(-1, 3).double() - want.reshape(-1, 3))[own].abs().max())  # noqa: E731
                r.update({"rays_torch_ms": tor[0], "rays_torch_ms_min_max": [tor[1], tor[2]], "rays_torch_peak_temporary_bytes": tor[3],
                          "rays_speedup": tor[0] / hip[0], "owned_texels": int(own.sum()),
                          "rays_hip_error_vs_float64": [miss(o, eo), miss(d, ed)], "rays_torch_error_vs_float64": [miss(wo, eo), miss(wd, ed)]})
                del eo, ed
                del wo, wd, own
            except torch.cuda.OutOfMemoryError:
                r["rays_torch_ms"] = "out of memory"
            torch.cuda.empty_cache()
        del o, d
        ed = timed(lambda: texture.mesh_raylen(m, "edge"), args.repeats, args.warmup)
        r.update({"raylen": texture.mesh_raylen(m, "edge"), "raylen_ms": ed[0]})
        vb = timed(lambda: texture.bake_texture(m, None, px, source="vertex"), args.repeats, args.warmup)
        r.update({"bake_vertex_ms": vb[0], "bake_vertex_ms_min_max": [vb[1], vb[2]], "bake_vertex_peak_temporary_bytes": vb[3]})
        if model is not None:
            bake_parts(m, model, px, args.chunk)  # warm-up
            parts = [bake_parts(m, model, px, args.chunk) for _ in range(3)]
            tot, ren = sorted(p[0] for p in parts)[1], sorted(p[1] for p in parts)[1]
            nb = timed(lambda: texture.bake_texture(m, model, px, source="nerf"), 3, 0)
            r.update({"bake_nerf_ms": nb[0], "bake_nerf_ms_min_max": [nb[1], nb[2]], "bake_nerf_peak_temporary_bytes": nb[3], "bake_nerf_chunk": args.chunk,
                      "bake_nerf_parts_total_ms": tot, "bake_nerf_parts_render_ms": ren, "bake_nerf_render_share": ren / tot})
        if not args.no_write:
            tex = texture.bake_texture(m, None, px, source="vertex")
            with tempfile.TemporaryDirectory() as tmp:
                t0 = time.perf_counter()
                paths = texture.write_textured_obj(tmp, m, tex)
                r.update({"write_seconds": time.perf_counter() - t0, "file_bytes": {k: os.path.getsize(p) for k, p in paths.items()}})
        results.append(r)
        del m
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
