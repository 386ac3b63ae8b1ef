"""Writes tests/golden/texture_reference.npz from the reference's own atlas unwrap (build container only; writes data, never source).

For every case of tests/texture_functional.py (CASES: faces and px_per_uv_triangle; case_mesh: vertices uniform in [-1, 1]^3, faces as random vertex
triples, normals normalize(randn + (0, 0, 3)), seeded by the face count) the reference's unwrap_mesh_per_uv_triangle
(nerfstudio/exporter/texture_utils.py, imported unchanged; mediapy and xatlas are absent and stubbed, neither is called) runs in float32; the file
records the inputs and its texture_coordinates, origins and directions.

    python scripts/make_golden_texture.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402
import texture_functional as xf  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "texture_reference.npz")


def import_unwrap():
    if not ref_import.reference_available():
        raise SystemExit("the reference tree is not present: the golden file can only be written where it is")
    ref_import.install_extended_stubs()
    for name in ("mediapy", "xatlas", "pymeshlab"):
        if name not in sys.modules:
            ref_import._perm_mod(name)
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    from nerfstudio.exporter.texture_utils import unwrap_mesh_per_uv_triangle

    return unwrap_mesh_per_uv_triangle


def main():
    unwrap = import_unwrap()
    f32 = lambda t: np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))  # noqa: E731
    arrays = {"cases": np.array(xf.CASES, dtype=np.int64)}
    for F, px in xf.CASES:
        vertices, faces, normals = xf.case_mesh(F)
        tc, origins, directions = unwrap(vertices, faces, normals, px)
        key = f"F{F}_px{px}"
        arrays.update({f"{key}_vertices": f32(vertices), f"{key}_faces": faces.numpy().astype(np.int32), f"{key}_normals": f32(normals),
                       f"{key}_texture_coordinates": f32(tc), f"{key}_origins": f32(origins), f"{key}_directions": f32(directions)})
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(xf.CASES)} cases")


if __name__ == "__main__":
    main()
