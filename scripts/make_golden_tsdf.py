"""Writes tests/golden/tsdf_reference.npz from the reference's own TSDF fusion (build container only; writes data, never source).

The scene is tests/tsdf_functional.py's: a 24 x 20 x 16 volume over (-1, -0.9, -0.8)..(1, 0.9, 0.8), four 64 x 48 look-at cameras outside the box with
their own focal lengths and a principal point half a pixel off centre, the analytic ray depth of a sphere of radius 0.6 (0 where a ray misses) and
random colours.  The reference's TSDF.from_aabb / integrate_tsdf (nerfstudio/exporter/tsdf_utils.py, imported unchanged; pymeshlab and skimage are
absent and stubbed, neither is called) fuse the four frames in float32; the file records the inputs -- with a fourth, thermal channel the reference
never sees -- and the reference's values, weights and colours.

    python scripts/make_golden_tsdf.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402
import tsdf_functional as tf  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tsdf_reference.npz")
DIMS, AABB, FRAMES, SIZE = (24, 20, 16), ((-1.0, -0.9, -0.8), (1.0, 0.9, 0.8)), 4, (48, 64)


def import_tsdf():
    if not ref_import.reference_available():
        raise SystemExit("the reference tree is not present: the golden file can only be written where it is")
    ref_import.install_extended_stubs()
    for name in ("pymeshlab", "skimage", "skimage.measure"):
        if name not in sys.modules:
            ref_import._perm_mod(name)
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    from nerfstudio.exporter.tsdf_utils import TSDF

    return TSDF


def main():
    TSDF = import_tsdf()
    H, W = SIZE
    c2w, intr = tf.scene_cameras(FRAMES, H, W, seed=0)
    c2w, intr = c2w.float(), intr.float()
    depth, rgbt, _ = tf.sphere_frames(c2w.double(), intr.double(), H, W, seed=0)
    tsdf = TSDF.from_aabb(torch.tensor(AABB), volume_dims=torch.tensor(DIMS))
    c2w4 = torch.cat([c2w, torch.tensor([[[0.0, 0.0, 0.0, 1.0]]]).expand(FRAMES, 1, 4)], dim=1)
    K = torch.zeros((FRAMES, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], 1.0
    tsdf.integrate_tsdf(c2w4, K, depth[:, None], color_images=rgbt[..., :3].permute(0, 3, 1, 2).contiguous())
    f32 = lambda t: np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))  # noqa: E731
    np.savez_compressed(OUT, dims=np.array(DIMS, dtype=np.int64), origin=f32(tsdf.origin), voxel=f32(tsdf.voxel_size),
                        truncation=np.float64(tsdf.truncation), c2w=f32(c2w), intr=f32(intr), depth=f32(depth), rgbt=f32(rgbt),
                        values=f32(tsdf.values), weights=f32(tsdf.weights), colors=f32(tsdf.colors))
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {int((tsdf.weights > 0).sum())} of {tsdf.weights.numel()} voxels observed")


if __name__ == "__main__":
    main()
