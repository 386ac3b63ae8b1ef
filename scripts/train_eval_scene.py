"""N3 end to end on an RGB+T dataset ON DISK: write the synthetic cube scene in the reference's transforms.json format (or take --data), train
thermal-nerfacto on it with the fused step, render every image of the val split in full and report PSNR / SSIM per spectrum.

    python scripts/train_eval_scene.py [--data DIR] [--steps 3000] [--frames 12]
        [--density-mode shared|separate] [--shared-camera-optimizer] [--shared-camera-optimizer-thermal] [--thermal-rig-offset tx ty tz rx ry rz]

--shared-camera-optimizer[-thermal] switch on the shared (rig) pose correction of the RGB / thermal branch (one [1,6] row per spectrum, trained
in the optimiser groups shared_camera_opt[_thermal]; the thermal one needs --density-mode separate, where the thermal branch exists).
--thermal-rig-offset displaces the POSE every thermal frame of the generated scene is written with by one rigid transform (world frame:
translation t, rotation exp(r) of the camera's axes) while its image stays the one of the true pose -- an unregistered thermal camera.  The
thermal row that undoes it is (-t, -r); the JSON line reports the rows after training.
"""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import nerfstudio_thermal_amd  # noqa: F401
from nerfstudio_thermal_amd import ops, synth
from nerfstudio_thermal_amd.config import CameraOptimizerConfig, ThermalNerfactoModelConfig
from nerfstudio_thermal_amd.dataparser import write_rgbt_dataset
from nerfstudio_thermal_amd.pipeline import ThermalPipeline


def rodrigues(r):
    th = float(np.linalg.norm(r))
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(r, dtype=np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def write_cube_scene(out_dir, frames_per_spectrum, device, thermal_rig_offset=None):
    """cameras on a ring looking at the cube; the thermal camera of a pair sits 5 cm beside its RGB camera (a rig), images rendered analytically.
    thermal_rig_offset (tx ty tz rx ry rz): the thermal frames' poses are WRITTEN displaced by it, their images are those of the true poses"""
    cams = synth.synth_cameras(frames_per_spectrum, frames_per_spectrum)
    n = frames_per_spectrum
    cams["c2w"][n:] = cams["c2w"][:n]
    cams["c2w"][n:, :, 3] += 0.05 * cams["c2w"][:n, :, 0]
    t = lambda k: torch.from_numpy(cams[k]).to(device)  # noqa: E731
    images = []
    for c in range(2 * n):
        H, W = int(cams["height"][c]), int(cams["width"][c])
        yy, xx = torch.meshgrid(torch.arange(H, device=device), torch.arange(W, device=device), indexing="ij")
        idx = torch.stack([torch.full((H * W,), c, device=device), yy.reshape(-1), xx.reshape(-1)], 1).contiguous()
        o, d, _, _ = ops.raygen(idx, t("c2w"), t("fx"), t("fy"), t("cx"), t("cy"), t("distortion"))
        images.append(synth.cube_scene_images(o.cpu().numpy(), d.cpu().numpy(), bool(cams["is_thermal"][c])).reshape(H, W, 3))
    if thermal_rig_offset is not None:
        off = np.asarray(thermal_rig_offset, dtype=np.float64)
        R = rodrigues(off[3:])
        cams["c2w"][n:, :, :3] = np.einsum("ij,njk->nik", R, cams["c2w"][n:, :, :3].astype(np.float64)).astype(np.float32)
        cams["c2w"][n:, :, 3] += off[:3].astype(np.float32)
    return write_rgbt_dataset(out_dir, cams, images)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--density-mode", choices=["shared", "separate"], default="shared")
    ap.add_argument("--shared-camera-optimizer", action="store_true")
    ap.add_argument("--shared-camera-optimizer-thermal", action="store_true")
    ap.add_argument("--thermal-rig-offset", type=float, nargs=6, default=None, metavar=("TX", "TY", "TZ", "RX", "RY", "RZ"))
    args = ap.parse_args()
    if args.shared_camera_optimizer_thermal and args.density_mode != "separate":
        ap.error("--shared-camera-optimizer-thermal corrects the thermal branch, which exists with --density-mode separate only")
    if args.thermal_rig_offset is not None and args.data is not None:
        ap.error("--thermal-rig-offset displaces the generated scene's thermal poses: it cannot be combined with --data")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    tmp = None
    data = args.data
    if data is None:
        tmp = tempfile.TemporaryDirectory()
        data = tmp.name
        write_cube_scene(data, args.frames, dev, args.thermal_rig_offset)
    cfg = ThermalNerfactoModelConfig(density_mode=args.density_mode)
    if args.shared_camera_optimizer:
        cfg.shared_camera_optimizer = CameraOptimizerConfig(mode="shared_SO3xR3", penalty_scale=1.0)
    if args.shared_camera_optimizer_thermal:
        cfg.shared_camera_optimizer_thermal = CameraOptimizerConfig(mode="shared_SO3xR3", penalty_scale=1.0)
    pipe = ThermalPipeline(data, model_config=cfg, device=dev)
    curve = []
    torch.cuda.synchronize(); t0 = time.perf_counter()
    done = 0
    while done < args.steps:
        k = min(500, args.steps - done)
        losses = pipe.train(k)
        done += k
        torch.cuda.synchronize()
        curve.append({"step": done, "seconds": time.perf_counter() - t0, **losses})
    train_s = time.perf_counter() - t0
    pipe.get_average_eval_image_metrics()  # (first pass: allocations, workspaces -- the second one is timed, as TEST_RAYS_PER_SEC is a steady-state figure)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    metrics = pipe.get_average_eval_image_metrics()
    torch.cuda.synchronize()
    eval_rays = int(sum(int(w) * int(h) for w, h in zip(pipe.eval_outputs.cameras["width"], pipe.eval_outputs.cameras["height"])))
    print(json.dumps({"dataset": "synthetic cube scene on disk (transforms.json, RGB frames first, per-frame intrinsics, is_thermal)" if tmp else data,
                      "train_images": len(pipe.train_outputs.image_filenames), "eval_images": len(pipe.eval_outputs.image_filenames), "steps": args.steps,
                      "train_seconds": train_s, "train_rays_per_s": args.steps * 4096 / train_s, "eval_seconds": time.perf_counter() - t1, "eval_rays": eval_rays,
                      "eval_rays_per_s_incl_image_loading_and_metrics": eval_rays / (time.perf_counter() - t1),
                      "eval_metrics": metrics, "density_mode": args.density_mode, "thermal_rig_offset": args.thermal_rig_offset,
                      "shared_rows": {sfx or "rgb": bn.shared.detach().cpu().reshape(-1).tolist() for sfx, bn in pipe.model.engine.nets.items()
                                      if bn.shared is not None},
                      "curve": curve}))


if __name__ == "__main__":
    main()
