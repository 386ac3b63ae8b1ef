"""Splat trainer on the synthetic RGB+T cube scene: ThermalSplatfactoModel trained on whole frames with splatfacto's objective.

The scene is train_eval_scene.py's (write_cube_scene: RGB 640x480 and thermal 160x120 frames on a ring, written to disk as a dataset) read back
through this package's dataparser by ThermalFullImageDatamanager (splat_datamanager.py): every frame is undistorted once on the device
(tn_image_undistort) into the pinhole frame the rasteriser renders, with the camera that goes with it, cached as uint8, and served as (camera, batch)
with every frame seen once per epoch: get_train_outputs -> get_loss_dict (L1 + SSIM, tn_image_loss) -> backward -> Optimizers(SPLAT_OPTIMIZERS,
HipAdam) -> the model's training callbacks (SH degree, gradient statistics, refinement).  At the end it reports PSNR / SSIM per spectrum on the
val split and the time per iteration as one JSON line.  The scene's cameras are distorted (synth.synth_cameras: RGB k1 = 0.05, thermal k1 = -0.08,
both with tangential terms: about 9 px at the corners of the RGB frames); --no-undistort trains on the raw frames with the parser's intrinsics
instead, the distortion dropped, as this script did before.  Either way the val split is scored on its undistorted frames.  With --seed-points N the
generated scene also gets a sparse point cloud -- N points on the cube's faces with their texture colours plus jitter (synth.cube_surface_points),
written as the dataset's PLY (transforms.json ply_file_path) -- and the model starts from it as splatfacto does (load_3D_points -> seed_points,
one Gaussian per point with kNN scales) instead of from --gaussians random ones.  --num-downscales N trains coarse to fine (splatfacto's resolution
schedule: 1 / 2^N of each frame's size at first, doubled every --resolution-schedule steps); the JSON line lists every stage with its factor, its
steps and its time per iteration, and the val split is scored in eval mode, at full size.  --tv-pixel-loss-mult / --cross-channel-loss-mult (default 0:
off) switch on ThermalNeRF's regularisers of the thermal render at the RGB cameras (get_loss_dict's tv_pixel_loss / cross_channel_loss: tn_thermal_reg;
the NeRF path runs both at 1e-6); the backward goes over the sum of the loss dict.  --differentiable-depth lets the training render's depth carry
gradients (classic mode), and --depth-tv-loss-mult / --depth-loss-mult (default 0: off; either switches the flag on) add get_loss_dict's depth_tv_loss
/ depth_loss over the covered pixels (tn_depth_loss); depth_loss needs a depth_image in the batch, which no dataparser here reads yet, and is 0
without one.  --crop-pos / --crop-rpy / --crop-scale (three floats each, all
three or none: centre, roll pitch yaw in radians, extents) give the eval render an oriented crop box (OrientedBox.from_params): after the val
split is scored on the whole scene, its frames are rendered again through get_outputs_for_camera(camera, box) and written as PNGs to --crop-out
(rgb_*.png, thermal_*.png; in separate mode with --removal-min-opacity-diff also removal_*.png and removal_thermal_*.png), and the line reports
the share of Gaussians the box keeps.  --strategy mcmc trains with gsplat's MCMC strategy instead of splatfacto's gradient-threshold refinement: a budget of
--max-gs-num Gaussians, relocation and growth every refine_every steps (tn_splat_mcmc_relocate), position noise of --noise-lr times the means' learning
rate after every step (tn_splat_mcmc_noise), and the two MCMC regularisers in the loss.  --use-bilateral-grid gives every training frame a bilateral
grid of affine colour transforms (current splatfacto's use_bilateral_grid: tn_bilagrid_slice on the training render, tv_loss in the loss, the groups
bilateral_grid / bilateral_grid_thermal with optim.SPLAT_BILAGRID_OPTIMIZERS); --frame-drift X simulates an automatic gain control on the generated
scene: every TRAINING frame is multiplied by a gain drawn uniformly in [1 - X, 1 + X] and shifted by an offset in [-X / 2, X / 2] (seeded by --seed,
clamped to [0, 1]); the held-out frames are left alone, so the val metrics say what the drift did to the scene itself.  Eval renders are never
corrected by a grid, so the line also reports psnr_rgb_affine_fit / psnr_thermal_affine_fit: each held-out frame's PSNR
after the least-squares affine colour map of its render onto its ground truth (a diagnostic of this script, plain torch).  --export-ply PATH writes
the trained Gaussians as a Gaussian-splat PLY (splat_io.export_gaussian_ply: spectrum "both", Gaussians below opacity 0.005 in both spectra and
those with a parameter that is not finite dropped); the line reports how many went out.  --export-world-frame writes that file in the dataset's own
frame (splat_transform.dataset_frame), where the point-cloud and mesh exports put theirs; the generated scene's dataparser transform is the identity,
so there it is the model's frame too and the line says so.  --prune-at STEP ... prunes by ray contribution at those steps (splat_prune.py: every
Gaussian scored over the training cameras of both spectra by its largest blending weight alpha T, tn_splat_raster_contrib; those below
--prune-min-contribution, RadSplat's 0.01 by default, are removed); the steps lie after --stop-split-at and are multiples of --refine-every, and the
line lists each prune's count.  --prune-observe scores the val split again after pruning the trained model at 0.01 and at keep ratios 0.5 and 0.25,
without fine-tuning, and puts the Gaussians back."""
import argparse
import functools
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import synth  # noqa: E402
from nerfstudio_thermal_amd import ThermalFullImageDatamanagerConfig  # noqa: E402
from nerfstudio_thermal_amd.dataparser import ThermalNerfDataParserConfig, load_image_float32, write_ply  # noqa: E402
from nerfstudio_thermal_amd.model import TrainingCallbackLocation  # noqa: E402
from nerfstudio_thermal_amd.config import CameraOptimizerConfig  # noqa: E402
from nerfstudio_thermal_amd.optim import SPLAT_BILAGRID_OPTIMIZERS, SPLAT_CAMERA_OPTIMIZERS, SPLAT_OPTIMIZERS, HipAdam, Optimizers  # noqa: E402
from nerfstudio_thermal_amd.splat import OrientedBox, PinholeCamera, ThermalSplatfactoModel, ThermalSplatfactoModelConfig, downscale_factor  # noqa: E402
from train_eval_scene import write_cube_scene  # noqa: E402


def frames_of(outputs, device):
    """(PinholeCamera, batch) per image of a dataparser split as it is on disk: fp32 frames resident on the device, the parser's intrinsics, the
    distortion dropped.  main() no longer trains on these (ThermalFullImageDatamanager undistorts and serves the frames); tests/test_splat_seed_gpu.py
    builds its frame list with it."""
    cams = outputs.cameras
    out = []
    for i, path in enumerate(outputs.image_filenames):
        cam = PinholeCamera(cams["c2w"][i].float(), float(cams["fx"][i]), float(cams["fy"][i]), float(cams["cx"][i]), float(cams["cy"][i]),
                            int(cams["width"][i]), int(cams["height"][i]))
        out.append((cam, {"image": load_image_float32(path).to(device), "is_thermal": bool(outputs.metadata["is_thermal"][i])}))
    return out


def add_seed_points(data: str, num: int, seed: int) -> None:
    """synth.cube_surface_points as <data>/sparse_pc.ply, named by transforms.json's ply_file_path"""
    xyz, rgb = synth.cube_surface_points(num, seed=seed)
    write_ply(os.path.join(data, "sparse_pc.ply"), xyz, rgb)
    path = os.path.join(data, "transforms.json")
    with open(path, encoding="utf-8") as f:
        meta = json.load(f)
    meta["ply_file_path"] = "sparse_pc.ply"
    with open(path, "w", encoding="utf-8") as f:
        json.dump(meta, f, indent=4)


def apply_frame_drift(cached_train, drift: float, seed: int):
    """A simulated automatic gain control: every cached training frame becomes clamp(gain * frame + offset, 0, 1), gain uniform in
    [1 - drift, 1 + drift], offset uniform in [-drift / 2, drift / 2], one pair per frame from a generator seeded by `seed`; uint8 frames stay
    uint8.  Returns the (gain, offset) pairs."""
    g = torch.Generator().manual_seed(seed + 7919)
    pairs = []
    for batch in cached_train:
        gain = 1.0 + drift * (2.0 * float(torch.rand((), generator=g)) - 1.0)
        offset = 0.5 * drift * (2.0 * float(torch.rand((), generator=g)) - 1.0)
        image = batch["image"]
        if image.dtype == torch.uint8:
            batch["image"] = ((image.float() / 255.0 * gain + offset).clamp(0.0, 1.0) * 255.0).round().to(torch.uint8)
        else:
            batch["image"] = (image * gain + offset).clamp(0.0, 1.0)
        pairs.append((gain, offset))
    return pairs


def affine_fit_psnr(pred: torch.Tensor, gt: torch.Tensor) -> float:
    """PSNR of an [H,W,C] render against its ground truth after the least-squares affine colour map pred -> gt of that frame (a C x (C + 1)
    matrix): what is left once a global gain, offset and colour mix are taken out.  A diagnostic of this script -- eval renders are never
    corrected by a bilateral grid --; plain torch."""
    C_ = pred.shape[2]
    x = torch.cat([pred.reshape(-1, C_), torch.ones((pred.shape[0] * pred.shape[1], 1), device=pred.device)], dim=1).double()
    y = gt.reshape(-1, C_).double()
    fit = x @ torch.linalg.lstsq(x, y).solution
    return float(-10.0 * torch.log10(torch.mean((fit - y) ** 2)))


def write_cropped_frames(model, val, box, out_dir: str) -> int:
    """The val frames through get_outputs_for_camera(camera, box), one PNG per image output; returns the number of frames."""
    from PIL import Image

    os.makedirs(out_dir, exist_ok=True)
    n = 0
    with torch.no_grad():
        for n, (cam, _) in enumerate(val, 1):
            out = model.get_outputs_for_camera(cam, box)
            for key in ("rgb", "thermal", "removal", "removal_thermal"):
                if key in out:
                    u8 = (out[key].clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).cpu().numpy()
                    Image.fromarray(u8[:, :, 0] if u8.shape[2] == 1 else u8).save(os.path.join(out_dir, f"{key}_{n:05d}.png"))
    model.set_crop(None)
    return n


def observe_pruning(model, train_cameras, val):
    """What pruning by ray contribution does to the trained model without fine-tuning: the Gaussians are scored once over the training cameras,
    then for RadSplat's threshold 0.01 and for keep ratios 0.5 and 0.25 the model is pruned, the val split scored (PSNR / SSIM per spectrum, means
    over its frames) and the Gaussians put back.  Returns {"before": ..., rule: ...}, each with its number of Gaussians."""
    from nerfstudio_thermal_amd import splat_prune

    def scored():
        sums = {}
        with torch.no_grad():
            for cam, batch in val:
                metrics, _ = model.get_image_metrics_and_images(model.get_outputs(cam), batch)
                for k, v in metrics.items():
                    sums.setdefault(k, []).append(v)
        return {"gaussians": model.num_points, **{k: sum(v) / len(v) for k, v in sums.items()}}

    was_training = model.training
    model.eval()
    saved = {k: model.gauss_params[k].detach().clone() for k in model.param_names}
    scores = splat_prune.score_gaussians(model, train_cameras)
    seen = scores.views_rgb + scores.views_thermal
    out = {"before": scored(), "seen_by_no_training_frame": int((seen == 0).sum()),
           "importance_quantiles_10_50_90": [float(q) for q in torch.quantile(scores.importance(), torch.tensor([0.1, 0.5, 0.9], device=seen.device))]}
    for name, rule in (("min_contribution_0.01", {"min_contribution": 0.01}), ("keep_ratio_0.5", {"keep_ratio": 0.5}), ("keep_ratio_0.25", {"keep_ratio": 0.25})):
        splat_prune.prune_gaussians(model, splat_prune.prune_mask(scores, **rule))
        out[name] = scored()
        model.load_gaussians(saved)
    model.train(was_training)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default=None)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--frames", type=int, default=12, help="frames per spectrum of the generated scene")
    ap.add_argument("--gaussians", type=int, default=20000, help="random initial Gaussians (uniform in a cube of side --init-extent)")
    ap.add_argument("--init-extent", type=float, default=1.0)
    ap.add_argument("--ssim-lambda", type=float, default=0.2)
    ap.add_argument("--background", default="random")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seed-points", type=int, default=0, help="start from N points sampled on the cube's surface (generated scene only)")
    ap.add_argument("--seed-from-dataset", action="store_true",
                    help="start from the cloud the dataset's transforms.json names as ply_file_path (--data only); a cloud with a thermal property, "
                         "as scripts/export_point_cloud.py writes it, seeds the thermal features too")
    ap.add_argument("--num-downscales", type=int, default=0, help="train at 1 / 2^N resolution at first (0: full size throughout)")
    ap.add_argument("--resolution-schedule", type=int, default=250, help="steps after which the training resolution doubles")
    ap.add_argument("--tv-pixel-loss-mult", type=float, default=0.0, help="weight of the thermal render's 2x2 total variation on RGB frames (0: off)")
    ap.add_argument("--differentiable-depth", action="store_true", help="let the training render's depth carry gradients (classic mode)")
    ap.add_argument("--depth-loss-mult", type=float, default=0.0, help="weight of the L1 distance of the depth render to the batch's depth_image (0: off)")
    ap.add_argument("--depth-tv-loss-mult", type=float, default=0.0, help="weight of the depth render's 2x2 total variation over its covered pixels (0: off)")
    ap.add_argument("--cross-channel-loss-mult", type=float, default=0.0,
                    help="weight of the thermal render's pixel differences against the RGB ground truth's on RGB frames (0: off)")
    ap.add_argument("--thermal-opacity-mode", default="shared", choices=("shared", "separate"),
                    help='"separate": the thermal channel has an opacity per Gaussian of its own (opacities_thermal)')
    ap.add_argument("--opacity-loss-mult", type=float, default=0.0, help="weight of density_loss between the two opacities (separate mode; 0: off)")
    ap.add_argument("--removal-min-opacity-diff", type=float, default=None,
                    help="separate mode: eval renders add `removal` / `removal_thermal`, composited from the Gaussians whose two opacities differ by "
                         "less than this share of the spectrum's own (ThermalNeRF's removal_min_density_diff); the line reports the shares removed")
    ap.add_argument("--crop-pos", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="centre of the eval render's crop box")
    ap.add_argument("--crop-rpy", type=float, nargs=3, default=None, metavar=("ROLL", "PITCH", "YAW"), help="its orientation, radians")
    ap.add_argument("--crop-scale", type=float, nargs=3, default=None, metavar=("SX", "SY", "SZ"), help="its extents")
    ap.add_argument("--crop-out", default="out/crop", help="where the cropped eval frames are written")
    ap.add_argument("--camera-optimizer", default="off", choices=("off", "SO3xR3", "shared_SO3xR3"),
                    help="refine the RGB frames' poses: a row per training frame, or one shared row (also applied to eval renders)")
    ap.add_argument("--camera-optimizer-thermal", default="off", choices=("off", "SO3xR3", "shared_SO3xR3"),
                    help="the same for the thermal frames (shared_SO3xR3: a mis-registered thermal rig)")
    ap.add_argument("--use-absgrad", action="store_true",
                    help="densify on the absolute 2D-mean gradients (AbsGS); raise --densify-grad-thresh with it (gsplat advises about 0.0008)")
    ap.add_argument("--densify-grad-thresh", type=float, default=0.0002)
    ap.add_argument("--strategy", default="default", choices=("default", "mcmc"),
                    help='"mcmc": a budget of --max-gs-num Gaussians, dead ones relocated onto live ones, position noise every step (gsplat\'s MCMCStrategy)')
    ap.add_argument("--max-gs-num", type=int, default=1_000_000, help="the MCMC strategy's budget of Gaussians")
    ap.add_argument("--noise-lr", type=float, default=5e5, help="the MCMC strategy's position noise, in units of the means' learning rate")
    ap.add_argument("--use-bilateral-grid", action="store_true",
                    help="a bilateral grid of affine colour transforms per training frame, applied to its training render (tv_loss regularises it)")
    ap.add_argument("--use-3d-filter", action="store_true",
                    help="Mip-Splatting's 3D smoothing filter from the full-resolution training cameras of both spectra (not with --strategy mcmc)")
    ap.add_argument("--frame-drift", type=float, default=0.0, metavar="X",
                    help="generated scene only: training frames times a per-frame gain in [1-X, 1+X] plus an offset in [-X/2, X/2]; val frames untouched")
    ap.add_argument("--no-undistort", action="store_true", help="train on the raw frames with the parser's intrinsics (the distortion dropped)")
    ap.add_argument("--export-ply", default=None, metavar="PATH",
                    help="write the trained Gaussians as a Gaussian-splat PLY (splat_io.export_gaussian_ply, spectrum both, opacity below 0.005 dropped)")
    ap.add_argument("--export-world-frame", action="store_true", help="write the --export-ply file in the dataset's frame (default: the model's)")
    ap.add_argument("--prune-at", type=int, nargs="+", default=[], metavar="STEP",
                    help="prune by ray contribution at these steps (RadSplat: 16000 24000): after --stop-split-at, multiples of --refine-every")
    ap.add_argument("--prune-min-contribution", type=float, default=0.01,
                    help="a Gaussian goes when its largest blending weight alpha T on any training ray of either spectrum is below this")
    ap.add_argument("--stop-split-at", type=int, default=15000, help="the step densification and opacity resets end at")
    ap.add_argument("--refine-every", type=int, default=100, help="steps between refinements")
    ap.add_argument("--prune-observe", action="store_true",
                    help="after training: the val metrics of the model pruned at 0.01 and at keep ratios 0.5 and 0.25, without fine-tuning "
                         "(the trained model itself is left as it is)")
    args = ap.parse_args()
    if args.export_world_frame and args.export_ply is None:
        ap.error("--export-world-frame goes with --export-ply")
    if args.seed_points and args.data is not None:
        ap.error("--seed-points samples the generated scene's cube; a dataset on disk brings its own ply_file_path")
    if args.frame_drift and args.data is not None:
        ap.error("--frame-drift drifts the generated scene's training frames; a dataset on disk is trained as it is")
    if not 0.0 <= args.frame_drift < 1.0:
        ap.error("--frame-drift takes X in [0, 1)")
    if args.seed_from_dataset and args.data is None:
        ap.error("--seed-from-dataset reads the ply_file_path of a dataset on disk: it needs --data")
    if args.use_3d_filter and args.strategy == "mcmc":
        ap.error("--use-3d-filter does not go with --strategy mcmc")
    if args.removal_min_opacity_diff is not None and args.thermal_opacity_mode != "separate":
        ap.error("--removal-min-opacity-diff compares the two opacities: it needs --thermal-opacity-mode separate")
    crop_args = (args.crop_pos, args.crop_rpy, args.crop_scale)
    if any(a is not None for a in crop_args) and not all(a is not None for a in crop_args):
        ap.error("--crop-pos, --crop-rpy and --crop-scale go together")
    crop_box = OrientedBox.from_params(*crop_args) if crop_args[0] is not None else None
    dev = torch.device("cuda", 0)
    tmp = None
    data = args.data
    if data is None:
        tmp = tempfile.TemporaryDirectory()
        data = tmp.name
        write_cube_scene(data, args.frames, dev)
        if args.seed_points:
            add_seed_points(data, args.seed_points, args.seed)
    seeded = bool(args.seed_points) or args.seed_from_dataset
    pc = ThermalNerfDataParserConfig(data=data, load_3D_points=seeded)
    dm = ThermalFullImageDatamanagerConfig(dataparser=pc, undistort=not args.no_undistort, seed=args.seed).setup(device=dev)
    # the val split is scored on its undistorted frames whatever the training frames were
    val = dm.fixed_indices_eval_dataloader if not args.no_undistort else \
        ThermalFullImageDatamanagerConfig(dataparser=pc, seed=args.seed).setup(device=dev).fixed_indices_eval_dataloader
    if args.frame_drift:
        apply_frame_drift(dm.cached_train, args.frame_drift, args.seed)
    seed_points = dm.seed_points if seeded else None
    if args.seed_from_dataset and seed_points is None:
        ap.error(f"--seed-from-dataset: {data} names no point cloud (ply_file_path)")
    cfg = ThermalSplatfactoModelConfig(num_random=args.gaussians, random_scale=args.init_extent, ssim_lambda=args.ssim_lambda,
                                       background_color=args.background, num_downscales=args.num_downscales,
                                       resolution_schedule=args.resolution_schedule, tv_pixel_loss_mult=args.tv_pixel_loss_mult,
                                       differentiable_depth=args.differentiable_depth or args.depth_loss_mult > 0 or args.depth_tv_loss_mult > 0,
                                       depth_loss_mult=args.depth_loss_mult, depth_tv_loss_mult=args.depth_tv_loss_mult,
                                       cross_channel_loss_mult=args.cross_channel_loss_mult, thermal_opacity_mode=args.thermal_opacity_mode,
                                       opacity_loss_mult=args.opacity_loss_mult, removal_min_opacity_diff=args.removal_min_opacity_diff,
                                       camera_optimizer=CameraOptimizerConfig(mode=args.camera_optimizer),
                                       camera_optimizer_thermal=CameraOptimizerConfig(mode=args.camera_optimizer_thermal), use_absgrad=args.use_absgrad,
                                       densify_grad_thresh=args.densify_grad_thresh, strategy=args.strategy, max_gs_num=args.max_gs_num,
                                       noise_lr=args.noise_lr, use_bilateral_grid=args.use_bilateral_grid, use_3d_filter=args.use_3d_filter,
                                       stop_split_at=args.stop_split_at, refine_every=args.refine_every, prune_at_steps=tuple(args.prune_at),
                                       prune_min_contribution=args.prune_min_contribution)
    model = ThermalSplatfactoModel(cfg, device=dev, seed=args.seed, num_train_data=dm.num_train_data, seed_points=seed_points,
                                   train_is_thermal=dm.train_is_thermal)
    if args.use_3d_filter:
        model.set_filter_cameras(dm.train_cameras)
    if args.prune_at:
        model.set_prune_cameras(dm.train_cameras)
    prunes = []  # (step, Gaussians before, removed) of every pruning step
    initial = model.num_points
    opts = Optimizers(model.get_param_groups(), {**SPLAT_OPTIMIZERS, **SPLAT_CAMERA_OPTIMIZERS, **SPLAT_BILAGRID_OPTIMIZERS}, optimizer_cls=HipAdam)
    cbs = model.get_training_callbacks(opts)
    curve = []
    stages = []  # one entry per run of steps at one downscale factor
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(args.steps):
        factor = downscale_factor(step, args.num_downscales, args.resolution_schedule, True)
        if not stages or stages[-1]["downscale_factor"] != factor:
            torch.cuda.synchronize()
            stages.append({"downscale_factor": factor, "first_step": step, "t0": time.perf_counter()})
        cam, batch = dm.next_train(step)
        for cb in cbs:
            cb.run_callback_at_location(step, TrainingCallbackLocation.BEFORE_TRAIN_ITERATION)
        opts.zero_grad_all()
        loss = model.get_loss_dict(model.get_train_outputs(cam), batch)
        functools.reduce(torch.add, loss.values()).backward()
        opts.optimizer_step_all()
        opts.scheduler_step_all()
        for cb in cbs:
            cb.run_callback_at_location(step, TrainingCallbackLocation.AFTER_TRAIN_ITERATION)
        if step in args.prune_at:
            prunes.append({"step": step, "gaussians": model.last_prune_counts[0], "removed": model.last_prune_counts[1]})
        if (step + 1) % 500 == 0 or step + 1 == args.steps:
            torch.cuda.synchronize()
            curve.append({"step": step + 1, "seconds": time.perf_counter() - t0, "main_loss": float(loss["main_loss"].detach()), "gaussians": model.num_points})
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    train_s = t1 - t0
    for st, end, first in zip(stages, [s["t0"] for s in stages[1:]] + [t1], [s["first_step"] for s in stages[1:]] + [args.steps]):
        st["steps"] = first - st["first_step"]
        st["ms_per_iteration"] = 1e3 * (end - st.pop("t0")) / st["steps"]
    sums = {}
    model.eval()  # the val split is scored at full size whatever the schedule's factor at the last step
    with torch.no_grad():
        for cam, batch in val:
            outputs = model.get_outputs(cam)
            metrics, _ = model.get_image_metrics_and_images(outputs, batch)
            th, pred, gt = model._frame_pred_gt(outputs, batch, resize_pred=True)  # the same frame after a per-frame affine colour fit
            metrics["psnr_thermal_affine_fit" if th else "psnr_rgb_affine_fit"] = affine_fit_psnr(pred, gt.float())
            for k, v in metrics.items():
                sums.setdefault(k, []).append(v)
    extra = {}
    if args.prune_at:
        extra["prunes"] = prunes
    if args.prune_observe:
        extra["prune_observation"] = observe_pruning(model, dm.train_cameras, val)
    if crop_box is not None:  # the same frames cropped to the box, written out; the whole-scene metrics above are untouched
        frames = write_cropped_frames(model, val, crop_box, args.crop_out)
        extra["crop"] = {"pos": args.crop_pos, "rpy": args.crop_rpy, "scale": args.crop_scale, "frames_written": frames, "out": args.crop_out,
                         "gaussians_kept_share": float(crop_box.within(model.means.detach()).float().mean()) if model.num_points else 0.0}
    if args.export_ply is not None:  # the splat file every viewer reads, with the thermal parameters under names of their own
        from nerfstudio_thermal_amd import splat_io

        os.makedirs(os.path.dirname(os.path.abspath(args.export_ply)), exist_ok=True)
        world = None
        if args.export_world_frame:
            from nerfstudio_thermal_amd.splat_transform import dataset_frame

            meta = json.load(open(os.path.join(data, "transforms.json"), encoding="utf-8"))
            world = dataset_frame(dm.train_dataparser_outputs, meta.get("applied_transform"))
        out = splat_io.export_gaussian_ply(model, args.export_ply, spectrum="both", min_opacity=0.005, transform=world)
        extra["export_ply"] = {k: out[k] for k in ("path", "exported", "dropped", "spectrum")}
        extra["export_ply"]["frame"] = "model" if world is None else \
            ("dataset (the dataparser's transform is the identity: also the model's)" if world.is_identity else "dataset")
    model.train()
    metrics = {k: sum(v) / len(v) for k, v in sums.items() if all(math.isfinite(x) for x in v)}
    pose_norms = {}
    model.camera_optimizer.get_metrics_dict(pose_norms)
    model.camera_optimizer_thermal.get_metrics_dict(pose_norms)
    extra.update({k: float(v) for k, v in pose_norms.items()})  # the refined poses' translation / rotation norms, when a mode is on
    if model.separate:  # the share of Gaussians whose two opacities ended more than 0.5 apart
        gp = model.gauss_params
        gap = (torch.sigmoid(gp["opacities"]) - torch.sigmoid(gp["opacities_thermal"])).abs()
        extra["opacity_gap_above_0.5_share"] = float((gap > 0.5).float().mean()) if gap.numel() else 0.0
        thr = args.removal_min_opacity_diff
        if thr is not None:  # the share of Gaussians the removal renders leave out of each spectrum
            o, ot = torch.sigmoid(gp["opacities"]), torch.sigmoid(gp["opacities_thermal"])
            extra["removal_min_opacity_diff"] = thr
            extra["removed_from_rgb_share"] = float((~(gap < thr * o)).float().mean()) if gap.numel() else 0.0
            extra["removed_from_thermal_share"] = float((~(gap < thr * ot)).float().mean()) if gap.numel() else 0.0
    print(json.dumps({"dataset": "synthetic cube scene (train_eval_scene.write_cube_scene)" if tmp else data, "train_images": dm.num_train_data,
                      "val_images": len(val), "steps": args.steps, "ssim_lambda": args.ssim_lambda, "background_color": args.background,
                      "initial_gaussians": initial, "seed_points": args.seed_points,
                      "seed_from_dataset": args.seed_from_dataset, "thermal_seeds": seed_points is not None and len(seed_points) == 3, "final_gaussians": model.num_points, "train_seconds": train_s,
                      "ms_per_iteration": 1e3 * train_s / max(args.steps, 1), "num_downscales": args.num_downscales,
                      "resolution_schedule": args.resolution_schedule, "tv_pixel_loss_mult": args.tv_pixel_loss_mult,
                      "differentiable_depth": cfg.differentiable_depth, "depth_loss_mult": args.depth_loss_mult, "depth_tv_loss_mult": args.depth_tv_loss_mult,
                      "cross_channel_loss_mult": args.cross_channel_loss_mult, "undistort": not args.no_undistort, "thermal_opacity_mode": args.thermal_opacity_mode,
                      "opacity_loss_mult": args.opacity_loss_mult, "camera_optimizer": args.camera_optimizer,
                      "camera_optimizer_thermal": args.camera_optimizer_thermal, "strategy": args.strategy, "max_gs_num": args.max_gs_num,
                      "noise_lr": args.noise_lr, "use_bilateral_grid": args.use_bilateral_grid, "use_3d_filter": args.use_3d_filter,
                      "filter_refreshes": model.filter_refreshes, "frame_drift": args.frame_drift, **extra, "stages": stages, "val_metrics": metrics, "curve": curve}))


if __name__ == "__main__":
    main()
