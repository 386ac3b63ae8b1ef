"""Times the frame path of render.py on the GPU (profiles/render.md): the compose launch alone (tn_frame_minmax for the depth panel + tn_frame_compose,
3 panels: rgb, thermal, depth) at 640 x 480 and 1920 x 1080 against the same colouring by the torch restatement (tests/render_functional.py) on the
device, and the per-frame loop of render_trajectory with one pinned buffer and with two, alternated, on a splat scene (with its parts -- the render,
the frame, the PNG encode -- timed alone) and on a fresh thermal-nerfacto model of the default size.

    python scripts/time_render_frames.py [--gaussians 100000] [--frames 24] [--nerf-frames 8] [--repeats 3] [--out FILE]

Device events around windows of many launches; every shape is warmed first; the HIP and the torch windows alternate in one process.  One JSON
document."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=100000)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--nerf-frames", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch

    import nerfstudio_thermal_amd  # noqa: F401
    import render_functional as rf
    import splat_functional as sf
    from nerfstudio_thermal_amd import render, splat
    from nerfstudio_thermal_amd.synth import look_at_camera

    if not torch.cuda.is_available():
        raise SystemExit("time_render_frames.py measures on the GPU: none found")
    dev = "cuda"
    names = ("rgb", "thermal", "depth")
    opts = render.ColormapOptions()
    lut = {k: v.to(dev) for k, v in rf.tables().items()}
    result = {"compose": [], "loop": []}

    def window(fn, launches):
        fn(); fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / launches * 1e3  # microseconds per call

    for W, H in ((640, 480), (1920, 1080)):
        g = torch.Generator().manual_seed(W)
        outputs = {"rgb": torch.rand((H, W, 3), generator=g).to(dev), "thermal": torch.rand((H, W, 1), generator=g).to(dev),
                   "depth": (0.3 + 6 * torch.rand((H, W, 1), generator=g)).to(dev), "accumulation": torch.rand((H, W, 1), generator=g).to(dev)}
        out = torch.empty((H, 3 * W, 3), dtype=torch.uint8, device=dev)

        def hip():
            render.compose_frame(outputs, names, opts, out=out)

        def torch_way():
            return rf.compose([dict(image=outputs["rgb"]), dict(image=outputs["thermal"], colormap="default"),
                               dict(image=outputs["depth"], colormap="default", depth=True, accumulation=outputs["accumulation"])], lut)

        assert torch.equal(render.compose_frame(outputs, names, opts), torch_way())  # the same bytes, at the size timed
        read = 4 * H * W * (3 + 1 + 1 + 1) + 4 * H * W  # the panels and the accumulation once, the depth panel a second time for its min / max
        row = {"width": W, "height": H, "panels": 3, "bytes_read": read, "bytes_written": 9 * H * W}
        hip_us, torch_us = [], []
        for _ in range(args.repeats):  # alternated
            hip_us.append(window(hip, args.launches))
            torch_us.append(window(torch_way, max(args.launches // 10, 5)))
        row.update(hip_us=hip_us, torch_us=torch_us, hip_gbytes_per_s=(read + 9 * H * W) / (min(hip_us) * 1e-6) / 1e9)
        result["compose"].append(row)

    # the per-frame loop: a splat scene, frames of 640 x 480
    torch.manual_seed(0)
    cfg = splat.ThermalSplatfactoModelConfig(sh_degree=1, sh_degree_interval=1, thermal_opacity_mode="shared")
    model = splat.ThermalSplatfactoModel(cfg, num_points=4, device=dev)
    model.load_gaussians(sf.scene(args.gaussians, 0, 1, scale_range=(-5.0, -4.0)))
    model.step = 10
    W, H = 640, 480
    fx = sf.fov_focal(W)
    ends = [render.PinholeCamera(look_at_camera(eye), fx, fx, W / 2, H / 2, W, H) for eye in ((2.3, 0.4, 0.6), (1.2, 1.9, 0.9))]
    cams = render.interpolated_path(ends, args.frames)
    tmp = tempfile.mkdtemp(prefix="render_frames_")
    try:
        render.render_trajectory(model, cams[:2], tmp)  # warm
        for rep in range(args.repeats):
            for buffers in (1, 2):
                torch.cuda.synchronize()
                t = time.perf_counter()
                render.render_trajectory(model, cams, tmp, pinned_buffers=buffers)
                torch.cuda.synchronize()
                result["loop"].append({"repeat": rep, "pinned_buffers": buffers, "frames": len(cams), "ms_per_frame": (time.perf_counter() - t) / len(cams) * 1e3})
        # where the loop's time goes: the render alone, the frame alone, the PNG alone
        torch.cuda.synchronize(); t = time.perf_counter()
        outs = [model.get_outputs_for_camera(c) for c in cams]
        torch.cuda.synchronize(); render_ms = (time.perf_counter() - t) / len(cams) * 1e3
        t = time.perf_counter()
        frames = [render.compose_frame(o, names) for o in outs]
        torch.cuda.synchronize(); compose_ms = (time.perf_counter() - t) / len(cams) * 1e3
        host = [f.cpu().numpy() for f in frames]
        t = time.perf_counter()
        for f in host:
            render.png_bytes(f)
        png_ms = (time.perf_counter() - t) / len(cams) * 1e3
        result["loop_parts_ms_per_frame"] = {"render": render_ms, "compose_with_host_work": compose_ms, "png_encode": png_ms}
        # the same loop on a fresh thermal-nerfacto model of the default size (untrained: the render costs what a trained one costs), fewer frames
        from nerfstudio_thermal_amd.config import ThermalNerfactoModelConfig
        from nerfstudio_thermal_amd.model import SceneBox

        nerf = ThermalNerfactoModelConfig(density_mode="shared").setup(scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1, -1], [1, 1, 1]])), num_train_data=8,
                                                                       metadata={"is_thermal": [False] * 4 + [True] * 4}, device=dev)
        nerf_cams = cams[:args.nerf_frames]
        render.render_trajectory(nerf, nerf_cams[:2], tmp)  # warm
        result["nerf_loop"] = []
        for rep in range(args.repeats):
            for buffers in (1, 2):
                torch.cuda.synchronize(); t = time.perf_counter()
                render.render_trajectory(nerf, nerf_cams, tmp, pinned_buffers=buffers)
                torch.cuda.synchronize()
                result["nerf_loop"].append({"repeat": rep, "pinned_buffers": buffers, "frames": len(nerf_cams),
                                            "ms_per_frame": (time.perf_counter() - t) / len(nerf_cams) * 1e3})
        torch.cuda.synchronize(); t = time.perf_counter()
        for c in nerf_cams:
            render.model_outputs(nerf, c)
        torch.cuda.synchronize()
        result["nerf_render_ms_per_frame"] = (time.perf_counter() - t) / len(nerf_cams) * 1e3
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    result["gaussians"] = args.gaussians
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
