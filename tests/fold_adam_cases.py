"""The cases of tests/test_fold_adam_gpu.py, runnable in two processes: the library reads TN_FOLD_ADAM once per process, so the unfused
reference (TN_FOLD_ADAM=0) runs in tests/fold_adam_worker.py and the default path in the pytest process, both through run_case().

A case is a short sequence of RenderEngine.train_step iterations on the tiny golden model (tests/test_trainer_sequence_gpu.py::_setup's shared
model; `log2` overrides the main table's size).  The worker runs the sequence on its own and records the training state after every iteration;
the test replays it: before iteration i it copies the worker's state after iteration i-1 into its arena (two runs are compared one iteration at
a time from identical states, as the tests of test_trainer_sequence_gpu.py do), runs the iteration and compares."""
import torch

from helpers import golden_inputs, make_params, tiny_cfg
from test_hip_ops_gpu import pkg_cfg

DEV = "cuda"
NONE, FUSED, FELL_BACK = 0.0, 1.0, 2.0  # the decision word (csrc/tn_adam.h: TN_FOLD_ADAM_*), slot 13 of the step's loss vector; slot 12: max |d enc|
SLOT_ENC_MAX, SLOT_DECISION = 12, 13
SAMPLES = 48
FLT_MAX = 3.4028234663852886e38
# Guard trip (case "guard"): every pixel of the image multiplied by this.  At 32 rays x 48 samples the limit FLT_MAX / (8 P) is 2.769e34, and max
# |d enc| of the case's second iteration is linear in the image: 0.0117 with the golden image, 2.587e34 at x 1e36 (every gradient finite, no skip),
# non-finite at x 1e37 (an intermediate overflows; the step is skipped).  x 1.2e36 gives 3.10e34: above the limit, everything still finite.
GUARD_IMAGE_SCALE = 1.2e36


def guard_limit(num_rays):
    return FLT_MAX / (8.0 * num_rays * SAMPLES)


def build(golden_dir, log2, tile=1, take=None):
    """-> model, rays (origins, directions, camera indices), image, is_thermal, jitters; `tile` repeats the golden batch, `take` keeps its first
    rays (whole patches either way)"""
    from nerfstudio_thermal_amd.model import SceneBox

    gi = golden_inputs(golden_dir)
    ocfg = tiny_cfg("shared", log2_hashmap_size=log2)
    model = pkg_cfg(ocfg).setup(scene_box=SceneBox(aabb=torch.tensor([[-1.0, -1, -1], [1, 1, 1]])), num_train_data=ocfg.num_images,
                                metadata={"is_thermal": list(ocfg.is_thermal_cam)}, device=DEV)
    model.arena.load(make_params(ocfg))
    model.train()
    rep = lambda t: t[:take].to(DEV).repeat((tile,) + (1,) * (t.dim() - 1)).contiguous()  # noqa: E731
    rays = (rep(gi["origins"]), rep(gi["directions"]), rep(gi["camera_indices"].reshape(-1)))
    jit = [rep(j.reshape(-1)) for j in gi["jitters"]]
    return model, rays, rep(gi["image"]), rep(gi["is_thermal"]), jit


def _offset(arena, t):
    return (t.data_ptr() - arena.params.data_ptr()) // 4


def level_range(model, level):
    """arena range [lo, hi) of the floats of one level of the main table"""
    fld = model.engine.nets[""].field
    n = 2 << fld.log2_hashmap_size
    lo = _offset(model.arena, fld.table) + level * n
    return lo, lo + n


def seed_level0(model):
    """Non-zero moments on every second slot of level 0.  With one 2 x 2 patch of rays the batch touches a few dozen of level 0's 17^3 cells; at
    2^18 slots the level has 64 buckets, so most of them receive no record at all and hold nothing but these moments."""
    a = model.arena
    lo, hi = level_range(model, 0)
    g = torch.Generator().manual_seed(5)
    m = (torch.rand(hi - lo, generator=g) - 0.5) * 1e-3
    v = torch.rand(hi - lo, generator=g) * 1e-6 + 1e-9
    keep = seeded_mask(hi - lo)
    a.exp_avg[lo:hi] = (m * keep).to(DEV)
    a.exp_avg_sq[lo:hi] = (v * keep).to(DEV)


def seeded_mask(n):
    return (torch.arange(n) // 2) % 2 == 0  # (slot = two consecutive floats)


# Case "small_inf": iteration -> (tensor of the field, element).  The launch that checks the small ranges has 1024 threads and reads eight
# elements per thread at a time; every tensor starts at a multiple of 64 floats of its range, so an odd element is never lane 0's: wave 0,
# wave 15, an element in a later batch of loads, the middle of the embedding.  Iterations below 10 update the proposal networks; of 10..12 at
# least one does not.
POISON = {1: ("w0", 37), 10: ("w0", 1000), 11: ("hw1", 3333), 12: ("emb", 133)}


def poison_small_range(tensor, element):
    """inf in the gradient arena at one element of one of the field's small tensors before the backward starts: the weight gradients are
    accumulated into the arena, so this range of the group -- and nothing else, d enc included -- ends the backward non-finite."""
    def hook(model):
        a = model.arena
        a.grads[_offset(a, getattr(model.engine.nets[""].field, tensor)) + element] = float("inf")
    return hook


# name -> log2 of the main table, iterations, {iteration: image kind}, {iteration: hook run before it}, batch repeat / first rays of the batch
CASES = {
    "seq12": dict(log2=12, iters=13, images={6: "inf"}),
    "seq13": dict(log2=13, iters=13, images={6: "inf"}),
    "empty18": dict(log2=18, iters=1, take=4, hooks={0: seed_level0}, keep_level=0),  # (records hold level 0 only: the table is 33 MB)
    "small_inf": dict(log2=12, iters=13, hooks={i: poison_small_range(*at) for i, at in POISON.items()}),
    "guard": dict(log2=12, iters=2, images={1: "huge"}),
    "chunks": dict(log2=12, iters=2, tile=342),  # 10944 rays x 48 = 525312 samples > 1024 bin blocks x 512: two fold blocks per bucket
}


def run_case(name, golden_dir, ref=None):
    """-> one record per iteration.  ref: the records of another run of the case; iteration i > 0 then starts from ref[i - 1]'s state."""
    from nerfstudio_thermal_amd.optim import DeviceGradScaler

    spec = CASES[name]
    model, rays, image, is_thermal, jit = build(golden_dir, spec["log2"], spec.get("tile", 1), spec.get("take"))
    lo, hi = level_range(model, spec["keep_level"]) if "keep_level" in spec else (0, model.arena.params.numel())
    snap = lambda: [t[lo:hi].detach().cpu().clone() for t in (model.arena.params, model.arena.exp_avg, model.arena.exp_avg_sq)]  # noqa: E731
    eng, a = model.engine, model.arena
    fld = eng.nets[""].field
    table = (level_range(model, 0)[0] - lo, level_range(model, fld.num_levels - 1)[1] - lo)  # the main table inside the recorded tensors
    scaler = DeviceGradScaler(DEV)
    images = {"inf": torch.full_like(image, float("inf")), "huge": image * GUARD_IMAGE_SCALE}
    out = []
    for it in range(spec["iters"]):
        if ref is not None and it > 0:
            for dst, src in zip((a.params, a.exp_avg, a.exp_avg_sq), ref[it - 1]["state"]):
                dst.copy_(src.to(DEV))
        hook = spec.get("hooks", {}).get(it)
        if hook is not None:
            hook(model)
        pre = snap()
        kind = spec.get("images", {}).get(it)
        eng.train_step(*rays, images[kind] if kind else image, is_thermal, it, jit, None, grad_scaler=scaler)
        torch.cuda.synchronize()
        L = eng._last_losses16
        out.append({
            "pre": pre, "state": snap(), "table": table,
            "scale": scaler.get_scale(), "lag": scaler.schedule_lag(), "skipped": [scaler.num_skipped(i) for i in range(3)],
            "grads_max": float(a.grads.abs().max()), "decision": float(L[SLOT_DECISION]), "enc_max": float(L[SLOT_ENC_MAX]),
            "updated": bool(eng.last_updated), "counters": (eng.steps_since_update, eng.adam_step_count, dict(eng.group_steps)),
        })
    return out
