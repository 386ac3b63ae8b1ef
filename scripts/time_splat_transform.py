"""The similarity of a set of Gaussians at 1 M Gaussians (profiles/splat_transform.md): tn_transform_splat, in place and out of place, timed with
device events after a warm-up and alternated, window by window, with the same move written in torch on the device (the geometry as tensor
expressions, one einsum per SH band and spectrum, float32 -- what one would write without the kernel).

    python scripts/time_splat_transform.py [--gaussians 1000000] [--sh-degree 3] [--repeats 10] [--inner 20]

A window is --inner calls between two events; the calls alternate the move and its inverse, so the parameters stay where they are however many
windows run in place.  The algorithmic bytes of a call are every moved float read once and written once, 2 * 4 * (3 + 3 + 4 + 3 R + R) * N (560 N
at degree 3), computed here from the tensors' shapes; the line gives them over the median time and that as a share of the 6.3 TB/s a streaming
kernel reaches on the MI355X.  It also reports the largest difference between the kernel's result and the torch expression's at this size (float32
round-off of the latter: the kernel evaluates in double and rounds once).  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import nerfstudio_thermal_amd  # noqa: E402,F401
from nerfstudio_thermal_amd import splat_calls  # noqa: E402
from nerfstudio_thermal_amd.splat_transform import BANDS, MOVED, Similarity, rotation_quaternion, sh_rotation_matrices, transform_struct  # noqa: E402

STREAM_BYTES_PER_S = 6.3e12  # the achievable HBM stream rate of the MI355X


def make_params(n, R, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    return {"means": r(n, 3), "scales": r(n, 3) - 3.0, "quats": torch.nn.functional.normalize(r(n, 4), dim=-1), "features_rest": 0.1 * r(n, R, 3),
            "features_rest_thermal": 0.1 * r(n, R, 1)}


class TorchMove:
    """The move of a Similarity as float32 torch expressions on the device."""

    def __init__(self, T: Similarity, dev):
        f = lambda t: t.to(device=dev, dtype=torch.float32)  # noqa: E731
        self.A, self.t, self.log_s = f(T.scale * T.R), f(T.t), float(torch.log(torch.tensor(T.scale)))
        self.q = rotation_quaternion(T.R).tolist()
        self.mats = [f(M) for M in sh_rotation_matrices(T.R)]

    def rest(self, c):
        K = c.shape[1] + 1
        return torch.cat([torch.einsum("ij,njc->nic", M, c[:, a - 1:b - 1]) for (a, b), M in zip(BANDS, self.mats) if b <= K], 1) if K > 1 else c.clone()

    def __call__(self, p):
        w1, x1, y1, z1 = self.q
        w2, x2, y2, z2 = p["quats"].unbind(-1)
        quats = torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                             w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)
        return {"means": p["means"] @ self.A.T + self.t, "scales": p["scales"] + self.log_s, "quats": quats, "features_rest": self.rest(p["features_rest"]),
                "features_rest_thermal": self.rest(p["features_rest_thermal"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10, help="timed windows per variant")
    ap.add_argument("--inner", type=int, default=20, help="calls per window (even: a move and its inverse alternate)")
    args = ap.parse_args()
    if args.inner < 2 or args.inner % 2 or not 0 <= args.sh_degree <= 3:
        ap.error("--inner takes an even number >= 2, --sh-degree 0..3")
    if not torch.cuda.is_available():
        raise SystemExit("time_splat_transform.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda", 0)
    n, R = args.gaussians, (args.sh_degree + 1) ** 2 - 1
    g = torch.Generator().manual_seed(5)
    q = torch.randn(4, generator=g, dtype=torch.float64)
    q = q / q.norm()
    w, x, y, z = q.tolist()
    rot = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)
    T = Similarity.from_matrix(torch.cat([0.4 * rot, torch.tensor([[0.7], [-1.3], [0.4]], dtype=torch.float64)], 1))
    moves = (T, T.inverse())
    structs = [transform_struct(m) for m in moves]
    torch_moves = [TorchMove(m, dev) for m in moves]
    p = make_params(n, R, dev)
    src = [p[k] for k in MOVED]
    dst = [torch.empty_like(t) for t in src]
    bytes_per_call = 2 * sum(t.numel() * t.element_size() for t in src)

    def hip_in_place(i):
        splat_calls.transform_call(structs[i % 2], *src, *src)

    def hip_out_of_place(i):
        splat_calls.transform_call(structs[i % 2], *src, *dst)

    def torch_out_of_place(i):
        return torch_moves[i % 2](p)

    def torch_in_place(i):
        for k, v in torch_moves[i % 2](p).items():
            p[k].copy_(v)

    variants = {"hip_in_place": hip_in_place, "hip_out_of_place": hip_out_of_place, "torch_out_of_place": torch_out_of_place, "torch_in_place": torch_in_place}

    # the two agree at this size: the kernel's result against the float32 expression's
    hip_out_of_place(0)
    want = torch_moves[0](p)
    diff = {k: float((d - want[k]).abs().max()) for k, d in zip(MOVED, dst) if d.numel()}

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(args.inner):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3 / args.inner

    for fn in variants.values():  # warm-up: code objects, the allocator's blocks
        window(fn)
    runs = {k: [] for k in variants}
    for _ in range(args.repeats):  # alternated, so a busy neighbour on the machine hits every variant alike
        for k, fn in variants.items():
            runs[k].append(window(fn))
    out = {"gaussians": n, "sh_degree": args.sh_degree, "rest_coefficients": R, "repeats": args.repeats, "calls_per_window": args.inner,
           "bytes_per_call": bytes_per_call, "bytes_per_gaussian": bytes_per_call // max(n, 1), "stream_bytes_per_s": STREAM_BYTES_PER_S,
           "max_abs_difference_hip_vs_torch_float32": diff}
    for k, v in runs.items():
        med = statistics.median(v)
        out[k] = {"median_s": med, "min_s": min(v), "max_s": max(v), "bytes_per_s": bytes_per_call / med,
                  "share_of_stream_rate": bytes_per_call / med / STREAM_BYTES_PER_S}
    out["torch_over_hip_in_place"] = out["torch_in_place"]["median_s"] / out["hip_in_place"]["median_s"]
    out["torch_over_hip_out_of_place"] = out["torch_out_of_place"]["median_s"] / out["hip_out_of_place"]["median_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
