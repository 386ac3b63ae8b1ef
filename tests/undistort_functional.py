"""Float64 restatement of the splat path's undistortion (splat.undistorted_camera / tn_image_undistort), in numpy.  Not a test.

Distortion model: tn_raygen's and oracle/thermal_nerfacto_oracle.py::undistort_opencv's, coefficients k = (k1, k2, k3, k4, p1, p2); with r = x^2 + y^2
  d = 1 + r (k1 + r (k2 + r (k3 + r k4))),  x_d = d x + 2 p1 x y + p2 (r + 2 x^2),  y_d = d y + 2 p2 x y + p1 (r + 2 y^2).
Pixel convention: the centre of pixel (u, v) is (u + 0.5, v + 0.5), so x = (u + 0.5 - cx) / fx.

Camera rule (`new_intrinsics`): the centres of all 2W + 2H - 4 border pixels are undistorted by Newton iteration; x0 = the largest x over the left
column, x1 = the smallest over the right column, y0 / y1 likewise over the top / bottom row; fx' = (W - 1) / (x1 - x0), cx' = 0.5 - fx' x0 (and
fy', cy'): output pixel 0 looks along x0, output pixel W - 1 along x1.  The rows and columns of that frame are not the undistorted positions of
the source's border pixels, so its own border can still read up to ~1e-3 px outside the source (or inside it).  The rectangle is therefore settled:
with the source positions of the new frame's border pixels (closed form), each side moves by its miss -- the left side by min sx over column 0, the
right by max sx - (W - 1) over column W - 1, top and bottom likewise -- divided by the focal length, until every miss is below 1e-9 px.  Then every
output pixel reads inside the source frame and on each side one border pixel reads its very edge.

Image rule (`source_positions`, `gather`, `undistort`): output pixel (u, v) -> x = (u + 0.5 - cx') / fx', y likewise -> (x_d, y_d) ->
s = (fx x_d + cx - 0.5, fy y_d + cy - 0.5), clamped to [-1, W] x [-1, H]; taps floor(s) and floor(s) + 1 with their indices clamped to the frame,
weight of the second s - floor(s); along x, then along y.  A uint8 input value v enters as float32(v) / float32(255); a uint8 output is
rint(255 clamp(value, 0, 1)).  With dtype = numpy.float32 the same formulas run in single precision, operation by operation: the floor the GPU
tolerance is measured from."""
from typing import Optional, Sequence, Tuple

import numpy as np

SYNTH_RGB = (0.05, -0.01, 0.0, 0.0, 1e-3, -5e-4)  # synth.synth_cameras' RGB cameras
SYNTH_THERMAL = (-0.08, 0.02, 0.0, 0.0, 1e-3, -5e-4)  # ... and its thermal cameras
STRONG = (-0.25, 0.09, -0.02, 0.004, 4e-3, -3e-3)  # a small uncooled thermal core's order of magnitude, every term live (invertibility: the CPU tests)
SETS = {"synth_rgb": SYNTH_RGB, "synth_thermal": SYNTH_THERMAL, "strong": STRONG}
NEWTON_ITERS = 50
NEWTON_TOL = 1e-9
SETTLE_ITERS = 100
SETTLE_TOL = 1e-9  # pixels

Intrinsics = Tuple[float, float, float, float]  # fx, fy, cx, cy


def distort(x, y, k: Sequence[float], dtype=np.float64):
    t = dtype
    k1, k2, k3, k4, p1, p2 = (t(v) for v in k)
    r = x * x + y * y
    d = t(1) + r * (k1 + r * (k2 + r * (k3 + r * k4)))
    xd = d * x + t(2) * p1 * x * y + p2 * (r + t(2) * x * x)
    yd = d * y + t(2) * p2 * x * y + p1 * (r + t(2) * y * y)
    return xd, yd


def undistort_points(xd: np.ndarray, yd: np.ndarray, k: Sequence[float]):
    """Newton on (x, y) -> distort(x, y) - (xd, yd) from (xd, yd), NEWTON_ITERS steps, float64 -> (x, y, the largest residual)."""
    k1, k2, k3, k4, p1, p2 = (float(v) for v in k)
    xd, yd = np.asarray(xd, dtype=np.float64), np.asarray(yd, dtype=np.float64)
    x, y = xd.copy(), yd.copy()
    with np.errstate(all="ignore"):
        for _ in range(NEWTON_ITERS):
            r = x * x + y * y
            d = 1 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
            d_r = k1 + r * (2 * k2 + r * (3 * k3 + r * 4 * k4))
            fx_ = d * x + 2 * p1 * x * y + p2 * (r + 2 * x * x) - xd
            fy_ = d * y + 2 * p2 * x * y + p1 * (r + 2 * y * y) - yd
            fx_x = d + 2 * x * x * d_r + 2 * p1 * y + 6 * p2 * x
            fx_y = 2 * x * y * d_r + 2 * p1 * x + 2 * p2 * y
            fy_x = 2 * x * y * d_r + 2 * p2 * y + 2 * p1 * x
            fy_y = d + 2 * y * y * d_r + 2 * p2 * x + 6 * p1 * y
            det = fx_x * fy_y - fx_y * fy_x
            x = x - (fx_ * fy_y - fy_ * fx_y) / det
            y = y - (fy_ * fx_x - fx_ * fy_x) / det
        ex, ey = distort(x, y, k)
        res = np.maximum(np.abs(ex - xd), np.abs(ey - yd))
    return x, y, (float(np.max(res)) if np.all(np.isfinite(res)) else float("inf"))


def new_intrinsics(intr: Intrinsics, W: int, H: int, k: Sequence[float]) -> Intrinsics:
    """The camera rule; ValueError as splat.undistorted_camera raises it."""
    fx, fy, cx, cy = (float(v) for v in intr)
    if not np.all(np.isfinite(np.asarray(k, dtype=np.float64))):
        raise ValueError("non-finite distortion coefficients")
    us, vs = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    col = lambda u: undistort_points(np.full(H, (u + 0.5 - cx) / fx), (vs + 0.5 - cy) / fy, k)  # noqa: E731
    row = lambda v: undistort_points((us + 0.5 - cx) / fx, np.full(W, (v + 0.5 - cy) / fy), k)  # noqa: E731
    left, right, top, bottom = col(0), col(W - 1), row(0), row(H - 1)
    if not max(s[2] for s in (left, right, top, bottom)) <= NEWTON_TOL:
        raise ValueError("the distortion cannot be inverted on the frame's border")
    rect = np.array([left[0].max(), right[0].min(), top[1].max(), bottom[1].min()])
    for _ in range(SETTLE_ITERS):
        x0, x1, y0, y1 = rect
        if not (x1 > x0 and y1 > y0):
            raise ValueError("the undistorted frame's inner rectangle is empty")
        new = ((W - 1) / (x1 - x0), (H - 1) / (y1 - y0), 0.5 - (W - 1) / (x1 - x0) * x0, 0.5 - (H - 1) / (y1 - y0) * y0)
        sx, sy = source_positions(intr, new, W, H, k, clamp=False)
        miss = np.array([sx[:, 0].min(), sx[:, -1].max() - (W - 1), sy[0].min(), sy[-1].max() - (H - 1)])
        if np.abs(miss).max() <= SETTLE_TOL:
            return new
        rect = rect - miss / np.array([fx, fx, fy, fy])
    raise ValueError("the undistorted frame's inner rectangle does not settle")


def source_positions(intr: Intrinsics, new: Intrinsics, W: int, H: int, k: Sequence[float], dtype=np.float64, clamp: bool = True):
    """(sx, sy) [H,W]: where output pixel (u, v) of the `new` camera reads the source frame, in pixel-index units."""
    t = dtype
    fx, fy, cx, cy = (t(v) for v in intr)
    nfx, nfy, ncx, ncy = (t(v) for v in new)
    u, v = np.meshgrid(np.arange(W).astype(t), np.arange(H).astype(t))
    x, y = (u + t(0.5) - ncx) / nfx, (v + t(0.5) - ncy) / nfy
    xd, yd = distort(x, y, k, t)
    sx, sy = fx * xd + cx - t(0.5), fy * yd + cy - t(0.5)
    if clamp:
        sx, sy = np.minimum(np.maximum(sx, t(-1)), t(W)), np.minimum(np.maximum(sy, t(-1)), t(H))
    assert sx.dtype == t and sy.dtype == t
    return sx, sy


def as_input(image: np.ndarray) -> np.ndarray:
    """What the kernel reads: float32 as it is, uint8 as float32(v) / float32(255)."""
    if image.dtype == np.uint8:
        return image.astype(np.float32) / np.float32(255)
    assert image.dtype == np.float32
    return image


def gather(image: np.ndarray, sx: np.ndarray, sy: np.ndarray, dtype=np.float64) -> np.ndarray:
    """Clamped bilinear gather of an [H,W,C] image at (sx, sy): along x, then along y, in `dtype`."""
    t = dtype
    img = image.astype(t)
    H, W = img.shape[:2]
    fx0, fy0 = np.floor(sx), np.floor(sy)
    wx, wy = (sx - fx0).astype(t)[..., None], (sy - fy0).astype(t)[..., None]
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    xa, xb, ya, yb = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1), np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    ux, uy = t(1) - wx, t(1) - wy
    top = ux * img[ya, xa] + wx * img[ya, xb]
    bot = ux * img[yb, xa] + wx * img[yb, xb]
    out = uy * top + wy * bot
    assert out.dtype == t
    return out


def to_u8(value: np.ndarray) -> np.ndarray:
    """rint(255 clamp(value, 0, 1)) in the value's own precision (round half to even, as rintf)."""
    t = value.dtype.type
    return np.rint(t(255) * np.clip(value, t(0), t(1))).astype(np.uint8)


def undistort(image: np.ndarray, intr: Intrinsics, k: Sequence[float], new: Optional[Intrinsics] = None, dtype=np.float64) -> np.ndarray:
    """[H,W,C] uint8 or float32 -> the undistorted frame [H,W,C] in `dtype` (not yet converted to uint8: `to_u8`)."""
    H, W = image.shape[:2]
    new = new_intrinsics(intr, W, H, k) if new is None else new
    sx, sy = source_positions(intr, new, W, H, k, dtype)
    return gather(as_input(image), sx, sy, dtype)


def random_image(h: int, w: int, c: int, seed: int, u8: bool = False) -> np.ndarray:
    """Independent uniform values per pixel and channel: neighbouring taps differ by up to the whole range."""
    rng = np.random.default_rng(seed)
    if u8:
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    return rng.random((h, w, c), dtype=np.float32)


def centred(W: int, H: int, f: float) -> Intrinsics:
    return (f, f, W / 2, H / 2)
