// Frames for people: the reference's colour maps (nerfstudio/utils/colormaps.py: apply_colormap, apply_float_colormap, apply_depth_colormap) and the
// side-by-side frame of ns-render (scripts/render.py _render_trajectory_video), as one launch per frame.  tests/render_functional.py restates the rule
// in torch.  Everything is fp32, every product, sum and quotient rounded on its own (the __f*_rn intrinsics: no contraction whatever the flags), in the
// order the reference's torch expressions evaluate; Python-side scalar arithmetic of the reference (far - near + 1e-10, colormap_max - colormap_min) is
// double, rounded to fp32 where torch rounds it (when the scalar meets the fp32 tensor).
//
// A panel is an [H,W,channels] fp32 image, channels 1 or 3.  Three channels pass through.  One channel, value x:
//   depth panels first:   x = clip((x - f32(near)) / f32(double(far) - double(near) + 1e-10), 0, 1), near / far = the given plane, or the frame's
//                         min / max where the record gives none (TN_FRAME_NEAR / TN_FRAME_FAR not set);
//   with TN_FRAME_NORMALIZE:  x = (x - lo) / ((hi - lo) + f32(1e-9)), lo / hi = min / max of the values at this point.  Every step before it is
//                         monotone, so lo / hi are the step's values AT the frame's min and max (the smaller / the larger of the two): the frame is read
//                         once, by tn_frame_minmax;
//   x = x * scale + offset (scale = f32(double(colormap_max) - double(colormap_min)), offset = f32(colormap_min)); x = clip(x, 0, 1);
//   with TN_FRAME_INVERT: x = 1 - x;  a NaN becomes 0;
//   colour = (x, x, x) where the record has no table, else row trunc(x * 255) of its table [256,3];
//   depth panels with an accumulation a:  colour = colour * a + (1 - a).
// clip keeps a NaN (torch.clip).  Bytes: trunc(clip(c, 0, 1) * 255 + 0.5), a NaN gives 0.
// The frame's min and max are over its FINITE values, (0, 0) where it has none: a deliberate difference from torch.min / torch.max, which one NaN turns
// into a NaN (and the frame black); frames that are all finite give the reference's numbers.
#include "tn_common.h"

#include <algorithm>

namespace {

constexpr int TB = 256;
constexpr int MINMAX_BLOCKS = TN_FRAME_MINMAX_WORKSPACE_BYTES / 8;  // a (min, max) pair per block
constexpr int MINMAX_PER_THREAD = 8;
constexpr int COMPOSE_MAX_BLOCKS = 2048;
constexpr float FLT_BIG = 3.4028234663852886e38f;

struct PanelK {
  const float* src;
  const float* acc;
  const float* minmax;
  double near_plane, far_plane;
  float scale, offset;
  int channels, flags, table;  // table: slot among the frame's distinct tables, -1 for none
};
struct FrameK {
  PanelK p[TN_FRAME_MAX_PANELS];
  const float* tables[TN_FRAME_MAX_PANELS];
  int num_panels, num_tables;
};
struct PanelConst {  // what a panel's pixels share (one thread per panel works them out)
  float near_f, den_f, lo, nden;
};

__device__ __forceinline__ float clip01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }  // keeps a NaN

__device__ __forceinline__ float depth_step(float x, float near_f, float den_f) { return clip01(__fdiv_rn(__fsub_rn(x, near_f), den_f)); }

__device__ PanelConst panel_const(const PanelK& p) {
  PanelConst c = {0.0f, 1.0f, 0.0f, 1.0f};
  float mn = 0.0f, mx = 0.0f;
  if (p.minmax != nullptr) mn = p.minmax[0], mx = p.minmax[1];
  float a = mn, b = mx;
  if (p.flags & TN_FRAME_DEPTH) {
    const double near_d = (p.flags & TN_FRAME_NEAR) ? p.near_plane : (double)mn, far_d = (p.flags & TN_FRAME_FAR) ? p.far_plane : (double)mx;
    c.near_f = (float)near_d;
    c.den_f = (float)(far_d - near_d + 1e-10);
    a = depth_step(mn, c.near_f, c.den_f), b = depth_step(mx, c.near_f, c.den_f);
  }
  if (p.flags & TN_FRAME_NORMALIZE) {
    const float lo = b < a ? b : a, hi = b < a ? a : b;
    c.lo = lo;
    c.nden = __fadd_rn(__fsub_rn(hi, lo), 1e-9f);
  }
  return c;
}

// the value in [0, 1] a one-channel pixel is coloured by
__device__ __forceinline__ float panel_value(const PanelK& p, const PanelConst& c, float x) {
  if (p.flags & TN_FRAME_DEPTH) x = depth_step(x, c.near_f, c.den_f);
  if (p.flags & TN_FRAME_NORMALIZE) x = __fdiv_rn(__fsub_rn(x, c.lo), c.nden);
  x = clip01(__fadd_rn(__fmul_rn(x, p.scale), p.offset));
  if (p.flags & TN_FRAME_INVERT) x = __fsub_rn(1.0f, x);
  return x != x ? 0.0f : x;
}

// the colour of pixel i of a panel; lut: the frame's tables in LDS
__device__ __forceinline__ void panel_colour(const PanelK& p, const PanelConst& c, const float* lut, int64_t i, float rgb[3]) {
  if (p.channels == 3) {
    rgb[0] = p.src[3 * i], rgb[1] = p.src[3 * i + 1], rgb[2] = p.src[3 * i + 2];
    return;
  }
  const float x = panel_value(p, c, p.src[i]);
  if (p.table < 0) {
    rgb[0] = rgb[1] = rgb[2] = x;
  } else {
    const float* row = lut + p.table * 768 + 3 * (int)__fmul_rn(x, 255.0f);  // x in [0, 1]: rows 0..255
    rgb[0] = row[0], rgb[1] = row[1], rgb[2] = row[2];
  }
  if ((p.flags & TN_FRAME_DEPTH) && p.acc != nullptr) {
    const float a = p.acc[i], rest = __fsub_rn(1.0f, a);
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[k] = __fadd_rn(__fmul_rn(rgb[k], a), rest);
  }
}

__device__ __forceinline__ uint32_t to_byte(float c) {
  const float v = __fadd_rn(__fmul_rn(clip01(c), 255.0f), 0.5f);
  return v != v ? 0u : (uint32_t)v;  // [0.5, 255.5]: truncation
}

// the frame's tables, its panel records and what each panel's pixels share, into LDS (the records arrive by value, as kernel arguments)
__device__ void load_frame_shared(const FrameK& f, float* lut, PanelK* panels, PanelConst* consts) {
  for (int i = threadIdx.x; i < f.num_tables * 768; i += TB) lut[i] = f.tables[i / 768][i % 768];
  if (threadIdx.x < f.num_panels) {
    panels[threadIdx.x] = f.p[threadIdx.x];
    consts[threadIdx.x] = panel_const(f.p[threadIdx.x]);
  }
  __syncthreads();
}

// Finite min and max: every block folds its threads' values in a fixed order and writes one pair; with one block the pair is the answer.
__device__ __forceinline__ void fold(float& mn, float& mx, float a, float b) { mn = fminf(mn, a), mx = fmaxf(mx, b); }

__device__ void block_minmax(float mn, float mx, float* __restrict__ out, bool final) {
  __shared__ float s_mn[TB / 64], s_mx[TB / 64];
  mn = tn_wave_min(mn), mx = tn_wave_max(mx);
  if ((threadIdx.x & 63) == 0) s_mn[threadIdx.x >> 6] = mn, s_mx[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < TB / 64; ++w) fold(mn, mx, s_mn[w], s_mx[w]);
    if (final && !(mn <= mx)) mn = mx = 0.0f;  // no finite value
    out[0] = mn, out[1] = mx;
  }
}

__global__ void __launch_bounds__(TB) k_frame_minmax_partial(const float* __restrict__ src, int64_t n, float* __restrict__ out, int final) {
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TB) {
    const float v = src[i];
    if (fabsf(v) <= FLT_BIG) fold(mn, mx, v, v);
  }
  block_minmax(mn, mx, out + 2 * blockIdx.x, final != 0);
}

__global__ void __launch_bounds__(TB) k_frame_minmax_final(const float* __restrict__ partial, int num, float* __restrict__ out) {
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < num; i += TB) fold(mn, mx, partial[2 * i], partial[2 * i + 1]);
  block_minmax(mn, mx, out, true);
}

// The frame [H, P W, 3] uint8 as one flat run of pixels q = y P W + p W + x: a thread owns pixels 4 r .. 4 r + 3 (12 bytes: three dwords where the
// frame is dword-aligned), the last run of the frame may be short.
__global__ void __launch_bounds__(TB) k_frame_compose(const FrameK f, int W, uint32_t total, uint8_t* __restrict__ out, int aligned) {
  __shared__ float lut[TN_FRAME_MAX_PANELS * 768];
  __shared__ PanelK panels[TN_FRAME_MAX_PANELS];
  __shared__ PanelConst consts[TN_FRAME_MAX_PANELS];
  load_frame_shared(f, lut, panels, consts);
  const uint32_t row = (uint32_t)f.num_panels * (uint32_t)W, runs = (total + 3u) / 4u;
  for (uint32_t r = blockIdx.x * TB + threadIdx.x; r < runs; r += gridDim.x * TB) {
    const uint32_t q0 = 4u * r, n = min(4u, total - q0);
    uint32_t y = q0 / row, col = q0 - y * row;
    uint32_t bytes[12];
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t p = col / (uint32_t)W, x = col - p * (uint32_t)W;
      float rgb[3];
      panel_colour(panels[p], consts[p], lut, (int64_t)y * W + x, rgb);
      bytes[3 * k] = to_byte(rgb[0]), bytes[3 * k + 1] = to_byte(rgb[1]), bytes[3 * k + 2] = to_byte(rgb[2]);
      if (++col == row) col = 0, ++y;
    }
    uint8_t* dst = out + 12ull * r;
    if (n == 4u && aligned) {
      uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
      for (int w = 0; w < 3; ++w) d32[w] = bytes[4 * w] | (bytes[4 * w + 1] << 8) | (bytes[4 * w + 2] << 16) | (bytes[4 * w + 3] << 24);
    } else {
      for (uint32_t b = 0; b < 3u * n; ++b) dst[b] = (uint8_t)bytes[b];
    }
  }
}

// one panel as float colours [H W, 3] (what a viewer takes)
__global__ void __launch_bounds__(TB) k_frame_colors(const FrameK f, int64_t total, float* __restrict__ out) {
  __shared__ float lut[768];
  __shared__ PanelK panels[1];
  __shared__ PanelConst consts[1];
  load_frame_shared(f, lut, panels, consts);
  for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TB) {
    float rgb[3];
    panel_colour(panels[0], consts[0], lut, i, rgb);
    out[3 * i] = rgb[0], out[3 * i + 1] = rgb[1], out[3 * i + 2] = rgb[2];
  }
}

int frame_of(const char* name, const TnFramePanel* panels, int32_t num_panels, int32_t H, int32_t W, int32_t max_panels, FrameK& f) {
  TN_REQUIRE(panels, "%s: null pointer (panels)", name);
  TN_REQUIRE(num_panels >= 1 && num_panels <= max_panels, "%s: %d panels (1..%d)", name, num_panels, max_panels);
  TN_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W * num_panels * 3 < (1ll << 31), "%s: panels of %d x %d (positive, and below 2^31 bytes a frame)", name, H, W);
  f.num_panels = num_panels, f.num_tables = 0;
  for (int i = 0; i < num_panels; ++i) {
    const TnFramePanel& s = panels[i];
    PanelK& p = f.p[i];
    TN_REQUIRE(s.channels == 1 || s.channels == 3, "%s: panel %d has %d channels (1 or 3)", name, i, s.channels);
    TN_REQUIRE(s.src, "%s: null pointer (source of panel %d)", name, i);
    TN_REQUIRE((((uintptr_t)s.src | (uintptr_t)s.accumulation | (uintptr_t)s.minmax | (uintptr_t)s.table) & 3) == 0, "%s: misaligned pointer (panel %d)", name, i);
    p.src = s.src, p.acc = s.accumulation, p.minmax = s.minmax, p.channels = s.channels, p.flags = s.flags, p.table = -1;
    p.near_plane = s.near_plane, p.far_plane = s.far_plane;
    p.scale = (float)(s.colormap_max - s.colormap_min), p.offset = (float)s.colormap_min;  // the difference in double, as Python takes it
    if (s.channels == 3) continue;
    const bool depth = (s.flags & TN_FRAME_DEPTH) != 0;
    const bool needs = (s.flags & TN_FRAME_NORMALIZE) || (depth && (s.flags & (TN_FRAME_NEAR | TN_FRAME_FAR)) != (TN_FRAME_NEAR | TN_FRAME_FAR));
    TN_REQUIRE(!needs || s.minmax, "%s: null pointer (panel %d is normalised, or a depth panel without both planes, and has no min / max)", name, i);
    if (s.table != nullptr) {
      int t = 0;
      while (t < f.num_tables && f.tables[t] != s.table) ++t;
      if (t == f.num_tables) f.tables[f.num_tables++] = s.table;
      p.table = t;
    }
  }
  return TN_OK;
}

}  // namespace

extern "C" int tn_frame_minmax(const float* src, int64_t n, float* out2, void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  TN_REQUIRE(n >= 1, "tn_frame_minmax: %lld values (at least 1)", (long long)n);
  TN_REQUIRE(src && out2 && workspace, "tn_frame_minmax: null pointer");
  TN_REQUIRE((((uintptr_t)src | (uintptr_t)out2 | (uintptr_t)workspace) & 3) == 0, "tn_frame_minmax: misaligned pointer");
  TN_REQUIRE(workspace_bytes >= TN_FRAME_MINMAX_WORKSPACE_BYTES, "tn_frame_minmax: workspace of %lld bytes, %d needed", (long long)workspace_bytes,
             TN_FRAME_MINMAX_WORKSPACE_BYTES);
  const int nb = (int)std::min<int64_t>(tn_cdiv(n, (int64_t)TB * MINMAX_PER_THREAD), MINMAX_BLOCKS);
  float* partial = static_cast<float*>(workspace);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_frame_minmax_partial, dim3(nb), dim3(TB), 0, st, src, n, nb == 1 ? out2 : partial, nb == 1 ? 1 : 0);
  TN_CHECK_LAUNCH("tn_frame_minmax(partial)");
  if (nb > 1) {
    hipLaunchKernelGGL(k_frame_minmax_final, dim3(1), dim3(TB), 0, st, (const float*)partial, nb, out2);
    TN_CHECK_LAUNCH("tn_frame_minmax(final)");
  }
  return TN_OK;
}

extern "C" int tn_frame_compose(const TnFramePanel* panels, int32_t num_panels, int32_t H, int32_t W, uint8_t* out_u8, tn_stream_t stream) {
  FrameK f;
  if (const int rc = frame_of("tn_frame_compose", panels, num_panels, H, W, TN_FRAME_MAX_PANELS, f)) return rc;
  TN_REQUIRE(out_u8, "tn_frame_compose: null pointer (out_u8)");
  const uint32_t total = (uint32_t)H * (uint32_t)W * (uint32_t)num_panels;
  const unsigned nb = (unsigned)std::min<int64_t>(tn_cdiv(tn_cdiv(total, 4), TB), COMPOSE_MAX_BLOCKS);
  hipLaunchKernelGGL(k_frame_compose, dim3(nb), dim3(TB), 0, tn_s(stream), f, W, total, out_u8, ((uintptr_t)out_u8 & 3) == 0 ? 1 : 0);
  TN_CHECK_LAUNCH("tn_frame_compose");
  return TN_OK;
}

extern "C" int tn_frame_colors(const TnFramePanel* panel, int32_t H, int32_t W, float* out_rgb, tn_stream_t stream) {
  FrameK f;
  if (const int rc = frame_of("tn_frame_colors", panel, 1, H, W, 1, f)) return rc;
  TN_REQUIRE(out_rgb && ((uintptr_t)out_rgb & 3) == 0, "tn_frame_colors: null or misaligned pointer (out_rgb)");
  const int64_t total = (int64_t)H * W;
  const unsigned nb = (unsigned)std::min<int64_t>(tn_cdiv(total, TB), COMPOSE_MAX_BLOCKS);
  hipLaunchKernelGGL(k_frame_colors, dim3(nb), dim3(TB), 0, tn_s(stream), f, total, out_rgb);
  TN_CHECK_LAUNCH("tn_frame_colors");
  return TN_OK;
}
