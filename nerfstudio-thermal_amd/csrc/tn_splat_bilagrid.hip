// N4 per-frame colour correction: bilateral grids ("Bilateral Guided Radiance Field Processing"; gsplat's bil_grids, splatfacto's
// use_bilateral_grid).  A frame's grid G [K][L][GH][GW], K = C (C + 1), holds an affine colour transform [A | b] (row-major C x (C + 1)) per
// vertex; pixel (i, j) of an [H,W,C] image reads it at (x, y, g) = ((j + 0.5) / W, (i + 0.5) / H, guidance) -- guidance = 0.299 r + 0.587 g + 0.114 b
// for C = 3, the value itself for C = 1 -- by trilinear interpolation (coordinates u (size - 1) clamped to [0, size - 1], cell = floor, upper
// neighbour clamped: grid_sample's bilinear / border / align_corners=True) and leaves out = A pixel + b.  The interpolation is nested lerps
// a + t (b - a), x then y then z, and the build has -ffp-contract=off: a grid that is constant over a cell is reproduced exactly, the identity grid
// returns the input's bits.
//
// No float atomics anywhere, no host synchronisation, every launch bit-reproducible:
//   k_bila_slice          one thread per pixel, 64 x 4 pixels per block; the grid is read through the caches (a frame's grid is at most a few
//                         hundred KiB and every block touches a handful of its cells).
//   k_bila_slice_bwd_img  the same walk: d out / d pixel = A^T v plus the path through the guidance coordinate (the coefficients' slope along z,
//                         times L - 1 inside (0, L - 1) and 0 on the clamp, times the luma weights).
//   k_bila_grid_partial   the grid's gradient as a GATHER: one block per (x, y) vertex, slice of rows and chunk of 8 z levels.  The block walks the
//                         pixel rectangle of the vertex's four neighbouring cells (every pixel is visited by its four corner vertices), each
//                         thread keeps the vertex's 8 x K sums in registers, and the block adds them in a fixed order (butterfly in the wave,
//                         then the waves in order) into one partial per slice.
//   k_bila_grid_finish    one thread per grid entry: the slices' partials in order.  Entries no pixel reaches are sums of nothing: exactly 0.
//   k_bila_tv / k_bila_tv_finish  the grids' total variation and its gradient: one thread per entry gathers its six neighbours, one partial sum per
//                         block, and one block adds the partials in a fixed order (double).
#include <algorithm>

#include "tn_common.h"

namespace {

constexpr int BB = 256;          // threads per block
constexpr int BTX = 64;          // pixels per block row (one wave)
constexpr int BTY = BB / BTX;    // pixel rows per block
constexpr int BLZ = 8;           // z levels a gradient block accumulates
constexpr int kMaxSide = 32768;  // largest image side
constexpr int kMaxGridSide = 256;  // largest grid side (every side is 2..256)
constexpr int kMaxSlices = 8;
constexpr int kMaxFrames = 1 << 20;
constexpr int64_t kMaxTvEntries = 1ll << 34;  // entries of all frames together (the launch has one block per 256)

struct BilaK {
  const float* grid;   // the frame's row [K][L][GH][GW]
  const float* img;    // [H][W][*], pixels ps floats apart
  int64_t ps;
  const float* v_out;  // backward: [H][W][C]
  float* out;          // forward: [H][W][C]
  float* v_img;        // backward: [H][W][C]
  float* part;         // backward: [S][K][L][GH][GW]
  float* v_grid;       // backward: [K][L][GH][GW]
  int H, W, GW, GH, L, S;
};

// one axis: u in [0, 1] -> lower index, upper index (clamped) and the weight of the upper one; `raw` is the coordinate before the clamp
__device__ __forceinline__ void bila_axis(float u, int size, int& i0, int& i1, float& t, float& raw) {
  const float m = (float)(size - 1);
  raw = u * m;
  const float c = fminf(fmaxf(raw, 0.0f), m);  // (a NaN coordinate lands on 0)
  const float f = floorf(c);
  i0 = (int)f;
  i1 = min(i0 + 1, size - 1);
  t = c - f;
}

template <int C>
__device__ __forceinline__ float bila_guidance(const float* p) {
  if constexpr (C == 3) {
    return (0.299f * p[0] + 0.587f * p[1]) + 0.114f * p[2];
  } else {
    return p[0];
  }
}

__device__ __forceinline__ float bila_lerp(float a, float b, float t) { return a + t * (b - a); }

struct BilaCell {
  int x0, x1, y0, y1, z0, z1;
  float tx, ty, tz, zraw;
};

template <int C>
__device__ __forceinline__ BilaCell bila_cell(const BilaK& k, int px, int py, const float* pix) {
  BilaCell c;
  float raw;
  bila_axis(((float)px + 0.5f) / (float)k.W, k.GW, c.x0, c.x1, c.tx, raw);
  bila_axis(((float)py + 0.5f) / (float)k.H, k.GH, c.y0, c.y1, c.ty, raw);
  bila_axis(bila_guidance<C>(pix), k.L, c.z0, c.z1, c.tz, c.zraw);
  return c;
}

// the K coefficients at the pixel (coef) and, with SLOPE, their difference between the two z levels (d coef / d clamped z coordinate)
template <int C, bool SLOPE>
__device__ __forceinline__ void bila_coefficients(const BilaK& k, const BilaCell& c, float* coef, float* slope) {
  constexpr int K = C * (C + 1);
  const int64_t plane = (int64_t)k.GH * k.GW, vol = plane * k.L;
  const int64_t r00 = c.z0 * plane + (int64_t)c.y0 * k.GW, r01 = c.z0 * plane + (int64_t)c.y1 * k.GW;
  const int64_t r10 = c.z1 * plane + (int64_t)c.y0 * k.GW, r11 = c.z1 * plane + (int64_t)c.y1 * k.GW;
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const float* g = k.grid + q * vol;
    const float a0 = bila_lerp(bila_lerp(g[r00 + c.x0], g[r00 + c.x1], c.tx), bila_lerp(g[r01 + c.x0], g[r01 + c.x1], c.tx), c.ty);
    const float a1 = bila_lerp(bila_lerp(g[r10 + c.x0], g[r10 + c.x1], c.tx), bila_lerp(g[r11 + c.x0], g[r11 + c.x1], c.tx), c.ty);
    coef[q] = bila_lerp(a0, a1, c.tz);
    if constexpr (SLOPE) slope[q] = a1 - a0;
  }
}

template <int C>
__global__ __launch_bounds__(BB) void k_bila_slice(BilaK k) {
  const int px = blockIdx.x * BTX + (threadIdx.x & (BTX - 1)), py = blockIdx.y * BTY + threadIdx.x / BTX;
  if (px >= k.W || py >= k.H) return;
  const int64_t p = (int64_t)py * k.W + px;
  float pix[C];
#pragma unroll
  for (int j = 0; j < C; ++j) pix[j] = k.img[p * k.ps + j];
  const BilaCell c = bila_cell<C>(k, px, py, pix);
  float coef[C * (C + 1)];
  bila_coefficients<C, false>(k, c, coef, nullptr);
#pragma unroll
  for (int o = 0; o < C; ++o) {
    float s = coef[o * (C + 1)] * pix[0];
#pragma unroll
    for (int j = 1; j < C; ++j) s += coef[o * (C + 1) + j] * pix[j];
    k.out[p * C + o] = s + coef[o * (C + 1) + C];
  }
}

template <int C>
__global__ __launch_bounds__(BB) void k_bila_slice_bwd_img(BilaK k) {
  const int px = blockIdx.x * BTX + (threadIdx.x & (BTX - 1)), py = blockIdx.y * BTY + threadIdx.x / BTX;
  if (px >= k.W || py >= k.H) return;
  const int64_t p = (int64_t)py * k.W + px;
  float pix[C], v[C];
#pragma unroll
  for (int j = 0; j < C; ++j) pix[j] = k.img[p * k.ps + j], v[j] = k.v_out[p * C + j];
  const BilaCell c = bila_cell<C>(k, px, py, pix);
  float coef[C * (C + 1)], slope[C * (C + 1)];
  bila_coefficients<C, true>(k, c, coef, slope);
  // d out_o / d z = slope(A_o) . pixel + slope(b_o); the clamp passes a gradient strictly inside (0, L - 1) only (grid_sample's border rule)
  float dz = 0.0f;
#pragma unroll
  for (int o = 0; o < C; ++o) {
    float s = slope[o * (C + 1)] * pix[0];
#pragma unroll
    for (int j = 1; j < C; ++j) s += slope[o * (C + 1) + j] * pix[j];
    dz += v[o] * (s + slope[o * (C + 1) + C]);
  }
  const float m = (float)(k.L - 1);
  dz = (c.zraw > 0.0f && c.zraw < m) ? dz * m : 0.0f;
  constexpr float luma[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
  for (int j = 0; j < C; ++j) {
    float s = v[0] * coef[j];
#pragma unroll
    for (int o = 1; o < C; ++o) s += v[o] * coef[o * (C + 1) + j];
    k.v_img[p * C + j] = s + dz * (C == 3 ? luma[j] : 1.0f);
  }
}

// blockIdx.x, .y: the vertex; blockIdx.z = slice * chunks + chunk of BLZ z levels
template <int C>
__global__ __launch_bounds__(BB) void k_bila_grid_partial(BilaK k, int chunks) {
  constexpr int K = C * (C + 1);
  __shared__ float red[BB / 64][BLZ * K];
  const int vx = blockIdx.x, vy = blockIdx.y, zc = blockIdx.z % chunks, s = blockIdx.z / chunks;
  const int t = threadIdx.x, zb = zc * BLZ;
  // a rectangle that holds every pixel whose cell has the vertex as a corner (coordinate in [v - 1, v + 1)), with slack: a pixel of another cell
  // inside it has weight 0 and is skipped
  const int xlo = max(((vx - 1) * k.W) / (k.GW - 1) - 2, 0), xhi = min(((vx + 1) * k.W + k.GW - 2) / (k.GW - 1) + 1, k.W - 1);
  const int ylo = max(((vy - 1) * k.H) / (k.GH - 1) - 2, 0), yhi = min(((vy + 1) * k.H + k.GH - 2) / (k.GH - 1) + 1, k.H - 1);
  const int rw = xhi - xlo + 1, rh = yhi - ylo + 1;
  const int y_first = ylo + (int)(((int64_t)s * rh) / k.S), y_end = ylo + (int)(((int64_t)(s + 1) * rh) / k.S);
  float acc[BLZ][K];
#pragma unroll
  for (int i = 0; i < BLZ; ++i)
#pragma unroll
    for (int q = 0; q < K; ++q) acc[i][q] = 0.0f;
  const int n = rw * (y_end - y_first);
  for (int i = t; i < n; i += BB) {
    const int ry = i / rw, px = xlo + (i - ry * rw), py = y_first + ry;
    const int64_t p = (int64_t)py * k.W + px;
    float pix[C];
#pragma unroll
    for (int j = 0; j < C; ++j) pix[j] = k.img[p * k.ps + j];
    const BilaCell c = bila_cell<C>(k, px, py, pix);
    const float wx = (c.x0 == vx ? 1.0f - c.tx : 0.0f) + (c.x1 == vx ? c.tx : 0.0f);
    const float wy = (c.y0 == vy ? 1.0f - c.ty : 0.0f) + (c.y1 == vy ? c.ty : 0.0f);
    const float wxy = wx * wy;
    if (wxy == 0.0f || (c.z1 < zb) || (c.z0 >= zb + BLZ)) continue;
    float u[K];  // d out / d coefficient times the upstream gradient
#pragma unroll
    for (int o = 0; o < C; ++o) {
      const float vo = k.v_out[p * C + o];
#pragma unroll
      for (int j = 0; j < C; ++j) u[o * (C + 1) + j] = vo * pix[j];
      u[o * (C + 1) + C] = vo;
    }
#pragma unroll
    for (int l = 0; l < BLZ; ++l) {
      const float wz = (c.z0 == zb + l ? 1.0f - c.tz : 0.0f) + (c.z1 == zb + l ? c.tz : 0.0f);
      const float w = wxy * wz;
#pragma unroll
      for (int q = 0; q < K; ++q) acc[l][q] += w * u[q];
    }
  }
  // the block's sums in a fixed order: butterfly within each wave, then the waves in order
#pragma unroll
  for (int l = 0; l < BLZ; ++l)
#pragma unroll
    for (int q = 0; q < K; ++q) {
      float a = acc[l][q];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
      if ((t & 63) == 0) red[t >> 6][l * K + q] = a;
    }
  __syncthreads();
  if (t < BLZ * K) {
    const int l = t / K, q = t - l * K, z = zb + l;
    if (z < k.L) {
      float a = red[0][t];
#pragma unroll
      for (int w = 1; w < BB / 64; ++w) a += red[w][t];
      const int64_t plane = (int64_t)k.GH * k.GW;
      k.part[(((int64_t)s * K + q) * k.L + z) * plane + (int64_t)vy * k.GW + vx] = a;
    }
  }
}

__global__ __launch_bounds__(BB) void k_bila_grid_finish(const float* part, int S, int64_t n, float* v_grid) {
  const int64_t i = (int64_t)blockIdx.x * BB + threadIdx.x;
  if (i >= n) return;
  float a = part[i];
  for (int s = 1; s < S; ++s) a += part[(int64_t)s * n + i];
  v_grid[i] = a;
}

struct TvK {
  const float* grids;  // [F K][L][GH][GW]
  float* grad;         // the same layout, or null
  float* part;         // one partial sum per block
  int64_t n;           // entries
  int GW, GH, L;
  float cx, cy, cz;     // 1 / entries of one frame's difference tensor, per axis
  float gx, gy, gz;     // 2 mult / (F entries of one frame's difference tensor), per axis
};

__global__ __launch_bounds__(BB) void k_bila_tv(TvK k) {
  __shared__ float red[BB / 64];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * BB + t;
  float e = 0.0f;
  if (i < k.n) {
    const int x = (int)(i % k.GW), y = (int)((i / k.GW) % k.GH), z = (int)((i / ((int64_t)k.GW * k.GH)) % k.L);
    const int64_t sy = k.GW, sz = (int64_t)k.GW * k.GH;
    const float c = k.grids[i];
    // forward differences carry the loss; the gradient gathers the differences on both sides
    const float fx = x + 1 < k.GW ? k.grids[i + 1] - c : 0.0f, bx = x > 0 ? c - k.grids[i - 1] : 0.0f;
    const float fy = y + 1 < k.GH ? k.grids[i + sy] - c : 0.0f, by = y > 0 ? c - k.grids[i - sy] : 0.0f;
    const float fz = z + 1 < k.L ? k.grids[i + sz] - c : 0.0f, bz = z > 0 ? c - k.grids[i - sz] : 0.0f;
    e = (k.cx * (fx * fx) + k.cy * (fy * fy)) + k.cz * (fz * fz);
    if (k.grad != nullptr) k.grad[i] = (k.gx * (bx - fx) + k.gy * (by - fy)) + k.gz * (bz - fz);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
  if ((t & 63) == 0) red[t >> 6] = e;
  __syncthreads();
  if (t == 0) {
    float s = red[0];
#pragma unroll
    for (int w = 1; w < BB / 64; ++w) s += red[w];
    k.part[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(BB) void k_bila_tv_finish(const float* part, int64_t n, double scale, float* out) {
  __shared__ double r[BB];
  const int t = threadIdx.x;
  double a = 0.0;
  for (int64_t i = t; i < n; i += BB) a += (double)part[i];
  r[t] = a;
  __syncthreads();
  for (int s = BB / 2; s > 0; s >>= 1) {
    if (t < s) r[t] += r[t + s];
    __syncthreads();
  }
  if (t == 0) out[0] = (float)(scale * r[0]);
}

bool bila_grid_ok(int32_t gw, int32_t gh, int32_t gl) {
  return gw >= 2 && gh >= 2 && gl >= 2 && gw <= kMaxGridSide && gh <= kMaxGridSide && gl <= kMaxGridSide;
}

bool bila_image_ok(int32_t H, int32_t W) { return H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide; }

// row slices of a vertex's pixel rectangle: more blocks on a large frame, one on a small one
int bila_slices(int32_t H) { return (int)std::min<int64_t>(std::max<int64_t>(H / 64, 1), kMaxSlices); }

int64_t bila_entries(int32_t C, int32_t gw, int32_t gh, int32_t gl) { return (int64_t)C * (C + 1) * gl * gh * gw; }

int bila_check(const char* who, const float* grids, int32_t F, int32_t row, int32_t C, int32_t gw, int32_t gh, int32_t gl, const float* image,
               int64_t ps, int32_t H, int32_t W) {
  TN_REQUIRE(grids && image, "%s: null pointer", who);
  TN_REQUIRE(C == 1 || C == 3, "%s: %d channels (1: thermal, 3: RGB)", who, C);
  TN_REQUIRE(bila_grid_ok(gw, gh, gl), "%s: grid %d x %d x %d, every side must be in 2..%d", who, gw, gh, gl, kMaxGridSide);
  TN_REQUIRE(F >= 1 && F <= kMaxFrames && row >= 0 && row < F, "%s: row %d of %d frames", who, row, F);
  TN_REQUIRE(bila_image_ok(H, W), "%s: %d x %d image, every side must be in 1..%d", who, H, W, kMaxSide);
  TN_REQUIRE(ps >= C, "%s: pixel stride %lld below the channel count %d", who, (long long)ps, C);
  return TN_OK;
}

}  // namespace

extern "C" int tn_bilagrid_slice(const float* grids, int32_t num_frames, int32_t row, int32_t channels, int32_t grid_w, int32_t grid_h, int32_t grid_l,
                                 const float* image, int64_t pixel_stride, int32_t height, int32_t width, float* out, tn_stream_t stream) {
  const int rc = bila_check("tn_bilagrid_slice", grids, num_frames, row, channels, grid_w, grid_h, grid_l, image, pixel_stride, height, width);
  if (rc != TN_OK) return rc;
  TN_REQUIRE(out, "tn_bilagrid_slice: null pointer");
  BilaK k = {};
  k.grid = grids + (int64_t)row * bila_entries(channels, grid_w, grid_h, grid_l);
  k.img = image, k.ps = pixel_stride, k.out = out;
  k.H = height, k.W = width, k.GW = grid_w, k.GH = grid_h, k.L = grid_l;
  const dim3 grid((unsigned)tn_cdiv(width, BTX), (unsigned)tn_cdiv(height, BTY));
  if (channels == 3) {
    hipLaunchKernelGGL(k_bila_slice<3>, grid, dim3(BB), 0, tn_s(stream), k);
  } else {
    hipLaunchKernelGGL(k_bila_slice<1>, grid, dim3(BB), 0, tn_s(stream), k);
  }
  TN_CHECK_LAUNCH("tn_bilagrid_slice");
  return TN_OK;
}

extern "C" int64_t tn_bilagrid_workspace_bytes(int32_t channels, int32_t grid_w, int32_t grid_h, int32_t grid_l, int32_t height, int32_t width) {
  if ((channels != 1 && channels != 3) || !bila_grid_ok(grid_w, grid_h, grid_l) || !bila_image_ok(height, width)) return -1;
  return (int64_t)bila_slices(height) * bila_entries(channels, grid_w, grid_h, grid_l) * (int64_t)sizeof(float);
}

extern "C" int tn_bilagrid_slice_backward(const float* grids, int32_t num_frames, int32_t row, int32_t channels, int32_t grid_w, int32_t grid_h,
                                          int32_t grid_l, const float* image, int64_t pixel_stride, int32_t height, int32_t width, const float* v_out,
                                          void* workspace, int64_t workspace_bytes, float* v_image, float* v_grid, tn_stream_t stream) {
  const int rc = bila_check("tn_bilagrid_slice_backward", grids, num_frames, row, channels, grid_w, grid_h, grid_l, image, pixel_stride, height, width);
  if (rc != TN_OK) return rc;
  TN_REQUIRE(v_out && workspace && v_image && v_grid, "tn_bilagrid_slice_backward: null pointer");
  const int64_t need = tn_bilagrid_workspace_bytes(channels, grid_w, grid_h, grid_l, height, width);
  TN_REQUIRE(workspace_bytes >= need, "tn_bilagrid_slice_backward: workspace of %lld bytes, %lld needed (tn_bilagrid_workspace_bytes)",
             (long long)workspace_bytes, (long long)need);
  const int64_t entries = bila_entries(channels, grid_w, grid_h, grid_l);
  BilaK k = {};
  k.grid = grids + (int64_t)row * entries;
  k.img = image, k.ps = pixel_stride, k.v_out = v_out, k.v_img = v_image, k.v_grid = v_grid;
  k.part = static_cast<float*>(workspace);
  k.H = height, k.W = width, k.GW = grid_w, k.GH = grid_h, k.L = grid_l, k.S = bila_slices(height);
  hipStream_t st = tn_s(stream);
  const dim3 pixels((unsigned)tn_cdiv(width, BTX), (unsigned)tn_cdiv(height, BTY));
  const int chunks = (int)tn_cdiv(grid_l, BLZ);
  const dim3 vertices((unsigned)grid_w, (unsigned)grid_h, (unsigned)(k.S * chunks));
  if (channels == 3) {
    hipLaunchKernelGGL(k_bila_slice_bwd_img<3>, pixels, dim3(BB), 0, st, k);
    TN_CHECK_LAUNCH("tn_bilagrid_slice_backward(image)");
    hipLaunchKernelGGL(k_bila_grid_partial<3>, vertices, dim3(BB), 0, st, k, chunks);
  } else {
    hipLaunchKernelGGL(k_bila_slice_bwd_img<1>, pixels, dim3(BB), 0, st, k);
    TN_CHECK_LAUNCH("tn_bilagrid_slice_backward(image)");
    hipLaunchKernelGGL(k_bila_grid_partial<1>, vertices, dim3(BB), 0, st, k, chunks);
  }
  TN_CHECK_LAUNCH("tn_bilagrid_slice_backward(grid)");
  hipLaunchKernelGGL(k_bila_grid_finish, dim3((unsigned)tn_cdiv(entries, BB)), dim3(BB), 0, st, (const float*)k.part, k.S, entries, v_grid);
  TN_CHECK_LAUNCH("tn_bilagrid_slice_backward(finish)");
  return TN_OK;
}

extern "C" int64_t tn_bilagrid_tv_workspace_bytes(int32_t num_frames, int32_t coefficients, int32_t grid_w, int32_t grid_h, int32_t grid_l) {
  if (num_frames < 1 || num_frames > kMaxFrames || coefficients < 1 || coefficients > 64 || !bila_grid_ok(grid_w, grid_h, grid_l)) return -1;
  const int64_t n = (int64_t)num_frames * coefficients * grid_l * grid_h * grid_w;
  if (n > kMaxTvEntries) return -1;
  return tn_cdiv(n, BB) * (int64_t)sizeof(float);
}

extern "C" int tn_bilagrid_tv(const float* grids, int32_t num_frames, int32_t coefficients, int32_t grid_w, int32_t grid_h, int32_t grid_l, float mult,
                              void* workspace, int64_t workspace_bytes, float* out, float* out_grad, tn_stream_t stream) {
  TN_REQUIRE(grids && workspace && out, "tn_bilagrid_tv: null pointer");
  TN_REQUIRE(bila_grid_ok(grid_w, grid_h, grid_l), "tn_bilagrid_tv: grid %d x %d x %d, every side must be in 2..%d", grid_w, grid_h, grid_l,
             kMaxGridSide);
  const int64_t need = tn_bilagrid_tv_workspace_bytes(num_frames, coefficients, grid_w, grid_h, grid_l);
  TN_REQUIRE(need >= 0, "tn_bilagrid_tv: %d frames of %d coefficients (1..%d frames, 1..64 coefficients, at most 2^34 entries)", num_frames, coefficients,
             kMaxFrames);
  TN_REQUIRE(workspace_bytes >= need, "tn_bilagrid_tv: workspace of %lld bytes, %lld needed (tn_bilagrid_tv_workspace_bytes)",
             (long long)workspace_bytes, (long long)need);
  TvK k = {};
  k.grids = grids, k.grad = out_grad, k.part = static_cast<float*>(workspace);
  k.GW = grid_w, k.GH = grid_h, k.L = grid_l;
  k.n = (int64_t)num_frames * coefficients * grid_l * grid_h * grid_w;
  const double K = coefficients;
  const double nx = K * grid_l * grid_h * (grid_w - 1), ny = K * grid_l * (grid_h - 1) * grid_w, nz = K * (grid_l - 1) * grid_h * grid_w;
  k.cx = (float)(1.0 / nx), k.cy = (float)(1.0 / ny), k.cz = (float)(1.0 / nz);
  const double g = 2.0 * (double)mult / (double)num_frames;
  k.gx = (float)(g / nx), k.gy = (float)(g / ny), k.gz = (float)(g / nz);
  hipStream_t st = tn_s(stream);
  const int64_t blocks = tn_cdiv(k.n, BB);
  hipLaunchKernelGGL(k_bila_tv, dim3((unsigned)blocks), dim3(BB), 0, st, k);
  TN_CHECK_LAUNCH("tn_bilagrid_tv");
  hipLaunchKernelGGL(k_bila_tv_finish, dim3(1), dim3(BB), 0, st, (const float*)k.part, blocks, (double)mult / (double)num_frames, out);
  TN_CHECK_LAUNCH("tn_bilagrid_tv(finish)");
  return TN_OK;
}
