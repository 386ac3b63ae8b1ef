// N4 training loss: splatfacto's (1 - lambda) * L1 + lambda * (1 - SSIM) of one rendered frame (nerfstudio/models/splatfacto.py:863-903), its
// value and its gradient with respect to the prediction.  SSIM is pytorch_msssim's (ssim / _ssim / gaussian_filter, v1.x): an 11-tap Gaussian
// window with sigma 1.5 applied separably as a VALID correlation, C1 = 0.01^2, C2 = 0.03^2, mean over the valid pixels and the channels.
//
// Three launches, no float atomics (bit-reproducible):
//   k_ssim_fwd    one block per 64 x 16 tile of the VALID map: stages x and y with their 10-pixel halo in LDS, filters the five moments
//                 (rows, then columns), writes the per-pixel SSIM's partial derivatives a = dS/d mu_x, b = dS/d G*(x^2), c = dS/d G*(xy) to
//                 the workspace (gradient requested) and one partial sum of S per block.
//   k_ssim_bwd    one block per 64 x 16 tile of the IMAGE: stages a, b, c with their halo (zero outside the valid map), filters them back with
//                 the transposed ("full") correlation and writes d loss / d pred = L1 term + SSIM term; one partial L1 sum per block.
//   k_loss_finish one block: the partial sums in a fixed order (double) -> [main_loss, L1, SSIM] on the device.
//
// Beside it, the resize of the resolution schedule's ground truth (splatfacto.py:648-657): tn_image_resize, one streaming launch (k_image_resize),
// and the undistortion of a training frame into a pinhole frame (what FullImageDatamanager._undistort_image does with OpenCV,
// data/datamanagers/full_images_datamanager.py:351-386): tn_image_undistort, one gathering launch (k_image_undistort).
//
// And the two image-space regularisers ThermalNeRF puts on the thermal render at the RGB cameras (model_components/losses.py:602-651, used at
// models/thermal_nerfacto.py:346-354), over every stride-1 2 x 2 window of a frame: tn_thermal_reg.  Two launches, no float atomics:
//   k_thermal_reg         one block per 64 x 16 tile of the frame: stages the thermal prediction and the ground truth's grey value with a 1-pixel
//                         halo in LDS; every pixel sums its right and its lower edge into the loss (an edge counts once per window that holds it)
//                         and GATHERS its gradient from its four edges; one partial sum per term and block.
//   k_thermal_reg_finish  one block: the partial sums in a fixed order (double) -> [tv_mult * tv, cross_mult * cc] on the device.
//
// And the two geometric priors on the depth render (tn_depth_loss): the L1 distance to a sensor depth and the 2 x 2 total variation of the depth,
// both only where the render is covered (accumulation > 0).  Their normalisations -- the number of valid pixels and of covered windows -- are data, so
// the gradient's constants exist only after the sums: three launches, no float atomics:
//   k_depth_loss<false>   one block per 64 x 16 tile: stages depth and coverage with a 1-pixel halo; one partial sum and one partial count per term.
//   k_depth_loss_finish   one block: sums and counts in a fixed order (double) -> the two losses and the two gradient constants on the device.
//   k_depth_loss<true>    the same tiles again (gradient requested): every pixel GATHERS its gradient from its own term and its four edges.
#include "tn_common.h"

namespace {

constexpr int LW = 11;            // window taps
constexpr int LR = LW - 1;        // halo
constexpr int LTX = 64;           // tile width (one wave of columns)
constexpr int LTY = 16;           // tile height
constexpr int LSX = LTX + LR;     // staged columns
constexpr int LSY = LTY + LR;     // staged rows
constexpr int LB = 256;           // threads per block
constexpr int LRO = LTY / (LB / LTX);  // output rows per thread in the column pass (4)
constexpr int LCO = 4;            // output columns per item in the row pass
constexpr float LC1 = 0.01f * 0.01f;
constexpr float LC2 = 0.03f * 0.03f;
static_assert(LTX % LCO == 0 && LTY % (LB / LTX) == 0, "tile shape");

struct LossK {
  const float* pred;
  const float* gt;
  int64_t ps, gs;  // pixel strides (floats)
  int H, W, C, Hv, Wv;
  float g[LW];
  float* abc;      // [C][3][Hv][Wv] or null (no gradient)
  float* grad;     // [H][W][C] or null
  float* part_s;   // one partial sum of S per k_ssim_fwd block
  float* part_l1;  // one partial sum of |x - y| per k_ssim_bwd block
  float cl;        // weight * (1 - lambda) / (C H W): the L1 term's gradient per unit sign
  float cs;        // -weight * lambda / (C Nq): the SSIM term's gradient per unit of (G^T a + 2 x G^T b + y G^T c)
};

// the block's sum of v in thread 0, in a fixed order (butterfly within each wave, then the waves in order)
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.0f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < LB / 64; ++i) s += red[i];
  }
  return s;
}

__global__ __launch_bounds__(LB) void k_ssim_fwd(LossK k) {
  __shared__ float sx[LSY][LSX], sy[LSY][LSX];
  __shared__ float hf[5][LSY][LTX];  // row-filtered x, y, x^2, y^2, xy
  __shared__ float red[LB / 64];
  const int t = threadIdx.x, tx0 = blockIdx.x * LTX, ty0 = blockIdx.y * LTY;
  const int col = t & (LTX - 1), r0 = (t / LTX) * LRO;
  const int64_t nv = (int64_t)k.Hv * k.Wv;
  float ssum = 0.0f;
  for (int c = 0; c < k.C; ++c) {
    for (int i = t; i < LSY * LSX; i += LB) {
      const int r = i / LSX, q = i - r * LSX, y = ty0 + r, x = tx0 + q;
      float a = 0.0f, b = 0.0f;
      if (y < k.H && x < k.W) {
        const int64_t p = (int64_t)y * k.W + x;
        a = k.pred[p * k.ps + c];
        b = k.gt[p * k.gs + c];
      }
      sx[r][q] = a;
      sy[r][q] = b;
    }
    __syncthreads();
    for (int i = t; i < LSY * (LTX / LCO); i += LB) {
      const int r = i / (LTX / LCO), q0 = (i % (LTX / LCO)) * LCO;
      float acc[5][LCO];
#pragma unroll
      for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int o = 0; o < LCO; ++o) acc[m][o] = 0.0f;
#pragma unroll
      for (int j = 0; j < LCO + LR; ++j) {
        const float xv = sx[r][q0 + j], yv = sy[r][q0 + j];
        const float v[5] = {xv, yv, xv * xv, yv * yv, xv * yv};
#pragma unroll
        for (int o = 0; o < LCO; ++o) {
          const int tap = j - o;
          if (tap >= 0 && tap < LW) {
#pragma unroll
            for (int m = 0; m < 5; ++m) acc[m][o] = fmaf(k.g[tap], v[m], acc[m][o]);
          }
        }
      }
#pragma unroll
      for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int o = 0; o < LCO; ++o) hf[m][r][q0 + o] = acc[m][o];
    }
    __syncthreads();
    float mo[5][LRO];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
      for (int o = 0; o < LRO; ++o) mo[m][o] = 0.0f;
#pragma unroll
    for (int j = 0; j < LRO + LR; ++j) {
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        const float v = hf[m][r0 + j][col];
#pragma unroll
        for (int o = 0; o < LRO; ++o) {
          const int tap = j - o;
          if (tap >= 0 && tap < LW) mo[m][o] = fmaf(k.g[tap], v, mo[m][o]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < LRO; ++o) {
      const int qy = ty0 + r0 + o, qx = tx0 + col;
      if (qy < k.Hv && qx < k.Wv) {
        const float mx = mo[0][o], my = mo[1][o];
        const float mxx = mx * mx, myy = my * my, mxy = mx * my;
        const float sxx = mo[2][o] - mxx, syy = mo[3][o] - myy, sxy = mo[4][o] - mxy;
        const float ad = mxx + myy + LC1, D = sxx + syy + LC2;
        const float A = (2.0f * mxy + LC1) / ad, B = (2.0f * sxy + LC2) / D;
        ssum += A * B;
        if (k.abc != nullptr) {
          const float da = B * (2.0f * my - 2.0f * mx * A) / ad + A * (2.0f * mx * B - 2.0f * my) / D;
          const float db = -A * B / D;
          const float dc = 2.0f * A / D;
          float* dst = k.abc + (int64_t)c * 3 * nv + (int64_t)qy * k.Wv + qx;
          dst[0] = da;
          dst[nv] = db;
          dst[2 * nv] = dc;
        }
      }
    }
    __syncthreads();  // sx / sy / hf are restaged for the next channel
  }
  const float s = block_sum(ssum, red);
  if (t == 0) k.part_s[blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(LB) void k_ssim_bwd(LossK k) {
  __shared__ float sm[3][LSY][LSX];  // a, b, c over the tile's window of the valid map (zero outside it)
  __shared__ float hf[3][LSY][LTX];
  __shared__ float red[LB / 64];
  const int t = threadIdx.x, tx0 = blockIdx.x * LTX, ty0 = blockIdx.y * LTY;
  const int col = t & (LTX - 1), r0 = (t / LTX) * LRO;
  const int64_t nv = (int64_t)k.Hv * k.Wv;
  const bool grad = k.grad != nullptr;  // block-uniform
  float l1 = 0.0f;
  for (int c = 0; c < k.C; ++c) {
    float gm[3][LRO];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
      for (int o = 0; o < LRO; ++o) gm[m][o] = 0.0f;
    if (grad) {
      const float* src = k.abc + (int64_t)c * 3 * nv;
      for (int i = t; i < LSY * LSX; i += LB) {
        const int r = i / LSX, q = i - r * LSX, y = ty0 - LR + r, x = tx0 - LR + q;
        const bool in = y >= 0 && y < k.Hv && x >= 0 && x < k.Wv;
        const int64_t p = in ? (int64_t)y * k.Wv + x : 0;
        sm[0][r][q] = in ? src[p] : 0.0f;
        sm[1][r][q] = in ? src[nv + p] : 0.0f;
        sm[2][r][q] = in ? src[2 * nv + p] : 0.0f;
      }
      __syncthreads();
      // pixel p receives from the valid pixels q = p - j, j = 0..10, with weight g[j]: staged column (p - tx0) + LR - j
      for (int i = t; i < LSY * (LTX / LCO); i += LB) {
        const int r = i / (LTX / LCO), q0 = (i % (LTX / LCO)) * LCO;
        float acc[3][LCO];
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
          for (int o = 0; o < LCO; ++o) acc[m][o] = 0.0f;
#pragma unroll
        for (int j = 0; j < LCO + LR; ++j) {
          const float v[3] = {sm[0][r][q0 + j], sm[1][r][q0 + j], sm[2][r][q0 + j]};
#pragma unroll
          for (int o = 0; o < LCO; ++o) {
            const int tap = LR - (j - o);
            if (tap >= 0 && tap < LW) {
#pragma unroll
              for (int m = 0; m < 3; ++m) acc[m][o] = fmaf(k.g[tap], v[m], acc[m][o]);
            }
          }
        }
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
          for (int o = 0; o < LCO; ++o) hf[m][r][q0 + o] = acc[m][o];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < LRO + LR; ++j) {
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          const float v = hf[m][r0 + j][col];
#pragma unroll
          for (int o = 0; o < LRO; ++o) {
            const int tap = LR - (j - o);
            if (tap >= 0 && tap < LW) gm[m][o] = fmaf(k.g[tap], v, gm[m][o]);
          }
        }
      }
    }
#pragma unroll
    for (int o = 0; o < LRO; ++o) {
      const int py = ty0 + r0 + o, px = tx0 + col;
      if (py < k.H && px < k.W) {
        const int64_t p = (int64_t)py * k.W + px;
        const float x = k.pred[p * k.ps + c], y = k.gt[p * k.gs + c];
        const float d = x - y;
        l1 += fabsf(d);
        if (grad) {
          const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
          const float s = gm[0][o] + 2.0f * x * gm[1][o] + y * gm[2][o];
          k.grad[p * k.C + c] = k.cl * sg + k.cs * s;
        }
      }
    }
    if (grad) __syncthreads();  // sm / hf are restaged for the next channel
  }
  const float s = block_sum(l1, red);
  if (t == 0) k.part_l1[blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(LB) void k_loss_finish(const float* part_s, int n_s, const float* part_l1, int n_l1, double n_valid, double n_all,
                                                    float lambda, float weight, float* out) {
  __shared__ double r_s[LB], r_l[LB];
  const int t = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int i = t; i < n_s; i += LB) a += (double)part_s[i];
  for (int i = t; i < n_l1; i += LB) b += (double)part_l1[i];
  r_s[t] = a;
  r_l[t] = b;
  __syncthreads();
  for (int s = LB / 2; s > 0; s >>= 1) {
    if (t < s) {
      r_s[t] += r_s[t + s];
      r_l[t] += r_l[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double ssim = r_s[0] / n_valid, l1 = r_l[0] / n_all;
    out[0] = (float)((double)weight * ((1.0 - (double)lambda) * l1 + (double)lambda * (1.0 - ssim)));
    out[1] = (float)l1;
    out[2] = (float)ssim;
  }
}

constexpr int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }

struct LossLayout {
  int64_t bx1, by1, bx2, by2, off_l1, off_abc, total;
};

LossLayout loss_layout(int32_t H, int32_t W, int32_t C) {
  LossLayout L;
  const int64_t Hv = H - LR, Wv = W - LR;
  L.bx1 = tn_cdiv(Wv, LTX), L.by1 = tn_cdiv(Hv, LTY);
  L.bx2 = tn_cdiv(W, LTX), L.by2 = tn_cdiv(H, LTY);
  L.off_l1 = align256(L.bx1 * L.by1 * 4);
  L.off_abc = L.off_l1 + align256(L.bx2 * L.by2 * 4);
  L.total = L.off_abc + align256(3 * (int64_t)C * Hv * Wv * 4);
  return L;
}

constexpr int32_t kMaxSide = 1 << 15;

// ---- tn_image_resize: bilinear, align_corners = False, no antialiasing (torch's upsample_bilinear2d in fp32).  A streaming kernel: one thread
// per output pixel (64 consecutive pixels of a row per wave, 4 rows per block), the four taps' channels loaded together, no LDS.
struct ResizeK {
  const void* in;
  float* out;
  int64_t ps;  // input pixel stride (elements)
  int H, W, h, w;
  float sy, sx;  // (float)in / out per axis
};

__device__ __forceinline__ float tap_value(float v) { return v; }
__device__ __forceinline__ float tap_value(uint8_t v) { return (float)v / 255.0f; }

// VEC (C = 2 or 4, the pixel aligned to its own size): one load per tap -- a dword for uint8 RGBA, 16 bytes for fp32
template <typename T, int C, bool VEC>
__device__ __forceinline__ void load_tap(const T* __restrict__ p, float (&v)[C]) {
  if constexpr (VEC) {
    struct alignas(C * sizeof(T)) Pixel {
      T c[C];
    };
    const Pixel px = *reinterpret_cast<const Pixel*>(p);
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = tap_value(px.c[c]);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = tap_value(p[c]);
  }
}

// area_pixel_compute_source_index + guard_index_and_lambda (ATen/native/UpSample.h): src = scale * (dst + 0.5) - 0.5 clamped below at 0,
// taps floor(src) and the next one (clamped to the last), weight of the second = src - floor(src)
__device__ __forceinline__ void resize_taps(float scale, int dst, int n_in, int& i0, int& i1, float& w1) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.0f ? 0.0f : s;
  i0 = min((int)s, n_in - 1);
  i1 = min(i0 + 1, n_in - 1);
  w1 = fminf(fmaxf(s - (float)i0, 0.0f), 1.0f);
}

template <typename T, int C, bool VEC>
__global__ __launch_bounds__(256) void k_image_resize(ResizeK k) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= k.w || y >= k.h) return;
  int x0, x1, y0, y1;
  float wx, wy;
  resize_taps(k.sx, x, k.W, x0, x1, wx);
  resize_taps(k.sy, y, k.H, y0, y1, wy);
  const T* in = static_cast<const T*>(k.in);
  const int64_t r0 = (int64_t)y0 * k.W, r1 = (int64_t)y1 * k.W;
  float v00[C], v01[C], v10[C], v11[C];
  load_tap<T, C, VEC>(in + (r0 + x0) * k.ps, v00);
  load_tap<T, C, VEC>(in + (r0 + x1) * k.ps, v01);
  load_tap<T, C, VEC>(in + (r1 + x0) * k.ps, v10);
  load_tap<T, C, VEC>(in + (r1 + x1) * k.ps, v11);
  const float ux = 1.0f - wx, uy = 1.0f - wy;
  float* o = k.out + ((int64_t)y * k.w + x) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) {  // along x, then along y
    const float top = ux * v00[c] + wx * v01[c];
    const float bot = ux * v10[c] + wx * v11[c];
    o[c] = uy * top + wy * bot;
  }
}

template <typename T, int C>
void launch_resize(const ResizeK& k, bool vec, hipStream_t st) {
  const dim3 grid((unsigned)tn_cdiv(k.w, 64), (unsigned)tn_cdiv(k.h, 4)), block(64, 4);
  if constexpr (C == 2 || C == 4) {
    if (vec) {
      hipLaunchKernelGGL((k_image_resize<T, C, true>), grid, block, 0, st, k);
      return;
    }
  }
  hipLaunchKernelGGL((k_image_resize<T, C, false>), grid, block, 0, st, k);
}

template <typename T>
void launch_resize_channels(const ResizeK& k, int C, hipStream_t st) {
  const bool vec = reinterpret_cast<uintptr_t>(k.in) % (C * sizeof(T)) == 0 && k.ps % C == 0;
  switch (C) {
    case 1: launch_resize<T, 1>(k, vec, st); break;
    case 2: launch_resize<T, 2>(k, vec, st); break;
    case 3: launch_resize<T, 3>(k, vec, st); break;
    default: launch_resize<T, 4>(k, vec, st); break;
  }
}

// ---- tn_image_undistort: output pixel (u, v) of the pinhole camera `n*` looks along (x, y); the distortion polynomial of tn_raygen's model
// (tn_misc.hip: undistort() inverts it) takes that to the source camera's (x_d, y_d), closed form; the frame is read there bilinearly.  A gather
// whose source addresses are nearly the destination's: the launch shape of k_image_resize (64 consecutive pixels of a row per wave, 4 rows per
// block, every channel of a pixel in one thread), no LDS.
__device__ __forceinline__ void store_value(float* o, float v) { *o = v; }
__device__ __forceinline__ void store_value(uint8_t* o, float v) { *o = (uint8_t)rintf(255.0f * fminf(fmaxf(v, 0.0f), 1.0f)); }

struct UndistortK {
  const void* in;
  void* out;
  int64_t ps;  // input pixel stride (elements)
  int H, W;
  TnUndistort p;
};

// taps floor(s) and floor(s) + 1 with their indices clamped to the frame, weight of the second = s - floor(s).  s is clamped to [-1, n] first
// (a NaN becomes -1), so the conversion to int is defined and both indices are in bounds whatever the camera.
__device__ __forceinline__ void undistort_taps(float s, int n, int& i0, int& i1, float& w1) {
  s = fminf(fmaxf(s, -1.0f), (float)n);
  const float f = floorf(s);
  const int i = (int)f;
  w1 = s - f;
  i0 = min(max(i, 0), n - 1);
  i1 = min(max(i + 1, 0), n - 1);
}

template <typename T, typename TO, int C, bool VEC>
__global__ __launch_bounds__(256) void k_image_undistort(UndistortK k) {
  const int u = blockIdx.x * 64 + threadIdx.x, v = blockIdx.y * 4 + threadIdx.y;
  if (u >= k.W || v >= k.H) return;
  const TnUndistort& p = k.p;
  const float x = ((float)u + 0.5f - p.new_cx) / p.new_fx, y = ((float)v + 0.5f - p.new_cy) / p.new_fy;
  const float r = x * x + y * y;
  const float d = 1.0f + r * (p.k[0] + r * (p.k[1] + r * (p.k[2] + r * p.k[3])));
  const float xd = d * x + 2.0f * p.k[4] * x * y + p.k[5] * (r + 2.0f * x * x);
  const float yd = d * y + 2.0f * p.k[5] * x * y + p.k[4] * (r + 2.0f * y * y);
  int x0, x1, y0, y1;
  float wx, wy;
  undistort_taps(p.fx * xd + p.cx - 0.5f, k.W, x0, x1, wx);
  undistort_taps(p.fy * yd + p.cy - 0.5f, k.H, y0, y1, wy);
  const T* in = static_cast<const T*>(k.in);
  const int64_t r0 = (int64_t)y0 * k.W, r1 = (int64_t)y1 * k.W;
  float v00[C], v01[C], v10[C], v11[C];
  load_tap<T, C, VEC>(in + (r0 + x0) * k.ps, v00);
  load_tap<T, C, VEC>(in + (r0 + x1) * k.ps, v01);
  load_tap<T, C, VEC>(in + (r1 + x0) * k.ps, v10);
  load_tap<T, C, VEC>(in + (r1 + x1) * k.ps, v11);
  const float ux = 1.0f - wx, uy = 1.0f - wy;
  TO* o = static_cast<TO*>(k.out) + ((int64_t)v * k.W + u) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) {  // along x, then along y
    const float top = ux * v00[c] + wx * v01[c];
    const float bot = ux * v10[c] + wx * v11[c];
    store_value(o + c, uy * top + wy * bot);
  }
}

template <typename T, typename TO, int C>
void launch_undistort(const UndistortK& k, bool vec, hipStream_t st) {
  const dim3 grid((unsigned)tn_cdiv(k.W, 64), (unsigned)tn_cdiv(k.H, 4)), block(64, 4);
  if constexpr (C == 2 || C == 4) {
    if (vec) {
      hipLaunchKernelGGL((k_image_undistort<T, TO, C, true>), grid, block, 0, st, k);
      return;
    }
  }
  hipLaunchKernelGGL((k_image_undistort<T, TO, C, false>), grid, block, 0, st, k);
}

template <typename T, typename TO>
void launch_undistort_channels(const UndistortK& k, int C, hipStream_t st) {
  const bool vec = reinterpret_cast<uintptr_t>(k.in) % (C * sizeof(T)) == 0 && k.ps % C == 0;
  switch (C) {
    case 1: launch_undistort<T, TO, 1>(k, vec, st); break;
    case 2: launch_undistort<T, TO, 2>(k, vec, st); break;
    case 3: launch_undistort<T, TO, 3>(k, vec, st); break;
    default: launch_undistort<T, TO, 4>(k, vec, st); break;
  }
}

// ---- tn_thermal_reg.  The windows' terms are edge terms: the window at (y, x) holds the horizontal edges (y, x)-(y, x+1) and (y+1, x)-(y+1, x+1) and
// the vertical edges (y, x)-(y+1, x) and (y, x+1)-(y+1, x+1), so a horizontal edge of row y is in as many windows as y has window rows around it
// (rows y - 1 and y: 2 inside the frame, 1 on its first and last row), a vertical edge of column x likewise.  With those multiplicities
//   sum over windows = sum over pixels of  mh(y) * |right edge| + mv(x) * |lower edge|
// and a pixel's gradient is a signed count over its four edges: a small integer, exact in fp32 whatever the order, times the term's constant.
constexpr int RTX = 64;                // tile width (one wave of columns)
constexpr int RTY = 16;                // tile height
constexpr int RSX = RTX + 2;           // staged columns (1-pixel halo)
constexpr int RSY = RTY + 2;           // staged rows
constexpr int RRO = RTY / (LB / RTX);  // rows per thread (4)
static_assert(RTY % (LB / RTX) == 0, "tile shape");

struct RegK {
  const float* pred;  // thermal prediction, pixels ps floats apart
  const float* gt;    // RGB ground truth, pixels gs floats apart
  int64_t ps, gs;
  int H, W;
  float* grad;     // [H][W] or null
  float* part_tv;  // one partial sum of the TV edge terms per block
  float* part_cc;  // one partial sum of the cross-channel edge terms per block
  float ctv, ccc;  // mult * 0.25 / windows: a term's gradient per unit of its signed edge count
};

__device__ __forceinline__ float sign0(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }  // sign(0) = 0, as torch.abs' backward

template <bool TV, bool CC>
__global__ __launch_bounds__(LB) void k_thermal_reg(RegK k) {
  __shared__ float st[RSY][RSX];           // thermal prediction (zero outside the frame: those edges carry weight 0)
  __shared__ float sq[CC ? RSY : 1][RSX];  // mean over the channels of the RGB ground truth
  __shared__ float red_tv[LB / 64], red_cc[LB / 64];
  const int t = threadIdx.x, tx0 = blockIdx.x * RTX, ty0 = blockIdx.y * RTY;
  for (int i = t; i < RSY * RSX; i += LB) {
    const int r = i / RSX, q = i - r * RSX, y = ty0 - 1 + r, x = tx0 - 1 + q;
    float a = 0.0f, b = 0.0f;
    if (y >= 0 && y < k.H && x >= 0 && x < k.W) {
      const int64_t p = (int64_t)y * k.W + x;
      a = k.pred[p * k.ps];
      if constexpr (CC) {
        const float* g = k.gt + p * k.gs;
        b = (g[0] + g[1] + g[2]) / 3.0f;
      }
    }
    st[r][q] = a;
    if constexpr (CC) sq[r][q] = b;
  }
  __syncthreads();
  const int col = t & (RTX - 1), r0 = (t / RTX) * RRO;
  const int px = tx0 + col, lc = col + 1;
  const float hasL = px > 0 ? 1.0f : 0.0f, hasR = px < k.W - 1 ? 1.0f : 0.0f, mv = hasL + hasR;
  float ltv = 0.0f, lcc = 0.0f;
#pragma unroll
  for (int o = 0; o < RRO; ++o) {
    const int py = ty0 + r0 + o, lr = r0 + o + 1;
    if (py < k.H && px < k.W) {
      const float hasU = py > 0 ? 1.0f : 0.0f, hasD = py < k.H - 1 ? 1.0f : 0.0f, mh = hasU + hasD;
      const float wL = mh * hasL, wR = mh * hasR, wU = mv * hasU, wD = mv * hasD;  // windows that hold each of the pixel's edges
      const float t0 = st[lr][lc], tL = st[lr][lc - 1], tR = st[lr][lc + 1], tU = st[lr - 1][lc], tD = st[lr + 1][lc];
      float g = 0.0f;
      if constexpr (TV) {  // |p0 - p1|, |p2 - p3| (left - right) and |p0 - p2|, |p1 - p3| (upper - lower)
        const float eL = tL - t0, eR = t0 - tR, eU = tU - t0, eD = t0 - tD;
        ltv += wR * fabsf(eR) + wD * fabsf(eD);
        g = k.ctv * (wR * sign0(eR) - wL * sign0(eL) + wD * sign0(eD) - wU * sign0(eU));
      }
      if constexpr (CC) {  // |(p1 - p0) - (q1 - q0)|, ... : the later pixel minus the earlier one, thermal minus grey
        const float q0 = sq[lr][lc];
        const float cL = (t0 - tL) - (q0 - sq[lr][lc - 1]), cR = (tR - t0) - (sq[lr][lc + 1] - q0);
        const float cU = (t0 - tU) - (q0 - sq[lr - 1][lc]), cD = (tD - t0) - (sq[lr + 1][lc] - q0);
        lcc += wR * fabsf(cR) + wD * fabsf(cD);
        g += k.ccc * (wL * sign0(cL) - wR * sign0(cR) + wU * sign0(cU) - wD * sign0(cD));
      }
      if (k.grad != nullptr) k.grad[(int64_t)py * k.W + px] = g;
    }
  }
  const int b = blockIdx.y * gridDim.x + blockIdx.x;
  if constexpr (TV) {
    const float s = block_sum(ltv, red_tv);
    if (t == 0) k.part_tv[b] = s;
  }
  if constexpr (CC) {
    const float s = block_sum(lcc, red_cc);
    if (t == 0) k.part_cc[b] = s;
  }
}

// a term that is switched off (null partials) is exactly 0
__global__ __launch_bounds__(LB) void k_thermal_reg_finish(const float* part_tv, const float* part_cc, int n, double stv, double scc, float* out) {
  __shared__ double r_tv[LB], r_cc[LB];
  const int t = threadIdx.x;
  double a = 0.0, b = 0.0;
  if (part_tv != nullptr)
    for (int i = t; i < n; i += LB) a += (double)part_tv[i];
  if (part_cc != nullptr)
    for (int i = t; i < n; i += LB) b += (double)part_cc[i];
  r_tv[t] = a;
  r_cc[t] = b;
  __syncthreads();
  for (int s = LB / 2; s > 0; s >>= 1) {
    if (t < s) {
      r_tv[t] += r_tv[t + s];
      r_cc[t] += r_cc[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    out[0] = part_tv != nullptr ? (float)(stv * r_tv[0]) : 0.0f;
    out[1] = part_cc != nullptr ? (float)(scc * r_cc[0]) : 0.0f;
  }
}

// ---- tn_depth_loss.  depth_loss = mean |depth - sensor| over the pixels with accumulation > 0 and a finite, positive sensor depth; depth_tv_loss =
// the total variation above (0.25 * mean of the four absolute differences) over the stride-1 2 x 2 windows whose FOUR pixels have accumulation > 0 --
// an uncovered pixel holds the frame's fill value, which would put an edge on every silhouette.  Either is 0 without a pixel / window to average over.
// As edge terms: a horizontal edge sits in the window above and the window below it, a vertical edge in the window left and right of it, and it counts
// once per COVERED window among the two; a pixel's windows are the four it is a corner of (NW, NE, SW, SE by the window's position around the pixel).
struct DepthLossK {
  const float* depth;   // [H][W]
  const float* alpha;   // [H][W] accumulation
  const float* sensor;  // [H][W] or null (no depth_loss)
  int H, W;
  int tv;               // the TV term is on
  float* grad;          // GRAD: [H][W]
  float* part;          // [4][blocks]: sum |depth - sensor|, its pixels, sum of the TV edge terms, covered windows
  int64_t part_stride;  // floats between the four
  const float* scale;   // GRAD: [2] on the device: depth_mult / pixels, tv_mult * 0.25 / windows (0 where there are none)
};

template <bool GRAD>
__global__ __launch_bounds__(LB) void k_depth_loss(DepthLossK k) {
  __shared__ float sd[RSY][RSX];    // depth (0 outside the frame)
  __shared__ float scv[RSY][RSX];   // 1 where the pixel is inside the frame and covered, else 0
  __shared__ float red[4][LB / 64];
  const int t = threadIdx.x, tx0 = blockIdx.x * RTX, ty0 = blockIdx.y * RTY;
  for (int i = t; i < RSY * RSX; i += LB) {
    const int r = i / RSX, q = i - r * RSX, y = ty0 - 1 + r, x = tx0 - 1 + q;
    float a = 0.0f, c = 0.0f;
    if (y >= 0 && y < k.H && x >= 0 && x < k.W) {
      const int64_t p = (int64_t)y * k.W + x;
      a = k.depth[p];
      c = k.alpha[p] > 0.0f ? 1.0f : 0.0f;
    }
    sd[r][q] = a;
    scv[r][q] = c;
  }
  __syncthreads();
  float c_d = 0.0f, c_tv = 0.0f;
  if constexpr (GRAD) c_d = k.scale[0], c_tv = k.scale[1];
  const int col = t & (RTX - 1), r0 = (t / RTX) * RRO;
  const int px = tx0 + col, lc = col + 1;
  float l_d = 0.0f, n_d = 0.0f, l_tv = 0.0f, n_tv = 0.0f;
#pragma unroll
  for (int o = 0; o < RRO; ++o) {
    const int py = ty0 + r0 + o, lr = r0 + o + 1;
    if (py < k.H && px < k.W) {
      const int64_t p = (int64_t)py * k.W + px;
      const float t0 = sd[lr][lc];
      float g = 0.0f;
      if (k.sensor != nullptr) {
        const float s = k.sensor[p];
        if (scv[lr][lc] > 0.0f && s > 0.0f && s <= 3.402823466e38f) {  // covered, and the sensor depth finite and positive (a NaN fails both)
          const float e = t0 - s;
          l_d += fabsf(e);
          n_d += 1.0f;
          g = c_d * sign0(e);
        }
      }
      if (k.tv) {
        // the four windows around the pixel; a window is covered when its four pixels are (one outside the frame is not)
        const float cN = scv[lr - 1][lc] * scv[lr][lc], cS = scv[lr][lc] * scv[lr + 1][lc];
        const float nw = cN * scv[lr - 1][lc - 1] * scv[lr][lc - 1], ne = cN * scv[lr - 1][lc + 1] * scv[lr][lc + 1];
        const float sw = cS * scv[lr][lc - 1] * scv[lr + 1][lc - 1], se = cS * scv[lr][lc + 1] * scv[lr + 1][lc + 1];
        const float wL = nw + sw, wR = ne + se, wU = nw + ne, wD = sw + se;  // covered windows that hold each of the pixel's edges
        const float eL = sd[lr][lc - 1] - t0, eR = t0 - sd[lr][lc + 1], eU = sd[lr - 1][lc] - t0, eD = t0 - sd[lr + 1][lc];
        if constexpr (GRAD) {
          g += c_tv * (wR * sign0(eR) - wL * sign0(eL) + wD * sign0(eD) - wU * sign0(eU));
        } else {
          l_tv += wR * fabsf(eR) + wD * fabsf(eD);  // (an edge of weight 0 joins finite values: the fill value is finite)
          n_tv += se;                               // the window whose top-left pixel this is
        }
      }
      if constexpr (GRAD) k.grad[p] = g;
    }
  }
  if constexpr (!GRAD) {
    const int b = blockIdx.y * gridDim.x + blockIdx.x;
    const float v[4] = {l_d, n_d, l_tv, n_tv};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float sum = block_sum(v[j], red[j]);
      if (t == 0) k.part[j * k.part_stride + b] = sum;
    }
  }
}

// out = [depth_mult * depth_loss, tv_mult * depth_tv_loss]; scale = the gradient's two constants.  A term without pixels / windows is exactly 0.
__global__ __launch_bounds__(LB) void k_depth_loss_finish(const float* part, int64_t part_stride, int n, double depth_mult, double tv_mult, float* out,
                                                          float* scale) {
  __shared__ double r[4][LB];
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double a = 0.0;
    for (int i = t; i < n; i += LB) a += (double)part[j * part_stride + i];
    r[j][t] = a;
  }
  __syncthreads();
  for (int s = LB / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j][t] += r[j][t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double cd = r[1][0] > 0.0 ? depth_mult / r[1][0] : 0.0, ctv = r[3][0] > 0.0 ? tv_mult * 0.25 / r[3][0] : 0.0;
    out[0] = (float)(cd * r[0][0]);
    out[1] = (float)(ctv * r[2][0]);
    scale[0] = (float)cd;
    scale[1] = (float)ctv;
  }
}

struct DepthLossLayout {
  int64_t bx, by, part_stride, off_scale, total;
};

DepthLossLayout depth_loss_layout(int32_t H, int32_t W) {
  DepthLossLayout L;
  L.bx = tn_cdiv(W, RTX), L.by = tn_cdiv(H, RTY);
  L.part_stride = align256(L.bx * L.by * 4) / 4;
  L.off_scale = 4 * L.part_stride * 4;
  L.total = L.off_scale + 256;
  return L;
}

struct RegLayout {
  int64_t bx, by, off_cc, total;
};

RegLayout reg_layout(int32_t H, int32_t W) {
  RegLayout L;
  L.bx = tn_cdiv(W, RTX), L.by = tn_cdiv(H, RTY);
  L.off_cc = align256(L.bx * L.by * 4);
  L.total = 2 * L.off_cc;
  return L;
}

}  // namespace

extern "C" int tn_image_resize(const void* in, int32_t in_dtype, int64_t in_pixel_stride, int32_t in_height, int32_t in_width, int32_t channels,
                               float* out, int32_t out_height, int32_t out_width, tn_stream_t stream) {
  TN_REQUIRE(in && out, "tn_image_resize: null pointer");
  TN_REQUIRE(in_dtype == TN_IMAGE_F32 || in_dtype == TN_IMAGE_U8, "tn_image_resize: input type %d (TN_IMAGE_F32 or TN_IMAGE_U8)", in_dtype);
  TN_REQUIRE(channels >= 1 && channels <= 4, "tn_image_resize: %d channels (1..4)", channels);
  TN_REQUIRE(in_pixel_stride >= channels, "tn_image_resize: pixel stride %lld below the channel count %d", (long long)in_pixel_stride, channels);
  TN_REQUIRE(in_height >= 1 && in_width >= 1 && out_height >= 1 && out_width >= 1, "tn_image_resize: %d x %d -> %d x %d, every side must be positive",
             in_height, in_width, out_height, out_width);
  TN_REQUIRE(in_height <= kMaxSide && in_width <= kMaxSide && out_height <= kMaxSide && out_width <= kMaxSide,
             "tn_image_resize: %d x %d -> %d x %d is larger than %d on a side", in_height, in_width, out_height, out_width, kMaxSide);
  ResizeK k;
  k.in = in, k.out = out, k.ps = in_pixel_stride;
  k.H = in_height, k.W = in_width, k.h = out_height, k.w = out_width;
  k.sy = (float)in_height / (float)out_height, k.sx = (float)in_width / (float)out_width;
  if (in_dtype == TN_IMAGE_U8)
    launch_resize_channels<uint8_t>(k, channels, tn_s(stream));
  else
    launch_resize_channels<float>(k, channels, tn_s(stream));
  TN_CHECK_LAUNCH("tn_image_resize");
  return TN_OK;
}

extern "C" int tn_image_undistort(const void* in, int32_t in_dtype, int64_t in_pixel_stride, int32_t height, int32_t width, int32_t channels,
                                  void* out, int32_t out_dtype, const TnUndistort* params, tn_stream_t stream) {
  TN_REQUIRE(in && out && params, "tn_image_undistort: null pointer");
  TN_REQUIRE(in_dtype == TN_IMAGE_F32 || in_dtype == TN_IMAGE_U8, "tn_image_undistort: input type %d (TN_IMAGE_F32 or TN_IMAGE_U8)", in_dtype);
  TN_REQUIRE(out_dtype == TN_IMAGE_F32 || out_dtype == TN_IMAGE_U8, "tn_image_undistort: output type %d (TN_IMAGE_F32 or TN_IMAGE_U8)", out_dtype);
  TN_REQUIRE(channels >= 1 && channels <= 4, "tn_image_undistort: %d channels (1..4)", channels);
  TN_REQUIRE(in_pixel_stride >= channels, "tn_image_undistort: pixel stride %lld below the channel count %d", (long long)in_pixel_stride, channels);
  TN_REQUIRE(height >= 1 && width >= 1, "tn_image_undistort: %d x %d image, every side must be positive", height, width);
  TN_REQUIRE(height <= kMaxSide && width <= kMaxSide, "tn_image_undistort: %d x %d image is larger than %d on a side", height, width, kMaxSide);
  const TnUndistort& p = *params;
  TN_REQUIRE(std::isfinite(p.fx) && std::isfinite(p.fy) && std::isfinite(p.new_fx) && std::isfinite(p.new_fy) && p.fx > 0.0f && p.fy > 0.0f &&
                 p.new_fx > 0.0f && p.new_fy > 0.0f,
             "tn_image_undistort: focal lengths %g %g -> %g %g must be finite and positive", (double)p.fx, (double)p.fy, (double)p.new_fx,
             (double)p.new_fy);
  bool finite = std::isfinite(p.cx) && std::isfinite(p.cy) && std::isfinite(p.new_cx) && std::isfinite(p.new_cy);
  for (int i = 0; i < 6; ++i) finite = finite && std::isfinite(p.k[i]);
  TN_REQUIRE(finite, "tn_image_undistort: non-finite principal point or distortion coefficient");
  UndistortK k;
  k.in = in, k.out = out, k.ps = in_pixel_stride, k.H = height, k.W = width, k.p = p;
  hipStream_t st = tn_s(stream);
  if (in_dtype == TN_IMAGE_U8) {
    if (out_dtype == TN_IMAGE_U8)
      launch_undistort_channels<uint8_t, uint8_t>(k, channels, st);
    else
      launch_undistort_channels<uint8_t, float>(k, channels, st);
  } else {
    if (out_dtype == TN_IMAGE_U8)
      launch_undistort_channels<float, uint8_t>(k, channels, st);
    else
      launch_undistort_channels<float, float>(k, channels, st);
  }
  TN_CHECK_LAUNCH("tn_image_undistort");
  return TN_OK;
}

extern "C" int64_t tn_image_loss_workspace_bytes(int32_t height, int32_t width, int32_t channels) {
  if (height < LW || width < LW || height > kMaxSide || width > kMaxSide || channels < 1 || channels > 4) return -1;
  return loss_layout(height, width, channels).total;
}

extern "C" int tn_image_loss(const float* pred, int64_t pred_pixel_stride, const float* gt, int64_t gt_pixel_stride, int32_t height, int32_t width,
                             int32_t channels, float ssim_lambda, float weight, void* workspace, int64_t workspace_bytes, float* out_loss,
                             float* out_grad, tn_stream_t stream) {
  TN_REQUIRE(pred && gt && workspace && out_loss, "tn_image_loss: null pointer");
  TN_REQUIRE(height >= LW && width >= LW, "tn_image_loss: %d x %d image, SSIM's %d-tap window needs at least %d x %d", height, width, LW, LW, LW);
  TN_REQUIRE(height <= kMaxSide && width <= kMaxSide, "tn_image_loss: %d x %d image is larger than %d on a side", height, width, kMaxSide);
  TN_REQUIRE(channels >= 1 && channels <= 4, "tn_image_loss: %d channels (1..4)", channels);
  TN_REQUIRE(pred_pixel_stride >= channels && gt_pixel_stride >= channels, "tn_image_loss: pixel strides %lld / %lld below the channel count %d",
             (long long)pred_pixel_stride, (long long)gt_pixel_stride, channels);
  const LossLayout L = loss_layout(height, width, channels);
  TN_REQUIRE(workspace_bytes >= L.total, "tn_image_loss: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  LossK k;
  k.pred = pred, k.gt = gt, k.ps = pred_pixel_stride, k.gs = gt_pixel_stride;
  k.H = height, k.W = width, k.C = channels, k.Hv = height - LR, k.Wv = width - LR;
  // gaussian_filter's window: coords = arange(11) - 5, g = exp(-coords^2 / (2 sigma^2)), g /= g.sum(), in fp32
  float gs = 0.0f;
  for (int i = 0; i < LW; ++i) {
    const float x = (float)(i - LW / 2);
    k.g[i] = expf(-(x * x) / (2.0f * 1.5f * 1.5f));
    gs += k.g[i];
  }
  for (int i = 0; i < LW; ++i) k.g[i] /= gs;
  char* ws = static_cast<char*>(workspace);
  k.part_s = reinterpret_cast<float*>(ws);
  k.part_l1 = reinterpret_cast<float*>(ws + L.off_l1);
  k.abc = out_grad ? reinterpret_cast<float*>(ws + L.off_abc) : nullptr;
  k.grad = out_grad;
  const double n_valid = (double)channels * k.Hv * k.Wv, n_all = (double)channels * height * width;
  k.cl = (float)((double)weight * (1.0 - (double)ssim_lambda) / n_all);
  k.cs = (float)(-(double)weight * (double)ssim_lambda / n_valid);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_ssim_fwd, dim3((unsigned)L.bx1, (unsigned)L.by1), dim3(LB), 0, st, k);
  TN_CHECK_LAUNCH("tn_image_loss(ssim_fwd)");
  hipLaunchKernelGGL(k_ssim_bwd, dim3((unsigned)L.bx2, (unsigned)L.by2), dim3(LB), 0, st, k);
  TN_CHECK_LAUNCH("tn_image_loss(ssim_bwd)");
  hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(LB), 0, st, k.part_s, (int)(L.bx1 * L.by1), k.part_l1, (int)(L.bx2 * L.by2), n_valid, n_all,
                     ssim_lambda, weight, out_loss);
  TN_CHECK_LAUNCH("tn_image_loss(finish)");
  return TN_OK;
}

extern "C" int64_t tn_thermal_reg_workspace_bytes(int32_t height, int32_t width) {
  if (height < 2 || width < 2 || height > kMaxSide || width > kMaxSide) return -1;
  return reg_layout(height, width).total;
}

extern "C" int tn_thermal_reg(const float* pred_thermal, int64_t pred_pixel_stride, const float* gt_rgb, int64_t gt_pixel_stride, int32_t height,
                              int32_t width, float tv_mult, float cross_mult, void* workspace, int64_t workspace_bytes, float* out_loss,
                              float* out_grad, tn_stream_t stream) {
  TN_REQUIRE(pred_thermal && gt_rgb && workspace && out_loss, "tn_thermal_reg: null pointer");
  TN_REQUIRE(height >= 2 && width >= 2, "tn_thermal_reg: %d x %d image, a 2 x 2 window needs at least 2 x 2", height, width);
  TN_REQUIRE(height <= kMaxSide && width <= kMaxSide, "tn_thermal_reg: %d x %d image is larger than %d on a side", height, width, kMaxSide);
  TN_REQUIRE(pred_pixel_stride >= 1 && gt_pixel_stride >= 3, "tn_thermal_reg: pixel strides %lld / %lld below the channel counts 1 / 3",
             (long long)pred_pixel_stride, (long long)gt_pixel_stride);
  const RegLayout L = reg_layout(height, width);
  TN_REQUIRE(workspace_bytes >= L.total, "tn_thermal_reg: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  const bool tv = tv_mult != 0.0f, cc = cross_mult != 0.0f;
  RegK k;
  k.pred = pred_thermal, k.gt = gt_rgb, k.ps = pred_pixel_stride, k.gs = gt_pixel_stride;
  k.H = height, k.W = width, k.grad = out_grad;
  char* ws = static_cast<char*>(workspace);
  k.part_tv = tv ? reinterpret_cast<float*>(ws) : nullptr;
  k.part_cc = cc ? reinterpret_cast<float*>(ws + L.off_cc) : nullptr;
  const double windows = (double)(height - 1) * (double)(width - 1);
  const double stv = (double)tv_mult * 0.25 / windows, scc = (double)cross_mult * 0.25 / windows;
  k.ctv = (float)stv, k.ccc = (float)scc;
  hipStream_t st = tn_s(stream);
  const dim3 grid((unsigned)L.bx, (unsigned)L.by);
  if (tv && cc) {
    hipLaunchKernelGGL((k_thermal_reg<true, true>), grid, dim3(LB), 0, st, k);
  } else if (tv) {
    hipLaunchKernelGGL((k_thermal_reg<true, false>), grid, dim3(LB), 0, st, k);
  } else if (cc) {
    hipLaunchKernelGGL((k_thermal_reg<false, true>), grid, dim3(LB), 0, st, k);
  } else if (out_grad != nullptr) {  // both terms off: no arithmetic, a zero gradient
    const hipError_t e = hipMemsetAsync(out_grad, 0, (size_t)height * (size_t)width * sizeof(float), st);
    if (e != hipSuccess) {
      tn_set_error("tn_thermal_reg: %s", hipGetErrorString(e));
      return TN_ELAUNCH;
    }
  }
  TN_CHECK_LAUNCH("tn_thermal_reg");
  hipLaunchKernelGGL(k_thermal_reg_finish, dim3(1), dim3(LB), 0, st, (const float*)k.part_tv, (const float*)k.part_cc, (int)(L.bx * L.by), stv, scc,
                     out_loss);
  TN_CHECK_LAUNCH("tn_thermal_reg(finish)");
  return TN_OK;
}

extern "C" int64_t tn_depth_loss_workspace_bytes(int32_t height, int32_t width) {
  if (height < 2 || width < 2 || height > kMaxSide || width > kMaxSide) return -1;
  return depth_loss_layout(height, width).total;
}

extern "C" int tn_depth_loss(const float* depth, const float* accumulation, const float* depth_image, int32_t height, int32_t width, float depth_mult,
                             float tv_mult, void* workspace, int64_t workspace_bytes, float* out_loss, float* out_grad, tn_stream_t stream) {
  TN_REQUIRE(depth && accumulation && workspace && out_loss, "tn_depth_loss: null pointer");
  TN_REQUIRE(height >= 2 && width >= 2, "tn_depth_loss: %d x %d image, a 2 x 2 window needs at least 2 x 2", height, width);
  TN_REQUIRE(height <= kMaxSide && width <= kMaxSide, "tn_depth_loss: %d x %d image is larger than %d on a side", height, width, kMaxSide);
  TN_REQUIRE(depth_mult >= 0.0f && tv_mult >= 0.0f, "tn_depth_loss: multipliers %g / %g, a loss multiplier cannot be negative", (double)depth_mult, (double)tv_mult);
  const DepthLossLayout L = depth_loss_layout(height, width);
  TN_REQUIRE(workspace_bytes >= L.total, "tn_depth_loss: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  DepthLossK k;
  k.depth = depth, k.alpha = accumulation;
  k.sensor = depth_mult != 0.0f ? depth_image : nullptr;  // a multiplier of 0 (or no sensor depth) skips the term: exactly 0
  k.H = height, k.W = width, k.tv = tv_mult != 0.0f ? 1 : 0;
  k.grad = out_grad;
  k.part = static_cast<float*>(workspace), k.part_stride = L.part_stride;
  float* scale = reinterpret_cast<float*>(static_cast<char*>(workspace) + L.off_scale);
  k.scale = scale;
  hipStream_t st = tn_s(stream);
  const dim3 grid((unsigned)L.bx, (unsigned)L.by);
  hipLaunchKernelGGL(k_depth_loss<false>, grid, dim3(LB), 0, st, k);
  TN_CHECK_LAUNCH("tn_depth_loss");
  hipLaunchKernelGGL(k_depth_loss_finish, dim3(1), dim3(LB), 0, st, (const float*)k.part, k.part_stride, (int)(L.bx * L.by), (double)depth_mult, (double)tv_mult,
                     out_loss, scale);
  TN_CHECK_LAUNCH("tn_depth_loss(finish)");
  if (out_grad != nullptr) {
    hipLaunchKernelGGL(k_depth_loss<true>, grid, dim3(LB), 0, st, k);
    TN_CHECK_LAUNCH("tn_depth_loss(gradient)");
  }
  return TN_OK;
}
