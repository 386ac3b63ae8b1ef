// A rigid move of a set of thermal Gaussians: the similarity x' = s R x + t applied to every Gaussian, so that the moved model seen from the moved
// camera renders the same frame.  This is what a dataset-frame (world-frame) splat export and import need; splat_transform.py is the host side.
//
// tn_transform_splat  means' = A x + t (A = s R) | log scales' = scales + log s | quats' = q_R (x) q (Hamilton product, the stored norm is kept) |
//                     the degree 1-3 SH coefficients of both spectra, band by band: rest'[k] = sum_j M_l[k][j] rest[j] per channel, with the real-SH
//                     rotation matrices M_1 [3,3], M_2 [5,5], M_3 [7,7] of R (the host derives them: splat_transform.sh_rotation_matrices)
//
// ONE launch, no atomics, no workspace, no host synchronisation.  Every output value is evaluated in double from the float inputs widened, in the
// fixed order of include/thermal_nerf_hip.h, and rounded once (the build has -ffp-contract=off): the same inputs give the same bytes, and
// tests/splat_transform_functional.py restates it bit for bit.
//
// k_splat_transform<R>: a block of TT threads owns TG consecutive Gaussians (R = rest coefficients per channel: 0, 3, 8 or 15).
//   in     the block walks the slab of each of the five attributes flat into LDS: consecutive lanes read consecutive floats (16 bytes a lane where
//          every pointer is 16-byte aligned -- a tile starts a multiple of 512 bytes into its tensor -- one float a lane otherwise)
//   move   a thread per (Gaussian, channel) for the coefficients -- three colour channels and the thermal one -- and a thread per Gaussian for each
//          of means, scales and quaternions; which of the seven a thread does is the same in a whole wave (TG is a multiple of the wave).  A thread
//          reads its 15 coefficients at the row stride 3 R (colour) or R (thermal) words: 45 and 15 are odd, so the 32 lanes of an LDS access hit
//          32 banks (degree 2, strides 24 and 8, takes bank conflicts and is not tuned).  The 83 matrix entries, A, t, log s and q_R come from the
//          kernel-argument struct: they are uniform, the compiler reads them with scalar loads.  Results go back to the same LDS words.
//   out    the block walks the slabs flat again, LDS -> the outputs
// A block has read its whole tile before it stores any of it and no block touches another's Gaussians, so every *_out may be its own input (the
// common case: in place).  Otherwise an output must overlap no other buffer of the call: pointers are equal or disjoint.
//
// A parameter that is not finite leaves its group of its Gaussian not finite (inf * 0 is NaN): the exporter's filter drops what it dropped before.
#include "tn_common.h"

namespace {

constexpr int TT = 256;  // threads per block
#ifndef TN_TRANSFORM_TILE
#define TN_TRANSFORM_TILE 128  // Gaussians per block: 70 floats each at degree 3 = 35 KiB of LDS, four blocks a CU (A/B: profiles/splat_transform.md)
#endif
constexpr int TG = TN_TRANSFORM_TILE;
#ifndef TN_TRANSFORM_UNROLL
#define TN_TRANSFORM_UNROLL 2  // 16-byte copies in flight per thread of a slab walk (A/B: profiles/splat_transform.md)
#endif
static_assert(TG % TN_WAVE == 0 && TG % 4 == 0, "a tile is whole waves of Gaussians, and its slabs start 16-byte aligned");
constexpr int64_t TRANSFORM_MAX_ROWS = (1ll << 31) - 1;

struct TransformK {
  const float *means, *scales, *quats, *rest, *rest_th;
  float *means_out, *scales_out, *quats_out, *rest_out, *rest_th_out;
  int64_t n;
  int vec;  // every pointer is 16-byte aligned
};

// the block's `total` floats from src (global) to dst (LDS) or back, flat
template <typename Dst, typename Src>
__device__ inline void tile_copy(Dst* __restrict__ dst, const Src* __restrict__ src, int total, bool vec) {
  int done = 0;
  if (vec) {
    const int nv = total >> 2;
#pragma unroll TN_TRANSFORM_UNROLL
    for (int j = threadIdx.x; j < nv; j += TT) reinterpret_cast<float4*>(dst)[j] = reinterpret_cast<const float4*>(src)[j];
    done = nv << 2;
  }
#pragma unroll 4
  for (int j = done + threadIdx.x; j < total; j += TT) dst[j] = src[j];
}

// one band of one channel: c[k * stride], k = 0 .. D - 1, becomes sum_j M[k][j] c[j * stride], j ascending, in double, rounded once
template <int D>
__device__ inline void rotate_band(const double* __restrict__ M, float* c, int stride) {
  double v[D];
#pragma unroll
  for (int j = 0; j < D; ++j) v[j] = (double)c[j * stride];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    double acc = M[k * D] * v[0];
#pragma unroll
    for (int j = 1; j < D; ++j) acc = acc + M[k * D + j] * v[j];
    c[k * stride] = (float)acc;
  }
}

template <int R>
__device__ inline void rotate_channel(const TnSplatTransform& T, float* c, int stride) {
  if (R >= 3) rotate_band<3>(T.sh1, c, stride);
  if (R >= 8) rotate_band<5>(T.sh2, c + 3 * stride, stride);
  if (R >= 15) rotate_band<7>(T.sh3, c + 8 * stride, stride);
}

template <int R>
__global__ void __launch_bounds__(TT) k_splat_transform(const TnSplatTransform T, const TransformK a) {
  __shared__ __attribute__((aligned(16))) float s_means[TG * 3];
  __shared__ __attribute__((aligned(16))) float s_scales[TG * 3];
  __shared__ __attribute__((aligned(16))) float s_quats[TG * 4];
  __shared__ __attribute__((aligned(16))) float s_rest[R > 0 ? TG * 3 * R : 4];
  __shared__ __attribute__((aligned(16))) float s_th[R > 0 ? TG * R : 4];
  const int64_t g0 = (int64_t)blockIdx.x * TG;
  const int cnt = (int)(a.n - g0 < TG ? a.n - g0 : TG);
  const bool vec = a.vec != 0;
  tile_copy(s_means, a.means + g0 * 3, cnt * 3, vec);
  tile_copy(s_scales, a.scales + g0 * 3, cnt * 3, vec);
  tile_copy(s_quats, a.quats + g0 * 4, cnt * 4, vec);
  if (R > 0) {
    tile_copy(s_rest, a.rest + g0 * (3 * R), cnt * 3 * R, vec);
    tile_copy(s_th, a.rest_th + g0 * R, cnt * R, vec);
  }
  __syncthreads();
  // kinds 0..2: a colour channel's coefficients, 3: the thermal ones, 4: means, 5: scales, 6: quaternions; uniform in a wave
  for (int item = (R > 0 ? 0 : 4 * TG) + threadIdx.x; item < 7 * TG; item += TT) {
    const int kind = item / TG, g = item % TG;
    if (g >= cnt) continue;
    if (kind < 3) {
      if (R > 0) rotate_channel<R>(T, s_rest + g * (3 * R) + kind, 3);
    } else if (kind == 3) {
      if (R > 0) rotate_channel<R>(T, s_th + g * R, 1);
    } else if (kind == 4) {
      float* p = s_means + 3 * g;
      const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
#pragma unroll
      for (int i = 0; i < 3; ++i) p[i] = (float)(((T.A[3 * i] * x + T.A[3 * i + 1] * y) + T.A[3 * i + 2] * z) + T.t[i]);
    } else if (kind == 5) {
      float* p = s_scales + 3 * g;
#pragma unroll
      for (int i = 0; i < 3; ++i) p[i] = (float)((double)p[i] + T.log_scale);
    } else {
      float* p = s_quats + 4 * g;
      const double w1 = T.q[0], x1 = T.q[1], y1 = T.q[2], z1 = T.q[3];
      const double w2 = (double)p[0], x2 = (double)p[1], y2 = (double)p[2], z2 = (double)p[3];
      p[0] = (float)(((w1 * w2 - x1 * x2) - y1 * y2) - z1 * z2);
      p[1] = (float)(((w1 * x2 + x1 * w2) + y1 * z2) - z1 * y2);
      p[2] = (float)(((w1 * y2 - x1 * z2) + y1 * w2) + z1 * x2);
      p[3] = (float)(((w1 * z2 + x1 * y2) - y1 * x2) + z1 * w2);
    }
  }
  __syncthreads();
  tile_copy(a.means_out + g0 * 3, s_means, cnt * 3, vec);
  tile_copy(a.scales_out + g0 * 3, s_scales, cnt * 3, vec);
  tile_copy(a.quats_out + g0 * 4, s_quats, cnt * 4, vec);
  if (R > 0) {
    tile_copy(a.rest_out + g0 * (3 * R), s_rest, cnt * 3 * R, vec);
    tile_copy(a.rest_th_out + g0 * R, s_th, cnt * R, vec);
  }
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" int tn_transform_splat(const TnSplatTransform* transform, const float* means, const float* log_scales, const float* quats,
                                  const float* features_rest, const float* thermal_rest, int64_t num_gaussians, int32_t num_rest_coeffs,
                                  float* means_out, float* log_scales_out, float* quats_out, float* features_rest_out, float* thermal_rest_out,
                                  tn_stream_t stream) {
  const int64_t n = num_gaussians;
  const int R = num_rest_coeffs;
  TN_REQUIRE(transform, "tn_transform_splat: null pointer (transform)");
  TN_REQUIRE(n >= 0 && n <= TRANSFORM_MAX_ROWS, "tn_transform_splat: %lld Gaussians (0..2^31 - 1)", (long long)n);
  TN_REQUIRE(R == 0 || R == 3 || R == 8 || R == 15, "tn_transform_splat: %d rest coefficients (0, 3, 8 or 15: degrees 0 to 3)", R);
  if (n == 0) return TN_OK;
  TN_REQUIRE(means && log_scales && quats && means_out && log_scales_out && quats_out, "tn_transform_splat: null pointer");
  TN_REQUIRE(R == 0 || (features_rest && thermal_rest && features_rest_out && thermal_rest_out),
             "tn_transform_splat: null pointer (%d rest coefficients)", R);
  TransformK a{means, log_scales, quats, features_rest, thermal_rest, means_out, log_scales_out, quats_out, features_rest_out, thermal_rest_out, n, 0};
  a.vec = aligned16(means) && aligned16(log_scales) && aligned16(quats) && aligned16(means_out) && aligned16(log_scales_out) && aligned16(quats_out) &&
          (R == 0 || (aligned16(features_rest) && aligned16(thermal_rest) && aligned16(features_rest_out) && aligned16(thermal_rest_out)));
  const dim3 grid((unsigned)tn_cdiv(n, TG)), block(TT);
  hipStream_t st = tn_s(stream);
  switch (R) {
    case 0: hipLaunchKernelGGL(k_splat_transform<0>, grid, block, 0, st, *transform, a); break;
    case 3: hipLaunchKernelGGL(k_splat_transform<3>, grid, block, 0, st, *transform, a); break;
    case 8: hipLaunchKernelGGL(k_splat_transform<8>, grid, block, 0, st, *transform, a); break;
    default: hipLaunchKernelGGL(k_splat_transform<15>, grid, block, 0, st, *transform, a); break;
  }
  TN_CHECK_LAUNCH("tn_transform_splat");
  return TN_OK;
}
