// N4 training, MCMC strategy ("3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat's MCMCStrategy, splatfacto's strategy = "mcmc"):
// the two device operations of ThermalSplatfactoModelConfig.strategy = "mcmc".  tests/splat_mcmc_functional.py restates both in float64.
//
// tn_splat_mcmc_relocate -- M draws (src_idx[j] -> dst_idx[j]) on tensors of num_rows rows, in place:
//   memset            count[num_rows] = 0 (workspace)
//   k_mcmc_count      count[src_idx[j]] += 1 (integer atomics: the sums do not depend on the order), own[j] = this draw saw 0 -- exactly one
//                     draw per drawn source owns it; which one varies between runs, what is written does not
//   k_mcmc_values     per owned source, from the values before the call: ratio r = min(count + 1, 51), every opacity chain
//                     c' = clamp(1 - (1 - c)^(1/r), min_opacity, 1 - eps) -> logit, and with the dominant chain p (p' unclamped)
//                     denom = sum_{i=1..r} sum_{k<i} binom(i-1, k) (-1)^k p'^(k+1) / sqrt(k+1) = sum_{k<r} binom(r, k+1) (-1)^k p'^(k+1) / sqrt(k+1)
//                     (the inner sums over i are the hockey-stick identity), log-scale + log(p / denom) on all three axes.  All in double from
//                     the fp32 inputs, rounded once; binom(r, k+1) by the exact integer recurrence in double (<= binom(51, 25) < 2^53).  The
//                     values go to the workspace, so nothing is overwritten while it may still be read.
//   k_mcmc_write      one thread per (tensor, draw, column): the destination row becomes the source row with the new opacity and scale; the
//                     owner also writes the new opacity and scale into the source row and zeroes both moments of the source row.  Opacity and
//                     scale are only ever read from the workspace here, every other tensor's source rows are never written: no thread reads
//                     what another writes, as long as no destination is a source and no destination repeats (the caller's rule).
// Cost: a refinement step only (every refine_every steps); it moves (2 reads or 1 read + 1 write) x 4 bytes x the row width (31 + 64 (K / 15)
// floats, + 1 separate) per draw plus 4 num_rows bytes of counters -- at 1 M Gaussians and 50 k draws about 40 MB, tens of microseconds of HBM time.
//
// tn_splat_mcmc_noise -- means += Sigma (z g scaler) in place, Sigma = R(q / |q|) diag(exp(log-scale)^2) R^T, g = 1 / (1 + exp(-100 ((1 - o_vis)
// - 0.995))), o_vis = sigmoid(opacity) (separate: the larger of the two sigmoids), z = randn [N,3], scaler = noise_lr x the means' learning rate:
//   k_mcmc_noise      one thread per Gaussian, fp32, no [N,3,3] temporary: Sigma v = R (s^2 * (R^T v)).
// Bound: memory.  Per Gaussian it reads means 12 + log-scales 12 + quats 16 + opacity 4 + randn 12 and writes means 12 = 68 bytes (72 separate)
// against about 90 flops and three transcendental calls, so at 1 M Gaussians 68 MB: about 17 us at 4 TB/s of achieved HBM bandwidth, and it
// runs every training step.  The plain-torch expression is about ten launches with [N,3,3] temporaries (several hundred bytes per Gaussian).
#include <algorithm>
#include <cfloat>

#include "tn_common.h"

namespace {

constexpr int MCMC_N_MAX = 51;  // the ratio's cap (gsplat's n_max)
constexpr int MCMC_VALS = 5;    // per source row: opacity logit, thermal opacity logit, three log-scales
constexpr int MCMC_WRITE_ELEMS = 1024;

struct McmcWs {
  int32_t* count;  // [num_rows]
  float* vals;     // [num_rows, MCMC_VALS]
  int32_t* own;    // [M]
};

static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

static McmcWs mcmc_layout(void* base, int64_t rows, int64_t M, size_t* total) {
  McmcWs w;
  char* p = (char*)base;
  size_t off = 0;
  const size_t n = (size_t)std::max<int64_t>(rows, 1), m = (size_t)std::max<int64_t>(M, 1);
  w.count = (int32_t*)(p + off), off += al256(sizeof(int32_t) * n);
  w.vals = (float*)(p + off), off += al256(sizeof(float) * MCMC_VALS * n);
  w.own = (int32_t*)(p + off), off += al256(sizeof(int32_t) * m);
  if (total) *total = off;
  return w;
}

__global__ void k_mcmc_count(const int64_t* __restrict__ src_idx, int64_t M, int64_t rows, int32_t* __restrict__ count, int32_t* __restrict__ own) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M) return;
  const int64_t s = src_idx[j];
  own[j] = (uint64_t)s < (uint64_t)rows ? (atomicAdd(&count[s], 1) == 0 ? 1 : 0) : 0;  // an index outside the tensors is skipped everywhere
}

__device__ static inline double mcmc_sigmoid(float x) { return 1.0 / (1.0 + exp(-(double)x)); }

__device__ static inline float mcmc_new_logit(double c, double inv_r, double lo) {
  double n = 1.0 - pow(1.0 - c, inv_r);
  n = fmin(fmax(n, lo), 1.0 - (double)FLT_EPSILON);
  return (float)log(n / (1.0 - n));
}

template <bool SEP>
__global__ void k_mcmc_values(const int64_t* __restrict__ src_idx, const int32_t* __restrict__ own, int64_t M, const int32_t* __restrict__ count,
                              const float* __restrict__ log_scales, const float* __restrict__ opacities, const float* __restrict__ opacities_th,
                              double min_opacity, float* __restrict__ vals) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M || !own[j]) return;
  const int64_t s = src_idx[j];
  const int r = min(count[s] + 1, MCMC_N_MAX);
  const double inv_r = 1.0 / (double)r;
  const double o = mcmc_sigmoid(opacities[s]);
  double p = o;
  float* v = vals + s * MCMC_VALS;
  v[0] = mcmc_new_logit(o, inv_r, min_opacity);
  if (SEP) {
    const double o_th = mcmc_sigmoid(opacities_th[s]);
    v[1] = mcmc_new_logit(o_th, inv_r, min_opacity);
    if (o_th > o) p = o_th;  // the dominant chain sets the scale; a tie goes to the RGB opacity
  }
  const double pn = 1.0 - pow(1.0 - p, inv_r);  // unclamped
  double denom = 0.0, binom = (double)r, pw = pn, sign = 1.0;  // binom(r, k + 1), p'^(k + 1), (-1)^k at k = 0
  for (int k = 0; k < r; ++k) {
    denom += sign * binom * pw / sqrt((double)(k + 1));
    binom = binom * (double)(r - k - 1) / (double)(k + 2);  // exact: both sides are integers below 2^53
    pw *= pn;
    sign = -sign;
  }
  const double gain = p / denom;  // s' = (p / denom) s
#pragma unroll
  for (int c = 0; c < 3; ++c) v[2 + c] = (float)log(gain * exp((double)log_scales[3 * s + c]));
}

template <int NT>
struct McmcTensors {  // the parameter tensors (splat.py _PARAM_NAMES order) and their Adam moments; moments may be absent (null)
  float* p[NT];
  float* m1[NT];
  float* m2[NT];
  int32_t width[NT];
  int64_t block_begin[NT + 1];  // first block of each tensor
};

template <int NT>
__global__ void __launch_bounds__(256) k_mcmc_write(McmcTensors<NT> t, const int64_t* __restrict__ src_idx, const int64_t* __restrict__ dst_idx,
                                                    const int32_t* __restrict__ own, int64_t M, int64_t rows, const float* __restrict__ vals) {
  int k = 0;
#pragma unroll
  for (int j = 1; j < NT; ++j) k += (int64_t)blockIdx.x >= t.block_begin[j] ? 1 : 0;  // block-uniform
  const int w = t.width[k];
  float* __restrict__ p = t.p[k];
  float* __restrict__ m1 = t.m1[k];
  float* __restrict__ m2 = t.m2[k];
  const int64_t count = M * w;
  const int64_t base = ((int64_t)blockIdx.x - t.block_begin[k]) * MCMC_WRITE_ELEMS;
#pragma unroll
  for (int u = 0; u < MCMC_WRITE_ELEMS / 256; ++u) {
    const int64_t e = base + u * 256 + threadIdx.x;
    if (e >= count) break;
    const int64_t j = e / w;
    const int c = (int)(e - j * w);
    const int64_t s = src_idx[j], d = dst_idx[j];
    if ((uint64_t)s >= (uint64_t)rows || (uint64_t)d >= (uint64_t)rows) continue;
    const bool fresh = k == 1 || k == 3 || k == 8;  // log-scales, opacities, thermal opacities: the relocation value
    const float v = k == 1 ? vals[s * MCMC_VALS + 2 + c] : k == 3 ? vals[s * MCMC_VALS] : k == 8 ? vals[s * MCMC_VALS + 1] : p[s * w + c];
    p[d * w + c] = v;
    if (own[j]) {
      if (fresh) p[s * w + c] = v;
      if (m1) {
        m1[s * w + c] = 0.f;
        m2[s * w + c] = 0.f;
      }
    }
  }
}

template <bool SEP>
__global__ void __launch_bounds__(256) k_mcmc_noise(float* __restrict__ means, const float* __restrict__ log_scales, const float* __restrict__ quats,
                                                    const float* __restrict__ opacities, const float* __restrict__ opacities_th,
                                                    const float* __restrict__ randn, int64_t N, float scaler) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float o = 1.0f / (1.0f + expf(-opacities[i]));
  if (SEP) o = fmaxf(o, 1.0f / (1.0f + expf(-opacities_th[i])));  // visible in either spectrum
  const float g = 1.0f / (1.0f + expf(-100.0f * ((1.0f - o) - 0.995f)));
  const float gs = g * scaler;
  const float v0 = randn[3 * i] * gs, v1 = randn[3 * i + 1] * gs, v2 = randn[3 * i + 2] * gs;
  const float4 q4 = *(const float4*)(quats + 4 * i);  // rows of 16 bytes in a 256-byte-aligned allocation
  float qw = q4.x, qx = q4.y, qy = q4.z, qz = q4.w;
  const float qn = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
  qw /= qn, qx /= qn, qy /= qn, qz /= qn;
  // R(q), gsplat's quat_to_rotmat (w x y z): the projection's and the split's convention
  const float r00 = 1.f - 2.f * (qy * qy + qz * qz), r01 = 2.f * (qx * qy - qw * qz), r02 = 2.f * (qx * qz + qw * qy);
  const float r10 = 2.f * (qx * qy + qw * qz), r11 = 1.f - 2.f * (qx * qx + qz * qz), r12 = 2.f * (qy * qz - qw * qx);
  const float r20 = 2.f * (qx * qz - qw * qy), r21 = 2.f * (qy * qz + qw * qx), r22 = 1.f - 2.f * (qx * qx + qy * qy);
  const float s0 = expf(log_scales[3 * i]), s1 = expf(log_scales[3 * i + 1]), s2 = expf(log_scales[3 * i + 2]);
  // Sigma v = R (s^2 * (R^T v))
  const float t0 = (s0 * s0) * ((r00 * v0 + r10 * v1) + r20 * v2);
  const float t1 = (s1 * s1) * ((r01 * v0 + r11 * v1) + r21 * v2);
  const float t2 = (s2 * s2) * ((r02 * v0 + r12 * v1) + r22 * v2);
  means[3 * i] += (r00 * t0 + r01 * t1) + r02 * t2;
  means[3 * i + 1] += (r10 * t0 + r11 * t1) + r12 * t2;
  means[3 * i + 2] += (r20 * t0 + r21 * t1) + r22 * t2;
}

template <int NT>
static int mcmc_relocate(const char* who, int64_t num_rows, int32_t num_rest_coeffs, const int64_t* src_idx, const int64_t* dst_idx, int64_t M,
                         float min_opacity, float* const* params, float* const* exp_avg, float* const* exp_avg_sq, void* workspace,
                         int64_t workspace_bytes, tn_stream_t stream) {
  TN_REQUIRE(num_rows >= 0 && num_rows < (1ll << 31), "%s: bad row count", who);
  TN_REQUIRE(M >= 0 && M < (1ll << 31), "%s: bad draw count %lld", who, (long long)M);
  TN_REQUIRE(num_rest_coeffs >= 0 && num_rest_coeffs <= 15, "%s: %d higher-order coefficients", who, num_rest_coeffs);
  TN_REQUIRE(min_opacity > 0.f && min_opacity < 1.f, "%s: min_opacity %g outside (0, 1)", who, (double)min_opacity);
  if (M == 0) return TN_OK;  // nothing drawn: nothing launched
  TN_REQUIRE(num_rows >= 1, "%s: %lld draws on no rows", who, (long long)M);
  TN_REQUIRE(src_idx && dst_idx && params && exp_avg && exp_avg_sq && workspace, "%s: null pointer", who);
  const int64_t need = tn_splat_mcmc_workspace_bytes(num_rows, M);
  TN_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes, (long long)need);
  const int32_t widths[9] = {3, 3, 4, 1, 3, 3 * num_rest_coeffs, 1, num_rest_coeffs, 1};
  McmcTensors<NT> t;
  int64_t blocks = 0;
  for (int j = 0; j < NT; ++j) {
    const bool on = widths[j] > 0;
    TN_REQUIRE(!on || params[j], "%s: null parameter %d", who, j);
    TN_REQUIRE((exp_avg[j] == nullptr) == (exp_avg_sq[j] == nullptr), "%s: moments of parameter %d are partly null", who, j);
    t.p[j] = params[j], t.m1[j] = on ? exp_avg[j] : nullptr, t.m2[j] = on ? exp_avg_sq[j] : nullptr;
    t.width[j] = std::max(widths[j], 1);
    t.block_begin[j] = blocks;
    blocks += on ? tn_cdiv(M * widths[j], MCMC_WRITE_ELEMS) : 0;
  }
  t.block_begin[NT] = blocks;
  TN_REQUIRE(blocks < (1ll << 31), "%s: %lld draws are too many", who, (long long)M);
  McmcWs ws = mcmc_layout(workspace, num_rows, M, nullptr);
  hipStream_t st = tn_s(stream);
  if (hipMemsetAsync(ws.count, 0, sizeof(int32_t) * (size_t)num_rows, st) != hipSuccess) {
    tn_set_error("%s: clearing the counters failed", who);
    return TN_ELAUNCH;
  }
  const dim3 gm((unsigned)tn_cdiv(M, 256));
  hipLaunchKernelGGL(k_mcmc_count, gm, dim3(256), 0, st, src_idx, M, num_rows, ws.count, ws.own);
  TN_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(k_mcmc_values<NT == 9>, gm, dim3(256), 0, st, src_idx, (const int32_t*)ws.own, M, (const int32_t*)ws.count, (const float*)params[1],
                     (const float*)params[3], NT == 9 ? (const float*)params[NT - 1] : nullptr, (double)min_opacity, ws.vals);
  TN_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(k_mcmc_write<NT>, dim3((unsigned)blocks), dim3(256), 0, st, t, src_idx, dst_idx, (const int32_t*)ws.own, M, num_rows,
                     (const float*)ws.vals);
  TN_CHECK_LAUNCH(who);
  return TN_OK;
}

static int mcmc_noise(const char* who, bool sep, float* means, const float* log_scales, const float* quats, const float* opacities,
                      const float* opacities_th, const float* randn, int64_t N, float scaler, tn_stream_t stream) {
  TN_REQUIRE(N >= 0 && N < (1ll << 31), "%s: bad Gaussian count", who);
  TN_REQUIRE(scaler == scaler && scaler >= 0.f && scaler <= FLT_MAX, "%s: scaler %g must be finite and >= 0", who, (double)scaler);
  if (N == 0) return TN_OK;
  TN_REQUIRE(means && log_scales && quats && opacities && randn && (!sep || opacities_th), "%s: null pointer", who);
  TN_REQUIRE(((uintptr_t)quats & 15) == 0, "%s: quats must be 16-byte aligned", who);
  const dim3 grid((unsigned)tn_cdiv(N, 256));
  if (sep)
    hipLaunchKernelGGL(k_mcmc_noise<true>, grid, dim3(256), 0, tn_s(stream), means, log_scales, quats, opacities, opacities_th, randn, N, scaler);
  else
    hipLaunchKernelGGL(k_mcmc_noise<false>, grid, dim3(256), 0, tn_s(stream), means, log_scales, quats, opacities, opacities_th, randn, N, scaler);
  TN_CHECK_LAUNCH(who);
  return TN_OK;
}

}  // namespace

extern "C" int64_t tn_splat_mcmc_workspace_bytes(int64_t num_rows, int64_t num_draws) {
  if (num_rows < 0 || num_rows >= (1ll << 31) || num_draws < 0 || num_draws >= (1ll << 31)) return -1;
  size_t total = 0;
  (void)mcmc_layout(nullptr, num_rows, num_draws, &total);
  return (int64_t)total;
}

// num_tensors says how many entries each of the three HOST arrays holds: 8, or 9 with the separate thermal opacity
extern "C" int tn_splat_mcmc_relocate(int64_t num_rows, int32_t num_rest_coeffs, const int64_t* src_idx, const int64_t* dst_idx, int64_t num_draws,
                                      float min_opacity, int32_t num_tensors, float* const* params, float* const* exp_avg, float* const* exp_avg_sq,
                                      void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  TN_REQUIRE(num_tensors == 8 || num_tensors == 9, "tn_splat_mcmc_relocate: %d tensors per array (8, or 9 with the thermal opacity)", num_tensors);
  return (num_tensors == 8 ? mcmc_relocate<8> : mcmc_relocate<9>)("tn_splat_mcmc_relocate", num_rows, num_rest_coeffs, src_idx, dst_idx, num_draws, min_opacity, params,
                                                                  exp_avg, exp_avg_sq, workspace, workspace_bytes, stream);
}

// opacities_thermal is optional: with it a Gaussian visible in either spectrum stays where it is (k_mcmc_noise<true>)
extern "C" int tn_splat_mcmc_noise(float* means, const float* log_scales, const float* quats, const float* opacities, const float* opacities_thermal,
                                   const float* randn, int64_t num_gaussians, float scaler, tn_stream_t stream) {
  return mcmc_noise("tn_splat_mcmc_noise", opacities_thermal != nullptr, means, log_scales, quats, opacities, opacities_thermal, randn, num_gaussians, scaler, stream);
}
