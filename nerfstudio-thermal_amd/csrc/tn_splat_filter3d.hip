// Mip-Splatting's 3D smoothing filter ("Mip-Splatting: Alias-free 3D Gaussian Splatting", eq. 6-7 and 9): every Gaussian is band-limited to the
// highest frequency any training camera could have sampled it at.  The screen-space half of the paper (the 2D Mip filter with opacity
// compensation) is rasterize_mode "antialiased"; this file is the world-space half, as a per-Gaussian pre-transform of log-scales and opacity
// logits -- the rasteriser is not touched.  splat_filter.py is the host side, tests/splat_filter3d_functional.py restates all three in float64.
//
// tn_filter3d_splat_compute -- filter_3D [N] from means [N,3] and a table of C cameras [C,18] (viewmat 12, fx fy cx cy, width height):
//   camera n sees Gaussian k iff z > near and -0.15 W <= u <= 1.15 W and -0.15 H <= v <= 1.15 H, with (x, y, z) = viewmat [p; 1],
//   u = fx x / z + cx, v = fy y / z + cy;  nu_k = max over the cameras that see k of max(fx, fy) / z;  filter_k = sqrt(variance) / nu_k.
//   A Gaussian no camera sees takes the smallest nu of the seen ones (the largest filter); when nothing is seen every row is 0 (filter off).
//   The official code's shortcut is NOT reproduced: it takes ONE focal length for the whole set -- the largest of all cameras -- over each
//   Gaussian's smallest depth.  A rig whose thermal camera has a quarter of the RGB camera's focal length in pixels makes that wrong by the
//   same factor for every Gaussian only the thermal camera sees, and for any whose nearest camera is not its sharpest.  Here the maximum is
//   taken per camera, as eq. 6-7 state it.
//   k_filter3d_compute  a thread per Gaussian walks the camera table, which the block stages in LDS FILTER_CHUNK cameras at a time (flat,
//                       coalesced; every lane then reads the same LDS word: a broadcast, no bank conflict); C is not bounded by a chunk.  All
//                       in double from the fp32 inputs widened, rounded once.  Unseen rows leave with the marker -1; the block's smallest nu
//                       (wave shuffles, then across the block's waves in LDS) goes to partial[block].
//   k_filter3d_finish   every block folds the partials in block order (a minimum: exact, the order cannot matter), then the blocks walk the
//                       rows and replace the markers by sqrt(variance) / nu_min, or 0 when nothing was seen.
//   Two launches, no atomics, no host synchronisation, no read-back: the same inputs give the same bits.
//
// tn_filter3d_splat_apply -- one launch, a thread per Gaussian, with f = filter_3D[k], s_i = exp(log s_i), r_i = s_i^2 / (s_i^2 + f^2):
//   log s'_i = 1/2 log(s_i^2 + f^2)
//   o'       = (o + log c) - log1p(e^o (1 - c)),  c = sqrt(r_0 r_1 r_2)     -- the logit of sigmoid(o) c, without cancelling or saturating:
//              log c = -1/2 ((log1p(t_0) + log1p(t_1)) + log1p(t_2)) with t_i = f^2 / s_i^2, and 1 - c = -expm1(log c)
//   and the same for the thermal opacity where the call has one (a NULL pair of thermal pointers is shared mode).  f == 0 copies the row bit for
//   bit (a branch, not log(exp(.))).
// tn_filter3d_splat_apply_backward -- one launch, closed form, with 1 - p = 1 / (1 + e^o), p = 1 / (1 + e^-o), 1 - p' = (1 - p) + p (1 - c),
//   1 - r_i = f^2 / (s_i^2 + f^2):
//   dL/d log s_i = g_s'_i r_i + (g_o' / (1 - p') [+ g_oth' / (1 - p'_th)]) (1 - r_i)        dL/d o = g_o' (1 - p) / (1 - p')
//   f == 0 copies the gradients bit for bit; filter_3D takes no gradient.
// Both evaluate in double and round once (the build has -ffp-contract=off).  Bound: memory -- the forward moves 36 bytes per Gaussian (44
// separate), the backward 52 (64).
#include "tn_common.h"

namespace {

constexpr int FILTER_THREADS = 256;
constexpr int FILTER_CAM_FLOATS = 18;  // viewmat 12 | fx fy cx cy | width height
constexpr int FILTER_CHUNK = 128;      // cameras staged per pass: 9 KiB of LDS
constexpr int FILTER_FINISH_BLOCKS = 256;
constexpr double FILTER_MARGIN = 0.15;  // Mip-Splatting's compute_3D_filter: 15 % beyond each image side still counts as seen

__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}

// the block's minimum, in every thread (sm: one double per wave)
__device__ __forceinline__ double block_min_d(double v, double* sm) {
  v = wave_min_d(v);
  if (tn_lane() == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double m = sm[0];
#pragma unroll
  for (int w = 1; w < FILTER_THREADS / TN_WAVE; ++w) m = fmin(m, sm[w]);
  __syncthreads();
  return m;
}

__global__ void __launch_bounds__(FILTER_THREADS) k_filter3d_compute(const float* __restrict__ means, const float* __restrict__ cams, int64_t N,
                                                                     int32_t C, double near, double sqrt_var, float* __restrict__ out,
                                                                     double* __restrict__ partial) {
  __shared__ float s_cam[FILTER_CHUNK * FILTER_CAM_FLOATS];
  __shared__ double s_min[FILTER_THREADS / TN_WAVE];
  const int64_t i = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  const bool live = i < N;
  double x = 0.0, y = 0.0, z = 0.0;
  if (live) x = (double)means[3 * i], y = (double)means[3 * i + 1], z = (double)means[3 * i + 2];
  double nu = 0.0;  // the largest max(fx, fy) / z over the cameras that see the Gaussian; 0: none has
  for (int32_t c0 = 0; c0 < C; c0 += FILTER_CHUNK) {
    const int cnt = C - c0 < FILTER_CHUNK ? C - c0 : FILTER_CHUNK;
    const float* src = cams + (int64_t)c0 * FILTER_CAM_FLOATS;
    for (int j = threadIdx.x; j < cnt * FILTER_CAM_FLOATS; j += FILTER_THREADS) s_cam[j] = src[j];
    __syncthreads();
    if (live) {
      for (int c = 0; c < cnt; ++c) {
        const float* m = s_cam + c * FILTER_CAM_FLOATS;  // the same address in every lane
        const double zc = (((double)m[8] * x + (double)m[9] * y) + (double)m[10] * z) + (double)m[11];
        if (!(zc > near)) continue;
        const double xc = (((double)m[0] * x + (double)m[1] * y) + (double)m[2] * z) + (double)m[3];
        const double yc = (((double)m[4] * x + (double)m[5] * y) + (double)m[6] * z) + (double)m[7];
        const double fx = (double)m[12], fy = (double)m[13], W = (double)m[16], H = (double)m[17];
        const double u = fx * xc / zc + (double)m[14], v = fy * yc / zc + (double)m[15];
        if (u >= -FILTER_MARGIN * W && u <= (1.0 + FILTER_MARGIN) * W && v >= -FILTER_MARGIN * H && v <= (1.0 + FILTER_MARGIN) * H)
          nu = fmax(nu, fmax(fx, fy) / zc);
      }
    }
    __syncthreads();
  }
  const bool seen = live && nu > 0.0;
  if (live) out[i] = seen ? (float)(sqrt_var / nu) : -1.0f;
  const double m = block_min_d(seen ? nu : (double)INFINITY, s_min);
  if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

__global__ void __launch_bounds__(FILTER_THREADS) k_filter3d_finish(float* __restrict__ out, const double* __restrict__ partial, int64_t num_partials,
                                                                    int64_t N, double sqrt_var) {
  __shared__ double s_min[FILTER_THREADS / TN_WAVE];
  double m = (double)INFINITY;
  for (int64_t b = threadIdx.x; b < num_partials; b += FILTER_THREADS) m = fmin(m, partial[b]);
  m = block_min_d(m, s_min);
  const float unseen = m < (double)INFINITY ? (float)(sqrt_var / m) : 0.0f;  // nothing seen anywhere: the filter is off
  for (int64_t i = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * FILTER_THREADS)
    if (out[i] < 0.0f) out[i] = unseen;
}

struct FilterRow {  // what the forward and the backward share: s_i^2 + f^2, r_i, 1 - r_i, log c and 1 - c
  double d[3], r[3], q[3], log_c, omc;
};

__device__ __forceinline__ FilterRow filter_row(const float* __restrict__ ls, double f) {
  FilterRow w;
  const double f2 = f * f;
  double l[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double s2 = exp(2.0 * (double)ls[a]);
    w.d[a] = s2 + f2;
    w.r[a] = s2 / w.d[a];
    w.q[a] = f2 / w.d[a];
    l[a] = log1p(f2 / s2);  // -log r_i
  }
  // c = sqrt((r_0 r_1) r_2) through its logarithm, so that 1 - c does not cancel where the filter is far below the scales
  w.log_c = -0.5 * ((l[0] + l[1]) + l[2]);
  w.omc = -expm1(w.log_c);
  return w;
}

__device__ __forceinline__ float filter_logit(float o, const FilterRow& w) {
  const double od = (double)o;
  return (float)((od + w.log_c) - log1p(exp(od) * w.omc));
}

// 1 - p and 1 - p' of one chain
__device__ __forceinline__ void filter_complements(float o, double omc, double& one_minus_p, double& one_minus_pp) {
  const double od = (double)o;
  one_minus_p = 1.0 / (1.0 + exp(od));
  const double p = 1.0 / (1.0 + exp(-od));
  one_minus_pp = one_minus_p + p * omc;
}

__global__ void __launch_bounds__(FILTER_THREADS) k_filter3d_apply(const float* __restrict__ log_scales, const float* __restrict__ opacities,
                                                                   const float* __restrict__ opacities_th, const float* __restrict__ filter,
                                                                   int64_t N, float* __restrict__ log_scales_out, float* __restrict__ opacities_out,
                                                                   float* __restrict__ opacities_th_out) {
  const int64_t i = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  if (i >= N) return;
  const float f = filter[i];
  const float ls[3] = {log_scales[3 * i], log_scales[3 * i + 1], log_scales[3 * i + 2]};
  const float o = opacities[i];
  const float oth = opacities_th ? opacities_th[i] : 0.0f;
  if (f == 0.0f) {  // the filter is off for this row: the values themselves
#pragma unroll
    for (int a = 0; a < 3; ++a) log_scales_out[3 * i + a] = ls[a];
    opacities_out[i] = o;
    if (opacities_th) opacities_th_out[i] = oth;
    return;
  }
  const FilterRow w = filter_row(ls, (double)f);
#pragma unroll
  for (int a = 0; a < 3; ++a) log_scales_out[3 * i + a] = (float)(0.5 * log(w.d[a]));
  opacities_out[i] = filter_logit(o, w);
  if (opacities_th) opacities_th_out[i] = filter_logit(oth, w);
}

__global__ void __launch_bounds__(FILTER_THREADS) k_filter3d_apply_backward(const float* __restrict__ log_scales, const float* __restrict__ opacities,
                                                                            const float* __restrict__ opacities_th, const float* __restrict__ filter,
                                                                            const float* __restrict__ g_ls_out, const float* __restrict__ g_o_out,
                                                                            const float* __restrict__ g_oth_out, int64_t N, float* __restrict__ g_ls,
                                                                            float* __restrict__ g_o, float* __restrict__ g_oth) {
  const int64_t i = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  if (i >= N) return;
  const float f = filter[i];
  const float gs[3] = {g_ls_out[3 * i], g_ls_out[3 * i + 1], g_ls_out[3 * i + 2]};
  const float go = g_o_out[i];
  const float goth = opacities_th ? g_oth_out[i] : 0.0f;
  if (f == 0.0f) {
#pragma unroll
    for (int a = 0; a < 3; ++a) g_ls[3 * i + a] = gs[a];
    g_o[i] = go;
    if (opacities_th) g_oth[i] = goth;
    return;
  }
  const float ls[3] = {log_scales[3 * i], log_scales[3 * i + 1], log_scales[3 * i + 2]};
  const FilterRow w = filter_row(ls, (double)f);
  double omp, ompp;
  filter_complements(opacities[i], w.omc, omp, ompp);
  double A = (double)go / ompp;
  g_o[i] = (float)((double)go * omp / ompp);
  if (opacities_th) {
    filter_complements(opacities_th[i], w.omc, omp, ompp);
    A = A + (double)goth / ompp;
    g_oth[i] = (float)((double)goth * omp / ompp);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) g_ls[3 * i + a] = (float)((double)gs[a] * w.r[a] + A * w.q[a]);
}

constexpr int64_t FILTER_MAX_ROWS = (1ll << 31) - 1;

}  // namespace

extern "C" int64_t tn_filter3d_splat_workspace_bytes(int64_t num_gaussians) {
  if (num_gaussians < 0 || num_gaussians > FILTER_MAX_ROWS) return -1;
  const int64_t blocks = tn_cdiv(num_gaussians, FILTER_THREADS);
  return (int64_t)sizeof(double) * (blocks > 1 ? blocks : 1);
}

extern "C" int tn_filter3d_splat_compute(const float* means, int64_t num_gaussians, const float* cameras, int32_t num_cameras, double near_plane,
                                         double variance, float* filter_3d, void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  const int64_t N = num_gaussians;
  TN_REQUIRE(N >= 0 && N <= FILTER_MAX_ROWS, "tn_filter3d_splat_compute: %lld Gaussians (0..2^31 - 1)", (long long)N);
  TN_REQUIRE(num_cameras >= 0, "tn_filter3d_splat_compute: %d cameras", num_cameras);
  TN_REQUIRE(near_plane == near_plane && near_plane >= 0.0 && near_plane <= 1.7976931348623157e308,
             "tn_filter3d_splat_compute: near = %g (>= 0, finite)", near_plane);
  TN_REQUIRE(variance == variance && variance >= 0.0 && variance <= 1.7976931348623157e308,
             "tn_filter3d_splat_compute: variance = %g (>= 0, finite)", variance);
  if (N == 0) return TN_OK;
  TN_REQUIRE(means && filter_3d && workspace && (num_cameras == 0 || cameras), "tn_filter3d_splat_compute: null pointer");
  TN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "tn_filter3d_splat_compute: the workspace must be 8-byte aligned");
  const int64_t need = tn_filter3d_splat_workspace_bytes(N);
  TN_REQUIRE(workspace_bytes >= need, "tn_filter3d_splat_compute: workspace of %lld bytes, %lld needed (tn_filter3d_splat_workspace_bytes)",
             (long long)workspace_bytes, (long long)need);
  const int64_t blocks = tn_cdiv(N, FILTER_THREADS);
  const double sqrt_var = sqrt(variance);
  double* partial = static_cast<double*>(workspace);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_filter3d_compute, dim3((unsigned)blocks), dim3(FILTER_THREADS), 0, st, means, cameras, N, num_cameras, near_plane, sqrt_var,
                     filter_3d, partial);
  TN_CHECK_LAUNCH("tn_filter3d_splat_compute");
  const int64_t fin = blocks < FILTER_FINISH_BLOCKS ? blocks : FILTER_FINISH_BLOCKS;
  hipLaunchKernelGGL(k_filter3d_finish, dim3((unsigned)fin), dim3(FILTER_THREADS), 0, st, filter_3d, (const double*)partial, blocks, N, sqrt_var);
  TN_CHECK_LAUNCH("tn_filter3d_splat_compute");
  return TN_OK;
}

extern "C" int tn_filter3d_splat_apply(const float* log_scales, const float* opacities, const float* opacities_thermal, const float* filter_3d,
                                       int64_t num_gaussians, float* log_scales_out, float* opacities_out, float* opacities_thermal_out,
                                       tn_stream_t stream) {
  const int64_t N = num_gaussians;
  TN_REQUIRE(N >= 0 && N <= FILTER_MAX_ROWS, "tn_filter3d_splat_apply: %lld Gaussians (0..2^31 - 1)", (long long)N);
  if (N == 0) return TN_OK;
  TN_REQUIRE(log_scales && opacities && filter_3d && log_scales_out && opacities_out, "tn_filter3d_splat_apply: null pointer");
  TN_REQUIRE((opacities_thermal == nullptr) == (opacities_thermal_out == nullptr),
             "tn_filter3d_splat_apply: the thermal opacities and their output are both null (shared mode) or both set");
  hipLaunchKernelGGL(k_filter3d_apply, dim3((unsigned)tn_cdiv(N, FILTER_THREADS)), dim3(FILTER_THREADS), 0, tn_s(stream), log_scales, opacities,
                     opacities_thermal, filter_3d, N, log_scales_out, opacities_out, opacities_thermal_out);
  TN_CHECK_LAUNCH("tn_filter3d_splat_apply");
  return TN_OK;
}

extern "C" int tn_filter3d_splat_apply_backward(const float* log_scales, const float* opacities, const float* opacities_thermal,
                                                const float* filter_3d, const float* v_log_scales_out, const float* v_opacities_out,
                                                const float* v_opacities_thermal_out, int64_t num_gaussians, float* v_log_scales,
                                                float* v_opacities, float* v_opacities_thermal, tn_stream_t stream) {
  const int64_t N = num_gaussians;
  TN_REQUIRE(N >= 0 && N <= FILTER_MAX_ROWS, "tn_filter3d_splat_apply_backward: %lld Gaussians (0..2^31 - 1)", (long long)N);
  if (N == 0) return TN_OK;
  TN_REQUIRE(log_scales && opacities && filter_3d && v_log_scales_out && v_opacities_out && v_log_scales && v_opacities,
             "tn_filter3d_splat_apply_backward: null pointer");
  TN_REQUIRE((opacities_thermal == nullptr) == (v_opacities_thermal_out == nullptr) && (opacities_thermal == nullptr) == (v_opacities_thermal == nullptr),
             "tn_filter3d_splat_apply_backward: the thermal opacities, their upstream and their gradient are all null (shared mode) or all set");
  hipLaunchKernelGGL(k_filter3d_apply_backward, dim3((unsigned)tn_cdiv(N, FILTER_THREADS)), dim3(FILTER_THREADS), 0, tn_s(stream), log_scales,
                     opacities, opacities_thermal, filter_3d, v_log_scales_out, v_opacities_out, v_opacities_thermal_out, N, v_log_scales, v_opacities,
                     v_opacities_thermal);
  TN_CHECK_LAUNCH("tn_filter3d_splat_apply_backward");
  return TN_OK;
}
