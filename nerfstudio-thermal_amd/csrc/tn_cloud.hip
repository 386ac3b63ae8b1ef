// Point-cloud export of the NeRF (the HIP form of ns-export pointcloud: nerfstudio/exporter/exporter_utils.py:83-260, generate_point_cloud).
//
// tn_cloud_append           one batch of rendered rays -> the kept rays' points, colours and thermal values appended to the cloud, in ray order
// tn_cloud_remove_outliers  Open3D's remove_statistical_outlier: neighbour means over the Morton tree of tn_knn (tn_splat_init.hip), their mean and
//                           standard deviation in double, the kept points compacted in their original order
// tn_cloud_append_view / tn_cloud_remove_outliers_view   the same two with the kept rays' directions carried beside the points (one optional pointer
//                           pair through the same write kernels: the plain entry points pass null and write what they always wrote)
// tn_cloud_estimate_normals a normal per point from the covariance of its knn nearest points (tn_knn_normals, tn_splat_init.hip: the wide search
//                           again), flipped against the point's view direction
//
// Both are stable compactions and share one scheme of three launches, none of which lets an atomic decide an order:
//   k_cloud_count<Keep>  one block per CB consecutive rows: the number of kept rows of the block
//   k_cloud_offsets      ONE block: the exclusive scan of the block counts, started at the rows the output already holds (the device counter),
//                        and the counter's new value min(cap, old + kept)
//   k_cloud_write<Keep>  the block evaluates the same predicate again (the same instructions on the same inputs: the same answer), ranks its kept
//                        rows by wave ballots, and writes row r to offset[block] + rank -- unless that lies at or beyond cap
// No float atomics; the double sums of the statistics are folded in a fixed order (per thread a grid-stride walk, per block a tree over LDS, then one
// block over the partials), so every output is bit-reproducible.  No host synchronisation.
#include <algorithm>

#include "tn_common.h"

namespace {

constexpr int CB = 256;             // threads (= rows) per block of the count / write launches
constexpr int STAT_BLOCKS = 256;    // partial sums of a statistics pass
constexpr int64_t CLOUD_MAX_ROWS = (1ll << 31) - 1;

constexpr int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }

// ray r of a rendered batch is kept iff it is opaque, its point is finite, and the point is strictly inside the box (when there is one)
struct RayKeep {
  const float *origins, *directions, *depth, *accumulation;
  float alpha_thresh;
  bool has_box;
  SplatCropK box;
  __device__ inline bool point(int64_t r, float& x, float& y, float& z) const {
    const float t = depth[r];
    x = __fadd_rn(origins[3 * r], __fmul_rn(directions[3 * r], t));
    y = __fadd_rn(origins[3 * r + 1], __fmul_rn(directions[3 * r + 1], t));
    z = __fadd_rn(origins[3 * r + 2], __fmul_rn(directions[3 * r + 2], t));
    if (!(accumulation[r] > alpha_thresh)) return false;
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    return !has_box || splat_in_crop(box, x, y, z);
  }
  __device__ inline bool operator()(int64_t r) const {
    float x, y, z;
    return point(r, x, y, z);
  }
};

// point i of a cloud is kept iff its neighbour mean is positive and below the threshold (stats[2]; a NaN threshold keeps nothing)
struct MeanKeep {
  const double* mean;
  const double* stats;
  __device__ inline bool operator()(int64_t i) const {
    const double m = mean[i];
    return m > 0.0 && m < stats[2];
  }
};

template <class Keep>
__global__ void __launch_bounds__(CB) k_cloud_count(Keep keep, int64_t n, int32_t* __restrict__ block_count) {
  __shared__ int wave_count[CB / TN_WAVE];
  const int64_t r = (int64_t)blockIdx.x * CB + threadIdx.x;
  const bool k = r < n && keep(r);
  const int c = __popcll(__ballot(k));
  if (tn_lane() == 0) wave_count[threadIdx.x / TN_WAVE] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < CB / TN_WAVE; ++w) s += wave_count[w];
    block_count[blockIdx.x] = s;
  }
}

// offset[b] = base + the kept rows of the blocks before b, with base = the rows already in the output (clamped to 0..cap); then the counter
__global__ void __launch_bounds__(CB) k_cloud_offsets(const int32_t* __restrict__ block_count, int64_t num_blocks, int64_t cap, int64_t* __restrict__ offset,
                                                      int64_t* __restrict__ count, bool count_is_total) {
  __shared__ int64_t sh[CB];
  __shared__ int64_t carry;
  if (threadIdx.x == 0) {
    const int64_t c = count_is_total ? 0 : *count;
    carry = c < 0 ? 0 : (c > cap ? cap : c);
  }
  __syncthreads();
  for (int64_t b0 = 0; b0 < num_blocks; b0 += CB) {
    const int64_t b = b0 + threadIdx.x;
    const int64_t v = b < num_blocks ? block_count[b] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < CB; o <<= 1) {  // inclusive scan of the chunk (integers: any order gives the same sums)
      const int64_t t = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    if (b < num_blocks) offset[b] = carry + sh[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 0) carry += sh[CB - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = carry < cap ? carry : cap;
}

// rank of the thread's row among the block's kept rows (every thread of the block calls it)
__device__ inline int block_rank(bool k) {
  __shared__ int wave_count[CB / TN_WAVE];
  const unsigned long long votes = __ballot(k);
  const int lane = tn_lane(), wave = threadIdx.x / TN_WAVE;
  if (lane == 0) wave_count[wave] = __popcll(votes);
  __syncthreads();
  int before = __popcll(votes & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) before += wave_count[w];
  return before;
}

__global__ void __launch_bounds__(CB) k_cloud_append_write(RayKeep keep, int64_t n, const float* __restrict__ rgb, int64_t rgb_stride,
                                                           const float* __restrict__ thermal, int64_t thermal_stride, const int64_t* __restrict__ offset,
                                                           int64_t cap, float* __restrict__ out_xyz, float* __restrict__ out_rgb,
                                                           float* __restrict__ out_thermal, float* __restrict__ out_view) {
  const int64_t r = (int64_t)blockIdx.x * CB + threadIdx.x;
  float x = 0.0f, y = 0.0f, z = 0.0f;
  const bool k = r < n && keep.point(r, x, y, z);
  const int64_t at = offset[blockIdx.x] + block_rank(k);
  if (!k || at >= cap) return;
  out_xyz[3 * at] = x, out_xyz[3 * at + 1] = y, out_xyz[3 * at + 2] = z;
  const float* c = rgb + r * rgb_stride;
  out_rgb[3 * at] = c[0], out_rgb[3 * at + 1] = c[1], out_rgb[3 * at + 2] = c[2];
  out_thermal[at] = thermal[r * thermal_stride];
  if (out_view) {  // the ray's direction as given, beside its point
#pragma unroll
    for (int a = 0; a < 3; ++a) out_view[3 * at + a] = keep.directions[3 * r + a];
  }
}

__global__ void __launch_bounds__(CB) k_cloud_filter_write(MeanKeep keep, int64_t n, const float* __restrict__ xyz, const float* __restrict__ rgb,
                                                           const float* __restrict__ thermal, const int64_t* __restrict__ offset,
                                                           float* __restrict__ out_xyz, float* __restrict__ out_rgb, float* __restrict__ out_thermal,
                                                           uint8_t* __restrict__ keep_out, const float* __restrict__ view, float* __restrict__ out_view) {
  const int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x;
  const bool k = i < n && keep(i);
  const int64_t at = offset[blockIdx.x] + block_rank(k);  // < n: at most i rows are kept before row i
  if (i < n && keep_out) keep_out[i] = k ? 1 : 0;
  if (!k) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) out_xyz[3 * at + a] = xyz[3 * i + a], out_rgb[3 * at + a] = rgb[3 * i + a];
  out_thermal[at] = thermal[i];
  if (out_view) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out_view[3 * at + a] = view[3 * i + a];
  }
}

// ---- statistics: sums over the points with a positive mean, in double and in a fixed order
__device__ inline void block_sum2(double& a, double& b) {
  __shared__ double sa[CB], sb[CB];
  sa[threadIdx.x] = a, sb[threadIdx.x] = b;
  __syncthreads();
  for (int w = CB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sa[threadIdx.x] += sa[threadIdx.x + w], sb[threadIdx.x] += sb[threadIdx.x + w];
    __syncthreads();
  }
  a = sa[0], b = sb[0];
  __syncthreads();
}

// pass 0: partial (sum of the positive means, their number); pass 1: partial (sum of (mean - m)^2 over them, unused) with m = stats[0]
template <int PASS>
__global__ void __launch_bounds__(CB) k_cloud_stat_partial(const double* __restrict__ mean, int64_t n, const double* __restrict__ stats,
                                                           double* __restrict__ partial) {
  const double m = PASS == 1 ? stats[0] : 0.0;
  double a = 0.0, b = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CB) {
    const double v = mean[i];
    if (v > 0.0) {
      if (PASS == 0) a += v, b += 1.0;
      else a += (v - m) * (v - m);
    }
  }
  block_sum2(a, b);
  if (threadIdx.x == 0) partial[2 * blockIdx.x] = a, partial[2 * blockIdx.x + 1] = b;
}

// pass 0: stats[0] = m = sum / V, V kept in stats[1] for the next pass; pass 1: stats = [m, s, thr]
template <int PASS>
__global__ void __launch_bounds__(CB) k_cloud_stat_final(const double* __restrict__ partial, int num_partial, double std_ratio, double* __restrict__ stats) {
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < num_partial; i += CB) a += partial[2 * i], b += partial[2 * i + 1];
  block_sum2(a, b);
  if (threadIdx.x != 0) return;
  if (PASS == 0) {
    stats[0] = a / b;  // no positive mean: 0 / 0, and the NaN keeps nothing
    stats[1] = b;
  } else {
    const double m = stats[0], V = stats[1];
    const double s = sqrt(a / (V - 1.0));  // one positive mean: 0 / 0 as well
    stats[1] = s;
    stats[2] = m + std_ratio * s;
  }
}

struct FilterLayout {
  int64_t tree, mean, partial, counts, offsets, total;
};

FilterLayout filter_layout(int64_t n, int64_t tree_bytes) {
  const int64_t nb = tn_cdiv(n, CB);
  FilterLayout L;
  L.tree = 0;
  L.mean = align256(tree_bytes);
  L.partial = L.mean + align256(n * 8);
  L.counts = L.partial + align256(2 * STAT_BLOCKS * 8);
  L.offsets = L.counts + align256(nb * 4);
  L.total = L.offsets + align256(nb * 8);
  return L;
}

}  // namespace

extern "C" int64_t tn_cloud_append_workspace_bytes(int64_t num_rays) {
  if (num_rays < 0 || num_rays > CLOUD_MAX_ROWS) return -1;
  const int64_t nb = tn_cdiv(num_rays, CB);
  return align256(nb * 4) + align256(nb * 8);
}

namespace {

// tn_cloud_append (with_view false, out_view null) and tn_cloud_append_view
int cloud_append(const float* origins, const float* directions, const float* depth, const float* accumulation, const float* rgb, int64_t rgb_stride,
                 const float* thermal, int64_t thermal_stride, int64_t num_rays, float alpha_thresh, const TnSplatCrop* box, float* out_xyz, float* out_rgb,
                 float* out_thermal, bool with_view, float* out_view, int64_t cap, int64_t* count, void* workspace, int64_t workspace_bytes,
                 tn_stream_t stream) {
  TN_REQUIRE(num_rays >= 0 && num_rays <= CLOUD_MAX_ROWS, "tn_cloud_append: %lld rays (0..2^31 - 1)", (long long)num_rays);
  TN_REQUIRE(cap >= 0, "tn_cloud_append: a capacity of %lld rows", (long long)cap);
  if (num_rays == 0) return TN_OK;
  TN_REQUIRE(origins && directions && depth && accumulation && rgb && thermal && count && workspace, "tn_cloud_append: null pointer");
  TN_REQUIRE(cap == 0 || (out_xyz && out_rgb && out_thermal && (out_view || !with_view)), "tn_cloud_append: null pointer (an output of %lld rows)",
             (long long)cap);
  TN_REQUIRE(rgb_stride >= 3 && thermal_stride >= 1, "tn_cloud_append: strides of %lld (rgb, >= 3) and %lld (thermal, >= 1) elements per ray",
             (long long)rgb_stride, (long long)thermal_stride);
  const int64_t need = tn_cloud_append_workspace_bytes(num_rays);
  TN_REQUIRE(workspace_bytes >= need, "tn_cloud_append: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  const int64_t nb = tn_cdiv(num_rays, CB);
  int32_t* counts = static_cast<int32_t*>(workspace);
  int64_t* offsets = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + align256(nb * 4));
  RayKeep keep{origins, directions, depth, accumulation, alpha_thresh, box != nullptr, SplatCropK{}};
  if (box) keep.box = make_cropk(box);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_cloud_count<RayKeep>, dim3((unsigned)nb), dim3(CB), 0, st, keep, num_rays, counts);
  TN_CHECK_LAUNCH("tn_cloud_append(count)");
  hipLaunchKernelGGL(k_cloud_offsets, dim3(1), dim3(CB), 0, st, counts, nb, cap, offsets, count, false);
  TN_CHECK_LAUNCH("tn_cloud_append(offsets)");
  hipLaunchKernelGGL(k_cloud_append_write, dim3((unsigned)nb), dim3(CB), 0, st, keep, num_rays, rgb, rgb_stride, thermal, thermal_stride, offsets, cap,
                     out_xyz, out_rgb, out_thermal, with_view ? out_view : nullptr);
  TN_CHECK_LAUNCH("tn_cloud_append(write)");
  return TN_OK;
}

}  // namespace

extern "C" int tn_cloud_append(const float* origins, const float* directions, const float* depth, const float* accumulation, const float* rgb,
                               int64_t rgb_stride, const float* thermal, int64_t thermal_stride, int64_t num_rays, float alpha_thresh,
                               const TnSplatCrop* box, float* out_xyz, float* out_rgb, float* out_thermal, int64_t cap, int64_t* count, void* workspace,
                               int64_t workspace_bytes, tn_stream_t stream) {
  return cloud_append(origins, directions, depth, accumulation, rgb, rgb_stride, thermal, thermal_stride, num_rays, alpha_thresh, box, out_xyz, out_rgb,
                      out_thermal, false, nullptr, cap, count, workspace, workspace_bytes, stream);
}

extern "C" int tn_cloud_append_view(const float* origins, const float* directions, const float* depth, const float* accumulation, const float* rgb,
                                    int64_t rgb_stride, const float* thermal, int64_t thermal_stride, int64_t num_rays, float alpha_thresh,
                                    const TnSplatCrop* box, float* out_xyz, float* out_rgb, float* out_thermal, float* out_view, int64_t cap,
                                    int64_t* count, void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  return cloud_append(origins, directions, depth, accumulation, rgb, rgb_stride, thermal, thermal_stride, num_rays, alpha_thresh, box, out_xyz, out_rgb,
                      out_thermal, true, out_view, cap, count, workspace, workspace_bytes, stream);
}

extern "C" int64_t tn_cloud_remove_outliers_workspace_bytes(int64_t n, int32_t nb_neighbors) {
  if (nb_neighbors < 2 || nb_neighbors > 32 || n < nb_neighbors || n > CLOUD_MAX_ROWS) return -1;
  const int64_t tree = tn_knn_tree_workspace_bytes(n);
  return tree < 0 ? -1 : filter_layout(n, tree).total;
}

namespace {

// tn_cloud_remove_outliers (with_view false, view and out_view null) and tn_cloud_remove_outliers_view
int cloud_remove_outliers(const float* xyz, const float* rgb, const float* thermal, bool with_view, const float* view, int64_t n, int32_t nb_neighbors,
                          double std_ratio, float* out_xyz, float* out_rgb, float* out_thermal, float* out_view, int64_t* out_count, double* stats,
                          double* mean, uint8_t* keep, void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  TN_REQUIRE(nb_neighbors >= 2 && nb_neighbors <= 32, "tn_cloud_remove_outliers: nb_neighbors = %d (2..32)", nb_neighbors);
  TN_REQUIRE(n >= 0 && n <= CLOUD_MAX_ROWS, "tn_cloud_remove_outliers: %lld points (below 2^31)", (long long)n);
  TN_REQUIRE(n >= nb_neighbors, "tn_cloud_remove_outliers: %lld points, nb_neighbors = %d needs at least as many", (long long)n, nb_neighbors);
  TN_REQUIRE(xyz && rgb && thermal && out_xyz && out_rgb && out_thermal && out_count && stats && workspace && (!with_view || (view && out_view)),
             "tn_cloud_remove_outliers: null pointer");
  const int64_t tree = tn_knn_tree_workspace_bytes(n);
  if (tree < 0) {
    tn_set_error("tn_cloud_remove_outliers: rocprim could not size its scratch for %lld points", (long long)n);
    return TN_ELAUNCH;
  }
  const FilterLayout L = filter_layout(n, tree);
  TN_REQUIRE(workspace_bytes >= L.total, "tn_cloud_remove_outliers: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  char* ws = static_cast<char*>(workspace);
  double* means = mean ? mean : reinterpret_cast<double*>(ws + L.mean);
  double* partial = reinterpret_cast<double*>(ws + L.partial);
  int32_t* counts = reinterpret_cast<int32_t*>(ws + L.counts);
  int64_t* offsets = reinterpret_cast<int64_t*>(ws + L.offsets);
  hipStream_t st = tn_s(stream);
  if (const int rc = tn_knn_neighbor_means(xyz, n, nb_neighbors, means, ws + L.tree, tree, st)) return rc;
  const int nsb = (int)std::min<int64_t>(tn_cdiv(n, CB * 8), STAT_BLOCKS);
  hipLaunchKernelGGL(k_cloud_stat_partial<0>, dim3(nsb), dim3(CB), 0, st, means, n, stats, partial);
  TN_CHECK_LAUNCH("tn_cloud_remove_outliers(sum)");
  hipLaunchKernelGGL(k_cloud_stat_final<0>, dim3(1), dim3(CB), 0, st, partial, nsb, std_ratio, stats);
  TN_CHECK_LAUNCH("tn_cloud_remove_outliers(mean)");
  hipLaunchKernelGGL(k_cloud_stat_partial<1>, dim3(nsb), dim3(CB), 0, st, means, n, stats, partial);
  TN_CHECK_LAUNCH("tn_cloud_remove_outliers(squares)");
  hipLaunchKernelGGL(k_cloud_stat_final<1>, dim3(1), dim3(CB), 0, st, partial, nsb, std_ratio, stats);
  TN_CHECK_LAUNCH("tn_cloud_remove_outliers(threshold)");
  const MeanKeep pred{means, stats};
  const int64_t nb = tn_cdiv(n, CB);
  hipLaunchKernelGGL(k_cloud_count<MeanKeep>, dim3((unsigned)nb), dim3(CB), 0, st, pred, n, counts);
  TN_CHECK_LAUNCH("tn_cloud_remove_outliers(count)");
  hipLaunchKernelGGL(k_cloud_offsets, dim3(1), dim3(CB), 0, st, counts, nb, n, offsets, out_count, true);
  TN_CHECK_LAUNCH("tn_cloud_remove_outliers(offsets)");
  hipLaunchKernelGGL(k_cloud_filter_write, dim3((unsigned)nb), dim3(CB), 0, st, pred, n, xyz, rgb, thermal, offsets, out_xyz, out_rgb, out_thermal, keep,
                     with_view ? view : nullptr, with_view ? out_view : nullptr);
  TN_CHECK_LAUNCH("tn_cloud_remove_outliers(write)");
  return TN_OK;
}

}  // namespace

extern "C" int tn_cloud_remove_outliers(const float* xyz, const float* rgb, const float* thermal, int64_t n, int32_t nb_neighbors, double std_ratio,
                                        float* out_xyz, float* out_rgb, float* out_thermal, int64_t* out_count, double* stats, double* mean,
                                        uint8_t* keep, void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  return cloud_remove_outliers(xyz, rgb, thermal, false, nullptr, n, nb_neighbors, std_ratio, out_xyz, out_rgb, out_thermal, nullptr, out_count, stats, mean,
                               keep, workspace, workspace_bytes, stream);
}

extern "C" int tn_cloud_remove_outliers_view(const float* xyz, const float* rgb, const float* thermal, const float* view, int64_t n, int32_t nb_neighbors,
                                             double std_ratio, float* out_xyz, float* out_rgb, float* out_thermal, float* out_view, int64_t* out_count,
                                             double* stats, double* mean, uint8_t* keep, void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  return cloud_remove_outliers(xyz, rgb, thermal, true, view, n, nb_neighbors, std_ratio, out_xyz, out_rgb, out_thermal, out_view, out_count, stats, mean,
                               keep, workspace, workspace_bytes, stream);
}

extern "C" int64_t tn_cloud_normals_workspace_bytes(int64_t n, int32_t knn) {
  if (knn < 3 || knn > 32 || n < 0 || n > CLOUD_MAX_ROWS || (n > 0 && n < knn)) return -1;
  return n == 0 ? 0 : tn_knn_tree_workspace_bytes(n);
}

extern "C" int tn_cloud_estimate_normals(const float* xyz, int64_t n, int32_t knn, const float* view, float* out_normals, void* workspace,
                                         int64_t workspace_bytes, tn_stream_t stream) {
  TN_REQUIRE(knn >= 3 && knn <= 32, "tn_cloud_estimate_normals: knn = %d (3..32, the point itself counted)", knn);
  TN_REQUIRE(n >= 0 && n <= CLOUD_MAX_ROWS, "tn_cloud_estimate_normals: %lld points (below 2^31)", (long long)n);
  if (n == 0) return TN_OK;
  TN_REQUIRE(n >= knn, "tn_cloud_estimate_normals: %lld points, knn = %d needs at least as many", (long long)n, knn);
  TN_REQUIRE(xyz && out_normals && workspace, "tn_cloud_estimate_normals: null pointer");
  const int64_t tree = tn_knn_tree_workspace_bytes(n);
  if (tree < 0) {
    tn_set_error("tn_cloud_estimate_normals: rocprim could not size its scratch for %lld points", (long long)n);
    return TN_ELAUNCH;
  }
  TN_REQUIRE(workspace_bytes >= tree, "tn_cloud_estimate_normals: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)tree);
  return tn_knn_normals(xyz, n, knn, view, out_normals, workspace, workspace_bytes, tn_s(stream));
}
