// Gaussian-splat PLY export (the HIP form of ns-export gaussian-splat: nerfstudio/scripts/exporter.py:480-546, ExportGaussianSplat): the model's
// structure-of-arrays parameters -> the file's array of records, filtered and compacted on the device, nothing read back.
//
// tn_export_splat_pack  the kept Gaussians' rows, in their original order, into out_rows [N, W]; their number into count
//
// A stable compaction in the three launches of tn_cloud.hip (the scheme is restated here, not shared: the two files have no code in common but
// the one-block scan), none of which lets an atomic decide an order:
//   k_export_count    one block per EB consecutive Gaussians.  The block walks each attribute's slab of its Gaussians flat (consecutive lanes read
//                     consecutive floats) and marks the Gaussians with a value that is not finite in LDS; then a thread per Gaussian applies the
//                     opacity threshold and the box, writes the ONE-BYTE KEEP FLAG of its Gaussian to the workspace, and the block its count
//   k_export_offsets  ONE block: the exclusive scan of the block counts, and count = their sum (set, not added to)
//   k_export_write    the block reads its flags back (the predicate is evaluated once: the flag byte was chosen over a second evaluation, which
//                     would read every parameter twice; a byte written by one launch and read by the next is as deterministic as the predicate),
//                     ranks the kept Gaussians by wave ballots and stages their indices in LDS.  Its output is ONE contiguous run of kept * W
//                     floats at offset[block] * W, which the block walks flat, j -> (row j / W, column j % W): every store is coalesced, the
//                     scattered reads stay within one Gaussian's parameters (about 250 bytes at degree 3)
// No atomics, no float arithmetic but colour_mode 1's map (double, rounded once): the same inputs give the same bytes.  No host synchronisation.
//
// The row (W floats; R = num_rest_coeffs, o = 9 + 3 R):
//   0..2 means | 3..5 zeros (nx ny nz) | 6..8 f_dc | 9..o-1 f_rest, channel-major | o opacity | o+1..o+3 log scales | o+4..o+7 quaternion as stored
//   spectrum both: | o+8 f_dc_thermal | o+9..o+8+R f_rest_thermal | o+9+R opacity_thermal (separate mode only)
#include "tn_common.h"

namespace {

constexpr int EB = 256;  // threads (= Gaussians) per block of the count / write launches
constexpr int64_t EXPORT_MAX_ROWS = (1ll << 31) - 1;
#ifndef TN_EXPORT_UNROLL
#define TN_EXPORT_UNROLL 8  // gathers in flight per thread of the write pass (A/B: profiles/splat_export.md)
#endif
constexpr int EU = TN_EXPORT_UNROLL;
constexpr int EXPORT_MAX_REST = 1024;  // rest coefficients per Gaussian (degree 3 has 15): EB * W stays far inside 32 bits

constexpr int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }

enum { SPEC_RGB = 0, SPEC_THERMAL = 1, SPEC_BOTH = 2 };

struct ExportK {
  const float *means, *scales, *quats, *op, *dc, *rest, *th_dc, *th_rest, *op_th;  // op_th null: shared opacity
  int64_t n;
  int R, spectrum, colour_mode, W;
  float min_logit;
  bool has_box;
  SplatCropK box;
};

int row_width(int R, int spectrum, bool sep) { return 17 + 3 * R + (spectrum == SPEC_BOTH ? 1 + R + (sep ? 1 : 0) : 0); }

// the sh_degree == 0 convention: the model's colour is sigmoid(dc), a viewer's is 0.5 + C0 f_dc
__device__ inline float dc_colour(float v) { return (float)((1.0 / (1.0 + exp(-(double)v)) - 0.5) / 0.28209479177387814); }

// marks in bad[] the Gaussians of the block (g0 .. g0 + cnt) that have a value that is not finite among their `width` floats of p
__device__ inline void mark_nonfinite(const float* __restrict__ p, int width, int64_t g0, int cnt, int* bad) {
  const float* slab = p + g0 * width;
  const int total = cnt * width;
  // j = row * width + col, advanced by EB floats a step without a division per float
  const int drow = EB / width, dcol = EB % width;
  int row = threadIdx.x / width, col = threadIdx.x % width;
#pragma unroll 4
  for (int j = threadIdx.x; j < total; j += EB) {
    if (!isfinite(slab[j])) bad[row] = 1;  // every writer stores the same 1
    row += drow, col += dcol;
    if (col >= width) col -= width, ++row;
  }
}

__global__ void __launch_bounds__(EB) k_export_count(ExportK a, uint8_t* __restrict__ flags, int32_t* __restrict__ block_count) {
  __shared__ int bad[EB];
  __shared__ int wave_count[EB / TN_WAVE];
  const int64_t g0 = (int64_t)blockIdx.x * EB;
  const int cnt = (int)(a.n - g0 < EB ? a.n - g0 : EB);
  bad[threadIdx.x] = 0;
  __syncthreads();
  const bool rgb = a.spectrum != SPEC_THERMAL, th = a.spectrum != SPEC_RGB;
  mark_nonfinite(a.means, 3, g0, cnt, bad);
  mark_nonfinite(a.scales, 3, g0, cnt, bad);
  mark_nonfinite(a.quats, 4, g0, cnt, bad);
  if (rgb) {
    mark_nonfinite(a.dc, 3, g0, cnt, bad);
    if (a.R > 0) mark_nonfinite(a.rest, 3 * a.R, g0, cnt, bad);
  }
  if (th) {
    mark_nonfinite(a.th_dc, 1, g0, cnt, bad);
    if (a.R > 0) mark_nonfinite(a.th_rest, a.R, g0, cnt, bad);
  }
  __syncthreads();
  const int64_t g = g0 + threadIdx.x;
  bool k = false;
  if (g < a.n) {
    // the opacity logits of the row: rgb its own, thermal the thermal one where there is one, both the two of them (kept by the larger)
    const bool use_op = rgb || !a.op_th, use_th = th && a.op_th;
    const float o = use_op ? a.op[g] : 0.0f, t = use_th ? a.op_th[g] : 0.0f;
    const bool fin = (!use_op || isfinite(o)) && (!use_th || isfinite(t));
    const float logit = use_op && use_th ? fmaxf(o, t) : (use_op ? o : t);
    k = !bad[threadIdx.x] && fin && logit >= a.min_logit;
    if (k && a.has_box) k = splat_in_crop(a.box, a.means[3 * g], a.means[3 * g + 1], a.means[3 * g + 2]);
    flags[g] = k ? 1 : 0;
  }
  const int c = __popcll(__ballot(k));
  if (tn_lane() == 0) wave_count[threadIdx.x / TN_WAVE] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < EB / TN_WAVE; ++w) s += wave_count[w];
    block_count[blockIdx.x] = s;
  }
}

// offset[b] = the kept Gaussians of the blocks before b; count = all of them
__global__ void __launch_bounds__(EB) k_export_offsets(const int32_t* __restrict__ block_count, int64_t num_blocks, int64_t* __restrict__ offset,
                                                       int64_t* __restrict__ count) {
  __shared__ int64_t sh[EB];
  __shared__ int64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t b0 = 0; b0 < num_blocks; b0 += EB) {
    const int64_t b = b0 + threadIdx.x;
    const int64_t v = b < num_blocks ? block_count[b] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < EB; o <<= 1) {  // inclusive scan of the chunk
      const int64_t t = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    if (b < num_blocks) offset[b] = carry + sh[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 0) carry += sh[EB - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = carry;
}

// column `col` of Gaussian g's row
__device__ inline float export_value(const ExportK& a, int64_t g, int col) {
  if (col < 3) return a.means[3 * g + col];
  if (col < 6) return 0.0f;
  const bool th = a.spectrum == SPEC_THERMAL;
  if (col < 9) {
    const float v = th ? a.th_dc[g] : a.dc[3 * g + (col - 6)];
    return a.colour_mode == 1 ? dc_colour(v) : v;
  }
  const int R = a.R, o = 9 + 3 * R;
  if (col < o) {  // f_rest_{c R + k} = features_rest[g, k, c]
    const int i = col - 9, c = (i >= R) + (i >= 2 * R), k = i - c * R;
    return th ? a.th_rest[g * R + k] : a.rest[(g * R + k) * 3 + c];
  }
  if (col == o) return th && a.op_th ? a.op_th[g] : a.op[g];
  if (col < o + 4) return a.scales[3 * g + (col - o - 1)];
  if (col < o + 8) return a.quats[4 * g + (col - o - 4)];
  if (col == o + 8) {
    const float v = a.th_dc[g];
    return a.colour_mode == 1 ? dc_colour(v) : v;
  }
  if (col < o + 9 + R) return a.th_rest[g * R + (col - o - 9)];
  return a.op_th[g];  // the last column of a separate-mode `both` row
}

__global__ void __launch_bounds__(EB) k_export_write(ExportK a, const uint8_t* __restrict__ flags, const int64_t* __restrict__ offset,
                                                     float* __restrict__ out_rows) {
  __shared__ int wave_count[EB / TN_WAVE];
  __shared__ int kept[EB];
  const int64_t g0 = (int64_t)blockIdx.x * EB, g = g0 + threadIdx.x;
  const bool k = g < a.n && flags[g] != 0;
  const unsigned long long votes = __ballot(k);
  const int lane = tn_lane(), wave = threadIdx.x / TN_WAVE;
  if (lane == 0) wave_count[wave] = __popcll(votes);
  __syncthreads();
  int before = __popcll(votes & ((1ull << lane) - 1ull)), total = 0;
  for (int w = 0; w < EB / TN_WAVE; ++w) {
    if (w < wave) before += wave_count[w];
    total += wave_count[w];
  }
  if (k) kept[before] = threadIdx.x;
  __syncthreads();
  float* run = out_rows + offset[blockIdx.x] * a.W;  // total <= the Gaussians from g0 on: the run ends inside [N, W]
  const int floats = total * a.W;
  // (row, col) of float j, advanced by EB floats a step without a division per float; EU gathers are issued before their EU stores
  const int drow = EB / a.W, dcol = EB % a.W;
  int row = threadIdx.x / a.W, col = threadIdx.x % a.W;
  for (int j0 = threadIdx.x; j0 < floats; j0 += EU * EB) {
    float v[EU];
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      v[u] = j0 + u * EB < floats ? export_value(a, g0 + kept[row], col) : 0.0f;
      row += drow, col += dcol;
      if (col >= a.W) col -= a.W, ++row;
    }
#pragma unroll
    for (int u = 0; u < EU; ++u)
      if (j0 + u * EB < floats) run[j0 + u * EB] = v[u];
  }
}

struct ExportLayout {
  int64_t flags, counts, offsets, total;
};

ExportLayout export_layout(int64_t n) {
  const int64_t nb = tn_cdiv(n, EB);
  ExportLayout L;
  L.flags = 0;
  L.counts = align256(n);
  L.offsets = L.counts + align256(nb * 4);
  L.total = L.offsets + align256(nb * 8);
  return L;
}

}  // namespace

extern "C" int64_t tn_export_splat_workspace_bytes(int64_t num_gaussians) {
  if (num_gaussians < 0 || num_gaussians > EXPORT_MAX_ROWS) return -1;
  return export_layout(num_gaussians).total;
}

extern "C" int tn_export_splat_pack(const float* means, const float* log_scales, const float* quats, const float* opacities, const float* features_dc,
                                    const float* features_rest, const float* thermal_dc, const float* thermal_rest, const float* opacities_thermal,
                                    int64_t num_gaussians, int32_t num_rest_coeffs, int32_t spectrum, int32_t colour_mode, float min_opacity_logit,
                                    const TnSplatCrop* crop, float* out_rows, int64_t* count, void* workspace, int64_t workspace_bytes,
                                    tn_stream_t stream) {
  const int64_t n = num_gaussians;
  TN_REQUIRE(n >= 0 && n <= EXPORT_MAX_ROWS, "tn_export_splat_pack: %lld Gaussians (0..2^31 - 1)", (long long)n);
  TN_REQUIRE(num_rest_coeffs >= 0 && num_rest_coeffs <= EXPORT_MAX_REST, "tn_export_splat_pack: %d rest coefficients (0..%d)", num_rest_coeffs,
             EXPORT_MAX_REST);
  TN_REQUIRE(spectrum == SPEC_RGB || spectrum == SPEC_THERMAL || spectrum == SPEC_BOTH, "tn_export_splat_pack: spectrum %d (0 rgb, 1 thermal, 2 both)",
             spectrum);
  TN_REQUIRE(colour_mode == 0 || colour_mode == 1, "tn_export_splat_pack: colour_mode %d (0 coefficients as stored, 1 the degree-0 colours)", colour_mode);
  TN_REQUIRE(colour_mode == 0 || num_rest_coeffs == 0, "tn_export_splat_pack: colour_mode 1 has no f_rest columns, %d rest coefficients given",
             num_rest_coeffs);
  TN_REQUIRE(!(min_opacity_logit != min_opacity_logit), "tn_export_splat_pack: min_opacity_logit is NaN (-inf switches the threshold off)");
  TN_REQUIRE(count, "tn_export_splat_pack: null pointer (count)");
  hipStream_t st = tn_s(stream);
  if (n == 0) {
    if (hipMemsetAsync(count, 0, sizeof(int64_t), st) != hipSuccess) {
      tn_set_error("tn_export_splat_pack: could not clear count: %s", hipGetErrorString(hipGetLastError()));
      return TN_ELAUNCH;
    }
    return TN_OK;
  }
  TN_REQUIRE(means && log_scales && quats && opacities && features_dc && thermal_dc && out_rows && workspace, "tn_export_splat_pack: null pointer");
  TN_REQUIRE(num_rest_coeffs == 0 || (features_rest && thermal_rest), "tn_export_splat_pack: null pointer (%d rest coefficients)", num_rest_coeffs);
  TN_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "tn_export_splat_pack: the workspace must be 8-byte aligned");
  const ExportLayout L = export_layout(n);
  TN_REQUIRE(workspace_bytes >= L.total, "tn_export_splat_pack: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  ExportK a{means, log_scales, quats, opacities, features_dc, features_rest, thermal_dc, thermal_rest, opacities_thermal, n, num_rest_coeffs, spectrum,
            colour_mode, row_width(num_rest_coeffs, spectrum, opacities_thermal != nullptr), min_opacity_logit, crop != nullptr, SplatCropK{}};
  if (crop) a.box = make_cropk(crop);
  char* ws = static_cast<char*>(workspace);
  uint8_t* flags = reinterpret_cast<uint8_t*>(ws + L.flags);
  int32_t* counts = reinterpret_cast<int32_t*>(ws + L.counts);
  int64_t* offsets = reinterpret_cast<int64_t*>(ws + L.offsets);
  const int64_t nb = tn_cdiv(n, EB);
  hipLaunchKernelGGL(k_export_count, dim3((unsigned)nb), dim3(EB), 0, st, a, flags, counts);
  TN_CHECK_LAUNCH("tn_export_splat_pack(count)");
  hipLaunchKernelGGL(k_export_offsets, dim3(1), dim3(EB), 0, st, counts, nb, offsets, count);
  TN_CHECK_LAUNCH("tn_export_splat_pack(offsets)");
  hipLaunchKernelGGL(k_export_write, dim3((unsigned)nb), dim3(EB), 0, st, a, flags, offsets, out_rows);
  TN_CHECK_LAUNCH("tn_export_splat_pack(write)");
  return TN_OK;
}
