// N4: forward Gaussian-splat render with an RGB + thermal colour per Gaussian, for gfx950.
//
// What it replaces: the three gsplat calls of SplatfactoModel.get_outputs (nerfstudio/models/splatfacto.py:739-807: project_gaussians,
// spherical_harmonics, rasterize_gaussians twice -- colour and depth).  gsplat (>=0.1.6, pyproject.toml:66) is a third-party CUDA package
// that is not in the reference tree: the arithmetic below follows its published algorithm (see oracle/splat_oracle.py; parity unpinned).
//
// Pipeline (4 launches + one radix sort):
//   k_splat_project    thread = Gaussian: view transform, 3D covariance, EWA projection (+0.3 px blur), conic, 3-sigma radius, tile bounding
//                      box; for visible Gaussians also the view-dependent colour (degree <= 3 SH, RGB and thermal) and the opacity -> one
//                      packed 48-byte record the rasteriser reads with three 16-byte loads
//   depth sort         rocprim radix sort of the N Gaussians by depth bits (32-bit keys, N elements)
//   rocprim scan       inclusive scan of tiles-per-Gaussian in depth order
//   k_splat_intersect  one (tile id, Gaussian id) pair per (Gaussian, tile), emitted in depth order; a wave owns 64 Gaussians and writes
//                      their pairs as ONE contiguous, coalesced range (lane = output position, owner found by binary search in LDS)
//   rocprim radix sort of the pairs on log2(#tiles) bits only (13 bits at 1080p = 2 passes over 8-byte pairs).  gsplat sorts
//                      (tile << 32 | depth) 64-bit keys: 6 passes over 12-byte pairs, 46 % of the frame in the first version of this
//                      file.  A stable sort by tile of a depth-ordered list gives the same order, ties included (equal depths keep the
//                      Gaussian order in both).
//   k_splat_tile_edges start / end of every tile's run
//   k_splat_raster     block = one 16x16 tile = 4 waves, lane = pixel.  256 records at a time are staged through LDS (each thread fetches
//                      one); every lane then walks the batch front to back.  The LDS reads are wave-uniform broadcasts (conflict-free);
//                      a wave whose 64 pixels are all finished skips the arithmetic; the colour (RGB+T) and depth images come out of ONE
//                      pass (the reference runs the rasteriser twice; in "antialiased" mode the depth pass uses the uncompensated
//                      opacity, so that variant carries a second transmittance).  The TRAIN instantiation (tn_splat_raster_chains with out_transmittance / out_last) also
//                      keeps each pixel's final transmittance and last contributor for the backward.
#include <cstring>
#include <tuple>
#include <type_traits>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "tn_common.h"
#include "tn_pose_finish.h"  // pose_exp / pose_exp_bwd: the pose map and its derivative, shared with the ray path

#define SPLAT_BLOCK 16
#define SPLAT_BATCH 256

// alpha = opacity exp(-sigma), sigma = 0.5 (cx dx^2 + cz dy^2) + cy dx dy, is evaluated as exp2(l2op - (A dx^2 + B dx dy + C dy^2)) with
// A = 0.5 cx log2(e), B = cy log2(e), C = 0.5 cz log2(e), l2op = log2(opacity): 5 FMAs + one v_exp_f32 per pixel instead of 9 multiply/adds,
// two scalings and a multiply by the opacity (the rasteriser is VALU-bound: rocprofv3 SQ_ACTIVE_INST_VALU = 70 % of its duration).
struct SplatRec {  // 64 bytes per Gaussian
  float4 a;        // x, y, A, B
  float4 b;        // C, l2op (compensated opacity in antialiased mode), hx, hy: half extents of the box around {alpha >= 1/255}
  float4 c;        // r, g, b, thermal
  float4 d;        // depth, l2op of the plain opacity; separate thermal opacity (SEP): l2op of the plain thermal opacity, l2op of the thermal
                   // opacity the thermal chain blends with (compensated in antialiased mode); else 0, 0
};
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct SplatWs {
  SplatRec* recs;
  int32_t* cum;        // inclusive scan of the tight tile counts in depth order
  int32_t* tbox;       // [N][4] tight tile box (x0, y0, x1, y1): gsplat's 3-sigma box cut down to the tiles alpha >= 1/255 can reach
  int32_t* thits;      // [N] tiles in the tight box
  int32_t* tile_bins;  // [num_tiles][2]
  uint32_t* lkeys[2];  // ~run length per tile (sort key: longest first)
  int32_t* lvals[2];   // tile ids; lvals[1] = the order the rasteriser takes the tiles in
  uint32_t* depth_max; // float bits (depths are positive)
  uint32_t* dkeys;     // sorted depth bits [N]
  int32_t* order;      // Gaussian ids in depth order [N]
  uint32_t* keys[2];   // tile id per intersection
  int32_t* vals[2];    // Gaussian id per intersection
  void* tmp;
  size_t tmp_bytes;
};

struct HitsInOrder {  // tiles-per-Gaussian read through the depth order (input of the scan)
  const int32_t* hits;
  __host__ __device__ int32_t operator()(int32_t id) const { return hits[id]; }
};

static size_t al256(size_t x) { return (x + 255) / 256 * 256; }

struct Carve {  // hands out the pieces of a workspace, each rounded up to 256 bytes; with a null base it only counts (off = the bytes needed)
  char* base;
  size_t off;
  void* take(size_t bytes) { size_t o = off; off += al256(bytes); return base ? (void*)(base + o) : (void*)nullptr; }
};

static size_t sort_tmp_bytes(int64_t capacity, int64_t N) {
  size_t a = 0, b = 0, c = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (size_t)std::max<int64_t>(capacity, 1 << 20), 0, 32);  // also covers the sort of the tile order (<= 2^20 tiles)
  (void)rocprim::radix_sort_pairs(nullptr, c, (uint32_t*)nullptr, (uint32_t*)nullptr, rocprim::counting_iterator<int32_t>(0), (int32_t*)nullptr,
                                  (size_t)std::max<int64_t>(N, 1), 0, 32);
  (void)rocprim::inclusive_scan(nullptr, b, rocprim::make_transform_iterator((const int32_t*)nullptr, HitsInOrder{nullptr}), (int32_t*)nullptr,
                                (size_t)std::max<int64_t>(N, 1), rocprim::plus<int32_t>());
  return al256(std::max(std::max(a, b), c)) + 4096;
}

static SplatWs splat_layout(void* base, int64_t N, int64_t capacity, int32_t num_tiles, size_t* total) {
  SplatWs w;
  Carve cv{(char*)base, 0};
  w.recs = (SplatRec*)cv.take(sizeof(SplatRec) * (size_t)N);
  w.cum = (int32_t*)cv.take(4 * (size_t)N);
  w.tbox = (int32_t*)cv.take(16 * (size_t)N);
  w.thits = (int32_t*)cv.take(4 * (size_t)N);
  w.tile_bins = (int32_t*)cv.take(8 * (size_t)num_tiles);
  w.depth_max = (uint32_t*)cv.take(256);
  for (int i = 0; i < 2; ++i) w.lkeys[i] = (uint32_t*)cv.take(4 * (size_t)num_tiles);
  for (int i = 0; i < 2; ++i) w.lvals[i] = (int32_t*)cv.take(4 * (size_t)num_tiles);
  w.dkeys = (uint32_t*)cv.take(4 * (size_t)N);
  w.order = (int32_t*)cv.take(4 * (size_t)N);
  for (int i = 0; i < 2; ++i) w.keys[i] = (uint32_t*)cv.take(4 * (size_t)capacity);
  for (int i = 0; i < 2; ++i) w.vals[i] = (int32_t*)cv.take(4 * (size_t)capacity);
  w.tmp_bytes = sort_tmp_bytes(capacity, N);
  w.tmp = cv.take(w.tmp_bytes);
  if (total) *total = cv.off;
  return w;
}

extern "C" int64_t tn_splat_workspace_bytes(int64_t num_gaussians, int64_t max_intersections, int32_t num_tiles) {
  if (num_gaussians < 0 || max_intersections < 0 || num_tiles < 1) return -1;
  size_t total = 0;
  (void)splat_layout(nullptr, num_gaussians, max_intersections, num_tiles, &total);
  return (int64_t)total;
}

// ------------------------------------------------------------------------------------------------ projection + colour
__device__ __forceinline__ float sh_eval(int degree, float x, float y, float z, const float* __restrict__ dc, const float* __restrict__ rest, int stride, int ch) {
  // coefficient k of channel ch: k == 0 -> dc[ch], else rest[(k-1)*stride + ch]
  float v = 0.28209479177387814f * dc[ch];
  if (degree < 1) return v;
#define CO(k) rest[((k) - 1) * stride + ch]
  v += 0.4886025119029199f * (-y * CO(1) + z * CO(2) - x * CO(3));
  if (degree < 2) return v;
  float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
  v += 1.0925484305920792f * xy * CO(4) + -1.0925484305920792f * yz * CO(5) + 0.31539156525252005f * (2.0f * zz - xx - yy) * CO(6) +
       -1.0925484305920792f * xz * CO(7) + 0.5462742152960396f * (xx - yy) * CO(8);
  if (degree < 3) return v;
  v += -0.5900435899266435f * y * (3.0f * xx - yy) * CO(9) + 2.890611442640554f * xy * z * CO(10) + -0.4570457994644658f * y * (4.0f * zz - xx - yy) * CO(11) +
       0.3731763325901154f * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * CO(12) + -0.4570457994644658f * x * (4.0f * zz - xx - yy) * CO(13) +
       1.445305721320277f * z * (xx - yy) * CO(14) + -0.5900435899266435f * x * (xx - 3.0f * yy) * CO(15);
#undef CO
  return v;
}

struct SplatCamK {
  float view[12];  // rows of the world->camera matrix (3x4)
  float proj[16];  // full projection matrix (4x4, row-major)
  float fx, fy, cx, cy, clip;
  float pos[3];
  int W, H, tbx, tby;
};

// Extra kernel arguments of an instantiation ride in a parameter pack that is empty in the others, which so keep their argument list and every
// kernel-argument offset: pack_arg<I> is the I-th of them.
template <int I, typename T, typename... R>
__device__ __forceinline__ auto pack_arg(T t, R... r) {
  if constexpr (I == 0) return t;
  else return pack_arg<I - 1>(r...);
}

// pack_has<T> / pack_get<T>: whether the pack holds an argument of type T, and that argument.
template <typename T, typename... R>
inline constexpr bool pack_has = (std::is_same_v<T, R> || ...);
template <typename T, typename A, typename... R>
__device__ __forceinline__ T pack_get(A a, R... r) {
  if constexpr (std::is_same_v<T, A>) return a;
  else return pack_get<T>(r...);
}

// Pose refinement (CameraOptimizer.apply_to_camera, cameras/camera_optimizers.py:178-186: c2w' = c2w [A(p); 0 0 0 1], A = exp_map_SO3xR3).  In the
// rasteriser's convention (F = diag(1, -1, -1), V0 = the view matrix of the TnSplatCamera) that is V' = D V0 with the rigid D = F A(p)^-1 F.
// k_splat_pose_camera writes the corrected camera as a RECORD of SPLAT_POSE_REC floats in device memory -- laid out as SplatCamK begins -- and the
// pose instantiations of the projection kernels (a SplatPoseK / SplatPoseBwdK in their trailing pack) read their camera from it instead of from
// their by-value SplatCamK: the pose never travels to the host.
//   [0..11] view' (3x4 rows)   [12..27] proj' (4x4 rows; row 2 is not read and stays 0)   [28..30] position'   [31] proj_x   [32] proj_y
// proj_x / proj_y: the two entries of the intrinsic part of projection_matrix the kernels' rows depend on (row 0 = proj_x view'[0], row 1 =
// proj_y view'[1], row 3 = view'[2]: one product each).
#define SPLAT_POSE_REC 40
static_assert(SPLAT_POSE_REC == TN_SPLAT_POSE_CAMERA_FLOATS, "the header documents the record's size");
struct SplatPoseK {
  const float* rec;
};
struct SplatPoseBwdK {
  const float* rec;
  double* partial;  // [blocks][12]: every block's sum of dL/d view'
};
__device__ __forceinline__ void splat_pose_load(SplatCamK& cam, const float* __restrict__ rec) {
#pragma unroll
  for (int i = 0; i < 12; ++i) cam.view[i] = rec[i];
#pragma unroll
  for (int i = 0; i < 16; ++i) cam.proj[i] = rec[12 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) cam.pos[i] = rec[28 + i];
}

// (the crop box of the eval render -- SplatCropK, splat_in_crop, make_cropk -- lives in tn_common.h: the point-cloud export tests its points with it too)

// SEP: the thermal channel has an opacity of its own (opac_th_logit, else unused): its log2 goes into the record's two spare floats, and the box
// around {alpha >= 1/255} comes from the larger of the two opacities, so neither chain of the rasteriser loses a contributor.
// Crop (one SplatCropK, or nothing): the crop instantiation tests every mean against the box FIRST.  A Gaussian outside leaves exactly as one behind
// the clip plane does -- radius 0, no tiles, zeros -- and never reaches the sort; a block whose Gaussians are ALL outside (one block-wide vote, taken
// by every thread before the barrier below, so the decision is uniform there) does not stage its SH slab -- 240 of the 300 bytes a Gaussian has at
// degree 3.  Without the pack the kernel is the one it was.
// Pose (one SplatPoseK, or nothing; with or without the box): view, projection rows and position come from the device record (uniform loads).
template <bool SEP, typename... Crop>
__global__ void __launch_bounds__(256) k_splat_project(SplatCamK cam, const float* __restrict__ means, const float* __restrict__ log_scales,
                                                       const float* __restrict__ quats, const float* __restrict__ opac_logit,
                                                       const float* __restrict__ f_dc, const float* __restrict__ f_rest,
                                                       const float* __restrict__ t_dc, const float* __restrict__ t_rest, int64_t N, int sh_degree,
                                                       int rest_coeffs, int antialiased, float2* __restrict__ xys, float* __restrict__ depths,
                                                       int32_t* __restrict__ radii, float* __restrict__ conics, float* __restrict__ comp_out,
                                                       int32_t* __restrict__ tiles_hit, int32_t* __restrict__ tile_box, SplatRec* __restrict__ recs,
                                                       int32_t* __restrict__ tbox, int32_t* __restrict__ thits,
                                                       const float* __restrict__ opac_th_logit, Crop... crop_arg) {
  constexpr bool CROP = pack_has<SplatCropK, Crop...>, POSE = pack_has<SplatPoseK, Crop...>;
  static_assert(sizeof...(Crop) == (CROP ? 1 : 0) + (POSE ? 1 : 0), "the pack takes one SplatCropK, one SplatPoseK, or both");
  if constexpr (POSE) splat_pose_load(cam, pack_get<SplatPoseK>(crop_arg...).rec);
  // The higher-order SH coefficients of the block's 256 Gaussians (45 + 15 floats each) go through LDS: the block copies its contiguous
  // 46 KB + 15 KB slab with coalesced 16-byte loads, and each thread then reads its own coefficients at stride 45 / 15 floats -- odd strides,
  // so the 64 lanes of a wave hit 64 different banks.  Reading them straight from global memory (each lane its own 180-byte run) cost
  // 3.6x the requests the data needs (TCC_REQ 17 M x 64 B for 300 MB) and made the kernel latency-bound (150 us per 1 M Gaussians; 124 us with the staging at 128 Gaussians per block).
  extern __shared__ float sh_lds[];
  float* s_rest = sh_lds;
  float* s_trest = sh_lds + (int)blockDim.x * rest_coeffs * 3;
  [[maybe_unused]] bool in_box = true;
  {
    const int64_t g0 = blockIdx.x * (int64_t)blockDim.x;
    const int cnt = (int)min((int64_t)blockDim.x, N - g0);
    bool stage = rest_coeffs > 0 && sh_degree >= 1;
    if constexpr (CROP) {
      const SplatCropK crop = pack_get<SplatCropK>(crop_arg...);
      const int64_t g = g0 + threadIdx.x;
      in_box = g < N && splat_in_crop(crop, means[3 * g], means[3 * g + 1], means[3 * g + 2]);
      // The vote: one block-wide OR, a barrier that hands every thread the same answer, so `stage` is uniform over the block before the staging
      // barrier below.  Every thread of the block gets here (the tail's threads too: the early return for i >= N comes after both barriers).
      stage = __syncthreads_or(in_box ? 1 : 0) != 0 && stage;
    }
    if (stage) {
      const int n3 = cnt * rest_coeffs * 3, n1 = cnt * rest_coeffs;
      const float* src3 = f_rest + g0 * rest_coeffs * 3;
      const float* src1 = t_rest + g0 * rest_coeffs;
      // both slabs start 16-byte aligned: blockDim * K * 3 * 4 and blockDim * K * 4 bytes per block are multiples of 16
      for (int t = threadIdx.x * 4; t + 3 < n3; t += blockDim.x * 4) *reinterpret_cast<float4*>(s_rest + t) = *reinterpret_cast<const float4*>(src3 + t);
      for (int t = (n3 & ~3) + threadIdx.x; t < n3; t += blockDim.x) s_rest[t] = src3[t];
      for (int t = threadIdx.x * 4; t + 3 < n1; t += blockDim.x * 4) *reinterpret_cast<float4*>(s_trest + t) = *reinterpret_cast<const float4*>(src1 + t);
      for (int t = (n1 & ~3) + threadIdx.x; t < n1; t += blockDim.x) s_trest[t] = src1[t];
    }
    __syncthreads();
  }
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N) return;
  float2 xy = make_float2(0.f, 0.f);
  float depth = 0.f, cmp = 0.f;
  float3 conic = make_float3(0.f, 0.f, 0.f);
  int radius = 0, area = 0;
  int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
  const float mx = means[3 * i], my = means[3 * i + 1], mz = means[3 * i + 2];
  const float* V = cam.view;
  float px = V[0] * mx + V[1] * my + V[2] * mz + V[3];
  float py = V[4] * mx + V[5] * my + V[6] * mz + V[7];
  float pz = V[8] * mx + V[9] * my + V[10] * mz + V[11];
  bool ok = pz > cam.clip;
  if constexpr (CROP) ok = ok && in_box;
  if (ok) {
    // Sigma = (R S)(R S)^T
    float qw = quats[4 * i], qx = quats[4 * i + 1], qy = quats[4 * i + 2], qz = quats[4 * i + 3];
    float qn = 1.0f / sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    qw *= qn; qx *= qn; qy *= qn; qz *= qn;
    float R[9] = {1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - qw * qz), 2.f * (qx * qz + qw * qy),
                  2.f * (qx * qy + qw * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - qw * qx),
                  2.f * (qx * qz - qw * qy), 2.f * (qy * qz + qw * qx), 1.f - 2.f * (qx * qx + qy * qy)};
    float s[3] = {expf(log_scales[3 * i]), expf(log_scales[3 * i + 1]), expf(log_scales[3 * i + 2])};
    float M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) M[3 * r + c] = R[3 * r + c] * s[c];
    float S[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) S[3 * r + c] = M[3 * r] * M[3 * c] + M[3 * r + 1] * M[3 * c + 1] + M[3 * r + 2] * M[3 * c + 2];
    // EWA: clamp to 1.3x the frustum, T = J W, cov2d = T Sigma T^T + 0.3 I
    float tan_x = 0.5f * (float)cam.W / cam.fx, tan_y = 0.5f * (float)cam.H / cam.fy;
    float lx = 1.3f * tan_x, ly = 1.3f * tan_y;
    float tx = pz * fminf(lx, fmaxf(-lx, px / pz));
    float ty = pz * fminf(ly, fmaxf(-ly, py / pz));
    float rz = 1.0f / pz, rz2 = rz * rz;
    float J0[3] = {cam.fx * rz, 0.f, -cam.fx * tx * rz2};
    float J1[3] = {0.f, cam.fy * rz, -cam.fy * ty * rz2};
    float T0[3], T1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      T0[c] = J0[0] * V[c] + J0[1] * V[4 + c] + J0[2] * V[8 + c];
      T1[c] = J1[0] * V[c] + J1[1] * V[4 + c] + J1[2] * V[8 + c];
    }
    float A0[3], A1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      A0[c] = T0[0] * S[c] + T0[1] * S[3 + c] + T0[2] * S[6 + c];
      A1[c] = T1[0] * S[c] + T1[1] * S[3 + c] + T1[2] * S[6 + c];
    }
    float c00 = A0[0] * T0[0] + A0[1] * T0[1] + A0[2] * T0[2];
    float c01 = A0[0] * T1[0] + A0[1] * T1[1] + A0[2] * T1[2];
    float c11 = A1[0] * T1[0] + A1[1] * T1[1] + A1[2] * T1[2];
    float det_orig = c00 * c11 - c01 * c01;
    float a = c00 + 0.3f, b = c01, c = c11 + 0.3f;
    float det = a * c - b * b;
    cmp = sqrtf(fmaxf(0.f, det_orig / det));
    ok = det != 0.f;
    if (ok) {
      float inv = 1.0f / det;
      conic = make_float3(c * inv, -b * inv, a * inv);
      float mid = 0.5f * (a + c);
      float disc = sqrtf(fmaxf(0.1f, mid * mid - det));
      radius = (int)ceilf(3.0f * sqrtf(fmaxf(mid + disc, mid - disc)));
      const float* P = cam.proj;
      float hx = P[0] * mx + P[1] * my + P[2] * mz + P[3];
      float hy = P[4] * mx + P[5] * my + P[6] * mz + P[7];
      float hw = P[12] * mx + P[13] * my + P[14] * mz + P[15];
      float rw = 1.0f / (hw + 1e-6f);
      xy = make_float2(0.5f * (float)cam.W * (hx * rw) + cam.cx - 0.5f, 0.5f * (float)cam.H * (hy * rw) + cam.cy - 0.5f);
      float tcx = xy.x / (float)SPLAT_BLOCK, tcy = xy.y / (float)SPLAT_BLOCK, tr = (float)radius / (float)SPLAT_BLOCK;
      x0 = min(max(0, (int)(tcx - tr)), cam.tbx);
      x1 = min(max(0, (int)(tcx + tr + 1.f)), cam.tbx);
      y0 = min(max(0, (int)(tcy - tr)), cam.tby);
      y1 = min(max(0, (int)(tcy + tr + 1.f)), cam.tby);
      area = (x1 - x0) * (y1 - y0);
      ok = area > 0;
      depth = pz;
    }
  }
  if (!ok) {
    xy = make_float2(0.f, 0.f); depth = 0.f; conic = make_float3(0.f, 0.f, 0.f); radius = 0; area = 0; cmp = 0.f;
    x0 = x1 = y0 = y1 = 0;
  }
  xys[i] = xy;
  depths[i] = depth;
  radii[i] = radius;
  conics[3 * i] = conic.x; conics[3 * i + 1] = conic.y; conics[3 * i + 2] = conic.z;
  comp_out[i] = cmp;
  tiles_hit[i] = area;
  tile_box[4 * i] = x0; tile_box[4 * i + 1] = y0; tile_box[4 * i + 2] = x1; tile_box[4 * i + 3] = y1;
  if (!ok) {
    tbox[4 * i] = tbox[4 * i + 1] = tbox[4 * i + 2] = tbox[4 * i + 3] = 0;
    thits[i] = 0;
    return;
  }
  // view-dependent colour (splatfacto.py:769-777): clamp(SH + 0.5, min 0); degree < 0 means "no SH": sigmoid of the DC term
  float dx = mx - cam.pos[0], dy = my - cam.pos[1], dz = mz - cam.pos[2];
  float dn = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
  dx *= dn; dy *= dn; dz *= dn;
  float col[4];
  const float* rest = s_rest + (int)threadIdx.x * rest_coeffs * 3;
  const float* trest = s_trest + (int)threadIdx.x * rest_coeffs;
  if (sh_degree >= 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) col[ch] = fmaxf(sh_eval(sh_degree, dx, dy, dz, f_dc + 3 * i, rest, 3, ch) + 0.5f, 0.0f);
    col[3] = fmaxf(sh_eval(sh_degree, dx, dy, dz, t_dc + i, trest, 1, 0) + 0.5f, 0.0f);
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) col[ch] = 1.0f / (1.0f + expf(-f_dc[3 * i + ch]));
    col[3] = 1.0f / (1.0f + expf(-t_dc[i]));
  }
  float op = 1.0f / (1.0f + expf(-opac_logit[i]));
  // Where can this Gaussian reach alpha >= 1/255 at all?  alpha = opacity exp(-sigma) >= 1/255  <=>  sigma <= ln(255 opacity) =: s_max, and
  // {sigma <= s_max} is the ellipse d^T cov2d^-1 d <= 2 s_max, whose bounding box has half extents sqrt(2 s_max cov_xx), sqrt(2 s_max cov_yy).
  // Tiles (and, in the rasteriser, 8x8 pixel quadrants) outside that box see nothing of the Gaussian: dropping them is EXACT.  The box is
  // intersected with gsplat's 3-sigma tile box (pixels outside THAT never see the Gaussian in the reference even where alpha >= 1/255).
  // In antialiased mode the depth pass uses the plain opacity (>= the compensated one): the bound uses the larger.
  float op_t = 0.0f;
  if (SEP) op_t = 1.0f / (1.0f + expf(-opac_th_logit[i]));
  float smax = logf(255.0f * (SEP ? fmaxf(op, op_t) : op));
  float hx = -1.0f, hy = -1.0f;
  int bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
  if (smax > 0.0f) {
    float inv_cd = 1.0f / (conic.x * conic.z - conic.y * conic.y);  // cov2d = conic^-1: cov_xx = conic.z / det, cov_yy = conic.x / det
    hx = sqrtf(2.0f * smax * conic.z * inv_cd) * 1.0005f + 1e-3f;
    hy = sqrtf(2.0f * smax * conic.x * inv_cd) * 1.0005f + 1e-3f;
    // tile t holds the pixel centres 16 t + 0.5 .. 16 t + 15.5
    bx0 = max(x0, (int)ceilf((xy.x - hx - 15.5f) / (float)SPLAT_BLOCK));
    bx1 = min(x1, (int)floorf((xy.x + hx - 0.5f) / (float)SPLAT_BLOCK) + 1);
    by0 = max(y0, (int)ceilf((xy.y - hy - 15.5f) / (float)SPLAT_BLOCK));
    by1 = min(y1, (int)floorf((xy.y + hy - 0.5f) / (float)SPLAT_BLOCK) + 1);
    if (bx1 <= bx0 || by1 <= by0) bx0 = bx1 = by0 = by1 = 0;
  }
  tbox[4 * i] = bx0; tbox[4 * i + 1] = by0; tbox[4 * i + 2] = bx1; tbox[4 * i + 3] = by1;
  thits[i] = (bx1 - bx0) * (by1 - by0);
  const float LOG2E = 1.4426950408889634f;
  SplatRec r;
  r.a = make_float4(xy.x, xy.y, 0.5f * conic.x * LOG2E, conic.y * LOG2E);
  r.b = make_float4(0.5f * conic.z * LOG2E, log2f(antialiased ? op * cmp : op), hx, hy);
  r.c = make_float4(col[0], col[1], col[2], col[3]);
  r.d = SEP ? make_float4(depth, log2f(op), log2f(op_t), log2f(antialiased ? op_t * cmp : op_t)) : make_float4(depth, log2f(op), 0.f, 0.f);
  recs[i] = r;
}

// ------------------------------------------------------------------------------------------------ tile binning
// One wave = 64 consecutive Gaussians of the depth order.  Their pairs occupy ONE contiguous range of the output (cum is the inclusive scan
// in the same order), so the lanes walk that range position by position -- coalesced 4-byte stores -- and find the owning Gaussian of a
// position by binary search over the wave's 64 range ends in LDS (a thread-per-Gaussian loop writes 64 scattered streams and serialises
// on the Gaussians that cover hundreds of tiles).
__global__ void __launch_bounds__(256) k_splat_intersect(const int32_t* __restrict__ order, const int32_t* __restrict__ tile_box,
                                                         const int32_t* __restrict__ cum, int64_t N, int tbx, uint32_t* __restrict__ keys,
                                                         int32_t* __restrict__ vals, int64_t capacity) {
  __shared__ int32_t s_end[4][64], s_x0[4][64], s_y0[4][64], s_w[4][64], s_id[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t j0 = (blockIdx.x * (int64_t)(blockDim.x >> 6) + wv) * 64;
  if (j0 >= N) return;  // whole wave
  const int64_t j = j0 + lane;
  int32_t end = 0, g = 0, x0 = 0, y0 = 0, w = 1;
  if (j < N) {
    end = cum[j];
    g = order[j];
    x0 = tile_box[4 * g]; y0 = tile_box[4 * g + 1];
    w = max(tile_box[4 * g + 2] - x0, 1);
  } else {
    end = cum[N - 1];
  }
  s_end[wv][lane] = end; s_x0[wv][lane] = x0; s_y0[wv][lane] = y0; s_w[wv][lane] = w; s_id[wv][lane] = g;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's own LDS writes are visible to its other lanes
  const int64_t begin = j0 == 0 ? 0 : cum[j0 - 1];
  const int64_t stop = s_end[wv][63];
  for (int64_t pos = begin + lane; pos < stop; pos += 64) {
    // first lane o with end_o > pos
    int lo = 0, hi = 63;
    while (lo < hi) {
      int mid = (lo + hi) >> 1;
      if ((int64_t)s_end[wv][mid] > pos) hi = mid; else lo = mid + 1;
    }
    int64_t first = lo == 0 ? begin : (int64_t)s_end[wv][lo - 1];
    int local = (int)(pos - first);
    int ww = s_w[wv][lo];
    int ty = local / ww, tx = local - ty * ww;
    if (pos < capacity) {
      keys[pos] = (uint32_t)((s_y0[wv][lo] + ty) * tbx + s_x0[wv][lo] + tx);
      vals[pos] = s_id[wv][lo];
    }
  }
}

__global__ void k_splat_tile_edges(const uint32_t* __restrict__ keys, int64_t M, int32_t* __restrict__ tile_bins) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= M) return;
  int32_t t = (int32_t)keys[i];
  if (i == 0) tile_bins[2 * t] = 0;
  else {
    int32_t tp = (int32_t)keys[i - 1];
    if (tp != t) { tile_bins[2 * tp + 1] = (int32_t)i; tile_bins[2 * t] = (int32_t)i; }
  }
  if (i == M - 1) tile_bins[2 * t + 1] = (int32_t)M;
}

// longest tiles first: a tile is a sequential front-to-back walk, so the frame ends when the deepest tile ends -- started last (row-major
// order puts the deep centre of the image in the middle of the launch) it runs alone at the end with the rest of the chip idle
__global__ void k_splat_tile_len(const int32_t* __restrict__ tile_bins, int num_tiles, uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= num_tiles) return;
  keys[t] = 0xffffffffu - (uint32_t)(tile_bins[2 * t + 1] - tile_bins[2 * t]);
  vals[t] = t;
}

// ------------------------------------------------------------------------------------------------ rasteriser
// The rules k_splat_raster and k_splat_raster_bwd must agree on bit for bit, each written once.  ALL these helpers take and return scalars on
// purpose: handed a float4 or both axes at once, the compiler packs x and y into v_pk instructions -- the same arithmetic, but no longer the
// instruction stream the rasteriser was tuned and measured with.  After any change to them, compare both kernels' assembly with the parent's
// again (profiles/splat_refactor.md).  lane -> pixel: a wave covers one 8x8 QUADRANT of the tile (the squarest 64-pixel footprint: the per-wave
// culling rejects the most Gaussians for it); 8 lanes = one 128-byte row of the RGBT output.  (qcx, qcy): centre of the quadrant's pixel centres.
__device__ __forceinline__ bool splat_lane_pixel(int tile_x, int tile_y, int W, int H, int& lane, int& wv, int& ix, int& iy, float& pxf, float& pyf,
                                                 float& qcx, float& qcy) {
  lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int qx0 = tile_x * SPLAT_BLOCK + 8 * (wv & 1), qy0 = tile_y * SPLAT_BLOCK + 8 * (wv >> 1);
  ix = qx0 + (lane & 7), iy = qy0 + (lane >> 3);
  pxf = (float)ix + 0.5f, pyf = (float)iy + 0.5f;
  qcx = (float)qx0 + 4.0f, qcy = (float)qy0 + 4.0f;
  return ix < W && iy < H;  // the pixel is inside the image
}
// one axis of the quadrant test: can a Gaussian centred at g with half extent h (k_splat_project's box) reach alpha >= 1/255 around qc?
__device__ __forceinline__ bool splat_axis_hit(float g, float h, float qc) { return fabsf(g - qc) <= h + 3.5f; }
// sigma log2(e) at the offset (dx, dy) = centre - pixel; A, B, C as in SplatRec
__device__ __forceinline__ float splat_power(float A, float B, float Cc, float dx, float dy) { return fmaf(dx, fmaf(A, dx, B * dy), Cc * dy * dy); }
// alpha before the clamp to 0.999 (the backward passes gradient only where the clamp is inactive); then alpha and the gate on it.  The gate's
// other half is power >= 0: the forward leaves a lane with power < 0 before the exponential, the backward tests it.
__device__ __forceinline__ float splat_alpha_raw(float l2op, float power) { return __builtin_amdgcn_exp2f(l2op - power); }
__device__ __forceinline__ float splat_alpha(float raw) { return fminf(0.999f, raw); }
__device__ __forceinline__ bool splat_visible(float alpha) { return alpha >= (1.0f / 255.0f); }

// The SEP instantiations' extra kernel arguments ride in a parameter pack (empty without SEP; pack_arg, above k_splat_project), so that the
// SEP = false kernels keep the argument list -- and with it every kernel-argument offset -- they had before SEP existed: their instruction stream
// is the parent's, bit for bit.
// TRAIN: the training variant (tn_splat_raster_chains with out_transmittance / out_last) also leaves what the backward needs per pixel -- the final transmittance and the number
// of list entries up to and including the last Gaussian that contributed -- and writes the colour BEFORE the clamp to 1 (the caller clamps,
// so the clamp's gradient mask is the caller's).  TRAIN = false is the eval rasteriser, unchanged.
// SEP: the thermal channel blends with its own opacity (SplatRec::d.w) through a transmittance chain of its own (Tt / done_t, the pattern of the
// antialiased depth pass) over the same list, with its own 1e-4 stop; RGB, accumulation and depth stay on the first chain.  It writes the
// thermal accumulation, and in TRAIN the thermal chain's final transmittance and last contributor.  SEP = false is the kernel as it was.
// sep_args (SEP only): float* out_alpha_th, float* out_T_th, int32_t* out_last_th.
template <bool AA, bool TRAIN, bool SEP, typename... SepArgs>
__global__ void __launch_bounds__(256) k_splat_raster(const SplatRec* __restrict__ recs, const int32_t* __restrict__ sorted_ids,
                                                      const int32_t* __restrict__ tile_bins, const int32_t* __restrict__ tile_order, int W, int H,
                                                      int tbx, float4 background, float* __restrict__ out_rgbt, float* __restrict__ out_depth,
                                                      float* __restrict__ out_alpha, uint32_t* __restrict__ depth_max, float* __restrict__ out_T,
                                                      int32_t* __restrict__ out_last, SepArgs... sep_args) {
  static_assert(sizeof...(SepArgs) == (SEP ? 3 : 0), "SEP takes out_alpha_th, out_T_th, out_last_th");
  __shared__ float4 sa[SPLAT_BATCH], sb[SPLAT_BATCH], sc[SPLAT_BATCH], sd[SPLAT_BATCH];
  __shared__ float smax[4];
  const int tile = tile_order[blockIdx.x];
  const int tile_x = tile % tbx, tile_y = tile / tbx;
  int lane, wv, ix, iy;
  float pxf, pyf, qcx, qcy;
  const bool inside = splat_lane_pixel(tile_x, tile_y, W, H, lane, wv, ix, iy, pxf, pyf, qcx, qcy);
  const int begin = tile_bins[2 * tile], end = tile_bins[2 * tile + 1];
  float T = 1.0f, Td = 1.0f, Tt = 1.0f;
  f32x2 acc01 = {0.f, 0.f}, acc23 = {0.f, 0.f};
  float dacc = 0.f;
  bool done = !inside, done_d = !inside, done_t = !inside;
  int last = 0, last_t = 0;  // TRAIN: list entries of this tile up to and including the last contributor (of the thermal chain: last_t)
  // software pipeline: the records of batch i+1 are fetched (two dependent gathers: id, then the 64-byte record) while batch i is blended
  float4 ra, rb, rc, rd;
  ra = rb = rc = rd = make_float4(0.f, 0.f, 0.f, 0.f);
  if (begin + (int)threadIdx.x < end) {
    const SplatRec* r = recs + sorted_ids[begin + (int)threadIdx.x];
    ra = r->a; rb = r->b; rc = r->c; rd = r->d;
  }
  for (int base = begin; base < end; base += SPLAT_BATCH) {
    // all 256 pixels finished -> nothing left to blend in this tile
    if (__syncthreads_count(((AA ? (done && done_d) : done) && (SEP ? done_t : true)) ? 1 : 0) == 256) break;
    sa[threadIdx.x] = ra; sb[threadIdx.x] = rb; sc[threadIdx.x] = rc; sd[threadIdx.x] = rd;
    __syncthreads();
    {
      int nidx = base + SPLAT_BATCH + (int)threadIdx.x;
      if (nidx < end) {
        const SplatRec* r = recs + sorted_ids[nidx];
        ra = r->a; rb = r->b; rc = r->c; rd = r->d;
      }
    }
    const int n = min(SPLAT_BATCH, end - base);
    // the whole wave is done: skip the arithmetic of this batch (wave-uniform branch)
    if (__all(((AA ? (done && done_d) : done) && (SEP ? done_t : true)) ? 1 : 0)) continue;
    // Per-wave culling, 64 Gaussians per step: lane l tests Gaussian 64 q + l against this wave's quadrant (box around {alpha >= 1/255},
    // see k_splat_project); the ballot is the list of Gaussians that can touch the quadrant, walked with scalar bit operations.  A
    // Gaussian that misses the quadrant costs 1/64 of a test instead of a full evaluation on all 64 lanes.
#pragma unroll 1
    for (int q = 0; q < SPLAT_BATCH / 64; ++q) {
      if (q * 64 >= n) break;
      const int kk = q * 64 + lane;
      bool keep = false;
      if (kk < n) {
        float4 a = sa[kk], b = sb[kk];
        keep = splat_axis_hit(a.x, b.z, qcx) && splat_axis_hit(a.y, b.w, qcy);
      }
      uint64_t live = __ballot(keep);
      while (live) {
        const int k = q * 64 + __builtin_ctzll(live);
        live &= live - 1;
        // wave-uniform (broadcast) LDS reads.  Holding the records in registers and broadcasting the fields with v_readlane instead was
        // measured slower (403 vs 360 us: +11 VALU instructions per Gaussian in a kernel that is VALU-issue bound).
        float4 a = sa[k], b = sb[k];
        float dx = a.x - pxf, dy = a.y - pyf;
        float power = splat_power(a.z, a.w, b.x, dx, dy);
        float ex = b.y - power;
        // nobody in the wave can reach alpha >= 1/255 = 2^-7.994 (or the form is negative): skip the exponential and the blend
        // (antialiased: the depth pass blends with the plain opacity, which is the larger one)
        // (SEP: the larger of the two plain opacities bounds every chain)
        if (!__any((power >= 0.f && (SEP ? fmaxf(AA ? sd[k].y : b.y, sd[k].z) - power : (AA ? sd[k].y - power : ex)) >= -8.0f) ? 1 : 0)) continue;
        if (power < 0.f) continue;
        const float alpha = splat_alpha(splat_alpha_raw(b.y, power));
        const bool vis_c = splat_visible(alpha);  // (evaluated ahead of the &&: inside it the compiler branches on `done` first)
        if (!done && vis_c) {
          float nT = fmaf(-alpha, T, T);
          if (nT <= 1e-4f) done = true;  // the pixel stops BEFORE this Gaussian (the backward sees that through `last`)
          else {
            float vis = alpha * T;
            float4 c = sc[k];
            f32x2 v2 = {vis, vis};
            acc01 = __builtin_elementwise_fma(v2, (f32x2){c.x, c.y}, acc01);
            if (SEP) acc23.x = fmaf(vis, c.z, acc23.x);
            else acc23 = __builtin_elementwise_fma(v2, (f32x2){c.z, c.w}, acc23);
            if (!AA) dacc = fmaf(vis, sd[k].x, dacc);
            T = nT;
            if (TRAIN) last = base + k - begin + 1;
          }
        }
        if (AA) {
          float4 d = sd[k];
          const float alpha_d = splat_alpha(splat_alpha_raw(d.y, power));
          const bool vis_d = splat_visible(alpha_d);
          if (!done_d && vis_d) {
            float nT = fmaf(-alpha_d, Td, Td);
            if (nT <= 1e-4f) done_d = true;
            else { dacc = fmaf(alpha_d * Td, d.x, dacc); Td = nT; }
          }
        }
        if (SEP) {
          const float alpha_t = splat_alpha(splat_alpha_raw(sd[k].w, power));
          const bool vis_t = splat_visible(alpha_t);
          if (!done_t && vis_t) {
            float nT = fmaf(-alpha_t, Tt, Tt);
            if (nT <= 1e-4f) done_t = true;  // the thermal chain's own stop, the same rule
            else {
              acc23.y = fmaf(alpha_t * Tt, sc[k].w, acc23.y);
              Tt = nT;
              if (TRAIN) last_t = base + k - begin + 1;
            }
          }
        }
      }
    }
  }
  const float acc[4] = {acc01.x, acc01.y, acc23.x, acc23.y};
  float dmax = 0.f;
  if (inside) {
    int64_t p = (int64_t)iy * W + ix;
    const float Tw = SEP ? Tt : T;  // what is left for the thermal background
    if (TRAIN) {
      reinterpret_cast<float4*>(out_rgbt)[p] =
          make_float4(acc[0] + T * background.x, acc[1] + T * background.y, acc[2] + T * background.z, acc[3] + Tw * background.w);
      out_T[p] = T;
      out_last[p] = last;
      if constexpr (SEP) { pack_arg<1>(sep_args...)[p] = Tt; pack_arg<2>(sep_args...)[p] = last_t; }
    } else {
      float4 o = make_float4(fminf(acc[0] + T * background.x, 1.0f), fminf(acc[1] + T * background.y, 1.0f), fminf(acc[2] + T * background.z, 1.0f),
                             fminf(acc[3] + Tw * background.w, 1.0f));
      reinterpret_cast<float4*>(out_rgbt)[p] = o;
    }
    out_alpha[p] = 1.0f - T;
    if constexpr (SEP) pack_arg<0>(sep_args...)[p] = 1.0f - Tt;
    out_depth[p] = dacc;  // un-normalised: k_splat_depth_finalize divides by alpha
    dmax = dacc;
  }
  // max of the un-normalised depth image (the reference fills alpha == 0 pixels with it, splatfacto.py:809); depths are >= 0
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, o, 64));
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = dmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    if (m > 0.f) atomicMax(depth_max, __float_as_uint(m));
  }
}

__global__ void k_splat_depth_finalize(float* __restrict__ depth, const float* __restrict__ alpha, const uint32_t* __restrict__ depth_max, int64_t n) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  float a = alpha[i];
  depth[i] = a > 0.f ? depth[i] / a : __uint_as_float(*depth_max);
}

// The removal renders of the separate thermal opacity (ThermalNeRF's, models/thermal_nerfacto.py:460-487, opacities for densities): the frame
// composited only from the Gaussians on which the two spectra agree.  With o, ot the plain opacities: keep_rgb = |o - ot| < thr o,
// keep_th = |ot - o| < thr ot (strict: thr = 0 keeps nothing).  Eval only, a sibling of k_splat_raster<*, false, true> over the same lists: the
// same tile order, lane -> pixel map, batches, pipelined gather, quadrant ballot and whole-wave skip, and its two chains' rules -- but only the
// two removal chains, no depth, no accumulation.  The thread that stages a record decides both keeps from exp2 of SplatRec::d.y / d.z and stores
// the two log-opacities the chains blend with (b.y, d.w) as they are, or as -inf when masked: a masked Gaussian then fails the 1/255 gate like any
// faint one, and the inner loop holds no test of its own for it.  A chain that keeps everything therefore does k_splat_raster's arithmetic in
// k_splat_raster's order: its image is that kernel's, bit for bit.  AA needs no instantiation here: b.y and d.w already hold what each mode blends
// with, and the compensation cancels in the comparison.  out: [H][W][4] = removal RGB over background.xyz, removal thermal over background.w.
__global__ void __launch_bounds__(256) k_splat_raster_removal(const SplatRec* __restrict__ recs, const int32_t* __restrict__ sorted_ids,
                                                              const int32_t* __restrict__ tile_bins, const int32_t* __restrict__ tile_order, int W, int H,
                                                              int tbx, float4 background, float thr, float* __restrict__ out) {
  __shared__ float4 sa[SPLAT_BATCH], sb[SPLAT_BATCH], sc[SPLAT_BATCH];
  __shared__ float sl2t[SPLAT_BATCH];  // l2op the thermal chain blends with (sb[].y is the RGB chain's), -inf when masked
  const int tile = tile_order[blockIdx.x];
  const int tile_x = tile % tbx, tile_y = tile / tbx;
  int lane, wv, ix, iy;
  float pxf, pyf, qcx, qcy;
  const bool inside = splat_lane_pixel(tile_x, tile_y, W, H, lane, wv, ix, iy, pxf, pyf, qcx, qcy);
  const int begin = tile_bins[2 * tile], end = tile_bins[2 * tile + 1];
  float T = 1.0f, Tt = 1.0f;
  f32x2 acc01 = {0.f, 0.f}, acc23 = {0.f, 0.f};
  bool done = !inside, done_t = !inside;
  float4 ra, rb, rc, rd;
  ra = rb = rc = rd = make_float4(0.f, 0.f, 0.f, 0.f);
  if (begin + (int)threadIdx.x < end) {
    const SplatRec* r = recs + sorted_ids[begin + (int)threadIdx.x];
    ra = r->a; rb = r->b; rc = r->c; rd = r->d;
  }
  for (int base = begin; base < end; base += SPLAT_BATCH) {
    if (__syncthreads_count((done && done_t) ? 1 : 0) == 256) break;
    {
      const float o = __builtin_amdgcn_exp2f(rd.y), ot = __builtin_amdgcn_exp2f(rd.z);
      const float diff = fabsf(o - ot);
      const float ninf = -__builtin_inff();
      sa[threadIdx.x] = ra;
      sb[threadIdx.x] = make_float4(rb.x, diff < thr * o ? rb.y : ninf, rb.z, rb.w);
      sc[threadIdx.x] = rc;
      sl2t[threadIdx.x] = diff < thr * ot ? rd.w : ninf;
    }
    __syncthreads();
    {
      int nidx = base + SPLAT_BATCH + (int)threadIdx.x;
      if (nidx < end) {
        const SplatRec* r = recs + sorted_ids[nidx];
        ra = r->a; rb = r->b; rc = r->c; rd = r->d;
      }
    }
    const int n = min(SPLAT_BATCH, end - base);
    if (__all((done && done_t) ? 1 : 0)) continue;
#pragma unroll 1
    for (int q = 0; q < SPLAT_BATCH / 64; ++q) {
      if (q * 64 >= n) break;
      const int kk = q * 64 + lane;
      bool keep = false;
      if (kk < n) {
        float4 a = sa[kk], b = sb[kk];
        // (a Gaussian masked in both chains leaves the walk here, before any lane evaluates it)
        keep = splat_axis_hit(a.x, b.z, qcx) && splat_axis_hit(a.y, b.w, qcy) && fmaxf(b.y, sl2t[kk]) >= -8.0f;
      }
      uint64_t live = __ballot(keep);
      while (live) {
        const int k = q * 64 + __builtin_ctzll(live);
        live &= live - 1;
        float4 a = sa[k], b = sb[k];
        const float l2t = sl2t[k];
        float dx = a.x - pxf, dy = a.y - pyf;
        float power = splat_power(a.z, a.w, b.x, dx, dy);
        // nobody in the wave can reach alpha >= 1/255 in either chain: the larger of the two masked opacities bounds both
        if (!__any((power >= 0.f && fmaxf(b.y, l2t) - power >= -8.0f) ? 1 : 0)) continue;
        if (power < 0.f) continue;
        const float alpha = splat_alpha(splat_alpha_raw(b.y, power));
        const bool vis_c = splat_visible(alpha);
        if (!done && vis_c) {
          float nT = fmaf(-alpha, T, T);
          if (nT <= 1e-4f) done = true;
          else {
            float vis = alpha * T;
            float4 c = sc[k];
            f32x2 v2 = {vis, vis};
            acc01 = __builtin_elementwise_fma(v2, (f32x2){c.x, c.y}, acc01);
            acc23.x = fmaf(vis, c.z, acc23.x);
            T = nT;
          }
        }
        const float alpha_t = splat_alpha(splat_alpha_raw(l2t, power));
        const bool vis_t = splat_visible(alpha_t);
        if (!done_t && vis_t) {
          float nT = fmaf(-alpha_t, Tt, Tt);
          if (nT <= 1e-4f) done_t = true;
          else {
            acc23.y = fmaf(alpha_t * Tt, sc[k].w, acc23.y);
            Tt = nT;
          }
        }
      }
    }
  }
  if (inside) {
    const float acc[4] = {acc01.x, acc01.y, acc23.x, acc23.y};
    reinterpret_cast<float4*>(out)[(int64_t)iy * W + ix] =
        make_float4(fminf(acc[0] + T * background.x, 1.0f), fminf(acc[1] + T * background.y, 1.0f), fminf(acc[2] + T * background.z, 1.0f),
                    fminf(acc[3] + Tt * background.w, 1.0f));
  }
}

// ------------------------------------------------------------------------------------------------ backward
// The exact derivative of the forward above (rgb, thermal, accumulation; depth only through the DEPTH instantiations below, which the
// depth groups of the two backward entry points select).  Three steps, no float atomics, so the gradients are bit-reproducible:
//   k_splat_raster_bwd  block = one tile, same lane -> pixel map as the forward.  Every pixel walks its list from the last contributor back
//                       to the front, recomputing alpha under the forward's rules and the transmittance before each Gaussian as T / (1 - alpha).
//                       The SPLAT_PAIR_GRADS partial sums of a (tile, Gaussian) pair are reduced over the wave (fixed butterfly), then over the
//                       4 waves (fixed order), and written ONCE to the pair's record.  Records sit at the pair's position in the depth-ordered
//                       list k_splat_intersect emitted before the sort by tile: there each Gaussian's pairs form one contiguous run.
//   k_splat_pair_fold   thread = Gaussian: sums its run in list order -> d xys, d conics, d colour (RGB+T), d ln(opacity)
//   k_splat_project_bwd thread = Gaussian: through the EWA projection, the covariance, the quaternion normalisation, SH and sigmoids to the
//                       parameters, written in their own layouts.
#define SPLAT_PAIR_GRADS 10  // per pair, summed over pixels: dsigma*dx, dsigma*dy, dsigma*dx^2/2, dsigma*dx*dy, dsigma*dy^2/2, d colour (4), d ln(opacity)
#define SPLAT_PAIR_GRADS_SEP (SPLAT_PAIR_GRADS + 1)  // separate thermal opacity: one more, d ln(thermal opacity)
// ABS (absgrad, the densification statistic of AbsGS / gsplat): two more slots at the END of the record (after d ln(thermal opacity) in SEP),
// sum over pixels of |J.x|, |J.y| with J = dsigma * (cx dx + cy dy, cy dx + cz dy) the pixel's term of d xys, both chains added BEFORE the
// absolute value.  The rasteriser holds the conic only in splat_power's scaled form (A, B, C) = (cx / 2, cy, cz / 2) log2(e), so the slots carry
// log2(e) |J| = |dsigma (2A dx + B dy)|, |dsigma (B dx + 2C dy)| (the doubling is exact) and k_splat_pair_fold multiplies the sum by ln 2.
#define SPLAT_PAIR_ABS 2
// DEPTH (an upstream gradient of the depth image, classic mode): depth = D / A with D = sum alpha_i T_i z_i on chain 1 (the RGB chain, in SEP too)
// and A = 1 - T_final > 0; elsewhere depth is the frame's maximum of D, a value without gradient.  With v_depth = dL / d depth that is a fifth
// colour channel without a background term plus a correction of v_alpha, per pixel
//   vD = v_depth / A (0 where A == 0),   v_alpha_eff = v_alpha - vD * depth   (d depth / d A = -D / A^2 = -depth / A)
// so inside the walk of chain 1 cv gains z_k vD (z_k = SplatRec::d.x), `rest` starts from v_alpha_eff, and the pair record gains ONE slot,
// d z = vis * vD, behind d ln(thermal opacity) and before the SPLAT_PAIR_ABS slots; k_splat_pair_fold sums it into v_depths [N] = dL / d depths.
#define SPLAT_PAIR_DEPTH 1
struct SplatDepthBwdK {  // the DEPTH instantiations' extra kernel argument (last in the pack)
  const float* depth;    // [H,W] the forward's normalised depth image
  const float* v_depth;  // [H,W] dL / d depth
};
struct SplatDepthFoldK {  // k_splat_pair_fold's
  float* v_depths;  // [N]
};

struct SplatBwdWs {
  float* pair;     // [max_intersections][SPLAT_PAIR_GRADS or SPLAT_PAIR_GRADS_SEP (+ SPLAT_PAIR_DEPTH) (+ SPLAT_PAIR_ABS)]
  int32_t* start;  // [N] first record of each Gaussian's run
};

static SplatBwdWs splat_bwd_layout(void* base, int64_t N, int64_t capacity, int pair_grads, size_t* total) {
  SplatBwdWs w;
  Carve cv{(char*)base, 0};
  w.pair = (float*)cv.take(sizeof(float) * pair_grads * (size_t)std::max<int64_t>(capacity, 1));
  w.start = (int32_t*)cv.take(4 * (size_t)std::max<int64_t>(N, 1));
  if (total) *total = cv.off;
  return w;
}

static int splat_pair_grads(bool sep, bool absgrad, bool depth) {
  return (sep ? SPLAT_PAIR_GRADS_SEP : SPLAT_PAIR_GRADS) + (depth ? SPLAT_PAIR_DEPTH : 0) + (absgrad ? SPLAT_PAIR_ABS : 0);
}

extern "C" int64_t tn_splat_backward_workspace_bytes(int64_t num_gaussians, int64_t max_intersections, int32_t sep, int32_t absgrad, int32_t depth) {
  if (num_gaussians < 0 || max_intersections < 0) return -1;
  size_t total = 0;
  (void)splat_bwd_layout(nullptr, num_gaussians, max_intersections, splat_pair_grads(sep != 0, absgrad != 0, depth != 0), &total);
  return (int64_t)total;
}

// start of Gaussian order[j]'s run of pairs: cum is the inclusive scan of the tight tile counts in depth order
__global__ void k_splat_run_start(const int32_t* __restrict__ order, const int32_t* __restrict__ cum, const int32_t* __restrict__ thits, int64_t N,
                                  int32_t* __restrict__ start) {
  int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= N) return;
  const int32_t g = order[j];
  start[g] = cum[j] - thits[g];
}

// SEP (separate thermal opacity): every pixel walks from the larger of its two chains' last contributors and keeps two T / rest pairs.  RGB and
// v_alpha feed chain 1 (alpha from SplatRec::b.y), the thermal channel and v_alpha_th chain 2 (alpha from SplatRec::d.w); the five geometry sums
// receive both chains' d_sigma, and the pair record grows by d ln(thermal opacity).  SEP = false is the kernel as it was.
// sep_args (SEP only): const float* final_T_th, const int32_t* last_th, const float* v_alpha_th.
// ABS: the record grows by the SPLAT_PAIR_ABS slots, which take the path of the others (lane, butterfly, sp, four waves in order, one write).
// ABS = false is the kernel as it was.  Static LDS: 61 440 B, SEP 66 560 B (gfx950 has 160 KB per CU: two blocks per CU as before).
// DEPTH (one SplatDepthBwdK behind the SEP arguments, see SPLAT_PAIR_DEPTH): the record grows by d z, which takes the path of the others, and the
// batch's z_k sit in one more float[SPLAT_BATCH].  Without it the kernel is the one it was.  Static LDS of the largest instantiation (SEP + ABS +
// DEPTH: 14 sums): 71 684 B, below the 80 KB that keep two blocks per CU.
template <bool SEP, bool ABS, typename... SepArgs>
__global__ void __launch_bounds__(256) k_splat_raster_bwd(const SplatRec* __restrict__ recs, const int32_t* __restrict__ sorted_ids,
                                                          const int32_t* __restrict__ tile_bins, const int32_t* __restrict__ tile_order, int W, int H,
                                                          int tbx, float4 background, const float* __restrict__ final_T, const int32_t* __restrict__ last,
                                                          const float* __restrict__ v_rgbt, const float* __restrict__ v_alpha,
                                                          const int32_t* __restrict__ start, const int32_t* __restrict__ tbox, float* __restrict__ pair,
                                                          SepArgs... sep_args) {
  constexpr bool DEPTH = pack_has<SplatDepthBwdK, SepArgs...>;
  static_assert(sizeof...(SepArgs) == (SEP ? 3 : 0) + (DEPTH ? 1 : 0), "SEP takes final_T_th, last_th, v_alpha_th; DEPTH one SplatDepthBwdK behind them");
  constexpr int NG = (SEP ? SPLAT_PAIR_GRADS_SEP : SPLAT_PAIR_GRADS) + (DEPTH ? SPLAT_PAIR_DEPTH : 0) + (ABS ? SPLAT_PAIR_ABS : 0);
  constexpr int TH = SEP ? SPLAT_PAIR_GRADS : NG - 1;  // SEP: the slot of d ln(thermal opacity)
  constexpr int DZ = SEP ? SPLAT_PAIR_GRADS_SEP : SPLAT_PAIR_GRADS;  // DEPTH: the slot of d z
  __shared__ float4 sa[SPLAT_BATCH], sb[SPLAT_BATCH], sc[SPLAT_BATCH];
  float* l2t = nullptr;  // SEP: l2op of the thermal chain (SplatRec::d.w) of the batch's Gaussians
  if constexpr (SEP) {
    __shared__ float s_l2t[SPLAT_BATCH];
    l2t = s_l2t;
  }
  [[maybe_unused]] float* sz = nullptr;  // DEPTH: view-space depth (SplatRec::d.x) of the batch's Gaussians
  if constexpr (DEPTH) {
    __shared__ float s_z[SPLAT_BATCH];
    sz = s_z;
  }
  __shared__ float sp[4][NG][SPLAT_BATCH];  // per wave partial sums of the batch's Gaussians (SEP: 57 KB of LDS with the records, 2 blocks per CU as before)
  __shared__ int s_n;
  const int tile = tile_order[blockIdx.x];
  const int tile_x = tile % tbx, tile_y = tile / tbx;
  int lane, wv, ix, iy;
  float pxf, pyf, qcx, qcy;
  const bool inside = splat_lane_pixel(tile_x, tile_y, W, H, lane, wv, ix, iy, pxf, pyf, qcx, qcy);
  const int begin = tile_bins[2 * tile];
  // T: transmittance after the Gaussian being visited (starts at the final one); rest: sum over the Gaussians behind it of
  // alpha_j T_j <colour_j, v> plus the background's T_final <bg, v> - T_final d accumulation (accumulation = 1 - T_final)
  float T = 1.f, rest = 0.f;
  float Tt = 1.f, rest_t = 0.f;  // SEP: the thermal chain's
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  [[maybe_unused]] float vD = 0.f;  // DEPTH: v_depth / accumulation
  int n = 0, nt = 0;
  if (inside) {
    const int64_t p = (int64_t)iy * W + ix;
    T = final_T[p];
    n = last[p];
    v = reinterpret_cast<const float4*>(v_rgbt)[p];
    float va = v_alpha[p];
    if constexpr (DEPTH) {  // v_alpha_eff; the depth channel has no background term
      const SplatDepthBwdK dk = pack_get<SplatDepthBwdK>(sep_args...);
      const float acc = 1.0f - T;  // the accumulation as the forward wrote it
      vD = acc > 0.f ? dk.v_depth[p] / acc : 0.f;
      va = va - vD * dk.depth[p];
    }
    if constexpr (SEP) {
      rest = T * (v.x * background.x + v.y * background.y + v.z * background.z - va);
      Tt = pack_arg<0>(sep_args...)[p];
      nt = pack_arg<1>(sep_args...)[p];
      rest_t = Tt * (v.w * background.w - pack_arg<2>(sep_args...)[p]);
    } else {
      rest = T * (v.x * background.x + v.y * background.y + v.z * background.z + v.w * background.w - va);
    }
  }
  int wn = SEP ? max(n, nt) : n;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wn = max(wn, __shfl_xor(wn, o, 64));
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  if (lane == 0 && wn > 0) atomicMax(&s_n, wn);
  __syncthreads();
  const int top = begin + s_n;
  for (int hi = top; hi > begin; hi -= SPLAT_BATCH) {
    const int lo = max(begin, hi - SPLAT_BATCH), cnt = hi - lo;
    __syncthreads();  // the previous batch's records and partial sums are consumed
    int64_t dst = -1;
    if ((int)threadIdx.x < cnt) {
      const int g = sorted_ids[lo + (int)threadIdx.x];
      const SplatRec* r = recs + g;
      sa[threadIdx.x] = r->a; sb[threadIdx.x] = r->b; sc[threadIdx.x] = r->c;
      if (SEP) l2t[threadIdx.x] = r->d.w;
      if constexpr (DEPTH) sz[threadIdx.x] = r->d.x;
      const int4 bx = reinterpret_cast<const int4*>(tbox)[g];
      dst = (int64_t)start[g] + (tile_y - bx.y) * (bx.z - bx.x) + (tile_x - bx.x);
    }
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int c = 0; c < NG; ++c) sp[w][c][threadIdx.x] = 0.f;
    __syncthreads();
    // back to front; per-wave culling as in the forward (the quadrant test is exact: outside it alpha < 1/255)
#pragma unroll 1
    for (int q = (cnt - 1) >> 6; q >= 0; --q) {
      const int kk = q * 64 + lane;
      bool keep = false;
      if (kk < cnt && lo + kk < begin + wn) {
        float4 a = sa[kk], b = sb[kk];
        keep = splat_axis_hit(a.x, b.z, qcx) && splat_axis_hit(a.y, b.w, qcy);
      }
      uint64_t live = __ballot(keep);
      while (live) {
        const int bit = 63 - __builtin_clzll(live);
        live &= ~(1ull << bit);
        const int k = q * 64 + bit;
        // the forward's rules (the helpers above): the same set of contributors
        const float4 a = sa[k], b = sb[k];
        const float dx = a.x - pxf, dy = a.y - pyf;
        const float power = splat_power(a.z, a.w, b.x, dx, dy);
        const float raw = splat_alpha_raw(b.y, power);
        const float alpha = splat_alpha(raw);
        const bool use = lo + k - begin < n && power >= 0.f && splat_visible(alpha);
        float raw_t = 0.f, alpha_t = 0.f;
        bool use_t = false;
        if (SEP) {
          raw_t = splat_alpha_raw(l2t[k], power);
          alpha_t = splat_alpha(raw_t);
          use_t = lo + k - begin < nt && power >= 0.f && splat_visible(alpha_t);
        }
        if (!__any((SEP ? (use || use_t) : use) ? 1 : 0)) continue;
        float g[NG];
#pragma unroll
        for (int c = 0; c < NG; ++c) g[c] = 0.f;
        if (use) {
          const float om = 1.0f - alpha;
          T = T / om;  // transmittance in front of this Gaussian
          const float4 col = sc[k];
          float cv = SEP ? col.x * v.x + col.y * v.y + col.z * v.z : col.x * v.x + col.y * v.y + col.z * v.z + col.w * v.w;
          if constexpr (DEPTH) cv += sz[k] * vD;  // the fifth channel
          const float vis = alpha * T;
          const float d_alpha = T * cv - rest / om;
          rest = fmaf(vis, cv, rest);
          g[5] = vis * v.x; g[6] = vis * v.y; g[7] = vis * v.z;
          if (!SEP) g[8] = vis * v.w;
          if constexpr (DEPTH) g[DZ] = vis * vD;
          if (raw <= 0.999f) {  // the clamp passes gradient where torch.clamp's backward does
            const float d_lnop = d_alpha * alpha;  // alpha = opacity exp(-sigma)
            const float d_sigma = -d_lnop;
            g[0] = d_sigma * dx; g[1] = d_sigma * dy;
            g[2] = 0.5f * d_sigma * dx * dx; g[3] = d_sigma * dx * dy; g[4] = 0.5f * d_sigma * dy * dy;
            g[9] = d_lnop;
          }
        }
        if (SEP && use_t) {  // the thermal chain: the same derivative with its own alpha, T and rest
          const float om = 1.0f - alpha_t;
          Tt = Tt / om;
          const float cv = sc[k].w * v.w;
          const float vis = alpha_t * Tt;
          const float d_alpha = Tt * cv - rest_t / om;
          rest_t = fmaf(vis, cv, rest_t);
          g[8] = vis * v.w;
          if (raw_t <= 0.999f) {
            const float d_lnop = d_alpha * alpha_t;
            const float d_sigma = -d_lnop;
            g[0] += d_sigma * dx; g[1] += d_sigma * dy;
            g[2] += 0.5f * d_sigma * dx * dx; g[3] += d_sigma * dx * dy; g[4] += 0.5f * d_sigma * dy * dy;
            g[TH] = d_lnop;
          }
        }
        if constexpr (ABS) {  // g[0], g[1] = dsigma dx, dsigma dy of this pixel, both chains added (0 on the clamp and for a lane that does not blend)
          g[NG - 2] = fabsf((a.z + a.z) * g[0] + a.w * g[1]);
          g[NG - 1] = fabsf(a.w * g[0] + (b.x + b.x) * g[1]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
          for (int c = 0; c < NG; ++c) g[c] += __shfl_xor(g[c], o, 64);
        if (lane == 0) {
#pragma unroll
          for (int c = 0; c < NG; ++c) sp[wv][c][k] = g[c];
        }
      }
    }
    __syncthreads();
    if (dst >= 0) {
      float* o = pair + dst * NG;
#pragma unroll
      for (int c = 0; c < NG; ++c) o[c] = ((sp[0][c][threadIdx.x] + sp[1][c][threadIdx.x]) + sp[2][c][threadIdx.x]) + sp[3][c][threadIdx.x];
    }
  }
}

// NG = SPLAT_PAIR_GRADS, or SPLAT_PAIR_GRADS_SEP: the sum after the ten is d ln(thermal opacity) -> v_lnop_th.  abs_args (ABS only, NG is then
// SPLAT_PAIR_ABS larger): float* v_xys_abs [N,2], the record's last two sums times ln 2 (see SPLAT_PAIR_ABS).  Without it the kernel as it was.
// DEPTH (one SplatDepthFoldK in the pack, NG SPLAT_PAIR_DEPTH larger): the sum behind d ln(thermal opacity) -> v_depths [N].
template <int NG, typename... AbsArgs>
__global__ void k_splat_pair_fold(const float* __restrict__ pair, const int32_t* __restrict__ start, const int32_t* __restrict__ thits,
                                  const float* __restrict__ conics, int64_t N, float* __restrict__ v_xys, float* __restrict__ v_conics,
                                  float* __restrict__ v_colors, float* __restrict__ v_lnop, float* __restrict__ v_lnop_th, AbsArgs... abs_args) {
  constexpr bool ABS = pack_has<float*, AbsArgs...>, DEPTH = pack_has<SplatDepthFoldK, AbsArgs...>;
  constexpr int BASE = NG - (ABS ? SPLAT_PAIR_ABS : 0) - (DEPTH ? SPLAT_PAIR_DEPTH : 0);
  static_assert(sizeof...(AbsArgs) == (ABS ? 1 : 0) + (DEPTH ? 1 : 0) && (BASE == SPLAT_PAIR_GRADS || BASE == SPLAT_PAIR_GRADS_SEP),
                "ABS takes v_xys_abs and SPLAT_PAIR_ABS more sums, DEPTH a SplatDepthFoldK and SPLAT_PAIR_DEPTH more");
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N) return;
  float s[NG];
#pragma unroll
  for (int c = 0; c < NG; ++c) s[c] = 0.f;
  const int cnt = thits[i];
  if (cnt > 0) {
    const float* p = pair + (int64_t)start[i] * NG;
    for (int j = 0; j < cnt; ++j, p += NG)
#pragma unroll
      for (int c = 0; c < NG; ++c) s[c] += p[c];
  }
  // d sigma / d xy = (cx dx + cy dy, cy dx + cz dy), dx = x - pixel
  const float cx = conics[3 * i], cy = conics[3 * i + 1], cz = conics[3 * i + 2];
  v_xys[2 * i] = cx * s[0] + cy * s[1];
  v_xys[2 * i + 1] = cy * s[0] + cz * s[1];
  v_conics[3 * i] = s[2]; v_conics[3 * i + 1] = s[3]; v_conics[3 * i + 2] = s[4];
  v_colors[4 * i] = s[5]; v_colors[4 * i + 1] = s[6]; v_colors[4 * i + 2] = s[7]; v_colors[4 * i + 3] = s[8];
  v_lnop[i] = s[9];
  constexpr bool SEP = BASE > SPLAT_PAIR_GRADS;
  if (SEP) v_lnop_th[i] = s[SEP ? SPLAT_PAIR_GRADS : NG - 1];
  if constexpr (DEPTH) pack_get<SplatDepthFoldK>(abs_args...).v_depths[i] = s[BASE];
  if constexpr (ABS) {
    float* v_xys_abs = pack_get<float*>(abs_args...);
    v_xys_abs[2 * i] = s[NG - 2] * 0.6931471805599453f;
    v_xys_abs[2 * i + 1] = s[NG - 1] * 0.6931471805599453f;
  }
}

// SH basis of degree <= 3 at the unit direction (x, y, z), the coefficients of sh_eval
__device__ __forceinline__ void sh_basis(int degree, float x, float y, float z, float* b) {
  b[0] = 0.28209479177387814f;
  if (degree < 1) return;
  b[1] = -0.4886025119029199f * y; b[2] = 0.4886025119029199f * z; b[3] = -0.4886025119029199f * x;
  if (degree < 2) return;
  float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
  b[4] = 1.0925484305920792f * xy; b[5] = -1.0925484305920792f * yz; b[6] = 0.31539156525252005f * (2.0f * zz - xx - yy);
  b[7] = -1.0925484305920792f * xz; b[8] = 0.5462742152960396f * (xx - yy);
  if (degree < 3) return;
  b[9] = -0.5900435899266435f * y * (3.0f * xx - yy); b[10] = 2.890611442640554f * xy * z; b[11] = -0.4570457994644658f * y * (4.0f * zz - xx - yy);
  b[12] = 0.3731763325901154f * z * (2.0f * zz - 3.0f * xx - 3.0f * yy); b[13] = -0.4570457994644658f * x * (4.0f * zz - xx - yy);
  b[14] = 1.445305721320277f * z * (xx - yy); b[15] = -0.5900435899266435f * x * (xx - 3.0f * yy);
}

// The sums over a wave of 16 values per lane with 17 exchanges instead of 16 x 6: a butterfly that halves what a lane holds at each of the first
// four steps -- the lane whose bit `o` is clear keeps the lower half of its values and hands the upper half to its partner, which keeps that half
// -- so after offsets 32, 16, 8, 4 a lane holds ONE component, k = lane >> 2, summed over the 16 lanes that share its two low bits; offsets 2 and
// 1 finish it.  Returns component lane >> 2 (in all four lanes of a quad).  A fixed tree: the same inputs give the same bits.
__device__ __forceinline__ double splat_wave_sum16(double (&v)[16], int lane) {
#pragma unroll
  for (int h = 8, o = 32; h >= 1; h >>= 1, o >>= 1) {
    const bool up = (lane & o) != 0;
#pragma unroll
    for (int j = 0; j < h; ++j) {
      const double keep = up ? v[h + j] : v[j], send = up ? v[j] : v[h + j];
      v[j] = keep + __shfl_xor(send, o, 64);
    }
  }
  v[0] += __shfl_xor(v[0], 2, 64);
  v[0] += __shfl_xor(v[0], 1, 64);
  return v[0];
}

// SEP: also d thermal-opacity logit (g_opac_th) from v_lnop_th = d ln(thermal opacity); in antialiased mode the compensation takes both
// Pose (one SplatPoseBwdK, or nothing -- then the kernel is the one it was): the camera comes from the device record, and every Gaussian with
// radii > 0 also contributes to dL/d view' [3,4] through the view-space point (gpx, gpy, gpz, frustum-clamp branches included), T = J W and the
// projection rows xys reads.  The 12 numbers are summed per wave (splat_wave_sum16) and per block (LDS) in double and leave as ONE partial per block; no atomics.
// Depth (one SplatDepthProjK, or nothing -- then the kernel is the one it was): depths[i] is the view-space z of the mean, so v_depths[i] = dL / d
// depths[i] adds v_depths[i] view[2, :3] to d mean, and in the pose instantiation v_depths[i] (mean, 1) to row 2 of dL/d view' before the sums above.
struct SplatDepthProjK {
  const float* v_depths;  // [N]
};
template <bool SEP, typename... Pose>
__global__ void __launch_bounds__(256) k_splat_project_bwd(SplatCamK cam, const float* __restrict__ means, const float* __restrict__ log_scales,
                                                           const float* __restrict__ quats, const float* __restrict__ opac_logit,
                                                           const float* __restrict__ f_dc, const float* __restrict__ f_rest, const float* __restrict__ t_dc,
                                                           const float* __restrict__ t_rest, int64_t N, int sh_degree, int rest_coeffs, int antialiased,
                                                           const int32_t* __restrict__ radii, const float* __restrict__ v_xys,
                                                           const float* __restrict__ v_conics, const float* __restrict__ v_colors,
                                                           const float* __restrict__ v_lnop, float* __restrict__ g_means, float* __restrict__ g_scales,
                                                           float* __restrict__ g_quats, float* __restrict__ g_opac, float* __restrict__ g_fdc,
                                                           float* __restrict__ g_frest, float* __restrict__ g_tdc, float* __restrict__ g_trest,
                                                           const float* __restrict__ opac_th_logit, const float* __restrict__ v_lnop_th,
                                                           float* __restrict__ g_opac_th, Pose... pose_arg) {
  constexpr bool POSE = pack_has<SplatPoseBwdK, Pose...>, DEPTH = pack_has<SplatDepthProjK, Pose...>;
  static_assert(sizeof...(Pose) == (POSE ? 1 : 0) + (DEPTH ? 1 : 0), "the pack takes one SplatPoseBwdK, one SplatDepthProjK, or both");
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  [[maybe_unused]] const bool live = i < N;  // (pose: the tail's threads stay for the block's reduction)
  [[maybe_unused]] float dV[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  [[maybe_unused]] float proj_x = 0.f, proj_y = 0.f;
  if constexpr (POSE) {
    const float* rec = pack_get<SplatPoseBwdK>(pose_arg...).rec;
    splat_pose_load(cam, rec);
    proj_x = rec[31]; proj_y = rec[32];
  } else {
    if (i >= N) return;
  }
  float gm[3] = {0.f, 0.f, 0.f}, gs[3] = {0.f, 0.f, 0.f}, gq[4] = {0.f, 0.f, 0.f, 0.f}, gop = 0.f, gop_t = 0.f;
  float gcol[4] = {0.f, 0.f, 0.f, 0.f};  // d (colour before the clamp / sigmoid argument), per channel
  float basis[16];
  int nb = 0;
  bool visible;
  if constexpr (POSE) visible = live && radii[i] > 0;
  else visible = radii[i] > 0;
  if (visible) {  // Gaussians the forward culled get no gradient
    const float mx = means[3 * i], my = means[3 * i + 1], mz = means[3 * i + 2];
    const float* V = cam.view;
    const float px = V[0] * mx + V[1] * my + V[2] * mz + V[3];
    const float py = V[4] * mx + V[5] * my + V[6] * mz + V[7];
    const float pz = V[8] * mx + V[9] * my + V[10] * mz + V[11];
    const float q0w = quats[4 * i], q0x = quats[4 * i + 1], q0y = quats[4 * i + 2], q0z = quats[4 * i + 3];
    const float qn = 1.0f / sqrtf(q0w * q0w + q0x * q0x + q0y * q0y + q0z * q0z);
    const float qw = q0w * qn, qx = q0x * qn, qy = q0y * qn, qz = q0z * qn;
    const float R[9] = {1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - qw * qz), 2.f * (qx * qz + qw * qy),
                        2.f * (qx * qy + qw * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - qw * qx),
                        2.f * (qx * qz - qw * qy), 2.f * (qy * qz + qw * qx), 1.f - 2.f * (qx * qx + qy * qy)};
    const float s[3] = {expf(log_scales[3 * i]), expf(log_scales[3 * i + 1]), expf(log_scales[3 * i + 2])};
    float M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) M[3 * r + c] = R[3 * r + c] * s[c];
    float S[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) S[3 * r + c] = M[3 * r] * M[3 * c] + M[3 * r + 1] * M[3 * c + 1] + M[3 * r + 2] * M[3 * c + 2];
    const float tan_x = 0.5f * (float)cam.W / cam.fx, tan_y = 0.5f * (float)cam.H / cam.fy;
    const float lx = 1.3f * tan_x, ly = 1.3f * tan_y;
    const float ux = px / pz, uy = py / pz;
    const bool in_x = ux >= -lx && ux <= lx, in_y = uy >= -ly && uy <= ly;
    const float tx = pz * fminf(lx, fmaxf(-lx, ux));
    const float ty = pz * fminf(ly, fmaxf(-ly, uy));
    const float rz = 1.0f / pz, rz2 = rz * rz;
    const float J0[3] = {cam.fx * rz, 0.f, -cam.fx * tx * rz2};
    const float J1[3] = {0.f, cam.fy * rz, -cam.fy * ty * rz2};
    float T0[3], T1[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      T0[c] = J0[0] * V[c] + J0[1] * V[4 + c] + J0[2] * V[8 + c];
      T1[c] = J1[0] * V[c] + J1[1] * V[4 + c] + J1[2] * V[8 + c];
    }
    float ST0[3], ST1[3];  // Sigma T0^T, Sigma T1^T (Sigma is symmetric)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      ST0[r] = S[3 * r] * T0[0] + S[3 * r + 1] * T0[1] + S[3 * r + 2] * T0[2];
      ST1[r] = S[3 * r] * T1[0] + S[3 * r + 1] * T1[1] + S[3 * r + 2] * T1[2];
    }
    const float c00 = T0[0] * ST0[0] + T0[1] * ST0[1] + T0[2] * ST0[2];
    const float c01 = T0[0] * ST1[0] + T0[1] * ST1[1] + T0[2] * ST1[2];
    const float c11 = T1[0] * ST1[0] + T1[1] * ST1[1] + T1[2] * ST1[2];
    const float a = c00 + 0.3f, b = c01, c = c11 + 0.3f;
    const float det = a * c - b * b, det_orig = c00 * c11 - c01 * c01;
    // conic = (c, -b, a) / det
    const float vcx = v_conics[3 * i], vcy = v_conics[3 * i + 1], vcz = v_conics[3 * i + 2];
    const float id = 1.0f / det, id2 = id * id;
    float va = -vcx * c * c * id2 + vcy * b * c * id2 + vcz * (id - a * c * id2);
    float vb = vcx * 2.f * b * c * id2 + vcy * (-id - 2.f * b * b * id2) + vcz * 2.f * a * b * id2;
    float vc = vcx * (id - a * c * id2) + vcy * a * b * id2 - vcz * a * a * id2;
    const float dl = v_lnop[i];
    float dl_t = 0.f;
    if (SEP) dl_t = v_lnop_th[i];
    const float dl_c = SEP ? dl + dl_t : dl;  // both compensated opacities carry the compensation
    if (antialiased && det_orig > 0.f) {  // ln compensation = (ln det_orig - ln det) / 2
      const float io = 1.0f / det_orig;
      va += 0.5f * dl_c * (c11 * io - c * id);
      vb += 0.5f * dl_c * (-2.f * c01 * io + 2.f * b * id);
      vc += 0.5f * dl_c * (c00 * io - a * id);
    }
    // opacity = sigmoid(logit): d ln(sigmoid) / d logit = sigmoid(-logit)
    gop = dl / (1.0f + expf(opac_logit[i]));
    if (SEP) gop_t = dl_t / (1.0f + expf(opac_th_logit[i]));
    // cov2d = T Sigma T^T, T = J W
    float gT0[3], gT1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      gT0[r] = 2.f * va * ST0[r] + vb * ST1[r];
      gT1[r] = 2.f * vc * ST1[r] + vb * ST0[r];
    }
    float G[9];  // d Sigma, entries taken independently
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) G[3 * r + cc] = va * T0[r] * T0[cc] + vb * T0[r] * T1[cc] + vc * T1[r] * T1[cc];
    float gJ0[3], gJ1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      gJ0[r] = gT0[0] * V[4 * r] + gT0[1] * V[4 * r + 1] + gT0[2] * V[4 * r + 2];
      gJ1[r] = gT1[0] * V[4 * r] + gT1[1] * V[4 * r + 1] + gT1[2] * V[4 * r + 2];
    }
    float g_rz = cam.fx * gJ0[0] + cam.fy * gJ1[1];
    const float g_rz2 = -cam.fx * tx * gJ0[2] - cam.fy * ty * gJ1[2];
    const float g_tx = -cam.fx * rz2 * gJ0[2], g_ty = -cam.fy * rz2 * gJ1[2];
    g_rz += 2.f * rz * g_rz2;
    float gpx = 0.f, gpy = 0.f, gpz = -rz * rz * g_rz;
    // tx = pz clamp(px / pz): inside the clamp d tx = d px; clamped, tx = +-lim pz
    if (in_x) gpx += g_tx; else gpz += g_tx * (ux > 0.f ? lx : -lx);
    if (in_y) gpy += g_ty; else gpz += g_ty * (uy > 0.f ? ly : -ly);
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) gm[cc] = V[cc] * gpx + V[4 + cc] * gpy + V[8 + cc] * gpz;
    // xys = 0.5 W hx / (hw + 1e-6) + cx - 0.5, ...
    const float* P = cam.proj;
    const float hx = P[0] * mx + P[1] * my + P[2] * mz + P[3];
    const float hy = P[4] * mx + P[5] * my + P[6] * mz + P[7];
    const float hw = P[12] * mx + P[13] * my + P[14] * mz + P[15];
    const float rw = 1.0f / (hw + 1e-6f);
    const float vx = v_xys[2 * i], vy = v_xys[2 * i + 1];
    const float g_hx = vx * 0.5f * (float)cam.W * rw, g_hy = vy * 0.5f * (float)cam.H * rw;
    const float g_hw = -(vx * 0.5f * (float)cam.W * hx + vy * 0.5f * (float)cam.H * hy) * rw * rw;
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) gm[cc] += P[cc] * g_hx + P[4 + cc] * g_hy + P[12 + cc] * g_hw;
    [[maybe_unused]] float vz = 0.f;
    if constexpr (DEPTH) {  // depths = view[2] . (mean, 1)
      vz = pack_get<SplatDepthProjK>(pose_arg...).v_depths[i];
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) gm[cc] += V[8 + cc] * vz;
    }
    if constexpr (POSE) {
      const float mh[4] = {mx, my, mz, 1.0f};
      const float ax = proj_x * g_hx, ay = proj_y * g_hy;  // proj row 0 = proj_x view'[0], row 1 = proj_y view'[1], row 3 = view'[2]
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        dV[cc] = gpx * mh[cc] + ax * mh[cc];
        dV[4 + cc] = gpy * mh[cc] + ay * mh[cc];
        dV[8 + cc] = gpz * mh[cc] + g_hw * mh[cc];
      }
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {  // T = J W: T0 = J0[0] W[0] + J0[2] W[2], T1 = J1[1] W[1] + J1[2] W[2]
        dV[cc] += gT0[cc] * J0[0];
        dV[4 + cc] += gT1[cc] * J1[1];
        dV[8 + cc] += gT0[cc] * J0[2] + gT1[cc] * J1[2];
      }
      if constexpr (DEPTH) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) dV[8 + cc] += vz * mh[cc];
      }
    }
    // Sigma = M M^T, M = R diag(s): d M = (G + G^T) M
    float gR[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        float gM = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) gM += (G[3 * r + k] + G[3 * k + r]) * M[3 * k + cc];
        gs[cc] += gM * R[3 * r + cc];
        gR[3 * r + cc] = gM * s[cc];
      }
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) gs[cc] *= s[cc];  // d log-scale
    // rotation matrix of the normalised quaternion
    const float dw = 2.f * (-qz * gR[1] + qy * gR[2] + qz * gR[3] - qx * gR[5] - qy * gR[6] + qx * gR[7]);
    const float dx = 2.f * (qy * gR[1] + qz * gR[2] + qy * gR[3] - 2.f * qx * gR[4] - qw * gR[5] + qz * gR[6] + qw * gR[7] - 2.f * qx * gR[8]);
    const float dy = 2.f * (-2.f * qy * gR[0] + qx * gR[1] + qw * gR[2] + qx * gR[3] + qz * gR[5] - qw * gR[6] + qz * gR[7] - 2.f * qy * gR[8]);
    const float dz = 2.f * (-2.f * qz * gR[0] - qw * gR[1] + qx * gR[2] + qw * gR[3] - 2.f * qz * gR[4] + qy * gR[5] + qx * gR[6] + qy * gR[7]);
    const float dot = qw * dw + qx * dx + qy * dy + qz * dz;
    gq[0] = (dw - qw * dot) * qn; gq[1] = (dx - qx * dot) * qn; gq[2] = (dy - qy * dot) * qn; gq[3] = (dz - qz * dot) * qn;
    // colour: clamp(SH + 0.5, min 0) (view directions carry no gradient), or sigmoid of the DC term
    const float* vcol = v_colors + 4 * i;
    if (sh_degree >= 0) {
      float ddx = mx - cam.pos[0], ddy = my - cam.pos[1], ddz = mz - cam.pos[2];
      const float dn = 1.0f / sqrtf(ddx * ddx + ddy * ddy + ddz * ddz);
      ddx *= dn; ddy *= dn; ddz *= dn;
      const float* rest = f_rest + i * rest_coeffs * 3;
      const float* trest = t_rest + i * rest_coeffs;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) gcol[ch] = sh_eval(sh_degree, ddx, ddy, ddz, f_dc + 3 * i, rest, 3, ch) + 0.5f >= 0.0f ? vcol[ch] : 0.f;
      gcol[3] = sh_eval(sh_degree, ddx, ddy, ddz, t_dc + i, trest, 1, 0) + 0.5f >= 0.0f ? vcol[3] : 0.f;
      nb = (sh_degree + 1) * (sh_degree + 1);
      sh_basis(sh_degree, ddx, ddy, ddz, basis);
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float sg = 1.0f / (1.0f + expf(-f_dc[3 * i + ch]));
        gcol[ch] = vcol[ch] * sg * (1.0f - sg);
      }
      const float sg = 1.0f / (1.0f + expf(-t_dc[i]));
      gcol[3] = vcol[3] * sg * (1.0f - sg);
    }
  }
  if constexpr (POSE) {
    __shared__ double s_part[4][12];  // blockDim.x == 256: four waves
    const int lane = tn_lane(), wv = threadIdx.x >> 6;
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = k < 12 ? (double)dV[k] : 0.0;
    const double w = splat_wave_sum16(v, lane);
    if ((lane & 3) == 0 && lane < 48) s_part[wv][lane >> 2] = w;
    __syncthreads();
    if (threadIdx.x < 12)
      pack_get<SplatPoseBwdK>(pose_arg...).partial[(int64_t)blockIdx.x * 12 + threadIdx.x] =
          ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) + s_part[3][threadIdx.x];
    if (!live) return;
  }
#pragma unroll
  for (int cc = 0; cc < 3; ++cc) { g_means[3 * i + cc] = gm[cc]; g_scales[3 * i + cc] = gs[cc]; }
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) g_quats[4 * i + cc] = gq[cc];
  g_opac[i] = gop;
  if (SEP) g_opac_th[i] = gop_t;
  const float b0 = nb > 0 ? basis[0] : 1.0f;  // sigmoid path: the DC gradient is gcol itself
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) g_fdc[3 * i + ch] = b0 * gcol[ch];
  g_tdc[i] = b0 * gcol[3];
  for (int k = 1; k <= rest_coeffs; ++k) {
    const float bk = k < nb ? basis[k] : 0.f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) g_frest[(i * rest_coeffs + (k - 1)) * 3 + ch] = bk * gcol[ch];
    g_trest[i * rest_coeffs + (k - 1)] = bk * gcol[3];
  }
}

// ------------------------------------------------------------------------------------------------ pose refinement
// sum of the terms c_k x_k (+ add) whose coefficient c_k (add) is not zero, first term first: with the coefficients of an identity transform the
// result IS the one x_k (or add) that remains, bit for bit -- no 1 * x + 0 * y + 0 * z, whose zero products can still flip the sign of a zero.
__device__ __forceinline__ float pose_dot_skip0(float c0, float x0, float c1, float x1, float c2, float x2, float add) {
  float acc = 0.0f;
  bool have = false;
  const float c[3] = {c0, c1, c2}, x[3] = {x0, x1, x2};
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (c[k] != 0.0f) {
      const float t = c[k] * x[k];
      acc = have ? acc + t : t;
      have = true;
    }
  if (add != 0.0f) acc = have ? acc + add : add;
  return acc;
}

// The corrected camera of one frame: cam = the frame's camera as the host built it (view V0, position), pose = the frame's row (t, w) on the
// device -> rec (layout above SplatPoseK).  One thread; A(p) = [R | t] = pose_exp.  D = F A^-1 F = [D_R | D_t], D_R[i][j] = f_i f_j R[j][i],
// D_t[i] = -f_i sum_j R[j][i] t[j]; view' = [D_R R0 | D_R T0 + D_t]; position' = c2w' [:3, 3] = Rc t + position with Rc[i][j] = f_j R0[j][i].
// With a zero row D is exactly the identity and every number written equals the host struct's (its projmat rows being single products too).
__global__ void k_splat_pose_camera(SplatCamK cam, float proj_x, float proj_y, const float* __restrict__ pose, float* __restrict__ rec) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const Pose a = pose_exp(pose);
  const float f[3] = {1.0f, -1.0f, -1.0f};
  float DR[9], Dt[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) DR[3 * i + j] = f[i] * f[j] * a.R[3 * j + i];
    Dt[i] = -f[i] * pose_dot_skip0(a.t[0], a.R[i], a.t[1], a.R[3 + i], a.t[2], a.R[6 + i], 0.0f);
  }
  const float* V0 = cam.view;
  float V[12];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      V[4 * i + j] = pose_dot_skip0(DR[3 * i], V0[j], DR[3 * i + 1], V0[4 + j], DR[3 * i + 2], V0[8 + j], j == 3 ? Dt[i] : 0.0f);
#pragma unroll
  for (int j = 0; j < 12; ++j) rec[j] = V[j];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rec[12 + j] = proj_x * V[j];
    rec[16 + j] = proj_y * V[4 + j];
    rec[20 + j] = 0.0f;
    rec[24 + j] = V[8 + j];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
    rec[28 + i] = pose_dot_skip0(a.t[0], f[0] * V0[i], a.t[1], f[1] * V0[4 + i], a.t[2], f[2] * V0[8 + i], cam.pos[i]);
  rec[31] = proj_x; rec[32] = proj_y;
#pragma unroll
  for (int j = 33; j < SPLAT_POSE_REC; ++j) rec[j] = 0.0f;
}

// Ends the pose backward: one block.  12 components x SPLAT_POSE_SEGS segments of consecutive blocks are folded in block order, the segment sums in
// segment order (double; the association depends on the block count alone), then thread 0 chains dL/d view' -> dL/dD -> dL/d(t, w):
//   dD_R = dV'_R R0^T + dV'_t T0^T, dD_t = dV'_t;  G = dL/dR: G[j][i] = f_i f_j dD_R[i][j] - f_i dD_t[i] t[j];  dL/dt[j] = -sum_i f_i dD_t[i] R[j][i];
//   dL/dw = pose_exp_bwd(w, G), the derivative the ray path uses.  The result is ADDED to grad_row[6]; dview_out [12] (optional) gets dL/d view'.
#define SPLAT_POSE_SEGS 16
__global__ void __launch_bounds__(12 * SPLAT_POSE_SEGS) k_splat_pose_finish(SplatCamK cam, const float* __restrict__ pose, const double* __restrict__ partial,
                                                                            int nblk, float* __restrict__ grad_row, float* __restrict__ dview_out) {
  __shared__ double s_seg[SPLAT_POSE_SEGS][12];
  __shared__ double s_dv[12];
  const int k = threadIdx.x % 12, seg = threadIdx.x / 12;
  const int per = (nblk + SPLAT_POSE_SEGS - 1) / SPLAT_POSE_SEGS;
  const int b0 = seg * per, b1 = min(nblk, b0 + per);
  double acc = 0.0;
  for (int b = b0; b < b1; ++b) acc += partial[(int64_t)b * 12 + k];
  s_seg[seg][k] = acc;
  __syncthreads();
  if (threadIdx.x < 12) {
    double t = 0.0;
    for (int q = 0; q < SPLAT_POSE_SEGS; ++q) t += s_seg[q][threadIdx.x];
    s_dv[threadIdx.x] = t;
    if (dview_out != nullptr) dview_out[threadIdx.x] = (float)t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const Pose a = pose_exp(pose);
  const double f[3] = {1.0, -1.0, -1.0};
  const float* V0 = cam.view;
  float G[9];
  double dt[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double dDt = s_dv[4 * i + 3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double dDR = ((s_dv[4 * i] * (double)V0[4 * j] + s_dv[4 * i + 1] * (double)V0[4 * j + 1]) + s_dv[4 * i + 2] * (double)V0[4 * j + 2]) +
                         dDt * (double)V0[4 * j + 3];
      G[3 * j + i] = (float)(f[i] * f[j] * dDR - f[i] * dDt * (double)a.t[j]);
      dt[j] -= f[i] * dDt * (double)a.R[3 * j + i];
    }
  }
  const float w[3] = {pose[3], pose[4], pose[5]};
  float dw[3];
  pose_exp_bwd(w, pose_exp_factors(w), G, dw);
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    grad_row[m] += (float)dt[m];
    grad_row[3 + m] += dw[m];
  }
}

// ------------------------------------------------------------------------------------------------ entry points
static int check_cam(const TnSplatCamera* cam, const char* who) {
  TN_REQUIRE(cam != nullptr, "%s: null camera", who);
  TN_REQUIRE(cam->width >= 1 && cam->height >= 1 && cam->width <= 16384 && cam->height <= 16384, "%s: bad image size %dx%d", who, cam->width, cam->height);
  TN_REQUIRE(cam->fx > 0.f && cam->fy > 0.f, "%s: bad focal length", who);
  return TN_OK;
}
static SplatCamK make_camk(const TnSplatCamera* cam) {
  SplatCamK k;
  for (int i = 0; i < 12; ++i) k.view[i] = cam->viewmat[i];
  for (int i = 0; i < 16; ++i) k.proj[i] = cam->projmat[i];
  k.fx = cam->fx; k.fy = cam->fy; k.cx = cam->cx; k.cy = cam->cy; k.clip = cam->clip_thresh;
  for (int i = 0; i < 3; ++i) k.pos[i] = cam->position[i];
  k.W = cam->width; k.H = cam->height;
  k.tbx = (cam->width + SPLAT_BLOCK - 1) / SPLAT_BLOCK;
  k.tby = (cam->height + SPLAT_BLOCK - 1) / SPLAT_BLOCK;
  return k;
}

// Optional inputs are groups of nullable pointers, and which groups a call gives picks the kernel instantiation.  with_flags turns the runtime
// flags into std::bool_constant arguments of `f`, in order, so every stage below writes its launch once; opt_args is the trailing kernel
// arguments a flag adds (a tuple, empty when the flag is off), and group_state tells a group given whole (1) from an absent (0) or a partly
// given (-1) one.
template <typename F>
static void with_flags(F&& f) { f(); }
template <typename F, typename... B>
static void with_flags(F&& f, bool flag, B... rest) {
  if (flag) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
template <bool ON, typename... T>
static auto opt_args(std::bool_constant<ON>, T... t) {
  if constexpr (ON) return std::make_tuple(t...);
  else return std::tuple<>();
}
template <typename... P>
static int group_state(P... p) {
  const int n = (int(p != nullptr) + ...);
  return n == 0 ? 0 : n == (int)sizeof...(P) ? 1 : -1;
}

// opacities_thermal (separate thermal opacity), crop (a HOST box) and pose_camera (tn_splat_pose_camera's device record, from which the kernel
// then reads its camera) are each optional on their own: SEP x CROP x POSE instantiations of one kernel.
extern "C" int tn_splat_project(const TnSplatCamera* camera, const float* pose_camera, const float* means, const float* log_scales, const float* quats,
                                const float* opacities, const float* features_dc, const float* features_rest, const float* thermal_dc,
                                const float* thermal_rest, const float* opacities_thermal, int64_t num_gaussians, int32_t num_rest_coeffs,
                                int32_t sh_degree, int32_t antialiased, float* xys, float* depths, int32_t* radii, float* conics, float* compensation,
                                int32_t* num_tiles_hit, int32_t* tile_box, void* workspace, int64_t max_intersections, const TnSplatCrop* crop,
                                tn_stream_t stream) {
  const char* who = "tn_splat_project";
  const bool sep = opacities_thermal != nullptr;
  int rc = check_cam(camera, who);
  if (rc) return rc;
  if (num_gaussians == 0) return TN_OK;
  TN_REQUIRE(means && log_scales && quats && opacities && features_dc && thermal_dc && xys && depths && radii && conics && compensation &&
                 num_tiles_hit && tile_box && workspace,
             "%s: null pointer", who);
  TN_REQUIRE(num_gaussians > 0 && num_gaussians < (1ll << 31), "%s: bad Gaussian count", who);
  TN_REQUIRE(max_intersections >= 0 || !sep, "%s: bad workspace capacity", who);
  TN_REQUIRE(sh_degree >= -1 && sh_degree <= 3, "%s: sh_degree %d unsupported (-1 = sigmoid of the DC term, 0..3)", who, sh_degree);
  TN_REQUIRE(num_rest_coeffs >= (sh_degree < 1 ? 0 : (sh_degree + 1) * (sh_degree + 1) - 1), "%s: %d higher-order coefficients for degree %d", who,
             num_rest_coeffs, sh_degree);
  TN_REQUIRE(num_rest_coeffs == 0 || (features_rest && thermal_rest), "%s: null SH coefficients", who);
  SplatCamK k = make_camk(camera);
  SplatWs ws = splat_layout(workspace, num_gaussians, max_intersections, k.tbx * k.tby, nullptr);
  const int PB = 128;  // Gaussians per block: 30 KB of LDS at degree 3 -> 5 blocks per CU (256 per block = 61 KB = 2 blocks: 136 vs 1xx us)
  const size_t lds = (size_t)PB * num_rest_coeffs * 4 * sizeof(float);
  TN_REQUIRE(lds <= (crop ? 65536 - 256 : 65536), "%s: %d higher-order coefficients do not fit the LDS staging", who, num_rest_coeffs);  // 256 B of static LDS: the words of __syncthreads_or
  const SplatCropK ck = crop ? make_cropk(crop) : SplatCropK{};
  with_flags([&](auto SEP, auto CROP, auto POSE) {
    std::apply([&](auto... extra) {
      hipLaunchKernelGGL((k_splat_project<decltype(SEP)::value, decltype(extra)...>), dim3((unsigned)tn_cdiv(num_gaussians, PB)), dim3(PB), lds, tn_s(stream), k,
                         means, log_scales, quats, opacities, features_dc, features_rest, thermal_dc, thermal_rest, num_gaussians, sh_degree, num_rest_coeffs,
                         antialiased, (float2*)xys, depths, radii, conics, compensation, num_tiles_hit, tile_box, ws.recs, ws.tbox, ws.thits, opacities_thermal,
                         extra...);
    }, std::tuple_cat(opt_args(CROP, ck), opt_args(POSE, SplatPoseK{pose_camera})));
  }, sep, crop != nullptr, pose_camera != nullptr);
  TN_CHECK_LAUNCH(who);
  return TN_OK;
}

// tn_splat_pose_camera: the frame's camera and one pose row (device) -> the corrected camera record (device), one launch, nothing read back.
extern "C" int tn_splat_pose_camera(const TnSplatCamera* camera, float proj_x, float proj_y, const float* pose_row, float* pose_camera, tn_stream_t stream) {
  int rc = check_cam(camera, "tn_splat_pose_camera");
  if (rc) return rc;
  TN_REQUIRE(pose_row && pose_camera, "tn_splat_pose_camera: null pointer");
  hipLaunchKernelGGL(k_splat_pose_camera, dim3(1), dim3(64), 0, tn_s(stream), make_camk(camera), proj_x, proj_y, pose_row, pose_camera);
  TN_CHECK_LAUNCH("tn_splat_pose_camera");
  return TN_OK;
}

__global__ void __launch_bounds__(256) k_splat_crop_mask(SplatCropK crop, const float* __restrict__ means, int64_t n, uint8_t* __restrict__ mask) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  mask[i] = splat_in_crop(crop, means[3 * i], means[3 * i + 1], means[3 * i + 2]) ? 1 : 0;
}

extern "C" int tn_splat_crop_mask(const TnSplatCrop* crop, const float* means, int64_t n, uint8_t* mask, tn_stream_t stream) {
  TN_REQUIRE(crop != nullptr, "tn_splat_crop_mask: null crop box");
  TN_REQUIRE(n >= 0 && n < (1ll << 31), "tn_splat_crop_mask: bad point count");
  if (n == 0) return TN_OK;
  TN_REQUIRE(means && mask, "tn_splat_crop_mask: null pointer");
  hipLaunchKernelGGL(k_splat_crop_mask, dim3((unsigned)tn_cdiv(n, 256)), dim3(256), 0, tn_s(stream), make_cropk(crop), means, n, mask);
  TN_CHECK_LAUNCH("tn_splat_crop_mask");
  return TN_OK;
}

extern "C" int tn_splat_bin(const TnSplatCamera* camera, const float* depths, int64_t num_gaussians, void* workspace, int64_t max_intersections,
                            int64_t* num_intersections_out, tn_stream_t stream) {
  int rc = check_cam(camera, "tn_splat_bin");
  if (rc) return rc;
  TN_REQUIRE(num_intersections_out != nullptr, "tn_splat_bin: null output");
  *num_intersections_out = 0;
  SplatCamK k = make_camk(camera);
  const int num_tiles = k.tbx * k.tby;
  TN_REQUIRE(workspace != nullptr, "tn_splat_bin: null workspace");
  SplatWs ws = splat_layout(workspace, num_gaussians, max_intersections, num_tiles, nullptr);
  hipStream_t st = tn_s(stream);
  if (hipMemsetAsync(ws.tile_bins, 0, 8 * (size_t)num_tiles, st) != hipSuccess || hipMemsetAsync(ws.depth_max, 0, 4, st) != hipSuccess) {
    tn_set_error("tn_splat_bin: memset failed");
    return TN_ELAUNCH;
  }
  // default tile order = identity (every run empty); replaced by longest-first once the runs are known
  hipLaunchKernelGGL(k_splat_tile_len, dim3((unsigned)tn_cdiv(num_tiles, 256)), dim3(256), 0, st, ws.tile_bins, num_tiles, ws.lkeys[1], ws.lvals[1]);
  TN_CHECK_LAUNCH("tn_splat_bin(order)");
  if (num_gaussians == 0) return TN_OK;
  TN_REQUIRE(depths != nullptr, "tn_splat_bin: null pointer");
  // depth order of the Gaussians (stable: equal depths keep their index order; culled Gaussians have depth 0 and no tiles)
  size_t tb = ws.tmp_bytes;
  if (rocprim::radix_sort_pairs(ws.tmp, tb, reinterpret_cast<const uint32_t*>(depths), ws.dkeys, rocprim::counting_iterator<int32_t>(0), ws.order,
                                (size_t)num_gaussians, 0, 32, st) != hipSuccess) {
    tn_set_error("tn_splat_bin: depth sort failed");
    return TN_ELAUNCH;
  }
  tb = ws.tmp_bytes;
  if (rocprim::inclusive_scan(ws.tmp, tb, rocprim::make_transform_iterator((const int32_t*)ws.order, HitsInOrder{ws.thits}), ws.cum,
                              (size_t)num_gaussians, rocprim::plus<int32_t>(), st) != hipSuccess) {
    tn_set_error("tn_splat_bin: scan failed");
    return TN_ELAUNCH;
  }
  // the number of (Gaussian, tile) pairs sizes the sort: one 4-byte read-back, as gsplat's own binning does (cum_tiles_hit[-1].item())
  int32_t total = 0;
  if (hipMemcpyAsync(&total, ws.cum + (num_gaussians - 1), 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    tn_set_error("tn_splat_bin: read-back of the intersection count failed");
    return TN_ELAUNCH;
  }
  *num_intersections_out = total;
  TN_REQUIRE(total >= 0, "tn_splat_bin: intersection count overflowed 2^31");
  if (total > max_intersections) {
    tn_set_error("tn_splat_bin: %d intersections exceed the workspace capacity %lld (call again with a larger workspace)", total, (long long)max_intersections);
    return TN_EINVAL;
  }
  if (total == 0) return TN_OK;
  hipLaunchKernelGGL(k_splat_intersect, dim3((unsigned)tn_cdiv(num_gaussians, 256)), dim3(256), 0, st, ws.order, ws.tbox, ws.cum, num_gaussians, k.tbx,
                     ws.keys[0], ws.vals[0], max_intersections);
  TN_CHECK_LAUNCH("tn_splat_bin(intersect)");
  int tile_bits = 1;
  while ((1 << tile_bits) < num_tiles) ++tile_bits;
  tb = ws.tmp_bytes;
  if (rocprim::radix_sort_pairs(ws.tmp, tb, ws.keys[0], ws.keys[1], ws.vals[0], ws.vals[1], (size_t)total, 0, tile_bits, st) != hipSuccess) {
    tn_set_error("tn_splat_bin: radix sort failed");
    return TN_ELAUNCH;
  }
  hipLaunchKernelGGL(k_splat_tile_edges, dim3((unsigned)tn_cdiv(total, 256)), dim3(256), 0, st, ws.keys[1], (int64_t)total, ws.tile_bins);
  TN_CHECK_LAUNCH("tn_splat_bin(edges)");
  hipLaunchKernelGGL(k_splat_tile_len, dim3((unsigned)tn_cdiv(num_tiles, 256)), dim3(256), 0, st, ws.tile_bins, num_tiles, ws.lkeys[0], ws.lvals[0]);
  TN_CHECK_LAUNCH("tn_splat_bin(lengths)");
  tb = ws.tmp_bytes;
  if (rocprim::radix_sort_pairs(ws.tmp, tb, ws.lkeys[0], ws.lkeys[1], ws.lvals[0], ws.lvals[1], (size_t)num_tiles, 0, 32, st) != hipSuccess) {
    tn_set_error("tn_splat_bin: tile order sort failed");
    return TN_ELAUNCH;
  }
  return TN_OK;
}

// The raster of both entry points below: AA x TRAIN x SEP (TRAIN = the caller wants the transmittance and last-contributor images, SEP = the
// thermal chain's outputs), then the depth normalisation.  `who` / `who_depth` name the entry point's two launches in error messages.
static int splat_raster(const char* who, const char* who_depth, const TnSplatCamera* camera, int64_t num_gaussians, void* workspace, int64_t max_intersections,
                        const float* background4, int32_t antialiased, float* out_rgbt, float* out_depth, float* out_alpha, float* out_T, int32_t* out_last,
                        float* out_alpha_th, float* out_T_th, int32_t* out_last_th, tn_stream_t stream) {
  SplatCamK k = make_camk(camera);
  SplatWs ws = splat_layout(workspace, num_gaussians, max_intersections, k.tbx * k.tby, nullptr);
  float4 bg = make_float4(background4[0], background4[1], background4[2], background4[3]);
  hipStream_t st = tn_s(stream);
  with_flags([&](auto AA, auto TRAIN, auto SEP) {
    std::apply([&](auto... sep_args) {
      hipLaunchKernelGGL((k_splat_raster<decltype(AA)::value, decltype(TRAIN)::value, decltype(SEP)::value, decltype(sep_args)...>), dim3(k.tbx * k.tby), dim3(256), 0,
                         st, ws.recs, ws.vals[1], ws.tile_bins, ws.lvals[1], k.W, k.H, k.tbx, bg, out_rgbt, out_depth, out_alpha, ws.depth_max, out_T, out_last,
                         sep_args...);
    }, opt_args(SEP, out_alpha_th, out_T_th, out_last_th));
  }, antialiased != 0, out_T != nullptr, out_alpha_th != nullptr);
  TN_CHECK_LAUNCH(who);
  int64_t n = (int64_t)k.W * k.H;
  hipLaunchKernelGGL(k_splat_depth_finalize, dim3((unsigned)tn_cdiv(n, 256)), dim3(256), 0, st, out_depth, out_alpha, ws.depth_max, n);
  TN_CHECK_LAUNCH(who_depth);
  return TN_OK;
}

// the short form: three images, shared opacity
extern "C" int tn_splat_raster(const TnSplatCamera* camera, int64_t num_gaussians, void* workspace, int64_t max_intersections, const float* background4,
                               int32_t antialiased, float* out_rgbt, float* out_depth, float* out_alpha, tn_stream_t stream) {
  int rc = check_cam(camera, "tn_splat_raster");
  if (rc) return rc;
  TN_REQUIRE(workspace && background4 && out_rgbt && out_depth && out_alpha, "tn_splat_raster: null pointer");
  return splat_raster("tn_splat_raster", "tn_splat_raster(depth)", camera, num_gaussians, workspace, max_intersections, background4, antialiased, out_rgbt, out_depth, out_alpha, nullptr,
                      nullptr, nullptr, nullptr, nullptr, stream);
}

// the raster with every optional output: {out_alpha_thermal} on a separate-opacity frame, {out_transmittance, out_last} for the backward, and
// the thermal chain's {out_transmittance_thermal, out_last_thermal}, which needs both of the others
extern "C" int tn_splat_raster_chains(const TnSplatCamera* camera, int64_t num_gaussians, void* workspace, int64_t max_intersections,
                                      const float* background4, int32_t antialiased, float* out_rgbt, float* out_depth, float* out_alpha,
                                      float* out_alpha_thermal, float* out_transmittance, int32_t* out_last, float* out_transmittance_thermal,
                                      int32_t* out_last_thermal, tn_stream_t stream) {
  const char* who = "tn_splat_raster_chains";
  int rc = check_cam(camera, who);
  if (rc) return rc;
  TN_REQUIRE(workspace && background4 && out_rgbt && out_depth && out_alpha, "%s: null pointer", who);
  TN_REQUIRE(num_gaussians >= 0 && max_intersections >= 0, "%s: bad sizes", who);
  const int train = group_state(out_transmittance, out_last), train_th = group_state(out_transmittance_thermal, out_last_thermal);
  TN_REQUIRE(train >= 0 && train_th >= 0, "%s: null pointer (a transmittance / last-contributor pair is partly given)", who);
  // (the TRAIN x SEP kernel writes both chains' pairs: the thermal pair goes with the other two groups, and only with them)
  TN_REQUIRE((train_th != 0) == (train && out_alpha_thermal), "%s: the thermal chain's transmittance and last contributor go with out_alpha_thermal and the RGB chain's pair",
             who);
  return splat_raster(who, "tn_splat_raster_chains(depth)", camera, num_gaussians, workspace, max_intersections, background4, antialiased, out_rgbt, out_depth, out_alpha,
                      out_transmittance, out_last, out_alpha_thermal, out_transmittance_thermal, out_last_thermal, stream);
}

extern "C" int tn_splat_raster_removal_sep(const TnSplatCamera* camera, int64_t num_gaussians, void* workspace, int64_t max_intersections,
                                           const float* background4, float min_opacity_diff, float* out_removal, tn_stream_t stream) {
  const char* who = "tn_splat_raster_removal_sep";
  int rc = check_cam(camera, who);
  if (rc) return rc;
  TN_REQUIRE(workspace && background4 && out_removal, "%s: null pointer", who);
  TN_REQUIRE(num_gaussians >= 0 && num_gaussians < (1ll << 31) && max_intersections >= 0, "%s: bad sizes", who);
  TN_REQUIRE(min_opacity_diff >= 0.f, "%s: min_opacity_diff %g must be a number >= 0", who, (double)min_opacity_diff);  // (false for NaN too)
  SplatCamK k = make_camk(camera);
  SplatWs ws = splat_layout(workspace, num_gaussians, max_intersections, k.tbx * k.tby, nullptr);
  float4 bg = make_float4(background4[0], background4[1], background4[2], background4[3]);
  hipLaunchKernelGGL(k_splat_raster_removal, dim3(k.tbx * k.tby), dim3(256), 0, tn_s(stream), ws.recs, ws.vals[1], ws.tile_bins, ws.lvals[1], k.W, k.H, k.tbx,
                     bg, min_opacity_diff, out_removal);
  TN_CHECK_LAUNCH(who);
  return TN_OK;
}

// The raster backward.  Optional groups: the thermal chain {transmittance_thermal, last_thermal, v_alpha_thermal, v_log_opacity_thermal} (SEP),
// {v_xys_abs} (ABS: v_xys_abs [N,2] = sum over pixels of |the pixel's term of v_xys|, per component) and the depth gradient {depth, v_depth,
// v_depths} (DEPTH; classic mode only: in antialiased mode the depth is blended by a chain of its own whose final transmittance and last
// contributor the training forward does not keep).  Every output a group does not add is bit-equal with and without it.
extern "C" int tn_splat_raster_backward(const TnSplatCamera* camera, int64_t num_gaussians, void* workspace, int64_t max_intersections,
                                        int64_t num_intersections, const float* background4, int32_t antialiased, const float* transmittance,
                                        const int32_t* last, const float* transmittance_thermal, const int32_t* last_thermal, const float* conics,
                                        const float* v_rgbt, const float* v_alpha, const float* v_alpha_thermal, void* bwd_workspace,
                                        int64_t bwd_workspace_bytes, float* v_xys, float* v_xys_abs, float* v_conics, float* v_colors,
                                        float* v_log_opacity, float* v_log_opacity_thermal, const float* depth, const float* v_depth, float* v_depths,
                                        tn_stream_t stream) {
  const char* who = "tn_splat_raster_backward";
  const int sep_group = group_state(transmittance_thermal, last_thermal, v_alpha_thermal, v_log_opacity_thermal), depth_group = group_state(depth, v_depth, v_depths);
  const bool sep = sep_group != 0, absgrad = v_xys_abs != nullptr, with_depth = depth_group != 0;
  TN_REQUIRE(!with_depth || antialiased == 0, "%s: the depth gradient exists in classic mode only (antialiased depth rides a chain of its own)", who);
  int rc = check_cam(camera, who);
  if (rc) return rc;
  TN_REQUIRE(num_gaussians >= 0 && num_gaussians < (1ll << 31), "%s: bad Gaussian count", who);
  TN_REQUIRE(max_intersections >= 0 && num_intersections >= 0 && num_intersections <= max_intersections, "%s: %lld intersections for a workspace of %lld", who,
             (long long)num_intersections, (long long)max_intersections);
  if (num_gaussians == 0) return TN_OK;
  TN_REQUIRE(sep_group >= 0, "%s: null pointer (the thermal chain's group transmittance_thermal, last_thermal, v_alpha_thermal, v_log_opacity_thermal is partly given)", who);
  TN_REQUIRE(depth_group >= 0, "%s: null pointer (the depth group depth, v_depth, v_depths is partly given)", who);
  TN_REQUIRE(workspace && background4 && transmittance && last && conics && v_rgbt && v_alpha && bwd_workspace && v_xys && v_conics && v_colors && v_log_opacity,
             "%s: null pointer", who);
  const int ng = splat_pair_grads(sep, absgrad, with_depth);
  const int64_t need = tn_splat_backward_workspace_bytes(num_gaussians, max_intersections, sep, absgrad, with_depth);
  TN_REQUIRE(bwd_workspace_bytes >= need, "%s: backward workspace of %lld bytes, %lld needed", who, (long long)bwd_workspace_bytes, (long long)need);
  SplatCamK k = make_camk(camera);
  const int num_tiles = k.tbx * k.tby;
  SplatWs ws = splat_layout(workspace, num_gaussians, max_intersections, num_tiles, nullptr);
  SplatBwdWs bw = splat_bwd_layout(bwd_workspace, num_gaussians, max_intersections, ng, nullptr);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_splat_run_start, dim3((unsigned)tn_cdiv(num_gaussians, 256)), dim3(256), 0, st, ws.order, ws.cum, ws.thits, num_gaussians, bw.start);
  TN_CHECK_LAUNCH(who);
  if (num_intersections > 0) {
    // pairs behind every pixel's last contributor are not visited: their records stay zero
    if (hipMemsetAsync(bw.pair, 0, sizeof(float) * ng * (size_t)num_intersections, st) != hipSuccess) {
      tn_set_error("%s: memset failed", who);
      return TN_ELAUNCH;
    }
    float4 bg = make_float4(background4[0], background4[1], background4[2], background4[3]);
    with_flags([&](auto SEP, auto ABS, auto DEPTH) {
      std::apply([&](auto... extra) {
        hipLaunchKernelGGL((k_splat_raster_bwd<decltype(SEP)::value, decltype(ABS)::value, decltype(extra)...>), dim3(num_tiles), dim3(256), 0, st, ws.recs, ws.vals[1],
                           ws.tile_bins, ws.lvals[1], k.W, k.H, k.tbx, bg, transmittance, last, v_rgbt, v_alpha, bw.start, ws.tbox, bw.pair, extra...);
      }, std::tuple_cat(opt_args(SEP, transmittance_thermal, last_thermal, v_alpha_thermal), opt_args(DEPTH, SplatDepthBwdK{depth, v_depth})));
    }, sep, absgrad, with_depth);
    TN_CHECK_LAUNCH(who);
  }
  with_flags([&](auto SEP, auto ABS, auto DEPTH) {
    constexpr int NG = (decltype(SEP)::value ? SPLAT_PAIR_GRADS_SEP : SPLAT_PAIR_GRADS) + (decltype(DEPTH)::value ? SPLAT_PAIR_DEPTH : 0) +
                       (decltype(ABS)::value ? SPLAT_PAIR_ABS : 0);
    std::apply([&](auto... extra) {
      hipLaunchKernelGGL((k_splat_pair_fold<NG, decltype(extra)...>), dim3((unsigned)tn_cdiv(num_gaussians, 256)), dim3(256), 0, st, bw.pair, bw.start, ws.thits, conics,
                         num_gaussians, v_xys, v_conics, v_colors, v_log_opacity, v_log_opacity_thermal, extra...);
    }, std::tuple_cat(opt_args(ABS, v_xys_abs), opt_args(DEPTH, SplatDepthFoldK{v_depths})));
  }, sep, absgrad, with_depth);
  TN_CHECK_LAUNCH(who);
  return TN_OK;
}

// ------------------------------------------------------------------------------------------------ ray contribution (splat_prune.py)
// What every Gaussian contributes to a frame's rays: for each pixel p and each list entry g the forward blends on one transmittance chain,
// w = pixel_weight[p] alpha T -- the weight the forward multiplies g's colour with.  Per Gaussian: the largest w (RadSplat's importance), the sum
// (LightGaussian's hit-weighted score), the number of pixels with w > 0 and whether the frame saw it at all, accumulated over frames in place.
//   k_splat_raster_contrib  the forward's walk (block = tile, wave = 8x8 quadrant, ballot culling, pipelined record fetch, the splat_* rules) on ONE
//                           chain, reducing per Gaussian instead of per pixel: (sum, max, count) over the wave's 64 lanes by a fixed butterfly
//                           (the count is a popcount of the ballot), parked per wave in LDS, the four waves combined in order, ONE record written to
//                           the pair's slot -- addressed as k_splat_raster_bwd addresses it.  EVERY slot of the tile's list is written: zeros for the
//                           Gaussians a wave's ballot skipped and for everything behind the batch at which all 256 pixels are done (the forward's
//                           `break`), so the fold never reads what nobody wrote and nothing is cleared beforehand.
//   k_splat_contrib_fold    thread = Gaussian: walks its run in list order and updates the four accumulators.
// No atomics: the same inputs give the same bits.  A Gaussian at which a pixel stops (nT <= 1e-4) is not blended there and scores nothing there.
// chain 0: SplatRec::b.y, the opacity RGB, accumulation and (classic) depth blend with; chain 1: SplatRec::d.w, the thermal chain of separate mode.
// Both are the compensated opacity in antialiased mode -- what the chain's COLOUR is blended with, not the depth pass's plain one.
// Static LDS: 8 KB of records + 1 KB of opacities + 12 KB of partial results.
#define SPLAT_PAIR_CONTRIB 3  // per pair: sum of w over the tile's pixels, max of w, pixels with w > 0 (<= 256: exact in a float)
__global__ void __launch_bounds__(256) k_splat_raster_contrib(const SplatRec* __restrict__ recs, const int32_t* __restrict__ sorted_ids,
                                                              const int32_t* __restrict__ tile_bins, const int32_t* __restrict__ tile_order, int W, int H,
                                                              int tbx, int chain, const float* __restrict__ pixel_weight, const int32_t* __restrict__ start,
                                                              const int32_t* __restrict__ tbox, float* __restrict__ pair) {
  __shared__ float4 sa[SPLAT_BATCH], sb[SPLAT_BATCH];
  __shared__ float sl[SPLAT_BATCH];                          // l2op of the chain
  __shared__ float sp[4][SPLAT_PAIR_CONTRIB][SPLAT_BATCH];  // per wave (sum, max, count) of the batch's Gaussians
  const int tile = tile_order[blockIdx.x];
  const int tile_x = tile % tbx, tile_y = tile / tbx;
  int lane, wv, ix, iy;
  float pxf, pyf, qcx, qcy;
  const bool inside = splat_lane_pixel(tile_x, tile_y, W, H, lane, wv, ix, iy, pxf, pyf, qcx, qcy);
  const int begin = tile_bins[2 * tile], end = tile_bins[2 * tile + 1];
  const float pw = inside ? (pixel_weight ? pixel_weight[(int64_t)iy * W + ix] : 1.0f) : 0.0f;
  float T = 1.0f;
  bool done = !inside;
  // software pipeline, as the forward's: batch i+1's records (and the slots of their pair records) are fetched while batch i is walked
  float4 ra, rb;
  float rl = 0.f;
  int64_t ndst = -1;
  ra = rb = make_float4(0.f, 0.f, 0.f, 0.f);
  auto fetch = [&](int idx) {
    ndst = -1;
    if (idx < end) {
      const int g = sorted_ids[idx];
      const SplatRec* r = recs + g;
      ra = r->a; rb = r->b;
      rl = chain ? r->d.w : r->b.y;
      const int4 bx = reinterpret_cast<const int4*>(tbox)[g];
      ndst = (int64_t)start[g] + (tile_y - bx.y) * (bx.z - bx.x) + (tile_x - bx.x);
    }
  };
  fetch(begin + (int)threadIdx.x);
  for (int base = begin; base < end; base += SPLAT_BATCH) {
    // all 256 pixels finished (where the forward leaves the tile): the rest of the list scores nothing, its records are zeros.  The barrier also
    // says that the previous batch's records and partial results are consumed.
    const bool fin = __syncthreads_count(done ? 1 : 0) == 256;
    const int64_t dst = ndst;
    if (!fin) {
      sa[threadIdx.x] = ra; sb[threadIdx.x] = rb; sl[threadIdx.x] = rl;
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int c = 0; c < SPLAT_PAIR_CONTRIB; ++c) sp[w][c][threadIdx.x] = 0.f;
    }
    fetch(base + SPLAT_BATCH + (int)threadIdx.x);
    if (fin) {  // (block-uniform)
      if (dst >= 0) {
        float* o = pair + dst * SPLAT_PAIR_CONTRIB;
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
      }
      continue;
    }
    __syncthreads();
    const int n = min(SPLAT_BATCH, end - base);
    if (!__all(done ? 1 : 0)) {  // a wave whose 64 pixels are done leaves its zeros
#pragma unroll 1
      for (int q = 0; q < SPLAT_BATCH / 64; ++q) {
        if (q * 64 >= n) break;
        const int kk = q * 64 + lane;
        bool keep = false;
        if (kk < n) {
          float4 a = sa[kk], b = sb[kk];
          keep = splat_axis_hit(a.x, b.z, qcx) && splat_axis_hit(a.y, b.w, qcy);
        }
        uint64_t live = __ballot(keep);
        while (live) {
          const int k = q * 64 + __builtin_ctzll(live);
          live &= live - 1;
          const float4 a = sa[k], b = sb[k];
          const float l2op = sl[k];
          const float dx = a.x - pxf, dy = a.y - pyf;
          const float power = splat_power(a.z, a.w, b.x, dx, dy);
          // nobody in the wave can reach alpha >= 1/255 = 2^-7.994 on this chain (or the form is negative): the record stays zero
          if (!__any((power >= 0.f && l2op - power >= -8.0f) ? 1 : 0)) continue;
          float w = 0.f;
          if (power >= 0.f) {
            const float alpha = splat_alpha(splat_alpha_raw(l2op, power));
            if (!done && splat_visible(alpha)) {
              const float nT = fmaf(-alpha, T, T);
              if (nT <= 1e-4f) done = true;  // the pixel stops BEFORE this Gaussian: it scores nothing here
              else {
                w = pw * (alpha * T);
                T = nT;
              }
            }
          }
          const int cnt = __popcll(__ballot(w > 0.f));
          float s = w, m = w;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            s += __shfl_xor(s, o, 64);
            m = fmaxf(m, __shfl_xor(m, o, 64));
          }
          if (lane == 0) { sp[wv][0][k] = s; sp[wv][1][k] = m; sp[wv][2][k] = (float)cnt; }
        }
      }
    }
    __syncthreads();
    if (dst >= 0) {
      const int t = threadIdx.x;
      float* o = pair + dst * SPLAT_PAIR_CONTRIB;
      o[0] = ((sp[0][0][t] + sp[1][0][t]) + sp[2][0][t]) + sp[3][0][t];
      o[1] = fmaxf(fmaxf(sp[0][1][t], sp[1][1][t]), fmaxf(sp[2][1][t], sp[3][1][t]));
      o[2] = ((sp[0][2][t] + sp[1][2][t]) + sp[2][2][t]) + sp[3][2][t];
    }
  }
}

// thread = Gaussian: its run of pair records in list order (a fixed fp32 sum), then the four accumulators in place
__global__ void __launch_bounds__(256) k_splat_contrib_fold(const float* __restrict__ pair, const int32_t* __restrict__ start,
                                                            const int32_t* __restrict__ thits, int64_t N, float* __restrict__ max_acc,
                                                            double* __restrict__ sum_acc, int64_t* __restrict__ hits_acc, int32_t* __restrict__ views_acc) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int cnt = thits[i];
  if (cnt <= 0) return;  // not on screen: nothing to add
  float s = 0.f, m = 0.f;
  int32_t hits = 0;
  const float* p = pair + (int64_t)start[i] * SPLAT_PAIR_CONTRIB;
  for (int j = 0; j < cnt; ++j, p += SPLAT_PAIR_CONTRIB) {
    s += p[0];
    m = fmaxf(m, p[1]);
    hits += (int32_t)p[2];
  }
  max_acc[i] = fmaxf(max_acc[i], m);
  sum_acc[i] += (double)s;
  hits_acc[i] += (int64_t)hits;
  views_acc[i] += m > 0.f ? 1 : 0;
}

extern "C" int64_t tn_splat_contrib_workspace_bytes(int64_t num_gaussians, int64_t max_intersections) {
  if (num_gaussians < 0 || num_gaussians >= (1ll << 31) || max_intersections < 0) return -1;
  size_t total = 0;
  (void)splat_bwd_layout(nullptr, num_gaussians, max_intersections, SPLAT_PAIR_CONTRIB, &total);
  return (int64_t)total;
}

// `antialiased` is the frame's flag as tn_splat_project took it: the records already hold the chain's compensated opacity, so it selects nothing
// here and is only validated (the signature is tn_splat_raster's).
extern "C" int tn_splat_raster_contrib(const TnSplatCamera* camera, int64_t num_gaussians, void* workspace, int64_t max_intersections,
                                       int32_t antialiased, int32_t chain, const float* pixel_weight, void* scratch, int64_t scratch_bytes,
                                       float* max_acc, double* sum_acc, int64_t* hits_acc, int32_t* views_acc, tn_stream_t stream) {
  const char* who = "tn_splat_raster_contrib";
  int rc = check_cam(camera, who);
  if (rc) return rc;
  TN_REQUIRE(num_gaussians >= 0 && num_gaussians < (1ll << 31) && max_intersections >= 0 && max_intersections < (1ll << 31), "%s: bad sizes", who);
  TN_REQUIRE((antialiased == 0 || antialiased == 1) && (chain == 0 || chain == 1), "%s: antialiased = %d, chain = %d (each 0 or 1)", who, antialiased, chain);
  if (num_gaussians == 0) return TN_OK;
  TN_REQUIRE(workspace && scratch && max_acc && sum_acc && hits_acc && views_acc, "%s: null pointer", who);
  const int64_t need = tn_splat_contrib_workspace_bytes(num_gaussians, max_intersections);
  TN_REQUIRE(scratch_bytes >= need, "%s: scratch of %lld bytes, %lld needed (tn_splat_contrib_workspace_bytes)", who, (long long)scratch_bytes, (long long)need);
  SplatCamK k = make_camk(camera);
  const int num_tiles = k.tbx * k.tby;
  SplatWs ws = splat_layout(workspace, num_gaussians, max_intersections, num_tiles, nullptr);
  SplatBwdWs cw = splat_bwd_layout(scratch, num_gaussians, max_intersections, SPLAT_PAIR_CONTRIB, nullptr);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_splat_run_start, dim3((unsigned)tn_cdiv(num_gaussians, 256)), dim3(256), 0, st, ws.order, ws.cum, ws.thits, num_gaussians, cw.start);
  TN_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(k_splat_raster_contrib, dim3(num_tiles), dim3(256), 0, st, ws.recs, ws.vals[1], ws.tile_bins, ws.lvals[1], k.W, k.H, k.tbx, chain, pixel_weight,
                     cw.start, ws.tbox, cw.pair);
  TN_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(k_splat_contrib_fold, dim3((unsigned)tn_cdiv(num_gaussians, 256)), dim3(256), 0, st, cw.pair, cw.start, ws.thits, num_gaussians, max_acc,
                     sum_acc, hits_acc, views_acc);
  TN_CHECK_LAUNCH(who);
  return TN_OK;
}

extern "C" int64_t tn_splat_pose_workspace_bytes(int64_t num_gaussians) {
  if (num_gaussians < 0 || num_gaussians >= (1ll << 31)) return -1;
  return (int64_t)al256((size_t)std::max<int64_t>(tn_cdiv(num_gaussians, 256), 1) * 12 * sizeof(double));
}

// The projection + SH backward.  Optional groups: the thermal opacity {opacities_thermal, v_log_opacity_thermal, v_opacities_thermal} (SEP), the
// pose {pose_camera, pose_row, workspace, grad_pose_row} (POSE: the camera of the forward's record, dL/d pose ADDED to grad_pose_row through the
// finishing launch, dL/d view' left in dview_out where that is given) and {v_depths} (DEPTH, classic mode only).
extern "C" int tn_splat_project_backward(const TnSplatCamera* camera, const float* pose_camera, const float* pose_row, const float* means,
                                         const float* log_scales, const float* quats, const float* opacities, const float* features_dc,
                                         const float* features_rest, const float* thermal_dc, const float* thermal_rest, const float* opacities_thermal,
                                         int64_t num_gaussians, int32_t num_rest_coeffs, int32_t sh_degree, int32_t antialiased, const int32_t* radii,
                                         const float* v_xys, const float* v_conics, const float* v_colors, const float* v_log_opacity,
                                         const float* v_log_opacity_thermal, const float* v_depths, float* v_means, float* v_log_scales, float* v_quats,
                                         float* v_opacities, float* v_features_dc, float* v_features_rest, float* v_thermal_dc, float* v_thermal_rest,
                                         float* v_opacities_thermal, void* workspace, int64_t workspace_bytes, float* grad_pose_row, float* dview_out,
                                         tn_stream_t stream) {
  const char* who = "tn_splat_project_backward";
  TN_REQUIRE(!v_depths || antialiased == 0, "%s: the depth gradient exists in classic mode only (antialiased depth rides a chain of its own)", who);
  int rc = check_cam(camera, who);
  if (rc) return rc;
  if (num_gaussians == 0) return TN_OK;
  TN_REQUIRE(num_gaussians > 0 && num_gaussians < (1ll << 31), "%s: bad Gaussian count", who);
  const int sep_group = group_state(opacities_thermal, v_log_opacity_thermal, v_opacities_thermal), pose_group = group_state(pose_camera, pose_row, workspace, grad_pose_row);
  TN_REQUIRE(sep_group >= 0, "%s: null pointer (the thermal opacity's group opacities_thermal, v_log_opacity_thermal, v_opacities_thermal is partly given)", who);
  TN_REQUIRE(pose_group >= 0 && (pose_group || !dview_out), "%s: null pointer (the pose group pose_camera, pose_row, workspace, grad_pose_row is partly given)", who);
  TN_REQUIRE(means && log_scales && quats && opacities && features_dc && thermal_dc && radii && v_xys && v_conics && v_colors && v_log_opacity &&
                 v_means && v_log_scales && v_quats && v_opacities && v_features_dc && v_thermal_dc,
             "%s: null pointer", who);
  TN_REQUIRE(sh_degree >= -1 && sh_degree <= 3, "%s: sh_degree %d unsupported (-1 = sigmoid of the DC term, 0..3)", who, sh_degree);
  TN_REQUIRE(num_rest_coeffs >= (sh_degree < 1 ? 0 : (sh_degree + 1) * (sh_degree + 1) - 1) && num_rest_coeffs <= 15,
             "%s: %d higher-order coefficients for degree %d", who, num_rest_coeffs, sh_degree);
  TN_REQUIRE(num_rest_coeffs == 0 || (features_rest && thermal_rest && v_features_rest && v_thermal_rest), "%s: null SH coefficients", who);
  if (pose_group) {
    const int64_t need = tn_splat_pose_workspace_bytes(num_gaussians);
    TN_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes, tn_splat_pose_workspace_bytes asks for %lld", who, (long long)workspace_bytes, (long long)need);
  }
  SplatCamK k = make_camk(camera);
  const int nblk = (int)tn_cdiv(num_gaussians, 256);
  with_flags([&](auto SEP, auto POSE, auto DEPTH) {
    std::apply([&](auto... extra) {
      hipLaunchKernelGGL((k_splat_project_bwd<decltype(SEP)::value, decltype(extra)...>), dim3((unsigned)nblk), dim3(256), 0, tn_s(stream), k, means, log_scales, quats,
                         opacities, features_dc, features_rest, thermal_dc, thermal_rest, num_gaussians, sh_degree, num_rest_coeffs, antialiased, radii, v_xys,
                         v_conics, v_colors, v_log_opacity, v_means, v_log_scales, v_quats, v_opacities, v_features_dc, v_features_rest, v_thermal_dc,
                         v_thermal_rest, opacities_thermal, v_log_opacity_thermal, v_opacities_thermal, extra...);
    }, std::tuple_cat(opt_args(POSE, SplatPoseBwdK{pose_camera, (double*)workspace}), opt_args(DEPTH, SplatDepthProjK{v_depths})));
  }, sep_group != 0, pose_group != 0, v_depths != nullptr);
  TN_CHECK_LAUNCH(who);
  if (pose_group) {  // folds the blocks' partials and chains them to the pose row
    hipLaunchKernelGGL(k_splat_pose_finish, dim3(1), dim3(12 * SPLAT_POSE_SEGS), 0, tn_s(stream), k, pose_row, (const double*)workspace, nblk, grad_pose_row, dview_out);
    TN_CHECK_LAUNCH(who);
  }
  return TN_OK;
}

// ------------------------------------------------------------------------------------------------ refinement
// splatfacto's densification (SplatfactoModel.after_train / refinement_after, nerfstudio/models/splatfacto.py:346-498).  No float atomics:
//   k_splat_grad_stats      thread = Gaussian: the per-step statistics of after_train
//   k_refine_classify       thread = Gaussian: split / duplicate decisions and the cull decision of every row that Gaussian ends up in
//                           (original, its split children, its duplicate) -> four 0/1 counters
//   rocprim scan            inclusive scan of the counters (struct of 4 int32): each surviving row's place in the output
//   k_refine_map            thread = Gaussian: output row -> (source row, kind)
//   k_refine_gather         flat output elements of the eight parameter tensors and their Adam moments, one block = 1024 consecutive
//                           elements of one tensor: coalesced writes, reads that walk the source rows in order
// The arithmetic of the decisions is torch's as the reference evaluates it: full-precision expf / logf, sigmoid = 1 / (1 + exp(-x)), and a
// division by a host scalar as a multiply by its float reciprocal (what torch's GPU division by a Python number computes).
struct RefCnt {
  int32_t split, orig, child, dup;  // is split / original survives / its split children survive / its duplicate survives
};
struct RefCntSum {
  __host__ __device__ RefCnt operator()(const RefCnt& a, const RefCnt& b) const {
    return RefCnt{a.split + b.split, a.orig + b.orig, a.child + b.child, a.dup + b.dup};
  }
};

struct RefineK {  // the decisions of one refinement, derived on the host from TnSplatRefine and the step
  float cull_alpha, cull_scale, grad_thresh, size_thresh, cull_screen, split_screen, max_size;
  int densify, cull_big, screen;
};

struct RefineWs {
  RefCnt* cnt;   // [N]
  RefCnt* incl;  // [N] inclusive scan of cnt
  int2* map;     // [(S + 2) N] output row -> (source row, code): -1 original, -2 duplicate, -3 duplicate of a split Gaussian, >= 0 split child (noise row)
  void* tmp;
  size_t tmp_bytes;
};

#define REFINE_MAX_SAMPLES 16
#define REFINE_GATHER_ELEMS 1024  // per block: 256 threads x 4 elements

static RefineWs refine_layout(void* base, int64_t N, int32_t S, size_t* total) {
  RefineWs w;
  Carve cv{(char*)base, 0};
  const size_t n = (size_t)std::max<int64_t>(N, 1);
  w.cnt = (RefCnt*)cv.take(sizeof(RefCnt) * n);
  w.incl = (RefCnt*)cv.take(sizeof(RefCnt) * n);
  w.map = (int2*)cv.take(sizeof(int2) * n * (size_t)(S + 2));
  size_t b = 0;
  (void)rocprim::inclusive_scan(nullptr, b, (const RefCnt*)nullptr, (RefCnt*)nullptr, n, RefCntSum());
  w.tmp_bytes = al256(b) + 256;
  w.tmp = cv.take(w.tmp_bytes);
  if (total) *total = cv.off;
  return w;
}

extern "C" int64_t tn_splat_refine_workspace_bytes(int64_t num_gaussians, int32_t n_split_samples) {
  if (num_gaussians < 0 || num_gaussians >= (1ll << 31) || n_split_samples < 1 || n_split_samples > REFINE_MAX_SAMPLES) return -1;
  size_t total = 0;
  (void)refine_layout(nullptr, num_gaussians, n_split_samples, &total);
  return (int64_t)total;
}

__global__ void k_splat_grad_stats(const float2* __restrict__ xys_grad, const int32_t* __restrict__ radii, int64_t N, float inv_size, int first,
                                   float* __restrict__ grad_norm_sum, float* __restrict__ vis_counts, float* __restrict__ max_2d_size) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float2 g = xys_grad[i];
  const float n = sqrtf(g.x * g.x + g.y * g.y);
  const int32_t r = radii[i];
  const bool vis = r > 0;
  float m;
  if (first) {  // the first call after a reset: every Gaussian, visible or not
    grad_norm_sum[i] = n;
    vis_counts[i] = 1.0f;
    m = 0.0f;
  } else {
    if (vis) {
      grad_norm_sum[i] = n + grad_norm_sum[i];
      vis_counts[i] = vis_counts[i] + 1.0f;
    }
    m = max_2d_size[i];
  }
  if (vis) m = fmaxf(m, (float)r * inv_size);
  max_2d_size[i] = m;
}

__device__ static inline float refine_shrink(float s) { return logf(expf(s) * (1.0f / 1.6f)); }  // log(exp(s) / 1.6), splatfacto.py:555-556

// SEP (separate thermal opacity): a Gaussian is transparent only when BOTH opacities are below the threshold -- one visible in either spectrum stays
template <bool SEP>
__global__ void k_refine_classify(const float* __restrict__ log_scales, const float* __restrict__ opacities, const float* __restrict__ grad_norm_sum,
                                  const float* __restrict__ vis_counts, const float* __restrict__ max_2d_size, int64_t N, RefineK k,
                                  RefCnt* __restrict__ cnt, const float* __restrict__ opacities_th) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float s0 = log_scales[3 * i], s1 = log_scales[3 * i + 1], s2 = log_scales[3 * i + 2];
  const float emax = fmaxf(fmaxf(expf(s0), expf(s1)), expf(s2));
  const float m2d = max_2d_size[i];
  bool split = false, dup = false;
  float emax_new = emax;  // max exp(scale) of the rows this Gaussian adds (split children, duplicate): after the parent's shrink
  if (k.densify) {
    const float avg = ((grad_norm_sum[i] / vis_counts[i]) * 0.5f) * k.max_size;
    const bool high = avg > k.grad_thresh;
    split = (emax > k.size_thresh || (k.screen && m2d > k.split_screen)) && high;
    if (split) emax_new = fmaxf(fmaxf(expf(refine_shrink(s0)), expf(refine_shrink(s1))), expf(refine_shrink(s2)));
    dup = emax_new <= k.size_thresh && high;  // on the updated scales: a split Gaussian can be duplicated too (splatfacto.py:413)
  }
  bool transparent = 1.0f / (1.0f + expf(-opacities[i])) < k.cull_alpha;
  if (SEP) transparent = transparent && 1.0f / (1.0f + expf(-opacities_th[i])) < k.cull_alpha;
  const bool cull_orig = transparent || split || (k.cull_big && (emax > k.cull_scale || (k.screen && m2d > k.cull_screen)));
  const bool cull_new = transparent || (k.cull_big && (emax_new > k.cull_scale || (k.screen && 0.0f > k.cull_screen)));  // new rows: max_2d_size 0
  cnt[i] = RefCnt{split ? 1 : 0, cull_orig ? 0 : 1, split && !cull_new ? 1 : 0, dup && !cull_new ? 1 : 0};
}

__global__ void k_refine_map(const RefCnt* __restrict__ cnt, const RefCnt* __restrict__ incl, int64_t N, int32_t S, int2* __restrict__ map) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const RefCnt c = cnt[i], in = incl[i], tot = incl[N - 1];
  const int32_t src = (int32_t)i;
  if (c.orig) map[in.orig - 1] = make_int2(src, -1);
  if (c.child) {
    const int64_t at = (int64_t)tot.orig + (in.child - 1);
    const int32_t noise_row = in.split - 1;  // rank among ALL split Gaussians: the noise is drawn before the cull
    for (int j = 0; j < S; ++j) map[at + (int64_t)j * tot.child] = make_int2(src, j * tot.split + noise_row);
  }
  if (c.dup) map[(int64_t)tot.orig + (int64_t)S * tot.child + (in.dup - 1)] = make_int2(src, c.split ? -3 : -2);
}

template <int NT>    // 8, or 9 with the separate thermal opacity (the ninth tensor, copied exactly as the opacities are)
struct RefTensors {  // the eight parameter tensors (splat.py _PARAM_NAMES order) and their Adam moments; moments may be absent (null)
  const float* src[NT];
  const float* src_m1[NT];
  const float* src_m2[NT];
  float* dst[NT];
  float* dst_m1[NT];
  float* dst_m2[NT];
  int32_t width[NT];
  int64_t block_begin[NT + 1];  // first block of each tensor
};

template <int NT>
__global__ void __launch_bounds__(256) k_refine_gather(RefTensors<NT> t, const int2* __restrict__ map, int64_t num_out, const float* __restrict__ noise,
                                                       int64_t noise_rows, const float* __restrict__ means, const float* __restrict__ log_scales,
                                                       const float* __restrict__ quats, int64_t N) {
  int k = 0;
#pragma unroll
  for (int j = 1; j < NT; ++j) k += (int64_t)blockIdx.x >= t.block_begin[j] ? 1 : 0;  // block-uniform
  const int w = t.width[k];
  const float* __restrict__ src = t.src[k];
  const float* __restrict__ m1 = t.src_m1[k];
  const float* __restrict__ m2 = t.src_m2[k];
  float* __restrict__ dst = t.dst[k];
  const int64_t count = num_out * w;
  const int64_t base = ((int64_t)blockIdx.x - t.block_begin[k]) * REFINE_GATHER_ELEMS;
#pragma unroll
  for (int u = 0; u < REFINE_GATHER_ELEMS / 256; ++u) {
    const int64_t e = base + u * 256 + threadIdx.x;
    if (e >= count) break;
    const int64_t row = e / w;
    const int c = (int)(e - row * w);
    const int2 m = map[row];
    float v = 0.f, a = 0.f, b = 0.f;
    if ((uint64_t)m.x < (uint64_t)N) {
      const int64_t s = (int64_t)m.x * w + c;
      v = src[s];
      if (m.y == -1 && m1) {
        a = m1[s];
        b = m2[s];
      }
      if (k == 1 && m.y != -1 && m.y != -2) v = refine_shrink(v);  // split children and duplicates of split Gaussians
      if (k == 0 && m.y >= 0) {
        // child mean: mean + R(q / |q|) (exp(parent's log-scale) * z), splatfacto.py:541-549 (gsplat's quat_to_rotmat, w x y z)
        if (m.y < noise_rows) {
          const int64_t g = m.x;
          float qw = quats[4 * g], qx = quats[4 * g + 1], qy = quats[4 * g + 2], qz = quats[4 * g + 3];
          const float qn = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
          qw /= qn, qx /= qn, qy /= qn, qz /= qn;
          float r0, r1, r2;
          if (c == 0) {
            r0 = 1.f - 2.f * (qy * qy + qz * qz), r1 = 2.f * (qx * qy - qw * qz), r2 = 2.f * (qx * qz + qw * qy);
          } else if (c == 1) {
            r0 = 2.f * (qx * qy + qw * qz), r1 = 1.f - 2.f * (qx * qx + qz * qz), r2 = 2.f * (qy * qz - qw * qx);
          } else {
            r0 = 2.f * (qx * qz - qw * qy), r1 = 2.f * (qy * qz + qw * qx), r2 = 1.f - 2.f * (qx * qx + qy * qy);
          }
          const float* z = noise + 3 * (int64_t)m.y;
          const float* ls = log_scales + 3 * g;
          v = (r0 * (expf(ls[0]) * z[0]) + r1 * (expf(ls[1]) * z[1]) + r2 * (expf(ls[2]) * z[2])) + means[3 * g + c];
        }
      }
    }
    dst[e] = v;
    if (m1) {
      t.dst_m1[k][e] = a;
      t.dst_m2[k][e] = b;
    }
  }
}

static int refine_k(const TnSplatRefine* cfg, int32_t step, const char* who, RefineK* k, int* cull) {
  TN_REQUIRE(cfg != nullptr, "%s: null config", who);
  TN_REQUIRE(cfg->refine_every >= 1 && cfg->reset_alpha_every >= 1, "%s: refine_every %d / reset_alpha_every %d must be >= 1", who, cfg->refine_every,
             cfg->reset_alpha_every);
  TN_REQUIRE(cfg->n_split_samples >= 1 && cfg->n_split_samples <= REFINE_MAX_SAMPLES, "%s: n_split_samples %d outside [1, %d]", who, cfg->n_split_samples,
             REFINE_MAX_SAMPLES);
  TN_REQUIRE(cfg->max_size >= 1, "%s: max_size %d (the training frame's max(H, W)) must be >= 1", who, cfg->max_size);
  TN_REQUIRE(step >= 0, "%s: negative step", who);
  const int64_t R = (int64_t)cfg->reset_alpha_every * cfg->refine_every;
  k->densify = step < cfg->stop_split_at && (int64_t)step % R > (int64_t)cfg->num_train_data + cfg->refine_every;
  *cull = k->densify || (step >= cfg->stop_split_at && cfg->continue_cull_post_densification);
  k->cull_big = (int64_t)step > R;
  k->screen = step < cfg->stop_screen_size_at;
  k->cull_alpha = cfg->cull_alpha_thresh, k->cull_scale = cfg->cull_scale_thresh, k->grad_thresh = cfg->densify_grad_thresh;
  k->size_thresh = cfg->densify_size_thresh, k->cull_screen = cfg->cull_screen_size, k->split_screen = cfg->split_screen_size;
  k->max_size = (float)cfg->max_size;
  return TN_OK;
}

extern "C" int tn_splat_grad_stats(const float* xys_grad, const int32_t* radii, int64_t num_gaussians, int32_t max_size, int32_t first,
                                   float* grad_norm_sum, float* vis_counts, float* max_2d_size, tn_stream_t stream) {
  TN_REQUIRE(num_gaussians >= 0 && num_gaussians < (1ll << 31), "tn_splat_grad_stats: bad Gaussian count");
  TN_REQUIRE(max_size >= 1, "tn_splat_grad_stats: max_size %d (the frame's max(H, W)) must be >= 1", max_size);
  if (num_gaussians == 0) return TN_OK;
  TN_REQUIRE(xys_grad && radii && grad_norm_sum && vis_counts && max_2d_size, "tn_splat_grad_stats: null pointer");
  hipLaunchKernelGGL(k_splat_grad_stats, dim3((unsigned)tn_cdiv(num_gaussians, 256)), dim3(256), 0, tn_s(stream), (const float2*)xys_grad, radii,
                     num_gaussians, 1.0f / (float)max_size, first ? 1 : 0, grad_norm_sum, vis_counts, max_2d_size);
  TN_CHECK_LAUNCH("tn_splat_grad_stats");
  return TN_OK;
}

// opacities_thermal (separate thermal opacity) is optional: with it the both-below cull rule (k_refine_classify<true>)
extern "C" int tn_splat_refine_plan(const TnSplatRefine* config, int32_t step, const float* log_scales, const float* opacities,
                                    const float* opacities_thermal, const float* grad_norm_sum, const float* vis_counts, const float* max_2d_size,
                                    int64_t num_gaussians, void* workspace, int64_t workspace_bytes, int64_t* counts_out, tn_stream_t stream) {
  const char* who = "tn_splat_refine_plan";
  RefineK k;
  int cull = 0;
  int rc = refine_k(config, step, who, &k, &cull);
  if (rc) return rc;
  TN_REQUIRE(num_gaussians >= 0 && num_gaussians < (1ll << 31), "%s: bad Gaussian count", who);
  TN_REQUIRE(counts_out != nullptr, "%s: null output", who);
  const int64_t N = num_gaussians;
  counts_out[0] = 0, counts_out[1] = N, counts_out[2] = 0, counts_out[3] = 0;
  if (N == 0 || !cull) return TN_OK;  // nothing to refine: every Gaussian stays where it is
  TN_REQUIRE(log_scales && opacities && grad_norm_sum && vis_counts && max_2d_size && workspace, "%s: null pointer", who);
  const int64_t need = tn_splat_refine_workspace_bytes(N, config->n_split_samples);
  TN_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes, (long long)need);
  RefineWs ws = refine_layout(workspace, N, config->n_split_samples, nullptr);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(opacities_thermal ? k_refine_classify<true> : k_refine_classify<false>, dim3((unsigned)tn_cdiv(N, 256)), dim3(256), 0, st, log_scales, opacities,
                     grad_norm_sum, vis_counts, max_2d_size, N, k, ws.cnt, opacities_thermal);
  TN_CHECK_LAUNCH(who);
  size_t tb = ws.tmp_bytes;
  if (rocprim::inclusive_scan(ws.tmp, tb, (const RefCnt*)ws.cnt, ws.incl, (size_t)N, RefCntSum(), st) != hipSuccess) {
    tn_set_error("%s: scan failed", who);
    return TN_ELAUNCH;
  }
  RefCnt tot;
  if (hipMemcpyAsync(&tot, ws.incl + (N - 1), sizeof(RefCnt), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    tn_set_error("%s: read-back of the counts failed", who);
    return TN_ELAUNCH;
  }
  counts_out[0] = tot.split, counts_out[1] = tot.orig, counts_out[2] = (int64_t)tot.child * config->n_split_samples, counts_out[3] = tot.dup;
  return TN_OK;
}

template <int NT>
static int splat_refine_apply(const char* who, const TnSplatRefine* config, int64_t num_gaussians, int32_t num_rest_coeffs, const void* workspace,
                                     int64_t workspace_bytes, const int64_t* counts, const float* noise, const float* const* params,
                                     const float* const* exp_avg, const float* const* exp_avg_sq, float* const* new_params, float* const* new_exp_avg,
                                     float* const* new_exp_avg_sq, tn_stream_t stream) {
  TN_REQUIRE(config != nullptr && counts != nullptr, "%s: null pointer", who);
  const int32_t S = config->n_split_samples;
  TN_REQUIRE(S >= 1 && S <= REFINE_MAX_SAMPLES, "%s: n_split_samples %d outside [1, %d]", who, S, REFINE_MAX_SAMPLES);
  TN_REQUIRE(num_gaussians >= 0 && num_gaussians < (1ll << 31), "%s: bad Gaussian count", who);
  TN_REQUIRE(num_rest_coeffs >= 0 && num_rest_coeffs <= 15, "%s: %d higher-order coefficients", who, num_rest_coeffs);
  const int64_t N = num_gaussians;
  TN_REQUIRE(counts[0] >= 0 && counts[0] <= N && counts[1] >= 0 && counts[1] <= N && counts[2] >= 0 && counts[2] <= S * counts[0] &&
                 counts[2] % S == 0 && counts[3] >= 0 && counts[3] <= N,
             "%s: counts (%lld, %lld, %lld, %lld) are not a plan of %lld Gaussians", who, (long long)counts[0], (long long)counts[1],
             (long long)counts[2], (long long)counts[3], (long long)N);
  const int64_t num_out = counts[1] + counts[2] + counts[3];
  if (num_out == 0) return TN_OK;  // everything culled (N == 0 included): nothing to write
  TN_REQUIRE(params && exp_avg && exp_avg_sq && new_params && new_exp_avg && new_exp_avg_sq && workspace, "%s: null pointer", who);
  TN_REQUIRE(counts[2] == 0 || noise != nullptr, "%s: null noise for %lld split children", who, (long long)counts[2]);
  const int64_t need = tn_splat_refine_workspace_bytes(N, S);
  TN_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed", who, (long long)workspace_bytes, (long long)need);
  const int32_t widths[9] = {3, 3, 4, 1, 3, 3 * num_rest_coeffs, 1, num_rest_coeffs, 1};
  RefTensors<NT> t;
  int64_t blocks = 0;
  for (int j = 0; j < NT; ++j) {
    const bool on = widths[j] > 0;
    TN_REQUIRE(!on || (params[j] && new_params[j]), "%s: null parameter %d", who, j);
    TN_REQUIRE((exp_avg[j] == nullptr) == (exp_avg_sq[j] == nullptr) && (exp_avg[j] == nullptr) == (new_exp_avg[j] == nullptr) &&
                   (exp_avg[j] == nullptr) == (new_exp_avg_sq[j] == nullptr),
               "%s: moments of parameter %d are partly null", who, j);
    t.src[j] = params[j], t.src_m1[j] = on ? exp_avg[j] : nullptr, t.src_m2[j] = on ? exp_avg_sq[j] : nullptr;
    t.dst[j] = new_params[j], t.dst_m1[j] = on ? new_exp_avg[j] : nullptr, t.dst_m2[j] = on ? new_exp_avg_sq[j] : nullptr;
    t.width[j] = std::max(widths[j], 1);
    t.block_begin[j] = blocks;
    blocks += on ? tn_cdiv(num_out * widths[j], REFINE_GATHER_ELEMS) : 0;
  }
  t.block_begin[NT] = blocks;
  TN_REQUIRE(blocks < (1ll << 31), "%s: %lld output rows are too many", who, (long long)num_out);
  RefineWs ws = refine_layout(const_cast<void*>(workspace), N, S, nullptr);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_refine_map, dim3((unsigned)tn_cdiv(N, 256)), dim3(256), 0, st, ws.cnt, ws.incl, N, S, ws.map);
  TN_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(k_refine_gather<NT>, dim3((unsigned)blocks), dim3(256), 0, st, t, ws.map, num_out, noise, (int64_t)counts[0] * S, params[0], params[1],
                     params[2], N);
  TN_CHECK_LAUNCH(who);
  return TN_OK;
}

// num_tensors says how many entries each of the six HOST arrays holds: 8, or 9 with the separate thermal opacity
extern "C" int tn_splat_refine_apply(const TnSplatRefine* config, int64_t num_gaussians, int32_t num_rest_coeffs, const void* workspace,
                                     int64_t workspace_bytes, const int64_t* counts, const float* noise, int32_t num_tensors, const float* const* params,
                                     const float* const* exp_avg, const float* const* exp_avg_sq, float* const* new_params, float* const* new_exp_avg,
                                     float* const* new_exp_avg_sq, tn_stream_t stream) {
  TN_REQUIRE(num_tensors == 8 || num_tensors == 9, "tn_splat_refine_apply: %d tensors per array (8, or 9 with the thermal opacity)", num_tensors);
  return (num_tensors == 8 ? splat_refine_apply<8> : splat_refine_apply<9>)("tn_splat_refine_apply", config, num_gaussians, num_rest_coeffs, workspace, workspace_bytes,
                                                                            counts, noise, params, exp_avg, exp_avg_sq, new_params, new_exp_avg, new_exp_avg_sq,
                                                                            stream);
}
