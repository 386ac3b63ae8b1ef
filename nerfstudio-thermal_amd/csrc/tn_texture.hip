// Texture baking for exported meshes: the counterpart of nerfstudio/exporter/texture_utils.py with unwrap_method "custom"
// (unwrap_mesh_per_uv_triangle, and the ray length and origin offset of export_textured_mesh).  tests/texture_functional.py restates the reference's
// formula in float64 and float32.
//
// THE ATLAS (the reference's layout)
//   F faces, px = px_per_uv_triangle >= 2.  Two faces share a square of (px + 3) x px texels; squares = ceil(F / 2), squares_w = ceil(sqrt(squares)),
//   squares_h = ceil(squares / squares_w), squares in row-major order; the image is W = squares_w (px + 3) wide and H = squares_h px high.  Face f lives
//   in square f / 2: the even face in the upper-left triangle, the odd one in the lower-right.
//   A texel (x, y) has the local offsets i = x mod (px + 3), j = y mod px and belongs to the lower-right triangle iff i + j >= px + 1.
//   The reference puts the triangles' corners on texel centres -- upper-left: texels (0, 0), (px - 1, 0), (0, px - 1); lower-right: (px + 2, px - 1),
//   (3, px - 1), (px + 2, 0) -- so its barycentric weights are small integers over px - 1:
//       upper-left   w1 = i / (px - 1),            w2 = j / (px - 1)
//       lower-right  w1 = (px + 2 - i) / (px - 1), w2 = (px - 1 - j) / (px - 1)           w0 = (1 - w1) - w2
//   evaluated in double: no UV image, no areas, no cancellation.  Texels of the 3-texel gap get weights outside [0, 1], as the reference's do (a
//   bilinear lookup next to the hypotenuse reads them).  A texel whose face index 2 square + lower is not below F (the tail of the last row, the
//   empty half of an odd last square) is addressed by no texture coordinate; it takes the LAST face with the local weights above, so it is finite.
//   A face that names a vertex outside [0, V) gives zeros (origin, direction, colour) and adds nothing to the mean edge.
//
// THE KERNELS (a thread per texel or per face, no atomics: the same inputs give the same bytes)
//   k_texture_coords   the [F,3,2] texture coordinates (corner texel + 0.5) / (W, H), in double, rounded once
//   k_texture_rays     texels [texel0, texel0 + count) of the row-major image: origin = sum w_i v_i, direction = -sum w_i n_i over max(length, 1e-12),
//                      both in double and rounded once to fp32; then, in fp32, origin -= (raylen / 2) direction (product and difference each rounded)
//   k_texture_vertex   the same texels: sum w_i rgbt[v_i], in double, rounded once
//   k_texture_store    a rendered chunk into the uint8 images (rint(255 clamp(v, 0, 1)), half to even; a NaN gives 0) and the optional float image
//   k_mean_edge_*      mean |v1 - v0| over the faces: double norms, a grid-stride sum per thread, wave and block sums in a fixed order, one block sums
//                      the blocks
#include "tn_common.h"

#include <algorithm>

namespace {

constexpr int TB = 256;                 // threads per block
constexpr int MAX_BLOCKS = 1 << 20;     // blocks of a grid-stride launch
constexpr int EDGE_BLOCKS = 1024;       // partial sums of the mean edge
constexpr int32_t PX_MAX = 32768;
constexpr int64_t FACES_MAX = ((1ll << 31) - 1) / 3;
constexpr int64_t VERTS_MAX = (1ll << 31) - 1;

struct AtlasK {
  int64_t F;
  int64_t total;  // W * H
  int32_t px, sw, squares_w, squares_h, W, H;
};

bool atlas_of(int64_t F, int32_t px, AtlasK& a) {
  if (F < 1 || F > FACES_MAX || px < 2 || px > PX_MAX) return false;
  const int64_t squares = (F + 1) / 2;
  int64_t s = (int64_t)sqrt((double)squares);
  while (s * s < squares) ++s;
  while (s > 1 && (s - 1) * (s - 1) >= squares) --s;
  a.F = F, a.px = px, a.sw = px + 3;
  a.squares_w = (int32_t)s, a.squares_h = (int32_t)((squares + s - 1) / s);
  a.W = a.squares_w * a.sw, a.H = a.squares_h * px;
  a.total = (int64_t)a.W * a.H;
  return true;
}

// texel t of the row-major image -> its face (clamped to F - 1) and the weights of the face's second and third corner
__device__ __forceinline__ void texel_decode(const AtlasK& a, int64_t t, int64_t& face, double& w1, double& w2) {
  const int64_t y64 = tn_div_index(t, a.W, a.total);
  const uint32_t y = (uint32_t)y64, x = (uint32_t)(t - y64 * a.W);
  const uint32_t sx = x / (uint32_t)a.sw, i = x - sx * (uint32_t)a.sw, sy = y / (uint32_t)a.px, j = y - sy * (uint32_t)a.px;
  const bool lower = i + j >= (uint32_t)a.px + 1u;
  const int64_t f = 2 * ((int64_t)sy * a.squares_w + sx) + (lower ? 1 : 0);
  face = f < a.F ? f : a.F - 1;
  const double den = (double)(a.px - 1);
  w1 = (double)(lower ? a.px + 2 - (int)i : (int)i) / den;
  w2 = (double)(lower ? a.px - 1 - (int)j : (int)j) / den;
}

// the three vertices of face f, or false where one lies outside [0, V)
__device__ __forceinline__ bool face_corners(const int32_t* __restrict__ faces, int64_t f, int64_t V, int64_t& i0, int64_t& i1, int64_t& i2) {
  i0 = (int64_t)(uint32_t)faces[3 * f], i1 = (int64_t)(uint32_t)faces[3 * f + 1], i2 = (int64_t)(uint32_t)faces[3 * f + 2];
  return i0 < V && i1 < V && i2 < V;
}

__device__ __forceinline__ double blend(double w0, double w1, double w2, float a, float b, float c) {
  return (w0 * (double)a + w1 * (double)b) + w2 * (double)c;
}

__global__ void __launch_bounds__(TB) k_texture_coords(AtlasK a, float* __restrict__ coords) {
  for (int64_t f = (int64_t)blockIdx.x * TB + threadIdx.x; f < a.F; f += (int64_t)gridDim.x * TB) {
    const int64_t sq = f >> 1;
    const int64_t sy = sq / a.squares_w, sx = sq - sy * a.squares_w;
    const bool lower = (f & 1) != 0;
    const int p = a.px;
    const int ci[3] = {lower ? p + 2 : 0, lower ? 3 : p - 1, lower ? p + 2 : 0};
    const int cj[3] = {lower ? p - 1 : 0, lower ? p - 1 : 0, lower ? 0 : p - 1};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      coords[6 * f + 2 * k] = (float)(((double)(sx * a.sw + ci[k]) + 0.5) / (double)a.W);
      coords[6 * f + 2 * k + 1] = (float)(((double)(sy * p + cj[k]) + 0.5) / (double)a.H);
    }
  }
}

__global__ void __launch_bounds__(TB) k_texture_rays(const float* __restrict__ vertices, const float* __restrict__ normals, int64_t V,
                                                     const int32_t* __restrict__ faces, AtlasK a, float half_raylen, int64_t texel0, int64_t count,
                                                     float* __restrict__ origins, float* __restrict__ directions) {
  for (int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x; r < count; r += (int64_t)gridDim.x * TB) {
    int64_t f, i0, i1, i2;
    double w1, w2;
    texel_decode(a, texel0 + r, f, w1, w2);
    const double w0 = (1.0 - w1) - w2;
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
    if (face_corners(faces, f, V, i0, i1, i2)) {
      double n[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        o[k] = (float)blend(w0, w1, w2, vertices[3 * i0 + k], vertices[3 * i1 + k], vertices[3 * i2 + k]);
        n[k] = -blend(w0, w1, w2, normals[3 * i0 + k], normals[3 * i1 + k], normals[3 * i2 + k]);
      }
      const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
      const double den = len > 1e-12 ? len : 1e-12;  // F.normalize's rule
#pragma unroll
      for (int k = 0; k < 3; ++k) d[k] = (float)(n[k] / den);
      if (half_raylen != 0.0f) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = __fsub_rn(o[k], __fmul_rn(half_raylen, d[k]));
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) origins[3 * r + k] = o[k], directions[3 * r + k] = d[k];
  }
}

__global__ void __launch_bounds__(TB) k_texture_vertex(const float4* __restrict__ rgbt, int64_t V, const int32_t* __restrict__ faces, AtlasK a,
                                                       int64_t texel0, int64_t count, float4* __restrict__ out) {
  for (int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x; r < count; r += (int64_t)gridDim.x * TB) {
    int64_t f, i0, i1, i2;
    double w1, w2;
    texel_decode(a, texel0 + r, f, w1, w2);
    const double w0 = (1.0 - w1) - w2;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (face_corners(faces, f, V, i0, i1, i2)) {
      const float4 c0 = rgbt[i0], c1 = rgbt[i1], c2 = rgbt[i2];
      v = make_float4((float)blend(w0, w1, w2, c0.x, c1.x, c2.x), (float)blend(w0, w1, w2, c0.y, c1.y, c2.y),
                      (float)blend(w0, w1, w2, c0.z, c1.z, c2.z), (float)blend(w0, w1, w2, c0.w, c1.w, c2.w));
    }
    out[r] = v;
  }
}

__device__ __forceinline__ uint8_t to_byte(float v) {  // rint(255 clamp(v, 0, 1)); a NaN gives 0
  const float s = __fmul_rn(v, 255.0f);
  return (uint8_t)rintf(fminf(fmaxf(s, 0.0f), 255.0f));
}

__global__ void __launch_bounds__(TB) k_texture_store(const float* __restrict__ rgb, int64_t rgb_stride, const float* __restrict__ thermal,
                                                      int64_t thermal_stride, int64_t count, int64_t texel0, uint8_t* __restrict__ rgb_image,
                                                      uint8_t* __restrict__ thermal_image, float4* __restrict__ float_image) {
  for (int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x; r < count; r += (int64_t)gridDim.x * TB) {
    const float cr = rgb[r * rgb_stride], cg = rgb[r * rgb_stride + 1], cb = rgb[r * rgb_stride + 2], ct = thermal[r * thermal_stride];
    const int64_t t = texel0 + r;
    rgb_image[3 * t] = to_byte(cr), rgb_image[3 * t + 1] = to_byte(cg), rgb_image[3 * t + 2] = to_byte(cb);
    thermal_image[t] = to_byte(ct);
    if (float_image != nullptr) float_image[t] = make_float4(cr, cg, cb, ct);
  }
}

__device__ inline double block_sum_d(double v) {  // the block's sum in thread 0: lanes by xor shuffles, then the waves in ascending order
  __shared__ double wave_sum[TB / TN_WAVE];
  v = tn_wave_sum_d(v);
  if (tn_lane() == 0) wave_sum[threadIdx.x / TN_WAVE] = v;
  __syncthreads();
  double all = 0.0;
#pragma unroll
  for (int x = 0; x < TB / TN_WAVE; ++x) all += wave_sum[x];
  return all;
}

__global__ void __launch_bounds__(TB) k_mean_edge_partial(const float* __restrict__ vertices, int64_t V, const int32_t* __restrict__ faces, int64_t F,
                                                          double* __restrict__ partial) {
  double s = 0.0;
  for (int64_t f = (int64_t)blockIdx.x * TB + threadIdx.x; f < F; f += (int64_t)gridDim.x * TB) {
    int64_t i0, i1, i2;
    if (!face_corners(faces, f, V, i0, i1, i2)) continue;
    const double dx = (double)vertices[3 * i1] - (double)vertices[3 * i0], dy = (double)vertices[3 * i1 + 1] - (double)vertices[3 * i0 + 1],
                 dz = (double)vertices[3 * i1 + 2] - (double)vertices[3 * i0 + 2];
    s += sqrt((dx * dx + dy * dy) + dz * dz);
  }
  const double all = block_sum_d(s);
  if (threadIdx.x == 0) partial[blockIdx.x] = all;
}

__global__ void __launch_bounds__(TB) k_mean_edge_final(const double* __restrict__ partial, int num, int64_t F, float* __restrict__ mean) {
  double s = 0.0;
  for (int i = threadIdx.x; i < num; i += TB) s += partial[i];
  const double all = block_sum_d(s);
  if (threadIdx.x == 0) mean[0] = (float)(all / (double)F);
}

unsigned blocks_of(int64_t n) { return (unsigned)std::min<int64_t>(tn_cdiv(n, TB), MAX_BLOCKS); }

// what the entry points over a texel range share: the atlas, the mesh, the range
int range_check(const char* name, int64_t V, const int32_t* faces, int64_t F, int32_t px, int64_t texel0, int64_t count, AtlasK& a) {
  TN_REQUIRE(atlas_of(F, px, a), "%s: %lld faces (1..(2^31 - 1) / 3) at %d texels per triangle (2..%d)", name, (long long)F, px, PX_MAX);
  TN_REQUIRE(V >= 1 && V <= VERTS_MAX, "%s: %lld vertices (1..2^31 - 1)", name, (long long)V);
  TN_REQUIRE(texel0 >= 0 && count >= 0 && texel0 <= a.total && count <= a.total - texel0,
             "%s: texels [%lld, %lld + %lld) outside the image of %d x %d", name, (long long)texel0, (long long)texel0, (long long)count, a.W, a.H);
  TN_REQUIRE(faces && ((uintptr_t)faces & 3) == 0, "%s: null or misaligned pointer (faces)", name);
  return TN_OK;
}

}  // namespace

extern "C" int tn_texture_layout(int64_t num_faces, int32_t px_per_uv_triangle, int64_t* layout) {
  AtlasK a;
  TN_REQUIRE(layout, "tn_texture_layout: null pointer");
  TN_REQUIRE(atlas_of(num_faces, px_per_uv_triangle, a), "tn_texture_layout: %lld faces (1..(2^31 - 1) / 3) at %d texels per triangle (2..%d)",
             (long long)num_faces, px_per_uv_triangle, PX_MAX);
  layout[0] = a.W, layout[1] = a.H, layout[2] = a.squares_w, layout[3] = a.squares_h;
  return TN_OK;
}

extern "C" int tn_texture_coords(int64_t num_faces, int32_t px_per_uv_triangle, float* texture_coordinates, tn_stream_t stream) {
  AtlasK a;
  TN_REQUIRE(atlas_of(num_faces, px_per_uv_triangle, a), "tn_texture_coords: %lld faces (1..(2^31 - 1) / 3) at %d texels per triangle (2..%d)",
             (long long)num_faces, px_per_uv_triangle, PX_MAX);
  TN_REQUIRE(texture_coordinates && ((uintptr_t)texture_coordinates & 3) == 0, "tn_texture_coords: null or misaligned pointer");
  hipLaunchKernelGGL(k_texture_coords, dim3(blocks_of(num_faces)), dim3(TB), 0, tn_s(stream), a, texture_coordinates);
  TN_CHECK_LAUNCH("tn_texture_coords");
  return TN_OK;
}

extern "C" int tn_texture_rays(const float* vertices, const float* normals, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                               int32_t px_per_uv_triangle, float raylen, int64_t texel0, int64_t count, float* origins, float* directions,
                               tn_stream_t stream) {
  AtlasK a;
  if (const int rc = range_check("tn_texture_rays", num_vertices, faces, num_faces, px_per_uv_triangle, texel0, count, a)) return rc;
  TN_REQUIRE(raylen >= 0.0f && raylen <= 3.4028234663852886e38f, "tn_texture_rays: raylen = %g (>= 0, finite)", (double)raylen);
  TN_REQUIRE(vertices && normals && (count == 0 || (origins && directions)), "tn_texture_rays: null pointer");
  TN_REQUIRE((((uintptr_t)vertices | (uintptr_t)normals | (uintptr_t)origins | (uintptr_t)directions) & 3) == 0, "tn_texture_rays: misaligned pointer");
  if (count == 0) return TN_OK;
  hipLaunchKernelGGL(k_texture_rays, dim3(blocks_of(count)), dim3(TB), 0, tn_s(stream), vertices, normals, num_vertices, faces, a, 0.5f * raylen, texel0,
                     count, origins, directions);
  TN_CHECK_LAUNCH("tn_texture_rays");
  return TN_OK;
}

extern "C" int tn_texture_vertex(const float* rgbt, int64_t num_vertices, const int32_t* faces, int64_t num_faces, int32_t px_per_uv_triangle,
                                 int64_t texel0, int64_t count, float* out_rgbt, tn_stream_t stream) {
  AtlasK a;
  if (const int rc = range_check("tn_texture_vertex", num_vertices, faces, num_faces, px_per_uv_triangle, texel0, count, a)) return rc;
  TN_REQUIRE(rgbt && (count == 0 || out_rgbt), "tn_texture_vertex: null pointer");
  TN_REQUIRE(((uintptr_t)rgbt & 15) == 0 && ((uintptr_t)out_rgbt & 15) == 0, "tn_texture_vertex: the two rgbt arrays must be 16-byte aligned");
  if (count == 0) return TN_OK;
  hipLaunchKernelGGL(k_texture_vertex, dim3(blocks_of(count)), dim3(TB), 0, tn_s(stream), reinterpret_cast<const float4*>(rgbt), num_vertices, faces, a,
                     texel0, count, reinterpret_cast<float4*>(out_rgbt));
  TN_CHECK_LAUNCH("tn_texture_vertex");
  return TN_OK;
}

extern "C" int tn_texture_store(const float* rgb, int64_t rgb_stride, const float* thermal, int64_t thermal_stride, int64_t count, int64_t texel0,
                                int64_t num_texels, uint8_t* rgb_image, uint8_t* thermal_image, float* float_image, tn_stream_t stream) {
  TN_REQUIRE(num_texels >= 0 && texel0 >= 0 && count >= 0 && texel0 <= num_texels && count <= num_texels - texel0,
             "tn_texture_store: texels [%lld, %lld + %lld) outside the image of %lld", (long long)texel0, (long long)texel0, (long long)count,
             (long long)num_texels);
  TN_REQUIRE(rgb_stride >= 3 && thermal_stride >= 1, "tn_texture_store: row strides of %lld and %lld floats (at least 3 and 1)", (long long)rgb_stride,
             (long long)thermal_stride);
  TN_REQUIRE(count == 0 || (rgb && thermal && rgb_image && thermal_image), "tn_texture_store: null pointer");
  TN_REQUIRE((((uintptr_t)rgb | (uintptr_t)thermal) & 3) == 0 && ((uintptr_t)float_image & 15) == 0,
             "tn_texture_store: misaligned pointer (the float image to 16 bytes)");
  if (count == 0) return TN_OK;
  hipLaunchKernelGGL(k_texture_store, dim3(blocks_of(count)), dim3(TB), 0, tn_s(stream), rgb, rgb_stride, thermal, thermal_stride, count, texel0, rgb_image,
                     thermal_image, reinterpret_cast<float4*>(float_image));
  TN_CHECK_LAUNCH("tn_texture_store");
  return TN_OK;
}

extern "C" int64_t tn_mesh_mean_edge_workspace_bytes(int64_t num_faces) {
  if (num_faces < 1 || num_faces > FACES_MAX) return -1;
  return (int64_t)EDGE_BLOCKS * 8;
}

extern "C" int tn_mesh_mean_edge(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces, float* mean, void* workspace,
                                 int64_t workspace_bytes, tn_stream_t stream) {
  TN_REQUIRE(num_faces >= 1 && num_faces <= FACES_MAX && num_vertices >= 1 && num_vertices <= VERTS_MAX,
             "tn_mesh_mean_edge: %lld vertices (1..2^31 - 1) and %lld faces (1..(2^31 - 1) / 3)", (long long)num_vertices, (long long)num_faces);
  TN_REQUIRE(vertices && faces && mean && workspace, "tn_mesh_mean_edge: null pointer");
  TN_REQUIRE((((uintptr_t)vertices | (uintptr_t)faces | (uintptr_t)mean) & 3) == 0 && ((uintptr_t)workspace & 7) == 0,
             "tn_mesh_mean_edge: misaligned pointer (the workspace to 8 bytes)");
  TN_REQUIRE(workspace_bytes >= (int64_t)EDGE_BLOCKS * 8, "tn_mesh_mean_edge: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)EDGE_BLOCKS * 8);
  double* partial = static_cast<double*>(workspace);
  const int nb = (int)std::min<int64_t>(tn_cdiv(num_faces, TB), EDGE_BLOCKS);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_mean_edge_partial, dim3(nb), dim3(TB), 0, st, vertices, num_vertices, faces, num_faces, partial);
  TN_CHECK_LAUNCH("tn_mesh_mean_edge(partial)");
  hipLaunchKernelGGL(k_mean_edge_final, dim3(1), dim3(TB), 0, st, (const double*)partial, nb, num_faces, mean);
  TN_CHECK_LAUNCH("tn_mesh_mean_edge(final)");
  return TN_OK;
}
