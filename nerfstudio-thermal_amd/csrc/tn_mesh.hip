// TSDF mesh export (the HIP form of ns-export tsdf: nerfstudio/exporter/tsdf_utils.py, TSDF.integrate_tsdf / get_mesh).
//
// tn_tsdf_integrate  B rendered frames -> the volume, ONE launch: a thread per voxel (consecutive lanes = consecutive z) walks the frames in order and
//                    keeps the running value, weight and RGB+T in registers; the volume is read and written at most once per call, and only where a
//                    frame observed the voxel.  No [B,*,N] temporaries.
// tn_mesh_count      marching tetrahedra on the Freudenthal split of every cell (six tetrahedra around the main diagonal, the same split in every
//                    cell): the edge flags of every lattice point, the vertices and triangles per block of 256 points, their exclusive scans and
//                    the two totals, left on the device
// tn_mesh_emit       the indexed mesh: vertices, normals, RGB+T in (lattice point, edge kind) order, faces in (cell, tetrahedron, triangle) order
//
// The order of every output is fixed by prefix sums (no atomics), and the arithmetic is written operation by operation (the build has
// -ffp-contract=off), so tests/tsdf_functional.py restates the extraction bit for bit.
#include "tn_common.h"

namespace {

constexpr int MB = 256;  // threads (= voxels / lattice points) per block
constexpr int64_t MESH_MAX_POINTS = (1ll << 31) - 1;

constexpr int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }

// ---------------------------------------------------------------------------------------------------- integration
struct TsdfVolumeK {
  float* values;
  float* weights;
  float4* rgbt;
  uint32_t N, Y, Z;
  float ox, oy, oz, sx, sy, sz;
  float truncation, max_weight;
};
struct TsdfFramesK {
  const float* depth;
  const float4* rgbt;
  const float* accumulation;  // or null
  const float* cameras;       // [B,16]: world -> camera rows of 3x4, fx fy cx cy
  float min_accumulation;
  int B, H, W;
  int ray_depth;  // compare Euclidean distances (else camera z)
};

__global__ void __launch_bounds__(MB) k_tsdf_integrate(TsdfVolumeK vol, TsdfFramesK fr) {
  const uint32_t p = blockIdx.x * MB + threadIdx.x;
  if (p >= vol.N) return;
  const uint32_t k = p % vol.Z, t = p / vol.Z, j = t % vol.Y, i = t / vol.Y;
  const float px = vol.ox + (float)i * vol.sx, py = vol.oy + (float)j * vol.sy, pz = vol.oz + (float)k * vol.sz;
  const float fw = (float)fr.W, fh = (float)fr.H;
  bool loaded = false;
  float val = 0.0f, w = 0.0f;
  float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int b = 0; b < fr.B; ++b) {
    const float* m = fr.cameras + 16 * b;  // wave-uniform
    const float x = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
    const float y = -(((m[4] * px + m[5] * py) + m[6] * pz) + m[7]);   // nerfstudio's camera looks down -z with y up: flip both
    const float z = -(((m[8] * px + m[9] * py) + m[10] * pz) + m[11]);
    if (!(z > 0.0f)) continue;  // behind the camera (or NaN): not observed
    const float vd = fr.ray_depth ? sqrtf((x * x + y * y) + z * z) : z;
    const float u = m[12] * (x / z) + m[14], v = m[13] * (y / z) + m[15];
    const float fu = rintf(u - 0.5f), fv = rintf(v - 0.5f);  // grid_sample(nearest, align_corners=False): half to even
    if (!(fu >= 0.0f && fu < fw && fv >= 0.0f && fv < fh)) continue;  // zero padding: depth 0
    const int64_t pix = ((int64_t)b * fr.H + (int)fv) * fr.W + (int)fu;
    const float d = fr.depth[pix];
    if (fr.accumulation != nullptr && fr.accumulation[pix] < fr.min_accumulation) continue;  // counts as depth 0
    const float dist = d - vd;
    if (!(vd > 0.0f && d > 0.0f && dist > -vol.truncation)) continue;
    float tsdf = dist / vol.truncation;
    tsdf = tsdf < -1.0f ? -1.0f : (tsdf > 1.0f ? 1.0f : tsdf);
    if (!loaded) {
      val = vol.values[p], w = vol.weights[p], c = vol.rgbt[p];
      loaded = true;
    }
    const float4 s = fr.rgbt[pix];
    const float tw = w + 1.0f;
    val = (val * w + tsdf) / tw;
    c.x = (c.x * w + s.x) / tw;
    c.y = (c.y * w + s.y) / tw;
    c.z = (c.z * w + s.z) / tw;
    c.w = (c.w * w + s.w) / tw;
    w = fminf(tw, vol.max_weight);
  }
  if (loaded) vol.values[p] = val, vol.weights[p] = w, vol.rgbt[p] = c;  // an unobserved voxel keeps its bits
}

// ---------------------------------------------------------------------------------------------------- extraction
// Corners of a cell are numbered dx + 2 dy + 4 dz.  The tetrahedra are (0, a, a + b, 7) for the six orders (a, b, c) of the axes, in lexicographic
// order; a tetrahedron is positively oriented iff the order is an even permutation.  An edge joins a corner to one that contains it; its kind is
// its direction: +x +y +z +xy +yz +xz +xyz.
__constant__ const uint8_t TET_CORNER[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__constant__ const uint8_t TET_ODD[6] = {0, 1, 1, 0, 0, 1};
__constant__ const uint8_t KIND_MASK[7] = {1, 2, 4, 3, 6, 5, 7};      // direction (as a corner number) of an edge kind
__constant__ const uint8_t MASK_KIND[8] = {0, 0, 1, 3, 2, 5, 4, 6};   // and back
// edges of a tetrahedron (v0 v1 v2 v3): 0: 01, 1: 02, 2: 03, 3: 12, 4: 13, 5: 23
__constant__ const uint8_t TET_EDGE[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// The 16 sign cases (bit n: v_n is inside, value < 0) of a POSITIVELY oriented tetrahedron: the triangles' edges, wound so that the normal points to
// the positive values.  One corner inside: the triangle of its three edges; two: the quad of the four mixed edges, split along its first diagonal;
// the complement of a case is the case reversed.  A negatively oriented tetrahedron swaps the last two corners of each triangle.
__constant__ const uint8_t CASE_TRIS[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
__constant__ const uint8_t CASE_EDGE[16][6] = {
    {0, 0, 0, 0, 0, 0}, {0, 1, 2, 0, 0, 0}, {0, 4, 3, 0, 0, 0}, {4, 3, 1, 4, 1, 2}, {1, 3, 5, 0, 0, 0}, {3, 5, 2, 3, 2, 0},
    {5, 1, 0, 5, 0, 4}, {2, 4, 5, 0, 0, 0}, {2, 5, 4, 0, 0, 0}, {5, 4, 0, 5, 0, 1}, {2, 5, 3, 2, 3, 0}, {1, 5, 3, 0, 0, 0},
    {4, 2, 1, 4, 1, 3}, {0, 3, 4, 0, 0, 0}, {0, 2, 1, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};

struct MeshVolumeK {
  const float* values;
  const float* weights;
  int X, Y, Z;
  uint32_t N;
  int observed_only;
  __device__ inline uint32_t at(int i, int j, int k) const { return ((uint32_t)i * Y + j) * Z + k; }
  __device__ inline float value(int i, int j, int k) const {  // clamp(values, -1, 1); a NaN stays one and counts as outside
    const float v = values[at(i, j, k)];
    return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
  }
  __device__ inline bool has_cells() const { return X > 1 && Y > 1 && Z > 1; }
  // the cell whose lowest corner is (i, j, k): inside the volume and, with observed_only, every corner observed
  __device__ inline bool cell(int i, int j, int k) const {
    if (i < 0 || j < 0 || k < 0 || i > X - 2 || j > Y - 2 || k > Z - 2) return false;
    if (!observed_only) return true;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) ok = ok && weights[at(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2))] > 0.0f;
    return ok;
  }
  // whether any cell around the edge of direction `mask` at (i, j, k) is emitted (without observed_only every edge inside the volume has one)
  __device__ inline bool edge_used(int i, int j, int k, int mask) const {
    if (!observed_only) return true;
    const int fx = (mask & 1) ? 0 : 1, fy = (mask & 2) ? 0 : 1, fz = (mask & 4) ? 0 : 1;
    for (int a = 0; a <= fx; ++a)
      for (int b = 0; b <= fy; ++b)
        for (int c = 0; c <= fz; ++c)
          if (cell(i - a, j - b, k - c)) return true;
    return false;
  }
};

__device__ inline void mesh_ijk(const MeshVolumeK& v, uint32_t p, int& i, int& j, int& k) {
  k = (int)(p % (uint32_t)v.Z);
  const uint32_t t = p / (uint32_t)v.Z;
  j = (int)(t % (uint32_t)v.Y), i = (int)(t / (uint32_t)v.Y);
}

// bit q: the edge of kind q at lattice point (i, j, k) crosses zero and carries a vertex
__device__ inline uint32_t mesh_edge_flags(const MeshVolumeK& v, int i, int j, int k) {
  if (!v.has_cells()) return 0u;
  const bool in0 = v.value(i, j, k) < 0.0f;
  uint32_t flags = 0u;
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const int m = KIND_MASK[q], i1 = i + (m & 1), j1 = j + ((m >> 1) & 1), k1 = k + (m >> 2);
    if (i1 >= v.X || j1 >= v.Y || k1 >= v.Z) continue;
    if ((v.value(i1, j1, k1) < 0.0f) != in0 && v.edge_used(i, j, k, m)) flags |= 1u << q;
  }
  return flags;
}

// bit c: corner c of the (emitted) cell at (i, j, k) is inside
__device__ inline uint32_t mesh_cube(const MeshVolumeK& v, int i, int j, int k) {
  uint32_t cube = 0u;
#pragma unroll
  for (int c = 0; c < 8; ++c) cube |= (v.value(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)) < 0.0f ? 1u : 0u) << c;
  return cube;
}
__device__ inline int tet_case(uint32_t cube, int t) {
  return (int)(((cube >> TET_CORNER[t][0]) & 1u) | (((cube >> TET_CORNER[t][1]) & 1u) << 1) | (((cube >> TET_CORNER[t][2]) & 1u) << 2) |
               (((cube >> TET_CORNER[t][3]) & 1u) << 3));
}
__device__ inline int mesh_cell_triangles(uint32_t cube) {
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) n += CASE_TRIS[tet_case(cube, t)];
  return n;
}

// exclusive prefix of v over the block's threads (every thread calls it), the block's sum in `total`
__device__ inline int block_excl_scan(int v, int& total) {
  __shared__ int wave_sum[MB / TN_WAVE];
  const int lane = tn_lane(), wave = threadIdx.x / TN_WAVE;
  int incl = v;
#pragma unroll
  for (int o = 1; o < TN_WAVE; o <<= 1) {
    const int t = __shfl_up(incl, o, TN_WAVE);
    if (lane >= o) incl += t;
  }
  __syncthreads();  // a second call of the same kernel reuses wave_sum
  if (lane == TN_WAVE - 1) wave_sum[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int x = 0; x < MB / TN_WAVE; ++x) {
    if (x < wave) before += wave_sum[x];
    all += wave_sum[x];
  }
  total = all;
  return before + incl - v;
}

__global__ void __launch_bounds__(MB) k_mesh_count(MeshVolumeK v, uint8_t* __restrict__ flags, int32_t* __restrict__ block_v, int32_t* __restrict__ block_f) {
  const uint32_t p = blockIdx.x * MB + threadIdx.x;
  int nv = 0, nf = 0;
  if (p < v.N) {
    int i, j, k;
    mesh_ijk(v, p, i, j, k);
    const uint32_t f = mesh_edge_flags(v, i, j, k);
    flags[p] = (uint8_t)f;
    nv = __popc(f);
    if (v.cell(i, j, k)) nf = mesh_cell_triangles(mesh_cube(v, i, j, k));
  }
  int tv, tf;
  block_excl_scan(nv, tv);
  block_excl_scan(nf, tf);
  if (threadIdx.x == 0) block_v[blockIdx.x] = tv, block_f[blockIdx.x] = tf;
}

// ONE block: the exclusive scans of the two block counts, and the totals
__global__ void __launch_bounds__(MB) k_mesh_offsets(const int32_t* __restrict__ block_v, const int32_t* __restrict__ block_f, int64_t num_blocks,
                                                     int64_t* __restrict__ off_v, int64_t* __restrict__ off_f, int64_t* __restrict__ totals) {
  int64_t carry_v = 0, carry_f = 0;  // the same in every thread
  for (int64_t b0 = 0; b0 < num_blocks; b0 += MB) {
    const int64_t b = b0 + threadIdx.x;
    const int cv = b < num_blocks ? block_v[b] : 0, cf = b < num_blocks ? block_f[b] : 0;  // <= 7 * 256 and 12 * 256 per block: the chunk sums fit an int
    int tv, tf;
    const int ev = block_excl_scan(cv, tv);
    const int ef = block_excl_scan(cf, tf);
    if (b < num_blocks) off_v[b] = carry_v + ev, off_f[b] = carry_f + ef;
    carry_v += tv, carry_f += tf;
  }
  if (threadIdx.x == 0) totals[0] = carry_v, totals[1] = carry_f;
}

struct MeshOutK {
  float ox, oy, oz, sx, sy, sz;
  const float4* rgbt;
  float* vertices;
  float* normals;
  float4* out_rgbt;
  int64_t cap_v;
  int32_t* faces;
  int64_t cap_f;
};

// d clamp(values) / d index along one axis at n of `dim` lattice points: central, one-sided at the border, 0 on an axis of one point
__device__ inline float mesh_diff(float lo, float mid, float hi, int n, int dim) {
  if (dim == 1) return 0.0f;
  if (n == 0) return hi - mid;
  if (n == dim - 1) return mid - lo;
  return (hi - lo) * 0.5f;
}
__device__ inline void mesh_gradient(const MeshVolumeK& v, const MeshOutK& o, int i, int j, int k, float& gx, float& gy, float& gz) {
  const float mid = v.value(i, j, k);
  const float xl = i > 0 ? v.value(i - 1, j, k) : mid, xh = i < v.X - 1 ? v.value(i + 1, j, k) : mid;
  const float yl = j > 0 ? v.value(i, j - 1, k) : mid, yh = j < v.Y - 1 ? v.value(i, j + 1, k) : mid;
  const float zl = k > 0 ? v.value(i, j, k - 1) : mid, zh = k < v.Z - 1 ? v.value(i, j, k + 1) : mid;
  gx = mesh_diff(xl, mid, xh, i, v.X) / o.sx;
  gy = mesh_diff(yl, mid, yh, j, v.Y) / o.sy;
  gz = mesh_diff(zl, mid, zh, k, v.Z) / o.sz;
}

// the vertices of every lattice point's flagged edges, and the index of each point's first vertex
__global__ void __launch_bounds__(MB) k_mesh_vertices(MeshVolumeK v, MeshOutK o, const uint8_t* __restrict__ flags, const int64_t* __restrict__ off_v,
                                                      int32_t* __restrict__ vbase) {
  const uint32_t p = blockIdx.x * MB + threadIdx.x;
  const uint32_t f = p < v.N ? flags[p] : 0u;
  int total;
  const int64_t first = off_v[blockIdx.x] + block_excl_scan(__popc(f), total);
  if (p >= v.N) return;
  vbase[p] = (int32_t)first;
  if (f == 0u) return;
  int i, j, k;
  mesh_ijk(v, p, i, j, k);
  const float a = v.value(i, j, k);
  float g0x, g0y, g0z;
  mesh_gradient(v, o, i, j, k, g0x, g0y, g0z);
  int64_t row = first;
  for (int q = 0; q < 7; ++q) {
    if (!((f >> q) & 1u)) continue;
    const int64_t r = row++;
    if (r < 0 || r >= o.cap_v) return;  // (negative: a workspace tn_mesh_count never filled)
    const int m = KIND_MASK[q], i1 = i + (m & 1), j1 = j + ((m >> 1) & 1), k1 = k + (m >> 2);
    const float b = v.value(i1, j1, k1);
    const float t = a / (a - b);  // the signs differ: a - b is not zero, 0 <= t <= 1
    o.vertices[3 * r] = o.ox + ((float)i + ((m & 1) ? t : 0.0f)) * o.sx;
    o.vertices[3 * r + 1] = o.oy + ((float)j + ((m & 2) ? t : 0.0f)) * o.sy;
    o.vertices[3 * r + 2] = o.oz + ((float)k + ((m & 4) ? t : 0.0f)) * o.sz;
    float g1x, g1y, g1z;
    mesh_gradient(v, o, i1, j1, k1, g1x, g1y, g1z);
    const float gx = g0x + t * (g1x - g0x), gy = g0y + t * (g1y - g0y), gz = g0z + t * (g1z - g0z);
    const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
    const bool flat = !(len > 0.0f);
    o.normals[3 * r] = flat ? 0.0f : gx / len;
    o.normals[3 * r + 1] = flat ? 0.0f : gy / len;
    o.normals[3 * r + 2] = flat ? 0.0f : gz / len;
    const uint32_t p1 = v.at(i1, j1, k1);
    uint32_t src = t <= 0.5f ? p : p1;  // the nearer end point, a tie takes the first
    if (!(v.weights[src] > 0.0f)) src = src == p ? p1 : p;  // unobserved: the other
    o.out_rgbt[r] = o.rgbt[src];
  }
}

// the triangles of every emitted cell, as indices of the vertices k_mesh_vertices wrote
__global__ void __launch_bounds__(MB) k_mesh_faces(MeshVolumeK v, MeshOutK o, const uint8_t* __restrict__ flags, const int32_t* __restrict__ vbase,
                                                   const int64_t* __restrict__ off_f) {
  const uint32_t p = blockIdx.x * MB + threadIdx.x;
  int i = 0, j = 0, k = 0, nf = 0;
  uint32_t cube = 0u;
  if (p < v.N) {
    mesh_ijk(v, p, i, j, k);
    if (v.cell(i, j, k)) {
      cube = mesh_cube(v, i, j, k);
      nf = mesh_cell_triangles(cube);
    }
  }
  int total;
  int64_t row = off_f[blockIdx.x] + block_excl_scan(nf, total);
  if (nf == 0) return;
  for (int t = 0; t < 6; ++t) {
    const int cs = tet_case(cube, t);
    for (int n = 0; n < CASE_TRIS[cs]; ++n) {
      const int64_t r = row++;
      if (r < 0 || r >= o.cap_f) return;
      int32_t idx[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int edge = CASE_EDGE[cs][3 * n + e];
        const int lo = TET_CORNER[t][TET_EDGE[edge][0]], hi = TET_CORNER[t][TET_EDGE[edge][1]];
        const uint32_t owner = v.at(i + (lo & 1), j + ((lo >> 1) & 1), k + (lo >> 2));
        const int q = MASK_KIND[hi ^ lo];
        idx[e] = vbase[owner] + __popc((uint32_t)flags[owner] & ((1u << q) - 1u));
      }
      const bool odd = TET_ODD[t] != 0;
      o.faces[3 * r] = idx[0], o.faces[3 * r + 1] = odd ? idx[2] : idx[1], o.faces[3 * r + 2] = odd ? idx[1] : idx[2];
    }
  }
}

struct MeshLayout {
  int64_t flags, vbase, block_v, block_f, off_v, off_f, total;
};
MeshLayout mesh_layout(int64_t n) {
  const int64_t nb = tn_cdiv(n, MB);
  MeshLayout L;
  L.flags = 0;
  L.vbase = L.flags + align256(n);
  L.block_v = L.vbase + align256(n * 4);
  L.block_f = L.block_v + align256(nb * 4);
  L.off_v = L.block_f + align256(nb * 4);
  L.off_f = L.off_v + align256(nb * 8);
  L.total = L.off_f + align256(nb * 8);
  return L;
}

bool dims_ok(int32_t X, int32_t Y, int32_t Z) { return X >= 1 && Y >= 1 && Z >= 1 && (int64_t)X * Y <= MESH_MAX_POINTS && (int64_t)X * Y * Z <= MESH_MAX_POINTS; }
bool positive(float v) { return v > 0.0f && v <= 3.4028234663852886e38f; }
bool finite3(float a, float b, float c) { return a - a == 0.0f && b - b == 0.0f && c - c == 0.0f; }

}  // namespace

extern "C" int tn_tsdf_integrate(float* values, float* weights, float* rgbt, int32_t X, int32_t Y, int32_t Z, float origin_x, float origin_y,
                                 float origin_z, float voxel_x, float voxel_y, float voxel_z, float truncation, float max_weight, const float* depth,
                                 const float* frame_rgbt, const float* accumulation, float min_accumulation, const float* cameras, int32_t num_frames,
                                 int32_t height, int32_t width, int32_t ray_depth, tn_stream_t stream) {
  TN_REQUIRE(dims_ok(X, Y, Z), "tn_tsdf_integrate: a volume of %d x %d x %d voxels (each >= 1, below 2^31 in all)", X, Y, Z);
  TN_REQUIRE(num_frames >= 0 && height >= 1 && width >= 1 && height <= (1 << 15) && width <= (1 << 15),
             "tn_tsdf_integrate: %d frames of %d x %d pixels (sizes 1..32768)", num_frames, height, width);
  TN_REQUIRE(finite3(origin_x, origin_y, origin_z) && positive(voxel_x) && positive(voxel_y) && positive(voxel_z),
             "tn_tsdf_integrate: the origin must be finite and the voxel size positive and finite");
  TN_REQUIRE(positive(truncation) && max_weight > 0.0f, "tn_tsdf_integrate: truncation = %g (positive, finite) and max_weight = %g (positive)",
             (double)truncation, (double)max_weight);
  TN_REQUIRE(ray_depth == 0 || ray_depth == 1, "tn_tsdf_integrate: ray_depth = %d (0: camera z, 1: distance along the ray)", ray_depth);
  if (num_frames == 0) return TN_OK;
  TN_REQUIRE(values && weights && rgbt && depth && frame_rgbt && cameras, "tn_tsdf_integrate: null pointer");
  TN_REQUIRE(((uintptr_t)rgbt & 15) == 0 && ((uintptr_t)frame_rgbt & 15) == 0, "tn_tsdf_integrate: the two rgbt arrays must be 16-byte aligned");
  const int64_t N = (int64_t)X * Y * Z;
  TsdfVolumeK vol{values, weights, reinterpret_cast<float4*>(rgbt), (uint32_t)N, (uint32_t)Y, (uint32_t)Z, origin_x, origin_y, origin_z,
                  voxel_x, voxel_y, voxel_z, truncation, max_weight};
  TsdfFramesK fr{depth, reinterpret_cast<const float4*>(frame_rgbt), accumulation, cameras, min_accumulation, num_frames, height, width, ray_depth};
  hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)tn_cdiv(N, MB)), dim3(MB), 0, tn_s(stream), vol, fr);
  TN_CHECK_LAUNCH("tn_tsdf_integrate");
  return TN_OK;
}

extern "C" int64_t tn_mesh_workspace_bytes(int32_t X, int32_t Y, int32_t Z) {
  if (!dims_ok(X, Y, Z)) return -1;
  return mesh_layout((int64_t)X * Y * Z).total;
}

extern "C" int tn_mesh_count(const float* values, const float* weights, int32_t X, int32_t Y, int32_t Z, int32_t observed_only, int64_t* totals,
                             void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  TN_REQUIRE(dims_ok(X, Y, Z), "tn_mesh_count: a volume of %d x %d x %d points (each >= 1, below 2^31 in all)", X, Y, Z);
  TN_REQUIRE(values && weights && totals && workspace, "tn_mesh_count: null pointer");
  const int64_t N = (int64_t)X * Y * Z;
  const MeshLayout L = mesh_layout(N);
  TN_REQUIRE(workspace_bytes >= L.total, "tn_mesh_count: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  char* ws = static_cast<char*>(workspace);
  const int64_t nb = tn_cdiv(N, MB);
  const MeshVolumeK v{values, weights, X, Y, Z, (uint32_t)N, observed_only != 0};
  int32_t* block_v = reinterpret_cast<int32_t*>(ws + L.block_v);
  int32_t* block_f = reinterpret_cast<int32_t*>(ws + L.block_f);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_mesh_count, dim3((unsigned)nb), dim3(MB), 0, st, v, reinterpret_cast<uint8_t*>(ws + L.flags), block_v, block_f);
  TN_CHECK_LAUNCH("tn_mesh_count(count)");
  hipLaunchKernelGGL(k_mesh_offsets, dim3(1), dim3(MB), 0, st, block_v, block_f, nb, reinterpret_cast<int64_t*>(ws + L.off_v),
                     reinterpret_cast<int64_t*>(ws + L.off_f), totals);
  TN_CHECK_LAUNCH("tn_mesh_count(offsets)");
  return TN_OK;
}

extern "C" int tn_mesh_emit(const float* values, const float* weights, const float* rgbt, int32_t X, int32_t Y, int32_t Z, int32_t observed_only,
                            float origin_x, float origin_y, float origin_z, float voxel_x, float voxel_y, float voxel_z, float* vertices,
                            float* normals, float* out_rgbt, int64_t num_vertices, int32_t* faces, int64_t num_faces, void* workspace,
                            int64_t workspace_bytes, tn_stream_t stream) {
  TN_REQUIRE(dims_ok(X, Y, Z), "tn_mesh_emit: a volume of %d x %d x %d points (each >= 1, below 2^31 in all)", X, Y, Z);
  TN_REQUIRE(num_vertices >= 0 && num_vertices <= MESH_MAX_POINTS && num_faces >= 0, "tn_mesh_emit: %lld vertices (0..2^31 - 1) and %lld faces",
             (long long)num_vertices, (long long)num_faces);
  TN_REQUIRE(finite3(origin_x, origin_y, origin_z) && positive(voxel_x) && positive(voxel_y) && positive(voxel_z),
             "tn_mesh_emit: the origin must be finite and the voxel size positive and finite");
  TN_REQUIRE(values && weights && rgbt && workspace, "tn_mesh_emit: null pointer");
  TN_REQUIRE(num_vertices == 0 || (vertices && normals && out_rgbt), "tn_mesh_emit: null pointer (outputs of %lld vertices)", (long long)num_vertices);
  TN_REQUIRE(num_faces == 0 || faces, "tn_mesh_emit: null pointer (an output of %lld faces)", (long long)num_faces);
  TN_REQUIRE(((uintptr_t)rgbt & 15) == 0 && ((uintptr_t)out_rgbt & 15) == 0, "tn_mesh_emit: the two rgbt arrays must be 16-byte aligned");
  const int64_t N = (int64_t)X * Y * Z;
  const MeshLayout L = mesh_layout(N);
  TN_REQUIRE(workspace_bytes >= L.total, "tn_mesh_emit: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  if (num_vertices == 0 && num_faces == 0) return TN_OK;
  char* ws = static_cast<char*>(workspace);
  const int64_t nb = tn_cdiv(N, MB);
  const MeshVolumeK v{values, weights, X, Y, Z, (uint32_t)N, observed_only != 0};
  const MeshOutK o{origin_x, origin_y, origin_z, voxel_x, voxel_y, voxel_z, reinterpret_cast<const float4*>(rgbt), vertices, normals,
                   reinterpret_cast<float4*>(out_rgbt), num_vertices, faces, num_faces};
  const uint8_t* flags = reinterpret_cast<const uint8_t*>(ws + L.flags);
  int32_t* vbase = reinterpret_cast<int32_t*>(ws + L.vbase);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_mesh_vertices, dim3((unsigned)nb), dim3(MB), 0, st, v, o, flags, reinterpret_cast<const int64_t*>(ws + L.off_v), vbase);
  TN_CHECK_LAUNCH("tn_mesh_emit(vertices)");
  hipLaunchKernelGGL(k_mesh_faces, dim3((unsigned)nb), dim3(MB), 0, st, v, o, flags, vbase, reinterpret_cast<const int64_t*>(ws + L.off_f));
  TN_CHECK_LAUNCH("tn_mesh_emit(faces)");
  return TN_OK;
}
