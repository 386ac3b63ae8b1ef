// Mesh simplification to a face budget by vertex clustering (Rossignac-Borrel clustering, the representative placed by Lindstrom's quadric rule):
// what stands where the reference's mesh export runs pymeshlab's quadric edge collapse (exporter_utils.py: get_mesh_from_filename with
// target_num_faces).  The algorithm is not pymeshlab's and no parity with it is claimed.
//
// THE ALGORITHM (tests/mesh_simplify_functional.py restates it in float64, operation by operation)
//   inputs    vertices [V,3], faces [F,3] int32, normals [V,3], rgbt [V,4]; a cell grid: origin (3 floats), cell (3 floats > 0), dims (3 ints, their
//             product below 2^31); a regularization (float).
//   cell      per axis i = floor((v - origin) / cell) in fp32 (IEEE subtraction, division and floor), clamped to [0, dims - 1] (a NaN goes to 0);
//             key = (ix * dims_y + iy) * dims_z + iz.
//   clusters  the vertices of one key; numbered in ascending key order.
//   position  all in double, relative to the cell's centre c = origin + (i + 0.5) * cell (every term converted to double first):
//             for every input face in ascending face index, e1 = p1 - p0, e2 = p2 - p0 (the doubles of the fp32 vertices), n = e1 x e2,
//             d = (n.x q.x + n.y q.y) + n.z q.z with q = p0 - c: A += n n^T and b += d n in the cluster of each of its three corners (a face with two
//             corners in a cluster contributes twice, with three thrice).  This is Lindstrom's area^2-weighted plane quadric.
//             m = the mean of the cluster's v - c in ascending vertex index; eps = regularization * ((Axx + Ayy) + Azz);
//             x solves (A + eps I) x = b + eps m by an LDL^T factorisation (solve_ldlt below: divisions only);
//             x = m where the trace is 0, and where x lies outside the closed cell (|x| <= 0.500001 cell fails on an axis: Lindstrom's rule, with
//             a margin of 1e-6 cell, see CELL_REACH -- a NaN lands here too); the vertex is c + x, rounded to fp32 once.
//   attributes rgbt = the mean of the cluster's rgbt in double, rounded once; normal = the sum of the cluster's normals in double over its length
//             (the square root of (x x + y y) + z z), zero where that length is not positive.
//   faces     indices become clusters; a face with two equal clusters is dropped; of the faces that name the same three clusters in any order only
//             the one with the lowest input index survives; survivors keep the input order.  A cluster no surviving face names is not emitted, the
//             others are renumbered in key order.  A face with an index outside [0, V) is dropped and adds to no quadric.
//
// THE LAUNCHES (no floating-point atomics and no atomics at all: every order is a stable sort's or a prefix sum's, two runs give the same bits)
//   tn_mesh_simplify_count   keys; one pass over the faces that counts those with three different keys per block; one block sums the blocks
//   tn_mesh_simplify_plan    keys; rocprim radix sort of (key, vertex) on the bits dims needs; segment heads, their scan = cluster ids;
//                            corner records (cluster, 3 face + corner), stable sort by cluster: a cluster's corners come out in face order;
//                            faces sorted by their largest cluster, then (stable) by the (smallest, middle) pair: the first of each run of equal
//                            triples survives; plain stores mark the clusters the survivors name; two scans give the output rows; the two totals
//   tn_mesh_simplify_emit    a thread per cluster walks its vertex segment and its corner segment with the sums in registers, solves and writes;
//                            a thread per face writes the survivors
#include "tn_common.h"

#include <string.h>

#include <rocprim/rocprim.hpp>

#include <algorithm>

namespace {

constexpr int SB = 256;             // threads per block
constexpr int COUNT_BLOCKS = 1024;  // blocks of the counting pass (grid stride)
constexpr int64_t SIMPLIFY_MAX = (1ll << 31) - 1;
// How far from its cell's centre, in cells, a solved vertex may lie: half a cell and a margin of 1e-6 cell.  The margin is there for meshes whose
// vertices sit exactly ON cell borders -- a TSDF's shell between observed free space (+1) and the unobserved fill (-1) crosses every lattice edge
// at t = 0.5, which is a border of the lattice-centred grid the export uses: such a vertex belongs to its cell by the key's rounding alone, the
// planes of its cluster pass through the border, and so does the solved point, to a few 1e-17.  Without the margin the rule would be decided there by
// the last bit of the solve.
constexpr double CELL_REACH = 0.500001;

constexpr int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }

struct SimplifyGridK {
  float ox, oy, oz, cx, cy, cz;
  int dx, dy, dz;
};

__device__ inline int cell_index(float v, float o, float c, int d) {
  const float t = floorf((v - o) / c);
  if (!(t > 0.0f)) return 0;  // below the grid, or a NaN
  return (double)t >= (double)(d - 1) ? d - 1 : (int)t;
}

__global__ void __launch_bounds__(SB) k_simplify_keys(const float* __restrict__ vertices, int64_t V, SimplifyGridK g, uint32_t* __restrict__ keys) {
  const int64_t v = (int64_t)blockIdx.x * SB + threadIdx.x;
  if (v >= V) return;
  const uint32_t ix = (uint32_t)cell_index(vertices[3 * v], g.ox, g.cx, g.dx), iy = (uint32_t)cell_index(vertices[3 * v + 1], g.oy, g.cy, g.dy),
                 iz = (uint32_t)cell_index(vertices[3 * v + 2], g.oz, g.cz, g.dz);
  keys[v] = (ix * (uint32_t)g.dy + iy) * (uint32_t)g.dz + iz;
}

// the three vertices of face f, or false where one lies outside [0, V)
__device__ inline bool face_vertices(const int32_t* __restrict__ faces, int64_t f, int64_t V, int32_t& i0, int32_t& i1, int32_t& i2) {
  i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  return (int64_t)(uint32_t)i0 < V && (int64_t)(uint32_t)i1 < V && (int64_t)(uint32_t)i2 < V;
}

// ---------------------------------------------------------------------------------------------------- the count
__device__ inline long long block_sum(long long v) {  // the block's sum, in every thread of wave 0
  __shared__ long long wave_sum[SB / TN_WAVE];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, TN_WAVE);
  if (tn_lane() == 0) wave_sum[threadIdx.x / TN_WAVE] = v;
  __syncthreads();
  long long all = 0;
#pragma unroll
  for (int x = 0; x < SB / TN_WAVE; ++x) all += wave_sum[x];
  return all;
}

__global__ void __launch_bounds__(SB) k_simplify_count_partial(const int32_t* __restrict__ faces, int64_t F, int64_t V, const uint32_t* __restrict__ keys,
                                                               int64_t* __restrict__ partial) {
  long long n = 0;
  for (int64_t f = (int64_t)blockIdx.x * SB + threadIdx.x; f < F; f += (int64_t)gridDim.x * SB) {
    int32_t i0, i1, i2;
    if (!face_vertices(faces, f, V, i0, i1, i2)) continue;
    const uint32_t a = keys[i0], b = keys[i1], c = keys[i2];
    n += (a != b && b != c && a != c) ? 1 : 0;
  }
  const long long all = block_sum(n);
  if (threadIdx.x == 0) partial[blockIdx.x] = all;
}

__global__ void __launch_bounds__(SB) k_simplify_count_final(const int64_t* __restrict__ partial, int num, int64_t* __restrict__ count) {
  long long n = 0;
  for (int i = threadIdx.x; i < num; i += SB) n += partial[i];
  const long long all = block_sum(n);
  if (threadIdx.x == 0) count[0] = all;
}

// ---------------------------------------------------------------------------------------------------- the plan
struct SimplifyWs {  // views of the workspace
  uint32_t *keys, *keys_sorted;
  int32_t *vorder, *vflag, *vscan, *cluster_of, *vstart, *newid;
  uint32_t *ckeys, *ckeys_sorted;
  int32_t* cvals;
  uint32_t *hi, *hi_sorted;
  int32_t* ord1;
  uint64_t *pair, *pair_sorted;
  int32_t *ord2, *keep, *fscan;
  int64_t* partial;
  int64_t* meta;  // [0]: the number of clusters
  void* tmp;
};

// vflag[i]: sorted vertex i opens a cluster
__global__ void __launch_bounds__(SB) k_simplify_heads(const uint32_t* __restrict__ keys_sorted, int64_t V, int32_t* __restrict__ vflag) {
  const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
  if (i >= V) return;
  vflag[i] = (i == 0 || keys_sorted[i] != keys_sorted[i - 1]) ? 1 : 0;
}

// the cluster of every vertex, the first sorted vertex of every cluster (and one past the last cluster's), the number of clusters
__global__ void __launch_bounds__(SB) k_simplify_clusters_of(const int32_t* __restrict__ vorder, const int32_t* __restrict__ vflag,
                                                             const int32_t* __restrict__ vscan, int64_t V, int32_t* __restrict__ cluster_of,
                                                             int32_t* __restrict__ vstart, int64_t* __restrict__ meta) {
  const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
  if (i >= V) return;
  const int32_t c = vscan[i] - 1;
  cluster_of[vorder[i]] = c;
  if (vflag[i]) vstart[c] = (int32_t)i;
  if (i == V - 1) vstart[c + 1] = (int32_t)V, meta[0] = c + 1;
}

// corner records: the cluster of corner r = 3 f + k (V, past every cluster, for a face with an index out of range)
__global__ void __launch_bounds__(SB) k_simplify_corners(const int32_t* __restrict__ faces, int64_t F, int64_t V, const int32_t* __restrict__ cluster_of,
                                                         uint32_t* __restrict__ ckeys) {
  const int64_t f = (int64_t)blockIdx.x * SB + threadIdx.x;
  if (f >= F) return;
  int32_t i0, i1, i2;
  const bool ok = face_vertices(faces, f, V, i0, i1, i2);
  ckeys[3 * f] = ok ? (uint32_t)cluster_of[i0] : (uint32_t)V;
  ckeys[3 * f + 1] = ok ? (uint32_t)cluster_of[i1] : (uint32_t)V;
  ckeys[3 * f + 2] = ok ? (uint32_t)cluster_of[i2] : (uint32_t)V;
}

// the clusters of face f sorted: lo <= mid <= hi (all 0, a dropped face, where an index is out of range)
__device__ inline void face_triple(const uint32_t* __restrict__ ckeys, int64_t f, int64_t V, uint32_t& lo, uint32_t& mid, uint32_t& hi) {
  uint32_t a = ckeys[3 * f], b = ckeys[3 * f + 1], c = ckeys[3 * f + 2];
  if ((int64_t)a >= V) a = b = c = 0u;
  lo = min(a, min(b, c)), hi = max(a, max(b, c));
  mid = a ^ b ^ c ^ lo ^ hi;
}

__global__ void __launch_bounds__(SB) k_simplify_face_hi(const uint32_t* __restrict__ ckeys, int64_t F, int64_t V, uint32_t* __restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * SB + threadIdx.x;
  if (f >= F) return;
  uint32_t lo, mid, hi;
  face_triple(ckeys, f, V, lo, mid, hi);
  out[f] = hi;
}

__global__ void __launch_bounds__(SB) k_simplify_face_pair(const uint32_t* __restrict__ ckeys, int64_t F, int64_t V, const int32_t* __restrict__ ord1,
                                                           int bits, uint64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
  if (i >= F) return;
  uint32_t lo, mid, hi;
  face_triple(ckeys, ord1[i], V, lo, mid, hi);
  out[i] = ((uint64_t)lo << bits) | (uint64_t)mid;
}

// keep[f]: face f survives (three different clusters, and the first of its run in (lo, mid, hi) order); the clusters of the survivors are marked
__global__ void __launch_bounds__(SB) k_simplify_face_heads(const uint32_t* __restrict__ ckeys, int64_t F, int64_t V, const int32_t* __restrict__ ord2,
                                                            int32_t* __restrict__ keep, int32_t* __restrict__ ref) {
  const int64_t i = (int64_t)blockIdx.x * SB + threadIdx.x;
  if (i >= F) return;
  const int32_t f = ord2[i];
  uint32_t lo, mid, hi;
  face_triple(ckeys, f, V, lo, mid, hi);
  bool k = lo != mid && mid != hi;
  if (k && i > 0) {
    uint32_t plo, pmid, phi;
    face_triple(ckeys, ord2[i - 1], V, plo, pmid, phi);
    k = plo != lo || pmid != mid || phi != hi;
  }
  keep[f] = k ? 1 : 0;
  if (k) ref[lo] = 1, ref[mid] = 1, ref[hi] = 1;  // plain stores of the same word
}

__global__ void k_simplify_totals(const int32_t* __restrict__ newid, int64_t V, const int32_t* __restrict__ fscan, int64_t F, int64_t* __restrict__ totals) {
  if (threadIdx.x == 0 && blockIdx.x == 0) totals[0] = (V > 0 && F > 0) ? newid[V - 1] : 0, totals[1] = (V > 0 && F > 0) ? fscan[F - 1] : 0;
}

// ---------------------------------------------------------------------------------------------------- the emit
struct SimplifyOutK {
  float* vertices;
  float* normals;
  float4* rgbt;
  int64_t cap_v;
  int32_t* faces;
  int64_t cap_f;
};

// (A + eps I) x = r for the symmetric positive definite A + eps I, by LDL^T, in this order
__device__ inline void solve_ldlt(double m00, double m01, double m02, double m11, double m12, double m22, double r0, double r1, double r2, double& x0,
                                  double& x1, double& x2) {
  const double l10 = m01 / m00, l20 = m02 / m00;
  const double d1 = m11 - l10 * m01;
  const double t = m12 - l20 * m01;
  const double l21 = t / d1;
  const double d2 = (m22 - l20 * m02) - l21 * t;
  const double y1 = r1 - l10 * r0;
  const double y2 = (r2 - l20 * r0) - l21 * y1;
  x2 = y2 / d2;
  x1 = y1 / d1 - l21 * x2;
  x0 = (r0 / m00 - l10 * x1) - l20 * x2;
}

__global__ void __launch_bounds__(SB) k_simplify_emit_clusters(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                               const float4* __restrict__ rgbt, int64_t V, const int32_t* __restrict__ faces, int64_t F,
                                                               SimplifyGridK g, double reg, SimplifyWs w, SimplifyOutK o) {
  const int64_t c = (int64_t)blockIdx.x * SB + threadIdx.x;
  const int64_t C = w.meta[0];
  if (c >= C || c >= V || w.vflag[c] == 0) return;  // (vflag holds the marks of the referenced clusters by now)
  const int64_t row = (int64_t)w.newid[c] - 1;
  const int64_t v0 = w.vstart[c], v1 = w.vstart[c + 1];
  if (row < 0 || row >= o.cap_v || v0 < 0 || v1 > V || v0 >= v1) return;  // (a workspace the plan never filled)
  const uint32_t key = w.keys_sorted[v0];
  const uint32_t iz = key % (uint32_t)g.dz, t = key / (uint32_t)g.dz, iy = t % (uint32_t)g.dy, ix = t / (uint32_t)g.dy;
  const double ccx = (double)g.ox + ((double)ix + 0.5) * (double)g.cx, ccy = (double)g.oy + ((double)iy + 0.5) * (double)g.cy,
               ccz = (double)g.oz + ((double)iz + 0.5) * (double)g.cz;
  // the vertex segment: mean position, normals, RGB+T
  double mx = 0.0, my = 0.0, mz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0, cr = 0.0, cg = 0.0, cb = 0.0, ct = 0.0;
  for (int64_t i = v0; i < v1; ++i) {
    const int64_t v = w.vorder[i];
    if (v < 0 || v >= V) return;
    mx += (double)vertices[3 * v] - ccx, my += (double)vertices[3 * v + 1] - ccy, mz += (double)vertices[3 * v + 2] - ccz;
    nx += (double)normals[3 * v], ny += (double)normals[3 * v + 1], nz += (double)normals[3 * v + 2];
    const float4 s = rgbt[v];
    cr += (double)s.x, cg += (double)s.y, cb += (double)s.z, ct += (double)s.w;
  }
  const double count = (double)(v1 - v0);
  mx /= count, my /= count, mz /= count;
  // the corner segment: the quadric
  const int64_t n3 = 3 * F;
  int64_t lo = 0, hi = n3;  // the first corner record of cluster c
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)w.ckeys_sorted[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  double axx = 0.0, axy = 0.0, axz = 0.0, ayy = 0.0, ayz = 0.0, azz = 0.0, bx = 0.0, by = 0.0, bz = 0.0;
  for (int64_t j = lo; j < n3 && (int64_t)w.ckeys_sorted[j] == c; ++j) {
    const int64_t f = (int64_t)w.cvals[j] / 3;
    if (f < 0 || f >= F) return;
    int32_t i0, i1, i2;
    if (!face_vertices(faces, f, V, i0, i1, i2)) continue;
    const double p0x = (double)vertices[3 * (int64_t)i0], p0y = (double)vertices[3 * (int64_t)i0 + 1], p0z = (double)vertices[3 * (int64_t)i0 + 2];
    const double e1x = (double)vertices[3 * (int64_t)i1] - p0x, e1y = (double)vertices[3 * (int64_t)i1 + 1] - p0y, e1z = (double)vertices[3 * (int64_t)i1 + 2] - p0z;
    const double e2x = (double)vertices[3 * (int64_t)i2] - p0x, e2y = (double)vertices[3 * (int64_t)i2 + 1] - p0y, e2z = (double)vertices[3 * (int64_t)i2 + 2] - p0z;
    const double fx = e1y * e2z - e1z * e2y, fy = e1z * e2x - e1x * e2z, fz = e1x * e2y - e1y * e2x;
    const double d = (fx * (p0x - ccx) + fy * (p0y - ccy)) + fz * (p0z - ccz);
    axx += fx * fx, axy += fx * fy, axz += fx * fz, ayy += fy * fy, ayz += fy * fz, azz += fz * fz;
    bx += d * fx, by += d * fy, bz += d * fz;
  }
  const double trace = (axx + ayy) + azz;
  double x = mx, y = my, z = mz;
  if (trace != 0.0) {
    const double eps = reg * trace;
    double sx, sy, sz;
    solve_ldlt(axx + eps, axy, axz, ayy + eps, ayz, azz + eps, bx + eps * mx, by + eps * my, bz + eps * mz, sx, sy, sz);
    if (fabs(sx) <= CELL_REACH * (double)g.cx && fabs(sy) <= CELL_REACH * (double)g.cy && fabs(sz) <= CELL_REACH * (double)g.cz) x = sx, y = sy, z = sz;
  }
  o.vertices[3 * row] = (float)(ccx + x), o.vertices[3 * row + 1] = (float)(ccy + y), o.vertices[3 * row + 2] = (float)(ccz + z);
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  const bool flat = !(len > 0.0);
  o.normals[3 * row] = flat ? 0.0f : (float)(nx / len), o.normals[3 * row + 1] = flat ? 0.0f : (float)(ny / len),
                  o.normals[3 * row + 2] = flat ? 0.0f : (float)(nz / len);
  o.rgbt[row] = make_float4((float)(cr / count), (float)(cg / count), (float)(cb / count), (float)(ct / count));
}

__global__ void __launch_bounds__(SB) k_simplify_emit_faces(int64_t F, int64_t V, SimplifyWs w, SimplifyOutK o) {
  const int64_t f = (int64_t)blockIdx.x * SB + threadIdx.x;
  if (f >= F || w.keep[f] == 0) return;
  const int64_t row = (int64_t)w.fscan[f] - 1;
  if (row < 0 || row >= o.cap_f) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t c = w.ckeys[3 * f + k];
    o.faces[3 * row + k] = (int64_t)c < V ? w.newid[c] - 1 : -1;
  }
}

// ---------------------------------------------------------------------------------------------------- host
int bit_length(int64_t v) {  // bits that hold 0..v (at least 1)
  int b = 1;
  while ((v >> b) != 0) ++b;
  return b;
}

struct SimplifyLayout {
  int64_t keys, keys_sorted, vorder, vflag, vscan, cluster_of, vstart, newid, ckeys, ckeys_sorted, cvals, hi, hi_sorted, ord1, pair, pair_sorted, ord2,
      keep, fscan, partial, meta, tmp, tmp_bytes, total;
};

// rocprim's scratch.  Its size query needs a device, and the workspace size must not: the layout reserves a bound -- a radix sort of n pairs keeps a
// second copy of the keys and the values and a few bytes of histogram and look-back state per block of some thousand elements; a scan only the
// latter -- and the plan, which runs where a device is, checks rocprim's own figures against it before the first launch.
int64_t sort_scratch_bound(int64_t n, int64_t pair_bytes) { return n * (pair_bytes + 4) + (1ll << 20); }

SimplifyLayout simplify_layout(int64_t V, int64_t F) {
  SimplifyLayout L;
  int64_t at = 0;
  auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at += align256(bytes);
    return here;
  };
  L.keys = take(V * 4), L.keys_sorted = take(V * 4), L.vorder = take(V * 4), L.vflag = take(V * 4), L.vscan = take(V * 4), L.cluster_of = take(V * 4);
  L.vstart = take((V + 1) * 4), L.newid = take(V * 4);
  L.ckeys = take(F * 12), L.ckeys_sorted = take(F * 12), L.cvals = take(F * 12);
  L.hi = take(F * 4), L.hi_sorted = take(F * 4), L.ord1 = take(F * 4), L.pair = take(F * 8), L.pair_sorted = take(F * 8), L.ord2 = take(F * 4);
  L.keep = take(F * 4), L.fscan = take(F * 4);
  L.partial = take(COUNT_BLOCKS * 8), L.meta = take(64);
  L.tmp_bytes = align256(std::max(std::max(sort_scratch_bound(V, 8), sort_scratch_bound(3 * F, 8)), sort_scratch_bound(F, 12)));
  L.tmp = take(L.tmp_bytes);
  L.total = at;
  return L;
}

// whether rocprim's scratch for every sort and scan of the plan fits the layout's bound
bool scratch_fits(int64_t V, int64_t F, const SimplifyLayout& L) {
  const size_t nv = (size_t)V, nf = (size_t)F;
  size_t a = 0, b = 0, c = 0, d = 0, e = 0;
  const bool ok =
      rocprim::radix_sort_pairs(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, rocprim::counting_iterator<int32_t>(0), (int32_t*)nullptr, nv, 0, 31) ==
          hipSuccess &&
      rocprim::radix_sort_pairs(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, rocprim::counting_iterator<int32_t>(0), (int32_t*)nullptr, 3 * nf, 0, 31) ==
          hipSuccess &&
      rocprim::radix_sort_pairs(nullptr, c, (uint64_t*)nullptr, (uint64_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, nf, 0, 62) == hipSuccess &&
      rocprim::inclusive_scan(nullptr, d, (const int32_t*)nullptr, (int32_t*)nullptr, nv, rocprim::plus<int32_t>()) == hipSuccess &&
      rocprim::inclusive_scan(nullptr, e, (const int32_t*)nullptr, (int32_t*)nullptr, nf, rocprim::plus<int32_t>()) == hipSuccess;
  return ok && (int64_t)std::max(std::max(std::max(a, b), std::max(c, d)), e) <= L.tmp_bytes;
}

SimplifyWs simplify_views(void* workspace, const SimplifyLayout& L) {
  char* ws = static_cast<char*>(workspace);
  SimplifyWs w;
  w.keys = reinterpret_cast<uint32_t*>(ws + L.keys), w.keys_sorted = reinterpret_cast<uint32_t*>(ws + L.keys_sorted);
  w.vorder = reinterpret_cast<int32_t*>(ws + L.vorder), w.vflag = reinterpret_cast<int32_t*>(ws + L.vflag);
  w.vscan = reinterpret_cast<int32_t*>(ws + L.vscan), w.cluster_of = reinterpret_cast<int32_t*>(ws + L.cluster_of);
  w.vstart = reinterpret_cast<int32_t*>(ws + L.vstart), w.newid = reinterpret_cast<int32_t*>(ws + L.newid);
  w.ckeys = reinterpret_cast<uint32_t*>(ws + L.ckeys), w.ckeys_sorted = reinterpret_cast<uint32_t*>(ws + L.ckeys_sorted);
  w.cvals = reinterpret_cast<int32_t*>(ws + L.cvals);
  w.hi = reinterpret_cast<uint32_t*>(ws + L.hi), w.hi_sorted = reinterpret_cast<uint32_t*>(ws + L.hi_sorted);
  w.ord1 = reinterpret_cast<int32_t*>(ws + L.ord1);
  w.pair = reinterpret_cast<uint64_t*>(ws + L.pair), w.pair_sorted = reinterpret_cast<uint64_t*>(ws + L.pair_sorted);
  w.ord2 = reinterpret_cast<int32_t*>(ws + L.ord2), w.keep = reinterpret_cast<int32_t*>(ws + L.keep), w.fscan = reinterpret_cast<int32_t*>(ws + L.fscan);
  w.partial = reinterpret_cast<int64_t*>(ws + L.partial), w.meta = reinterpret_cast<int64_t*>(ws + L.meta);
  w.tmp = ws + L.tmp;
  return w;
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 0 && V <= SIMPLIFY_MAX && F >= 0 && 3 * F <= SIMPLIFY_MAX; }
bool positive(float v) { return v > 0.0f && v <= 3.4028234663852886e38f; }
bool finite3(float a, float b, float c) { return a - a == 0.0f && b - b == 0.0f && c - c == 0.0f; }
bool dims_ok(int32_t X, int32_t Y, int32_t Z) { return X >= 1 && Y >= 1 && Z >= 1 && (int64_t)X * Y <= SIMPLIFY_MAX && (int64_t)X * Y * Z <= SIMPLIFY_MAX; }

// what the three entry points share: sizes, grid, the input mesh, the workspace
int simplify_check(const char* name, const float* vertices, int64_t V, const int32_t* faces, int64_t F, float ox, float oy, float oz, float cx, float cy,
                   float cz, int32_t dx, int32_t dy, int32_t dz, const void* workspace, int64_t workspace_bytes, SimplifyLayout& L) {
  TN_REQUIRE(sizes_ok(V, F), "%s: %lld vertices (0..2^31 - 1) and %lld faces (0..(2^31 - 1) / 3)", name, (long long)V, (long long)F);
  TN_REQUIRE(dims_ok(dx, dy, dz), "%s: a grid of %d x %d x %d cells (each >= 1, below 2^31 in all)", name, dx, dy, dz);
  TN_REQUIRE(finite3(ox, oy, oz) && positive(cx) && positive(cy) && positive(cz), "%s: the origin must be finite and the cell size positive and finite",
             name);
  TN_REQUIRE(workspace && (V == 0 || vertices) && (F == 0 || faces), "%s: null pointer", name);
  TN_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)vertices & 3) == 0 && ((uintptr_t)faces & 3) == 0,
             "%s: misaligned pointer (the workspace to 256 bytes, the arrays to their elements)", name);
  L = simplify_layout(V, F);
  TN_REQUIRE(workspace_bytes >= L.total, "%s: workspace of %lld bytes, %lld needed", name, (long long)workspace_bytes, (long long)L.total);
  return TN_OK;
}

unsigned blocks_of(int64_t n) { return (unsigned)tn_cdiv(n, SB); }

}  // namespace

extern "C" int64_t tn_mesh_simplify_workspace_bytes(int64_t num_vertices, int64_t num_faces) {
  if (!sizes_ok(num_vertices, num_faces)) return -1;
  return simplify_layout(num_vertices, num_faces).total;
}

extern "C" int tn_mesh_simplify_count(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces, float origin_x, float origin_y,
                                      float origin_z, float cell_x, float cell_y, float cell_z, int32_t dims_x, int32_t dims_y, int32_t dims_z,
                                      int64_t* count, void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  SimplifyLayout L;
  if (const int rc = simplify_check("tn_mesh_simplify_count", vertices, num_vertices, faces, num_faces, origin_x, origin_y, origin_z, cell_x, cell_y, cell_z,
                                    dims_x, dims_y, dims_z, workspace, workspace_bytes, L))
    return rc;
  TN_REQUIRE(count && ((uintptr_t)count & 7) == 0, "tn_mesh_simplify_count: null or misaligned pointer (count)");
  const SimplifyWs w = simplify_views(workspace, L);
  const SimplifyGridK g{origin_x, origin_y, origin_z, cell_x, cell_y, cell_z, dims_x, dims_y, dims_z};
  hipStream_t st = tn_s(stream);
  int nb = 0;
  if (num_vertices > 0 && num_faces > 0) {
    hipLaunchKernelGGL(k_simplify_keys, dim3(blocks_of(num_vertices)), dim3(SB), 0, st, vertices, num_vertices, g, w.keys);
    TN_CHECK_LAUNCH("tn_mesh_simplify_count(keys)");
    nb = (int)std::min<int64_t>(tn_cdiv(num_faces, SB), COUNT_BLOCKS);
    hipLaunchKernelGGL(k_simplify_count_partial, dim3(nb), dim3(SB), 0, st, faces, num_faces, num_vertices, (const uint32_t*)w.keys, w.partial);
    TN_CHECK_LAUNCH("tn_mesh_simplify_count(partial)");
  }
  hipLaunchKernelGGL(k_simplify_count_final, dim3(1), dim3(SB), 0, st, (const int64_t*)w.partial, nb, count);
  TN_CHECK_LAUNCH("tn_mesh_simplify_count(final)");
  return TN_OK;
}

extern "C" int tn_mesh_simplify_plan(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces, float origin_x, float origin_y,
                                     float origin_z, float cell_x, float cell_y, float cell_z, int32_t dims_x, int32_t dims_y, int32_t dims_z,
                                     int64_t* totals, void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  SimplifyLayout L;
  if (const int rc = simplify_check("tn_mesh_simplify_plan", vertices, num_vertices, faces, num_faces, origin_x, origin_y, origin_z, cell_x, cell_y, cell_z,
                                    dims_x, dims_y, dims_z, workspace, workspace_bytes, L))
    return rc;
  TN_REQUIRE(totals && ((uintptr_t)totals & 7) == 0, "tn_mesh_simplify_plan: null or misaligned pointer (totals)");
  const int64_t V = num_vertices, F = num_faces;
  const SimplifyWs w = simplify_views(workspace, L);
  const SimplifyGridK g{origin_x, origin_y, origin_z, cell_x, cell_y, cell_z, dims_x, dims_y, dims_z};
  hipStream_t st = tn_s(stream);
  if (V > 0 && F > 0) {
    if (!scratch_fits(V, F, L)) {
      tn_set_error("tn_mesh_simplify_plan: rocprim's scratch for %lld vertices and %lld faces does not fit the %lld bytes reserved for it", (long long)V,
                   (long long)F, (long long)L.tmp_bytes);
      return TN_ELAUNCH;
    }
    size_t tb = (size_t)L.tmp_bytes;
    const int key_bits = bit_length((int64_t)dims_x * dims_y * dims_z - 1), id_bits = bit_length(V);  // cluster ids are below V, V itself marks a bad face
    hipLaunchKernelGGL(k_simplify_keys, dim3(blocks_of(V)), dim3(SB), 0, st, vertices, V, g, w.keys);
    TN_CHECK_LAUNCH("tn_mesh_simplify_plan(keys)");
    bool ok = rocprim::radix_sort_pairs(w.tmp, tb, w.keys, w.keys_sorted, rocprim::counting_iterator<int32_t>(0), w.vorder, (size_t)V, 0, key_bits, st) ==
              hipSuccess;
    hipLaunchKernelGGL(k_simplify_heads, dim3(blocks_of(V)), dim3(SB), 0, st, (const uint32_t*)w.keys_sorted, V, w.vflag);
    TN_CHECK_LAUNCH("tn_mesh_simplify_plan(heads)");
    tb = (size_t)L.tmp_bytes;
    ok = ok && rocprim::inclusive_scan(w.tmp, tb, (const int32_t*)w.vflag, w.vscan, (size_t)V, rocprim::plus<int32_t>(), st) == hipSuccess;
    hipLaunchKernelGGL(k_simplify_clusters_of, dim3(blocks_of(V)), dim3(SB), 0, st, (const int32_t*)w.vorder, (const int32_t*)w.vflag,
                       (const int32_t*)w.vscan, V, w.cluster_of, w.vstart, w.meta);
    TN_CHECK_LAUNCH("tn_mesh_simplify_plan(clusters)");
    hipLaunchKernelGGL(k_simplify_corners, dim3(blocks_of(F)), dim3(SB), 0, st, faces, F, V, (const int32_t*)w.cluster_of, w.ckeys);
    TN_CHECK_LAUNCH("tn_mesh_simplify_plan(corners)");
    tb = (size_t)L.tmp_bytes;
    ok = ok && rocprim::radix_sort_pairs(w.tmp, tb, w.ckeys, w.ckeys_sorted, rocprim::counting_iterator<int32_t>(0), w.cvals, (size_t)(3 * F), 0, id_bits,
                                         st) == hipSuccess;
    hipLaunchKernelGGL(k_simplify_face_hi, dim3(blocks_of(F)), dim3(SB), 0, st, (const uint32_t*)w.ckeys, F, V, w.hi);
    TN_CHECK_LAUNCH("tn_mesh_simplify_plan(largest)");
    tb = (size_t)L.tmp_bytes;
    ok = ok && rocprim::radix_sort_pairs(w.tmp, tb, w.hi, w.hi_sorted, rocprim::counting_iterator<int32_t>(0), w.ord1, (size_t)F, 0, id_bits, st) == hipSuccess;
    hipLaunchKernelGGL(k_simplify_face_pair, dim3(blocks_of(F)), dim3(SB), 0, st, (const uint32_t*)w.ckeys, F, V, (const int32_t*)w.ord1, id_bits, w.pair);
    TN_CHECK_LAUNCH("tn_mesh_simplify_plan(pairs)");
    tb = (size_t)L.tmp_bytes;
    ok = ok && rocprim::radix_sort_pairs(w.tmp, tb, w.pair, w.pair_sorted, w.ord1, w.ord2, (size_t)F, 0, 2 * id_bits, st) == hipSuccess;
    ok = ok && hipMemsetAsync(w.vflag, 0, (size_t)V * 4, st) == hipSuccess;  // from here on: the marks of the referenced clusters
    hipLaunchKernelGGL(k_simplify_face_heads, dim3(blocks_of(F)), dim3(SB), 0, st, (const uint32_t*)w.ckeys, F, V, (const int32_t*)w.ord2, w.keep, w.vflag);
    TN_CHECK_LAUNCH("tn_mesh_simplify_plan(survivors)");
    tb = (size_t)L.tmp_bytes;
    ok = ok && rocprim::inclusive_scan(w.tmp, tb, (const int32_t*)w.keep, w.fscan, (size_t)F, rocprim::plus<int32_t>(), st) == hipSuccess;
    tb = (size_t)L.tmp_bytes;
    ok = ok && rocprim::inclusive_scan(w.tmp, tb, (const int32_t*)w.vflag, w.newid, (size_t)V, rocprim::plus<int32_t>(), st) == hipSuccess;
    if (!ok) {
      tn_set_error("tn_mesh_simplify_plan: a rocprim sort or scan failed");
      return TN_ELAUNCH;
    }
  }
  hipLaunchKernelGGL(k_simplify_totals, dim3(1), dim3(TN_WAVE), 0, st, (const int32_t*)w.newid, V, (const int32_t*)w.fscan, F, totals);
  TN_CHECK_LAUNCH("tn_mesh_simplify_plan(totals)");
  return TN_OK;
}

extern "C" int tn_mesh_simplify_emit(const float* vertices, const float* normals, const float* rgbt, int64_t num_vertices, const int32_t* faces,
                                     int64_t num_faces, float origin_x, float origin_y, float origin_z, float cell_x, float cell_y, float cell_z,
                                     int32_t dims_x, int32_t dims_y, int32_t dims_z, float regularization, float* out_vertices, float* out_normals,
                                     float* out_rgbt, int64_t num_out_vertices, int32_t* out_faces, int64_t num_out_faces, void* workspace,
                                     int64_t workspace_bytes, tn_stream_t stream) {
  SimplifyLayout L;
  if (const int rc = simplify_check("tn_mesh_simplify_emit", vertices, num_vertices, faces, num_faces, origin_x, origin_y, origin_z, cell_x, cell_y, cell_z,
                                    dims_x, dims_y, dims_z, workspace, workspace_bytes, L))
    return rc;
  TN_REQUIRE(regularization >= 0.0f && regularization <= 3.4028234663852886e38f, "tn_mesh_simplify_emit: regularization = %g (>= 0, finite)",
             (double)regularization);
  TN_REQUIRE(num_out_vertices >= 0 && num_out_vertices <= num_vertices && num_out_faces >= 0 && num_out_faces <= num_faces,
             "tn_mesh_simplify_emit: %lld vertices and %lld faces out of %lld and %lld", (long long)num_out_vertices, (long long)num_out_faces,
             (long long)num_vertices, (long long)num_faces);
  TN_REQUIRE(num_vertices == 0 || (normals && rgbt), "tn_mesh_simplify_emit: null pointer");
  TN_REQUIRE(num_out_vertices == 0 || (out_vertices && out_normals && out_rgbt), "tn_mesh_simplify_emit: null pointer (outputs of %lld vertices)",
             (long long)num_out_vertices);
  TN_REQUIRE(num_out_faces == 0 || out_faces, "tn_mesh_simplify_emit: null pointer (an output of %lld faces)", (long long)num_out_faces);
  TN_REQUIRE(((uintptr_t)rgbt & 15) == 0 && ((uintptr_t)out_rgbt & 15) == 0, "tn_mesh_simplify_emit: the two rgbt arrays must be 16-byte aligned");
  if (num_out_vertices == 0 && num_out_faces == 0) return TN_OK;
  const int64_t V = num_vertices, F = num_faces;
  const SimplifyWs w = simplify_views(workspace, L);
  const SimplifyGridK g{origin_x, origin_y, origin_z, cell_x, cell_y, cell_z, dims_x, dims_y, dims_z};
  const SimplifyOutK o{out_vertices, out_normals, reinterpret_cast<float4*>(out_rgbt), num_out_vertices, out_faces, num_out_faces};
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_simplify_emit_clusters, dim3(blocks_of(V)), dim3(SB), 0, st, vertices, normals, reinterpret_cast<const float4*>(rgbt), V, faces, F, g,
                     (double)regularization, w, o);
  TN_CHECK_LAUNCH("tn_mesh_simplify_emit(clusters)");
  hipLaunchKernelGGL(k_simplify_emit_faces, dim3(blocks_of(F)), dim3(SB), 0, st, F, V, w, o);
  TN_CHECK_LAUNCH("tn_mesh_simplify_emit(faces)");
  return TN_OK;
}
