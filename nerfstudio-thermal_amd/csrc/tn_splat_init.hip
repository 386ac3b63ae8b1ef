// N4 seeding: exact k-nearest-neighbour distances over a point cloud, the HIP form of splatfacto's k_nearest_sklearn
// (nerfstudio/models/splatfacto.py:272-290: NearestNeighbors(k + 1) over the cloud itself, column 0 -- the point -- dropped).
//
// Row i holds the k smallest (d2, j) over j != i in lexicographic order, d2 = (dx*dx + dy*dy) + dz*dz with dx = xi - xj in fp32 (the
// library builds with -ffp-contract=off), distance = sqrtf(d2).  The search is exact: every result is bit-identical to a brute force with
// the same formula, whatever the tree looks like, so the tree only has to be fast, never tight.  No float atomics, no host synchronisation.
//
// Morton-ordered implicit BVH:
//   k_knn_box         bounding box of the cloud (min / max per axis): one partial box per block, then one block folds them
//   k_knn_morton      63-bit Morton code per point (3 x 21 bits over the box; a zero extent maps to 0)
//   rocprim sort      radix sort of (code, index) pairs -- stable, so equal codes keep index order
//   k_knn_gather      sorted points as float4 (x, y, z, original index)
//   k_knn_leaves      every KL consecutive sorted points form a leaf: its box from the actual coordinates and its smallest original index;
//                     leaves are padded to a power of two P with empty nodes
//   k_knn_level       one launch per tree level, bottom-up: a node is the union of its two children (heap layout, root 1, leaves P..2P-1)
//   k_knn_query<K>    one thread per sorted point: the k-best list (registers, insertion unrolled for the compile-time K) is seeded from the
//                     point's own leaf, then a stackless near-child-first traversal (one trail bit per level) visits every node that can
//                     still hold a better (d2, j); the row is written at the point's original index.
//   k_knn_query_mean<K>  the same search (knn_search) with a wide list, K in {7, 15, 19, 31}, for the statistical outlier rule of the point-cloud
//                     export (tn_knn_neighbor_means, called by tn_cloud_remove_outliers): it writes one double per point, no [n,k] table.
//   k_knn_query_normal<K>  the same wide search for the normals of the exported cloud (tn_knn_normals, called by tn_cloud_estimate_normals): the
//                     neighbours' covariance in double, its smallest eigenvector by Jacobi rotations, oriented; one fp32 row per point.
// knn_build_tree builds the tree for all three; tn_knn itself stays at k = 1..8.
//
// Pruning is exact: the box distance uses the point formula on the box's nearest coordinate, and correctly rounded subtraction, squaring
// and addition are monotone, so it is a lower bound of every computed d2 inside the box.  A node is skipped when that bound exceeds the
// current k-th best d2, or equals it and the node's smallest original index is above the k-th best index (the tie rule: smaller index wins).
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "tn_common.h"

namespace {

constexpr int KL = 16;       // points per leaf
constexpr int KB = 256;      // threads per block
constexpr int KMAX = 8;      // largest k
constexpr uint32_t KMORTON_MAX = (1u << 21) - 1;

struct KBox {
  float lx, ly, lz, hx, hy, hz;
};

struct KBoxUnion {
  __host__ __device__ KBox operator()(const KBox& a, const KBox& b) const {
    return KBox{fminf(a.lx, b.lx), fminf(a.ly, b.ly), fminf(a.lz, b.lz), fmaxf(a.hx, b.hx), fmaxf(a.hy, b.hy), fmaxf(a.hz, b.hz)};
  }
};

constexpr int KBOX_BLOCKS = 1024;  // partial boxes of the first reduction pass

__device__ inline KBox empty_box() { return KBox{INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY}; }

// the union of the boxes of the block's threads, returned to thread 0 (min / max: any order gives the same box)
__device__ inline KBox block_union(KBox b) {
  __shared__ KBox sh[KB];
  sh[threadIdx.x] = b;
  __syncthreads();
  for (int w = KB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = KBoxUnion()(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  return sh[0];
}

__global__ void __launch_bounds__(KB) k_knn_box_partial(const float* __restrict__ p, int64_t n, KBox* __restrict__ partial) {
  KBox b = empty_box();
  for (int64_t i = (int64_t)blockIdx.x * KB + threadIdx.x; i < n; i += (int64_t)gridDim.x * KB) {
    const float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
    b = KBoxUnion()(b, KBox{x, y, z, x, y, z});
  }
  b = block_union(b);
  if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

__global__ void __launch_bounds__(KB) k_knn_box_final(const KBox* __restrict__ partial, int num_partial, KBox* __restrict__ box) {
  KBox b = empty_box();
  for (int i = threadIdx.x; i < num_partial; i += KB) b = KBoxUnion()(b, partial[i]);
  b = block_union(b);
  if (threadIdx.x == 0) *box = b;
}

// 32 bytes: two float4 loads.  An empty node has an empty box (lo = +inf, hi = -inf) and minidx = INT32_MAX.
struct alignas(16) KNode {
  float lx, ly, lz;
  int32_t minidx;
  float hx, hy, hz;
  int32_t pad;
};

__device__ inline uint64_t spread21(uint32_t v) {
  uint64_t x = v & 0x1fffffu;
  x = (x | (x << 32)) & 0x1f00000000ffffull;
  x = (x | (x << 16)) & 0x1f0000ff0000ffull;
  x = (x | (x << 8)) & 0x100f00f00f00f00full;
  x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
  x = (x | (x << 2)) & 0x1249249249249249ull;
  return x;
}

__device__ inline uint32_t quantise(float v, float lo, float hi) {
  const float ext = hi - lo;
  if (!(ext > 0.0f)) return 0u;  // zero extent (a plane, a line, one point) -- or a non-finite box
  const float t = fminf(fmaxf((v - lo) / ext, 0.0f), 1.0f);  // fmaxf / fminf also send NaN to the range
  return (uint32_t)(t * (float)KMORTON_MAX);
}

__global__ void __launch_bounds__(KB) k_knn_morton(const float* __restrict__ p, int64_t n, const KBox* __restrict__ box, uint64_t* __restrict__ codes) {
  const int64_t i = (int64_t)blockIdx.x * KB + threadIdx.x;
  if (i >= n) return;
  const KBox b = *box;
  const uint32_t qx = quantise(p[3 * i], b.lx, b.hx), qy = quantise(p[3 * i + 1], b.ly, b.hy), qz = quantise(p[3 * i + 2], b.lz, b.hz);
  codes[i] = (spread21(qx) << 2) | (spread21(qy) << 1) | spread21(qz);
}

__global__ void __launch_bounds__(KB) k_knn_gather(const float* __restrict__ p, int64_t n, const int32_t* __restrict__ order, float4* __restrict__ sp) {
  const int64_t s = (int64_t)blockIdx.x * KB + threadIdx.x;
  if (s >= n) return;
  const int32_t o = order[s];
  sp[s] = make_float4(p[3 * (int64_t)o], p[3 * (int64_t)o + 1], p[3 * (int64_t)o + 2], __int_as_float(o));
}

__device__ inline void store_node(KNode* nodes, int64_t at, const KNode& v) {
  float4* d = reinterpret_cast<float4*>(nodes + at);
  d[0] = make_float4(v.lx, v.ly, v.lz, __int_as_float(v.minidx));
  d[1] = make_float4(v.hx, v.hy, v.hz, 0.0f);
}

__device__ inline KNode load_node(const KNode* nodes, int64_t at) {
  const float4* s = reinterpret_cast<const float4*>(nodes + at);
  const float4 a = s[0], b = s[1];
  return KNode{a.x, a.y, a.z, __float_as_int(a.w), b.x, b.y, b.z, 0};
}

__device__ inline KNode empty_node() {
  return KNode{INFINITY, INFINITY, INFINITY, INT32_MAX, -INFINITY, -INFINITY, -INFINITY, 0};
}

// leaves P .. 2P-1 of the heap: one thread per leaf (padding leaves are empty)
__global__ void __launch_bounds__(KB) k_knn_leaves(const float4* __restrict__ sp, int64_t n, int64_t num_padded, KNode* __restrict__ nodes) {
  const int64_t l = (int64_t)blockIdx.x * KB + threadIdx.x;
  if (l >= num_padded) return;
  KNode v = empty_node();
  const int64_t b = l * KL, e = b + KL < n ? b + KL : n;
  for (int64_t s = b; s < e; ++s) {
    const float4 q = sp[s];
    v.lx = fminf(v.lx, q.x), v.ly = fminf(v.ly, q.y), v.lz = fminf(v.lz, q.z);
    v.hx = fmaxf(v.hx, q.x), v.hy = fmaxf(v.hy, q.y), v.hz = fmaxf(v.hz, q.z);
    v.minidx = min(v.minidx, __float_as_int(q.w));
  }
  store_node(nodes, num_padded + l, v);
}

// nodes first .. 2 first - 1 from their children
__global__ void __launch_bounds__(KB) k_knn_level(int64_t first, KNode* __restrict__ nodes) {
  const int64_t t = (int64_t)blockIdx.x * KB + threadIdx.x;
  if (t >= first) return;
  const int64_t at = first + t;
  const KNode a = load_node(nodes, 2 * at), b = load_node(nodes, 2 * at + 1);
  const KNode v{fminf(a.lx, b.lx), fminf(a.ly, b.ly), fminf(a.lz, b.lz), min(a.minidx, b.minidx), fmaxf(a.hx, b.hx), fmaxf(a.hy, b.hy), fmaxf(a.hz, b.hz), 0};
  store_node(nodes, at, v);
}

__device__ inline float point_d2(float xi, float yi, float zi, float xj, float yj, float zj) {
  const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
  return (dx * dx + dy * dy) + dz * dz;
}

// the same formula on the box's nearest coordinate: a lower bound of point_d2 for every point inside the box
__device__ inline float axis_gap(float v, float lo, float hi) { return v < lo ? v - lo : (v > hi ? v - hi : 0.0f); }
__device__ inline float box_d2(float x, float y, float z, const KNode& b) {
  const float dx = axis_gap(x, b.lx, b.hx), dy = axis_gap(y, b.ly, b.hy), dz = axis_gap(z, b.lz, b.hz);
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ inline bool knn_less(float d2, int32_t j, float e2, int32_t ej) { return d2 < e2 || (d2 == e2 && j < ej); }

template <int K>
struct KBest {
  float d[K];
  int32_t j[K];
  __device__ inline void init() {
#pragma unroll
    for (int m = 0; m < K; ++m) d[m] = INFINITY, j[m] = INT32_MAX;
  }
  // every slot is written once from the old values of itself and its predecessor: constant indices only (no scratch)
  __device__ inline void insert(float c2, int32_t cj) {
    if (!knn_less(c2, cj, d[K - 1], j[K - 1])) return;
#pragma unroll
    for (int m = K - 1; m > 0; --m) {
      const bool below = knn_less(c2, cj, d[m - 1], j[m - 1]);
      const bool here = knn_less(c2, cj, d[m], j[m]);
      d[m] = below ? d[m - 1] : (here ? c2 : d[m]);
      j[m] = below ? j[m - 1] : (here ? cj : j[m]);
    }
    if (knn_less(c2, cj, d[0], j[0])) d[0] = c2, j[0] = cj;
  }
  __device__ inline bool prunes(float b2, int32_t minidx) const {
    return minidx == INT32_MAX || b2 > d[K - 1] || (b2 == d[K - 1] && minidx > j[K - 1]);
  }
};

// the exact K best (d2, j) over j != the point at sorted position s, into `best`
template <int K>
__device__ inline void knn_search(const float4* __restrict__ sp, int64_t n, const KNode* __restrict__ nodes, int64_t num_padded, int64_t s, const float4 q,
                                  KBest<K>& best) {
  best.init();
  const int64_t own = s / KL;
  {
    const int64_t b = own * KL, e = b + KL < n ? b + KL : n;
    for (int64_t t = b; t < e; ++t) {
      if (t == s) continue;
      const float4 r = sp[t];
      best.insert(point_d2(q.x, q.y, q.z, r.x, r.y, r.z), __float_as_int(r.w));
    }
  }
  // stackless traversal of the heap: node, its depth, and per depth one bit "this is the second (far) child"
  int64_t node = 1;
  int depth = 0;
  uint32_t trail = 0;
  while (true) {
    const KNode b = load_node(nodes, node);
    if (!best.prunes(box_d2(q.x, q.y, q.z, b), b.minidx)) {
      if (node < num_padded) {  // internal: go to the nearer child first (ties: the left one)
        const KNode c0 = load_node(nodes, 2 * node), c1 = load_node(nodes, 2 * node + 1);
        const float d0 = box_d2(q.x, q.y, q.z, c0), d1 = box_d2(q.x, q.y, q.z, c1);
        node = 2 * node + (d1 < d0 ? 1 : 0);
        ++depth;
        trail &= ~(1u << depth);
        continue;
      }
      const int64_t leaf = node - num_padded;
      if (leaf != own) {
        const int64_t lb = leaf * KL, le = lb + KL < n ? lb + KL : n;
        for (int64_t t = lb; t < le; ++t) {
          const float4 r = sp[t];
          best.insert(point_d2(q.x, q.y, q.z, r.x, r.y, r.z), __float_as_int(r.w));
        }
      }
    }
    // climb past every finished second child, then step to the sibling
    while (depth > 0 && ((trail >> depth) & 1u)) node >>= 1, --depth;
    if (depth == 0) break;
    node ^= 1;
    trail |= 1u << depth;
  }
}

template <int K>
__global__ void __launch_bounds__(KB) k_knn_query(const float4* __restrict__ sp, int64_t n, const KNode* __restrict__ nodes, int64_t num_padded,
                                                  float* __restrict__ out_dist, int32_t* __restrict__ out_index) {
  const int64_t s = (int64_t)blockIdx.x * KB + threadIdx.x;
  if (s >= n) return;
  const float4 q = sp[s];
  const int32_t self = __float_as_int(q.w);
  KBest<K> best;
  knn_search<K>(sp, n, nodes, num_padded, s, q, best);
  const int64_t row = (int64_t)self * K;
#pragma unroll
  for (int m = 0; m < K; ++m) out_dist[row + m] = sqrtf(best.d[m]);
  if (out_index) {
#pragma unroll
    for (int m = 0; m < K; ++m) out_index[row + m] = best.j[m];
  }
}

// The wide query of the statistical outlier rule (tn_cloud_remove_outliers): the exact K >= used nearest, of which the first `used` -- they are
// the exact `used` nearest -- are summed as distances, ascending, in double, and divided by `divisor`; nothing but mean[self] is written.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; the list is 2 K registers held at constant indices, and the unrolled insertion
// keeps old and new values of a slot alive side by side):
//   K = 7: 58 VGPRs, 8 waves / SIMD;  K = 15: 91, 5;  K = 19: 112, 4;  K = 31: 172, 2 -- no scratch and no spills in any of them.
// The block size stays KB = 256 (4 waves): at K = 19, the reference's nb_neighbors = 20, a CU holds 16 waves = 4 whole blocks, and at K = 31 8 waves
// = 2 whole blocks, so no register file is left partly empty by the block granularity; a smaller block would only add launches of the same waves.
template <int K>
__global__ void __launch_bounds__(KB) k_knn_query_mean(const float4* __restrict__ sp, int64_t n, const KNode* __restrict__ nodes, int64_t num_padded,
                                                       int used, double divisor, double* __restrict__ mean) {
  const int64_t s = (int64_t)blockIdx.x * KB + threadIdx.x;
  if (s >= n) return;
  const float4 q = sp[s];
  KBest<K> best;
  knn_search<K>(sp, n, nodes, num_padded, s, q, best);
  double sum = 0.0;
#pragma unroll
  for (int m = 0; m < K; ++m)
    if (m < used) sum += (double)sqrtf(best.d[m]);
  mean[__float_as_int(q.w)] = sum / divisor;
}

// One Jacobi rotation in the (p, q) plane of a symmetric 3x3 matrix: a_pq becomes zero, r is the third index, and the columns p and q of the
// accumulated eigenvector matrix V turn with it (t = tan of the angle, the smaller root; theta * theta may overflow to inf, which gives t = 0).
__device__ inline void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p, double& v1q,
                                     double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq, aqq += t * apq, apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp, arq = rq;
  const double x0 = c * v0p - s * v0q, x1 = c * v1p - s * v1q, x2 = c * v2p - s * v2q;
  v0q = s * v0p + c * v0q, v1q = s * v1p + c * v1q, v2q = s * v2p + c * v2q;
  v0p = x0, v1p = x1, v2p = x2;
}

constexpr int JACOBI_SWEEPS = 12;        // a 3x3 reaches the threshold below in 5..7 sweeps (the off-diagonal shrinks quadratically); the cap only bounds the loop
constexpr double JACOBI_DONE = 0x1p-100;  // on a matrix of trace 1: what is left moves an eigenvector by 2^-100 / (its eigenvalue gap)

// The query of tn_cloud_estimate_normals: the same search, then -- the distance list is dead, only the index list is live -- the `used` neighbours
// are gathered from the cloud by their original indices (queries run in Morton order, so neighbouring threads gather neighbouring rows), their
// differences to the point are summed in double in list order (the point itself, first of its neighbourhood, adds zeros), the covariance
// C = S2 / knn - (S1 / knn)(S1 / knn)^T is scaled by its trace and diagonalised by cyclic Jacobi rotations in double, and the unit eigenvector of
// the smallest eigenvalue is oriented and rounded once.  Nothing but normals[self] is written.
template <int K>
__global__ void __launch_bounds__(KB) k_knn_query_normal(const float4* __restrict__ sp, int64_t n, const KNode* __restrict__ nodes, int64_t num_padded,
                                                         const float* __restrict__ xyz, int used, double knn, const float* __restrict__ view,
                                                         float* __restrict__ normals) {
  const int64_t s = (int64_t)blockIdx.x * KB + threadIdx.x;
  if (s >= n) return;
  const float4 q = sp[s];
  KBest<K> best;
  knn_search<K>(sp, n, nodes, num_padded, s, q, best);
  const int64_t self = __float_as_int(q.w);
  const double px = q.x, py = q.y, pz = q.z;
  double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
#pragma unroll
  for (int m = 0; m < K; ++m) {
    if (m < used) {  // n - 1 >= used other points exist: the first `used` slots are real indices in 0..n-1
      const int64_t j = best.j[m];
      const double cx = (double)xyz[3 * j] - px, cy = (double)xyz[3 * j + 1] - py, cz = (double)xyz[3 * j + 2] - pz;
      s1x += cx, s1y += cy, s1z += cz;
      sxx += cx * cx, sxy += cx * cy, sxz += cx * cz, syy += cy * cy, syz += cy * cz, szz += cz * cz;
    }
  }
  const double mx = s1x / knn, my = s1y / knn, mz = s1z / knn;
  double a00 = sxx / knn - mx * mx, a01 = sxy / knn - mx * my, a02 = sxz / knn - mx * mz;
  double a11 = syy / knn - my * my, a12 = syz / knn - my * mz, a22 = szz / knn - mz * mz;
  double nx = 0.0, ny = 0.0, nz = 1.0;  // a covariance that is exactly zero (all knn points coincide): Open3D's fallback
  if (a00 != 0.0 || a01 != 0.0 || a02 != 0.0 || a11 != 0.0 || a12 != 0.0 || a22 != 0.0) {
    const double tr = (a00 + a11) + a22;
    const double big = fmax(fmax(fmax(fabs(a00), fabs(a11)), fmax(fabs(a22), fabs(a01))), fmax(fabs(a02), fabs(a12)));
    const double scale = tr > 0.0 ? tr : big;  // the trace of a covariance is positive; rounding alone could take a tiny one below zero
    a00 /= scale, a01 /= scale, a02 /= scale, a11 /= scale, a12 /= scale, a22 /= scale;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
      if ((fabs(a01) + fabs(a02)) + fabs(a12) <= JACOBI_DONE) break;
      jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
      jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
      jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    // the column of the smallest eigenvalue (ties: the lowest index), selected without indexing
    const bool c1 = a11 < a00 && a11 <= a22, c2 = a22 < a00 && a22 < a11;
    nx = c2 ? v02 : (c1 ? v01 : v00), ny = c2 ? v12 : (c1 ? v11 : v10), nz = c2 ? v22 : (c1 ? v21 : v20);
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (len > 0.0 && len < INFINITY) nx /= len, ny /= len, nz /= len;
    else nx = 0.0, ny = 0.0, nz = 1.0;
  }
  bool flip;
  if (view) {
    const double dot = ((double)view[3 * self] * nx + (double)view[3 * self + 1] * ny) + (double)view[3 * self + 2] * nz;
    flip = dot > 0.0;
  } else {
    flip = nz != 0.0 ? nz < 0.0 : (ny != 0.0 ? ny < 0.0 : nx < 0.0);
  }
  normals[3 * self] = (float)(flip ? -nx : nx), normals[3 * self + 1] = (float)(flip ? -ny : ny), normals[3 * self + 2] = (float)(flip ? -nz : nz);
}

constexpr int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }

int64_t padded_leaves(int64_t n) {
  const int64_t leaves = (n + KL - 1) / KL;
  int64_t p = 1;
  while (p < leaves) p <<= 1;
  return p;
}

struct KnnLayout {
  int64_t box, partial, codes, codes_sorted, order, points, nodes, tmp, tmp_bytes, total;
  bool ok;  // rocprim answered the sort's scratch query (for a large sort the query needs the device)
};

KnnLayout knn_layout(int64_t n) {
  KnnLayout L;
  size_t sb = 0;
  const hipError_t es = rocprim::radix_sort_pairs(nullptr, sb, (uint64_t*)nullptr, (uint64_t*)nullptr, rocprim::counting_iterator<int32_t>(0),
                                                   (int32_t*)nullptr, (size_t)n, 0, 63);
  L.ok = es == hipSuccess;
  L.box = 0;
  L.partial = align256(sizeof(KBox));
  L.codes = L.partial + align256(KBOX_BLOCKS * (int64_t)sizeof(KBox));
  L.codes_sorted = L.codes + align256(n * 8);
  L.order = L.codes_sorted + align256(n * 8);
  L.points = L.order + align256(n * 4);
  L.nodes = L.points + align256(n * 16);
  L.tmp = L.nodes + align256(2 * padded_leaves(n) * (int64_t)sizeof(KNode));
  L.tmp_bytes = align256((int64_t)std::max(sb, (size_t)1));
  L.total = L.tmp + L.tmp_bytes;
  return L;
}

struct KnnTree {
  KBox *box, *partial;
  uint64_t *codes, *codes_sorted;
  int32_t* order;
  float4* sp;
  KNode* nodes;
  void* tmp;
};

KnnTree knn_tree_views(void* workspace, const KnnLayout& L) {
  char* ws = static_cast<char*>(workspace);
  return KnnTree{reinterpret_cast<KBox*>(ws + L.box),       reinterpret_cast<KBox*>(ws + L.partial),  reinterpret_cast<uint64_t*>(ws + L.codes),
                 reinterpret_cast<uint64_t*>(ws + L.codes_sorted), reinterpret_cast<int32_t*>(ws + L.order), reinterpret_cast<float4*>(ws + L.points),
                 reinterpret_cast<KNode*>(ws + L.nodes),    ws + L.tmp};
}

// box, Morton codes, sort, sorted points, leaves, levels: the tree both tn_knn and tn_knn_neighbor_means query (n >= 1, a workspace of L.total bytes)
int knn_build_tree(const float* points, int64_t n, const KnnLayout& L, const KnnTree& T, hipStream_t st) {
  const int nbox = (int)std::min<int64_t>(tn_cdiv(n, KB * 8), KBOX_BLOCKS);
  hipLaunchKernelGGL(k_knn_box_partial, dim3(nbox), dim3(KB), 0, st, points, n, T.partial);
  TN_CHECK_LAUNCH("tn_knn(box_partial)");
  hipLaunchKernelGGL(k_knn_box_final, dim3(1), dim3(KB), 0, st, T.partial, nbox, T.box);
  TN_CHECK_LAUNCH("tn_knn(box_final)");
  const unsigned gn = (unsigned)tn_cdiv(n, KB);
  hipLaunchKernelGGL(k_knn_morton, dim3(gn), dim3(KB), 0, st, points, n, T.box, T.codes);
  TN_CHECK_LAUNCH("tn_knn(morton)");
  size_t tb = (size_t)L.tmp_bytes;
  if (rocprim::radix_sort_pairs(T.tmp, tb, T.codes, T.codes_sorted, rocprim::counting_iterator<int32_t>(0), T.order, (size_t)n, 0, 63, st) != hipSuccess) {
    tn_set_error("tn_knn: rocprim::radix_sort_pairs failed");
    return TN_ELAUNCH;
  }
  hipLaunchKernelGGL(k_knn_gather, dim3(gn), dim3(KB), 0, st, points, n, T.order, T.sp);
  TN_CHECK_LAUNCH("tn_knn(gather)");
  const int64_t P = padded_leaves(n);
  hipLaunchKernelGGL(k_knn_leaves, dim3((unsigned)tn_cdiv(P, KB)), dim3(KB), 0, st, T.sp, n, P, T.nodes);
  TN_CHECK_LAUNCH("tn_knn(leaves)");
  for (int64_t first = P >> 1; first >= 1; first >>= 1) {
    hipLaunchKernelGGL(k_knn_level, dim3((unsigned)tn_cdiv(first, KB)), dim3(KB), 0, st, first, T.nodes);
    TN_CHECK_LAUNCH("tn_knn(level)");
  }
  return TN_OK;
}

template <int K>
void launch_query_mean(const KnnTree& T, int64_t n, int used, int32_t nb, double* mean, hipStream_t st) {
  hipLaunchKernelGGL(k_knn_query_mean<K>, dim3((unsigned)tn_cdiv(n, KB)), dim3(KB), 0, st, (const float4*)T.sp, n, (const KNode*)T.nodes, padded_leaves(n), used,
                     (double)nb, mean);
}

template <int K>
void launch_query_normal(const KnnTree& T, int64_t n, const float* xyz, int used, int32_t knn, const float* view, float* normals, hipStream_t st) {
  hipLaunchKernelGGL(k_knn_query_normal<K>, dim3((unsigned)tn_cdiv(n, KB)), dim3(KB), 0, st, (const float4*)T.sp, n, (const KNode*)T.nodes, padded_leaves(n), xyz,
                     used, (double)knn, view, normals);
}

template <int K>
void launch_query(const float4* sp, int64_t n, const KNode* nodes, int64_t P, float* out_dist, int32_t* out_index, hipStream_t st) {
  hipLaunchKernelGGL(k_knn_query<K>, dim3((unsigned)tn_cdiv(n, KB)), dim3(KB), 0, st, sp, n, nodes, P, out_dist, out_index);
}

}  // namespace

extern "C" int64_t tn_knn_workspace_bytes(int64_t n, int32_t k) {
  if (n < 0 || n > INT32_MAX || k < 1 || k > KMAX) return -1;
  if (n == 0) return 0;
  const KnnLayout L = knn_layout(n);
  return L.ok ? L.total : -1;
}

extern "C" int tn_knn(const float* points, int64_t n, int32_t k, float* out_dist, int32_t* out_index, void* workspace, int64_t workspace_bytes,
                      tn_stream_t stream) {
  TN_REQUIRE(k >= 1 && k <= KMAX, "tn_knn: k = %d (1..%d)", k, KMAX);
  TN_REQUIRE(n >= 0 && n <= INT32_MAX, "tn_knn: %lld points (0..%d)", (long long)n, INT32_MAX);
  if (n == 0) return TN_OK;
  TN_REQUIRE(points && out_dist && workspace, "tn_knn: null pointer");
  TN_REQUIRE(n >= (int64_t)k + 1, "tn_knn: %lld points, k = %d needs at least k + 1", (long long)n, k);
  const KnnLayout L = knn_layout(n);
  if (!L.ok) {
    tn_set_error("tn_knn: rocprim could not size its scratch for %lld points", (long long)n);
    return TN_ELAUNCH;
  }
  TN_REQUIRE(workspace_bytes >= L.total, "tn_knn: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  hipStream_t st = tn_s(stream);
  const KnnTree T = knn_tree_views(workspace, L);
  if (const int rc = knn_build_tree(points, n, L, T, st)) return rc;
  const float4* sp = T.sp;
  const KNode* nodes = T.nodes;
  const int64_t P = padded_leaves(n);
  switch (k) {
    case 1: launch_query<1>(sp, n, nodes, P, out_dist, out_index, st); break;
    case 2: launch_query<2>(sp, n, nodes, P, out_dist, out_index, st); break;
    case 3: launch_query<3>(sp, n, nodes, P, out_dist, out_index, st); break;
    case 4: launch_query<4>(sp, n, nodes, P, out_dist, out_index, st); break;
    case 5: launch_query<5>(sp, n, nodes, P, out_dist, out_index, st); break;
    case 6: launch_query<6>(sp, n, nodes, P, out_dist, out_index, st); break;
    case 7: launch_query<7>(sp, n, nodes, P, out_dist, out_index, st); break;
    default: launch_query<8>(sp, n, nodes, P, out_dist, out_index, st); break;
  }
  TN_CHECK_LAUNCH("tn_knn(query)");
  return TN_OK;
}

// ---- internal (tn_common.h): the neighbour means of the statistical outlier rule, for tn_cloud_remove_outliers (tn_cloud.hip)
int64_t tn_knn_tree_workspace_bytes(int64_t n) {
  if (n < 1 || n > INT32_MAX) return -1;
  const KnnLayout L = knn_layout(n);
  return L.ok ? L.total : -1;
}

int tn_knn_neighbor_means(const float* points, int64_t n, int32_t nb_neighbors, double* mean, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  const KnnLayout L = knn_layout(n);
  if (!L.ok) {
    tn_set_error("tn_cloud_remove_outliers: rocprim could not size its scratch for %lld points", (long long)n);
    return TN_ELAUNCH;
  }
  TN_REQUIRE(workspace_bytes >= L.total, "tn_cloud_remove_outliers: tree workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  const KnnTree T = knn_tree_views(workspace, L);
  if (const int rc = knn_build_tree(points, n, L, T, st)) return rc;
  const int used = nb_neighbors - 1;  // 1..31; n - 1 >= used other points exist, so the first `used` slots of a longer list are all real
  if (used <= 7) launch_query_mean<7>(T, n, used, nb_neighbors, mean, st);
  else if (used <= 15) launch_query_mean<15>(T, n, used, nb_neighbors, mean, st);
  else if (used <= 19) launch_query_mean<19>(T, n, used, nb_neighbors, mean, st);
  else launch_query_mean<31>(T, n, used, nb_neighbors, mean, st);
  TN_CHECK_LAUNCH("tn_cloud_remove_outliers(query)");
  return TN_OK;
}

// ---- internal (tn_common.h): the oriented normals of tn_cloud_estimate_normals (tn_cloud.hip)
int tn_knn_normals(const float* points, int64_t n, int32_t knn, const float* view, float* normals, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  const KnnLayout L = knn_layout(n);
  if (!L.ok) {
    tn_set_error("tn_cloud_estimate_normals: rocprim could not size its scratch for %lld points", (long long)n);
    return TN_ELAUNCH;
  }
  TN_REQUIRE(workspace_bytes >= L.total, "tn_cloud_estimate_normals: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  const KnnTree T = knn_tree_views(workspace, L);
  if (const int rc = knn_build_tree(points, n, L, T, st)) return rc;
  const int used = knn - 1;  // 2..31 other points, of which n - 1 >= used exist
  if (used <= 7) launch_query_normal<7>(T, n, points, used, knn, view, normals, st);
  else if (used <= 15) launch_query_normal<15>(T, n, points, used, knn, view, normals, st);
  else if (used <= 19) launch_query_normal<19>(T, n, points, used, knn, view, normals, st);
  else launch_query_normal<31>(T, n, points, used, knn, view, normals, st);
  TN_CHECK_LAUNCH("tn_cloud_estimate_normals(query)");
  return TN_OK;
}
