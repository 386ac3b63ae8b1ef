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
// knn_build_tree builds the tree for both; tn_knn itself stays at k = 1..8.
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
