// Dense-grid Poisson surface reconstruction from an oriented point cloud (the counterpart of `ns-export poisson`: nerfstudio/scripts/exporter.py
// ExportPoissonMesh, Open3D's create_from_point_cloud_poisson).  Not Kazhdan's adaptive octree: one regular lattice, a 7-point Laplacian with a
// Dirichlet boundary, conjugate gradients.  The rule of every entry point is stated in include/thermal_nerf_hip.h; tests/poisson_functional.py
// restates it in float64.
//
// Kernels (gfx950, blocks of 256 = four waves; every volume is walked z fastest, so a wave reads and writes whole rows):
//   k_poisson_keys / k_poisson_cell_starts   the plan: a cell key per point (the sentinel `cells` for a skipped point), rocprim's stable radix sort of
//                                            (key, index), and the first sorted row of every cell by a lower bound over the sorted keys;
//   k_poisson_splat                          a GATHER: a thread per lattice point walks its eight adjacent cells and their points in the plan's order,
//                                            sums in double registers and stores once -- no atomics, so the same inputs give the same bits.  Surface
//                                            cells hold a few points and most lattice points none, so the cost is the sixteen cell-start loads of
//                                            a thread; a duplicate-heavy cell is walked by the eight threads of its corners only;
//   k_poisson_sample / _divergence / _apply  streaming, a thread per point or lattice point;
//   k_cg_*                                   the solve: three launches per iteration (A p and p . A p; x, r and r . r; p), every dot product as one
//                                            double partial per block and a fold of the partials, in a fixed order, by every block that needs the
//                                            sum.  alpha, beta and the stop flag never leave the device; a launch that finds the flag set returns.
// Bound of an iteration: it moves 11 arrays of X Y Z floats (12 with a screening volume): p -> A p; x p r A p -> x r; r p -> p.
#include "tn_common.h"

#include <string.h>

#include <rocprim/rocprim.hpp>

#include <algorithm>

#define POISSON_BLOCK 256        /* threads of a block: one partial sum per block */
#define POISSON_MAX_BLOCKS 1024  /* blocks of a solve launch (grid-stride beyond): the partials one fold reads */

namespace {

constexpr int64_t PB = POISSON_BLOCK;
constexpr int64_t POISSON_MAX = 2147483647ll;  // lattice points and cloud points are below 2^31
constexpr int64_t align256(int64_t b) { return (b + 255) & ~int64_t(255); }

struct PGridK {
  int X, Y, Z;
  double ox, oy, oz;  // origin and voxel: the fp32 arguments, widened
  double hx, hy, hz;
};

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }
__device__ __forceinline__ bool finite_f(float v) { return v - v == 0.0f; }

// lattice point e -> (i, j, k), z fastest; e < 2^31
__device__ __forceinline__ void lattice_of(uint32_t e, const PGridK& g, int& i, int& j, int& k) {
  const uint32_t q = e / (uint32_t)g.Z;
  k = (int)(e - q * (uint32_t)g.Z);
  i = (int)(q / (uint32_t)g.Y);
  j = (int)(q - (uint32_t)i * (uint32_t)g.Y);
}

// ---------------------------------------------------------------------------------------------------- the plan
__global__ void __launch_bounds__(POISSON_BLOCK) k_poisson_keys(const float* __restrict__ points, int64_t n, PGridK g, uint32_t cells,
                                                                uint32_t* __restrict__ keys) {
  const int64_t p = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (p >= n) return;
  const double tx = ((double)points[3 * p] - g.ox) / g.hx, ty = ((double)points[3 * p + 1] - g.oy) / g.hy, tz = ((double)points[3 * p + 2] - g.oz) / g.hz;
  uint32_t key = cells;
  if (finite_d(tx) && finite_d(ty) && finite_d(tz)) {
    const double cx = floor(tx), cy = floor(ty), cz = floor(tz);
    if (cx >= 0.0 && cx <= (double)(g.X - 2) && cy >= 0.0 && cy <= (double)(g.Y - 2) && cz >= 0.0 && cz <= (double)(g.Z - 2))
      key = ((uint32_t)cx * (uint32_t)(g.Y - 1) + (uint32_t)cy) * (uint32_t)(g.Z - 1) + (uint32_t)cz;
  }
  keys[p] = key;
}

// start[c] = the first sorted row whose key is at least c, for c in 0..cells (start[cells] = the number of kept points)
__global__ void __launch_bounds__(POISSON_BLOCK) k_poisson_cell_starts(const uint32_t* __restrict__ sorted, int64_t n, uint32_t cells,
                                                                       int32_t* __restrict__ start) {
  const int64_t c = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (c > (int64_t)cells) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sorted[mid] < (uint32_t)c) lo = mid + 1; else hi = mid;
  }
  start[c] = (int32_t)lo;
}

// ---------------------------------------------------------------------------------------------------- splat
__global__ void __launch_bounds__(POISSON_BLOCK) k_poisson_splat(const float* __restrict__ points, const float* __restrict__ values, int C,
                                                                 const float* __restrict__ weights, int normalize, PGridK g,
                                                                 const int32_t* __restrict__ order, const int32_t* __restrict__ start,
                                                                 float* __restrict__ out, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (e >= total) return;
  int i, j, k;
  lattice_of((uint32_t)e, g, i, j, k);
  double acc[4] = {0.0, 0.0, 0.0, 0.0}, den = 0.0;
  for (int dx = 0; dx < 2; ++dx) {
    const int ci = i - 1 + dx;
    if (ci < 0 || ci > g.X - 2) continue;
    for (int dy = 0; dy < 2; ++dy) {
      const int cj = j - 1 + dy;
      if (cj < 0 || cj > g.Y - 2) continue;
      for (int dz = 0; dz < 2; ++dz) {
        const int ck = k - 1 + dz;
        if (ck < 0 || ck > g.Z - 2) continue;
        const uint32_t cell = ((uint32_t)ci * (uint32_t)(g.Y - 1) + (uint32_t)cj) * (uint32_t)(g.Z - 1) + (uint32_t)ck;
        const int32_t s1 = start[cell + 1];
        for (int32_t s = start[cell]; s < s1; ++s) {
          const int64_t p = order[s];
          const double w = weights != nullptr ? (double)weights[p] : 1.0;
          double v[4] = {1.0, 1.0, 1.0, 1.0};
          bool ok = finite_d(w);
          if (values != nullptr)
            for (int c = 0; c < C; ++c) {
              const float f = values[p * C + c];
              ok = ok && finite_f(f);
              v[c] = (double)f;
            }
          if (!ok) continue;
          const double tx = ((double)points[3 * p] - g.ox) / g.hx, ty = ((double)points[3 * p + 1] - g.oy) / g.hy,
                       tz = ((double)points[3 * p + 2] - g.oz) / g.hz;
          const double fx = tx - floor(tx), fy = ty - floor(ty), fz = tz - floor(tz);
          // the cell below the lattice point (offset 0) sees it as its upper corner, the cell at it (offset 1) as its lower corner
          const double wx = dx == 0 ? fx : 1.0 - fx, wy = dy == 0 ? fy : 1.0 - fy, wz = dz == 0 ? fz : 1.0 - fz;
          const double wt = w * ((wx * wy) * wz);
          den += wt;
          for (int c = 0; c < C; ++c) acc[c] += wt * v[c];
        }
      }
    }
  }
  for (int c = 0; c < C; ++c) out[e * C + c] = normalize ? (den > 0.0 ? (float)(acc[c] / den) : 0.0f) : (float)acc[c];
}

__global__ void __launch_bounds__(POISSON_BLOCK) k_poisson_zero(float* __restrict__ out, int64_t total) {
  for (int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x; e < total; e += (int64_t)gridDim.x * PB) out[e] = 0.0f;
}

// ---------------------------------------------------------------------------------------------------- sample
__global__ void __launch_bounds__(POISSON_BLOCK) k_poisson_sample(const float* __restrict__ points, int64_t n, const float* __restrict__ volume,
                                                                  PGridK g, double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (p >= n) return;
  const double tx = ((double)points[3 * p] - g.ox) / g.hx, ty = ((double)points[3 * p + 1] - g.oy) / g.hy, tz = ((double)points[3 * p + 2] - g.oz) / g.hz;
  if (!(finite_d(tx) && finite_d(ty) && finite_d(tz))) {
    out[p] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const double cx = fmin(fmax(floor(tx), 0.0), (double)(g.X - 2)), cy = fmin(fmax(floor(ty), 0.0), (double)(g.Y - 2)),
               cz = fmin(fmax(floor(tz), 0.0), (double)(g.Z - 2));
  const double fx = tx - cx, fy = ty - cy, fz = tz - cz;
  const int64_t base = ((int64_t)cx * g.Y + (int64_t)cy) * g.Z + (int64_t)cz;
  double sum = 0.0;
  for (int dx = 0; dx < 2; ++dx)
    for (int dy = 0; dy < 2; ++dy)
      for (int dz = 0; dz < 2; ++dz) {
        const double wx = dx == 0 ? 1.0 - fx : fx, wy = dy == 0 ? 1.0 - fy : fy, wz = dz == 0 ? 1.0 - fz : fz;
        sum += ((wx * wy) * wz) * (double)volume[base + ((int64_t)dx * g.Y + dy) * g.Z + dz];
      }
  out[p] = sum;
}

// ---------------------------------------------------------------------------------------------------- divergence, operator
__global__ void __launch_bounds__(POISSON_BLOCK) k_poisson_divergence(const float* __restrict__ V, PGridK g, float* __restrict__ b, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (e >= total) return;
  int i, j, k;
  lattice_of((uint32_t)e, g, i, j, k);
  const int64_t sy = g.Z, sx = (int64_t)g.Y * g.Z;
  const double xp = i < g.X - 1 ? (double)V[3 * (e + sx)] : 0.0, xm = i > 0 ? (double)V[3 * (e - sx)] : 0.0;
  const double yp = j < g.Y - 1 ? (double)V[3 * (e + sy) + 1] : 0.0, ym = j > 0 ? (double)V[3 * (e - sy) + 1] : 0.0;
  const double zp = k < g.Z - 1 ? (double)V[3 * (e + 1) + 2] : 0.0, zm = k > 0 ? (double)V[3 * (e - 1) + 2] : 0.0;
  const double dx = (xp - xm) / (2.0 * g.hx), dy = (yp - ym) / (2.0 * g.hy), dz = (zp - zm) / (2.0 * g.hz);
  b[e] = (float)(-((dx + dy) + dz));
}

// (A x)(e) in double; x is 0 outside the grid
__device__ __forceinline__ double apply_at(const float* __restrict__ x, const float* __restrict__ s, const PGridK& g, int i, int j, int k, int64_t e) {
  const int64_t sy = g.Z, sx = (int64_t)g.Y * g.Z;
  const double xc = (double)x[e];
  const double xm = i > 0 ? (double)x[e - sx] : 0.0, xp = i < g.X - 1 ? (double)x[e + sx] : 0.0;
  const double ym = j > 0 ? (double)x[e - sy] : 0.0, yp = j < g.Y - 1 ? (double)x[e + sy] : 0.0;
  const double zm = k > 0 ? (double)x[e - 1] : 0.0, zp = k < g.Z - 1 ? (double)x[e + 1] : 0.0;
  const double ax = ((2.0 * xc - xm) - xp) / (g.hx * g.hx), ay = ((2.0 * xc - ym) - yp) / (g.hy * g.hy), az = ((2.0 * xc - zm) - zp) / (g.hz * g.hz);
  double r = (ax + ay) + az;
  if (s != nullptr) r = r + (double)s[e] * xc;
  return r;
}

__global__ void __launch_bounds__(POISSON_BLOCK) k_poisson_apply(const float* __restrict__ x, const float* __restrict__ s, PGridK g,
                                                                 float* __restrict__ out, int64_t total) {
  const int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x;
  if (e >= total) return;
  int i, j, k;
  lattice_of((uint32_t)e, g, i, j, k);
  out[e] = (float)apply_at(x, s, g, i, j, k, e);
}

// ---------------------------------------------------------------------------------------------------- conjugate gradients
// the sum of a block's 256 values in a fixed order (a butterfly inside each wave, then the four waves left to right); every thread gets it
__device__ __forceinline__ double block_sum_d(double v, double* lds) {
  v = tn_wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  __syncthreads();
  return s;
}
// the sum of nb block partials: thread t adds partials t, t + 256, ... in that order, then block_sum_d
__device__ __forceinline__ double fold_partials(const double* __restrict__ partials, int nb, double* lds) {
  double a = 0.0;
  for (int b = threadIdx.x; b < nb; b += POISSON_BLOCK) a += partials[b];
  return block_sum_d(a, lds);
}

// a state slot: [iterations, r . r, b . b, done]; slot (it & 1) is read by iteration it, the other one written by its last launch
#define CG_STATE_DOUBLES 4

// r = b - A x (A x rounded to fp32 first, as tn_poisson_apply rounds it), p = r; partials of r . r and b . b
__global__ void __launch_bounds__(POISSON_BLOCK) k_cg_init(const float* __restrict__ b, const float* __restrict__ s, const float* __restrict__ x, PGridK g,
                                                           float* __restrict__ r, float* __restrict__ p, double* __restrict__ part_rr,
                                                           double* __restrict__ part_bb, int64_t total) {
  __shared__ double lds[4];
  double rr = 0.0, bb = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x; e < total; e += (int64_t)gridDim.x * PB) {
    int i, j, k;
    lattice_of((uint32_t)e, g, i, j, k);
    const float ax = (float)apply_at(x, s, g, i, j, k, e);
    const double be = (double)b[e];
    const float re = (float)(be - (double)ax);
    r[e] = re;
    p[e] = re;
    rr += (double)re * (double)re;
    bb += be * be;
  }
  rr = block_sum_d(rr, lds);
  bb = block_sum_d(bb, lds);
  if (threadIdx.x == 0) part_rr[blockIdx.x] = rr, part_bb[blockIdx.x] = bb;
}
__global__ void __launch_bounds__(POISSON_BLOCK) k_cg_start(const double* __restrict__ part_rr, const double* __restrict__ part_bb, int nb, double tol,
                                                            int max_iterations, double* __restrict__ state) {
  __shared__ double lds[4];
  const double rr = fold_partials(part_rr, nb, lds), bb = fold_partials(part_bb, nb, lds);
  if (threadIdx.x == 0) {
    state[0] = 0.0, state[1] = rr, state[2] = bb;
    state[3] = (rr <= (tol * tol) * bb || max_iterations <= 0) ? 1.0 : 0.0;
  }
}
// launch 1 of an iteration: A p and the partials of p . A p
__global__ void __launch_bounds__(POISSON_BLOCK) k_cg_apply(const float* __restrict__ p, const float* __restrict__ s, PGridK g, float* __restrict__ Ap,
                                                            double* __restrict__ part_pAp, const double* __restrict__ state, int64_t total) {
  __shared__ double lds[4];
  if (state[3] != 0.0) return;
  double acc = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x; e < total; e += (int64_t)gridDim.x * PB) {
    int i, j, k;
    lattice_of((uint32_t)e, g, i, j, k);
    const float a = (float)apply_at(p, s, g, i, j, k, e);
    Ap[e] = a;
    acc += (double)p[e] * (double)a;
  }
  acc = block_sum_d(acc, lds);
  if (threadIdx.x == 0) part_pAp[blockIdx.x] = acc;
}
// launch 2: alpha = r . r / p . A p; x += alpha p, r -= alpha A p (each in double, rounded once); the partials of the new r . r
__global__ void __launch_bounds__(POISSON_BLOCK) k_cg_update(float* __restrict__ x, float* __restrict__ r, const float* __restrict__ p,
                                                             const float* __restrict__ Ap, const double* __restrict__ part_pAp,
                                                             double* __restrict__ part_rr, const double* __restrict__ state, int64_t total) {
  __shared__ double lds[4];
  if (state[3] != 0.0) return;
  const double pAp = fold_partials(part_pAp, (int)gridDim.x, lds);
  const double alpha = pAp > 0.0 ? state[1] / pAp : 0.0;
  double acc = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x; e < total; e += (int64_t)gridDim.x * PB) {
    x[e] = (float)((double)x[e] + alpha * (double)p[e]);
    const float re = (float)((double)r[e] - alpha * (double)Ap[e]);
    r[e] = re;
    acc += (double)re * (double)re;
  }
  acc = block_sum_d(acc, lds);
  if (threadIdx.x == 0) part_rr[blockIdx.x] = acc;
}
// launch 3: beta = new r . r / old r . r; p = r + beta p; block 0 writes the next state slot (a copy of this one once the run has stopped)
__global__ void __launch_bounds__(POISSON_BLOCK) k_cg_direction(const float* __restrict__ r, float* __restrict__ p, const double* __restrict__ part_rr,
                                                                const double* __restrict__ state, double* __restrict__ next, double tol,
                                                                int max_iterations, int64_t total) {
  __shared__ double lds[4];
  if (state[3] != 0.0) {
    if (blockIdx.x == 0 && threadIdx.x < CG_STATE_DOUBLES) next[threadIdx.x] = state[threadIdx.x];
    return;
  }
  const double rr_new = fold_partials(part_rr, (int)gridDim.x, lds), rr_old = state[1];
  const double beta = rr_old > 0.0 ? rr_new / rr_old : 0.0;
  for (int64_t e = (int64_t)blockIdx.x * PB + threadIdx.x; e < total; e += (int64_t)gridDim.x * PB)
    p[e] = (float)((double)r[e] + beta * (double)p[e]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double it = state[0] + 1.0, bb = state[2];
    next[0] = it, next[1] = rr_new, next[2] = bb;
    next[3] = (rr_new <= (tol * tol) * bb || it >= (double)max_iterations) ? 1.0 : 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------- host
int bit_length(int64_t v) {  // bits that hold 0..v (at least 1)
  int b = 1;
  while ((v >> b) != 0) ++b;
  return b;
}
bool positive(float v) { return v > 0.0f && v <= 3.4028234663852886e38f; }
bool finite3(float a, float b, float c) { return a - a == 0.0f && b - b == 0.0f && c - c == 0.0f; }
bool dims_ok(int32_t X, int32_t Y, int32_t Z) { return X >= 2 && Y >= 2 && Z >= 2 && (int64_t)X * Y <= POISSON_MAX && (int64_t)X * Y * Z <= POISSON_MAX; }
bool count_ok(int64_t n) { return n >= 0 && n <= POISSON_MAX; }

int grid_check(const char* name, int32_t X, int32_t Y, int32_t Z, float hx, float hy, float hz) {
  TN_REQUIRE(dims_ok(X, Y, Z), "%s: a lattice of %d x %d x %d points (each >= 2, below 2^31 in all)", name, X, Y, Z);
  TN_REQUIRE(positive(hx) && positive(hy) && positive(hz), "%s: the voxel size must be positive and finite", name);
  return TN_OK;
}
PGridK make_grid(int32_t X, int32_t Y, int32_t Z, float ox, float oy, float oz, float hx, float hy, float hz) {
  return PGridK{X, Y, Z, (double)ox, (double)oy, (double)oz, (double)hx, (double)hy, (double)hz};
}
unsigned blocks_of(int64_t n) { return (unsigned)tn_cdiv(n, PB); }
int solve_blocks(int64_t total) { return (int)std::min<int64_t>(tn_cdiv(total, PB), POISSON_MAX_BLOCKS); }

struct PlanLayout {
  int64_t keys, sorted, order, start, tmp, tmp_bytes, total;
};
// rocprim's scratch cannot be sized without a device: the layout reserves a bound (a second copy of keys and values, histograms and look-back state)
// and tn_poisson_bin, which runs where a device is, checks rocprim's own figure against it before the first launch
PlanLayout plan_layout(int64_t n, int64_t cells) {
  PlanLayout L;
  int64_t at = 0;
  auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at += align256(bytes);
    return here;
  };
  L.keys = take(n * 4), L.sorted = take(n * 4), L.order = take(n * 4), L.start = take((cells + 1) * 4);
  L.tmp_bytes = align256(n * 12 + (1ll << 20));
  L.tmp = take(L.tmp_bytes);
  L.total = at;
  return L;
}
int64_t cells_of(int32_t X, int32_t Y, int32_t Z) { return (int64_t)(X - 1) * (Y - 1) * (Z - 1); }

struct SolveLayout {
  int64_t r, p, Ap, part_a, part_b, state, total;
};
SolveLayout solve_layout(int64_t total) {
  SolveLayout L;
  int64_t at = 0;
  auto take = [&at](int64_t bytes) {
    const int64_t here = at;
    at += align256(bytes);
    return here;
  };
  L.r = take(total * 4), L.p = take(total * 4), L.Ap = take(total * 4);
  L.part_a = take(POISSON_MAX_BLOCKS * 8), L.part_b = take(POISSON_MAX_BLOCKS * 8), L.state = take(2 * CG_STATE_DOUBLES * 8);
  L.total = at;
  return L;
}

}  // namespace

extern "C" int64_t tn_poisson_workspace_bytes(int64_t n, int32_t X, int32_t Y, int32_t Z) {
  if (!count_ok(n) || !dims_ok(X, Y, Z)) return -1;
  return n == 0 ? 0 : plan_layout(n, cells_of(X, Y, Z)).total;
}

extern "C" int tn_poisson_bin(const float* points, int64_t n, int32_t X, int32_t Y, int32_t Z, float origin_x, float origin_y, float origin_z,
                              float voxel_x, float voxel_y, float voxel_z, void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  TN_REQUIRE(count_ok(n), "tn_poisson_bin: %lld points (0..2^31 - 1)", (long long)n);
  if (const int rc = grid_check("tn_poisson_bin", X, Y, Z, voxel_x, voxel_y, voxel_z)) return rc;
  TN_REQUIRE(finite3(origin_x, origin_y, origin_z), "tn_poisson_bin: the origin must be finite");
  if (n == 0) return TN_OK;
  TN_REQUIRE(points && workspace, "tn_poisson_bin: null pointer");
  TN_REQUIRE(((uintptr_t)workspace & 255) == 0, "tn_poisson_bin: the workspace must be 256-byte aligned");
  const int64_t cells = cells_of(X, Y, Z);
  const PlanLayout L = plan_layout(n, cells);
  TN_REQUIRE(workspace_bytes >= L.total, "tn_poisson_bin: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  char* ws = static_cast<char*>(workspace);
  uint32_t *keys = reinterpret_cast<uint32_t*>(ws + L.keys), *sorted = reinterpret_cast<uint32_t*>(ws + L.sorted);
  int32_t *order = reinterpret_cast<int32_t*>(ws + L.order), *start = reinterpret_cast<int32_t*>(ws + L.start);
  const int key_bits = bit_length(cells);  // the sentinel `cells` included
  size_t need = 0;
  if (rocprim::radix_sort_pairs(nullptr, need, (uint32_t*)nullptr, (uint32_t*)nullptr, rocprim::counting_iterator<int32_t>(0), (int32_t*)nullptr, (size_t)n,
                                0, key_bits) != hipSuccess ||
      (int64_t)need > L.tmp_bytes) {
    tn_set_error("tn_poisson_bin: rocprim's scratch for %lld points does not fit the %lld bytes reserved for it", (long long)n, (long long)L.tmp_bytes);
    return TN_ELAUNCH;
  }
  const PGridK g = make_grid(X, Y, Z, origin_x, origin_y, origin_z, voxel_x, voxel_y, voxel_z);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_poisson_keys, dim3(blocks_of(n)), dim3(POISSON_BLOCK), 0, st, points, n, g, (uint32_t)cells, keys);
  TN_CHECK_LAUNCH("tn_poisson_bin(keys)");
  size_t tb = (size_t)L.tmp_bytes;
  if (rocprim::radix_sort_pairs(ws + L.tmp, tb, keys, sorted, rocprim::counting_iterator<int32_t>(0), order, (size_t)n, 0, key_bits, st) != hipSuccess) {
    tn_set_error("tn_poisson_bin: rocprim's sort failed");
    return TN_ELAUNCH;
  }
  hipLaunchKernelGGL(k_poisson_cell_starts, dim3(blocks_of(cells + 1)), dim3(POISSON_BLOCK), 0, st, (const uint32_t*)sorted, n, (uint32_t)cells, start);
  TN_CHECK_LAUNCH("tn_poisson_bin(cell starts)");
  return TN_OK;
}

extern "C" int tn_poisson_splat(const float* points, int64_t n, const float* values, int32_t C, const float* weights, int32_t normalize, int32_t X,
                                int32_t Y, int32_t Z, float origin_x, float origin_y, float origin_z, float voxel_x, float voxel_y, float voxel_z,
                                float* out, const void* workspace, int64_t workspace_bytes, tn_stream_t stream) {
  TN_REQUIRE(count_ok(n), "tn_poisson_splat: %lld points (0..2^31 - 1)", (long long)n);
  if (const int rc = grid_check("tn_poisson_splat", X, Y, Z, voxel_x, voxel_y, voxel_z)) return rc;
  TN_REQUIRE(finite3(origin_x, origin_y, origin_z), "tn_poisson_splat: the origin must be finite");
  TN_REQUIRE(C >= 1 && C <= 4 && (values != nullptr || C == 1 || n == 0), "tn_poisson_splat: C = %d (1..4; 1 without a value array)", C);
  TN_REQUIRE(normalize == 0 || normalize == 1, "tn_poisson_splat: normalize = %d (0 or 1)", normalize);
  TN_REQUIRE(out, "tn_poisson_splat: null pointer");
  const int64_t total = (int64_t)X * Y * Z;
  hipStream_t st = tn_s(stream);
  if (n == 0) {
    hipLaunchKernelGGL(k_poisson_zero, dim3((unsigned)std::min<int64_t>(tn_cdiv(total * C, PB), 4096)), dim3(POISSON_BLOCK), 0, st, out, total * C);
    TN_CHECK_LAUNCH("tn_poisson_splat(zero)");
    return TN_OK;
  }
  TN_REQUIRE(points && workspace, "tn_poisson_splat: null pointer");
  TN_REQUIRE(((uintptr_t)workspace & 255) == 0, "tn_poisson_splat: the workspace must be 256-byte aligned");
  const PlanLayout L = plan_layout(n, cells_of(X, Y, Z));
  TN_REQUIRE(workspace_bytes >= L.total, "tn_poisson_splat: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  const char* ws = static_cast<const char*>(workspace);
  const PGridK g = make_grid(X, Y, Z, origin_x, origin_y, origin_z, voxel_x, voxel_y, voxel_z);
  hipLaunchKernelGGL(k_poisson_splat, dim3(blocks_of(total)), dim3(POISSON_BLOCK), 0, st, points, values, (int)C, weights, (int)normalize, g,
                     reinterpret_cast<const int32_t*>(ws + L.order), reinterpret_cast<const int32_t*>(ws + L.start), out, total);
  TN_CHECK_LAUNCH("tn_poisson_splat");
  return TN_OK;
}

extern "C" int tn_poisson_sample(const float* points, int64_t n, const float* volume, int32_t X, int32_t Y, int32_t Z, float origin_x, float origin_y,
                                 float origin_z, float voxel_x, float voxel_y, float voxel_z, double* out, tn_stream_t stream) {
  TN_REQUIRE(count_ok(n), "tn_poisson_sample: %lld points (0..2^31 - 1)", (long long)n);
  if (const int rc = grid_check("tn_poisson_sample", X, Y, Z, voxel_x, voxel_y, voxel_z)) return rc;
  TN_REQUIRE(finite3(origin_x, origin_y, origin_z), "tn_poisson_sample: the origin must be finite");
  if (n == 0) return TN_OK;
  TN_REQUIRE(points && volume && out, "tn_poisson_sample: null pointer");
  const PGridK g = make_grid(X, Y, Z, origin_x, origin_y, origin_z, voxel_x, voxel_y, voxel_z);
  hipLaunchKernelGGL(k_poisson_sample, dim3(blocks_of(n)), dim3(POISSON_BLOCK), 0, tn_s(stream), points, n, volume, g, out);
  TN_CHECK_LAUNCH("tn_poisson_sample");
  return TN_OK;
}

extern "C" int tn_poisson_divergence(const float* field, int32_t X, int32_t Y, int32_t Z, float voxel_x, float voxel_y, float voxel_z, float* out,
                                     tn_stream_t stream) {
  if (const int rc = grid_check("tn_poisson_divergence", X, Y, Z, voxel_x, voxel_y, voxel_z)) return rc;
  TN_REQUIRE(field && out, "tn_poisson_divergence: null pointer");
  const PGridK g = make_grid(X, Y, Z, 0.0f, 0.0f, 0.0f, voxel_x, voxel_y, voxel_z);
  const int64_t total = (int64_t)X * Y * Z;
  hipLaunchKernelGGL(k_poisson_divergence, dim3(blocks_of(total)), dim3(POISSON_BLOCK), 0, tn_s(stream), field, g, out, total);
  TN_CHECK_LAUNCH("tn_poisson_divergence");
  return TN_OK;
}

extern "C" int tn_poisson_apply(const float* x, const float* screening, int32_t X, int32_t Y, int32_t Z, float voxel_x, float voxel_y, float voxel_z,
                                float* out, tn_stream_t stream) {
  if (const int rc = grid_check("tn_poisson_apply", X, Y, Z, voxel_x, voxel_y, voxel_z)) return rc;
  TN_REQUIRE(x && out, "tn_poisson_apply: null pointer");
  TN_REQUIRE(x != out, "tn_poisson_apply: out must not be x");
  const PGridK g = make_grid(X, Y, Z, 0.0f, 0.0f, 0.0f, voxel_x, voxel_y, voxel_z);
  const int64_t total = (int64_t)X * Y * Z;
  hipLaunchKernelGGL(k_poisson_apply, dim3(blocks_of(total)), dim3(POISSON_BLOCK), 0, tn_s(stream), x, screening, g, out, total);
  TN_CHECK_LAUNCH("tn_poisson_apply");
  return TN_OK;
}

extern "C" int64_t tn_poisson_solve_workspace_bytes(int32_t X, int32_t Y, int32_t Z) {
  if (!dims_ok(X, Y, Z)) return -1;
  return solve_layout((int64_t)X * Y * Z).total;
}

extern "C" int tn_poisson_solve(const float* b, const float* screening, float* x, int32_t X, int32_t Y, int32_t Z, float voxel_x, float voxel_y,
                                float voxel_z, double tol, int32_t max_iterations, int32_t check_every, double* record, void* workspace,
                                int64_t workspace_bytes, tn_stream_t stream) {
  if (const int rc = grid_check("tn_poisson_solve", X, Y, Z, voxel_x, voxel_y, voxel_z)) return rc;
  TN_REQUIRE(tol >= 0.0 && tol <= 1.7976931348623157e308, "tn_poisson_solve: tol = %g (>= 0, finite)", tol);
  TN_REQUIRE(max_iterations >= 0, "tn_poisson_solve: max_iterations = %d (>= 0)", max_iterations);
  TN_REQUIRE(check_every >= 1, "tn_poisson_solve: check_every = %d (>= 1)", check_every);
  TN_REQUIRE(b && x && record && workspace, "tn_poisson_solve: null pointer");
  TN_REQUIRE(((uintptr_t)workspace & 255) == 0, "tn_poisson_solve: the workspace must be 256-byte aligned");
  const int64_t total = (int64_t)X * Y * Z;
  const SolveLayout L = solve_layout(total);
  TN_REQUIRE(workspace_bytes >= L.total, "tn_poisson_solve: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)L.total);
  char* ws = static_cast<char*>(workspace);
  float *r = reinterpret_cast<float*>(ws + L.r), *p = reinterpret_cast<float*>(ws + L.p), *Ap = reinterpret_cast<float*>(ws + L.Ap);
  double *part_a = reinterpret_cast<double*>(ws + L.part_a), *part_b = reinterpret_cast<double*>(ws + L.part_b);
  double* state = reinterpret_cast<double*>(ws + L.state);
  const PGridK g = make_grid(X, Y, Z, 0.0f, 0.0f, 0.0f, voxel_x, voxel_y, voxel_z);
  const int nb = solve_blocks(total);
  hipStream_t st = tn_s(stream);
  hipLaunchKernelGGL(k_cg_init, dim3(nb), dim3(POISSON_BLOCK), 0, st, b, screening, (const float*)x, g, r, p, part_a, part_b, total);
  TN_CHECK_LAUNCH("tn_poisson_solve(init)");
  hipLaunchKernelGGL(k_cg_start, dim3(1), dim3(POISSON_BLOCK), 0, st, (const double*)part_a, (const double*)part_b, nb, tol, (int)max_iterations, state);
  TN_CHECK_LAUNCH("tn_poisson_solve(start)");
  double host[CG_STATE_DOUBLES] = {0.0, 0.0, 0.0, 0.0};
  int32_t it = 0;
  for (;;) {  // the only host synchronisations: one read-back of the state slot per check_every iterations
    const int32_t until = (int32_t)std::min<int64_t>((int64_t)it + check_every, max_iterations);
    for (; it < until; ++it) {
      const double* cur = state + (it & 1) * CG_STATE_DOUBLES;
      double* next = state + ((it + 1) & 1) * CG_STATE_DOUBLES;
      hipLaunchKernelGGL(k_cg_apply, dim3(nb), dim3(POISSON_BLOCK), 0, st, (const float*)p, screening, g, Ap, part_a, cur, total);
      hipLaunchKernelGGL(k_cg_update, dim3(nb), dim3(POISSON_BLOCK), 0, st, x, r, (const float*)p, (const float*)Ap, (const double*)part_a, part_b, cur,
                         total);
      hipLaunchKernelGGL(k_cg_direction, dim3(nb), dim3(POISSON_BLOCK), 0, st, (const float*)r, p, (const double*)part_b, cur, next, tol,
                         (int)max_iterations, total);
      TN_CHECK_LAUNCH("tn_poisson_solve(iteration)");
    }
    if (hipMemcpyAsync(host, state + (it & 1) * CG_STATE_DOUBLES, sizeof(host), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      tn_set_error("tn_poisson_solve: reading the record back failed: %s", hipGetErrorString(hipGetLastError()));
      return TN_ELAUNCH;
    }
    if (host[3] != 0.0 || it >= max_iterations) break;
  }
  record[0] = host[0], record[1] = host[1], record[2] = host[2];
  return TN_OK;
}
