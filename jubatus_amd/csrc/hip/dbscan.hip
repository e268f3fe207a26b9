// DBSCAN over a weighted coreset: the density graph on the GPU.
//
// The reference (Jubatus 0.9.2) clusters with k-means and GMM only; the
// dbscan method and its order-independent definition are this project's own
// (docs/clustering_dbscan.md), and parity with later Jubatus releases is
// unpinned. models/clustering.py holds the float64 host path of the same
// five rules.
//
// Points x_0..x_{n-1} (d dims), weights w_i >= 0, eps2 = eps^2, min_mass:
//   1. A[i][j] = |x_i - x_j|^2 <= eps2, A[i][i] = 1
//   2. mass[i] = sum_j A[i][j] w[j];  core[i] = mass[i] >= min_mass
//   3. connected components of the core points under A; a core point's label
//      is the smallest point index of its component
//   4. a non-core point takes the smallest label among its core neighbours,
//      -1 (noise) without one
//
// Launch chain (one stream, no host synchronisation in between):
//   adj_kernel      adjacency bitmap adj[n][nw] (nw = ceil(n / 64) words of 64
//                   bits, bit j & 63 of word j >> 6 is A[i][j]); the distances
//                   d2 = max((xn2[i] + xn2[j]) - 2 g, 0) with the Gram term g on
//                   v_mfma_f32_16x16x4_f32 (fragment maps as sqdist_mfma_kernel
//                   of clustering.hip). One wave owns 16 rows x 64 columns: four
//                   16 x 16 tiles on four independent accumulators, their
//                   compare results packed by 16 ballots, and lanes 0..15 each
//                   store one finished word. g(i, j) and g(j, i) multiply the
//                   same pairs in the same k order and both norms come from
//                   xn2, so the bitmap is bitwise symmetric with no second pass.
//   mass_kernel     one wave per row: every lane sums w over the set bits of
//                   its words (ascending words, ascending bits), the lanes are
//                   combined by the xor butterfly: a fixed order, the same bits
//                   on every launch
//   core_kernel     core bitmap [nw] by ballot, parent[i] = i
//   union_kernel    one thread per (row, word): for a core row i every set bit
//                   j > i of adj[i] & core is united with i, lock-free:
//                   atomicCAS(&parent[hi], hi, lo) on the two roots, hi > lo.
//                   Parents only ever point to smaller indices, so no cycle can
//                   form and the final root of a component is its minimum under
//                   any interleaving. parent is read with agent-scope atomic
//                   loads (past the CU's L1) and written with agent-scope
//                   atomics only; a read that is stale all the same can only
//                   show an older, still valid ancestor, and a failed CAS
//                   returns the current parent, from which the retry goes on:
//                   max(root a, root b) falls with every retry.
//   flatten_kernel  label[i] = find(i) for core points, -1 otherwise: a launch
//                   of its own, so every root is final before the border stage
//   border_kernel   rule 4 for the non-core points, one wave per row
//
// Every loop is bounded: a find walks at most n steps, a union retries at
// most n times. Running out writes a code to status[0] (1: find, 2: union)
// and the thread moves on, so a bug shows as an error code, never as a hung
// queue. No float atomics, no LDS.
#include <math.h>

#include "jb_device.hpp"
#include "jb_hip_api.h"

namespace jb {

typedef float dbs_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kDbscanMaxN = 65536;   // adj is n * n / 8 bytes: 512 MB here
constexpr int kDbscanThreads = 256;

__global__ __launch_bounds__(kDbscanThreads) void dbscan_adj_kernel(
    const float* __restrict__ X, int n, int d, const float* __restrict__ xn2, float eps2, int nw,
    uint64_t* __restrict__ adj) {
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int row0 = (blockIdx.x * 4 + wv) * 16;
  const int wcol = blockIdx.y;               // word column: columns wcol * 64 ..
  if (row0 >= n) return;                     // wave-uniform
  const int ar = lane & 15;                  // A row / B column inside a tile
  const int kq = lane >> 4;                  // k offset 0..3
  const int xi = row0 + ar;
  const float* xa = X + (int64_t)min(xi, n - 1) * d;
  const float* xb[4];
  bool bin[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int cj = wcol * 64 + t * 16 + ar;
    bin[t] = cj < n;
    xb[t] = X + (int64_t)min(cj, n - 1) * d;
  }
  dbs_f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = dbs_f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kk = 0; kk < d; kk += 4) {
    const int kc = kk + kq;
    const bool kin = kc < d;
    const float a = (xi < n && kin) ? xa[kc] : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float b = (bin[t] && kin) ? xb[t][kc] : 0.f;
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
    }
  }
  // D: lane l, reg r -> row (l >> 4) * 4 + r, col l & 15. The ballot of reg r
  // holds row 4 q + r in its bits 16 q .. 16 q + 15.
  float rn[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) rn[r] = xn2[min(row0 + kq * 4 + r, n - 1)];
  uint64_t word = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int col = wcol * 64 + t * 16 + ar;
    const float cn = xn2[min(col, n - 1)];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + kq * 4 + r;
      const float d2 = fmaxf((rn[r] + cn) - 2.f * acc[t][r], 0.f);
      const bool on = col < n && (d2 <= eps2 || row == col);
      const uint64_t b = __ballot(on);
      if ((lane & 3) == r) word |= ((b >> (16 * ((lane >> 2) & 3))) & 0xffffull) << (16 * t);
    }
  }
  // lane l < 16 has gathered row row0 + l (r = l & 3, q = l >> 2)
  if (lane < 16 && row0 + lane < n) adj[(int64_t)(row0 + lane) * nw + wcol] = word;
}

__global__ __launch_bounds__(kDbscanThreads) void dbscan_mass_kernel(
    const uint64_t* __restrict__ adj, const float* __restrict__ w, int n, int nw,
    float* __restrict__ mass) {
  const int lane = threadIdx.x & 63;
  const int i = (int)(((int64_t)blockIdx.x * kDbscanThreads + threadIdx.x) >> 6);
  if (i >= n) return;                        // wave-uniform
  const uint64_t* row = adj + (int64_t)i * nw;
  float s = 0.f;
  for (int q = lane; q < nw; q += 64) {
    uint64_t b = row[q];
    while (b) {
      const int j = q * 64 + __builtin_ctzll(b);
      b &= b - 1;
      s += w[j];
    }
  }
  s = wave_sum(s);
  if (lane == 0) mass[i] = s;
}

__global__ __launch_bounds__(kDbscanThreads) void dbscan_core_kernel(
    const float* __restrict__ mass, float min_mass, int n, uint64_t* __restrict__ core,
    int32_t* __restrict__ parent) {
  const int i = blockIdx.x * kDbscanThreads + threadIdx.x;   // a wave covers one core word
  const bool on = i < n && mass[i] >= min_mass;
  const uint64_t b = __ballot(on);
  if (i < n) parent[i] = i;
  if ((threadIdx.x & 63) == 0 && i < n) core[i >> 6] = b;
}

__device__ __forceinline__ int dbs_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x, halving the path on the way (atomicMin keeps parents falling);
// -1 with status[0] = 1 when the walk does not end within n steps
__device__ int dbs_find(int32_t* parent, int x, int n, int32_t* status) {
  for (int s = 0; s <= n; ++s) {
    const int p = dbs_load(parent + x);
    if (p == x) return x;
    const int g = dbs_load(parent + p);
    if (g != p) atomicMin(parent + x, g);
    x = g;
  }
  status[0] = 1;
  return -1;
}

__device__ int dbs_union(int32_t* parent, int a, int b, int n, int32_t* status) {
  for (int t = 0; t <= n; ++t) {
    a = dbs_find(parent, a, n, status);
    b = dbs_find(parent, b, n, status);
    if (a < 0 || b < 0) return -1;
    if (a == b) return a;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return lo;
    a = old;                                 // hi has a parent by now: go on from it
    b = lo;
  }
  status[0] = 2;
  return -1;
}

__global__ __launch_bounds__(kDbscanThreads) void dbscan_union_kernel(
    const uint64_t* __restrict__ adj, const uint64_t* __restrict__ core, int n, int nw,
    int32_t* parent, int32_t* status) {
  const int64_t t = (int64_t)blockIdx.x * kDbscanThreads + threadIdx.x;
  if (t >= (int64_t)n * nw) return;
  const int i = (int)(t / nw), q = (int)(t % nw);
  if (q * 64 + 63 <= i) return;              // only j > i
  if (!((core[i >> 6] >> (i & 63)) & 1)) return;
  uint64_t b = adj[t] & core[q];
  if (q == (i >> 6)) b &= ~((2ull << (i & 63)) - 1);   // clear bits 0..i&63
  int root = i;
  while (b) {
    const int j = q * 64 + __builtin_ctzll(b);
    b &= b - 1;
    const int r = dbs_union(parent, root, j, n, status);
    if (r >= 0) root = r;
  }
}

__global__ __launch_bounds__(kDbscanThreads) void dbscan_flatten_kernel(
    const uint64_t* __restrict__ core, int n, int32_t* parent, int32_t* __restrict__ label,
    int32_t* status) {
  const int i = blockIdx.x * kDbscanThreads + threadIdx.x;
  if (i >= n) return;
  const bool on = (core[i >> 6] >> (i & 63)) & 1;
  label[i] = on ? dbs_find(parent, i, n, status) : -1;
}

__global__ __launch_bounds__(kDbscanThreads) void dbscan_border_kernel(
    const uint64_t* __restrict__ adj, const uint64_t* __restrict__ core, int n, int nw,
    int32_t* label) {
  const int lane = threadIdx.x & 63;
  const int i = (int)(((int64_t)blockIdx.x * kDbscanThreads + threadIdx.x) >> 6);
  if (i >= n) return;                        // wave-uniform
  if ((core[i >> 6] >> (i & 63)) & 1) return;
  // reads the labels of core points (final since flatten), writes those of
  // non-core points only
  const uint64_t* row = adj + (int64_t)i * nw;
  int best = 0x7fffffff;
  for (int q = lane; q < nw; q += 64) {
    uint64_t b = row[q] & core[q];
    while (b) {
      const int j = q * 64 + __builtin_ctzll(b);
      b &= b - 1;
      best = min(best, label[j]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
  if (lane == 0) label[i] = best == 0x7fffffff ? -1 : best;
}

}  // namespace jb

// X [n, d] fp32, xn2 [n] its row norms, w [n] weights; out: adj [n, nw] words,
// mass [n], label [n] (smallest point index of the cluster, -1 noise), status
// [1]; scratch: core [nw] words, parent [n]. 0: queued; -2: an argument out of
// range (nothing launched); otherwise the HIP error of a launch.
extern "C" int jb_dbscan(const float* X, int n, int d, const float* xn2, const float* w, float eps2,
                         float min_mass, uint64_t* adj, float* mass, uint64_t* core,
                         int32_t* parent, int32_t* label, int32_t* status, hipStream_t stream) {
  if (n < 1 || n > jb::kDbscanMaxN || d < 1) return -2;
  if (!(eps2 >= 0.f) || !(eps2 < INFINITY) || !(min_mass > 0.f)) return -2;
  if (X == nullptr || xn2 == nullptr || w == nullptr || adj == nullptr || mass == nullptr ||
      core == nullptr || parent == nullptr || label == nullptr || status == nullptr)
    return -2;
  const int nw = (n + 63) / 64;
  const int T = jb::kDbscanThreads;
  const dim3 blk(T);
  const dim3 per_thread((n + T - 1) / T);
  const dim3 per_wave((int)(((int64_t)n * 64 + T - 1) / T));
  const dim3 per_word((int)(((int64_t)n * nw + T - 1) / T));
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(jb::dbscan_adj_kernel, dim3((n + 63) / 64, nw), blk, 0, stream, X, n, d, xn2,
                     eps2, nw, adj);
  hipLaunchKernelGGL(jb::dbscan_mass_kernel, per_wave, blk, 0, stream, adj, w, n, nw, mass);
  hipLaunchKernelGGL(jb::dbscan_core_kernel, per_thread, blk, 0, stream, mass, min_mass, n, core,
                     parent);
  hipLaunchKernelGGL(jb::dbscan_union_kernel, per_word, blk, 0, stream, adj, core, n, nw, parent,
                     status);
  hipLaunchKernelGGL(jb::dbscan_flatten_kernel, per_thread, blk, 0, stream, core, n, parent, label,
                     status);
  hipLaunchKernelGGL(jb::dbscan_border_kernel, per_wave, blk, 0, stream, adj, core, n, nw, label);
  return (int)hipGetLastError();
}
