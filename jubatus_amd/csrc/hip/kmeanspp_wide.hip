// k-means++ seeding on the whole GPU, for points past the LDS-resident
// kernels of clustering.hip (kmeanspp_wave_kernel, kmeanspp_blk_kernel), where
// jb_kmeanspp falls to one workgroup that walks all n x d floats per draw.
// Same draw rule as those kernels and models/clustering.py _kmeanspp:
//   draw j picks min(bisect_right(cum, u[j] cum[-1]), n - 1), cum the double
//   running sum in row order of p_i = fl32(d2_i w_i) (draw 0: p_i = w_i), d2_i
//   the fp32 minimum over the rows chosen so far of sum_q (x_iq - c_q)^2 in
//   the direct form, an fmaf chain in ascending q. (Not the norm expansion: it
//   cancels for near points, and those near-zero masses are what the draw
//   weighs.) Zero mass at draw j: out[j] = -1, status = j + 1, and the host
//   finishes with its uniform fallback, as after jb_kmeanspp.
//
// The chain: one launch per draw, queued back to back with no host
// synchronisation, and a tail launch. Workgroup g of G owns the contiguous
// rows [g L, g L + L): the bisect runs over rows in index order, so a
// workgroup's mass is one term of the prefix. G <= kMaxGrid and L (a multiple
// of 64) are fixed functions of n. Launch j
//   1. leaves if the status word is set (a stopped chain falls through);
//   2. relaxes its rows against row out[j - 1], 256 rows a tile, one thread a
//      row: the tile and the centre move through LDS in chunks of kDC columns
//      with coalesced loads, the next chunk's loads in flight in registers
//      while this one is summed; the tile's row stride kXS is odd, so the 64
//      lanes of a wave walk 64 distinct banks. Nothing of size d is in LDS.
//      d2_i = fminf(d2_i, dist), nearest_i = j - 1 where dist < d2_i strictly:
//      the first nearest in draw order on ties;
//   3. sums its rows' p_i in double in a fixed order and stores the partial;
//   4. every thread fences (agent-scope release), thread 0 takes a ticket; the
//      workgroup with the last ticket fences (acquire), scans the G partials
//      in workgroup order, finds the workgroup whose interval holds
//      u[j] total, rescans that workgroup's rows (d2 w recomputed, double, row
//      order), writes out[j] and resets the ticket.
// The tail launch only relaxes against out[m - 1]: d2 and nearest then
// describe all m representatives. No grid barrier, no cooperative launch, no
// float atomics; every sum has a fixed order, so two runs give the same bits.
//
// The matrix cores do not fit here: a draw is one matrix-vector pass of
// subtract-square-add (not a product of two operands), and the chain is
// sequential in its draws, so there is never a second centre to batch with.
#include "jb_hip_api.h"
#include "jb_slab.hpp"

namespace jb {
namespace kpw {

using jb::slab::kDC;        // columns per chunk in LDS
using jb::slab::kMaxGrid;   // one workgroup a CU
using jb::slab::kT;         // threads of every kernel

constexpr int kXS = kDC + 1;              // row stride of the tile: odd, a thread-per-row walk hits 64 banks
constexpr int kState = 4;                 // int32 words: ticket, status, unused x 2
// jb_kmeanspp_wide_pays: the chain from this many floats of X on. Measured (tools/kpp_bench.py
// --wide, profiles/kmeanspp_wide.md): slower at 12 000 floats, faster at every m from 80 000 on.
constexpr int64_t kPaysFloats = (int64_t)1 << 17;

struct Geo {
  int G;        // workgroups; 0: outside the range
  int64_t L;    // rows a workgroup owns
};

__host__ inline Geo geometry(int64_t n, int64_t d, int64_t m) {
  Geo g = {0, 0};
  if (n < 1 || n > INT32_MAX || d < 1 || d > INT32_MAX || m < 1 || m > n) return g;
  g.L = ((n + kMaxGrid - 1) / kMaxGrid + 63) / 64 * 64;
  g.G = (int)((n + g.L - 1) / g.L);
  return g;
}

// the wave's sum in every lane, a fixed butterfly
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the block's sum in a fixed order, every thread gets it (red: 4 doubles)
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();                   // (red may still be read from the previous call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// Inclusive prefix sums of v over the block's threads; *excl is exactly the
// previous thread's inclusive sum, so the intervals [excl, incl) tile
// [0, total) with no gap and no overlap. sc: kT + 4 doubles.
__device__ __forceinline__ double block_scan_d(double v, double* sc, double* excl) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  double incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double x = __shfl_up(incl, o, 64);
    if (lane >= o) incl += x;
  }
  __syncthreads();                   // (sc may still be read from the previous call)
  if (lane == 63) sc[kT + wv] = incl;
  __syncthreads();
  double base = 0.0;
  for (int k = 0; k < wv; ++k) base += sc[kT + k];
  incl += base;
  sc[t] = incl;
  __syncthreads();
  *excl = t > 0 ? sc[t - 1] : 0.0;
  return incl;
}

constexpr int kRows = kT / kDC;             // rows of a full chunk that one pass of the block's threads covers

// A full chunk, columns [q0, q0 + kDC) of the tile's rows [t0, r1) and of the
// centre, into registers: thread t takes column t % kDC of rows t / kDC + kRows u,
// a wave two rows of 128 contiguous bytes. Rows past r1 load nothing.
__device__ __forceinline__ void load_full(float (&v)[kDC], float* vc, const float* __restrict__ X, int64_t d,
                                          int64_t t0, int64_t r1, int64_t c, int64_t q0) {
  const int t = threadIdx.x, i = t / kDC, q = t % kDC;
  const int rows = r1 - t0 < kT ? (int)(r1 - t0) : kT;
  const float* p = X + (t0 + i) * d + q0 + q;
#pragma unroll
  for (int u = 0; u < kDC; ++u) {
    v[u] = i + kRows * u < rows ? *p : 0.f;
    p += kRows * d;
  }
  *vc = t < kDC ? X[c * d + q0 + t] : 0.f;
}

__device__ __forceinline__ void store_full(const float (&v)[kDC], float vc, float* sX, float* sC) {
  const int t = threadIdx.x, i = t / kDC, q = t % kDC;
#pragma unroll
  for (int u = 0; u < kDC; ++u) sX[(i + kRows * u) * kXS + q] = v[u];
  if (t < kDC) sC[t] = vc;
}

// The last chunk when it is narrower (dc < kDC columns), straight into LDS:
// element e = row * dc + column, consecutive threads on consecutive floats
__device__ __forceinline__ void stage_part(float* sX, float* sC, const float* __restrict__ X, int64_t d, int64_t t0,
                                           int64_t r1, int64_t c, int64_t q0, int dc) {
  const int t = threadIdx.x;
  const int rows = r1 - t0 < kT ? (int)(r1 - t0) : kT;
  for (int e = t; e < rows * dc; e += kT) {
    const int i = e / dc, q = e - i * dc;
    sX[i * kXS + q] = X[(t0 + i) * d + q0 + q];
  }
  if (t < dc) sC[t] = X[c * d + q0 + t];
}

// sum_q (x_iq - c_q)^2 of row t0 + threadIdx.x against row c, ascending q
// (rows past r1: whatever the tile held, the caller drops them). Every thread
// of the block calls it: the tile is staged by all of them.
__device__ __forceinline__ float relax_tile(const float* __restrict__ X, int d, int64_t t0, int64_t r1, int64_t c,
                                            float* sX, float* sC) {
  float v[kDC], vc;
  const float* xr = sX + threadIdx.x * kXS;
  float s = 0.f;
  if (d >= kDC) load_full(v, &vc, X, d, t0, r1, c, 0);
  for (int64_t q0 = 0; q0 < d; q0 += kDC) {
    const int dc = d - q0 < kDC ? (int)(d - q0) : kDC;
    __syncthreads();                               // the last chunk's readers are done
    if (dc == kDC) store_full(v, vc, sX, sC);
    else stage_part(sX, sC, X, d, t0, r1, c, q0, dc);
    __syncthreads();
    if (dc == kDC) {
      if (q0 + 2 * kDC <= d) load_full(v, &vc, X, d, t0, r1, c, q0 + kDC);   // in flight while this chunk is summed
#pragma unroll
      for (int q = 0; q < kDC; ++q) {
        const float a = xr[q] - sC[q];
        s = fmaf(a, a, s);
      }
    } else {
      for (int q = 0; q < dc; ++q) {
        const float a = xr[q] - sC[q];
        s = fmaf(a, a, s);
      }
    }
  }
  return s;
}

// the mass of row i at draw j
__device__ __forceinline__ float mass_of(int j, const float* __restrict__ w, const float* d2, int64_t i) {
  return j == 0 ? w[i] : d2[i] * w[i];
}

__global__ void kmeanspp_wide_init_kernel(int32_t* state, int32_t* status) {
  if (threadIdx.x < kState) state[threadIdx.x] = 0;
  if (threadIdx.x == 0) *status = 0;
}

// launch j of the chain (0 <= j <= m; j == m: the tail). d2, part and state
// are written by one workgroup and read by another inside a launch: no
// __restrict__ on them, and the reader is behind the acquire fence.
__global__ __launch_bounds__(kT) void kmeanspp_wide_kernel(const float* __restrict__ X, int n, int d,
                                                           const float* __restrict__ w,
                                                           const double* __restrict__ u, int m, int j, int64_t L,
                                                           int32_t* out, int32_t* status, int32_t* nearest,
                                                           float* d2, double* part, int32_t* state) {
  __shared__ float sX[kT * kXS];
  __shared__ float sC[kDC];
  __shared__ double sc[kT + 4];
  __shared__ int s_last, s_g, s_row;
  __shared__ double s_base;
  if (j > 0 && state[1]) return;                   // stopped at an earlier draw
  const int t = threadIdx.x;
  const int64_t r0 = blockIdx.x * L, r1 = r0 + L < n ? r0 + L : n;
  const int64_t c = j > 0 ? out[j - 1] : 0;
  double mass = 0.0;                               // of rows r0 + t, r0 + t + kT, ...
  for (int64_t t0 = r0; t0 < r1; t0 += kT) {
    const int64_t i = t0 + t;
    float nd = 0.f;
    if (j > 0) {
      const float s = relax_tile(X, d, t0, r1, c, sX, sC);
      if (i < r1) {
        const float old = j == 1 ? INFINITY : d2[i];
        nd = fminf(old, s);
        if (j == 1 || s < old) {
          d2[i] = nd;
          if (nearest != nullptr) nearest[i] = j - 1;
        }
      }
    }
    if (j < m && i < r1) mass += (double)(j == 0 ? w[i] : nd * w[i]);
  }
  if (j == m) return;                              // the tail: every row relaxed against out[m - 1]
  const double mine = block_sum_d(mass, sc);
  if (t == 0) part[blockIdx.x] = mine;
  __threadfence();                                 // release: this thread's d2 rows, the partial
  __syncthreads();
  if (t == 0) s_last = atomicAdd(&state[0], 1) == (int)gridDim.x - 1;
  __syncthreads();
  if (!s_last) return;
  __threadfence();                                 // acquire: every other workgroup has taken its ticket
  // the pick, by the last workgroup
  const int G = (int)gridDim.x;                    // (<= kT: a thread a workgroup)
  double excl;
  double incl = block_scan_d(t < G ? part[t] : 0.0, sc, &excl);
  if (t == kT - 1) s_base = incl;
  if (t == 0) { s_g = -1; s_row = -1; }
  __syncthreads();
  const double total = s_base;
  if (!(total > 0.0)) {                            // no mass left: the host takes over
    if (t == 0) {
      out[j] = -1;
      state[1] = j + 1;
      *status = j + 1;
      state[0] = 0;
    }
    return;
  }
  const double target = u[j] * total;
  __syncthreads();                                 // (s_base is overwritten next)
  if (excl <= target && target < incl) { s_g = t; s_base = excl; }
  __syncthreads();
  int row = n - 1;                                 // u total rounded onto the end
  if (s_g >= 0) {
    // the rows of workgroup s_g, a contiguous run a thread
    const int64_t a0 = s_g * L, a1 = a0 + L < n ? a0 + L : n;
    const int64_t per = (a1 - a0 + kT - 1) / kT;
    const int64_t i0 = a0 + t * per < a1 ? a0 + t * per : a1, i1 = i0 + per < a1 ? i0 + per : a1;
    const double base = s_base;
    double sum = 0.0;
    int heavy = -1;                                // my last row with mass
    for (int64_t i = i0; i < i1; ++i) {
      const float p = mass_of(j, w, d2, i);
      sum += (double)p;
      if (p > 0.f) heavy = (int)i;
    }
    incl = block_scan_d(sum, sc, &excl);
    if (base + excl <= target && target < base + incl) {
      int r = heavy;                               // (the walk below may round short of the scan)
      double run = 0.0;
      for (int64_t i = i0; i < i1; ++i) {
        run += (double)mass_of(j, w, d2, i);
        if (base + (excl + run) > target) { r = (int)i; break; }
      }
      s_row = r;
    }
    __syncthreads();
    const int hit = s_row;
    __syncthreads();
    if (hit < 0) {                                 // the rescan rounded short of the partial: the last row with mass
      if (heavy >= 0) atomicMax(&s_row, heavy);
      __syncthreads();
    }
    if (s_row >= 0) row = s_row;
  }
  if (t == 0) {
    out[j] = row;
    state[0] = 0;                                  // the ticket, for the next launch
  }
}

}  // namespace kpw
}  // namespace jb

extern "C" int64_t jb_kmeanspp_wide_work(int n, int d, int m) {
  const jb::kpw::Geo g = jb::kpw::geometry(n, d, m);
  if (g.G == 0) return 0;
  // state | partials (double) [G] | d2 [n], the last 4 n bytes
  return 4 * jb::kpw::kState + 8 * (int64_t)g.G + 4 * (int64_t)n;
}

extern "C" int jb_kmeanspp_wide_pays(int n, int d, int m) {
  if (jb::kpw::geometry(n, d, m).G == 0) return 0;
  // jb_kmeanspp's LDS-resident kernels take it (clustering.hip: 64 P rows a
  // wave or 256 P4 rows a block, column-major, within 64 KiB)
  if (n <= 64 * 32) {
    const int P = n <= 64 * 4 ? 4 : n <= 64 * 8 ? 8 : n <= 64 * 16 ? 16 : 32;
    if (sizeof(float) * (size_t)(64 * P) * d <= 64 * 1024) return 0;
  }
  return (int64_t)n * d >= jb::kpw::kPaysFloats ? 1 : 0;
}

extern "C" int jb_kmeanspp_wide(const float* X, int n, int d, const float* w, const double* u, int m, int32_t* out,
                                int32_t* status, int32_t* nearest, void* work, int64_t work_bytes,
                                hipStream_t stream) {
  using namespace jb::kpw;
  const Geo g = geometry(n, d, m);
  if (g.G == 0) return -2;
  if (X == nullptr || w == nullptr || u == nullptr || out == nullptr || status == nullptr || work == nullptr ||
      work_bytes < jb_kmeanspp_wide_work(n, d, m))
    return (int)hipErrorInvalidValue;
  int32_t* state = static_cast<int32_t*>(work);
  double* part = reinterpret_cast<double*>(state + kState);
  float* d2 = reinterpret_cast<float*>(part + g.G);
  hipLaunchKernelGGL(kmeanspp_wide_init_kernel, dim3(1), dim3(64), 0, stream, state, status);
  for (int64_t j = 0; j <= m; ++j)                 // (j == m: the tail)
    hipLaunchKernelGGL(kmeanspp_wide_kernel, dim3(g.G), dim3(kT), 0, stream, X, n, d, w, u, m, (int)j, g.L, out,
                       status, nearest, d2, part, state);
  return (int)hipGetLastError();
}
