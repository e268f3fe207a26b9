// Weighted Lloyd (k-means) on the whole GPU, for k x dims past the LDS of the
// one-workgroup lloyd_kernel (clustering.hip). Same rule as that kernel and
// models/clustering.py _recluster:
//   a_i  = argmin_j |x_i - c_j|^2, the first index on ties
//   C'_j = sum_{a_i = j} w_i x_i / max(sum_{a_i = j} w_i, 1e-12); a centre whose
//          weight sum is not > 0 keeps its value
//   stop after the first iteration with |C' - C| <= atol + rtol |C| in every
//   element (torch.allclose) or after `iters`, then one assignment pass under
//   the returned C. iters == 0 only assigns.
//
// One iteration is two launches on the caller's stream, no grid-wide barrier
// and no float atomics:
//   kmeans_wide_step_kernel    G workgroups; each walks slabs g, g + G, ... of
//                              SP points: scores, row arg-min, one-hot update
//                              sums into the workgroup's own partial [k d + k]
//   kmeans_wide_reduce_kernel  one workgroup per centre, a thread per (j, q):
//                              the G partials summed in workgroup order, the
//                              empty-centre rule, the allclose test, C and
//                              |c_j|^2 for the next scores
// and a last ASSIGN pass of the step kernel writes the assignment. G and every
// summation order are fixed functions of (n, k, d): two runs on the same
// inputs return the same bits.
//
// Scores: s_ij = |c_j|^2 - 2 x_i . c_j (|x_i|^2 is constant in a row), the form
// sqdist_mfma_kernel and the host loops use at these shapes. The Gram term
// runs on v_mfma_f32_16x16x4_f32 (fragment maps at the top of clustering.hip).
// X moves through LDS in chunks of kDC dims; the C fragments stream from
// global memory (every workgroup reads the same table, so it stays in L2).
// The four k-slots of a step need not be adjacent dims, only the same dims in
// A and B: lane group l >> 4 takes dims 4 (l >> 4) .. + 3 of a 16-dim block,
// one float4 from LDS and one from C for four steps. A wave owns the centre
// tiles wave, wave + 4, ... for all the slab's points, so a C fragment is
// loaded once a workgroup and the accumulators (at most 16 tiles) stay in
// registers over all dim chunks. The tile lands in the LDS table sR [SP][KP],
// padding columns at +inf.
//
// Row arg-min: one wave a row, min and lowest index by DPP / permlane. The
// wave then overwrites its row with w_i at the winner and 0 elsewhere, and
// S = R^T X, nk = R^T 1 run on the MFMA into the workgroup's own partial, as
// in jb_slab.hpp (update_sums without the squares). The one-hot GEMM does k
// times the additions of a scatter; it costs what the scores cost, needs no
// atomics and fixes the order.
//
// Convergence: the workspace holds {stopped, iterations, changed, ticket}.
// Reduce blocks that see a change atomicOr `changed` (an integer atomic,
// order-free); the last block to finish counts the iteration and sets
// `stopped` when nothing changed. Every kernel of a later iteration reads
// `stopped` first and returns. done_iters is that count: the update iterations
// run, the converging one included (lloyd_kernel leaves `iters` in its word
// whether or not it stopped early; the two agree when it did not). jb_lloyd_wide enqueues iterations in groups of
// kGroup and reads the first two words between groups: THIS ENTRY
// SYNCHRONISES THE STREAM (once per group that is not the last).
#include <stdlib.h>

#include "jb_hip_api.h"
#include "jb_slab.hpp"

namespace jb {
namespace kw {

using namespace jb::slab;   // kT, kDC, Geo, block_sum, stage_x, update_sums: as in jb_slab.hpp

constexpr int kGroup = 8;            // iterations enqueued between two reads of the state
constexpr int kState = 4;            // int32 words: stopped, iterations, changed, ticket

// one partial: S [k d] | nk [k]; the fixed part of the workspace: the state | |c_j|^2 [k]
__host__ inline Geo geometry(int64_t n, int64_t d, int64_t k) {
  return jb::slab::geometry(n, d, k, k * d + k, kState + k);
}

// |c_j|^2 of the block's centre, the same order wherever it is computed
__device__ __forceinline__ float row_norm2(const float* __restrict__ cj, int d, float* red) {
  float s = 0.f;
  for (int q = threadIdx.x; q < d; q += kT) s = fmaf(cj[q], cj[q], s);
  return block_sum(s, red);
}

// the smaller of two (value, index) pairs, the lower index on equal values
__device__ __forceinline__ void take_min(float& bv, int& bj, float ov, int oj) {
  if (ov < bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
}

// the wave's minimum and its lowest index in every lane, no LDS
__device__ __forceinline__ void wave_argmin(float& bv, int& bj, int lane) {
  take_min(bv, bj, dpp_f<kDppXor1>(bv), dpp_i<kDppXor1>(bj));
  take_min(bv, bj, dpp_f<kDppXor2>(bv), dpp_i<kDppXor2>(bj));
  take_min(bv, bj, dpp_f<kDppHalfMirror>(bv), dpp_i<kDppHalfMirror>(bj));
  take_min(bv, bj, dpp_f<kDppMirror>(bv), dpp_i<kDppMirror>(bj));
  take_min(bv, bj, partner16_f(bv, lane), partner16_i(bj, lane));
  take_min(bv, bj, partner32_f(bv, lane), partner32_i(bj, lane));
}

// C[j][q .. q + 3], zeros past k and past d; vec: rows of C are float4-aligned
__device__ __forceinline__ float4 load_c4(const float* __restrict__ C, int j, int q, int k, int d, bool vec) {
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (j >= k || q >= d) return v;
  const float* p = C + (int64_t)j * d + q;
  if (vec) return *reinterpret_cast<const float4*>(p);   // (d % 4 == 0 and q % 4 == 0: q + 3 < d)
  v.x = p[0];
  if (q + 1 < d) v.y = p[1];
  if (q + 2 < d) v.z = p[2];
  if (q + 3 < d) v.w = p[3];
  return v;
}

// before the first iteration: |c_j|^2 of the caller's centres and a clear state
__global__ __launch_bounds__(kT) void kmeans_wide_init_kernel(const float* __restrict__ C, int d,
                                                              float* __restrict__ CN2, int32_t* state) {
  __shared__ float red[4];
  const int j = blockIdx.x;
  const float c2 = row_norm2(C + (int64_t)j * d, d, red);
  if (threadIdx.x == 0) CN2[j] = c2;
  if (j == 0 && threadIdx.x < kState) state[threadIdx.x] = 0;
}

// RT: 16-point row tiles of a slab (SP = 16 RT); JW: the centre tiles a wave
// may own (KP / 16 / 4 rounded up, at the largest KP of that slab size).
// ASSIGN: scores and arg-min only, every point's centre written out.
template <int RT, int JW, bool ASSIGN>
__global__ __launch_bounds__(kT) void kmeans_wide_step_kernel(const float* __restrict__ X, int n, int d,
                                                              const float* __restrict__ w,
                                                              const float* __restrict__ C,
                                                              const float* __restrict__ CN2, int k, Geo g,
                                                              const int32_t* state, float* __restrict__ part,
                                                              int32_t* __restrict__ assign,
                                                              int32_t* __restrict__ done_iters) {
  if (!ASSIGN && state[0]) return;                 // converged in an earlier iteration
  extern __shared__ float s_kw[];
  constexpr int SP = 16 * RT;
  const int RS = g.RS, KP = g.KP;
  float* sR = s_kw;                                // [SP][RS]
  float* sX = sR + (size_t)SP * RS;                // [SP][kXS]
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int ar = lane & 15, kq = lane >> 4;
  const bool vec = (d & 3) == 0 && (reinterpret_cast<uintptr_t>(C) & 15) == 0;
  if (ASSIGN && blockIdx.x == 0 && t == 0 && done_iters != nullptr) *done_iters = state[1];
  float* P1 = part + (int64_t)blockIdx.x * g.PS;
  float* Pn = P1 + (int64_t)k * d;
  const int64_t slabs = ((int64_t)n + SP - 1) / SP;
  bool first = true;
  for (int64_t s = blockIdx.x; s < slabs; s += gridDim.x) {
    const int64_t row0 = s * SP;
    // scores: acc[jw][it] = X tile it . C tile (wv + 4 jw), a chunk of dims at a time
    f32x4 acc[JW][RT];
#pragma unroll
    for (int jw = 0; jw < JW; ++jw)
#pragma unroll
      for (int it = 0; it < RT; ++it) acc[jw][it] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q0 = 0; q0 < d; q0 += kDC) {
      __syncthreads();                             // the tile's last readers are done
      stage_x(sX, X, n, d, row0, q0, SP);
      __syncthreads();
#pragma unroll
      for (int h = 0; h < kDC / 16; ++h) {
        if (q0 + 16 * h >= d) break;               // (block-uniform)
        const int qb = q0 + 16 * h + 4 * kq;
        float4 a[RT];
#pragma unroll
        for (int it = 0; it < RT; ++it)
          a[it] = *reinterpret_cast<const float4*>(sX + (it * 16 + ar) * kXS + 16 * h + 4 * kq);
#pragma unroll
        for (int jw = 0; jw < JW; ++jw) {
          const int j0 = (wv + 4 * jw) * 16;
          if (j0 < KP) {                           // (wave-uniform)
            const float4 b = load_c4(C, j0 + ar, qb, k, d, vec);
#pragma unroll
            for (int it = 0; it < RT; ++it) {
              acc[jw][it] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[it].x, b.x, acc[jw][it], 0, 0, 0);
              acc[jw][it] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[it].y, b.y, acc[jw][it], 0, 0, 0);
              acc[jw][it] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[it].z, b.z, acc[jw][it], 0, 0, 0);
              acc[jw][it] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[it].w, b.w, acc[jw][it], 0, 0, 0);
            }
          }
        }
      }
    }
    // (sR's last readers, the previous slab's update, passed the barriers above)
#pragma unroll
    for (int jw = 0; jw < JW; ++jw) {
      const int j = (wv + 4 * jw) * 16 + ar;
      if (j < KP) {
        const float cn = j < k ? CN2[j] : 0.f;
#pragma unroll
        for (int it = 0; it < RT; ++it)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            sR[(it * 16 + kq * 4 + r) * RS + j] = j < k ? fmaf(-2.f, acc[jw][it][r], cn) : INFINITY;
      }
    }
    __syncthreads();
    // rows: one wave a row, lanes over the centres
    for (int i = wv; i < SP; i += kT / 64) {
      float* r = sR + i * RS;
      const int64_t gi = row0 + i;
      if (gi >= n) {                               // (wave-uniform) a row past the end weighs nothing
        if (!ASSIGN)
          for (int j = lane; j < KP; j += 64) r[j] = 0.f;
        continue;
      }
      float bv = INFINITY;
      int bj = INT_MAX;
      for (int j = lane; j < KP; j += 64) {
        const float v = r[j];
        if (v < bv) { bv = v; bj = j; }
      }
      wave_argmin(bv, bj, lane);
      if (bj == INT_MAX) bj = 0;                   // no finite score: lloyd_kernel's default
      if (ASSIGN) {
        if (lane == 0) assign[gi] = bj;
        continue;
      }
      const float wi = w[gi];
      for (int j = lane; j < KP; j += 64) r[j] = j == bj ? wi : 0.f;
    }
    if (ASSIGN) continue;
    // update sums of the slab on the matrix cores: A = R^T from sR, B = the X tile
    update_sums<false, 4>(sR, sX, X, n, d, k, row0, SP, RS, KP, P1, nullptr, Pn, first, wv, lane);
    first = false;
  }
}

// one workgroup per centre j, a thread per (j, q): the partials in workgroup
// order, the empty-centre rule, the allclose test against the old C, the new
// C and its |c_j|^2; the last block to finish closes the iteration
__global__ __launch_bounds__(kT) void kmeans_wide_reduce_kernel(const float* __restrict__ part, int G, int64_t PS,
                                                                int k, int d, float atol, float rtol,
                                                                float* __restrict__ C, float* __restrict__ CN2,
                                                                int32_t* state) {
  __shared__ float red[4];
  if (state[0]) return;
  const int j = blockIdx.x, t = threadIdx.x;
  const int64_t kd = (int64_t)k * d;
  float m = 0.f;
#pragma unroll 8
  for (int g = 0; g < G; ++g) m += part[(int64_t)g * PS + kd + j];
  float* cj = C + (int64_t)j * d;
  int changed = 0;
  for (int q = t; q < d; q += kT) {
    const float* p = part + (int64_t)j * d + q;
    float s = 0.f;
#pragma unroll 8
    for (int g = 0; g < G; ++g) s += p[(int64_t)g * PS];
    const float old = cj[q];
    const float nc = m > 0.f ? s / fmaxf(m, 1e-12f) : old;
    if (fabsf(nc - old) > atol + rtol * fabsf(old)) changed = 1;
    cj[q] = nc;
  }
  __syncthreads();                                 // the block's C row is written
  const float c2 = row_norm2(cj, d, red);
  if (t == 0) CN2[j] = c2;
  const int any = __syncthreads_or(changed);
  if (t == 0) {
    if (any) atomicOr(&state[2], 1);
    __threadfence();
    if (atomicAdd(&state[3], 1) == (int)gridDim.x - 1) {   // every other block has taken its ticket
      const int ch = atomicOr(&state[2], 0);
      state[1] += 1;
      if (!ch) state[0] = 1;
      state[2] = 0;
      state[3] = 0;
    }
  }
}

template <bool ASSIGN>
__host__ inline void launch_step(const Geo& g, size_t lds, hipStream_t stream, const float* X, int n, int d,
                                 const float* w, const float* C, const float* CN2, int k, const int32_t* state,
                                 float* part, int32_t* assign, int32_t* done_iters) {
#define JB_KW_STEP(RT, JW)                                                                                       \
  hipLaunchKernelGGL((kmeans_wide_step_kernel<RT, JW, ASSIGN>), dim3(g.G), dim3(kT), lds, stream, X, n, d, w, C, \
                     CN2, k, g, state, part, assign, done_iters)
  if (g.SP == 64) JB_KW_STEP(4, 2);
  else if (g.SP == 32) JB_KW_STEP(2, 6);
  else JB_KW_STEP(1, 16);
#undef JB_KW_STEP
}

}  // namespace kw
}  // namespace jb

extern "C" int64_t jb_lloyd_wide_work(int n, int d, int k) {
  const jb::kw::Geo g = jb::kw::geometry(n, d, k);
  if (g.G == 0) return 0;
  return 4 * (jb::kw::kState + (int64_t)k + g.G * g.PS);
}

extern "C" int jb_lloyd_wide(const float* X, int n, int d, const float* w, float* C, int k, int iters, float atol,
                             float rtol, int32_t* assign, int32_t* done_iters, void* work, int64_t work_bytes,
                             hipStream_t stream) {
  using namespace jb::kw;
  const Geo g = geometry(n, d, k);
  if (g.G == 0) return -2;
  if (work == nullptr || work_bytes < jb_lloyd_wide_work(n, d, k) || assign == nullptr || iters < 0)
    return (int)hipErrorInvalidValue;
  int32_t* state = static_cast<int32_t*>(work);
  float* CN2 = reinterpret_cast<float*>(state + kState);
  float* part = CN2 + k;
  const size_t lds = lds_bytes(g);
  if (lds > 64 * 1024) {                           // (only the 16-point slabs get there)
    const hipError_t attr =
        allow_large_lds<kmeans_wide_step_kernel<1, 16, false>, kmeans_wide_step_kernel<1, 16, true>>();
    if (attr != hipSuccess) return (int)attr;
  }
  hipLaunchKernelGGL(kmeans_wide_init_kernel, dim3(k), dim3(kT), 0, stream, C, d, CN2, state);
  for (int it = 0; it < iters;) {
    for (int e = it + kGroup < iters ? it + kGroup : iters; it < e; ++it) {
      launch_step<false>(g, lds, stream, X, n, d, w, C, CN2, k, state, part, nullptr, nullptr);
      hipLaunchKernelGGL(kmeans_wide_reduce_kernel, dim3(k), dim3(kT), 0, stream, part, g.G, g.PS, k, d, atol, rtol,
                         C, CN2, state);
    }
    if (it == iters) break;                        // nothing left to enqueue either way
    int32_t st[2] = {0, 0};                        // stopped, iterations
    hipError_t e = hipMemcpyAsync(st, state, sizeof(st), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return (int)e;
    if (st[0]) break;
  }
  launch_step<true>(g, lds, stream, X, n, d, w, C, CN2, k, state, part, assign, done_iters);
  return (int)hipGetLastError();
}
