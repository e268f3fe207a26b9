// Diagonal-covariance GMM EM on the whole GPU, for k x dims past the LDS of
// the one-workgroup gmm_em_kernel (clustering.hip). Same formulas as that
// kernel and models/clustering.py _em:
//   r_ij = w_i softmax_j(log pi_j - 1/2 sum_q log(2 pi var_jq)
//                        - 1/2 sum_q (x_iq - C_jq)^2 / var_jq),  pi >= 1e-12 in the log
//   nk_j = max(sum_i r_ij, 1e-9), C = S1 / nk, var = max(S2 / nk - C^2, 1e-6),
//   pi = nk / sum nk, with S1 = R^T X and S2 = R^T X^2.
// `iters` is a fixed count; assign_i is the argmax of the log posterior under
// the returned parameters.
//
// One iteration is three launches on the caller's stream, no host sync and no
// grid-wide barrier anywhere:
//   gmm_wide_em_kernel      G workgroups; each walks slabs g, g + G, ... of SP
//                           points: E-step, row softmax, M-step partial sums
//                           into the workgroup's own partial [2 k d + k]
//   gmm_wide_reduce_kernel  one thread per (j, q): the G partials summed in
//                           workgroup order, clamps, C / var / 1 / var
//   gmm_wide_consts_kernel  one workgroup per component: pi and the log
//                           constant lc_j = log pi_j - 1/2 sum_q log(2 pi var_jq)
// and a last E-only pass of the em kernel writes the assignment. G and every
// summation order are fixed functions of (n, k, d): two runs on the same
// inputs return the same bits.
//
// E-step: on the VALU in the direct form (x - c)^2 * (1 / var). It is NOT
// expanded into X^2 (1/var)^T - 2 X (C/var)^T to reach the matrix cores: at
// the 1e-6 variance floor those terms reach ~1e8 and cancel, and fp32 loses
// whole units of log-probability. X moves through LDS in chunks of kDC
// dims; C and 1 / var stream from global memory (every workgroup reads the
// same tables, so they stay in L2) into registers, a component per lane, and
// are reused over the slab's points. The quadratic forms accumulate in the
// LDS table sR [SP][k], which the softmax then turns into responsibilities
// in place (one wave per row, max and sum by DPP / permlane).
//
// M-step: S1, S2 and nk are true GEMMs over the points with no cancellation,
// so they run on the matrix cores into the workgroup's own partial, as in
// jb_slab.hpp (update_sums with the squares).
#include <stdlib.h>

#include "jb_hip_api.h"
#include "jb_slab.hpp"

namespace jb {
namespace gw {

using namespace jb::slab;   // kT, kDC, Geo, block_sum, stage_x, update_sums: as in jb_slab.hpp

// one partial: S1 [k d] | S2 [k d] | nk [k]; the fixed part of the workspace: 1 / var [k d] | lc [k] | nk [k]
__host__ inline Geo geometry(int64_t n, int64_t d, int64_t k) {
  return jb::slab::geometry(n, d, k, 2 * k * d + k, k * d + 2 * k);
}

// E-step: threads along the components (a power of two), kT / JT point groups
__host__ inline int estep_threads(int k) {
  int JT = 1;
  while (JT < k && JT < kT) JT <<= 1;
  return JT;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// ASSIGN: the E-step only, then every point's argmax (first index on ties)
template <bool ASSIGN>
__global__ __launch_bounds__(kT) void gmm_wide_em_kernel(const float* __restrict__ X, int n, int d,
                                                         const float* __restrict__ w,
                                                         const float* __restrict__ C,
                                                         const float* __restrict__ IV,
                                                         const float* __restrict__ LC, int k, Geo g,
                                                         int JT, float* __restrict__ part,
                                                         int32_t* __restrict__ assign) {
  extern __shared__ float s_gw[];
  float* sR = s_gw;                                // [SP][RS]
  float* sX = sR + (size_t)g.SP * g.RS;            // [SP][kXS]
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int SP = g.SP, RS = g.RS, KP = g.KP;
  const int jl = t & (JT - 1), ig = t / JT, IT = kT / JT;
  float* P1 = part + (int64_t)blockIdx.x * g.PS;
  float* P2 = P1 + (int64_t)k * d;
  float* Pn = P2 + (int64_t)k * d;
  const int64_t slabs = ((int64_t)n + SP - 1) / SP;
  bool first = true;
  for (int64_t s = blockIdx.x; s < slabs; s += gridDim.x) {
    const int64_t row0 = s * SP;
    // E-step: sR[i][j] = sum_q (x_iq - C_jq)^2 / var_jq, a chunk of dims at a time
    for (int q0 = 0; q0 < d; q0 += kDC) {
      __syncthreads();                             // the tile's last readers are done
      stage_x(sX, X, n, d, row0, q0, SP);
      __syncthreads();
      for (int j = jl; j < k; j += JT) {
        float c[kDC], iv[kDC];
        const float* cj = C + (int64_t)j * d + q0;
        const float* ivj = IV + (int64_t)j * d + q0;
#pragma unroll
        for (int q = 0; q < kDC; ++q) {
          const bool in = q0 + q < d;
          c[q] = in ? cj[q] : 0.f;
          iv[q] = in ? ivj[q] : 0.f;
        }
        for (int i = ig; i < SP; i += IT) {
          const float4* xr = reinterpret_cast<const float4*>(sX + i * kXS);
          float acc = 0.f;
#pragma unroll
          for (int q4 = 0; q4 < kDC / 4; ++q4) {
            const float4 x = xr[q4];
            const float d0 = x.x - c[4 * q4], d1 = x.y - c[4 * q4 + 1];
            const float d2 = x.z - c[4 * q4 + 2], d3 = x.w - c[4 * q4 + 3];
            acc = fmaf(d0 * d0, iv[4 * q4], acc);
            acc = fmaf(d1 * d1, iv[4 * q4 + 1], acc);
            acc = fmaf(d2 * d2, iv[4 * q4 + 2], acc);
            acc = fmaf(d3 * d3, iv[4 * q4 + 3], acc);
          }
          float* r = sR + i * RS + j;
          *r = q0 == 0 ? acc : *r + acc;
        }
      }
    }
    __syncthreads();
    // rows: one wave a row, lanes over the components
    for (int i = wv; i < SP; i += kT / 64) {
      float* r = sR + i * RS;
      const int64_t gi = row0 + i;
      if (ASSIGN) {
        if (gi >= n) continue;                     // (wave-uniform)
        float bv = -INFINITY;
        int bj = INT_MAX;
        for (int j = lane; j < k; j += 64) {
          const float v = LC[j] - 0.5f * r[j];
          if (v > bv) { bv = v; bj = j; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const float ov = __shfl_xor(bv, off, 64);
          const int oj = __shfl_xor(bj, off, 64);
          if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
        }
        if (lane == 0) assign[gi] = bj == INT_MAX ? 0 : bj;
        continue;
      }
      if (gi >= n) {                               // a row past the end weighs nothing
        for (int j = lane; j < KP; j += 64) r[j] = 0.f;
        continue;
      }
      float mx = -INFINITY;
      for (int j = lane; j < k; j += 64) {
        const float v = LC[j] - 0.5f * r[j];
        r[j] = v;
        mx = fmaxf(mx, v);
      }
      mx = wave_max(mx);
      float den = 0.f;
      for (int j = lane; j < k; j += 64) {
        const float e = expf(r[j] - mx);
        r[j] = e;
        den += e;
      }
      den = wave_sum_fast(den, lane);
      const float wi = w[gi] / den;
      for (int j = lane; j < KP; j += 64) r[j] = j < k ? wi * r[j] : 0.f;
    }
    if (ASSIGN) continue;
    // M-step partial sums of the slab on the matrix cores
    update_sums<true, 0>(sR, sX, X, n, d, k, row0, SP, RS, KP, P1, P2, Pn, first, wv, lane);
    first = false;
  }
}

// one thread per (j, q): the partials in workgroup order, the clamps, C, var
// and the next E-step's 1 / var; q == 0 also leaves nk_j for the consts kernel
__global__ __launch_bounds__(kT) void gmm_wide_reduce_kernel(const float* __restrict__ part, int G, int64_t PS,
                                                             int k, int d, float* __restrict__ C,
                                                             float* __restrict__ var, float* __restrict__ IV,
                                                             float* __restrict__ NK) {
  const int64_t e = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int64_t kd = (int64_t)k * d;
  if (e >= kd) return;
  const int j = (int)(e / d);
  float s1 = 0.f, s2 = 0.f, m = 0.f;
  for (int g = 0; g < G; ++g) {
    const float* p = part + (int64_t)g * PS;
    s1 += p[e];
    s2 += p[kd + e];
    m += p[2 * kd + j];
  }
  m = fmaxf(m, 1e-9f);
  const float c = s1 / m;
  const float v = fmaxf(s2 / m - c * c, 1e-6f);
  C[e] = c;
  var[e] = v;
  IV[e] = 1.f / v;
  if (e - (int64_t)j * d == 0) NK[j] = m;
}

// one workgroup per component j: lc_j from var and pi. FROM_NK: pi_j = nk_j /
// sum nk first (after an M-step); otherwise pi is the caller's, and 1 / var
// is written here too (before the first E-step).
template <bool FROM_NK>
__global__ __launch_bounds__(kT) void gmm_wide_consts_kernel(const float* __restrict__ var, int k, int d,
                                                             const float* __restrict__ NK, float* __restrict__ pi,
                                                             float* __restrict__ IV, float* __restrict__ LC) {
  __shared__ float red[4];
  const int j = blockIdx.x, t = threadIdx.x;
  float pj;
  if (FROM_NK) {
    float s = 0.f;
    for (int jj = t; jj < k; jj += kT) s += NK[jj];
    pj = NK[j] / block_sum(s, red);
  } else {
    pj = pi[j];
  }
  float ld = 0.f;
  for (int q = t; q < d; q += kT) {
    const float v = var[(int64_t)j * d + q];
    ld += logf(6.283185307179586f * v);
    if (!FROM_NK) IV[(int64_t)j * d + q] = 1.f / v;
  }
  ld = block_sum(ld, red);
  if (t == 0) {
    if (FROM_NK) pi[j] = pj;
    LC[j] = logf(fmaxf(pj, 1e-12f)) - 0.5f * ld;
  }
}

}  // namespace gw
}  // namespace jb

extern "C" int64_t jb_gmm_em_wide_work(int n, int d, int k) {
  const jb::gw::Geo g = jb::gw::geometry(n, d, k);
  if (g.G == 0) return 0;
  return 4 * ((int64_t)k * d + 2 * (int64_t)k + g.G * g.PS);
}

extern "C" int jb_gmm_em_wide(const float* X, int n, int d, const float* w, float* C, float* var, float* pi, int k,
                              int iters, int32_t* assign, void* work, int64_t work_bytes, hipStream_t stream) {
  using namespace jb::gw;
  const Geo g = geometry(n, d, k);
  if (g.G == 0) return -2;
  if (work == nullptr || work_bytes < jb_gmm_em_wide_work(n, d, k)) return (int)hipErrorInvalidValue;
  const int64_t kd = (int64_t)k * d;
  float* IV = static_cast<float*>(work);
  float* LC = IV + kd;
  float* NK = LC + k;
  float* part = NK + k;
  const size_t lds = lds_bytes(g);
  const int JT = estep_threads(k);
  if (lds > 64 * 1024) {
    const hipError_t attr = allow_large_lds<gmm_wide_em_kernel<false>, gmm_wide_em_kernel<true>>();
    if (attr != hipSuccess) return (int)attr;
  }
  hipLaunchKernelGGL(gmm_wide_consts_kernel<false>, dim3(k), dim3(kT), 0, stream, var, k, d, NK, pi, IV, LC);
  const unsigned rgrid = (unsigned)((kd + kT - 1) / kT);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(gmm_wide_em_kernel<false>, dim3(g.G), dim3(kT), lds, stream, X, n, d, w, C, IV, LC, k, g, JT,
                       part, nullptr);
    hipLaunchKernelGGL(gmm_wide_reduce_kernel, dim3(rgrid), dim3(kT), 0, stream, part, g.G, g.PS, k, d, C, var, IV,
                       NK);
    hipLaunchKernelGGL(gmm_wide_consts_kernel<true>, dim3(k), dim3(kT), 0, stream, var, k, d, NK, pi, IV, LC);
  }
  if (assign != nullptr)
    hipLaunchKernelGGL(gmm_wide_em_kernel<true>, dim3(g.G), dim3(kT), lds, stream, X, n, d, w, C, IV, LC, k, g, JT,
                       part, assign);
  return (int)hipGetLastError();
}
