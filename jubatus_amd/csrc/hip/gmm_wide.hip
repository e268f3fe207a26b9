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
// so they run on v_mfma_f32_16x16x4_f32 (fragment maps at the top of
// clustering.hip): A = R^T from sR, lane l holds R[i0 + (l >> 4)][j0 + (l & 15)];
// B = the X tile, lane l holds X[i0 + (l >> 4)][q0 + (l & 15)], its square for
// S2 and a column of ones for nk; a step covers 4 points. A wave owns the
// (16 components x 16 dims) tiles wave, wave + 4, ... of a chunk, and the lane
// that holds an output element is the only writer of that element of the
// workgroup's partial: a plain store for the first slab, read-add-write after
// it. No float atomics.
#include <stdlib.h>

#include "jb_device.hpp"
#include "jb_hip_api.h"

namespace jb {
namespace gw {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kT = 256;              // threads of every kernel here
constexpr int kDC = 32;              // dims per X chunk in LDS
constexpr int kXS = 48;              // row stride of the X tile: rows i .. i + 3 on distinct banks
constexpr int kMaxK = 1024;
constexpr int64_t kMaxKD = (int64_t)1 << 22;
constexpr int64_t kWorkCap = (int64_t)256 << 20;
constexpr int kMaxGrid = 256;        // one workgroup a CU

struct Geo {
  int KP;        // k padded to the 16-component tile
  int SP;        // points a slab
  int RS;        // row stride of sR
  int JT;        // E-step: threads along the components (a power of two), kT / JT point groups
  int G;         // workgroups of the em kernel
  int64_t PS;    // floats of one partial: S1 [k d] | S2 [k d] | nk [k]
};

// 0 in G: outside the supported range
__host__ inline Geo geometry(int64_t n, int64_t d, int64_t k) {
  Geo g = {};
  if (n < 1 || n > INT32_MAX || d < 1 || k < 1 || k > kMaxK || k * d > kMaxKD) return g;
  g.KP = (int)((k + 15) / 16 * 16);
  g.SP = g.KP <= 128 ? 64 : g.KP <= 384 ? 32 : 16;
  g.RS = (g.KP + 47) / 64 * 64 + 16;             // RS % 64 == 16: 4 rows x 16 columns, 64 banks
  g.JT = 1;
  while (g.JT < k && g.JT < kT) g.JT <<= 1;
  g.PS = 2 * k * d + k;
  const int64_t fixed = k * d + 2 * k;            // 1 / var, lc, nk
  const int64_t room = (kWorkCap / 4 - fixed) / g.PS;
  const int64_t slabs = (n + g.SP - 1) / g.SP;
  int64_t G = slabs < kMaxGrid ? slabs : kMaxGrid;
  if (G > room) G = room;
  g.G = (int)G;
  return g;
}

__host__ inline size_t lds_bytes(const Geo& g) { return sizeof(float) * ((size_t)g.SP * g.RS + (size_t)g.SP * kXS); }

// the block's sum in a fixed order, every thread gets it (red: 4 floats)
__device__ __forceinline__ float block_sum(float v, float* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  v = wave_sum_fast(v, lane);
  __syncthreads();                   // (red may still be read from the previous call)
  if (lane == 0) red[wv] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// rows [row0, row0 + SP) x dims [q0, q0 + kDC) of X into the LDS tile, zeros
// past n and past d
__device__ __forceinline__ void stage_x(float* __restrict__ sX, const float* __restrict__ X, int n, int d,
                                        int64_t row0, int q0, int SP) {
  for (int e = threadIdx.x; e < SP * kDC; e += kT) {
    const int i = e / kDC, q = e - i * kDC;
    const int64_t gi = row0 + i;
    sX[i * kXS + q] = (gi < n && q0 + q < d) ? X[gi * d + q0 + q] : 0.f;
  }
}

// ASSIGN: the E-step only, then every point's argmax (first index on ties)
template <bool ASSIGN>
__global__ __launch_bounds__(kT) void gmm_wide_em_kernel(const float* __restrict__ X, int n, int d,
                                                         const float* __restrict__ w,
                                                         const float* __restrict__ C,
                                                         const float* __restrict__ IV,
                                                         const float* __restrict__ LC, int k, Geo g,
                                                         float* __restrict__ part,
                                                         int32_t* __restrict__ assign) {
  extern __shared__ float s_gw[];
  float* sR = s_gw;                                // [SP][RS]
  float* sX = sR + (size_t)g.SP * g.RS;            // [SP][kXS]
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int SP = g.SP, RS = g.RS, KP = g.KP;
  const int jl = t & (g.JT - 1), ig = t / g.JT, IT = kT / g.JT;
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
      for (int j = jl; j < k; j += g.JT) {
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
    const int jtiles = KP / 16;
    for (int q0 = 0; q0 < d; q0 += kDC) {
      __syncthreads();                             // sR complete / the tile's last readers are done
      stage_x(sX, X, n, d, row0, q0, SP);
      __syncthreads();
      for (int tile = wv; tile < jtiles * (kDC / 16); tile += kT / 64) {
        const int j0 = (tile / (kDC / 16)) * 16, qq0 = (tile % (kDC / 16)) * 16;
        if (q0 + qq0 >= d) continue;               // (wave-uniform)
        const bool with_nk = q0 + qq0 == 0;
        f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f}, a0 = {0.f, 0.f, 0.f, 0.f};
        const float* ra = sR + (lane >> 4) * RS + j0 + (lane & 15);
        const float* xb = sX + (lane >> 4) * kXS + qq0 + (lane & 15);
        for (int i0 = 0; i0 < SP; i0 += 4) {
          const float a = ra[i0 * RS];
          const float b = xb[i0 * kXS];
          a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, a1, 0, 0, 0);
          a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b * b, a2, 0, 0, 0);
          if (with_nk) a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.f, a0, 0, 0, 0);
        }
        const int q = q0 + qq0 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = j0 + (lane >> 4) * 4 + r;
          if (j >= k) continue;
          if (q < d) {
            const int64_t e = (int64_t)j * d + q;
            P1[e] = first ? a1[r] : P1[e] + a1[r];
            P2[e] = first ? a2[r] : P2[e] + a2[r];
          }
          if (with_nk && (lane & 15) == 0) Pn[j] = first ? a0[r] : Pn[j] + a0[r];
        }
      }
    }
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
  if (lds > 64 * 1024) {
    static const hipError_t attr = [] {
      hipError_t e = hipFuncSetAttribute((const void*)gmm_wide_em_kernel<false>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)gmm_wide_em_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024);
      return e;
    }();
    if (attr != hipSuccess) return (int)attr;
  }
  hipLaunchKernelGGL(gmm_wide_consts_kernel<false>, dim3(k), dim3(kT), 0, stream, var, k, d, NK, pi, IV, LC);
  const unsigned rgrid = (unsigned)((kd + kT - 1) / kT);
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(gmm_wide_em_kernel<false>, dim3(g.G), dim3(kT), lds, stream, X, n, d, w, C, IV, LC, k, g, part,
                       nullptr);
    hipLaunchKernelGGL(gmm_wide_reduce_kernel, dim3(rgrid), dim3(kT), 0, stream, part, g.G, g.PS, k, d, C, var, IV,
                       NK);
    hipLaunchKernelGGL(gmm_wide_consts_kernel<true>, dim3(k), dim3(kT), 0, stream, var, k, d, NK, pi, IV, LC);
  }
  if (assign != nullptr)
    hipLaunchKernelGGL(gmm_wide_em_kernel<true>, dim3(g.G), dim3(kT), lds, stream, X, n, d, w, C, IV, LC, k, g, part,
                       assign);
  return (int)hipGetLastError();
}
