// Nearest-neighbour regression: the reduction of the neighbours' targets
// behind the top-k (models/nn_regression.py is the numerical oracle).
//
// The reference (Jubatus 0.9.2) ships PA regression only; the NN / cosine /
// euclidean regression methods are this project's own definition, and parity
// with later Jubatus releases is unpinned.
//
// Input: the [nq, k] lists of jb_topk (csrc/hip/topk.hip), padded with +inf /
// INT_MAX, or the output of any other top-k of the same layout (any k), and
// the per-slot targets in HBM. Per query, over the entries that are kept (d
// finite and 0 <= row < nrows):
//   mode 0  uniform    w = 1
//   mode 1  distance   w = exp(-alpha (d - d_min)),  d_min the smallest kept d:
//                      the nearest row weighs 1, so no alpha underflows them all
//   mode 2  similarity w = max(0, 1 - d)             (d = 1 - cosine)
//   out = sum w t / sum w   (0 when nothing is kept or sum w == 0)
//   out_n = number of kept entries
//
// One wave64 per query, four per block; lanes stride over k. Every lane sums
// its entries in index order in fp32 and the lanes are combined by the xor
// butterfly of wave_sum, so the order is fixed and the same input gives the
// same bits on every run. No atomics, no LDS.
#include <math.h>

#include "jb_device.hpp"
#include "jb_hip_api.h"

namespace jb {

constexpr int kNnReduceThreads = 256;

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ bool nn_kept(float d, int32_t r, int nrows) {
  return fabsf(d) < INFINITY && r >= 0 && r < nrows;      // a NaN d compares false
}

template <int MODE>
__global__ __launch_bounds__(kNnReduceThreads) void nn_reduce_kernel(
    const float* __restrict__ dist, const int32_t* __restrict__ row, int nq, int k,
    const float* __restrict__ targets, int nrows, float alpha, float* __restrict__ out,
    int32_t* __restrict__ out_n) {
  const int lane = threadIdx.x & 63;
  const int q = (int)(((int64_t)blockIdx.x * kNnReduceThreads + threadIdx.x) >> 6);
  if (q >= nq) return;                                     // wave-uniform
  const float* d = dist + (int64_t)q * k;
  const int32_t* r = row + (int64_t)q * k;
  float dmin = INFINITY;
  if (MODE == 1) {
    for (int j = lane; j < k; j += 64) {
      const float dj = d[j];
      if (nn_kept(dj, r[j], nrows)) dmin = fminf(dmin, dj);
    }
    dmin = wave_min(dmin);
  }
  float sw = 0.f, swt = 0.f;
  int n = 0;
  for (int j = lane; j < k; j += 64) {
    const float dj = d[j];
    const int32_t rj = r[j];
    if (!nn_kept(dj, rj, nrows)) continue;
    float w = 1.f;
    if (MODE == 1) w = expf(-alpha * (dj - dmin));
    if (MODE == 2) w = fmaxf(0.f, 1.f - dj);
    sw += w;
    swt += w * targets[rj];
    ++n;
  }
  sw = wave_sum(sw);
  swt = wave_sum(swt);
  n = wave_sum_i(n);
  if (lane == 0) {
    out[q] = sw > 0.f ? swt / sw : 0.f;
    out_n[q] = n;
  }
}

}  // namespace jb

// 0: done (nothing to do when nq <= 0); -2: an argument out of range (jb_topk's
// convention); otherwise the HIP error of the launch.
extern "C" int jb_nn_reduce(const float* dist, const int32_t* row, int nq, int k,
                            const float* targets, int nrows, int mode, float alpha,
                            float* out, int32_t* out_n, hipStream_t stream) {
  if (nq <= 0) return 0;
  if (k < 0 || nrows < 0 || mode < 0 || mode > 2 || !(alpha >= 0.f) || !(alpha < INFINITY))
    return -2;
  if (out == nullptr || out_n == nullptr) return -2;
  if (k > 0 && (dist == nullptr || row == nullptr)) return -2;
  if (k > 0 && nrows > 0 && targets == nullptr) return -2;
  const int waves = jb::kNnReduceThreads / 64;
  const int blocks = (int)(((int64_t)nq + waves - 1) / waves);
  const dim3 g(blocks), b(jb::kNnReduceThreads);
  if (mode == 0)
    hipLaunchKernelGGL(jb::nn_reduce_kernel<0>, g, b, 0, stream, dist, row, nq, k, targets, nrows,
                       alpha, out, out_n);
  else if (mode == 1)
    hipLaunchKernelGGL(jb::nn_reduce_kernel<1>, g, b, 0, stream, dist, row, nq, k, targets, nrows,
                       alpha, out, out_n);
  else
    hipLaunchKernelGGL(jb::nn_reduce_kernel<2>, g, b, 0, stream, dist, row, nq, k, targets, nrows,
                       alpha, out, out_n);
  return (int)hipGetLastError();
}
