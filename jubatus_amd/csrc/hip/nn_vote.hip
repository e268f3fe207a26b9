// Nearest-neighbour classifiers (NN, cosine, euclidean): the label vote behind
// the top-k (models/nn_classifier.py _score is the numerical oracle).
//
// Input: the [nq, k] lists of jb_topk (csrc/hip/topk.hip), padded with +inf /
// INT_MAX, or the output of any other top-k of the same layout (any k), and
// row_lab, the label id of every slot in HBM (-1: the row has no label). An
// entry (d, r) is kept iff d is finite (a NaN d is not), 0 <= r < nrows and
// 0 <= row_lab[r] < nlabels; an id outside [0, nlabels) never indexes out.
//   mode 0  NN, euclidean   w = exp(-alpha d)   (unshifted, as the host _score;
//                                                not nn_reduce's d_min shift)
//   mode 1  cosine          w = 1 - d           (d = 1 - cosine: the cosine
//                                                itself, negative ones included)
//   out[q, row_lab[r]] += w;  every element of out [nq, nlabels] is written,
//   0 where no neighbour votes.
//
// One wave64 per query, four per block. The wave zeroes its row of out with
// coalesced stores (element i by lane i & 63), then takes k in chunks of 64,
// lane = entry. Per chunk it loops over the distinct labels present: the
// label l of the first lane not yet done, an xor-butterfly sum of the weights
// of the lanes that carry l, and those lanes retire; at most min(64, labels)
// rounds per chunk. Lane l & 63 owns label l: it keeps the running sum of one
// label in registers over the chunks and adds it into out[q, l] when another
// label of the same lane arrives (only with more than 64 labels) and at the
// end. Every access to out[q, l] comes from that one lane, so the wave needs
// no atomics and no fence, and the order of the fp32 additions is a fixed
// function of the input: the same input gives the same bits on every run.
#include <math.h>

#include "jb_device.hpp"
#include "jb_hip_api.h"

namespace jb {

constexpr int kNnVoteThreads = 256;

template <int MODE>
__global__ __launch_bounds__(kNnVoteThreads) void nn_vote_kernel(
    const float* __restrict__ dist, const int32_t* __restrict__ row, int nq, int k,
    const int32_t* __restrict__ row_lab, int nrows, int nlabels, float alpha, float* out) {
  const int lane = threadIdx.x & 63;
  const int q = (int)(((int64_t)blockIdx.x * kNnVoteThreads + threadIdx.x) >> 6);
  if (q >= nq) return;                                     // wave-uniform
  const float* d = dist + (int64_t)q * k;
  const int32_t* r = row + (int64_t)q * k;
  float* o = out + (int64_t)q * nlabels;
  for (int i = lane; i < nlabels; i += 64) o[i] = 0.f;
  int held = -1;                                           // the label this lane sums, if any
  float acc = 0.f;
  for (int c0 = 0; c0 < k; c0 += 64) {
    const int j = c0 + lane;
    int lab = -1;
    float w = 0.f;
    if (j < k) {
      const float dj = d[j];
      const int32_t rj = r[j];
      if (fabsf(dj) < INFINITY && rj >= 0 && rj < nrows) {  // a NaN d compares false
        const int32_t lj = row_lab[rj];
        if (lj >= 0 && lj < nlabels) {
          lab = lj;
          w = MODE == 0 ? expf(-alpha * dj) : 1.f - dj;
        }
      }
    }
    unsigned long long todo = __ballot(lab >= 0);
    while (todo) {                                         // wave-uniform
      const int l = __shfl(lab, __ffsll(todo) - 1, 64);
      const bool mine = lab == l;
      const float s = wave_sum_fast(mine ? w : 0.f, lane);
      if (lane == (l & 63)) {
        if (held != l) {
          if (held >= 0) o[held] += acc;
          held = l;
          acc = 0.f;
        }
        acc += s;
      }
      todo &= ~__ballot(mine);
    }
  }
  if (held >= 0) o[held] += acc;
}

}  // namespace jb

// 0: done (nothing to do when nq <= 0); -2: an argument out of range
// (jb_nn_reduce's convention); otherwise the HIP error of the launch.
extern "C" int jb_nn_vote(const float* dist, const int32_t* row, int nq, int k,
                          const int32_t* row_lab, int nrows, int nlabels, int mode, float alpha,
                          float* out, hipStream_t stream) {
  if (nq <= 0) return 0;
  if (k < 0 || nrows < 0 || nlabels <= 0 || mode < 0 || mode > 1 || !(alpha >= 0.f) ||
      !(alpha < INFINITY))
    return -2;
  if (out == nullptr) return -2;
  if (k > 0 && (dist == nullptr || row == nullptr)) return -2;
  if (k > 0 && nrows > 0 && row_lab == nullptr) return -2;
  const int waves = jb::kNnVoteThreads / 64;
  const int blocks = (int)(((int64_t)nq + waves - 1) / waves);
  const dim3 g(blocks), b(jb::kNnVoteThreads);
  if (mode == 0)
    hipLaunchKernelGGL(jb::nn_vote_kernel<0>, g, b, 0, stream, dist, row, nq, k, row_lab, nrows,
                       nlabels, alpha, out);
  else
    hipLaunchKernelGGL(jb::nn_vote_kernel<1>, g, b, 0, stream, dist, row, nq, k, row_lab, nrows,
                       nlabels, alpha, out);
  return (int)hipGetLastError();
}
