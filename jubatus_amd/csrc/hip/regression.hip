// Online regression on a hashed weight vector in HBM: passive-aggressive
// (PA, the reference's only method) and, with rules defined by this project,
// PA1, PA2, perceptron, CW, AROW and NHERD.
//
// Reference: the regression engine's train/estimate loops,
// jubatus/server/server/regression_serv.cpp:123-149, over jubatus_core's PA
// regression (EXTERNAL). Rule (numerical oracle: models/regression.py):
//   running mean / variance of the targets (count, sum, sum of squares)
//   err = y - w.x,  loss = |err| - sensitivity * stddev
//   loss > 0:  w += sign(err) * min(C, loss) / ||x||^2 * x
// Slots with idx < 0 (unmatched converter rules) are skipped. An index that
// occurs several times in one sample (a repeated key, a hash collision)
// counts once per occurrence in w.x, in ||x||^2 and in the update: every
// increment lands, in both modes (tests/test_gpu_regression.py).
//
// The other six methods are the classifier's
// formulas (models/linear_oracle.py) with one label, no rival label and
// 1 - margin replaced by loss. The reference (Jubatus 0.9.2) ships PA
// regression only, so these rules are this project's own, their oracle is
// models/regression.py, and parity with later Jubatus releases is unpinned.
// With S = 1/P (P: diagonal precision, initial value 1), v = sum x^2 S:
//   PA1         tau = min(C, loss / ||x||^2)          w += sgn tau x
//   PA2         tau = loss / (||x||^2 + 1/(2C))
//   perceptron  tau = learning rate
//   AROW        beta = 1 / (v + 1/C), alpha = loss beta
//               w += sgn alpha S x,  P += beta x^2 / (1 - beta S x^2)
//   NHERD       alpha = loss / (v + 1/C), beta = (C^2 v + 2C) / (1 + C v)^2
//   CW          m = -loss, phi = C, b = 1 + 2 phi m,
//               gamma = (-b + sqrt(max(0, b^2 - 8 phi (m - phi v)))) / (4 phi v) > 0
//               w += sgn gamma S x,  P += 2 gamma phi x^2
// all but CW when loss > 0 and ||x||^2 > 0; CW when v > 0 and gamma > 0.
// Every occurrence's increment, on w and on P, is computed from the P the
// sample found (gather, compute, scatter).
//
// One wave64 per update stream (see linear.hip for the stream model); the
// lanes own features. The w update is a float atomic add in both modes, so
// lanes that hold the same index cannot lose each other's increment. Exact
// mode (one stream): the adds are drained before the next sample reads w,
// which therefore sees its predecessor's w, and the target statistics are
// carried in registers. Concurrent streams: no drain, and atomics for the statistics
// deltas. A concurrent wave reads the global statistics ONCE, when it
// starts, while waves that finished earlier may already have added their
// deltas: with sensitivity > 0 the stddev a stream sees, and so its updates,
// depend on launch timing (sensitivity == 0 is deterministic up to the order
// of the float adds). That is the "atomic" mode of a batch of requests, the
// default; the "exact" mode, whose result is the requests applied one after
// the other, is regression_ordered.hip (jb_regression_train_ordered).
//
// Known limit: the statistics are fp32 sums, and sum2/count - mean^2 cancels;
// the stddev is lost once |mean| / stddev reaches a few thousand.
#include "jb_hip_api.h"
#include "jb_linear.hpp"
#include "jb_regression.hpp"

namespace jb {

// One stream's samples in order, every one by regression_sample
// (jb_regression.hpp). PA keeps one chunk of 64 slots in registers and reads
// the slots past it again in the scatter (the reference's method, mostly narrow
// samples); the other methods keep kRegChunks. A confidence-method sample
// wider than the register slots without slot_scratch is a caller error: the
// stream stops there and its statistics become NaN (nothing is written
// through the null pointer).
template <int M, bool CONC>
__global__ __launch_bounds__(256) void regression_train_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ fidx,
    const float* __restrict__ fval, const float* __restrict__ targets,
    const int64_t* __restrict__ stream_ptr, int nstreams, float* W, float* P, float* stats,
    float* slot_scratch, float C, float eps) {
  constexpr int RC = M == PA ? 1 : kRegChunks;
  const int lane = threadIdx.x & 63;
  const int wid = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wid >= nstreams) return;
  // CONC: a snapshot taken at this wave's start; earlier-finishing waves of
  // the same launch may or may not be in it (timing-dependent for eps > 0)
  float sum = stats[0], sq = stats[1], cnt = stats[2];
  float dsum = 0.f, dsq = 0.f, dcnt = 0.f;
  // The loop is written with its test at the bottom. With the test at the top
  // the compiler waits there, in every turn, for the stream_ptr loads above
  // (measured on CW / AROW / NHERD), and that vector-memory wait also drains
  // the previous sample's adds in front of the row_ptr load instead of behind
  // the slot loads.
  int64_t s = stream_ptr[wid];
  const int64_t end = stream_ptr[wid + 1];
  if (s < end) do {
    const int64_t beg = row_ptr[s];
    const int n = (int)(row_ptr[s + 1] - beg);
    if (M >= CW && n > kRegSlots && slot_scratch == nullptr) {
      sum = dsum = __builtin_nanf("");
      break;
    }
    const GlobalTables<CONC> t{fidx, fval, beg, W, P, slot_scratch};
    const float y = regression_sample<M, RC, true>(t, n, targets + s, C, eps, lane, sum, sq, cnt);
    dsum += y; dsq += y * y; dcnt += 1.f;
  } while (++s < end);
  if (lane == 0) {
    if (CONC) {
      atomicAdd(stats + 0, dsum);
      atomicAdd(stats + 1, dsq);
      atomicAdd(stats + 2, dcnt);
    } else {
      stats[0] = sum; stats[1] = sq; stats[2] = cnt;
    }
  }
}

// y_hat = w.x per sample (wave per sample)
__global__ __launch_bounds__(256) void regression_estimate_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ fidx,
    const float* __restrict__ fval, int n_samples, const float* W, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int s = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (s >= n_samples) return;
  const int64_t beg = row_ptr[s];
  const int n = (int)(row_ptr[s + 1] - beg);
  float dot = 0.f;
  for (int j = lane; j < n; j += 64) {
    const int32_t idx = fidx[beg + j];
    if (idx >= 0) dot += fval[beg + j] * W[idx];
  }
  dot = wave_sum(dot);
  if (lane == 0) out[s] = dot;
}

}  // namespace jb

// the one train entry point: contract in jb_hip_api.h
extern "C" int jb_regression_train_m(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                                     const float* targets, const int64_t* stream_ptr, int nstreams,
                                     float* W, float* P, float* stats, float* slot_scratch,
                                     int method, float C, float eps, int concurrent,
                                     hipStream_t stream) {
  if (method < jb::PERCEPTRON || method > jb::NHERD) return (int)hipErrorInvalidValue;
  if (method >= jb::CW && P == nullptr) return (int)hipErrorInvalidValue;
  if (nstreams <= 0) return 0;
  const int threads = 256, blocks = (nstreams * 64 + threads - 1) / threads;
#define JB_STREAM(M)                                                                              \
  if (concurrent)                                                                                 \
    hipLaunchKernelGGL((jb::regression_train_kernel<M, true>), dim3(blocks), dim3(threads), 0,    \
                       stream, row_ptr, fidx, fval, targets, stream_ptr, nstreams, W, P, stats,   \
                       slot_scratch, C, eps);                                                     \
  else                                                                                            \
    hipLaunchKernelGGL((jb::regression_train_kernel<M, false>), dim3(blocks), dim3(threads), 0,   \
                       stream, row_ptr, fidx, fval, targets, stream_ptr, nstreams, W, P, stats,   \
                       slot_scratch, C, eps);
  JB_REG_DISPATCH(method, JB_STREAM)
#undef JB_STREAM
  return (int)hipGetLastError();
}

extern "C" int jb_regression_estimate(const int64_t* row_ptr, const int32_t* fidx,
                                      const float* fval, int n, const float* W, float* out,
                                      hipStream_t stream) {
  if (n <= 0) return 0;
  const int threads = 256, blocks = (n * 64 + threads - 1) / threads;
  hipLaunchKernelGGL(jb::regression_estimate_kernel, dim3(blocks), dim3(threads), 0, stream,
                     row_ptr, fidx, fval, n, W, out);
  return (int)hipGetLastError();
}
