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
// The other six methods (regression_train_m_kernel) are the classifier's
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

template <bool CONC>
__global__ __launch_bounds__(256) void regression_train_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ fidx,
    const float* __restrict__ fval, const float* __restrict__ targets,
    const int64_t* __restrict__ stream_ptr, int nstreams, float* W, float* stats, float C,
    float eps) {
  const int lane = threadIdx.x & 63;
  const int wid = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wid >= nstreams) return;
  // CONC: a snapshot taken at this wave's start; earlier-finishing waves of
  // the same launch may or may not be in it (timing-dependent for eps > 0)
  float sum = stats[0], sq = stats[1], cnt = stats[2];
  float dsum = 0.f, dsq = 0.f, dcnt = 0.f;
  for (int64_t s = stream_ptr[wid]; s < stream_ptr[wid + 1]; ++s) {
    const int64_t beg = row_ptr[s];
    const int n = (int)(row_ptr[s + 1] - beg);
    float dot = 0.f, nrm = 0.f;
    int32_t idx0 = -1;
    float x0 = 0.f;
    for (int base = 0; base < n; base += 64) {
      const int j = base + lane;
      int32_t idx = -1;
      float x = 0.f;
      if (j < n) { idx = fidx[beg + j]; x = fval[beg + j]; }
      // exact mode: the previous sample's adds are drained here, before the
      // first read of w, so they complete behind this sample's row_ptr /
      // fidx / fval loads and not in front of them
      if (!CONC) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (idx >= 0) {
        const float w = ld_agent_r(W + idx);
        dot += x * w;
        nrm += x * x;
      }
      if (base == 0) { idx0 = idx; x0 = x; }
    }
    dot = wave_sum(dot);
    nrm = wave_sum(nrm);
    const float y = targets[s];
    sum += y; sq += y * y; cnt += 1.f;
    dsum += y; dsq += y * y; dcnt += 1.f;
    const float avg = sum / cnt;
    const float sd = sqrtf(fmaxf(0.f, sq / cnt - avg * avg));
    const float err = y - dot;
    const float sgn = err > 0.f ? 1.f : -1.f;
    const float loss = sgn * err - eps * sd;
    if (!(loss > 0.f) || !(nrm > 0.f)) continue;
    const float coeff = sgn * fminf(C, loss) / nrm;
    for (int base = 0; base < n; base += 64) {
      const int j = base + lane;
      if (j >= n) continue;
      int32_t idx; float x;
      if (base == 0) { idx = idx0; x = x0; }
      else { idx = fidx[beg + j]; x = fval[beg + j]; }
      if (idx < 0) continue;
      atomicAdd(W + idx, coeff * x);   // per occurrence: equal indices on two lanes both land
    }
  }
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

// ------------------------------------------------- the methods besides PA
// (regression_step and the register-slot geometry: jb_regression.hpp)
//
// PA1 / PA2 / perceptron / CW / AROW / NHERD, same stream model and idioms as
// regression_train_kernel. The confidence methods (COV) gather 1/P with w.
//
// The pre-sample-P rule: every occurrence's w step and P increment take the P
// the sample found, also when the index occurs again in another chunk. The
// first kRegSlots slots keep idx, x and P in registers, so their scatter reads
// nothing. A wider sample's remaining slots read P again, which is only
// sound while no P add of this sample has been issued: their w steps go first
// and their P increments are parked in slot_scratch[beg + j] (one float per
// slot, the caller's), then the register slots scatter, then the parked
// increments are added. A wide sample without slot_scratch is a caller
// error: the stream stops there and its statistics become NaN (nothing is
// written through the null pointer).
//
// Concurrent streams, confidence methods: a slot whose index is unique among
// the register slots adds its P increment first with a returning atomic and
// steps w with the returned P, the variance at this update's place in the
// row's atomic order (linear.hip "Serialized confidence" has the reason; one
// stream gets back the value it gathered). Repeated slots and the slots past
// the registers keep the gathered value.
template <int M, bool CONC>
__global__ __launch_bounds__(256) void regression_train_m_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ fidx,
    const float* __restrict__ fval, const float* __restrict__ targets,
    const int64_t* __restrict__ stream_ptr, int nstreams, float* W, float* P, float* stats,
    float* slot_scratch, float C, float eps) {
  constexpr bool COV = M >= CW;
  const int lane = threadIdx.x & 63;
  const int wid = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (wid >= nstreams) return;
  float sum = stats[0], sq = stats[1], cnt = stats[2];
  float dsum = 0.f, dsq = 0.f, dcnt = 0.f;
  for (int64_t s = stream_ptr[wid]; s < stream_ptr[wid + 1]; ++s) {
    const int64_t beg = row_ptr[s];
    const int n = (int)(row_ptr[s + 1] - beg);
    if (COV && n > kRegSlots && slot_scratch == nullptr) {
      sum = dsum = __builtin_nanf("");
      break;
    }
    float dot = 0.f, nrm = 0.f, var = 0.f;
    int32_t ri[kRegChunks];
    float rx[kRegChunks], rp[kRegChunks];
#pragma unroll
    for (int c = 0; c < kRegChunks; ++c) {
      ri[c] = -1; rx[c] = 0.f; rp[c] = 1.f;
      if (c * 64 < n) {
        const int j = c * 64 + lane;
        if (j < n) { ri[c] = fidx[beg + j]; rx[c] = fval[beg + j]; }
        // exact mode: the previous sample's adds, on w and on P, are drained
        // before this sample's first table read (as regression_train_kernel)
        if (!CONC) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (ri[c] >= 0) {
          const float w = ld_agent_r(W + ri[c]);
          if (COV) rp[c] = ld_agent_r(P + ri[c]);
          const float x2 = rx[c] * rx[c];
          dot += rx[c] * w;
          nrm += x2;
          if (COV) var += x2 * (1.f / rp[c]);
        }
      }
    }
    for (int base = kRegSlots; base < n; base += 64) {
      const int j = base + lane;
      if (j >= n) continue;
      const int32_t idx = fidx[beg + j];
      if (idx < 0) continue;
      const float x = fval[beg + j];
      const float w = ld_agent_r(W + idx);
      dot += x * w;
      nrm += x * x;
      if (COV) var += x * x * (1.f / ld_agent_r(P + idx));
    }
    dot = wave_sum(dot);
    nrm = wave_sum(nrm);
    if (COV) var = wave_sum(var);
    const float y = targets[s];
    sum += y; sq += y * y; cnt += 1.f;
    dsum += y; dsq += y * y; dcnt += 1.f;
    const float avg = sum / cnt;
    const float sd = sqrtf(fmaxf(0.f, sq / cnt - avg * avg));
    const float err = y - dot;
    const float sgn = err > 0.f ? 1.f : -1.f;
    const float loss = sgn * err - eps * sd;
    float tau = 0.f, beta = 0.f;
    if (!regression_step<M>(loss, nrm, var, C, &tau, &beta)) continue;
    const float coeff = sgn * tau;
    if (!COV) {
#pragma unroll
      for (int c = 0; c < kRegChunks; ++c)
        if (ri[c] >= 0) atomicAdd(W + ri[c], coeff * rx[c]);   // per occurrence
      for (int base = kRegSlots; base < n; base += 64) {
        const int j = base + lane;
        if (j >= n) continue;
        const int32_t idx = fidx[beg + j];
        if (idx >= 0) atomicAdd(W + idx, coeff * fval[beg + j]);
      }
      continue;
    }
    // 1. slots past the registers: P is still as the sample found it
    for (int base = kRegSlots; base < n; base += 64) {
      const int j = base + lane;
      if (j >= n) continue;
      const int32_t idx = fidx[beg + j];
      if (idx < 0) continue;
      const float x = fval[beg + j];
      const float sv = 1.f / ld_agent_r(P + idx);
      atomicAdd(W + idx, coeff * sv * x);
      slot_scratch[beg + j] = dprec(M, beta, x, sv);
    }
    // every P read of step 1 has returned (and every parked increment is
    // written) before the first P add below is issued
    if (n > kRegSlots) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // 2. register slots
    bool dup[kRegChunks];
#pragma unroll
    for (int c = 0; c < kRegChunks; ++c) dup[c] = !CONC;
    if (CONC) {
#pragma unroll
      for (int c = 0; c < kRegChunks; ++c) {
        const int m = min(64, n - c * 64);
        for (int j = 0; j < m; ++j) {
          const int32_t ij = __builtin_amdgcn_readlane(ri[c], j);
#pragma unroll
          for (int d = 0; d < kRegChunks; ++d) dup[d] |= ij == ri[d] && !(c == d && j == lane);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kRegChunks; ++c) {
      if (ri[c] < 0) continue;
      const float sv = 1.f / rp[c];
      const float dp = dprec(M, beta, rx[c], sv);
      if (CONC && !dup[c]) {
        const float pr = atomicAdd(P + ri[c], dp);
        atomicAdd(W + ri[c], coeff * rx[c] / pr);
      } else {
        atomicAdd(W + ri[c], coeff * sv * rx[c]);
        atomicAdd(P + ri[c], dp);
      }
    }
    // 3. the parked increments
    for (int base = kRegSlots; base < n; base += 64) {
      const int j = base + lane;
      if (j >= n) continue;
      const int32_t idx = fidx[beg + j];
      if (idx >= 0) atomicAdd(P + idx, ld_agent_r(slot_scratch + beg + j));
    }
  }
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

}  // namespace jb

// PA keeps its own kernel (docs/PERFORMANCE.md); jb_regression_train_m forwards here
static int launch_pa(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                     const float* targets, const int64_t* stream_ptr, int nstreams, float* W,
                     float* stats, float C, float eps, int concurrent, hipStream_t stream) {
  if (nstreams <= 0) return 0;
  const int threads = 256, blocks = (nstreams * 64 + threads - 1) / threads;
  if (concurrent)
    hipLaunchKernelGGL(jb::regression_train_kernel<true>, dim3(blocks), dim3(threads), 0, stream,
                       row_ptr, fidx, fval, targets, stream_ptr, nstreams, W, stats, C, eps);
  else
    hipLaunchKernelGGL(jb::regression_train_kernel<false>, dim3(blocks), dim3(threads), 0, stream,
                       row_ptr, fidx, fval, targets, stream_ptr, nstreams, W, stats, C, eps);
  return (int)hipGetLastError();
}

// the one train entry point: contract in jb_hip_api.h
extern "C" int jb_regression_train_m(const int64_t* row_ptr, const int32_t* fidx, const float* fval,
                                     const float* targets, const int64_t* stream_ptr, int nstreams,
                                     float* W, float* P, float* stats, float* slot_scratch,
                                     int method, float C, float eps, int concurrent,
                                     hipStream_t stream) {
  if (method == jb::PA)
    return launch_pa(row_ptr, fidx, fval, targets, stream_ptr, nstreams, W, stats, C, eps,
                     concurrent, stream);
  if (method < jb::PERCEPTRON || method > jb::NHERD) return (int)hipErrorInvalidValue;
  if (method >= jb::CW && P == nullptr) return (int)hipErrorInvalidValue;
  if (nstreams <= 0) return 0;
  const int threads = 256, blocks = (nstreams * 64 + threads - 1) / threads;
#define JB_REG_LAUNCH(M)                                                                            \
  case M:                                                                                           \
    if (concurrent)                                                                                 \
      hipLaunchKernelGGL((jb::regression_train_m_kernel<M, true>), dim3(blocks), dim3(threads), 0,  \
                         stream, row_ptr, fidx, fval, targets, stream_ptr, nstreams, W, P, stats,   \
                         slot_scratch, C, eps);                                                     \
    else                                                                                            \
      hipLaunchKernelGGL((jb::regression_train_m_kernel<M, false>), dim3(blocks), dim3(threads), 0, \
                         stream, row_ptr, fidx, fval, targets, stream_ptr, nstreams, W, P, stats,   \
                         slot_scratch, C, eps);                                                     \
    break;
  switch (method) {
    JB_REG_LAUNCH(jb::PERCEPTRON)
    JB_REG_LAUNCH(jb::PA1)
    JB_REG_LAUNCH(jb::PA2)
    JB_REG_LAUNCH(jb::CW)
    JB_REG_LAUNCH(jb::AROW)
    JB_REG_LAUNCH(jb::NHERD)
  }
#undef JB_REG_LAUNCH
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
