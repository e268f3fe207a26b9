// The regression train kernels' one sample step (regression.hip,
// regression_ordered.hip): the step sizes of the seven methods, the target
// statistics, the gather-compute-scatter of one sample over a table-access
// type, the two table-access types and the method dispatch.
#pragma once
#include "jb_linear.hpp"

namespace jb {

// step sizes of one sample (M: Method of jb_linear.hpp): w += sgn tau (S) x,
// P increments from beta (dprec); false when the sample causes no update
template <int M>
__device__ __forceinline__ bool regression_step(float loss, float nrm, float var, float C,
                                                float* tau, float* beta) {
  *beta = 0.f;
  if (M == CW) {
    if (!(var > 0.f)) return false;
    const float m = -loss, phi = C;
    const float b = 1.f + 2.f * phi * m;
    const float gamma = (-b + sqrtf(fmaxf(0.f, b * b - 8.f * phi * (m - phi * var)))) / (4.f * phi * var);
    if (!(gamma > 0.f)) return false;
    *tau = gamma;
    *beta = 2.f * gamma * phi;
    return true;
  }
  if (!(loss > 0.f) || !(nrm > 0.f)) return false;
  if (M == PA) {
    *tau = fminf(C, loss) / nrm;
  } else if (M == PA1) {
    *tau = fminf(C, loss / nrm);
  } else if (M == PA2) {
    *tau = loss / (nrm + 0.5f / C);
  } else if (M == PERCEPTRON) {
    *tau = C;                                   // the learning rate
  } else if (M == AROW) {
    *beta = 1.f / (var + 1.f / C);
    *tau = loss * *beta;
  } else {                                      // NHERD
    *tau = loss / (var + 1.f / C);
    const float cv = 1.f + C * var;
    *beta = (C * C * var + 2.f * C) / (cv * cv);
  }
  return true;
}

// the target statistics take y; -> the loss and the sign of the error
__device__ __forceinline__ float take_target(float y, float dot, float eps, float& sum, float& sq,
                                             float& cnt, float* sgn) {
  sum += y; sq += y * y; cnt += 1.f;
  const float avg = sum / cnt;
  const float sd = sqrtf(fmaxf(0.f, sq / cnt - avg * avg));
  const float err = y - dot;
  *sgn = err > 0.f ? 1.f : -1.f;
  return *sgn * err - eps * sd;
}

// slots of a sample whose key, x and pre-sample P stay in registers between
// the gather and the scatter: kRegChunks chunks of 64 (PA on the stream
// kernel and the ordered kernel's samples of at most 64 slots keep one chunk)
constexpr int kRegChunks = 4;
constexpr int kRegSlots = kRegChunks * 64;

// One sample on the tables behind T: gather, compute, scatter, by one wave64
// alone (no workgroup barrier). Lane j owns slots j, j + 64, ... of the
// sample's n; the first RC chunks keep key, x and P in registers, and TAIL
// says whether slots past them can exist at all. The target *y is read after
// the wave sums and returned; sum / sq / cnt are the target statistics, which
// take it also when the sample causes no update.
//
// T supplies what differs between the callers (GlobalTables, LdsTables):
//   key(j), x(j)       slot j; key < 0 is a skipped slot
//   w(key), p(key)     the tables at a key
//   add_w, add_p       float atomic adds (an index repeated inside the sample
//                      counts per occurrence); add_p returns the P before it
//   park(j, v), parked(j)   a P increment kept per slot
//   drain()            before the first table read of a register chunk
//   wait()             between steps 1 and 2 below
//   kReturning         the concurrent rule of step 2
//
// The pre-sample-P rule: every occurrence's w step and P increment take the P
// the sample found, also when the index occurs again in another chunk. The
// register slots scatter from what they gathered and read nothing. The slots
// past them read P again, which is only sound while no P add of this sample
// has been issued, so the confidence methods (COV) scatter in three steps:
// the slots past the registers step w and park their P increments, then the
// register slots scatter, then the parked increments are added.
//
// kReturning (concurrent streams): a slot whose key is unique among the
// register slots adds its P increment first with a returning atomic and steps
// w with the returned P, the variance at this update's place in the row's
// atomic order (linear.hip "Serialized confidence" has the reason). Repeated
// slots and the slots past the registers keep the gathered value.
template <int M, int RC, bool TAIL, typename T>
__device__ __forceinline__ float regression_sample(const T& t, int n, const float* y, float C,
                                                   float eps, int lane, float& sum, float& sq,
                                                   float& cnt) {
  constexpr bool COV = M >= CW;
  constexpr int kReg = RC * 64;
  float dot = 0.f, nrm = 0.f, var = 0.f;
  int32_t rk[RC];
  float rx[RC], rp[RC];
#pragma unroll
  for (int c = 0; c < RC; ++c) {
    rk[c] = -1; rx[c] = 0.f; rp[c] = 1.f;
    // one chunk and no tail: no wave-uniform test at all, j < n masks the
    // chunk (a branch less on the chain of a narrow sample, measured)
    if ((RC == 1 && !TAIL) || c * 64 < n) {
      const int j = c * 64 + lane;
      if (j < n) { rk[c] = t.key(j); rx[c] = t.x(j); }
      // behind the slot loads and not in front of them: what is drained
      // completes while this sample's own slots are on their way; a sample
      // without slots drains nothing
      if (c * 64 < n) t.drain();
      if (rk[c] >= 0) {
        const float w = t.w(rk[c]);
        if (COV) rp[c] = t.p(rk[c]);
        const float x2 = rx[c] * rx[c];
        dot += rx[c] * w;
        nrm += x2;
        if (COV) var += x2 * (1.f / rp[c]);
      }
    }
  }
  if (TAIL) {
    for (int base = kReg; base < n; base += 64) {
      const int j = base + lane;
      if (j >= n) continue;
      const int32_t k = t.key(j);
      if (k < 0) continue;
      const float x = t.x(j);
      const float w = t.w(k);
      dot += x * w;
      nrm += x * x;
      if (COV) var += x * x * (1.f / t.p(k));
    }
  }
  dot = wave_sum(dot);
  nrm = wave_sum(nrm);
  if (COV) var = wave_sum(var);
  const float target = *y;
  float sgn;
  const float loss = take_target(target, dot, eps, sum, sq, cnt, &sgn);
  float tau = 0.f, beta = 0.f;
  if (!regression_step<M>(loss, nrm, var, C, &tau, &beta)) return target;
  const float coeff = sgn * tau;
  if (!COV) {
#pragma unroll
    for (int c = 0; c < RC; ++c)
      if (rk[c] >= 0) t.add_w(rk[c], coeff * rx[c]);
    if (TAIL) {
      for (int base = kReg; base < n; base += 64) {
        const int j = base + lane;
        if (j >= n) continue;
        const int32_t k = t.key(j);
        if (k >= 0) t.add_w(k, coeff * t.x(j));
      }
    }
    return target;
  }
  // 1. slots past the registers: P is still as the sample found it
  if (TAIL) {
    for (int base = kReg; base < n; base += 64) {
      const int j = base + lane;
      if (j >= n) continue;
      const int32_t k = t.key(j);
      if (k < 0) continue;
      const float x = t.x(j);
      const float sv = 1.f / t.p(k);
      t.add_w(k, coeff * sv * x);
      t.park(j, dprec(M, beta, x, sv));
    }
    // every P read of step 1 has returned (and every parked increment is
    // written) before the first P add below is issued
    if (n > kReg) t.wait();
  }
  // 2. register slots
  bool dup[RC];
#pragma unroll
  for (int c = 0; c < RC; ++c) dup[c] = !T::kReturning;
  if (T::kReturning) {
#pragma unroll
    for (int c = 0; c < RC; ++c) {
      const int m = min(64, n - c * 64);
      for (int j = 0; j < m; ++j) {
        const int32_t kj = __builtin_amdgcn_readlane(rk[c], j);
#pragma unroll
        for (int d = 0; d < RC; ++d) dup[d] |= kj == rk[d] && !(c == d && j == lane);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < RC; ++c) {
    if (rk[c] < 0) continue;
    const float sv = 1.f / rp[c];
    const float dp = dprec(M, beta, rx[c], sv);
    if (T::kReturning && !dup[c]) {
      const float pr = t.add_p(rk[c], dp);
      t.add_w(rk[c], coeff * rx[c] / pr);
    } else {
      t.add_w(rk[c], coeff * sv * rx[c]);
      t.add_p(rk[c], dp);
    }
  }
  // 3. the parked increments
  if (TAIL) {
    for (int base = kReg; base < n; base += 64) {
      const int j = base + lane;
      if (j >= n) continue;
      const int32_t k = t.key(j);
      if (k >= 0) t.add_p(k, t.parked(j));
    }
  }
  return target;
}

// The sample at fidx / fval[beg ..] on W / P in global memory; a key is a row
// index. The tables are read with agent-scope loads. One stream (!CONC): the
// adds of the wave's previous sample are drained before this sample's first
// table read, which therefore sees them. park: one float per slot in the
// caller's slot_scratch, needed by a COV sample wider than the register slots
// (the callers check for it).
template <bool CONC>
struct GlobalTables {
  static constexpr bool kReturning = CONC;
  const int32_t* fidx;
  const float* fval;
  int64_t beg;
  float* W;
  float* P;
  float* slot_scratch;
  __device__ __forceinline__ int32_t key(int j) const { return fidx[beg + j]; }
  __device__ __forceinline__ float x(int j) const { return fval[beg + j]; }
  __device__ __forceinline__ float w(int32_t k) const { return ld_agent(W + k); }
  __device__ __forceinline__ float p(int32_t k) const { return ld_agent(P + k); }
  __device__ __forceinline__ void add_w(int32_t k, float v) const { atomicAdd(W + k, v); }
  __device__ __forceinline__ float add_p(int32_t k, float v) const { return atomicAdd(P + k, v); }
  __device__ __forceinline__ void park(int j, float v) const { slot_scratch[beg + j] = v; }
  __device__ __forceinline__ float parked(int j) const { return ld_agent(slot_scratch + beg + j); }
  __device__ __forceinline__ void drain() const {
    if (!CONC) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __device__ __forceinline__ void wait() const { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

// The sample at s_pos / s_x[off ..] on a window's tables in LDS; a key is a
// table position. A wave's LDS operations execute in program order, so there
// is nothing to drain or to wait for.
struct LdsTables {
  static constexpr bool kReturning = false;
  const int* s_pos;
  const float* s_x;
  float* s_w;
  float* s_p;
  float* s_dp;
  int off;
  __device__ __forceinline__ int32_t key(int j) const { return s_pos[off + j]; }
  __device__ __forceinline__ float x(int j) const { return s_x[off + j]; }
  __device__ __forceinline__ float w(int32_t k) const { return s_w[k]; }
  __device__ __forceinline__ float p(int32_t k) const { return s_p[k]; }
  __device__ __forceinline__ void add_w(int32_t k, float v) const { atomicAdd(s_w + k, v); }
  __device__ __forceinline__ float add_p(int32_t k, float v) const { return atomicAdd(s_p + k, v); }
  __device__ __forceinline__ void park(int j, float v) const { s_dp[off + j] = v; }
  __device__ __forceinline__ float parked(int j) const { return s_dp[off + j]; }
  __device__ __forceinline__ void drain() const {}
  __device__ __forceinline__ void wait() const {}
};

}  // namespace jb

// method template dispatch (MV: a Method of jb_linear.hpp)
#define JB_REG_DISPATCH(MV, CALL)                      \
  switch (MV) {                                        \
    case jb::PERCEPTRON: CALL(jb::PERCEPTRON); break;  \
    case jb::PA: CALL(jb::PA); break;                  \
    case jb::PA1: CALL(jb::PA1); break;                \
    case jb::PA2: CALL(jb::PA2); break;                \
    case jb::CW: CALL(jb::CW); break;                  \
    case jb::AROW: CALL(jb::AROW); break;              \
    case jb::NHERD: CALL(jb::NHERD); break;            \
    default: return (int)hipErrorInvalidValue;         \
  }
