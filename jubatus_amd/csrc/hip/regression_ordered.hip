// Serial-equivalent regression training of a batch of requests: the samples
// 0 .. n_samples-1 of one CSR batch are applied in index order, whatever the
// number of requests they came from (the callers lay the requests out back to
// back in request order, so index order is the serial order). The result is
// what the reference leaves behind under its model lock
// (jubatus/server/server/regression_serv.cpp:95-130), and it does not depend
// on timing. All seven methods, rules and oracle as regression.hip /
// models/regression.py.
//
// One launch is ONE workgroup of 1024 threads. There are no cross-workgroup
// flags and no spin waits; the waves meet at workgroup barriers under uniform
// control flow only, and every loop is bounded by its input. The chain of
// dependent reads of a sequential stream (slots, table gather, the previous
// sample's adds) stays inside the CU: the kernel works in windows whose rows
// live in LDS.
//
//  a. cut     a window is the longest run of whole samples from the current
//             position whose slot occurrences sum to at most win_slots
//             (binary search over row_ptr, every thread the same).
//  b. load    all waves read the window's fidx / fval coalesced and insert
//             the row indices into an open-addressing table in LDS (LDS
//             compare-and-swap, linear probing, at most `tab` probes). The
//             table has tab = max(64, 2 * win_slots rounded up to a power of
//             two) entries, so its load is at most 0.5 by construction. After
//             a barrier the occupied entries gather W[row] (and P[row] for CW /
//             AROW / NHERD): once per distinct row, all in flight together
//             (no load feeds control flow). P itself is stored, never 1/P: a
//             row that is loaded
//             and written back untouched keeps its bits. Every occurrence
//             keeps (table position, x) in LDS; a skipped slot (idx < 0) has
//             position -1.
//  c. apply   after a barrier wave 0 applies the window's samples one after
//             the other from LDS: lane j owns slots j, j + 64, ... as in
//             regression_train_m_kernel, the sums are wave_sum, the step is
//             regression_step, the target statistics ride in wave 0's
//             registers as sequential fp32 sums. Increments are LDS float
//             atomic adds, so an index repeated inside a sample counts per
//             occurrence. Every occurrence's w step and P increment take the
//             pre-sample P: the first 256 slots keep it in registers, the
//             slots beyond read it before any P add of the sample is issued
//             and park their increments per occurrence in LDS; a wave's LDS
//             operations execute in program order.
//  d. store   after a barrier all waves write the occupied entries back to
//             W / P and empty the table. The next window's gathers and the
//             global path of (e) must see these stores: every wave drains
//             its stores, barrier, one lane releases and acquires at agent
//             scope, barrier; the tables are read with agent-scope loads
//             (ld_agent_r), as the existing kernels do.
//  e. wide    a single sample of more than win_slots occurrences is applied
//             between two windows by wave 0 alone, directly on global memory,
//             with the gather-compute-scatter of regression_train_m_kernel
//             (one stream) and a drain. slot_scratch has that kernel's
//             contract: one float per slot, needed by CW / AROW / NHERD for
//             samples of more than 256 slots.
//
// Home position of row index idx in a table of 2^bits entries (mirrored by
// ops/hip.py regression_ordered_home):
//     home = ((uint32)idx * 0x9E3779B1u) >> (32 - bits)
// and the probe sequence is home, home + 1, ... modulo the table size.
//
// status[0] is 0 on success. A can't-happen exit writes a nonzero code to
// status[0] and the index of the first sample that was NOT applied to
// status[1]; every sample before it is applied and written back, the
// statistics count exactly those, and nothing after it is touched:
//     1  the LDS table took no more rows (a full probe)
//     2  row_ptr is not monotone
//     3  CW / AROW / NHERD, a sample of more than 256 slots on the global
//        path without slot_scratch
#include "jb_hip_api.h"
#include "jb_linear.hpp"
#include "jb_regression.hpp"

namespace jb {
namespace ord {

// 16 waves: the load and store phases of a window are latency-bound loops
// over its slots and its table, so their length goes with 1 / threads
constexpr int kThreads = 1024;
// default and largest window: 4096 slot occurrences, a table of 8192 entries
constexpr int kWinSlots = 4096;
constexpr int kMinTab = 64;

// LDS image: key, w, P per table entry; position, x, parked P increment per occurrence
__host__ __device__ constexpr int tab_entries(int win) {
  int t = kMinTab;
  while (t < 2 * win) t <<= 1;
  return t;
}
__host__ __device__ constexpr int lds_bytes(int win) { return tab_entries(win) * 12 + win * 12; }
static_assert(tab_entries(kWinSlots) == 8192, "load 0.5 at the default window");
// 144 KiB of dynamic LDS + the few static words below, of the CU's 160 KiB
static_assert(lds_bytes(kWinSlots) + 256 <= 160 * 1024, "the window image must fit the CU's LDS");

enum : int { kOk = 0, kErrProbe = 1, kErrRowPtr = 2, kErrScratch = 3 };

template <int M>
__device__ __forceinline__ bool ordered_step(float loss, float nrm, float var, float C, float* tau,
                                             float* beta) {
  if (M == PA) {                      // regression_train_kernel: sgn * min(C, loss) / ||x||^2
    *beta = 0.f;
    if (!(loss > 0.f) || !(nrm > 0.f)) return false;
    *tau = fminf(C, loss) / nrm;
    return true;
  }
  return regression_step<M>(loss, nrm, var, C, tau, beta);
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

// c. a sample of at most 64 slots, from LDS (wave 0): one slot a lane, no
// loops (lds_sample below, cut down to its first chunk; the same arithmetic)
template <int M>
__device__ __forceinline__ void lds_sample_narrow(const int* s_pos, const float* s_x, float* s_w,
                                                  float* s_p, int off, int n, float y, float C,
                                                  float eps, int lane, float& sum, float& sq,
                                                  float& cnt) {
  constexpr bool COV = M >= CW;
  float dot = 0.f, nrm = 0.f, var = 0.f;
  int pos = -1;
  float x = 0.f, p = 1.f;
  if (lane < n) { pos = s_pos[off + lane]; x = s_x[off + lane]; }
  if (pos >= 0) {
    const float w = s_w[pos];
    if (COV) p = s_p[pos];
    const float x2 = x * x;
    dot += x * w;
    nrm += x2;
    if (COV) var += x2 * (1.f / p);
  }
  dot = wave_sum(dot);
  nrm = wave_sum(nrm);
  if (COV) var = wave_sum(var);
  float sgn;
  const float loss = take_target(y, dot, eps, sum, sq, cnt, &sgn);
  float tau = 0.f, beta = 0.f;
  if (!ordered_step<M>(loss, nrm, var, C, &tau, &beta)) return;
  const float coeff = sgn * tau;
  if (pos < 0) return;
  if (!COV) {
    atomicAdd(s_w + pos, coeff * x);                       // per occurrence
    return;
  }
  const float sv = 1.f / p;
  atomicAdd(s_w + pos, coeff * sv * x);
  atomicAdd(s_p + pos, dprec(M, beta, x, sv));
}

// c. one sample of the window of any width, from LDS (wave 0). off / n: its
// occurrences in s_pos / s_x. The shape of regression_train_m_kernel: the first kRegSlots
// slots keep position, x and the pre-sample P in registers between the gather
// and the scatter (their LDS reads are all in flight together); a wider
// sample's remaining slots step w first, while P is still as the sample found
// it, and park their P increments in s_dp.
template <int M>
__device__ __forceinline__ void lds_sample(const int* s_pos, const float* s_x, float* s_w, float* s_p,
                                           float* s_dp, int off, int n, float y, float C, float eps,
                                           int lane, float& sum, float& sq, float& cnt) {
  constexpr bool COV = M >= CW;
  float dot = 0.f, nrm = 0.f, var = 0.f;
  int rpos[kRegChunks];
  float rx[kRegChunks], rp[kRegChunks];
#pragma unroll
  for (int c = 0; c < kRegChunks; ++c) {
    rpos[c] = -1; rx[c] = 0.f; rp[c] = 1.f;
    if (c * 64 < n) {
      const int j = c * 64 + lane;
      if (j < n) { rpos[c] = s_pos[off + j]; rx[c] = s_x[off + j]; }
      if (rpos[c] >= 0) {
        const float w = s_w[rpos[c]];
        if (COV) rp[c] = s_p[rpos[c]];
        const float x2 = rx[c] * rx[c];
        dot += rx[c] * w;
        nrm += x2;
        if (COV) var += x2 * (1.f / rp[c]);
      }
    }
  }
  for (int j = kRegSlots + lane; j < n; j += 64) {
    const int pos = s_pos[off + j];
    if (pos < 0) continue;
    const float x = s_x[off + j];
    const float w = s_w[pos];
    dot += x * w;
    nrm += x * x;
    if (COV) var += x * x * (1.f / s_p[pos]);
  }
  dot = wave_sum(dot);
  nrm = wave_sum(nrm);
  if (COV) var = wave_sum(var);
  float sgn;
  const float loss = take_target(y, dot, eps, sum, sq, cnt, &sgn);
  float tau = 0.f, beta = 0.f;
  if (!ordered_step<M>(loss, nrm, var, C, &tau, &beta)) return;
  const float coeff = sgn * tau;
  if (!COV) {
#pragma unroll
    for (int c = 0; c < kRegChunks; ++c)
      if (rpos[c] >= 0) atomicAdd(s_w + rpos[c], coeff * rx[c]);   // per occurrence
    for (int j = kRegSlots + lane; j < n; j += 64) {
      const int pos = s_pos[off + j];
      if (pos >= 0) atomicAdd(s_w + pos, coeff * s_x[off + j]);
    }
    return;
  }
  // 1. slots past the registers: every P read here is the pre-sample P (no P
  //    add of this sample has been issued; a wave's LDS operations execute in
  //    program order), the P increments are parked
  for (int j = kRegSlots + lane; j < n; j += 64) {
    const int pos = s_pos[off + j];
    if (pos < 0) continue;
    const float x = s_x[off + j];
    const float sv = 1.f / s_p[pos];
    atomicAdd(s_w + pos, coeff * sv * x);
    s_dp[off + j] = dprec(M, beta, x, sv);
  }
  // 2. register slots, from the P they gathered
#pragma unroll
  for (int c = 0; c < kRegChunks; ++c) {
    if (rpos[c] < 0) continue;
    const float sv = 1.f / rp[c];
    atomicAdd(s_w + rpos[c], coeff * sv * rx[c]);
    atomicAdd(s_p + rpos[c], dprec(M, beta, rx[c], sv));
  }
  // 3. the parked increments
  for (int j = kRegSlots + lane; j < n; j += 64) {
    const int pos = s_pos[off + j];
    if (pos >= 0) atomicAdd(s_p + pos, s_dp[off + j]);
  }
}

// e. one sample on global memory (wave 0): regression_train_m_kernel's one-stream
// body. -> false: CW / AROW / NHERD past the register slots without slot_scratch
// (nothing applied, the statistics untouched)
template <int M>
__device__ __forceinline__ bool global_sample(const int32_t* __restrict__ fidx,
                                              const float* __restrict__ fval, int64_t beg, int n,
                                              float y, float* W, float* P, float* slot_scratch,
                                              float C, float eps, int lane, float& sum, float& sq,
                                              float& cnt) {
  constexpr bool COV = M >= CW;
  if (COV && n > kRegSlots && slot_scratch == nullptr) return false;
  float dot = 0.f, nrm = 0.f, var = 0.f;
  int32_t ri[kRegChunks];
  float rx[kRegChunks], rp[kRegChunks];
#pragma unroll
  for (int c = 0; c < kRegChunks; ++c) {
    ri[c] = -1; rx[c] = 0.f; rp[c] = 1.f;
    if (c * 64 < n) {
      const int j = c * 64 + lane;
      if (j < n) { ri[c] = fidx[beg + j]; rx[c] = fval[beg + j]; }
      // earlier adds of this wave are drained before the first table read
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
  float sgn;
  const float loss = take_target(y, dot, eps, sum, sq, cnt, &sgn);
  float tau = 0.f, beta = 0.f;
  if (!ordered_step<M>(loss, nrm, var, C, &tau, &beta)) return true;
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
    return true;
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
#pragma unroll
  for (int c = 0; c < kRegChunks; ++c) {
    if (ri[c] < 0) continue;
    const float sv = 1.f / rp[c];
    atomicAdd(W + ri[c], coeff * sv * rx[c]);
    atomicAdd(P + ri[c], dprec(M, beta, rx[c], sv));
  }
  // 3. the parked increments
  for (int base = kRegSlots; base < n; base += 64) {
    const int j = base + lane;
    if (j >= n) continue;
    const int32_t idx = fidx[beg + j];
    if (idx >= 0) atomicAdd(P + idx, ld_agent_r(slot_scratch + beg + j));
  }
  return true;
}

// d. the stores of every wave are visible to every later agent-scope load of
// this workgroup (uniform control flow: every thread calls it). -> the error
// word, read between the two barriers: every write of the phase before lies
// in front of the first barrier and the next write behind the second one, so
// every thread returns the same value.
__device__ __forceinline__ int publish_block(const int* s_err) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int err = *s_err;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  return err;
}

template <int M>
__global__ __launch_bounds__(kThreads) void regression_ordered_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ fidx,
    const float* __restrict__ fval, const float* __restrict__ targets, int64_t n_samples, float* W,
    float* P, float* stats, float* slot_scratch, float C, float eps, int win, int bits,
    int32_t* status) {
  constexpr bool COV = M >= CW;
  extern __shared__ __attribute__((aligned(16))) char s_ord[];
  __shared__ int s_err;        // code of the first can't-happen event, 0 for none
  __shared__ int s_fail;       // apply phase: the first sample that was not applied
  const int tab = 1 << bits;
  int* s_key = reinterpret_cast<int*>(s_ord);               // [tab] row index, -1 empty
  float* s_w = reinterpret_cast<float*>(s_key + tab);       // [tab]
  float* s_p = s_w + tab;                                   // [tab]
  int* s_pos = reinterpret_cast<int*>(s_p + tab);           // [win] table position, -1 skipped
  float* s_x = reinterpret_cast<float*>(s_pos + win);       // [win]
  float* s_dp = s_x + win;                                  // [win] parked P increments
  const int tid = threadIdx.x, lane = tid & 63;
  const bool wave0 = tid < 64;

  for (int t = tid; t < tab; t += kThreads) s_key[t] = -1;
  if (tid == 0) { s_err = kOk; s_fail = 0; }
  float sum = stats[0], sq = stats[1], cnt = stats[2];      // wave 0's are the live ones
  __syncthreads();

  int code = kOk;
  int64_t s = 0;               // the first sample not applied yet
  while (s < n_samples) {      // every turn advances s or leaves
    // a. the longest run of whole samples [s, e) with at most win occurrences
    const int64_t base = row_ptr[s];
    int64_t lo = s, hi = n_samples;
    while (lo < hi) {          // row_ptr[lo] - base <= win holds throughout
      const int64_t mid = lo + (hi - lo + 1) / 2;
      if (row_ptr[mid] - base <= win) lo = mid; else hi = mid - 1;
    }
    const int64_t e = lo;
    if (e == s) {
      // e. the sample at s alone is wider than a window
      const int64_t wide = row_ptr[s + 1] - base;
      if (wide <= 0 || wide > INT32_MAX) { code = kErrRowPtr; break; }
      if (wave0) {
        const bool ok = global_sample<M>(fidx, fval, base, (int)wide, targets[s], W, P, slot_scratch,
                                         C, eps, lane, sum, sq, cnt);
        if (!ok && lane == 0) s_err = kErrScratch;
      }
      const int err = publish_block(&s_err);
      if (err != kOk) { code = err; break; }
      s += 1;
      continue;
    }
    const int occ = (int)(row_ptr[e] - base);
    if (occ < 0) { code = kErrRowPtr; break; }
    // b. the window's slots into LDS (a thread keeps its own slots: no barrier
    // between the two loops), its rows into the table, then the gather
    for (int t = tid; t < occ; t += kThreads) {
      s_pos[t] = fidx[base + t];
      s_x[t] = fval[base + t];
    }
    for (int t = tid; t < occ; t += kThreads) {
      const int32_t idx = s_pos[t];
      int pos = -1;
      if (idx >= 0) {
        uint32_t h = ((uint32_t)idx * 0x9E3779B1u) >> (32 - bits);
        for (int probe = 0; probe < tab; ++probe) {
          const int old = atomicCAS(s_key + h, -1, idx);
          if (old == -1 || old == idx) { pos = (int)h; break; }
          h = (h + 1) & (uint32_t)(tab - 1);
        }
        if (pos < 0) s_err = kErrProbe;
      }
      s_pos[t] = pos;
    }
    __syncthreads();
    for (int t = tid; t < tab; t += kThreads) {
      const int key = s_key[t];
      if (key < 0) continue;
      s_w[t] = ld_agent_r(W + key);
      if (COV) s_p[t] = ld_agent_r(P + key);
    }
    __syncthreads();
    // c. wave 0 applies the samples in order (none of them when the load failed;
    // the other waves learn of either failure from publish_block below)
    if (wave0 && s_err == kOk) {
      for (int64_t blk = s; blk < e; blk += 64) {
        // offsets and targets of 64 samples at a time, off the per-sample chain
        const int m = (int)(e - blk < 64 ? e - blk : 64);
        int64_t b = 0, en = 0;
        float tg = 0.f;
        if (lane < m) {
          b = row_ptr[blk + lane] - base;
          en = row_ptr[blk + lane + 1] - base;
          tg = targets[blk + lane];
        }
        const bool bad = lane < m && (b < 0 || en < b || en > occ);
        const uint64_t badm = __ballot(bad);
        const int good = badm ? __ffsll((unsigned long long)badm) - 1 : m;
        for (int k = 0; k < good; ++k) {
          const int off = __builtin_amdgcn_readlane((int)b, k);
          const int n = __builtin_amdgcn_readlane((int)en, k) - off;
          const float y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tg), k));
          if (n <= 64)
            lds_sample_narrow<M>(s_pos, s_x, s_w, s_p, off, n, y, C, eps, lane, sum, sq, cnt);
          else
            lds_sample<M>(s_pos, s_x, s_w, s_p, s_dp, off, n, y, C, eps, lane, sum, sq, cnt);
        }
        if (badm) {
          if (lane == 0) { s_err = kErrRowPtr; s_fail = (int)(blk + good - s); }
          break;
        }
      }
    }
    __syncthreads();
    // d. the occupied entries back to the tables; the table is emptied
    for (int t = tid; t < tab; t += kThreads) {
      const int key = s_key[t];
      if (key < 0) continue;
      W[key] = s_w[t];
      if (COV) P[key] = s_p[t];
      s_key[t] = -1;
    }
    const int err = publish_block(&s_err);
    if (err != kOk) { code = err; s += s_fail; break; }   // s_fail: 0 unless the apply phase set it
    s = e;
  }
  if (tid == 0) {
    stats[0] = sum; stats[1] = sq; stats[2] = cnt;
    status[0] = code;
    status[1] = code == kOk ? 0 : (int32_t)s;
  }
}

}  // namespace ord
}  // namespace jb

// contract in jb_hip_api.h
extern "C" int jb_regression_train_ordered(const int64_t* row_ptr, const int32_t* fidx,
                                           const float* fval, const float* targets,
                                           int64_t n_samples, float* W, float* P, float* stats,
                                           float* slot_scratch, int method, float C, float eps,
                                           int win_slots, int32_t* status, hipStream_t stream) {
  namespace ord = jb::ord;
  if (method < jb::PERCEPTRON || method > jb::NHERD) return (int)hipErrorInvalidValue;
  if (method >= jb::CW && P == nullptr) return (int)hipErrorInvalidValue;
  if (win_slots < 0 || win_slots > ord::kWinSlots) return (int)hipErrorInvalidValue;
  if (status == nullptr || n_samples > INT32_MAX) return (int)hipErrorInvalidValue;   // status[1] is 32 bits
  if (n_samples <= 0) return 0;
  const int win = win_slots ? win_slots : ord::kWinSlots;
  const int tab = ord::tab_entries(win);
  int bits = 0;
  while ((1 << bits) < tab) ++bits;
  const int bytes = ord::lds_bytes(win);
#define JB_ORD_LAUNCH(M)                                                                          \
  case M: {                                                                                       \
    static const hipError_t attr = hipFuncSetAttribute(                                           \
        (const void*)jb::ord::regression_ordered_kernel<M>,                                       \
        hipFuncAttributeMaxDynamicSharedMemorySize, jb::ord::lds_bytes(jb::ord::kWinSlots));      \
    if (attr != hipSuccess) return (int)attr;                                                     \
    hipLaunchKernelGGL((jb::ord::regression_ordered_kernel<M>), dim3(1), dim3(jb::ord::kThreads), \
                       bytes, stream, row_ptr, fidx, fval, targets, n_samples, W, P, stats,       \
                       slot_scratch, C, eps, win, bits, status);                                  \
    break;                                                                                        \
  }
  switch (method) {
    JB_ORD_LAUNCH(jb::PERCEPTRON)
    JB_ORD_LAUNCH(jb::PA)
    JB_ORD_LAUNCH(jb::PA1)
    JB_ORD_LAUNCH(jb::PA2)
    JB_ORD_LAUNCH(jb::CW)
    JB_ORD_LAUNCH(jb::AROW)
    JB_ORD_LAUNCH(jb::NHERD)
  }
#undef JB_ORD_LAUNCH
  return (int)hipGetLastError();
}
