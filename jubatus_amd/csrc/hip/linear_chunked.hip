// Linear classifiers with a run-time label capacity (LC a multiple of 256, up
// to 16384): the train and classify kernels behind label capacities above
// 1024, where the per-lane accumulators of the LC-templated kernels of
// linear.hip (LC / 64 registers per lane) no longer fit.
//
// Reference: the same train / classify loops as linear.hip
// (jubatus/server/server/classifier_serv.cpp:128-173); the reference keeps its
// weights in a map keyed by label and has no label limit. The arithmetic is
// the one of general_sample (jb_linear.hpp) and models/linear_oracle.py.
//
// Train: one workgroup of 1, 4 or 16 wave64s per update stream; the samples
// of a stream are applied in order. Per sample
//   stage   the (idx, x) pairs go to LDS once (the first kStage of them; the
//           slots past that are read from global memory where they are used)
//   score   wave w takes the label chunks w, w + waves, ... of 256 labels;
//           inside a chunk lane l owns labels l, l + 64, l + 128, l + 192 and
//           sums x * W[idx * LC + label] over the features in feature order
//           (agent-scope loads: one 256-byte segment per instruction)
//   select  every lane keeps the score of y if it owns it and its best active
//           wrong label; reduced inside the wave, then across the waves through
//           LDS, ties to the lowest label index
//   update  the features are spread over all threads; only the columns y and
//           l* are written, with the memory-side adds of apply_row<kAtomic>
// Every __syncthreads() below is executed by every thread for every sample of
// the stream, whether the sample has a valid label, updates, or neither: the
// barriers sit at the top level of the sample loop and only the work between
// them is predicated.
//
// Classify: one wave per (sample, chunk), the same summation order.
#include <stdlib.h>

#include "jb_hip_api.h"
#include "jb_linear.hpp"

namespace jb {

constexpr int kChunk = 256;      // labels per chunk: 4 per lane
constexpr int kChunkK = kChunk / 64;
constexpr int kStage = 512;      // slots of a sample staged in LDS
constexpr int kScoreU = 8;       // slots whose row loads are in flight together
constexpr int kMaxWaves = 16;
constexpr int kMaxLC = 16384;
// waves per stream when the caller names none: exact mode at LC = 16384 ran
// fastest with 16 (profiles/many_labels.md)
constexpr int kDefaultWaves = 16;

// scores of the 4 labels col, col + 64, .. of one sample: slots below ns from
// the LDS stage, the rest from global memory. The slot is wave-uniform, so
// the row base is a scalar and the loads of a pass are unconditional (an
// invalid slot reads row 0 and is not accumulated).
template <typename WT>
__device__ __forceinline__ void chunk_scores(const int32_t* sI, const float* sX, int ns,
                                             const int32_t* __restrict__ fidx,
                                             const float* __restrict__ fval, int64_t beg, int n,
                                             const WT* W, int LC, int col, float (&acc)[kChunkK]) {
#pragma unroll
  for (int k = 0; k < kChunkK; ++k) acc[k] = 0.f;
  // kScoreU slots per pass: their kScoreU * 4 loads are all issued before the
  // first is used, then accumulated in slot order
  for (int j0 = 0; j0 < n; j0 += kScoreU) {
    float x[kScoreU], w[kScoreU][kChunkK];
    bool v[kScoreU];
#pragma unroll
    for (int u = 0; u < kScoreU; ++u) {
      const int j = j0 + u;
      int32_t idx = -1;
      x[u] = 0.f;
      if (j < n) {
        idx = j < ns ? sI[j] : fidx[beg + j];
        x[u] = j < ns ? sX[j] : fval[beg + j];
      }
      idx = __builtin_amdgcn_readfirstlane(idx);
      v[u] = idx >= 0;
      const WT* wr = W + (int64_t)(v[u] ? idx : 0) * LC + col;
#pragma unroll
      for (int k = 0; k < kChunkK; ++k) w[u][k] = ldw(wr + 64 * k);
    }
#pragma unroll
    for (int u = 0; u < kScoreU; ++u) {
#pragma unroll
      for (int k = 0; k < kChunkK; ++k) acc[k] = v[u] ? acc[k] + x[u] * w[u][k] : acc[k];
    }
  }
}

template <typename WT>
__global__ __launch_bounds__(64 * kMaxWaves) void linear_train_chunked_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ fidx,
    const float* __restrict__ fval, const int32_t* __restrict__ labels,
    const int64_t* __restrict__ stream_ptr, int nstreams, WT* W, float* P,
    const int32_t* __restrict__ active, int LC, int method, float C, int mode,
    unsigned long long* __restrict__ stats, uint8_t* __restrict__ touched) {
  __shared__ int32_t sI[kStage];
  __shared__ float sX[kStage];
  __shared__ float sA[kStage];      // 1 / P[row][y] and 1 / P[row][l*] of the staged
  __shared__ float sB[kStage];      // slots, read before the sample's update
  __shared__ float rBest[kMaxWaves];
  __shared__ int rBl[kMaxWaves];
  __shared__ float rVar[kMaxWaves];
  __shared__ float rNrm[kMaxWaves];
  __shared__ float rSy;
  const int tid = threadIdx.x;
  const int nthr = blockDim.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int nw = nthr >> 6;
  const int nchunks = LC / kChunk;
  const bool use_s = method >= CW;
  // the grid is one workgroup per stream, so the range is workgroup-uniform
  const int64_t s_beg = stream_ptr[blockIdx.x];
  const int64_t s_end = stream_ptr[blockIdx.x + 1];
  unsigned n_upd = 0, n_valid = 0;
  for (int64_t s = s_beg; s < s_end; ++s) {
    const int y = labels[s];
    const bool valid = y >= 0 && y < LC;
    const int64_t beg = row_ptr[s];
    const int n = valid ? (int)(row_ptr[s + 1] - beg) : 0;
    const int ns = n < kStage ? n : kStage;
    // ---- stage
    for (int j = tid; j < ns; j += nthr) {
      sI[j] = fidx[beg + j];
      sX[j] = fval[beg + j];
    }
    if (tid == 0) rSy = 0.f;
    __syncthreads();
    // ---- score and select
    float best = -INFINITY;
    int bl = -1;
    if (valid) {
      for (int c = wv; c < nchunks; c += nw) {
        const int col = c * kChunk + lane;
        float acc[kChunkK];
        chunk_scores<WT>(sI, sX, ns, fidx, fval, beg, n, W, LC, col, acc);
#pragma unroll
        for (int k = 0; k < kChunkK; ++k) {
          const int l = col + 64 * k;
          if (l == y) rSy = acc[k];
          else if (active[l] != 0 && acc[k] > best) { best = acc[k]; bl = l; }
        }
      }
      argmax_wrong<64>(best, bl);
    }
    if (lane == 0) {
      rBest[wv] = best;
      rBl[wv] = bl;
    }
    __syncthreads();
    best = -INFINITY;
    bl = -1;
    for (int w = 0; w < nw; ++w) {
      const float ob = rBest[w];
      const int ol = rBl[w];
      if (ol >= 0 && (bl < 0 || ob > best || (ob == best && ol < bl))) { best = ob; bl = ol; }
    }
    const int lstar = bl;
    const float margin = rSy - (lstar >= 0 ? best : 0.f);
    // ---- variance and norm
    float var = 0.f, nrm = 0.f;
    for (int j = tid; j < n; j += nthr) {
      const int32_t idx = j < ns ? sI[j] : fidx[beg + j];
      const float x = j < ns ? sX[j] : fval[beg + j];
      if (idx >= 0) {
        const int64_t row = (int64_t)idx * LC;
        nrm += x * x;
        if (use_s) {
          const float a = 1.f / ld_agent(P + row + y);
          const float b = lstar >= 0 ? 1.f / ld_agent(P + row + lstar) : 0.f;
          var += x * x * (a + b);
          if (j < ns) {
            sA[j] = a;
            sB[j] = lstar >= 0 ? b : 1.f;
          }
        }
      }
    }
    var = wave_sum(var);
    nrm = wave_sum(nrm);
    if (lane == 0) {
      rVar[wv] = var;
      rNrm[wv] = nrm;
    }
    __syncthreads();
    var = 0.f;
    nrm = 0.f;
    for (int w = 0; w < nw; ++w) {
      var += rVar[w];
      nrm += rNrm[w];
    }
    float tau = 0.f, beta = 0.f;
    const bool upd = valid && step_coeffs(method, margin, var, nrm, lstar >= 0, C, &tau, &beta);
    if (valid) ++n_valid;
    if (upd) ++n_upd;
    // ---- update, staged slots: the thread of a row's first slot applies every
    //      slot of that row in feature order with the precision from before the
    //      sample, so a repeated row counts every time and in a fixed order
    if (upd) {
      for (int j = tid; j < ns; j += nthr) {
        const int32_t idx = sI[j];
        if (idx < 0) continue;
        bool first = true;
        for (int i = 0; i < j; ++i) {
          if (sI[i] == idx) { first = false; break; }
        }
        if (!first) continue;
        const int64_t row = (int64_t)idx * LC;
        const float a = use_s ? sA[j] : 1.f;
        const float b = use_s ? sB[j] : 1.f;
        apply_row<kAtomic>(W, P, row, sX[j], y, lstar, use_s, method, tau, beta, a, b, 0.f, 0.f,
                           (uint32_t)beg);
        for (int i = j + 1; i < ns; ++i) {
          if (sI[i] == idx)
            apply_row<kAtomic>(W, P, row, sX[i], y, lstar, use_s, method, tau, beta, a, b, 0.f, 0.f,
                               (uint32_t)beg);
        }
        if (touched != nullptr) touched[idx] = 1;
      }
      if (n > ns) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // ---- update, slots past the stage (a sample wider than kStage): after the
    //      staged ones have landed, one slot per thread. A row that is also
    //      staged takes its staged precision, so it too is applied against the
    //      state before the sample and after its staged occurrences.
    //      Known limit: a row that repeats only among the slots past the stage
    //      is applied slot by slot as general_sample does, each with the
    //      precision it finds and in the order the atomics land, so for such a
    //      row two runs may differ in the last bits; "the same bits on every
    //      run" holds for everything else.
    if (upd) {
      for (int j = kStage + tid; j < n; j += nthr) {
        const int32_t idx = fidx[beg + j];
        if (idx < 0) continue;
        const float x = fval[beg + j];
        const int64_t row = (int64_t)idx * LC;
        float a = 1.f, b = 1.f;
        if (use_s) {
          int hit = -1;
          for (int i = 0; i < kStage; ++i) {
            if (sI[i] == idx) { hit = i; break; }
          }
          a = hit >= 0 ? sA[hit] : 1.f / ld_agent(P + row + y);
          b = hit >= 0 ? sB[hit] : (lstar >= 0 ? 1.f / ld_agent(P + row + lstar) : 1.f);
        }
        apply_row<kAtomic>(W, P, row, x, y, lstar, use_s, method, tau, beta, a, b, 0.f, 0.f,
                           (uint32_t)beg);
        if (touched != nullptr) touched[idx] = 1;
      }
    }
    // ---- exact mode: sample s + 1 sees sample s. Every wave drains its own
    //      stores and atomics and releases at agent scope before the barrier;
    //      the next sample reads the table with agent-scope loads only.
    if (mode == kExact) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    }
    __syncthreads();
  }
  if (stats != nullptr && tid == 0 && n_valid > 0) {
    atomicAdd(stats, (unsigned long long)n_upd);
    atomicAdd(stats + 1, (unsigned long long)n_valid);
  }
}

// one wave per (sample, chunk of 256 labels)
template <typename WT>
__global__ __launch_bounds__(256) void linear_classify_chunked_kernel(
    const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ fidx,
    const float* __restrict__ fval, int n_samples, const WT* W, int LC, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int nchunks = LC / kChunk;
  const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (g >= (int64_t)n_samples * nchunks) return;
  const int s = (int)(g / nchunks);
  const int col = (int)(g % nchunks) * kChunk + lane;
  const int64_t beg = row_ptr[s];
  const int n = (int)(row_ptr[s + 1] - beg);
  float acc[kChunkK];
  chunk_scores<WT>(nullptr, nullptr, 0, fidx, fval, beg, n, W, LC, col, acc);
#pragma unroll
  for (int k = 0; k < kChunkK; ++k) out[(int64_t)s * LC + col + 64 * k] = acc[k];
}

static bool chunked_lc_ok(int LC) { return LC >= kChunk && LC <= kMaxLC && LC % kChunk == 0; }

// waves per stream: JUBATUS_LABEL_WAVES (1, 4 or 16) or the measured default
static int label_waves() {
  static const int w = [] {
    const char* e = getenv("JUBATUS_LABEL_WAVES");
    const int v = e != nullptr ? atoi(e) : 0;
    return (v == 1 || v == 4 || v == 16) ? v : kDefaultWaves;
  }();
  return w;
}

}  // namespace jb

extern "C" int jb_linear_train_chunked(const int64_t* row_ptr, const int32_t* fidx,
                                       const float* fval, const int32_t* labels,
                                       const int64_t* stream_ptr, int nstreams, void* W,
                                       int w_bf16, float* P, const int32_t* active, int LC,
                                       int method, float C, int mode, int waves,
                                       unsigned long long* stats, uint8_t* touched,
                                       hipStream_t stream) {
  if (!jb::chunked_lc_ok(LC)) return -1;
  if (waves == 0) waves = jb::label_waves();
  if (waves != 1 && waves != 4 && waves != 16) return -2;
  if (mode != jb::kExact && mode != jb::kAtomic && mode != jb::kHogwild) return -5;
  if (mode == jb::kExact && nstreams > 1) return -5;
  if (W == nullptr || active == nullptr || (method >= jb::CW && P == nullptr)) return -4;
  if (method < jb::PERCEPTRON || method > jb::NHERD) return -6;
  if (nstreams <= 0) return 0;
  if (w_bf16)
    hipLaunchKernelGGL((jb::linear_train_chunked_kernel<jb::bf16_t>), dim3(nstreams),
                       dim3(64 * waves), 0, stream, row_ptr, fidx, fval, labels, stream_ptr,
                       nstreams, (jb::bf16_t*)W, P, active, LC, method, C, mode, stats, touched);
  else
    hipLaunchKernelGGL((jb::linear_train_chunked_kernel<float>), dim3(nstreams), dim3(64 * waves),
                       0, stream, row_ptr, fidx, fval, labels, stream_ptr, nstreams, (float*)W, P,
                       active, LC, method, C, mode, stats, touched);
  return (int)hipGetLastError();
}

extern "C" int jb_linear_classify_chunked(const int64_t* row_ptr, const int32_t* fidx,
                                          const float* fval, int n_samples, const void* W,
                                          int w_bf16, int LC, float* out, hipStream_t stream) {
  if (!jb::chunked_lc_ok(LC)) return -1;
  if (W == nullptr || out == nullptr) return -4;
  if (n_samples <= 0) return 0;
  const int64_t waves = (int64_t)n_samples * (LC / jb::kChunk);
  const int64_t blocks = (waves + 3) / 4;
  if (blocks > INT32_MAX) return -2;
  if (w_bf16)
    hipLaunchKernelGGL((jb::linear_classify_chunked_kernel<jb::bf16_t>), dim3((unsigned)blocks),
                       dim3(256), 0, stream, row_ptr, fidx, fval, n_samples,
                       (const jb::bf16_t*)W, LC, out);
  else
    hipLaunchKernelGGL((jb::linear_classify_chunked_kernel<float>), dim3((unsigned)blocks),
                       dim3(256), 0, stream, row_ptr, fidx, fval, n_samples, (const float*)W, LC,
                       out);
  return (int)hipGetLastError();
}
