// The row source of the top-k kernels (topk.hip for k <= 128, topk_wide.hip
// past it): where a query's distances come from and the one set of
// expressions that computes them, so every path returns the same bits.
#pragma once

#include <limits.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace jb {

constexpr int kTopThreads = 256;
constexpr int kTopR = 8;                          // rows per thread per tile
constexpr int kTopTile = kTopThreads * kTopR;     // 2048
constexpr int kTopMaxWords = 16;                  // hash_num <= 1024

struct TopkSrc {
  // MODE 0: fused signature scan
  const uint64_t* qbits;
  const float* qnorm;
  const uint64_t* tbits;
  const float* tnorm;
  const uint8_t* valid;
  int words, hash_num, metric;
  // MODE 1: score vector [nq][n] (flip: distance = 1 - score)
  // MODE 2: candidate pairs [nq][n]
  const float* src_d;
  const int32_t* src_i;
  int flip;
};

// The distance of row r (n: rows of the source, 0 = r is out of range).
// Branch-free: an out-of-range row loads row 0 and is masked afterwards, and
// the norm's address is selected rather than branched on, so the loads of a
// thread's R rows sit in one basic block and issue back to back (a branch per
// row made the compiler drain vmcnt after every load: R serial HBM round
// trips per tile).
template <int MODE>
__device__ __forceinline__ void load_item(const TopkSrc& s, int q, int64_t n, int64_t r,
                                          const uint64_t* qb, float qn, float& d, int& id) {
  const bool in = r < n;
  const int64_t rr = in ? r : 0;
  if (MODE == 0) {
    const int64_t w0 = rr * s.words;
    const uint8_t ok = s.valid[rr];
    // metric 1 reads the norm; the others read (and ignore) 4 bytes of the
    // row's own signature, which always exist
    const float* np = s.metric == 1 ? s.tnorm + rr : reinterpret_cast<const float*>(s.tbits + w0);
    const float braw = *np;
    int ham = __popcll(qb[0] ^ s.tbits[w0]);
    if (s.words > 1) {
#pragma unroll
      for (int w = 1; w < kTopMaxWords; ++w)
        if (w < s.words) ham += __popcll(qb[w] ^ s.tbits[w0 + w]);
    }
    const float b = s.metric == 1 ? braw : 0.f;
    const float frac = (float)ham / (float)s.hash_num;
    if (s.metric == 1)
      d = sqrtf(fmaxf(0.f, qn * qn + b * b - 2.f * qn * b * __cosf(3.14159265f * frac)));
    else
      d = frac;
    if (!ok) d = INFINITY;
  } else if (MODE == 1) {
    const float v = s.src_d[(int64_t)q * n + rr];
    d = s.flip ? 1.f - v : v;
    if (!(d < INFINITY) || d != d) d = INFINITY;   // -inf scores / NaN -> absent
  } else {
    d = s.src_d[(int64_t)q * n + rr];
    id = s.src_i[(int64_t)q * n + rr];
  }
  if (MODE != 2) id = (int)r;
  if (!in) { d = INFINITY; id = INT_MAX; }
}

// R rows at once (nn[u]: n for row u, 0 = out of range). MODE 0 in phases -
// every row's valid byte, norm and first signature word, then (tables wider
// than 64 bits only) the other words, then the distances - so the first
// phase's loads are one basic block and all R rows are in flight together
template <int MODE, int R>
__device__ __forceinline__ void load_rows(const TopkSrc& s, int q, const int64_t (&nn)[R],
                                          const int64_t (&r)[R], const uint64_t* qb, float qn,
                                          float (&d)[R], int (&id)[R], const float* ctab = nullptr) {
  if (MODE != 0) {
#pragma unroll
    for (int u = 0; u < R; ++u) load_item<MODE>(s, q, nn[u], r[u], qb, qn, d[u], id[u]);
    return;
  }
  int64_t w0[R];
  uint8_t ok[R];
  float braw[R];
  uint64_t b0[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const int64_t rr = r[u] < nn[u] ? r[u] : 0;
    w0[u] = rr * s.words;
    ok[u] = s.valid[rr];
    const float* np = s.metric == 1 ? s.tnorm + rr : reinterpret_cast<const float*>(s.tbits + w0[u]);
    braw[u] = *np;
    b0[u] = s.tbits[w0[u]];
  }
  int ham[R];
#pragma unroll
  for (int u = 0; u < R; ++u) ham[u] = __popcll(qb[0] ^ b0[u]);
  if (s.words > 1) {
#pragma unroll
    for (int u = 0; u < R; ++u)
      for (int w = 1; w < s.words; ++w) ham[u] += __popcll(qb[w] ^ s.tbits[w0[u] + w]);
  }
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const float frac = (float)ham[u] / (float)s.hash_num;
    float v;
    if (s.metric == 1) {
      // ctab[h] = the same cos expression per hamming distance (bit-identical)
      const float c = ctab != nullptr ? ctab[ham[u]] : __cosf(3.14159265f * frac);
      v = sqrtf(fmaxf(0.f, qn * qn + braw[u] * braw[u] - 2.f * qn * braw[u] * c));
    } else {
      v = frac;
    }
    const bool in = r[u] < nn[u];
    d[u] = (in && ok[u]) ? v : INFINITY;
    id[u] = in ? (int)r[u] : INT_MAX;
  }
}

}  // namespace jb
