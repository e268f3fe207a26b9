// Exact top-k for neighbour lists of 129 to 4096 entries (kTopWideMaxK), the
// range past topk.hip's register / LDS lists. Same sources (jb_topk_src.hpp:
// the fused signature scan, or a [nq][nrows] score matrix), same result
// contract as jb_topk: out_d / out_i [nq][k] ascending by (distance, row),
// ties to the lower row, absent rows never returned, (+inf, INT_MAX) padding.
//
// A list this long does not fit a wave's registers, so nothing is kept per
// block: a radix select finds the k-th key, and one more pass emits exactly
// the k rows at or below it.
//
//   key    32 bits per row. lsh / minhash: the hamming count (<= 1024, one
//          11-bit digit). euclid_lsh / scores: the fp32 distance's bits made
//          order-preserving (sign flip; -0 canonicalised to +0), three digits
//          of 11 + 11 + 10 bits. (key << 32 | row) is distinct per row.
//   W0     wide_init_kernel zeroes the query's histograms and state words.
//   W1     wide_hist_kernel, grid (blocks, nq), once per digit: block b owns a
//          contiguous row range (a multiple of the 2048-row tile: block order
//          is row order), computes the distances of its rows (8 a thread,
//          load_rows), bins the digit of the rows that match the digits chosen
//          so far into an LDS histogram - the wave first folds equal digits
//          with ballots, quantised distances put whole waves into one bin -
//          and adds its non-empty bins to the query's global histogram
//          (integer atomics: order-independent). The block with the last
//          ticket scans the 2048 bins and writes the digit where the running
//          count reaches the rows still wanted, and what remains.
//   W2     wide_tie_kernel, only when fewer rows are wanted at the threshold
//          key T than are equal to it (r < eq): per-block counts of the rows
//          equal to T; the last block finds the block b* holding the r-th one
//          and how many b* may emit. With r == eq (the rule for continuous
//          distances) every block returns at once.
//   W3     wide_collect_kernel: every row with key < T, and the permitted ones
//          with key == T - all in blocks before b*, the first few in row order
//          inside b* (a block scan per register slot), none after - into the
//          query's k composites through one wave-aggregated counter. Exactly
//          min(k, qualifying) arrive: no overflow, no retry.
//   W4     wide_sort_kernel, one workgroup a query: bitonic sort of the
//          composites in LDS (4096 x 8 B), then distance and row. A float key
//          is the distance's own bits; a hamming key gives ham / hash_num, the
//          expression of load_item.
//
// No host synchronisation, no nq x N intermediate in mode 0, and two launches
// on the same inputs give the same bits (integer histograms, a sort of
// distinct composites).
#include <limits.h>

#include "jb_hip_api.h"
#include "jb_topk_src.hpp"

namespace jb {
namespace tkw {

constexpr int kTopWideMaxK = 4096;
constexpr int kBins = 2048;                  // bins of one digit's histogram
constexpr int kLevels = 3;                   // digits of a float key
constexpr int kMaxBlocks = 512;              // two blocks a CU; <= 2 per thread in W2's scan
constexpr int kSortThreads = 1024;
constexpr int kPeel = 4;                     // rounds of wave-level folding before plain LDS atomics
constexpr uint32_t kAbsent = 0xffffffffu;    // key of an invalid / out-of-range row; above every real key

// state words of a query
enum { kPrefix = 0,   // the digits chosen so far; after the last level the threshold key T
       kRemain,       // rows still wanted among those matching the prefix; finally r
       kTie,          // 0: every row equal to T is emitted (r == eq), 1: b* / take decide, 2: fewer than k qualify
       kAll,          // fewer than k rows qualify: every valid row is emitted
       kBstar, kTake, kCount,
       kTicket,       // + level (0..2), + 3 for W2
       kStateWords = 16 };

struct Scratch {
  uint64_t* comp;     // [nq][k]
  uint32_t* hist;     // [nq][kLevels][kBins]
  uint32_t* state;    // [nq][kStateWords]
  uint32_t* blk;      // [nq][kMaxBlocks]
};

__device__ __forceinline__ uint32_t key_of(float d, int ham, float hn) {
  if (!(d < INFINITY)) return kAbsent;       // invalid, out of range, NaN
  if (ham) return (uint32_t)(int)rintf(d * hn);
  uint32_t b = __float_as_uint(d);
  if (b == 0x80000000u) b = 0u;              // -0 sorts with +0
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float dist_of(uint32_t key, int ham, int hash_num) {
  if (ham) return (float)(int)key / (float)hash_num;
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__device__ __forceinline__ uint32_t load_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// exclusive scan of v over the block's kTopThreads threads (in thread order)
// and the block's total; s_w: 4 words of LDS. Called by all threads.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* s_w, int t, uint32_t* total) {
  const int lane = t & 63, wv = t >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t x = __shfl_up(incl, o, 64);
    if (lane >= o) incl += x;
  }
  if (lane == 63) s_w[wv] = incl;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kTopThreads / 64; ++w) {
    const uint32_t x = s_w[w];
    base += w < wv ? x : 0u;
    tot += x;
  }
  __syncthreads();                           // s_w may be written again
  *total = tot;
  return base + incl - v;
}

// the first of a thread's N consecutive counts at which the running count
// (`before` ahead of them) reaches `want`; the caller knows one of them does
struct Pick {
  int at;
  uint32_t before, count;
};

template <int N>
__device__ __forceinline__ Pick pick(const uint32_t (&c)[N], uint32_t before, uint32_t want) {
  Pick p{-1, 0u, 0u};
  uint32_t run = before;
#pragma unroll
  for (int i = 0; i < N; ++i) {               // unrolled: c stays in registers
    if (p.at < 0 && run + c[i] >= want) p = Pick{i, run, c[i]};
    run += c[i];
  }
  return p;
}

// the query's signature into LDS (read from there by load_rows: a broadcast)
// and, for euclid_lsh, the cos table of topk_kernel (the same expression)
template <int MODE>
__device__ __forceinline__ const float* query_setup(const TopkSrc& s, int q, int t, uint64_t* s_q,
                                                    float* s_cos, float* qn) {
  const float* ctab = nullptr;
  *qn = 0.f;
  if (MODE == 0) {
    for (int w = t; w < s.words; w += kTopThreads) s_q[w] = s.qbits[(int64_t)q * s.words + w];
    *qn = s.qnorm[q];
    if (s.metric == 1) {
      for (int h = t; h <= s.hash_num; h += kTopThreads)
        s_cos[h] = __cosf(3.14159265f * ((float)h / (float)s.hash_num));
      ctab = s_cos;
    }
  }
  __syncthreads();
  return ctab;
}

// keys and row indices of the thread's 8 rows of the tile at `base` (rows at
// and past b1 are absent)
template <int MODE>
__device__ __forceinline__ void tile_keys(const TopkSrc& s, int q, int64_t n, int64_t base, int64_t b1,
                                          int t, const uint64_t* qb, float qn, const float* ctab,
                                          int ham, uint32_t (&key)[kTopR], int (&ix)[kTopR]) {
  int64_t rows[kTopR], nn[kTopR];
  float d[kTopR];
#pragma unroll
  for (int r = 0; r < kTopR; ++r) {
    rows[r] = base + (int64_t)r * kTopThreads + t;
    nn[r] = rows[r] < b1 ? n : 0;
  }
  load_rows<MODE, kTopR>(s, q, nn, rows, qb, qn, d, ix, ctab);
  const float hn = (float)s.hash_num;
#pragma unroll
  for (int r = 0; r < kTopR; ++r) key[r] = key_of(d[r], ham, hn);
}

// one count into the LDS histogram per lane that is `on`. Up to kPeel rounds
// fold the lanes that share the first active lane's digit into one add; what
// is still on after that (many distinct digits) adds by itself.
__device__ __forceinline__ void lds_bin(uint32_t* h, bool on, uint32_t digit, int lane) {
  for (int it = 0; it < kPeel; ++it) {
    const uint64_t act = __ballot(on);
    if (act == 0) return;                    // wave-uniform
    const int lead = __ffsll((long long)act) - 1;
    const uint32_t dg = (uint32_t)__shfl((int)digit, lead, 64);
    const bool same = on && digit == dg;
    const uint64_t m = __ballot(same);
    if (lane == lead) atomicAdd(&h[dg], (uint32_t)__popcll(m));
    on = on && !same;
  }
  if (on) atomicAdd(&h[digit], 1u);
}

__global__ __launch_bounds__(256) void wide_init_kernel(int k, uint32_t* __restrict__ hist,
                                                        uint32_t* __restrict__ state) {
  const int q = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < kLevels * kBins) hist[(int64_t)q * kLevels * kBins + j] = 0u;
  if (j < kStateWords) state[(int64_t)q * kStateWords + j] = j == kRemain ? (uint32_t)k : 0u;
}

// takes the block's ticket; true in every thread of the last block of the grid
__device__ __forceinline__ bool last_block(uint32_t* ticket, int* s_last, int t) {
  __threadfence();                           // release: this thread's atomics / stores
  __syncthreads();
  if (t == 0) *s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!*s_last) return false;
  __threadfence();                           // acquire: every other block has taken its ticket
  return true;
}

template <int MODE>
__global__ __launch_bounds__(kTopThreads) void wide_hist_kernel(const TopkSrc s, int64_t n,
                                                                int64_t per_block, int ham, int level,
                                                                int last_level,
                                                                uint32_t* __restrict__ hist,
                                                                uint32_t* __restrict__ state) {
  __shared__ uint32_t s_h[kBins];
  __shared__ uint64_t s_q[kTopMaxWords];
  __shared__ float s_cos[MODE == 0 ? kTopMaxWords * 64 + 1 : 1];
  __shared__ uint32_t s_w[kTopThreads / 64];
  __shared__ int s_last;
  const int q = blockIdx.y, t = threadIdx.x, lane = t & 63;
  uint32_t* st = state + (int64_t)q * kStateWords;
  uint32_t* gh = hist + ((int64_t)q * kLevels + level) * kBins;
  if (level > 0 && st[kAll] != 0u) return;   // block-uniform; written by level 0's last block
  const uint32_t prefix = st[kPrefix];
  // this level's digit, and the bits above it that must match the prefix
  const int shift = ham ? 0 : (level == 0 ? 21 : level == 1 ? 10 : 0);
  const uint32_t mask = (ham || level < 2) ? 2047u : 1023u;
  const int hs = level == 1 ? 21 : 10;       // (level 0 filters nothing)
  for (int b = t; b < kBins; b += kTopThreads) s_h[b] = 0u;
  float qn;
  const float* ctab = query_setup<MODE>(s, q, t, s_q, s_cos, &qn);
  const int64_t b0 = (int64_t)blockIdx.x * per_block;
  const int64_t b1 = b0 + per_block < n ? b0 + per_block : n;
  for (int64_t base = b0; base < b1; base += kTopTile) {
    uint32_t key[kTopR];
    int ix[kTopR];
    tile_keys<MODE>(s, q, n, base, b1, t, s_q, qn, ctab, ham, key, ix);
#pragma unroll
    for (int r = 0; r < kTopR; ++r) {
      const bool on = key[r] != kAbsent && (level == 0 || (key[r] >> hs) == (prefix >> hs));
      lds_bin(s_h, on, (key[r] >> shift) & mask, lane);
    }
  }
  __syncthreads();
  for (int b = t; b < kBins; b += kTopThreads) {
    const uint32_t c = s_h[b];
    if (c != 0u) atomicAdd(&gh[b], c);
  }
  if (!last_block(&st[kTicket + level], &s_last, t)) return;
  // the last block: the bin where the running count reaches the rows wanted
  constexpr int PER = kBins / kTopThreads;
  const uint32_t remain = st[kRemain];
  uint32_t c[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    c[i] = load_agent(&gh[t * PER + i]);
    sum += c[i];
  }
  uint32_t total;
  const uint32_t excl = block_scan(sum, s_w, t, &total);
  if (excl < remain && remain <= excl + sum) {      // one thread
    const Pick p = pick<PER>(c, excl, remain);
    st[kPrefix] = prefix | ((uint32_t)(t * PER + p.at) << shift);
    st[kRemain] = remain - p.before;
    if (last_level) st[kTie] = remain - p.before == p.count ? 0u : 1u;
  }
  if (t == 0 && total < remain) {                   // level 0 only: fewer than k rows qualify
    st[kAll] = 1u;
    st[kPrefix] = kAbsent;
    st[kTie] = 2u;
  }
}

template <int MODE>
__global__ __launch_bounds__(kTopThreads) void wide_tie_kernel(const TopkSrc s, int64_t n,
                                                               int64_t per_block, int ham,
                                                               uint32_t* __restrict__ state,
                                                               uint32_t* __restrict__ blk) {
  __shared__ uint64_t s_q[kTopMaxWords];
  __shared__ float s_cos[MODE == 0 ? kTopMaxWords * 64 + 1 : 1];
  __shared__ uint32_t s_w[kTopThreads / 64];
  __shared__ int s_last;
  const int q = blockIdx.y, t = threadIdx.x;
  uint32_t* st = state + (int64_t)q * kStateWords;
  uint32_t* qblk = blk + (int64_t)q * kMaxBlocks;
  if (st[kTie] != 1u) return;                // block-uniform: no choice among the ties
  const uint32_t T = st[kPrefix];
  float qn;
  const float* ctab = query_setup<MODE>(s, q, t, s_q, s_cos, &qn);
  const int64_t b0 = (int64_t)blockIdx.x * per_block;
  const int64_t b1 = b0 + per_block < n ? b0 + per_block : n;
  uint32_t mine = 0;
  for (int64_t base = b0; base < b1; base += kTopTile) {
    uint32_t key[kTopR];
    int ix[kTopR];
    tile_keys<MODE>(s, q, n, base, b1, t, s_q, qn, ctab, ham, key, ix);
#pragma unroll
    for (int r = 0; r < kTopR; ++r) mine += key[r] == T ? 1u : 0u;
  }
  uint32_t total;
  block_scan(mine, s_w, t, &total);
  if (t == 0) qblk[blockIdx.x] = total;
  if (!last_block(&st[kTicket + kLevels], &s_last, t)) return;
  // the last block: b* holds the r-th row equal to T, in block (= row) order
  constexpr int PER = kMaxBlocks / kTopThreads;
  const uint32_t r = st[kRemain];
  uint32_t c[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int b = t * PER + i;
    c[i] = b < (int)gridDim.x ? load_agent(&qblk[b]) : 0u;
    sum += c[i];
  }
  const uint32_t excl = block_scan(sum, s_w, t, &total);
  if (excl < r && r <= excl + sum) {                // one thread (r <= eq = total)
    const Pick p = pick<PER>(c, excl, r);
    st[kBstar] = (uint32_t)(t * PER + p.at);
    st[kTake] = r - p.before;
  }
}

template <int MODE>
__global__ __launch_bounds__(kTopThreads) void wide_collect_kernel(const TopkSrc s, int64_t n,
                                                                   int64_t per_block, int k, int ham,
                                                                   uint32_t* __restrict__ state,
                                                                   uint64_t* __restrict__ comp) {
  __shared__ uint64_t s_q[kTopMaxWords];
  __shared__ float s_cos[MODE == 0 ? kTopMaxWords * 64 + 1 : 1];
  __shared__ uint32_t s_w[kTopThreads / 64];
  const int q = blockIdx.y, t = threadIdx.x, lane = t & 63;
  uint32_t* st = state + (int64_t)q * kStateWords;
  uint64_t* qcomp = comp + (int64_t)q * k;
  const uint32_t T = st[kPrefix], tie = st[kTie], bstar = st[kBstar], take = st[kTake];
  // rows equal to T: all of them (no choice, or a block before b*), or inside
  // b* the first `take` in row order; block-uniform
  const bool eq_all = tie == 0u || (tie == 1u && blockIdx.x < bstar);
  const bool ordered = tie == 1u && blockIdx.x == bstar;
  uint32_t seen = 0;                          // rows equal to T in the tiles before this one
  float qn;
  const float* ctab = query_setup<MODE>(s, q, t, s_q, s_cos, &qn);
  const int64_t b0 = (int64_t)blockIdx.x * per_block;
  const int64_t b1 = b0 + per_block < n ? b0 + per_block : n;
  for (int64_t base = b0; base < b1; base += kTopTile) {
    uint32_t key[kTopR];
    int ix[kTopR];
    tile_keys<MODE>(s, q, n, base, b1, t, s_q, qn, ctab, ham, key, ix);
    bool emit[kTopR];
#pragma unroll
    for (int r = 0; r < kTopR; ++r) emit[r] = key[r] < T || (eq_all && key[r] == T);
    if (ordered) {
      // row order inside a tile is (register slot, thread)
#pragma unroll
      for (int r = 0; r < kTopR; ++r) {
        const bool eq = key[r] == T;
        uint32_t total;
        const uint32_t before = seen + block_scan(eq ? 1u : 0u, s_w, t, &total);
        emit[r] = emit[r] || (eq && before < take);
        seen += total;
      }
    }
    uint64_t m[kTopR];
    int total = 0;
#pragma unroll
    for (int r = 0; r < kTopR; ++r) {
      m[r] = __ballot(emit[r]);
      total += __popcll(m[r]);
    }
    if (total == 0) continue;                 // wave-uniform: the common case on a large table
    uint32_t at = 0;
    if (lane == 0) at = atomicAdd(&st[kCount], (uint32_t)total);
    at = (uint32_t)__shfl((int)at, 0, 64);
#pragma unroll
    for (int r = 0; r < kTopR; ++r) {
      if (emit[r]) {
        const uint32_t pos = at + __builtin_amdgcn_mbcnt_hi((uint32_t)(m[r] >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)m[r], 0u));
        if (pos < (uint32_t)k) qcomp[pos] = ((uint64_t)key[r] << 32) | (uint32_t)ix[r];
      }
      at += (uint32_t)__popcll(m[r]);
    }
  }
}

__global__ __launch_bounds__(kSortThreads) void wide_sort_kernel(int k, int ham, int hash_num,
                                                                 const uint32_t* __restrict__ state,
                                                                 const uint64_t* __restrict__ comp,
                                                                 float* __restrict__ out_d,
                                                                 int32_t* __restrict__ out_i) {
  __shared__ uint64_t s_c[kTopWideMaxK];
  const int q = blockIdx.x, t = threadIdx.x;
  const uint32_t have = state[(int64_t)q * kStateWords + kCount];
  const int cnt = have < (uint32_t)k ? (int)have : k;
  int P = 2;                                  // the sort's size: a power of two >= k
  while (P < k) P <<= 1;
  for (int j = t; j < P; j += kSortThreads) s_c[j] = j < cnt ? comp[(int64_t)q * k + j] : ~0ull;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = t; i < P / 2; i += kSortThreads) {
        const int lo = 2 * i - (i & (stride - 1));
        const int hi = lo + stride;
        const uint64_t a = s_c[lo], b = s_c[hi];
        const bool up = (lo & size) == 0;
        if ((a > b) == up) { s_c[lo] = b; s_c[hi] = a; }
      }
      __syncthreads();
    }
  }
  // the real composites are below the ~0 fill: the first cnt entries
  for (int j = t; j < k; j += kSortThreads) {
    const uint64_t v = s_c[j];
    out_d[(int64_t)q * k + j] = j < cnt ? dist_of((uint32_t)(v >> 32), ham, hash_num) : INFINITY;
    out_i[(int64_t)q * k + j] = j < cnt ? (int32_t)(uint32_t)v : INT_MAX;
  }
}

}  // namespace tkw
}  // namespace jb

namespace {

using namespace jb::tkw;

// blocks of the scan grid and the rows of one block (a multiple of the tile):
// one tile a block up to kMaxBlocks blocks
struct Geo {
  int blocks;
  int64_t per_block;
};

Geo geo(int64_t nrows) {
  const int64_t tiles = (nrows + jb::kTopTile - 1) / jb::kTopTile;
  const int64_t tpb = (tiles + kMaxBlocks - 1) / kMaxBlocks;
  return {(int)((tiles + tpb - 1) / tpb), tpb * jb::kTopTile};
}

int64_t per_query_bytes(int k) {
  return (int64_t)k * 8 + ((int64_t)kLevels * kBins + kStateWords + kMaxBlocks) * 4;
}

Scratch carve(void* p, int nq, int k) {
  Scratch sc;
  sc.comp = static_cast<uint64_t*>(p);
  sc.hist = reinterpret_cast<uint32_t*>(sc.comp + (int64_t)nq * k);
  sc.state = sc.hist + (int64_t)nq * kLevels * kBins;
  sc.blk = sc.state + (int64_t)nq * kStateWords;
  return sc;
}

template <int MODE>
int chain(const jb::TopkSrc& s, int nq, int64_t nrows, int k, int ham, const Scratch& sc, float* out_d,
          int32_t* out_i, hipStream_t stream) {
  const Geo g = geo(nrows);
  const dim3 grid((unsigned)g.blocks, (unsigned)nq), block(jb::kTopThreads);
  hipLaunchKernelGGL(wide_init_kernel, dim3((kLevels * kBins + 255) / 256, (unsigned)nq), dim3(256), 0,
                     stream, k, sc.hist, sc.state);
  const int levels = ham ? 1 : kLevels;
  for (int level = 0; level < levels; ++level)
    hipLaunchKernelGGL(wide_hist_kernel<MODE>, grid, block, 0, stream, s, nrows, g.per_block, ham, level,
                       level == levels - 1 ? 1 : 0, sc.hist, sc.state);
  hipLaunchKernelGGL(wide_tie_kernel<MODE>, grid, block, 0, stream, s, nrows, g.per_block, ham, sc.state,
                     sc.blk);
  hipLaunchKernelGGL(wide_collect_kernel<MODE>, grid, block, 0, stream, s, nrows, g.per_block, k, ham,
                     sc.state, sc.comp);
  hipLaunchKernelGGL(wide_sort_kernel, dim3((unsigned)nq), dim3(kSortThreads), 0, stream, k, ham,
                     s.hash_num, sc.state, sc.comp, out_d, out_i);
  return (int)hipGetLastError();
}

}  // namespace

// bytes of device scratch a jb_topk_wide call of this shape needs (8-byte
// aligned; its contents need no preparation: the chain zeroes what it counts in)
extern "C" int64_t jb_topk_wide_scratch_bytes(int nq, int64_t nrows, int k) {
  if (nq <= 0 || nrows <= 0 || k <= 0 || k > kTopWideMaxK) return 0;
  return (int64_t)nq * per_query_bytes(k);
}

// jb_topk for k up to 4096 (operands as jb_topk's; one scratch of
// jb_topk_wide_scratch_bytes). nq <= 65535 a call, nrows < 2^31.
extern "C" int jb_topk_wide(int mode, const uint64_t* qbits, const float* qnorm, int nq,
                            const uint64_t* tbits, const float* tnorm, const uint8_t* valid,
                            int64_t nrows, int words, int hash_num, int metric, const float* src_d,
                            int flip, int k, void* scratch, float* out_d, int32_t* out_i,
                            hipStream_t stream) {
  if (nq <= 0 || nrows <= 0 || k <= 0) return 0;
  if (k > kTopWideMaxK || nq > 65535 || nrows > (int64_t)INT_MAX || (mode != 0 && mode != 1)) return -2;
  if (mode == 0 && (words <= 0 || words > jb::kTopMaxWords || hash_num <= 0 || hash_num > 64 * words)) return -2;
  const jb::TopkSrc s{qbits, qnorm, tbits, tnorm, valid, words, hash_num, metric, src_d, nullptr, flip};
  const Scratch sc = carve(scratch, nq, k);
  const int ham = (mode == 0 && metric != 1) ? 1 : 0;
  return mode == 0 ? chain<0>(s, nq, nrows, k, ham, sc, out_d, out_i, stream)
                   : chain<1>(s, nq, nrows, k, ham, sc, out_d, out_i, stream);
}
