// Many-query scan of the device inverted index: up to 64 queries scored in
// ONE pass over the row pool (sparse_pool.hip scores 8; a batch of 256 reads
// the pool 32 times there and 4 times here). Storage, query CSR, scores and
// their [nq][nrows] layout are those of sparse_pool.hip.
//
// Work split: one lane per (row, query). QM = 16 / 32 / 64 query lanes per
// row, so a wave holds 64 / QM rows: lane l owns row-group l / QM and query
// l % QM, and the fp64 dot product of that pair lives in that one lane from
// the row's first entry to the score. No cross-lane reduction, no DPP.
// One workgroup of 1024 threads per CU (the table fills most of LDS; 16 waves
// keep four per SIMD to hide the pool loads) loops over tiles of R = 1024 / QM
// rows; the next tile's row metadata is loaded while this tile is scored.
//
// LDS (dynamic, up to 160 KiB; wide_lds() is the one place that sizes it):
//   qn2[QM] fp64 | keys[T] int32 (-1 = empty) | uid[T] int32 (0 = not yet
//   published, 1 + unique id, -1 = dropped) | vals[U][QM] fp32 | two score
//   tiles [QM][R + 1] fp32 | the unique counter
// U = the pass's DISTINCT features (not its entries), T = power of two >= 2 U.
// Lane (row, q) reads vals[u][q]: the QM lanes of a row read consecutive
// banks. A lane would store its score to out[q * nrows + r], stride nrows
// across the wave; the tile turns that around: written from registers, then
// stored with the lanes running along r. Two tiles, so that a step costs one
// barrier (a tile is rewritten two barriers after it was read).
//
// Table build, by every workgroup: atomicCAS insert of the feature, the winner
// publishes its unique id, one atomicAdd of the value into vals[uid][q]. The
// host merged repeated features (csr_normalize), so every cell gets exactly
// one add onto 0 and the table is deterministic. An insert whose id would
// reach U, or that finds no free key after T probes, is dropped: whatever
// the host passed, nothing is written outside the table.
//
// Row walk, per step and row: the QM lanes load QM consecutive entries
// (clamped, unpredicated), each probes the table once, a ballot gives the
// hits, and for every hit in ASCENDING ENTRY ORDER (uid, value) is broadcast
// from its lane - v_readlane with a scalar index when the row is the whole
// wave (QM = 64), ds_bpermute inside the row's lanes otherwise - and every
// lane does dot += (double)value * (double)vals[uid][q].
//
// Arithmetic: the product of two floats is exact in fp64 and the sum runs in
// entry order, so a pair's dot product - and with jb_pool.hpp's epilogue its
// score - is bit-identical to pool_rows_kernel<*, 1> (one lane per row).
//
// No MFMA: the operands are two sparse vectors that meet in a hash table.
// Densifying row tiles for v_mfma_f64_16x16x4_f64 would multiply mostly
// zeros and lose the entry-order sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jb_hip_api.h"
#include "jb_pool.hpp"

namespace jb {

constexpr int kWideThreads = 1024;
constexpr int kWideMaxQ = 64;
constexpr size_t kWideLdsCap = 160 * 1024;
constexpr int kWideMaxUniq = 1 << 16;     // far past what the LDS holds; keeps the sizes in int

struct WideMeta {
  int64_t off;
  double n2;
  int32_t len;
  uint8_t vld;
};

__device__ __forceinline__ WideMeta wide_meta(int64_t r, int64_t nrows,
                                              const int64_t* __restrict__ r_off,
                                              const int32_t* __restrict__ r_len,
                                              const double* __restrict__ r_n2,
                                              const uint8_t* __restrict__ valid) {
  const int64_t rc = r < nrows ? r : nrows - 1;      // unpredicated loads of a clamped row
  return WideMeta{r_off[rc], r_n2[rc], r_len[rc], valid[rc]};
}

template <int QM>
__global__ __launch_bounds__(kWideThreads) void pool_rows_wide_kernel(
    DevQuery qs, int nq, int U, int tbits, const int64_t* __restrict__ r_off,
    const int32_t* __restrict__ r_len, const double* __restrict__ r_n2,
    const uint8_t* __restrict__ valid, int64_t nrows, const int32_t* __restrict__ p_idx,
    const float* __restrict__ p_val, int metric, float* __restrict__ out) {
  constexpr int G = 64 / QM;                  // rows of a wave
  constexpr int R = (kWideThreads / 64) * G;  // rows of a workgroup step
  constexpr int TS = R + 1;
  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
  const int T = 1 << tbits;
  double* s_qn2 = reinterpret_cast<double*>(s_dyn);
  int32_t* s_key = reinterpret_cast<int32_t*>(s_qn2 + QM);
  int32_t* s_uid = s_key + T;
  float* s_vals = reinterpret_cast<float*>(s_uid + T);
  float* s_tile = s_vals + (size_t)U * QM;
  int* s_cnt = reinterpret_cast<int*>(s_tile + 2 * QM * TS);

  for (int i = threadIdx.x; i < T; i += kWideThreads) { s_key[i] = -1; s_uid[i] = 0; }
  for (int i = threadIdx.x; i < U * QM; i += kWideThreads) s_vals[i] = 0.f;
  if (threadIdx.x < QM) s_qn2[threadIdx.x] = (int)threadIdx.x < nq ? qs.norm2(threadIdx.x) : 0.0;
  if (threadIdx.x == 0) *s_cnt = 0;
  __syncthreads();
  // table build: one thread per query entry
  const int64_t e1 = qs.end(nq - 1);
  for (int64_t e = qs.base() + threadIdx.x; e < e1; e += kWideThreads) {
    int q = 0, hi = nq - 1;       // the last query that starts at or before e: the one holding it
    while (q < hi) {
      const int mid = (q + hi + 1) >> 1;
      if (qs.start(mid) <= e) q = mid; else hi = mid - 1;
    }
    const int32_t f = qs.f(e);
    const float v = qs.v(e);
    uint32_t h = pool_hash(f) >> (32 - tbits);
    bool found = false;
    for (int probe = 0; probe < T; ++probe) {
      const int32_t old = atomicCAS(&s_key[h], -1, f);
      if (old == -1) {
        const int id = atomicAdd(s_cnt, 1);
        __atomic_store_n(&s_uid[h], id < U ? id + 1 : -1, __ATOMIC_RELAXED);
      }
      if (old == -1 || old == f) { found = true; break; }
      h = (h + 1) & (T - 1);
    }
    if (!found) continue;
    int u;
    while ((u = __atomic_load_n(&s_uid[h], __ATOMIC_RELAXED)) == 0) {}
    if (u > 0) atomicAdd(&s_vals[(u - 1) * QM + q], v);
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int g = lane / QM, q = lane % QM;
  const int rl = (threadIdx.x >> 6) * G + g;      // this lane's row within the tile
  const double qn = s_qn2[q];
  const int64_t stride = (int64_t)gridDim.x * R;
  int64_t base = (int64_t)blockIdx.x * R;
  WideMeta m = wide_meta(base + rl, nrows, r_off, r_len, r_n2, valid);
  for (int par = 0; base < nrows; base += stride, par ^= 1) {
    const int64_t r = base + rl;
    const WideMeta nx = wide_meta(r + stride, nrows, r_off, r_len, r_n2, valid);
    const bool live = r < nrows && m.vld;
    const int len = live ? m.len : 0;
    double dot = 0.0;
    for (int j0 = 0; __any(j0 < len); j0 += QM) {
      const int j = j0 + q;
      const int jc = j < len ? j : len - 1;
      const int64_t src = len > 0 ? m.off + jc : 0;     // (an empty row reads entry 0 and drops it)
      const int32_t f = p_idx[src];
      const float v = p_val[src];
      int u = -1;
      if (j < len) {
        uint32_t h = pool_hash(f) >> (32 - tbits);
        for (int probe = 0; probe < T; ++probe) {
          const int32_t key = s_key[h];
          if (key == f) { u = s_uid[h] - 1; break; }
          if (key == -1) break;
          h = (h + 1) & (T - 1);
        }
      }
      uint64_t hits = __ballot(u >= 0);
      if constexpr (QM == 64) {
        while (hits) {                       // wave-uniform: scalar loop, scalar lane index
          const int b = __builtin_ctzll(hits);
          hits &= hits - 1;
          const int uu = __builtin_amdgcn_readlane(u, b);
          const float vv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), b));
          dot += (double)vv * (double)s_vals[uu * QM + q];
        }
      } else {
        uint32_t mine = (uint32_t)(hits >> (g * QM)) & (uint32_t)(~0ull >> (64 - QM));
        while (__any(mine != 0)) {           // the rows of a wave step together
          const int b = mine ? __builtin_ctz(mine) : 0;
          const int uu = __shfl(u, g * QM + b, 64);
          const float vv = __shfl(v, g * QM + b, 64);
          if (mine) dot += (double)vv * (double)s_vals[uu * QM + q];
          mine &= mine - 1;
        }
      }
    }
    float* tile = s_tile + par * (QM * TS);
    tile[q * TS + rl] = pool_score(live, metric, dot, qn, m.n2);
    __syncthreads();
    for (int i = threadIdx.x; i < nq * R; i += kWideThreads) {
      const int oq = i / R, orow = i % R;
      if (base + orow < nrows) out[(int64_t)oq * nrows + base + orow] = tile[oq * TS + orow];
    }
    m = nx;
  }
}

}  // namespace jb

namespace {
// bytes of LDS of a pass of QM query lanes over nuniq distinct features
// (0: nuniq out of range), and the bits of its feature table
size_t wide_lds(int QM, int nuniq, int* tbits) {
  if (nuniq < 0 || nuniq > jb::kWideMaxUniq) return 0;
  const size_t U = nuniq > 0 ? nuniq : 1;
  int tb = 4;
  while (((size_t)1 << tb) < 2 * U) ++tb;
  const size_t R = (size_t)jb::kWideThreads / QM;
  if (tbits) *tbits = tb;
  return 8 * (size_t)QM + 8 * ((size_t)1 << tb) + 4 * U * QM + 4 * 2 * QM * (R + 1) + 16;
}

// CUs of the current device (asked per launch: a process may switch devices)
int wide_blocks() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
    n = 64;
  return n;
}

template <int QM>
int wide_launch(const jb::DevQuery& qs, int nq, int nuniq, int tbits, size_t lds,
                const int64_t* r_off, const int32_t* r_len, const double* r_n2,
                const uint8_t* valid, int64_t nrows, const int32_t* p_idx, const float* p_val,
                int metric, float* out, hipStream_t stream) {
  // past 64 KiB of dynamic LDS a kernel has to be told, on the device it is
  // launched on: set per launch where it is needed
  if (lds > 64 * 1024) {
    const hipError_t attr = hipFuncSetAttribute(
        (const void*)jb::pool_rows_wide_kernel<QM>, hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)jb::kWideLdsCap);
    if (attr != hipSuccess) return (int)attr;
  }
  constexpr int64_t R = jb::kWideThreads / QM;
  const int64_t want = (nrows + R - 1) / R, cus = wide_blocks();
  const unsigned blocks = (unsigned)(want < cus ? want : cus);
  hipLaunchKernelGGL((jb::pool_rows_wide_kernel<QM>), dim3(blocks), dim3(jb::kWideThreads), lds,
                     stream, qs, nq, nuniq > 0 ? nuniq : 1, tbits, r_off, r_len, r_n2, valid, nrows,
                     p_idx, p_val, metric, out);
  return (int)hipGetLastError();
}
}  // namespace

// the query lanes (16, 32 or 64) of a wide pass of nq queries with nuniq
// distinct features between them; 0: no wide pass holds them (nq > 64, or the
// LDS layout past 160 KiB). The launcher and the pass planner of
// models/similarity.py both ask here.
extern "C" int jb_pool_wide_qm(int nq, int nuniq) {
  if (nq < 1 || nq > jb::kWideMaxQ) return 0;
  const int QM = nq <= 16 ? 16 : nq <= 32 ? 32 : 64;
  const size_t lds = wide_lds(QM, nuniq, nullptr);
  return lds != 0 && lds <= jb::kWideLdsCap ? QM : 0;
}

// scores [nq][nrows] of nq (<= 64) device-CSR queries over the pool in one
// pass; nuniq: the distinct features of the nq queries (an upper bound will
// do; inserts past it are dropped). -2: an argument out of range, -3:
// jb_pool_wide_qm(nq, nuniq) is 0; nothing is launched in either case.
extern "C" int jb_pool_scan_wide(const int64_t* qptr, const int32_t* qidx, const float* qval,
                                 const double* qn2, int nq, int nuniq, const int64_t* r_off,
                                 const int32_t* r_len, const double* r_n2, const uint8_t* valid,
                                 int64_t nrows, const int32_t* p_idx, const float* p_val,
                                 int metric, float* out, hipStream_t stream) {
  if (nq < 1 || nq > jb::kWideMaxQ || nuniq < 0 || nrows < 0 || (metric != 0 && metric != 1) ||
      !qptr || !qidx || !qval || !qn2 || !r_off || !r_len || !r_n2 || !valid || !p_idx ||
      !p_val || !out)
    return -2;
  const int QM = jb_pool_wide_qm(nq, nuniq);
  if (QM == 0) return -3;
  if (nrows == 0) return 0;
  int tbits = 0;
  const size_t lds = wide_lds(QM, nuniq, &tbits);
  const jb::DevQuery qs{qptr, qidx, qval, qn2, nullptr};
#define JB_WIDE(Q)                                                                              \
  wide_launch<Q>(qs, nq, nuniq, tbits, lds, r_off, r_len, r_n2, valid, nrows, p_idx, p_val, metric, \
                 out, stream)
  return QM == 16 ? JB_WIDE(16) : QM == 32 ? JB_WIDE(32) : JB_WIDE(64);
#undef JB_WIDE
}
