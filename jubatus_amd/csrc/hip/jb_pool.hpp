// What the two scan kernels of the device inverted index share
// (sparse_pool.hip: up to 8 queries a pass, one lane or a few per row;
// sparse_pool_wide.hip: up to 64 queries a pass, one lane per (row, query)):
// the hash of the LDS feature table, the device-CSR query source and the
// score epilogue.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace jb {

__device__ __forceinline__ uint32_t pool_hash(int32_t f) { return (uint32_t)f * 0x9E3779B1u; }

// Queries of a scan: a device CSR (qptr / qidx / qval / qn2; qptr holds
// absolute positions in qidx / qval, so a pass over queries [a, b) of a batch
// takes qptr + a and qn2 + a) or stored rows (qslots: their runs are read
// from the pool).
struct DevQuery {
  const int64_t* qptr;
  const int32_t* qidx;
  const float* qval;
  const double* qn2;
  const int32_t* qslots;
  __device__ bool by_slot() const { return qslots != nullptr; }
  __device__ int32_t slot(int q) const { return qslots[q]; }
  __device__ int64_t start(int q) const { return qptr[q]; }
  __device__ int64_t end(int q) const { return qptr[q + 1]; }
  __device__ int64_t base() const { return qptr[0]; }
  __device__ double norm2(int q) const { return qn2[q]; }
  __device__ int32_t f(int64_t i) const { return qidx[i]; }
  __device__ float v(int64_t i) const { return qval[i]; }
};

// score of one (query, row) pair from its fp64 dot product and squared norms:
// cosine similarity (metric 0) or euclidean distance (1); -inf / +inf for a
// slot that holds no row
__device__ __forceinline__ float pool_score(bool live, int metric, double dot, double qn2,
                                            double rn2) {
  if (!live) return metric == 0 ? -INFINITY : INFINITY;
  if (metric == 0) {
    const double den = sqrt(qn2) * sqrt(rn2);
    return den > 0.0 ? (float)(dot / den) : 0.f;
  }
  // dot products and norms in double: the euclidean distance of a row
  // to itself (|q|^2 + |r|^2 - 2 q.r) must cancel to ~0
  return (float)sqrt(fmax(0.0, qn2 + rn2 - 2.0 * dot));
}

}  // namespace jb
