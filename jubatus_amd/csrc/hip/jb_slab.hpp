// The slab layer under the whole-GPU clustering chains (kmeans_wide.hip,
// gmm_wide.hip): G workgroups walk slabs g, g + G, ... of SP points, keep a
// table sR [SP][RS] (scores, then responsibilities) and an X tile sX [SP][kXS]
// in LDS, and sum R^T X into a partial of their own, which a reduce kernel
// then adds up in workgroup order. G and every summation order are fixed
// functions of (n, k, d).
//
// Included from those two files only. It carries no flags of its own: both are
// compiled without the packed fp32 VALU forms (build_ext.py HIP_FILE_FLAGS),
// and so must be whatever else includes it.
#pragma once
#include "jb_device.hpp"

namespace jb {
namespace slab {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kT = 256;              // threads of every kernel on this layer
constexpr int kDC = 32;              // dims per X chunk in LDS
constexpr int kXS = 48;              // row stride of the X tile: rows i .. i + 3 on distinct banks
constexpr int kMaxK = 1024;
constexpr int64_t kMaxKD = (int64_t)1 << 22;
constexpr int64_t kWorkCap = (int64_t)256 << 20;
constexpr int kMaxGrid = 256;        // one workgroup a CU

struct Geo {
  int KP;        // k padded to the 16-row tile
  int SP;        // points a slab: 64 / 32 / 16 (kmeans_wide: a wave holds at most 16 score tiles)
  int RS;        // row stride of sR
  int G;         // workgroups that walk the slabs
  int64_t PS;    // floats of one partial
};

// partial_floats: one workgroup's partial; fixed_floats: the rest of the
// workspace, which holds fixed_floats + G * partial_floats floats within
// kWorkCap bytes. 0 in G: outside the supported range.
__host__ inline Geo geometry(int64_t n, int64_t d, int64_t k, int64_t partial_floats, int64_t fixed_floats) {
  Geo g = {};
  if (n < 1 || n > INT32_MAX || d < 1 || k < 1 || k > kMaxK || k * d > kMaxKD) return g;
  g.KP = (int)((k + 15) / 16 * 16);
  g.SP = g.KP <= 128 ? 64 : g.KP <= 384 ? 32 : 16;
  g.RS = (g.KP + 47) / 64 * 64 + 16;             // RS % 64 == 16: 4 rows x 16 columns, 64 banks
  g.PS = partial_floats;
  const int64_t room = (kWorkCap / 4 - fixed_floats) / g.PS;
  const int64_t slabs = (n + g.SP - 1) / g.SP;
  int64_t G = slabs < kMaxGrid ? slabs : kMaxGrid;
  if (G > room) G = room;
  g.G = (int)G;
  return g;
}

__host__ inline size_t lds_bytes(const Geo& g) { return sizeof(float) * ((size_t)g.SP * g.RS + (size_t)g.SP * kXS); }

// Past 64 KiB of dynamic LDS (only the 16-point slabs get there) a kernel has
// to be told: every kernel of the list once a process, the first error kept
template <auto... KERNELS>
__host__ inline hipError_t allow_large_lds() {
  static const hipError_t attr = [] {
    hipError_t e = hipSuccess;
    ((e = e != hipSuccess ? e
                          : hipFuncSetAttribute((const void*)KERNELS, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                160 * 1024)),
     ...);
    return e;
  }();
  return attr;
}

// the block's sum in a fixed order, every thread gets it (red: 4 floats)
__device__ __forceinline__ float block_sum(float v, float* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  v = wave_sum_fast(v, lane);
  __syncthreads();                   // (red may still be read from the previous call)
  if (lane == 0) red[wv] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// rows [row0, row0 + SP) x dims [q0, q0 + kDC) of X into the LDS tile, zeros
// past n and past d
__device__ __forceinline__ void stage_x(float* __restrict__ sX, const float* __restrict__ X, int n, int d,
                                        int64_t row0, int q0, int SP) {
  for (int e = threadIdx.x; e < SP * kDC; e += kT) {
    const int i = e / kDC, q = e - i * kDC;
    const int64_t gi = row0 + i;
    sX[i * kXS + q] = (gi < n && q0 + q < d) ? X[gi * d + q0 + q] : 0.f;
  }
}

// The update sums of one slab on the matrix cores: P1 += R^T X, Pn += R^T 1
// and, with SQ, P2 += R^T X^2, for the slab's weights R in sR (rows past n and
// columns past k at zero). True GEMMs over the points with no cancellation, so
// they run on v_mfma_f32_16x16x4_f32 (fragment maps at the top of
// clustering.hip): A = R^T from sR, lane l holds R[i0 + (l >> 4)][j0 + (l & 15)];
// B = the X tile, lane l holds X[i0 + (l >> 4)][q0 + (l & 15)], its square for
// P2 and a column of ones for Pn (with the tile at dim 0 only); a step covers
// 4 points. A wave owns the (16 rows of R^T x 16 dims) tiles wave, wave + 4,
// ... of a chunk, and the lane that holds an output element is the only
// writer of that element of the workgroup's partial: a plain store for the
// workgroup's first slab, read-add-write after it. No float atomics.
// UNROLL: of the loop over the points; 0 leaves it to the compiler. wv, lane:
// the thread's wave and lane, the caller's own values (recomputed or widened
// here, they and d end up in registers twice: 4 more VGPRs in kmeans_wide).
template <bool SQ, int UNROLL>
__device__ __forceinline__ void update_sums(const float* sR, float* sX, const float* __restrict__ X, int n, int d,
                                            int k, int64_t row0, int SP, int RS, int KP, float* P1, float* P2,
                                            float* Pn, bool first, int wv, int lane) {
  const int ar = lane & 15, kq = lane >> 4;
  const int jtiles = KP / 16;
  const int64_t ld = d;                          // (widened here, not inside the loops: see above)
  for (int q0 = 0; q0 < d; q0 += kDC) {
    __syncthreads();                             // sR complete / the tile's last readers are done
    stage_x(sX, X, n, d, row0, q0, SP);
    __syncthreads();
    for (int tile = wv; tile < jtiles * (kDC / 16); tile += kT / 64) {
      const int j0 = (tile / (kDC / 16)) * 16, qq0 = (tile % (kDC / 16)) * 16;
      if (q0 + qq0 >= d) continue;               // (wave-uniform)
      const bool with_nk = q0 + qq0 == 0;
      f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f}, a0 = {0.f, 0.f, 0.f, 0.f};
      const float* ra = sR + kq * RS + j0 + ar;
      const float* xb = sX + kq * kXS + qq0 + ar;
      auto step = [&](int i0) {
        const float a = ra[i0 * RS];
        const float b = xb[i0 * kXS];
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, a1, 0, 0, 0);
        if (SQ) a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b * b, a2, 0, 0, 0);
        if (with_nk) a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, 1.f, a0, 0, 0, 0);
      };
      if constexpr (UNROLL > 0) {
#pragma unroll UNROLL
        for (int i0 = 0; i0 < SP; i0 += 4) step(i0);
      } else {
        for (int i0 = 0; i0 < SP; i0 += 4) step(i0);
      }
      const int q = q0 + qq0 + ar;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + kq * 4 + r;
        if (j >= k) continue;
        if (q < d) {
          const int64_t e = j * ld + q;
          P1[e] = first ? a1[r] : P1[e] + a1[r];
          if (SQ) P2[e] = first ? a2[r] : P2[e] + a2[r];
        }
        if (with_nk && ar == 0) Pn[j] = first ? a0[r] : Pn[j] + a0[r];
      }
    }
  }
}

}  // namespace slab
}  // namespace jb
