// Device half of the GPU fv_converter: rule table + per-datum feature
// emission, shared by the batch kernel (fv_hash.hip) and the fused
// low-latency classify kernel (classify_direct.hip).
// Feature-name scheme: jubatus_amd/fv_converter/converter.py.
//
// Num filters (num_filter_rules with a built-in method) run here as extra rows
// of the num rule table. A filter appends (key + suffix, f(x)) to the datum
// before the num rules run, and FNV-1a streams, so "a chain of filters f1 < f2
// < ... followed by num rule r" is one more row: its suffix bytes are
// s1..sm + "@type" (hashed after the key exactly as a base row's "@type"), its
// matchers see the key extended by the leading bytes of that suffix, and a
// chain programme in the blob gives the fp64 arithmetic in front of the cast
// to fp32. Slots stay value-major, row-minor: n_nrules counts base + derived
// rows. Example:
//   "num_filter_types": {"z": {"method": "gaussian_normalization",
//                              "average": 170, "standard_deviation": 8}},
//   "num_filter_rules": [{"key": "height", "type": "z", "suffix": "_z"}],
//   "num_rules":        [{"key": "*_z", "type": "num"}]
// packs two rows: the base row ("*_z", "@num") and the derived row of chain
// (0,) with suffix "_z@num".
#pragma once
#include "jb_device.hpp"
#include "../native/jb_fv_layout.hpp"

namespace jb {

// One key matcher + one feature-name suffix. Packed by the host
// (jubatus_amd/fv_converter/gpu_path.py, GpuRuleTable).
struct GpuRule {
  int32_t match_kind;   // 0 '*', 1 prefix "abc*", 2 suffix "*abc", 3 exact
  int32_t match_off;    // offset of the matcher bytes in the rule blob
  int32_t match_len;
  int32_t suffix_off;   // offset of "@str#bin/bin" / "@num" / "@log"
  int32_t suffix_len;
  int32_t value_kind;   // string rules: 0 = constant weight; num rules: 0 num, 1 log,
                        // | kDerivedRow on a filter-chain row
  float weight;         // string rules: sample_weight*global_weight for one occurrence
  int32_t pad;          // derived num rows: offset of the chain programme in the blob
};

// The layout of derived num rows (kDerivedRow, the chain programme, FilterStep,
// kFilter*) is shared with the host twin and the packers: ../native/jb_fv_layout.hpp.

__device__ __forceinline__ bool key_matches(const GpuRule& r, const uint8_t* blob,
                                            const uint8_t* k, int kn) {
  if (r.match_kind == 0) return true;
  const uint8_t* m = blob + r.match_off;
  int mn = r.match_len;
  if (r.match_kind == 3 && kn != mn) return false;
  if (kn < mn) return false;
  const uint8_t* base = (r.match_kind == 2) ? (k + kn - mn) : k;
  for (int i = 0; i < mn; ++i)
    if (base[i] != m[i]) return false;
  return true;
}

// A matcher over the virtual concatenation key || ext (ext: the leading bytes
// of a derived row's suffix); the string is never built.
__device__ __forceinline__ bool ext_key_matches(int kind, const uint8_t* m, int mn,
                                                const uint8_t* k, int kn,
                                                const uint8_t* e, int en) {
  if (kind == 0) return true;
  const int tn = kn + en;
  if (kind == 3 && tn != mn) return false;
  if (tn < mn) return false;
  const int start = (kind == 2) ? tn - mn : 0;
  for (int i = 0; i < mn; ++i) {
    const int p = start + i;
    const uint8_t c = p < kn ? k[p] : e[p - kn];
    if (c != m[i]) return false;
  }
  return true;
}

// One filter in fp64, the expressions of converter.py / jb_hostfv_wide.hpp
// term by term (no contraction, no reassociation). sigmoid: a finite
// -g(x - b) above ~709.78 gives exp = inf and y = 0.0, as the reference's C++
// does; Python's math.exp raises OverflowError there.
__device__ __forceinline__ double filter_apply(int method, double a, double b, int truncate,
                                               double x) {
#pragma clang fp contract(off)
  switch (method) {
    case kFilterAdd: return x + a;
    case kFilterLinear: {
      double y = (x - a) / (b - a);
      if (truncate) {             // std::min(1.0, std::max(0.0, y)): NaN -> 0.0
        y = (0.0 < y) ? y : 0.0;
        y = (y < 1.0) ? y : 1.0;
      }
      return y;
    }
    case kFilterGauss: return (x - a) / b;
    default: return 1.0 / (1.0 + exp(-a * (x - b)));
  }
}

// A derived row on one value: every chain step's matcher on the key extended
// so far, then the row's own matcher on the whole derived key; *y = fm(..f1(x)).
__device__ __forceinline__ bool chain_matches(const GpuRule& r, const uint8_t* blob,
                                              const uint8_t* k, int kn, double* y) {
  const uint8_t* pg = blob + r.pad;
  const int n_steps = *reinterpret_cast<const int32_t*>(pg);
  const int ext_len = *reinterpret_cast<const int32_t*>(pg + 4);
  const uint8_t* ext = blob + r.suffix_off;
  const FilterStep* st = reinterpret_cast<const FilterStep*>(pg + 8);
  double v = *y;
  for (int j = 0; j < n_steps; ++j) {
    const FilterStep s = st[j];
    if (!ext_key_matches(s.match_kind, blob + s.match_off, s.match_len, k, kn, ext, s.ext_len))
      return false;
    v = filter_apply(s.method, s.a, s.b, s.truncate, v);
  }
  *y = v;
  return ext_key_matches(r.match_kind, blob + r.match_off, r.match_len, k, kn, ext, ext_len);
}

// Walk one datum and emit its feature slots; returns false on a structural
// error (the host scanner validated the bytes already, so this is defensive).
__device__ __forceinline__ bool emit_datum(Reader& rd, int64_t slot, const int64_t slot_end,
                                           const GpuRule* __restrict__ srules, int n_srules,
                                           const GpuRule* __restrict__ nrules, int n_nrules,
                                           const uint8_t* blob, uint64_t H,
                                           int32_t* __restrict__ out_idx,
                                           float* __restrict__ out_val) {
  int64_t top = rd.array_len();
  if (top < 2) return false;
  // ---- string_values: [[key, value], ...]
  int64_t ns = rd.array_len();
  for (int64_t i = 0; i < ns && rd.ok; ++i) {
    if (rd.array_len() != 2) return false;
    const uint8_t *k, *v; int kn, vn;
    if (!rd.raw(&k, &kn) || !rd.raw(&v, &vn)) return false;
    uint64_t hk = fnv_bytes(kFnvOffset, k, kn);
    hk = fnv_byte(hk, '$');
    hk = fnv_bytes(hk, v, vn);
    for (int r = 0; r < n_srules; ++r) {
      const GpuRule rule = srules[r];
      if (slot >= slot_end) return false;
      if (key_matches(rule, blob, k, kn)) {
        const uint64_t h = fnv_bytes(hk, blob + rule.suffix_off, rule.suffix_len);
        out_idx[slot] = (int32_t)hash_to_index(h, H);
        out_val[slot] = rule.weight;
      } else {
        out_idx[slot] = -1;
        out_val[slot] = 0.f;
      }
      ++slot;
    }
  }
  // ---- num_values: [[key, number], ...]
  int64_t nn = rd.ok ? rd.array_len() : -1;
  for (int64_t i = 0; i < nn && rd.ok; ++i) {
    if (rd.array_len() != 2) return false;
    const uint8_t* k; int kn; double x;
    if (!rd.raw(&k, &kn) || !rd.number(&x)) return false;
    const uint64_t hk = fnv_bytes(kFnvOffset, k, kn);
    for (int r = 0; r < n_nrules; ++r) {
      const GpuRule rule = nrules[r];
      if (slot >= slot_end) return false;
      double y = x;
      const bool hit = (rule.value_kind & kDerivedRow) ? chain_matches(rule, blob, k, kn, &y)
                                                       : key_matches(rule, blob, k, kn);
      if (hit) {
        const uint64_t h = fnv_bytes(hk, blob + rule.suffix_off, rule.suffix_len);
        out_idx[slot] = (int32_t)hash_to_index(h, H);
        out_val[slot] = (rule.value_kind & 1) ? logf(fmaxf(1.f, (float)y)) : (float)y;
      } else {
        out_idx[slot] = -1;
        out_val[slot] = 0.f;
      }
      ++slot;
    }
  }
  return rd.ok && slot == slot_end;
}

}  // namespace jb
