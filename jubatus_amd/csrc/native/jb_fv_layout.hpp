// Num filters as derived rows of the num rule table: the layout shared by the
// device emitter (csrc/hip/jb_fv.hpp), its host twin (jb_hostfv.hpp) and the
// packers (fv_converter/gpu_path.py GpuRuleTable, csrc/server/
// jb_server_common.hpp build_rules). Plain C++, no device code.
//
// A derived num row carries kDerivedRow in value_kind (base rows are 0 or 1,
// so the test needs no read of the programme) and points with `pad` at its
// chain programme, 8-byte aligned in the blob:
//   int32 n_steps, int32 ext_len      ext_len = |s1..sm|: the key extension
//                                     the row's own matcher sees
//   n_steps x FilterStep
// Its suffix bytes are s1..sm + "@type"; the steps' and the row's matchers see
// the key extended by the leading ext_len bytes of that suffix.
#pragma once
#include <stdint.h>

namespace jb {

constexpr int32_t kDerivedRow = 0x100;   // value_kind bit of a filter-chain row
// The cap on filter chains per config (chains that survive pruning; three "*"
// filters make 7), gpu_path.MAX_FILTER_CHAINS. Configs above it keep the host
// converter. The rule blob is staged in LDS up to fv_hash.hip's kBlobCap =
// 1024 bytes; a programme takes 8 + 40 bytes per step and every (chain, base
// row) pair a suffix, so configs with many chains (seven chains and one rule:
// 0.6 KB; fifteen: 1.4 KB) read matchers and steps from global memory
// (L2-resident, a kilobyte or two shared by every lane). That path is
// correct and tested; its cost against the LDS copy has not been measured.
constexpr int kMaxFilterChains = 16;
enum { kFilterAdd = 0, kFilterLinear = 1, kFilterGauss = 2, kFilterSigmoid = 3 };
struct FilterStep {      // gpu_path._STEP "<iiiiiidd"
  int32_t match_kind, match_off, match_len;   // the filter's key matcher
  int32_t ext_len;      // bytes of the row's suffix appended to the key for this step
  int32_t method;       // kFilter*
  int32_t truncate;     // linear_normalization: clamp to [0, 1]
  double a, b;          // add: value, - | linear: min, max | gauss: average, sd | sigmoid: gain, bias
};
static_assert(sizeof(FilterStep) == 40, "FilterStep is packed by the host as <iiiiiidd");

}  // namespace jb
