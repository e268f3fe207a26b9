// The scratch buffer of the serial-equivalent (exact) train mode, in one
// place: the 32 tail words every committer reports through, the stop reasons,
// and the byte layout behind them. serial.hip (the bound committer, label
// capacities > 64), vcommit.hip (the verified committer, <= 64) and
// stepper.hip use these names; ops/hip.py mirrors the tail words in TAIL_WORDS
// (tests/test_serial_layout.py holds the two together).
//
//   [tail: int64 x kTailWords]
//   LC <= 64: [S0][PP0][FI][FX][AUX][SL], each n_max entries (VcScratch), then
//             the verified committer's fixed region, 256-aligned
//   LC >  64: [slack: n_max floats][|x|_1: n_max floats]
#pragma once
#include <stdint.h>

namespace jb {

// Tail words (int64 each). Words 4-19 are diagnostics whose meaning depends
// on the committer that ran the batch (kTailVerified tells which).
enum : int {
  kTailStart = 0,        // both committers, stepper chunks: first sample left to the single-stream kernel
  kTailEnd = 1,          // both committers, stepper chunks: end of the batch
  kTailSteps = 2,        // both committers: exact steps
  kTailRounds = 3,       // both committers: rounds
  kTailBoundPhase0 = 4,  // bound committer: shader cycles of its 6 phases (words 4-9, JB_SERIAL_TIMING)
  kTailVcNonCand = 7,    // verify kernel: non-candidates cleared by the bound
  kTailVcWindowLen = 8,  // verify kernel: window length the batch ends with
  kTailVcT = 9,          // verify kernel: candidate threshold T (float bits)
  kTailBoundWall = 10,   // bound committer: wall clock of the kernel, 100 MHz ticks
  kTailVcPhase0 = 10,    // verify kernel: shader cycles of kernel C's 5 phases (words 10-14, JB_COMMIT_PROF)
  kTailBoundCycles = 11, // bound committer: shader cycles of the kernel
  kTailBoundWave0 = 12,  // bound committer: each of its 8 waves' own work (words 12-19)
  kTailVcPhaseWall = 15, // verify kernel: shader cycles of kernel C, all phases
  kTailStepped = 16,     // verify kernel, stepper chunks: samples the stepper chunks applied
  kTailChunks = 17,      // verify kernel, stepper chunks: stepper chunks
  kTailSegEst = 18,      // verify kernel, stepper chunks: segments the next batch should get
  kTailCsWindows = 19,   // verify kernel: windows whose candidates the stepper walked
  kTailReason = 20,      // both committers, stepper chunks: why the batch stopped (kStop*)
  kTailSegments = 21,    // both committers: segments used
  kTailWasted = 22,      // verify kernel: exact steps that did not update
  kTailRefresh = 23,     // verify kernel: guard-band re-scores
  kTailUpdates = 24,     // verify kernel: updates the committer applied
  kTailRows = 25,        // verify kernel: rows in the LDS store of the last window
  kTailExact = 26,       // verify kernel: samples re-scored exactly
  kTailCand = 27,        // verify kernel: candidates walked
  kTailRetries = 28,     // verify kernel: windows that failed verification
  kTailSatWindows = 29,  // verify kernel: windows the full store ended
  kTailTicks = 30,       // verify kernel: wall clock of kernel C, 100 MHz ticks
  kTailVerified = 31,    // init kernel of the verified committer: 1, it ran this batch
  kTailWords = 32
};
constexpr int64_t kTailBytes = 8 * kTailWords;

// why a committer stopped (tail[kTailReason]): the batch is done; its table
// or its segments ran out (the next segment, or the single-stream kernel,
// takes the rest); too many updates (the rest goes to the sequential kernel);
// the bound committer's segment wasted too many exact steps (the next segment
// scores the rest again)
constexpr int64_t kStopDone = 0, kStopSaturated = 1, kStopDense = 2, kStopRescore = 3;

constexpr int64_t round_up_256(int64_t v) { return (v + 255) / 256 * 256; }

// The verified committer's fixed region: state words, candidate bits of the
// longest window, the staged store (row keys, rmax, dW, dP).
constexpr int64_t kVcWindowMax = 65536;             // samples of the longest window
constexpr int kVcBitWords = (int)(kVcWindowMax / 64);
constexpr int64_t kVcStateBytes = 512;
constexpr int64_t kVcStoreRows = 1024, kVcStoreFloats = 16384;
constexpr int64_t kVcFixed =
    kVcStateBytes + 8 * kVcBitWords + 4 * kVcStoreRows + 4 * kVcStoreRows + 2 * 4 * kVcStoreFloats;

// The verified committer's per-sample arrays, each n_max entries long, in
// scratch order after the tail words; the fixed region follows them.
struct VcScratch {
  enum Array : int {
    S0,    // scores at the window start: 64 floats
    PP0,   // precisions of y and the best wrong label: 32 float2
    FI,    // feature indices: 32
    FX,    // feature values: 32
    AUX,   // label, best wrong label, feature count: int4
    SL,    // slack: float
    kArrays
  };
  static constexpr int64_t kEntry[kArrays] = {256, 256, 128, 128, 16, 4};
  // bytes a sample takes in the arrays before a (all of them: a = kArrays)
  static constexpr int64_t per_sample(int a = kArrays) { return a <= 0 ? 0 : kEntry[a - 1] + per_sample(a - 1); }
  static constexpr int64_t offset(Array a, int64_t n_max) { return kTailBytes + per_sample(a) * n_max; }
  static constexpr int64_t fixed_offset(int64_t n_max) { return kTailBytes + round_up_256(per_sample() * n_max); }
  static constexpr int64_t bytes(int64_t n_max) { return fixed_offset(n_max) + kVcFixed; }
};
static_assert(VcScratch::per_sample() == 788 && VcScratch::offset(VcScratch::SL, 1) == kTailBytes + 784, "");

// The bound committer's per-sample arrays: slack and |x|_1, a float each.
struct BoundScratch {
  static constexpr int64_t slack_offset() { return kTailBytes; }
  static constexpr int64_t l1_offset(int64_t n_max) { return kTailBytes + 4 * n_max; }
  static constexpr int64_t bytes(int64_t n_max) { return kTailBytes + round_up_256(8 * n_max); }
};

}  // namespace jb
