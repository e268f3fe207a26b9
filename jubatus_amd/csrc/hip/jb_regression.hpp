// Device functions shared by the regression train kernels (regression.hip,
// regression_ordered.hip): the agent-scope table load, the step sizes of the
// methods besides PA and the register-slot geometry of a wide sample.
#pragma once
#include "jb_linear.hpp"

namespace jb {

__device__ __forceinline__ float ld_agent_r(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// step sizes of one sample (M: Method of jb_linear.hpp): w += sgn tau (S) x,
// P increments from beta (dprec); false when the sample causes no update
template <int M>
__device__ __forceinline__ bool regression_step(float loss, float nrm, float var, float C,
                                                float* tau, float* beta) {
  *beta = 0.f;
  if (M == CW) {
    if (!(var > 0.f)) return false;
    const float m = -loss, phi = C;
    const float b = 1.f + 2.f * phi * m;
    const float gamma = (-b + sqrtf(fmaxf(0.f, b * b - 8.f * phi * (m - phi * var)))) / (4.f * phi * var);
    if (!(gamma > 0.f)) return false;
    *tau = gamma;
    *beta = 2.f * gamma * phi;
    return true;
  }
  if (!(loss > 0.f) || !(nrm > 0.f)) return false;
  if (M == PA1) {
    *tau = fminf(C, loss / nrm);
  } else if (M == PA2) {
    *tau = loss / (nrm + 0.5f / C);
  } else if (M == PERCEPTRON) {
    *tau = C;                                   // the learning rate
  } else if (M == AROW) {
    *beta = 1.f / (var + 1.f / C);
    *tau = loss * *beta;
  } else {                                      // NHERD
    *tau = loss / (var + 1.f / C);
    const float cv = 1.f + C * var;
    *beta = (C * C * var + 2.f * C) / (cv * cv);
  }
  return true;
}

// slots of a sample whose idx, x and pre-sample P stay in registers between
// the gather and the scatter: kRegChunks chunks of 64
constexpr int kRegChunks = 4;
constexpr int kRegSlots = kRegChunks * 64;

}  // namespace jb
