// The gate activations of the LSTM kernels (csrc/lstm.hip, csrc/lstm_train.hip): one definition, so the training forward rounds
// exactly as the inference kernels do.
#pragma once
#include "common.h"

static __device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + __expf(-x)); }
static __device__ __forceinline__ float tanh_f(float x) {
  // tanh(x) = 1 - 2 / (exp(2x) + 1): exact to fp32 rounding, saturates cleanly at +-1 (exp overflow -> inf -> 1 - 0)
  return 1.0f - 2.0f / (__expf(2.0f * x) + 1.0f);
}
