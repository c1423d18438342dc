// The per-element term of torch.nn.BCELoss as ATen evaluates it, shared by the training criterion (csrc/criterion.hip)
// and the evaluation pass (csrc/eval_metrics.hip):
//   bce(p, y) = -(y max(log p, -100) + (1 - y) max(log(1 - p), -100))
// fp32; a NaN stays a NaN, and a probability outside [0, 1] gives one through the logs.
#pragma once
#include "common.h"

namespace mlgnn {

// std::max(l, -100) as ATen writes it: a NaN stays
__device__ __forceinline__ float clamp_log(float l) { return l < -100.f ? -100.f : l; }

__device__ __forceinline__ float bce_value(float p, float y) {
  return (y - 1.f) * clamp_log(log1pf(-p)) - y * clamp_log(logf(p));
}

}  // namespace mlgnn
