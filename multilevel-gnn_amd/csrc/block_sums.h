// The workgroup sums of the per-pair fold-preparation kernels (csrc/edge_select.hip, csrc/kraskov_mi.hip) in one fixed
// order: the 64 lanes of a wave by an xor butterfly, then the four waves in wave order.  No atomics, so the bits of a sum
// depend on nothing but the lanes' own values.
#pragma once
#include "common.h"

namespace mlgnn {

// The sums of V values over the workgroup in the fixed order, in every lane.  `scratch`: V * kWavesPerBlock doubles of
// LDS that no other reduction of the kernel uses (so one barrier suffices).
template <int V>
__device__ __forceinline__ void block_sums(double (&v)[V], double* scratch) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < V; ++q) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[q] += __shfl_xor(v[q], o);
    if ((tid & (kWave - 1)) == 0) scratch[q * kWavesPerBlock + tid / kWave] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < V; ++q) {
    const double* r = scratch + q * kWavesPerBlock;
    v[q] = ((r[0] + r[1]) + r[2]) + r[3];
  }
}

}  // namespace mlgnn
