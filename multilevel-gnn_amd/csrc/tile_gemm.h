// One 16x16 output tile on v_mfma_f32_16x16x4_f32 with operands fetched through accessors, for the
// small pooled-graph kernels (diffpool.hip, densesage.hip): lane l supplies A[i = l & 15][k = l >> 4]
// and B[k = l >> 4][j = l & 15] per k-step of 4; C/D: col = l & 15, row = 4 * (l >> 4) + reg.
#pragma once
#include "split_precision.h"
#include "dispatch.h"

namespace mlgnn {

// acc[i][j] = sum_k a_at(i, k) * b_at(k, j).  The accessors return 0 for every k at or past the end of
// their operand (the loop runs in blocks of kTileUnroll k-steps: all operand loads of a block are issued
// before its MFMAs, so their latencies overlap instead of adding up).
constexpr int kTileUnroll = 8;

template <typename FA, typename FB>
__device__ __forceinline__ f32x4 tile_gemm(int kdim, FA a_at, FB b_at) {
  const int lane = threadIdx.x & (kWave - 1);
  const int l15 = lane & 15, lk = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < kdim; k0 += 4 * kTileUnroll) {
    float a[kTileUnroll], b[kTileUnroll];
#pragma unroll
    for (int u = 0; u < kTileUnroll; ++u) {
      a[u] = a_at(l15, k0 + 4 * u + lk);
      b[u] = b_at(k0 + 4 * u + lk, l15);
    }
#pragma unroll
    for (int u = 0; u < kTileUnroll; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc, 0, 0, 0);
  }
  return acc;
}

// ---- one operand resident in registers (densesage.hip) --------------------------------------------------------------
// A wave whose tiles all share one operand (a weight column tile, an adjacency row tile) loads that operand ONCE, in MFMA
// fragment layout, and keeps it for all of its tiles: f[u] = at(4 u + (lane >> 4)) for the 8 KB k-steps of KB blocks.  The
// product below issues exactly the MFMA chains of two tile_gemm(32 KB, ...) calls -- the same k order and the same zero padding to a
// multiple of 32 -- so their results are bit for bit the same.
template <int KB, typename F>
__device__ __forceinline__ void frag_load(float (&f)[8 * KB], F at) {
  const int lk = (threadIdx.x & (kWave - 1)) >> 4;
#pragma unroll
  for (int u = 0; u < 8 * KB; ++u) f[u] = at(4 * u + lk);
}

// two products over one pass of the A operand: acc0 = A b0, acc1 = A b1 (each its own chain, as two tile_gemm calls)
template <int KB, typename FA>
__device__ __forceinline__ void tile_gemm2_b_resident(const float (&b0)[8 * KB], const float (&b1)[8 * KB], FA a_at,
                                                      f32x4& acc0, f32x4& acc1) {
  const int lane = threadIdx.x & (kWave - 1);
  const int l15 = lane & 15, lk = lane >> 4;
  acc0 = f32x4{0.f, 0.f, 0.f, 0.f};
  acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int blk = 0; blk < KB; ++blk) {
    float a[kTileUnroll];
#pragma unroll
    for (int u = 0; u < kTileUnroll; ++u) a[u] = a_at(l15, 32 * blk + 4 * u + lk);
#pragma unroll
    for (int u = 0; u < kTileUnroll; ++u) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b0[8 * blk + u], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b1[8 * blk + u], acc1, 0, 0, 0);
    }
  }
}

// f(IC<KB>{}) for the KB in 1 .. MAXKB that equals kb (block-uniform): the fragment arrays above need their length at
// compile time
template <int MAXKB, typename F>
__device__ __forceinline__ void for_k_blocks(int kb, F&& f) {
  if constexpr (MAXKB > 1) {
    if (kb < MAXKB) { for_k_blocks<MAXKB - 1>(kb, f); return; }
  }
  f(IC<MAXKB>{});
}

}  // namespace mlgnn
