// Split-precision arithmetic shared by the MFMA kernels (tallgemm.hip, wgrad.hip, linear_bwd.hip and the other dense
// sources): the vector types of the matrix-core operands, the power-of-two operand scale, the two- and three-way
// splits, the fold of a table of partial maxima, and the accumulator layout of the 32x32 MFMA.  Device code.
#pragma once
#include "common.h"

namespace mlgnn {

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x2 = __attribute__((ext_vector_type(2))) int;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void glb_void_t;

// C/D layout of the 32x32 MFMA: accumulator register r of a lane in half h (= lane >> 5) is row
// (r & 3) + 8 (r >> 2) + 4 h of the tile, column lane & 31
constexpr int mfma32_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// Power of two s with  max * s in [2^13, 2^14)  and its inverse; max = 0 or denormal -> 1.  With this scale the low
// part x_lo = fp16(x s - fp16(x s)) stays a normal fp16 number for every element within 2^-17 of the maximum, so
// |x - x_hi - x_lo| <= 2^-22 |x| there and <= 2^-39 max |x| below; the clamp 20..234 keeps both s and inv normal.
__device__ __forceinline__ void pow2_scale(float max_abs, float& s, float& inv) {
  int e = (int)((__builtin_bit_cast(uint32_t, max_abs) >> 23) & 0xff);       // biased exponent
  e = min(max(e, 20), 234);
  s = __builtin_bit_cast(float, (uint32_t)(254 + 13 - e) << 23);             // 2^(13 - (e - 127))
  inv = __builtin_bit_cast(float, (uint32_t)(e - 13) << 23);                 // 2^((e - 127) - 13)
}

// scaled two-way split of 8 floats: hi = fp16(x s), lo = fp16(x s - hi)
__device__ __forceinline__ void split2(const float (&v)[8], float s, f16x8& h, f16x8& l) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float x = v[j] * s;
    const _Float16 hh = (_Float16)x;
    h[j] = hh;
    l[j] = (_Float16)(x - (float)hh);
  }
}

// exact three-way split of 8 floats into bf16 terms, two at a time (v_cvt_pk_bf16_f32 rounds to nearest even; the
// widening back is a shift / mask of the packed word)
__device__ __forceinline__ void split3(const float (&v)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
  u32x4 hw, mw, lw;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x2 x = {v[2 * j], v[2 * j + 1]};
    const uint32_t hp = __builtin_bit_cast(uint32_t, __builtin_convertvector(x, bf16x2));
    const f32x2 r1 = {x[0] - __builtin_bit_cast(float, hp << 16), x[1] - __builtin_bit_cast(float, hp & 0xffff0000u)};
    const uint32_t mp = __builtin_bit_cast(uint32_t, __builtin_convertvector(r1, bf16x2));
    const f32x2 r2 = {r1[0] - __builtin_bit_cast(float, mp << 16), r1[1] - __builtin_bit_cast(float, mp & 0xffff0000u)};
    const uint32_t lp = __builtin_bit_cast(uint32_t, __builtin_convertvector(r2, bf16x2));
    hw[j] = hp; mw[j] = mp; lw[j] = lp;
  }
  h = __builtin_bit_cast(bf16x8, hw); m = __builtin_bit_cast(bf16x8, mw); l = __builtin_bit_cast(bf16x8, lw);
}

// An operand's global maximum travels as kMaxParts partial maxima (one per slice of the row maxima its producer wrote,
// or one per workgroup of the producing launch): a small launch in front writes the table, every wave of the main
// kernel folds it itself (no atomics, no host round trip).
constexpr int kMaxParts = 256;
template <int PARTS = kMaxParts>
__device__ __forceinline__ float fold_max_parts(const float* part) {          // the same value in every lane
  static_assert(PARTS % kWave == 0, "whole waves of partials");
  const int lane = threadIdx.x & (kWave - 1);
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < PARTS / kWave; ++i) m = fmaxf(m, part[lane + i * kWave]);
  return wave_max(m);
}

}  // namespace mlgnn
