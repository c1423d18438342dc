// Dense multi-head self-attention over a short sequence (the pathway readout 'MSA': nn.TransformerEncoderLayer over the
// P = 146 pathway tokens of every graph, reference models/deepergcn.py:126-128,296-305): fp32, atomic-free, every sum in
// a fixed order (bitwise reproducible), plain IEEE arithmetic (expf / logf, no fast-math flags for this file).
//
//   qkv [B*P, 3*H*D] = linear(x, in_proj_weight, in_proj_bias): thirds q | k | v, head h at columns h*D .. (h+1)*D
//   s_ij = <q_i, k_j> / sqrt(D),  a_ij = softmax_j(s_ij),  lse_i = max_j s_ij + log sum_j exp(s_ij - max)
//   out_i = sum_j (keep_ij * keep_scale * a_ij) v_j                    out [B*P, H*D]: what out_proj reads
//
// One workgroup of 16 waves (8 when the LDS image leaves no room for 16 strips) owns one (b, h) pair; its q, k, v head
// slices (and, in the backward, grad_out's) are copied once into LDS as [P][D | 1] images: the odd row stride makes both access patterns conflict-free, lanes over rows at a
// fixed channel (scores) and lanes over channels of one row (the products with v / k / q).  A wave owns one row at a
// time:
//   score phase    lanes over the keys j (P <= 256: at most 4 passes of 64), q_i broadcast from LDS; the row maximum and
//                  sum are wave reductions; the finished probabilities go to a per-wave LDS strip
//   product phase  lanes over (channel, key group): group g adds the keys j = g, g + G, ... in four interleaved chains,
//                  the G groups are combined by an xor butterfly
// The backward runs the same two phases twice inside the workgroup, by query rows (grad q) and then by key rows (grad k,
// grad v: scores recomputed with the lanes over the queries), so no sum crosses workgroups and nothing is added
// atomically.  Dl_i = <grad_out_i, out_i> is taken as sum_j a_ij dA_ij (the same number, from the row's own
// registers: `out` is not read again) in the query-row phase and kept in LDS for the key-row phase.
//
// Algorithmic bytes per (b, h): forward 3*P*D*4 in, P*D*4 + P*4 out (+ P*P mask bytes); backward 4*P*D*4 + P*4 in
// (+ 2*P*P mask bytes: the key-row phase reads the mask by columns), 3*P*D*4 out.
#include <cmath>
#include <type_traits>
#include "common.h"
#include "launch.h"
#include "mlgnn.h"

// Only the fused multiply-adds written as fmaf() below: the compiler contracts nothing on its own, so the scaled score
// s_ij is the same rounded number wherever it is recomputed (a single key gives a = exp(0) = 1 exactly).
#pragma clang fp contract(off)

namespace mlgnn {
namespace {

constexpr int kMhaWaves = 8;                   // waves per workgroup the LDS budget is stated for ...
constexpr int kMhaWavesWide = 16;              // ... and what is launched when the per-wave strips of 16 still fit
constexpr int kMhaMaxBlock = kMhaWavesWide * kWave;
constexpr int kMhaMaxP = 256;
constexpr int kMhaMaxD = 64;
constexpr int kMhaLdsBytes = 160 * 1024;

struct MhaShape {
  int B, P, H, D;
  int ds;          // LDS row stride: D | 1
  int dl_log2;     // lanes per row of the product phase (log2): the power of two >= D
  int vec4;        // 16-byte global loads (D % 4 == 0 and 16-byte aligned operands)
  float scale;     // 1 / sqrt(D)
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// src[i * ld + c], i < P, c < D  ->  dst[i * ds + c]
__device__ __forceinline__ void load_tile(float* __restrict__ dst, const float* __restrict__ src, size_t ld,
                                          const MhaShape& s) {
  if (s.vec4) {
    const int dq = s.D >> 2;
    for (int e = threadIdx.x; e < s.P * dq; e += blockDim.x) {
      const int i = e / dq, c = (e - i * dq) * 4;
      const float4 t = *reinterpret_cast<const float4*>(src + (size_t)i * ld + c);
      float* d = dst + i * s.ds + c;
      d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    }
  } else {
    for (int e = threadIdx.x; e < s.P * s.D; e += blockDim.x) {
      const int i = e / s.D, c = e - i * s.D;
      dst[i * s.ds + c] = src[(size_t)i * ld + c];
    }
  }
}

// sv[t] = <X[r], Y[row t of this lane]>, and with TWO also da[t] = <U[r], W[row t]>: channels in order, row r broadcast
template <int NP, bool TWO>
__device__ __forceinline__ void row_dots(const float* X, const float* Y, const float* U, const float* W, int r,
                                         const int (&ro)[NP], const MhaShape& s, float (&sv)[NP], float (&da)[NP]) {
#pragma unroll
  for (int t = 0; t < NP; ++t) { sv[t] = 0.f; da[t] = 0.f; }
  const float* xr = X + r * s.ds;
  const float* ur = U + r * s.ds;
#pragma unroll 4
  for (int c = 0; c < s.D; ++c) {
    const float x = xr[c];
#pragma unroll
    for (int t = 0; t < NP; ++t) sv[t] = fmaf(x, Y[ro[t] + c], sv[t]);
    if constexpr (TWO) {
      const float u = ur[c];
#pragma unroll
      for (int t = 0; t < NP; ++t) da[t] = fmaf(u, W[ro[t] + c], da[t]);
    }
  }
}

// sum_r strip[r] * M[r][c] over all P rows for this lane's channel: group g takes r = g, g + G, ... in order, then the
// groups meet in an xor butterfly (the result is in every lane of the channel)
__device__ __forceinline__ float strip_dot(const float* strip, const float* M, int cc, int g, const MhaShape& s) {
  const int G = kWave >> s.dl_log2;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;                 // four chains (rows r, r + G, r + 2G, r + 3G of each step)
  int r = g;
  for (; r + 3 * G < s.P; r += 4 * G) {
    a0 = fmaf(strip[r], M[r * s.ds + cc], a0);
    a1 = fmaf(strip[r + G], M[(r + G) * s.ds + cc], a1);
    a2 = fmaf(strip[r + 2 * G], M[(r + 2 * G) * s.ds + cc], a2);
    a3 = fmaf(strip[r + 3 * G], M[(r + 3 * G) * s.ds + cc], a3);
  }
  for (; r < s.P; r += G) a0 = fmaf(strip[r], M[r * s.ds + cc], a0);
  float acc = (a0 + a1) + (a2 + a3);
  for (int off = 1 << s.dl_log2; off < kWave; off <<= 1) acc += __shfl_xor(acc, off);
  return acc;
}

__device__ __forceinline__ float keep_factor(const uint8_t* __restrict__ keep, size_t at, float keep_scale) {
  return (float)keep[at] * keep_scale;
}

template <int NP>
__global__ __launch_bounds__(kMhaMaxBlock) void mha_fwd_kernel(const float* __restrict__ qkv, const uint8_t* __restrict__ keep,
                                                           float keep_scale, float* __restrict__ out,
                                                           float* __restrict__ lse, const MhaShape s) {
  extern __shared__ __attribute__((aligned(16))) float mha_smem[];
  const int P = s.P, D = s.D, hd = s.H * s.D;
  float* Q = mha_smem;
  float* K = Q + P * s.ds;
  float* V = K + P * s.ds;
  float* strips = V + P * s.ds;                                  // [waves][P]
  const int bh = blockIdx.x, b = bh / s.H, h = bh - b * s.H;
  const size_t ld = (size_t)3 * hd;
  const float* base = qkv + (size_t)b * P * ld + (size_t)h * D;
  load_tile(Q, base, ld, s);
  load_tile(K, base + hd, ld, s);
  load_tile(V, base + 2 * hd, ld, s);
  __syncthreads();

  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int lane = threadIdx.x & (kWave - 1);
  const int nwaves = blockDim.x / kWave;
  float* strip = strips + wave * P;
  int ro[NP];
#pragma unroll
  for (int t = 0; t < NP; ++t) ro[t] = min(t * kWave + lane, P - 1) * s.ds;
  const int c = lane & ((1 << s.dl_log2) - 1), g = lane >> s.dl_log2, cc = min(c, D - 1);
  const float ninf = -__builtin_inff();

  for (int i = wave; i < P; i += nwaves) {
    float sv[NP], unused[NP];
    row_dots<NP, false>(Q, K, Q, K, i, ro, s, sv, unused);
    float m = ninf;
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      sv[t] = (t * kWave + lane < P) ? sv[t] * s.scale : ninf;
      m = fmaxf(m, sv[t]);
    }
    m = wave_max(m);
    float e[NP], sum = 0.f;
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      e[t] = (t * kWave + lane < P) ? expf(sv[t] - m) : 0.f;
      sum += e[t];
    }
    sum = wave_sum(sum);
    if (lane == 0) lse[(size_t)bh * P + i] = m + logf(sum);
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int j = t * kWave + lane;
      if (j < P) {
        float p = e[t] / sum;
        if (keep) p *= keep_factor(keep, ((size_t)bh * P + i) * P + j, keep_scale);
        strip[j] = p;
      }
    }
    wave_sync();
    const float o = strip_dot(strip, V, cc, g, s);
    if (g == 0 && c < D) out[((size_t)b * P + i) * hd + (size_t)h * D + c] = o;
    wave_sync();
  }
}

template <int NP>
__global__ __launch_bounds__(kMhaMaxBlock) void mha_bwd_kernel(const float* __restrict__ go, const float* __restrict__ qkv,
                                                           const float* __restrict__ lse,
                                                           const uint8_t* __restrict__ keep, float keep_scale,
                                                           float* __restrict__ gqkv, const MhaShape s) {
  extern __shared__ __attribute__((aligned(16))) float mha_smem[];
  const int P = s.P, D = s.D, hd = s.H * s.D;
  float* Q = mha_smem;
  float* K = Q + P * s.ds;
  float* V = K + P * s.ds;
  float* G = V + P * s.ds;                                       // grad_out's head slice
  float* L = G + P * s.ds;                                       // lse [P]
  float* Dl = L + P;                                             // <grad_out_i, out_i> [P]
  float* strips = Dl + P;                                        // [waves][2][P]
  const int bh = blockIdx.x, b = bh / s.H, h = bh - b * s.H;
  const size_t ld = (size_t)3 * hd;
  const float* base = qkv + (size_t)b * P * ld + (size_t)h * D;
  const float* gbase = go + (size_t)b * P * hd + (size_t)h * D;
  float* gq = gqkv + (size_t)b * P * ld + (size_t)h * D;
  load_tile(Q, base, ld, s);
  load_tile(K, base + hd, ld, s);
  load_tile(V, base + 2 * hd, ld, s);
  load_tile(G, gbase, (size_t)hd, s);
  for (int i = threadIdx.x; i < P; i += blockDim.x) L[i] = lse[(size_t)bh * P + i];
  __syncthreads();

  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int lane = threadIdx.x & (kWave - 1);
  const int nwaves = blockDim.x / kWave;
  float* strip_a = strips + wave * 2 * P;
  float* strip_b = strip_a + P;
  int ro[NP];
#pragma unroll
  for (int t = 0; t < NP; ++t) ro[t] = min(t * kWave + lane, P - 1) * s.ds;
  const int c = lane & ((1 << s.dl_log2) - 1), g = lane >> s.dl_log2, cc = min(c, D - 1);
  const bool writer = g == 0 && c < D;

  // by query rows: dS_ij over the keys j, grad q_i = sum_j dS_ij k_j / sqrt(D)
  for (int i = wave; i < P; i += nwaves) {
    float sv[NP], da[NP];
    row_dots<NP, true>(Q, K, G, V, i, ro, s, sv, da);
    const float li = L[i];
    float a[NP], di = 0.f;
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int j = t * kWave + lane;
      a[t] = 0.f;
      if (j < P) {
        a[t] = expf(sv[t] * s.scale - li);
        if (keep) da[t] *= keep_factor(keep, ((size_t)bh * P + i) * P + j, keep_scale);
        di = fmaf(a[t], da[t], di);
      }
    }
    di = wave_sum(di);                                           // Dl_i = sum_j a_ij dA_ij  (= <grad_out_i, out_i>)
    if (lane == 0) Dl[i] = di;
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int j = t * kWave + lane;
      if (j < P) strip_a[j] = a[t] * (da[t] - di);
    }
    wave_sync();
    const float dq = strip_dot(strip_a, K, cc, g, s) * s.scale;
    if (writer) gq[(size_t)i * ld + c] = dq;
    wave_sync();
  }

  __syncthreads();                                               // Dl of every query row is in LDS

  // by key rows: the same dS_ij over the queries i, grad k_j = sum_i dS_ij q_i / sqrt(D), grad v_j = sum_i keep a_ij grad_out_i
  for (int j = wave; j < P; j += nwaves) {
    float sv[NP], da[NP];
    row_dots<NP, true>(K, Q, V, G, j, ro, s, sv, da);
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const int i = t * kWave + lane;
      if (i < P) {
        const float a = expf(sv[t] * s.scale - L[i]);
        const float kf = keep ? keep_factor(keep, ((size_t)bh * P + i) * P + j, keep_scale) : 1.f;
        strip_a[i] = a * ((keep ? kf * da[t] : da[t]) - Dl[i]);
        strip_b[i] = keep ? kf * a : a;
      }
    }
    wave_sync();
    const float dk = strip_dot(strip_a, Q, cc, g, s) * s.scale;
    const float dv = strip_dot(strip_b, G, cc, g, s);
    if (writer) {
      gq[(size_t)j * ld + hd + c] = dk;
      gq[(size_t)j * ld + 2 * hd + c] = dv;
    }
    wave_sync();
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
int64_t fwd_lds_bytes(int64_t P, int64_t D, int waves = kMhaWaves) { return (3 * P * (D | 1) + waves * P) * 4; }
int64_t bwd_lds_bytes(int64_t P, int64_t D, int waves = kMhaWaves) { return (4 * P * (D | 1) + 2 * P + 2 * waves * P) * 4; }

bool shape_ok(int64_t B, int64_t P, int64_t H, int64_t D) {
  return B >= 0 && B < ((int64_t)1 << 32) && P >= 0 && P <= kMhaMaxP && H >= 1 && H <= 16 && D >= 1 && D <= kMhaMaxD
         && bwd_lds_bytes(P, D) <= kMhaLdsBytes && B * P * 3 * H * D * 4 < ((int64_t)1 << 32);
}

MhaShape make_shape(int64_t B, int64_t P, int64_t H, int64_t D, bool vec_aligned) {
  MhaShape s;
  s.B = (int)B; s.P = (int)P; s.H = (int)H; s.D = (int)D;
  s.ds = (int)(D | 1);
  s.dl_log2 = lanes_per_row_log2(D, 1);
  s.vec4 = (D % 4 == 0 && vec_aligned) ? 1 : 0;
  s.scale = (float)(1.0 / sqrt((double)D));
  return s;
}

template <typename F>
void for_passes(int64_t P, F&& f) {
  if (P <= 64) f(std::integral_constant<int, 1>{});
  else if (P <= 128) f(std::integral_constant<int, 2>{});
  else if (P <= 192) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 4>{});
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_mha_supported(int64_t B, int64_t P, int64_t H, int64_t D) { return shape_ok(B, P, H, D) ? 1 : 0; }

extern "C" int mlgnn_mha_fwd(const float* qkv, const uint8_t* keep, float keep_scale, float* out, float* lse,
                             int64_t B, int64_t P, int64_t H, int64_t D, void* stream) {
  if (!shape_ok(B, P, H, D)) return MLGNN_E_SHAPE;
  if (B == 0 || P == 0) return 0;
  if (!qkv || !out || !lse) return MLGNN_E_NULL;
  const MhaShape s = make_shape(B, P, H, D, aligned(qkv));
  const int waves = fwd_lds_bytes(P, D, kMhaWavesWide) <= kMhaLdsBytes ? kMhaWavesWide : kMhaWaves;
  const int lds = (int)fwd_lds_bytes(P, D, waves);
  hipStream_t st = as_stream(stream);
  hipError_t lds_err = hipSuccess;
  for_passes(P, [&](auto np) {
    auto kernel = &mha_fwd_kernel<decltype(np)::value>;
    lds_err = allow_dynamic_lds(kernel, lds);
    if (lds_err != hipSuccess) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(B * H)), dim3(waves * kWave), lds, st, qkv, keep, keep_scale, out, lse, s);
  });
  return lds_err != hipSuccess ? (int)lds_err : (int)hipGetLastError();
}

// both phases of the backward run inside the workgroup that owns the (b, h) pair: no workspace (0 floats, NULL is fine)
extern "C" int64_t mlgnn_mha_bwd_workspace_floats(int64_t B, int64_t P, int64_t H, int64_t D) {
  if (!shape_ok(B, P, H, D)) return MLGNN_E_SHAPE;
  return 0;
}

extern "C" int mlgnn_mha_bwd(const float* grad_out, const float* qkv, const float* out, const float* lse,
                             const uint8_t* keep, float keep_scale, float* grad_qkv, float* workspace,
                             int64_t workspace_floats, int64_t B, int64_t P, int64_t H, int64_t D, void* stream) {
  if (!shape_ok(B, P, H, D)) return MLGNN_E_SHAPE;
  if (B == 0 || P == 0) return 0;
  if (!grad_out || !qkv || !out || !lse || !grad_qkv) return MLGNN_E_NULL;
  const int64_t need = mlgnn_mha_bwd_workspace_floats(B, P, H, D);
  if (workspace_floats < need || (need > 0 && !workspace)) return MLGNN_E_WORKSPACE;
  const MhaShape s = make_shape(B, P, H, D, aligned(qkv, grad_out));
  const int waves = bwd_lds_bytes(P, D, kMhaWavesWide) <= kMhaLdsBytes ? kMhaWavesWide : kMhaWaves;
  const int lds = (int)bwd_lds_bytes(P, D, waves);
  hipStream_t st = as_stream(stream);
  hipError_t lds_err = hipSuccess;
  for_passes(P, [&](auto np) {
    auto kernel = &mha_bwd_kernel<decltype(np)::value>;
    lds_err = allow_dynamic_lds(kernel, lds);
    if (lds_err != hipSuccess) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(B * H)), dim3(waves * kWave), lds, st, grad_out, qkv, lse, keep, keep_scale,
                       grad_qkv, s);
  });
  return lds_err != hipSuccess ? (int)lds_err : (int)hipGetLastError();
}
