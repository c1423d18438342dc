// Direct k x k convolution (k = 3, 5; stride 1, padding k/2) over a channel-last image, forward and backward, fp32:
// the convolutions of the PathCNN baseline (models/pathcnn.py: 146 x 3 pca_dim image, 1 -> 32 -> 64 channels) and of the
// pathway head for conv_kernel_list other than [1, 1].  Semantics of F.conv2d(x, w, b, padding = k / 2) (+ ReLU).
//
//   x [B, H, W, Cin]  (the memory of a channel-last [B, Cin, H, W] tensor)     w [Cout, Cin, k, k] as nn.Conv2d holds it
//   y [B, H, W, Cout]
//
// Every product is an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains): no im2col tensor, no atomics,
// every sum in a fixed order (bitwise reproducible).
//
//   forward / input gradient (one kernel, conv_kernel<BWD>): one workgroup per (sample, band of R output rows).  The
//     band's input rows with the k/2 halo are staged in LDS as [rows][cols][channels], zero-filled outside the image and in
//     the padded channels, so the tap loop has no bounds checks.  M = the band's R * W positions (<= 64), N = output
//     channels, K = (tap, input channel).  A wave owns 16-wide output-channel tiles and walks the band's (at most four)
//     16-position tiles with every weight fragment it loads; per tap and block of 16 input channels one 16-byte LDS read
//     is the A operand of four MFMAs (the lane with k-index q takes channels 4 q .. 4 q + 3, the weights are read in the
//     same order).  Bias and ReLU in the epilogue; 16 consecutive lanes store 16 consecutive channels.
//     The input gradient is the same product over grad_y (masked by y > 0 while it is staged: the ReLU backward has no
//     pass of its own) with the taps flipped and the two channel counts exchanged.
//   weight / bias gradient (conv_wgrad_kernel + conv_wgrad_reduce_kernel): per tap dW[tap] += patch^T . grad_y_masked,
//     M = input channels, N = output channels, K = positions.  The (sample, band) units are dealt to a fixed number of
//     workgroup columns; a workgroup owns up to 32 of the (tap, 16 x 16) tiles (8 accumulators per wave) and walks its
//     units, staging the x patch and the masked grad_y band per unit.  The bias gradient is the column sums of the
//     staged band.  Partials go to the caller's workspace, a second launch adds them in column order.
#include "common.h"
#include "launch.h"
#include "mlgnn.h"
#include "tile_gemm.h"

namespace mlgnn {
namespace {

constexpr int kConvMaxC = 128;
constexpr int kConvMaxW = 32;
constexpr int kConvBandPositions = 64;         // M of one band: at most four 16-row tiles
constexpr int kConvBandTiles = kConvBandPositions / 16;
constexpr int kConvPatchBudget = 64 * 1024;    // LDS bytes of a patch above which a band gets fewer rows
constexpr int kConvTilesPerWave = 8;
constexpr int kConvTilesPerGroup = kConvTilesPerWave * kWavesPerBlock;
constexpr int kConvWgradBlocks = 512;          // workgroups of the partials launch (columns x tile groups), about

struct ConvShape {
  int B, H, W;
  int Cr, Cn;        // channels summed over / produced by this product
  int k, pad;
  int R;             // output rows per band
  int nb;            // bands per sample
  int PR, PW;        // patch rows, columns
  int Cr16;          // Cr rounded up to 16
  int CS;            // LDS floats per patch position
  int relu;
};

inline int round16(int64_t c) { return (int)((c + 15) / 16 * 16); }

// patch position stride of the forward / input-gradient kernel: lanes read 16 positions x 4 channel quads, so an odd
// number of quads keeps the 16 positions of a tile row on distinct banks
inline int stride_quads_odd(int c16) { return c16 + 4; }
// ... and of the weight-gradient kernel, where lanes read 16 consecutive channels of 4 consecutive positions
inline int stride_mod64_16(int c16) { return c16 + ((16 - c16 % 64) + 64) % 64; }

inline int band_rows(int64_t H, int64_t W, int64_t k, int64_t cmax) {
  int64_t R = kConvBandPositions / W;
  if (R > H) R = H;
  if (R < 1) R = 1;
  const int64_t cs = stride_mod64_16(round16(cmax));
  while (R > 1 && (R + k - 1) * (W + k - 1) * cs * 4 > kConvPatchBudget) --R;
  return (int)R;
}

bool shape_ok(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t k) {
  if (!(k == 3 || k == 5)) return false;
  if (B < 0 || H < 1 || W < 1 || W > kConvMaxW || Cin < 1 || Cin > kConvMaxC || Cout < 1 || Cout > kConvMaxC) return false;
  const int64_t lim = (int64_t)1 << 32;
  if (H >= lim || (B != 0 && H > (lim / 4) / B)) return false;     // (B * H below 2^30: the products below cannot overflow)
  const int64_t cmax = Cin > Cout ? Cin : Cout;
  return B * H * W * cmax * 4 < lim;
}

ConvShape make_shape(int64_t B, int64_t H, int64_t W, int64_t Cr, int64_t Cn, int64_t k, int64_t cmax, bool wgrad, int relu) {
  ConvShape s;
  s.B = (int)B; s.H = (int)H; s.W = (int)W; s.Cr = (int)Cr; s.Cn = (int)Cn; s.k = (int)k; s.pad = (int)(k / 2);
  s.R = band_rows(H, W, k, cmax);
  s.nb = (int)((H + s.R - 1) / s.R);
  s.PR = s.R + s.k - 1;
  s.PW = s.W + s.k - 1;
  s.Cr16 = round16(Cr);
  s.CS = wgrad ? stride_mod64_16(s.Cr16) : stride_quads_odd(s.Cr16);
  s.relu = relu;
  return s;
}

// patch[(pr * PW + pc) * CS + c] = src[b, r0 - pad + pr, pc - pad, c] (* [mask > 0]), 0 outside the image and for c >= Cr
__device__ __forceinline__ void stage_patch(float* __restrict__ patch, const float* __restrict__ src,
                                            const float* __restrict__ mask, int b, int r0, const ConvShape& s) {
  const int total = s.PR * s.PW * s.Cr16;
  for (int e = threadIdx.x; e < total; e += blockDim.x) {
    const int pos = e / s.Cr16, c = e - pos * s.Cr16;
    const int pr = pos / s.PW, pc = pos - pr * s.PW;
    const int iy = r0 - s.pad + pr, ix = pc - s.pad;
    float v = 0.f;
    if (c < s.Cr && iy >= 0 && iy < s.H && ix >= 0 && ix < s.W) {
      const size_t at = (((size_t)b * s.H + iy) * s.W + ix) * s.Cr + c;
      v = src[at];
      if (mask != nullptr && !(mask[at] > 0.f)) v = 0.f;
    }
    patch[pos * s.CS + c] = v;
  }
}

// BWD = false: dst = conv(src, w) + bias (relu);  Cr = Cin, Cn = Cout, w[(n * Cr + c) * kk + tap]
// BWD = true:  dst = grad_x from src = grad_y (masked by mask = y > 0);  Cr = Cout, Cn = Cin, w[(c * Cn + n) * kk + kk - 1 - tap]
template <bool BWD>
__global__ __launch_bounds__(kBlock) void conv_kernel(const float* __restrict__ src, const float* __restrict__ mask,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ dst, const ConvShape s) {
  extern __shared__ __attribute__((aligned(16))) float conv_smem[];
  float* patch = conv_smem;
  const int b = blockIdx.x / s.nb, band = blockIdx.x - b * s.nb;
  const int r0 = band * s.R;
  stage_patch(patch, src, mask, b, r0, s);
  __syncthreads();

  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int lane = threadIdx.x & (kWave - 1);
  const int l15 = lane & 15, lk = lane >> 4;
  const int kk = s.k * s.k;
  const int Mb = s.R * s.W;
  const int MT = (Mb + 15) >> 4, NT = (s.Cn + 15) >> 4;

  // a wave owns output-channel tiles and walks all (at most four) position tiles of the band with each weight
  // fragment it loads: the strided weight reads are the expensive operand
  int abase[kConvBandTiles];
#pragma unroll
  for (int mt = 0; mt < kConvBandTiles; ++mt) {
    int p = mt * 16 + l15;
    p = p < Mb ? p : 0;                                             // rows past the band are computed and dropped
    const int py = p / s.W, px = p - py * s.W;
    abase[mt] = (py * s.PW + px) * s.CS + 4 * lk;
  }
  for (int nt = wave; nt < NT; nt += kWavesPerBlock) {
    const int n = nt * 16 + l15;
    const bool n_ok = n < s.Cn;
    f32x4 acc[kConvBandTiles];
#pragma unroll
    for (int mt = 0; mt < kConvBandTiles; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < kk; ++tap) {
      const int ty = tap / s.k, tx = tap - ty * s.k;
      const int toff = (ty * s.PW + tx) * s.CS;
      const int wtap = BWD ? kk - 1 - tap : tap;
      for (int c0 = 0; c0 < s.Cr16; c0 += 16) {
        float bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = c0 + 4 * lk + u;
          const bool ok = n_ok && c < s.Cr;
          const int cc = ok ? c : 0, nn = ok ? n : 0;
          const size_t wi = BWD ? ((size_t)cc * s.Cn + nn) * kk + wtap : ((size_t)nn * s.Cr + cc) * kk + wtap;
          const float t = w[wi];
          bv[u] = ok ? t : 0.f;
        }
#pragma unroll
        for (int mt = 0; mt < kConvBandTiles; ++mt) {
          if (mt < MT) {
            const float4 a = *reinterpret_cast<const float4*>(patch + abase[mt] + toff + c0);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bv[0], acc[mt], 0, 0, 0);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bv[1], acc[mt], 0, 0, 0);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bv[2], acc[mt], 0, 0, 0);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bv[3], acc[mt], 0, 0, 0);
          }
        }
      }
    }
    // C/D: column (channel) l15, rows (positions) 4 lk + r
    const float bn = (!BWD && bias != nullptr && n_ok) ? bias[n] : 0.f;
#pragma unroll
    for (int mt = 0; mt < kConvBandTiles; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = mt * 16 + 4 * lk + r;
        const int qy = q / s.W, qx = q - qy * s.W;
        const int oy = r0 + qy;
        if (q < Mb && oy < s.H && n_ok) {
          float v = acc[mt][r] + bn;
          if (!BWD && s.relu) v = relu_keep_nan(v);
          dst[(((size_t)b * s.H + oy) * s.W + qx) * s.Cn + n] = v;
        }
      }
    }
  }
}

struct WgradShape {
  int Cout, Co16, GS;   // grad_y channels, rounded to 16, LDS floats per band position
  int CIT, COT;         // 16-wide tiles over Cin / Cout
  int ntiles;           // kk * CIT * COT
  int ntp;              // ntiles rounded up to a whole tile group
  int G;                // workgroup columns the units are dealt to
  int units, upc;       // (sample, band) units, units per column
};

// ws: [G][ntp][64 lanes][4] accumulator images, then [G][kConvMaxC] bias partials
__global__ __launch_bounds__(kBlock) void conv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                            const float* __restrict__ y, float* __restrict__ ws,
                                                            const ConvShape s, const WgradShape g) {
  extern __shared__ __attribute__((aligned(16))) float conv_smem[];
  float* patch = conv_smem;                                        // x: [PR * PW][CS]
  float* gym = patch + s.PR * s.PW * s.CS;                         // masked grad_y: [Mp][GS]
  int* pos_off = reinterpret_cast<int*>(gym + kConvBandPositions * g.GS);   // [64]: patch offset of a band position, -1 = none

  const int col = blockIdx.x, tg = blockIdx.y;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int lane = threadIdx.x & (kWave - 1);
  const int l15 = lane & 15, lk = lane >> 4;
  const int Mb = s.R * s.W;
  const int Mp = (Mb + 3) & ~3;

  // this wave's tiles: consecutive ids = consecutive output-channel tiles of one (tap, input-channel tile)
  int a_off[kConvTilesPerWave], b_off[kConvTilesPerWave];
  bool live[kConvTilesPerWave];
  const int tile0 = tg * kConvTilesPerGroup + wave * kConvTilesPerWave;
#pragma unroll
  for (int t = 0; t < kConvTilesPerWave; ++t) {
    const int tile = tile0 + t;
    live[t] = tile < g.ntiles;
    const int tl = live[t] ? tile : 0;
    const int cot = tl % g.COT, rest = tl / g.COT;
    const int cit = rest % g.CIT, tap = rest / g.CIT;
    const int ty = tap / s.k, tx = tap - ty * s.k;
    a_off[t] = (ty * s.PW + tx) * s.CS + cit * 16 + l15;
    b_off[t] = cot * 16 + l15;
  }
  f32x4 acc[kConvTilesPerWave];
#pragma unroll
  for (int t = 0; t < kConvTilesPerWave; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bias_sum = 0.f;

  const int u_end = min(g.units, (col + 1) * g.upc);
  for (int u = col * g.upc; u < u_end; ++u) {
    const int b = u / s.nb, band = u - b * s.nb;
    const int r0 = band * s.R;
    __syncthreads();                                               // the previous unit's readers are done
    stage_patch(patch, x, nullptr, b, r0, s);
    for (int e = threadIdx.x; e < Mp * g.Co16; e += blockDim.x) {
      const int p = e / g.Co16, c = e - p * g.Co16;
      const int py = p / s.W, px = p - py * s.W;
      const int oy = r0 + py;
      float v = 0.f;
      if (p < Mb && oy < s.H && c < g.Cout) {
        const size_t at = (((size_t)b * s.H + oy) * s.W + px) * g.Cout + c;
        v = gy[at];
        if (y != nullptr && !(y[at] > 0.f)) v = 0.f;
      }
      gym[p * g.GS + c] = v;
    }
    if (threadIdx.x < kConvBandPositions) {
      const int p = threadIdx.x;
      const int py = p / s.W, px = p - py * s.W;
      pos_off[p] = (p < Mb && r0 + py < s.H) ? (py * s.PW + px) * s.CS : -1;
    }
    __syncthreads();

    for (int p0 = 0; p0 < Mp; p0 += 4) {
      const int off = pos_off[p0 + lk];
      const int po = off < 0 ? 0 : off;
      const float* gp = gym + (p0 + lk) * g.GS;
#pragma unroll
      for (int t = 0; t < kConvTilesPerWave; ++t) {
        if (live[t]) {
          float a = patch[po + a_off[t]];
          a = off < 0 ? 0.f : a;
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, gp[b_off[t]], acc[t], 0, 0, 0);
        }
      }
    }
    if (tg == 0 && (int)threadIdx.x < g.Cout) {
      float sum = 0.f;
      for (int p = 0; p < Mp; ++p) sum += gym[p * g.GS + threadIdx.x];
      bias_sum += sum;
    }
  }

#pragma unroll
  for (int t = 0; t < kConvTilesPerWave; ++t) {
    if (live[t]) {
      float* o = ws + (((size_t)col * g.ntp + tile0 + t) * kWave + lane) * 4;
      *reinterpret_cast<float4*>(o) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    }
  }
  if (tg == 0 && (int)threadIdx.x < g.Cout)
    ws[(size_t)g.G * g.ntp * 256 + (size_t)col * kConvMaxC + threadIdx.x] = bias_sum;
}

__global__ __launch_bounds__(kBlock) void conv_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw,
                                                                   float* __restrict__ gb, int Cin, int kk,
                                                                   const WgradShape g) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int nacc = g.ntiles * 256;
  if (idx < nacc) {
    if (gw == nullptr) return;
    const int tile = idx >> 8, e = idx & 255;
    const int lane = e >> 2, r = e & 3;
    const int cot = tile % g.COT, rest = tile / g.COT;
    const int cit = rest % g.CIT, tap = rest / g.CIT;
    const int co = cot * 16 + (lane & 15), ci = cit * 16 + 4 * (lane >> 4) + r;
    if (co >= g.Cout || ci >= Cin) return;
    float sum = 0.f;
    for (int c = 0; c < g.G; ++c) sum += ws[((size_t)c * g.ntp + tile) * 256 + e];
    gw[((size_t)co * Cin + ci) * kk + tap] = sum;
  } else {
    const int n = idx - nacc;
    if (gb == nullptr || n >= g.Cout) return;
    float sum = 0.f;
    for (int c = 0; c < g.G; ++c) sum += ws[(size_t)g.G * g.ntp * 256 + (size_t)c * kConvMaxC + n];
    gb[n] = sum;
  }
}

WgradShape make_wgrad(const ConvShape& s, int64_t Cin, int64_t Cout) {
  WgradShape g;
  g.Cout = (int)Cout;
  g.Co16 = round16(Cout);
  g.GS = stride_mod64_16(g.Co16);
  g.CIT = (int)((Cin + 15) / 16);
  g.COT = (int)((Cout + 15) / 16);
  g.ntiles = s.k * s.k * g.CIT * g.COT;
  const int groups = (g.ntiles + kConvTilesPerGroup - 1) / kConvTilesPerGroup;
  g.ntp = groups * kConvTilesPerGroup;
  const int64_t units = (int64_t)s.B * s.nb;
  int64_t G = kConvWgradBlocks / groups;
  if (G < 1) G = 1;
  if (G > units) G = units;
  if (G < 1) G = 1;
  g.G = (int)G;
  g.units = (int)units;
  g.upc = (int)((units + G - 1) / G);
  return g;
}

int64_t wgrad_floats(const WgradShape& g) { return (int64_t)g.G * ((int64_t)g.ntp * 256 + kConvMaxC); }

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_conv2d_supported(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t k) {
  return shape_ok(B, H, W, Cin, Cout, k) ? 1 : 0;
}

extern "C" int mlgnn_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int relu, int64_t B,
                                int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t k, void* stream) {
  if (!shape_ok(B, H, W, Cin, Cout, k)) return MLGNN_E_SHAPE;
  if (B == 0) return 0;
  if (!x || !w || !y) return MLGNN_E_NULL;
  const ConvShape s = make_shape(B, H, W, Cin, Cout, k, Cin > Cout ? Cin : Cout, false, relu ? 1 : 0);
  const int lds = s.PR * s.PW * s.CS * 4;
  if (const hipError_t e = allow_dynamic_lds(&conv_kernel<false>, lds); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(conv_kernel<false>, dim3((unsigned)(B * s.nb)), dim3(kBlock), lds, static_cast<hipStream_t>(stream),
                     x, (const float*)nullptr, w, bias, y, s);
  return (int)hipGetLastError();
}

extern "C" int64_t mlgnn_conv2d_bwd_workspace_floats(int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t k) {
  if (!shape_ok(B, H, W, Cin, Cout, k)) return MLGNN_E_SHAPE;
  if (B == 0) return 0;
  const ConvShape s = make_shape(B, H, W, Cin, Cout, k, Cin > Cout ? Cin : Cout, true, 0);
  return wgrad_floats(make_wgrad(s, Cin, Cout));
}

extern "C" int mlgnn_conv2d_bwd(const float* grad_y, const float* x, const float* w, const float* y, int relu,
                                float* grad_x, float* grad_w, float* grad_bias, float* workspace,
                                int64_t workspace_floats, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                                int64_t k, void* stream) {
  if (!shape_ok(B, H, W, Cin, Cout, k)) return MLGNN_E_SHAPE;
  if (B == 0) return 0;
  if (!grad_y || !x || !w || (relu && !y)) return MLGNN_E_NULL;
  const int64_t cmax = Cin > Cout ? Cin : Cout;
  const bool want_w = grad_w != nullptr || grad_bias != nullptr;
  const ConvShape sw = make_shape(B, H, W, Cin, Cout, k, cmax, true, 0);
  const WgradShape g = make_wgrad(sw, Cin, Cout);
  if (want_w && (workspace_floats < wgrad_floats(g) || !workspace)) return MLGNN_E_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* mask = relu ? y : nullptr;
  if (grad_x != nullptr) {
    const ConvShape s = make_shape(B, H, W, Cout, Cin, k, cmax, false, 0);
    const int lds = s.PR * s.PW * s.CS * 4;
    if (const hipError_t e = allow_dynamic_lds(&conv_kernel<true>, lds); e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(conv_kernel<true>, dim3((unsigned)(B * s.nb)), dim3(kBlock), lds, st, grad_y, mask, w,
                       (const float*)nullptr, grad_x, s);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
  }
  if (want_w) {
    const int lds = (sw.PR * sw.PW * sw.CS + kConvBandPositions * g.GS + kConvBandPositions) * 4;
    if (const hipError_t e = allow_dynamic_lds(&conv_wgrad_kernel, lds); e != hipSuccess) return (int)e;
    const int groups = g.ntp / kConvTilesPerGroup;
    hipLaunchKernelGGL(conv_wgrad_kernel, dim3((unsigned)g.G, (unsigned)groups), dim3(kBlock), lds, st, x, grad_y, mask,
                       workspace, sw, g);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    const int threads = g.ntiles * 256 + kConvMaxC;
    hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       workspace, grad_w, grad_bias, (int)Cin, (int)(k * k), g);
    rc = (int)hipGetLastError();
    if (rc != 0) return rc;
  }
  return 0;
}
