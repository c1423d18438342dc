// The tail every model family hands its head: max-pool over (ph, pw) windows (stride = window, no padding, floor mode) of a
// channel-last image, dropout, flatten in NCHW order and one appended column (the age) -- one launch per direction.
//
//   x    [B, H, W, C]                 channel-last memory of a [B, C, H, W] tensor (what conv2d / HeadConv2d write)
//   out  [B, C * Ho * Wo (+ 1)]       out[b, (c * Ho + ho) * Wo + wo]; the last column is extra[b] when it is given
//
// so the op is a transposition per sample -- pooled positions s = ho * Wo + wo by channels in, channels by pooled positions
// out -- with the window maximum (forward) or the scatter to the window's winner (backward) on the way.  A workgroup
// owns a kTs x kTc tile (pooled positions x channels): the channel-last side is touched in runs along C, the flattened side
// in runs along s, and the tile turns through LDS (rows padded by one float: both the row-wise and the column-wise
// access are conflict-free, as in transpose_batched_kernel of sage.hip).  The flattened rows have odd length with the
// extra column, so that side is accessed one float per lane.
//
// The winner follows ATen's max_pool2d: scan h then w, start at the first element, a later element replaces it when it
// is greater or NaN.  Its position inside the window (dh * pw + dw < 256) is one byte per pooled element, in output
// order like the keep flags; the backward needs nothing else.  Both directions are copies and at most one fp32
// multiply by keep * keep_scale (a multiply, not a select: NaN and Inf times 0 stay NaN).  No atomics, no memset: every
// element of out / grad_x is written exactly once, the remainder rows and columns of grad_x (zeros) by the workgroups
// of the last pooled row / column.
#include "common.h"
#include "mlgnn.h"

namespace mlgnn {
namespace {

constexpr int kTs = 32;            // pooled positions per tile
constexpr int kTc = 64;            // channels per tile
constexpr int kPoolMaxWindow = 16;
constexpr int64_t kPoolMaxBatchSlab = 65535;   // gridDim.z

struct PoolShape {
  int H, W, C, ph, pw, Ho, Wo, S;  // S = Ho * Wo
  int c_tiles;
  size_t out_stride;               // C * S (+ 1 with the extra column)
};

// fp32, 1 <= ph, pw <= 16, H >= ph, W >= pw, C >= 1, B >= 0, x and out (with the extra column) below 4 GiB
bool shape_ok(int64_t B, int64_t H, int64_t W, int64_t C, int64_t ph, int64_t pw) {
  const int64_t lim = (int64_t)1 << 30;                  // floats in 4 GiB
  if (ph < 1 || pw < 1 || ph > kPoolMaxWindow || pw > kPoolMaxWindow) return false;
  if (B < 0 || C < 1 || H < ph || W < pw) return false;
  if (H >= lim || W >= lim || C >= lim || B > lim) return false;
  const int64_t hw = H * W;
  if (hw >= lim) return false;
  const int64_t per = hw * C;                            // < 2^60
  if (per >= lim) return false;
  const int64_t row = C * (H / ph) * (W / pw) + 1;       // <= per + 1
  const int64_t widest = per > row ? per : row;
  return B * widest < lim;
}

PoolShape make_shape(int64_t H, int64_t W, int64_t C, int64_t ph, int64_t pw, bool extra) {
  PoolShape s;
  s.H = (int)H; s.W = (int)W; s.C = (int)C; s.ph = (int)ph; s.pw = (int)pw;
  s.Ho = (int)(H / ph); s.Wo = (int)(W / pw); s.S = s.Ho * s.Wo;
  s.c_tiles = (int)((C + kTc - 1) / kTc);
  s.out_stride = (size_t)C * s.S + (extra ? 1 : 0);
  return s;
}

unsigned grid_x(const PoolShape& s) { return (unsigned)((s.S + kTs - 1) / kTs) * (unsigned)s.c_tiles; }

// PH, PW > 0: the window at compile time (the shipped configurations); 0: s.ph x s.pw
template <int PH, int PW>
__global__ __launch_bounds__(kBlock) void pool_flatten_fwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ keep,
                                                                 float keep_scale, const float* __restrict__ extra,
                                                                 float* __restrict__ out, uint8_t* __restrict__ winner,
                                                                 PoolShape s) {
  __shared__ float tile[kTs][kTc + 1];
  __shared__ int wtile[kTs][kTc + 1];
  const int ph = PH ? PH : s.ph, pw = PW ? PW : s.pw;
  const int b = blockIdx.z;
  const int c0 = (int)(blockIdx.x % s.c_tiles) * kTc, s0 = (int)(blockIdx.x / s.c_tiles) * kTs;
  const float* xb = x + (size_t)b * s.H * s.W * s.C;
  {
    const int tx = threadIdx.x & (kTc - 1), ty = threadIdx.x / kTc;            // 64 channels x 4 pooled positions
    const int c = c0 + tx;
    if (c < s.C) {
      for (int i = ty; i < kTs && s0 + i < s.S; i += kBlock / kTc) {
        const int ho = (s0 + i) / s.Wo, wo = (s0 + i) - ho * s.Wo;
        const float* p = xb + ((size_t)ho * ph * s.W + (size_t)wo * pw) * s.C + c;
        float best = p[0];
        int win = 0;
#pragma unroll
        for (int dh = 0; dh < ph; ++dh) {
#pragma unroll
          for (int dw = 0; dw < pw; ++dw) {
            const float v = p[((size_t)dh * s.W + dw) * s.C];
            if (v > best || v != v) { best = v; win = dh * pw + dw; }
          }
        }
        tile[i][tx] = best;
        wtile[i][tx] = win;
      }
    }
  }
  __syncthreads();
  {
    const int tx = threadIdx.x & (kTs - 1), ty = threadIdx.x / kTs;            // 32 pooled positions x 8 channels
    const int sp = s0 + tx;
    if (sp < s.S) {
      for (int i = ty; i < kTc && c0 + i < s.C; i += kBlock / kTs) {
        const size_t e = (size_t)(c0 + i) * s.S + sp;                          // within the sample's row
        float v = tile[tx][i];
        if (keep) v *= (float)keep[(size_t)b * s.C * s.S + e] * keep_scale;
        out[(size_t)b * s.out_stride + e] = v;
        if (winner) winner[(size_t)b * s.C * s.S + e] = (uint8_t)wtile[tx][i];
      }
    }
  }
  if (extra && blockIdx.x == 0 && threadIdx.x == 0) out[(size_t)b * s.out_stride + (size_t)s.C * s.S] = extra[b];
}

template <int PH, int PW>
__global__ __launch_bounds__(kBlock) void pool_flatten_bwd_kernel(const float* __restrict__ grad_out, const uint8_t* __restrict__ keep,
                                                                 float keep_scale, const uint8_t* __restrict__ winner,
                                                                 float* __restrict__ grad_x, PoolShape s) {
  __shared__ float tile[kTs][kTc + 1];
  __shared__ int wtile[kTs][kTc + 1];
  const int ph = PH ? PH : s.ph, pw = PW ? PW : s.pw;
  const int b = blockIdx.z;
  const int c0 = (int)(blockIdx.x % s.c_tiles) * kTc, s0 = (int)(blockIdx.x / s.c_tiles) * kTs;
  {
    const int tx = threadIdx.x & (kTs - 1), ty = threadIdx.x / kTs;
    const int sp = s0 + tx;
    if (sp < s.S) {
      for (int i = ty; i < kTc && c0 + i < s.C; i += kBlock / kTs) {
        const size_t e = (size_t)(c0 + i) * s.S + sp;
        float g = grad_out[(size_t)b * s.out_stride + e];
        if (keep) g *= (float)keep[(size_t)b * s.C * s.S + e] * keep_scale;
        tile[tx][i] = g;
        wtile[tx][i] = winner ? (int)winner[(size_t)b * s.C * s.S + e] : 0;
      }
    }
  }
  __syncthreads();
  {
    const int tx = threadIdx.x & (kTc - 1), ty = threadIdx.x / kTc;
    const int c = c0 + tx;
    if (c < s.C) {
      float* gb = grad_x + (size_t)b * s.H * s.W * s.C + c;
      for (int i = ty; i < kTs && s0 + i < s.S; i += kBlock / kTc) {
        const int ho = (s0 + i) / s.Wo, wo = (s0 + i) - ho * s.Wo;
        const float g = tile[i][tx];
        const int win = wtile[i][tx];
        float* p = gb + ((size_t)ho * ph * s.W + (size_t)wo * pw) * s.C;
#pragma unroll
        for (int dh = 0; dh < ph; ++dh) {
#pragma unroll
          for (int dw = 0; dw < pw; ++dw) p[((size_t)dh * s.W + dw) * s.C] = (dh * pw + dw == win) ? g : 0.f;
        }
        // the remainder columns (floor mode drops them) belong to the last pooled column, the remainder rows to the last
        // pooled row: fewer than pw columns, fewer than ph rows
        const int w_end = (wo == s.Wo - 1) ? s.W : (wo + 1) * pw;
        for (int w = (wo + 1) * pw; w < w_end; ++w)
          for (int dh = 0; dh < ph; ++dh) gb[((size_t)(ho * ph + dh) * s.W + w) * s.C] = 0.f;
        if (ho == s.Ho - 1)
          for (int h = s.Ho * ph; h < s.H; ++h)
            for (int w = wo * pw; w < w_end; ++w) gb[((size_t)h * s.W + w) * s.C] = 0.f;
      }
    }
  }
}

template <int PH, int PW>
int launch_fwd(const float* x, const uint8_t* keep, float keep_scale, const float* extra, float* out, uint8_t* winner,
               int64_t B, const PoolShape& s, hipStream_t st) {
  const size_t per_x = (size_t)s.H * s.W * s.C, per_o = (size_t)s.C * s.S;
  for (int64_t b0 = 0; b0 < B; b0 += kPoolMaxBatchSlab) {
    const int64_t nb = B - b0 < kPoolMaxBatchSlab ? B - b0 : kPoolMaxBatchSlab;
    hipLaunchKernelGGL((pool_flatten_fwd_kernel<PH, PW>), dim3(grid_x(s), 1, (unsigned)nb), dim3(kBlock), 0, st,
                       x + b0 * per_x, keep ? keep + b0 * per_o : nullptr, keep_scale, extra ? extra + b0 : nullptr,
                       out + b0 * s.out_stride, winner ? winner + b0 * per_o : nullptr, s);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}

template <int PH, int PW>
int launch_bwd(const float* grad_out, const uint8_t* keep, float keep_scale, const uint8_t* winner, float* grad_x, int64_t B,
               const PoolShape& s, hipStream_t st) {
  const size_t per_x = (size_t)s.H * s.W * s.C, per_o = (size_t)s.C * s.S;
  for (int64_t b0 = 0; b0 < B; b0 += kPoolMaxBatchSlab) {
    const int64_t nb = B - b0 < kPoolMaxBatchSlab ? B - b0 : kPoolMaxBatchSlab;
    hipLaunchKernelGGL((pool_flatten_bwd_kernel<PH, PW>), dim3(grid_x(s), 1, (unsigned)nb), dim3(kBlock), 0, st,
                       grad_out + b0 * s.out_stride, keep ? keep + b0 * per_o : nullptr, keep_scale,
                       winner ? winner + b0 * per_o : nullptr, grad_x + b0 * per_x, s);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
  }
  return 0;
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_pool_flatten_supported(int64_t B, int64_t H, int64_t W, int64_t C, int64_t ph, int64_t pw) {
  return shape_ok(B, H, W, C, ph, pw) ? 1 : 0;
}

extern "C" int mlgnn_pool_flatten_fwd(const float* x, const uint8_t* keep, float keep_scale, const float* extra, float* out,
                                      uint8_t* winner, int64_t B, int64_t H, int64_t W, int64_t C, int64_t ph, int64_t pw,
                                      void* stream) {
  if (!shape_ok(B, H, W, C, ph, pw)) return MLGNN_E_SHAPE;
  if (B == 0) return 0;
  if (!x || !out) return MLGNN_E_NULL;
  const PoolShape s = make_shape(H, W, C, ph, pw, extra != nullptr);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (ph == 4 && pw == 2) return launch_fwd<4, 2>(x, keep, keep_scale, extra, out, winner, B, s, st);
  if (ph == 1 && pw == 1) return launch_fwd<1, 1>(x, keep, keep_scale, extra, out, winner, B, s, st);
  if (ph == 4 && pw == 1) return launch_fwd<4, 1>(x, keep, keep_scale, extra, out, winner, B, s, st);
  return launch_fwd<0, 0>(x, keep, keep_scale, extra, out, winner, B, s, st);
}

extern "C" int mlgnn_pool_flatten_bwd(const float* grad_out, const uint8_t* keep, float keep_scale, const uint8_t* winner,
                                      float* grad_x, int64_t has_extra, int64_t B, int64_t H, int64_t W, int64_t C,
                                      int64_t ph, int64_t pw, void* stream) {
  if (!shape_ok(B, H, W, C, ph, pw)) return MLGNN_E_SHAPE;
  if (B == 0) return 0;
  if (!grad_out || !grad_x || (!winner && ph * pw != 1)) return MLGNN_E_NULL;
  const PoolShape s = make_shape(H, W, C, ph, pw, has_extra != 0);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (ph == 4 && pw == 2) return launch_bwd<4, 2>(grad_out, keep, keep_scale, winner, grad_x, B, s, st);
  if (ph == 1 && pw == 1) return launch_bwd<1, 1>(grad_out, keep, keep_scale, winner, grad_x, B, s, st);
  if (ph == 4 && pw == 1) return launch_bwd<4, 1>(grad_out, keep, keep_scale, winner, grad_x, B, s, st);
  return launch_bwd<0, 0>(grad_out, keep, keep_scale, winner, grad_x, B, s, st);
}
