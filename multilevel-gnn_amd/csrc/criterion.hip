// The training criterion of the supervised models (the reference's train.py:53-61): BCELoss on the [B, 2] softmax output
// in one of four weightings, plus the pca feature loss  -coef * log(mean_m std_m)  over the batch columns of pca_feature
// seen as [B, M].  Two launches forward (one without a feature term), one backward.
//
//   bce[b, j] = -(y max(log p, -100) + (1 - y) max(log(1 - p), -100))                 ATen's clamp
//   loss_bce  = sum_{b, j} W[b, j] bce[b, j] / (2 B),    c_b = (y[b, 1] == 1)
//     plain: W = 1    class: W[b, j] = cw[b, j]    sample: W[b, j] = cw[b, c_b]    batch: W = mean_b cw[b, c_b]
//   std_m     = unbiased (B - 1) standard deviation of column m,  mean_std = sum_m std_m / M
//   loss      = loss_bce - coef log(mean_std),   terms = (loss_bce, mean_std, -coef log(mean_std))
//
// Forward 1, column statistics: a workgroup owns 256 columns, lanes run along m (every row read of a wave is one
// contiguous run: 16 bytes per lane when M % 4 == 0 and the operands are 16-byte aligned, else four 256-byte runs),
// the four waves take the rows b = w, w + 4, ...  Two passes, both on values shifted by the column's first row x_0:
// s = sum (x - x_0), then q = sum ((x - x_0) - s / B)^2 -- a constant column has s = 0 and q = 0 exactly, whatever its
// value, and nearly constant columns lose nothing to the size of their mean (E[x^2] - E[x]^2 would).  The waves' sums meet
// in LDS in wave order.  Per column the kernel may write mean_m and inv_m = 1 / ((B - 1) std_m), 0 where std_m == 0, for
// the backward; per workgroup it writes one partial sum of std, added over the 256 columns in an order that does not
// depend on the load width.
// Forward 2, one workgroup: adds the partials (thread t takes t, t + 256, ..., then lanes, then waves), forms the BCE sum
// and the batch mode's scalar weight the same way, the log, loss and terms.
// Backward, one launch: workgroup 0 writes grad_pred = g W (p - y) / max((1 - p) p, 1e-12) / (2 B) (it alone can form
// the batch mode's W); the others own a tile of columns x a run of rows of
//   grad_feat[b, m] = std_m == 0 ? 0 : g (-coef) / (M mean_std) (x - mean_m) inv_m          a select, as ATen masks it
// g and mean_std are read on the device.  No atomics, every sum in a fixed order: bitwise reproducible.
#include "bce_term.h"
#include "common.h"
#include "launch.h"
#include "mlgnn.h"

namespace mlgnn {
namespace {

constexpr int64_t kCritMaxBatch = 65536;
constexpr int kColTile = 256;              // columns per workgroup of the statistics kernel: 64 lanes x 4
constexpr int kRowsPerRun = 4;             // backward: rows a thread walks with its column statistics in registers

enum CritMode { kPlain = 0, kClass = 1, kSample = 2, kBatch = 3 };

bool shape_ok(int64_t B, int64_t M) {
  if (B < 0 || M < 0 || B > kCritMaxBatch) return false;
  if (B == 0 || M == 0) return true;                                  // an empty batch is a no-op; M == 0: no feature term
  return B >= 2 && M <= (((int64_t)1 << 30) - 1) / B;                 // B * M floats below 4 GiB
}

int64_t col_tiles(int64_t M) { return (M + kColTile - 1) / kColTile; }

struct BceArgs {
  const float* pred;
  const float* y;
  const float* cw;
  int B, mode, cw_stride;      // cw_stride: 0 for a [2] weight, 2 for [R, 2]
};

// the sum of v over the workgroup, the same in every thread: lanes (xor butterfly), then the waves in wave order
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int w = 1; w < kWavesPerBlock; ++w) t += red[w];
  __syncthreads();
  return t;
}

// batch mode: mean_b cw[b, c_b]
__device__ __forceinline__ float batch_weight(const BceArgs& a, float* red) {
  float sw = 0.f;
  for (int b = threadIdx.x; b < a.B; b += kBlock) {
    const int c = a.y[2 * b + 1] == 1.f ? 1 : 0;
    sw += a.cw[(size_t)b * a.cw_stride + c];
  }
  return block_sum(sw, red) / (float)a.B;
}

// W[b, 0], W[b, 1] of the modes that weight inside the sum (batch: 1, its scalar is applied to the mean)
__device__ __forceinline__ void row_weights(const BceArgs& a, int b, float y1, float& w0, float& w1) {
  w0 = 1.f; w1 = 1.f;
  if (a.mode == kClass) {
    w0 = a.cw[(size_t)b * a.cw_stride];
    w1 = a.cw[(size_t)b * a.cw_stride + 1];
  } else if (a.mode == kSample) {
    w0 = w1 = a.cw[(size_t)b * a.cw_stride + (y1 == 1.f ? 1 : 0)];
  }
}

// VEC == 4: lane l owns the columns c0 + 4 l .. + 3 (one 16-byte load); VEC == 1: c0 + l, + 64, + 128, + 192
template <int VEC>
__device__ __forceinline__ int tile_slot(int lane, int j) { return VEC == 4 ? lane * 4 + j : j * kWave + lane; }

template <int VEC>
__device__ __forceinline__ void load_row(float (&v)[4], const float* __restrict__ row, int c0, int lane, int M) {
  if constexpr (VEC == 4) {
    const int c = c0 + lane * 4;
    if (c < M) load_vec<4>(v, row + c);                              // M % 4 == 0: all four columns or none
    else v[0] = v[1] = v[2] = v[3] = 0.f;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j * kWave + lane;
      v[j] = c < M ? row[c] : 0.f;
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void crit_colstats_kernel(const float* __restrict__ feat, float* __restrict__ partials,
                                                              float* __restrict__ colstats, int B, int M) {
  __shared__ float red[kWavesPerBlock][kColTile];
  __shared__ float stds[kColTile];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c0 = blockIdx.x * kColTile;
  float x0[4], v[4], s[4] = {0.f, 0.f, 0.f, 0.f};
  load_row<VEC>(x0, feat, c0, lane, M);
#pragma unroll 4
  for (int b = wave; b < B; b += kWavesPerBlock) {
    load_row<VEC>(v, feat + (size_t)b * M, c0, lane, M);
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] += v[j] - x0[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[wave][tile_slot<VEC>(lane, j)] = s[j];
  __syncthreads();
  float delta[4], q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = tile_slot<VEC>(lane, j);
    delta[j] = (((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]) / (float)B;
  }
  __syncthreads();                                                   // red is written again below
#pragma unroll 4
  for (int b = wave; b < B; b += kWavesPerBlock) {
    load_row<VEC>(v, feat + (size_t)b * M, c0, lane, M);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = (v[j] - x0[j]) - delta[j];
      q[j] = fmaf(d, d, q[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[wave][tile_slot<VEC>(lane, j)] = q[j];
  __syncthreads();
  if (wave == 0) {
    float mean[4], inv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = tile_slot<VEC>(lane, j);
      const float sd = sqrtf((((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]) / (float)(B - 1));
      stds[k] = c0 + k < M ? sd : 0.f;
      mean[j] = x0[j] + delta[j];
      inv[j] = sd == 0.f ? 0.f : 1.f / ((float)(B - 1) * sd);
    }
    if (colstats) {
      if constexpr (VEC == 4) {
        const int c = c0 + lane * 4;
        if (c < M) {
          store_vec<4>(colstats + c, mean);
          store_vec<4>(colstats + (size_t)M + c, inv);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = c0 + j * kWave + lane;
          if (c < M) { colstats[c] = mean[j]; colstats[(size_t)M + c] = inv[j]; }
        }
      }
    }
  }
  __syncthreads();
  if (wave == 0) {                                                   // the tile's 256 std values by column index
    const float t = wave_sum(((stds[lane] + stds[lane + kWave]) + stds[lane + 2 * kWave]) + stds[lane + 3 * kWave]);
    if (lane == 0) partials[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(kBlock) void crit_finish_kernel(BceArgs a, const float* __restrict__ partials, int nparts, int M,
                                                            float coef, float* __restrict__ loss, float* __restrict__ terms) {
  __shared__ float red[kWavesPerBlock];
  float acc = 0.f;
  for (int b = threadIdx.x; b < a.B; b += kBlock) {
    const float p0 = a.pred[2 * b], p1 = a.pred[2 * b + 1], y0 = a.y[2 * b], y1 = a.y[2 * b + 1];
    float w0, w1;
    row_weights(a, b, y1, w0, w1);
    acc += w0 * bce_value(p0, y0) + w1 * bce_value(p1, y1);
  }
  float loss_bce = block_sum(acc, red) / (float)(2 * a.B);
  if (a.mode == kBatch) loss_bce = batch_weight(a, red) * loss_bce;
  float mean_std = 0.f, feat_term = 0.f;
  if (M > 0) {
    float ps = 0.f;
    for (int i = threadIdx.x; i < nparts; i += kBlock) ps += partials[i];
    mean_std = block_sum(ps, red) / (float)M;
    feat_term = -coef * logf(mean_std);
  }
  if (threadIdx.x == 0) {
    loss[0] = loss_bce + feat_term;
    if (terms) { terms[0] = loss_bce; terms[1] = mean_std; terms[2] = feat_term; }
  }
}

struct BwdArgs {
  const float* feat;
  const float* colstats;       // [2, M]: mean_m, inv_m
  const float* terms;          // terms[1] = mean_std
  const float* g;              // the upstream cotangent, one float
  float* grad_pred;
  float* grad_feat;
  int M, tiles, rows_per, pred_blocks;
  float coef;
};

template <int VEC>
__global__ __launch_bounds__(kBlock) void crit_bwd_kernel(BceArgs a, BwdArgs w) {
  const float g = w.g[0];
  if ((int)blockIdx.x < w.pred_blocks) {                             // workgroup 0, when grad_pred is wanted
    __shared__ float red[kWavesPerBlock];
    const float wb = a.mode == kBatch ? batch_weight(a, red) : 1.f;
    const float n = (float)(2 * a.B);
    for (int b = threadIdx.x; b < a.B; b += kBlock) {
      const float p0 = a.pred[2 * b], p1 = a.pred[2 * b + 1], y0 = a.y[2 * b], y1 = a.y[2 * b + 1];
      float w0, w1;
      row_weights(a, b, y1, w0, w1);
      w.grad_pred[2 * b] = g * (p0 - y0) / fmaxf((1.f - p0) * p0, 1e-12f) * (w0 * wb) / n;
      w.grad_pred[2 * b + 1] = g * (p1 - y1) / fmaxf((1.f - p1) * p1, 1e-12f) * (w1 * wb) / n;
    }
    return;
  }
  const int blk = (int)blockIdx.x - w.pred_blocks;
  const int tile = blk % w.tiles, run = blk / w.tiles;
  const int c = (tile * kBlock + (int)threadIdx.x) * VEC;
  if (c >= w.M) return;
  const float scale = g * -w.coef / ((float)w.M * w.terms[1]);
  float mean[VEC], inv[VEC], x[VEC], d[VEC];
  load_vec<VEC>(mean, w.colstats + c);
  load_vec<VEC>(inv, w.colstats + (size_t)w.M + c);
  const int b1 = min(a.B, (run + 1) * w.rows_per);
  for (int b = run * w.rows_per; b < b1; ++b) {
    load_vec<VEC>(x, w.feat + (size_t)b * w.M + c);
#pragma unroll
    for (int j = 0; j < VEC; ++j) d[j] = inv[j] == 0.f ? 0.f : (scale * inv[j]) * (x[j] - mean[j]);
    store_vec<VEC>(w.grad_feat + (size_t)b * w.M + c, d);
  }
}

bool weighted(int mode) { return mode == kClass || mode == kSample || mode == kBatch; }

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_criterion_supported(int64_t B, int64_t M) { return shape_ok(B, M) ? 1 : 0; }

extern "C" int64_t mlgnn_criterion_workspace(int64_t B, int64_t M) {
  if (!shape_ok(B, M)) return MLGNN_E_SHAPE;
  return B == 0 ? 0 : col_tiles(M);
}

extern "C" int mlgnn_criterion_fwd(const float* pred, const float* y, const float* class_weight, int64_t cw_rows,
                                   const float* feat, float coef, int mode, float* workspace, int64_t workspace_floats,
                                   float* colstats, float* loss, float* terms, int64_t B, int64_t M, void* stream) {
  if (!shape_ok(B, M) || cw_rows < 0) return MLGNN_E_SHAPE;
  if (mode < kPlain || mode > kBatch) return MLGNN_E_MODE;
  if (B == 0) return 0;
  if (weighted(mode) && cw_rows != 0 && cw_rows < B) return MLGNN_E_SHAPE;
  if (!pred || !y || !loss || (weighted(mode) && !class_weight) || (M > 0 && !feat)) return MLGNN_E_NULL;
  const int64_t tiles = col_tiles(M);
  if (M > 0 && (!workspace || workspace_floats < tiles)) return MLGNN_E_WORKSPACE;
  hipStream_t st = as_stream(stream);
  if (M > 0) {
    const bool vec = M % 4 == 0 && aligned(feat, colstats);
    if (vec) hipLaunchKernelGGL(crit_colstats_kernel<4>, dim3((unsigned)tiles), dim3(kBlock), 0, st, feat, workspace, colstats, (int)B, (int)M);
    else hipLaunchKernelGGL(crit_colstats_kernel<1>, dim3((unsigned)tiles), dim3(kBlock), 0, st, feat, workspace, colstats, (int)B, (int)M);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
  }
  const BceArgs a{pred, y, class_weight, (int)B, mode, cw_rows == 0 ? 0 : 2};
  hipLaunchKernelGGL(crit_finish_kernel, dim3(1), dim3(kBlock), 0, st, a, workspace, (int)tiles, (int)M, coef, loss, terms);
  return (int)hipGetLastError();
}

extern "C" int mlgnn_criterion_bwd(const float* pred, const float* y, const float* class_weight, int64_t cw_rows,
                                   const float* feat, const float* colstats, const float* terms, const float* grad_loss,
                                   float coef, int mode, float* grad_pred, float* grad_feat, int64_t B, int64_t M,
                                   void* stream) {
  if (!shape_ok(B, M) || cw_rows < 0) return MLGNN_E_SHAPE;
  if (mode < kPlain || mode > kBatch) return MLGNN_E_MODE;
  if (B == 0) return 0;
  if (weighted(mode) && cw_rows != 0 && cw_rows < B) return MLGNN_E_SHAPE;
  if (M == 0) grad_feat = nullptr;
  if (!pred || !y || !grad_loss || (weighted(mode) && !class_weight)) return MLGNN_E_NULL;
  if (grad_feat && (!feat || !colstats || !terms)) return MLGNN_E_NULL;
  if (!grad_pred && !grad_feat) return 0;
  const BceArgs a{pred, y, class_weight, (int)B, mode, cw_rows == 0 ? 0 : 2};
  BwdArgs w{feat, colstats, terms, grad_loss, grad_pred, grad_feat, (int)M, 0, 1, grad_pred ? 1 : 0, coef};
  const bool vec = M % 4 == 0 && aligned(feat, colstats, grad_feat);
  int64_t blocks = w.pred_blocks;
  if (grad_feat) {
    const int64_t per_tile = (int64_t)kBlock * (vec ? 4 : 1);
    w.tiles = (int)((M + per_tile - 1) / per_tile);
    // runs of kRowsPerRun rows, longer once that would pass kMaxBlocks workgroups
    int64_t runs = (B + kRowsPerRun - 1) / kRowsPerRun;
    const int64_t most = kMaxBlocks / w.tiles > 0 ? kMaxBlocks / w.tiles : 1;
    if (runs > most) runs = most;
    w.rows_per = (int)((B + runs - 1) / runs);
    runs = (B + w.rows_per - 1) / w.rows_per;
    blocks += runs * w.tiles;
  }
  hipStream_t st = as_stream(stream);
  if (vec) hipLaunchKernelGGL(crit_bwd_kernel<4>, dim3((unsigned)blocks), dim3(kBlock), 0, st, a, w);
  else hipLaunchKernelGGL(crit_bwd_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, st, a, w);
  return (int)hipGetLastError();
}
