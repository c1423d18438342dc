// The evaluation pass of the training loop (the reference's train.py:71-109, and the pooled scores of :338-356): the mean
// BCE loss of the batches, the accuracy and scikit-learn's roc_auc_score of R independent rows -- a row is one split, or
// one pooled prediction vector -- in ONE launch, one workgroup per row, no host step.
//
//   label t_i = (y[i, 0] >= 0.5),  score s_i = pred[i, 0],  decision (s_i > 0.5)
//   acc  = #{(s_i > 0.5) == t_i} / n
//   loss = mean over the row's batches, in batch order, of  fp32(sum over the batch's 2 n_b elements of bce / (2 n_b))
//          (csrc/bce_term.h: ATen's clamped term in fp32; the sums in fp64)
//   auc  = num / den, one IEEE division of exact integers:
//          num = sum over negatives j of (2 #{positives with s > s_j} + #{positives with s == s_j}),  den = 2 P N_neg
//          -- the trapezoid area under the ROC curve over distinct thresholds, ties sharing one, times den.
//
// Phases of a workgroup (NP = the launch's padded row length, a power of two >= 64 chosen from n_max):
// 1. every sample's two BCE terms, as one double, into LDS; the counts (positives, correct, non-finite scores) and the
//    sort key of each sample stay in registers.  key = ((ord(s) + 1) << 1) | t with ord the order-preserving map of the
//    float's bits to uint32 after -0.0 became +0.0 (one threshold); 0 pads the row behind every real key.
// 2. loss: wave w takes the batches w, w + 4, ...: lanes add the batch's doubles lane, lane + 64, ... in that order, an
//    xor butterfly joins them, the batch value is rounded to fp32 as torch's is, and the wave adds its batch values in
//    batch order; the four waves meet through block_sums (csrc/block_sums.h).
// 3. the keys replace the terms in LDS and are sorted descending by the bitonic network of csrc/mutual_info_cd.h (thread
//    t owns the pairs (i, i | j)).  Not stable; num does not depend on the order inside a tie group.
// 4. prefix counts of positives along the sorted order (a chunk per thread, a shuffle scan per wave, the waves in wave
//    order), then every negative finds by two binary searches the first position whose score is not above its own and
//    the first below it: the two counts are differences of the prefix array.
// Integer sums: xor butterfly, then the waves through LDS.  No float atomics, every float sum in a fixed order: bitwise
// reproducible.  Every row, batch and sample index is clamped to its range before it is used, so no address depends on
// what the pointer arrays or the scores hold; a row longer than NP (n_max understated) is cut at NP.
#include "bce_term.h"
#include "block_sums.h"
#include "common.h"
#include "launch.h"
#include "mlgnn.h"
#include "mutual_info_cd.h"

namespace mlgnn {
namespace {

constexpr int64_t kEvalMaxRows = 65536;
constexpr int64_t kEvalMaxSamples = kMiMaxSamples;               // 2048: the longest row
constexpr int kEvalMinPad = 64;
using EvalPads = IntList<64, 128, 256, 512, 1024, 2048>;

bool eval_shape(int64_t R, int64_t n_max, int64_t n_total, int64_t n_batches) {
  if (R < 1 || R > kEvalMaxRows || n_max < 0 || n_max > kEvalMaxSamples) return false;
  if (n_total < 0 || n_total > R * n_max) return false;           // (R n_max <= 2^27)
  return n_batches >= 0 && n_batches <= n_total;
}

int eval_pad(int64_t n_max) {
  const int p = mi_pow2_at_least(n_max);
  return p < kEvalMinPad ? kEvalMinPad : p;
}

__device__ __forceinline__ int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// descending order of the keys = descending order of the scores; -0.0 and +0.0 share a key
__device__ __forceinline__ uint64_t eval_key(float s, bool positive) {
  uint32_t b = __float_as_uint(s);
  if ((b << 1) == 0) b = 0;                                        // -0.0 -> +0.0
  const uint32_t ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (((uint64_t)ord + 1) << 1) | (positive ? 1u : 0u);
}

// the sum of v over the workgroup, in every thread (integers: any order gives the same value)
__device__ __forceinline__ long long block_count(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  const long long t = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return t;
}

template <int NP>
__global__ __launch_bounds__(kBlock) void eval_metrics_kernel(
    const float2* __restrict__ pred, const float2* __restrict__ y, const int32_t* __restrict__ row_ptr,
    const int32_t* __restrict__ batch_ptr, const int32_t* __restrict__ row_batch_ptr, int n_total, int n_batches,
    double* __restrict__ out_f64, long long* __restrict__ out_i64) {
  constexpr int kPer = (NP + kBlock - 1) / kBlock;                 // samples per thread
  constexpr int kChunk = NP / kBlock > 0 ? NP / kBlock : 1;       // sorted positions per thread of the prefix count
  __shared__ uint64_t buf[NP];                                     // the BCE terms (doubles), then the sort keys
  __shared__ int ppos[NP + 1];                                     // positives in the sorted positions [0, i)
  __shared__ double red_f[kWavesPerBlock];
  __shared__ long long red_i[kWavesPerBlock];
  __shared__ int wave_total[kWavesPerBlock];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int r = blockIdx.x;
  const int r0 = clamp_int(row_ptr[r], 0, n_total);
  const int n = min(clamp_int(row_ptr[r + 1], r0, n_total) - r0, NP);
  const int b0 = clamp_int(row_batch_ptr[r], 0, n_batches);
  const int b1 = clamp_int(row_batch_ptr[r + 1], b0, n_batches);

  // 1. terms, counts, keys
  double* term = reinterpret_cast<double*>(buf);
  uint64_t key[kPer];
  int pos = 0, correct = 0, nonfinite = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int i = tid + q * kBlock;
    key[q] = 0;
    if (i < n) {
      const float2 p = pred[(size_t)r0 + i], t = y[(size_t)r0 + i];
      term[i] = (double)bce_value(p.x, t.x) + (double)bce_value(p.y, t.y);
      const bool positive = t.x >= 0.5f;
      pos += positive ? 1 : 0;
      correct += ((p.x > 0.5f) == positive) ? 1 : 0;
      nonfinite += (fabsf(p.x) < INFINITY) ? 0 : 1;                // NaN compares false
      key[q] = eval_key(p.x, positive);
    }
  }
  const int n_pos = (int)block_count(pos, red_i);                  // (its barriers publish the terms)
  const int n_correct = (int)block_count(correct, red_i);
  const int n_nonfinite = (int)block_count(nonfinite, red_i);

  // 2. the mean of the batch means
  double wacc[1] = {0.0};
  for (int b = b0 + wave; b < b1; b += kWavesPerBlock) {
    const int s = clamp_int(batch_ptr[b], r0, r0 + n) - r0;
    const int e = clamp_int(batch_ptr[b + 1], r0 + s, r0 + n) - r0;
    double sum = 0.0;
    for (int i = s + lane; i < e; i += kWave) sum += term[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    const float batch_loss = (float)(sum / (double)(2 * (e - s)));  // an empty batch: NaN, as torch's mean
    if (lane == 0) wacc[0] += (double)batch_loss;
  }
  block_sums<1>(wacc, red_f);                                       // lanes 1..63 hold 0; (its barrier ends the term reads)
  const double loss = wacc[0] / (double)(b1 - b0);

  // 3. sort the keys, descending
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int i = tid + q * kBlock;
    if (i < NP) buf[i] = key[q];
  }
  __syncthreads();
  for (int kk = 2; kk <= NP; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (NP >> 1); t += kBlock) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int p = i | j;
        const bool down = (i & kk) == 0;
        const uint64_t a = buf[i], b = buf[p];
        if (down ? a < b : b < a) { buf[i] = b; buf[p] = a; }
      }
      __syncthreads();
    }
  }

  // 4. prefix counts of positives, then the negatives' two searches
  {
    const int first = tid * kChunk;
    int c = 0;
    if (first < NP) {
#pragma unroll
      for (int k = 0; k < kChunk; ++k) c += (int)(buf[first + k] & 1u);
    }
    int inc = c;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int v = __shfl_up(inc, o);
      if (lane >= o) inc += v;
    }
    if (lane == kWave - 1) wave_total[wave] = inc;
    __syncthreads();
    int run = inc - c;
    for (int w = 0; w < wave; ++w) run += wave_total[w];
    if (first < NP) {
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        ppos[first + k] = run;
        run += (int)(buf[first + k] & 1u);
      }
      if (first + kChunk == NP) ppos[NP] = run;
    }
    __syncthreads();
  }
  long long num = 0;
  for (int i = tid; i < n; i += kBlock) {
    const uint64_t k = buf[i];
    if (k & 1u) continue;
    const uint64_t sk = k >> 1;
    int a = 0, len = n;                                             // first a with score[a] <= s
    while (len > 0) {
      const int h = len >> 1;
      if ((buf[a + h] >> 1) > sk) { a += h + 1; len -= h + 1; } else { len = h; }
    }
    int b = a;                                                      // first b with score[b] < s
    len = n - a;
    while (len > 0) {
      const int h = len >> 1;
      if ((buf[b + h] >> 1) >= sk) { b += h + 1; len -= h + 1; } else { len = h; }
    }
    num += (long long)(ppos[a] + ppos[b]);                          // 2 ppos[a] + (ppos[b] - ppos[a])
  }
  num = block_count(num, red_i);

  if (tid == 0) {
    const long long den = 2ll * n_pos * (n - n_pos);
    const double nan = __builtin_nan("");
    double* f = out_f64 + (size_t)r * 3;
    long long* o = out_i64 + (size_t)r * 6;
    f[0] = (den == 0 || n_nonfinite > 0) ? nan : (double)num / (double)den;
    f[1] = n == 0 ? nan : (double)n_correct / (double)n;
    f[2] = (n == 0 || b1 == b0) ? nan : loss;
    o[0] = n; o[1] = n_pos; o[2] = n_correct; o[3] = n_nonfinite; o[4] = num; o[5] = den;
  }
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_eval_metrics_supported(int64_t R, int64_t n_max, int64_t n_total, int64_t n_batches) {
  return eval_shape(R, n_max, n_total, n_batches) ? 1 : 0;
}

extern "C" int64_t mlgnn_eval_metrics_workspace_bytes(int64_t R, int64_t n_max, int64_t n_total, int64_t n_batches) {
  return eval_shape(R, n_max, n_total, n_batches) ? 0 : MLGNN_E_SHAPE;
}

extern "C" int mlgnn_eval_metrics(const float* pred, const float* y, const int32_t* row_ptr, const int32_t* batch_ptr,
                                  const int32_t* row_batch_ptr, int64_t R, int64_t n_max, int64_t n_total,
                                  int64_t n_batches, double* out_f64, int64_t* out_i64, void* work, int64_t work_bytes,
                                  void* stream) {
  if (!pred || !y || !row_ptr || !batch_ptr || !row_batch_ptr || !out_f64 || !out_i64) return MLGNN_E_NULL;
  if (!eval_shape(R, n_max, n_total, n_batches)) return MLGNN_E_SHAPE;
  if (!aligned<8>(pred, y, out_f64, out_i64) || !aligned<4>(row_ptr, batch_ptr, row_batch_ptr)) return MLGNN_E_ALIGN;
  if (work_bytes < 0) return MLGNN_E_WORKSPACE;                     // the op needs none; `work` may be NULL
  (void)work;
  hipStream_t st = as_stream(stream);
  const bool launched = EvalPads::dispatch(eval_pad(n_max), [&](auto np) {
    hipLaunchKernelGGL(eval_metrics_kernel<decltype(np)::value>, dim3((unsigned)R), dim3(kBlock), 0, st,
                       reinterpret_cast<const float2*>(pred), reinterpret_cast<const float2*>(y), row_ptr, batch_ptr,
                       row_batch_ptr, (int)n_total, (int)n_batches, out_f64, reinterpret_cast<long long*>(out_i64));
  });
  if (!launched) return MLGNN_E_SHAPE;
  return (int)hipGetLastError();
}
