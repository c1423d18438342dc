// The log-rank screen of the reference's utils/km_util.py (draw_kmfit :63-105, draw_kmfit_by_group :117-129): R rows of
// per-patient scores over ONE cohort of n patients, each row split at its median (or at the caller's threshold) into two
// groups that are compared by the log-rank test and, on request, described by their Kaplan-Meier curves -- in ONE launch,
// one workgroup per row, fp64, no host step.
//
// Shared by all rows (the host prepares it once per call, mlgnn/survival.py survival_table): the stable ascending order of
// the times (`order`), the events in that order (`event_sorted`), the M distinct times as group_start [M + 1] into that
// order, and deaths [M], the events at each distinct time (0 for a censored-only time).
//
// Phases of a workgroup (NP = the launch's padded cohort size, a power of two >= 64 chosen from n):
// 1. the row's n scores as doubles into LDS, +inf behind them; the non-finite ones are counted.
// 2. no caller threshold: the bitonic network of csrc/mutual_info_cd.h sorts them ascending, and the threshold is
//    numpy.median: the middle value (n odd) or (a + b) / 2 of the two middle values (n even).
// 3. along the time order, flag = (score < threshold) and flag & event, packed as one int (flag | (flag & event) << 16:
//    both sums stay below 2^16), get an exclusive prefix sum -- a chunk per thread, a shuffle scan per wave, the waves in
//    wave order -- into LDS, over the sort buffer, which nobody reads any more.
// 4. thread t takes the distinct times j = t, t + 256, ...:  n_j = n - group_start[j],  n1_j = N1 - prefix(group_start[j]),
//    d_j = deaths[j], d1_j = a difference of the event prefix, and adds
//       E term  d_j n1_j / n_j                                              one division of two exact integers
//       V term  d_j n1_j (n_j - n1_j) (n_j - d_j) / (n_j^2 (n_j - 1))       likewise (numerator < 2^44, denominator < 2^33)
//    in that order of j (0 where d_j = 0, and the V term where n_j = 1); block_sums (csrc/block_sums.h) joins the lanes
//    and the waves in its fixed order.  chi2 = (O1 - E1)^2 / V, NaN when V is not positive.
// 5. want_km: S_g(t_j) = prod_{i <= j} (n_gi - d_gi) / n_gi for both groups (the factor is 1 where n_gi = 0), every factor
//    one division of two exact integers, as a prefix product: a chunk per thread in order, a shuffle scan per wave, the
//    waves in wave order.  However the product is bracketed, element j carries j + 1 divisions and j multiplications.
// No float atomics, every float sum and product in a fixed order: bitwise reproducible, and a row's bits do not depend
// on the other rows of the launch.  Every index read from a table is clamped to its range before it is used, so no
// address depends on what the tables or the scores hold.
#include "block_sums.h"
#include "common.h"
#include "launch.h"
#include "mlgnn.h"
#include "mutual_info_cd.h"

namespace mlgnn {
namespace {

constexpr int64_t kScreenMaxRows = 65536;
constexpr int64_t kScreenMaxPatients = kMiMaxSamples;              // 2048
constexpr int64_t kScreenMaxStride = (int64_t)1 << 31;             // (so the span of the scores stays below 2^48 elements)
constexpr int kScreenMinPad = 64;
using ScreenPads = IntList<64, 128, 256, 512, 1024, 2048>;

bool screen_shape(int64_t R, int64_t n, int64_t M, int want_km) {
  return R >= 1 && R <= kScreenMaxRows && n >= 1 && n <= kScreenMaxPatients && M >= 1 && M <= n &&
         (want_km == 0 || want_km == 1);
}

int screen_pad(int64_t n) {
  const int p = mi_pow2_at_least(n);
  return p < kScreenMinPad ? kScreenMinPad : p;
}

__device__ __forceinline__ int clamp_index(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ double load_score(const void* __restrict__ scores, bool f64, long long at) {
  return f64 ? static_cast<const double*>(scores)[at] : (double)static_cast<const float*>(scores)[at];
}

// the sum of v over the workgroup, in every thread (integers: any order gives the same value)
__device__ __forceinline__ long long screen_count(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  const long long t = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return t;
}

template <int NP>
__global__ __launch_bounds__(kBlock) void survival_screen_kernel(
    const void* __restrict__ scores, int score_is_f64, long long row_stride, long long patient_stride,
    const int32_t* __restrict__ order, const int32_t* __restrict__ event_sorted, const int32_t* __restrict__ group_start,
    const int32_t* __restrict__ deaths, const double* __restrict__ threshold, int n, int M, int want_km,
    double* __restrict__ out_f64, long long* __restrict__ out_i64, double* __restrict__ km) {
  constexpr int kPer = (NP + kBlock - 1) / kBlock;                 // scores per thread
  constexpr int kChunk = NP / kBlock > 0 ? NP / kBlock : 1;       // time-order positions (distinct times) per thread
  static_assert(4 * (NP + 1) <= 8 * NP, "the prefix array lies over the sort buffer");
  __shared__ double buf[NP];                                       // the scores, sorted; then the packed prefix sums
  __shared__ double red_f[2 * kWavesPerBlock];
  __shared__ long long red_i[kWavesPerBlock];
  __shared__ int wave_total[kWavesPerBlock];
  __shared__ double wave_prod[2][kWavesPerBlock];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int r = blockIdx.x;
  const bool f64 = score_is_f64 != 0;
  const long long row_at = (long long)r * row_stride;
  const double inf = __builtin_huge_val();

  // 1. the scores
  int nonfinite = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int i = tid + q * kBlock;
    if (i < NP) {
      double v = inf;
      if (i < n) {
        v = load_score(scores, f64, row_at + (long long)i * patient_stride);
        nonfinite += (fabs(v) < inf) ? 0 : 1;                      // NaN compares false
      }
      buf[i] = v;
    }
  }
  const int n_nonfinite = (int)screen_count(nonfinite, red_i);    // (its barriers publish the scores)

  // 2. the threshold
  double thr;
  if (threshold != nullptr) {
    thr = threshold[r];
  } else {
    for (int kk = 2; kk <= NP; kk <<= 1) {
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (NP >> 1); t += kBlock) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int p = i | j;
          const bool up = (i & kk) == 0;
          const double a = buf[i], b = buf[p];
          if (up ? b < a : a < b) { buf[i] = b; buf[p] = a; }
        }
        __syncthreads();
      }
    }
    thr = (n & 1) ? buf[(n - 1) >> 1] : (buf[(n >> 1) - 1] + buf[n >> 1]) / 2.0;
  }

  // 3. exclusive prefix sums of flag | (flag & event) << 16 along the time order
  int* prefix = reinterpret_cast<int*>(buf);                       // [NP + 1]
  int total;
  {
    const int first = tid * kChunk;
    int fl[kChunk];
    int c = 0;
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int p = first + k;
      int f = 0;
      if (p < n) {
        const int patient = clamp_index(order[p], 0, n - 1);
        const double s = load_score(scores, f64, row_at + (long long)patient * patient_stride);
        const int g1 = s < thr ? 1 : 0;
        f = g1 | ((g1 & (event_sorted[p] != 0 ? 1 : 0)) << 16);
      }
      fl[k] = f;
      c += f;
    }
    int inc = c;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int v = __shfl_up(inc, o);
      if (lane >= o) inc += v;
    }
    if (lane == kWave - 1) wave_total[wave] = inc;
    __syncthreads();                                               // (every thread has read its threshold from buf)
    int run = inc - c;
    for (int w = 0; w < wave; ++w) run += wave_total[w];
    if (first < NP) {
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        prefix[first + k] = run;
        run += fl[k];
      }
      if (first + kChunk == NP) prefix[NP] = run;
    }
    __syncthreads();
    total = prefix[NP];
  }
  const int N1 = total & 0xffff, O1 = total >> 16;

  // 4. the log-rank terms, and 5. the curve factors of this thread's distinct times
  double acc[2] = {0.0, 0.0};
  long long all_deaths = 0;
  for (int j = tid; j < M; j += kBlock) {
    const int a = clamp_index(group_start[j], 0, n);
    const int pa = prefix[a];
    const long long nj = n - a, n1 = N1 - (pa & 0xffff);
    const long long d = deaths[j];
    all_deaths += d;
    if (d > 0 && nj >= 1) {
      acc[0] += (double)(d * n1) / (double)nj;
      if (nj > 1) acc[1] += (double)(d * n1 * (nj - n1) * (nj - d)) / (double)(nj * nj * (nj - 1));
    }
  }
  block_sums<2>(acc, red_f);
  all_deaths = screen_count(all_deaths, red_i);

  if (want_km && km != nullptr) {
    const int first = tid * kChunk;
    double pr[2][kChunk];
    double c[2] = {1.0, 1.0};
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int j = first + k;
      double fac[2] = {1.0, 1.0};
      if (j < M) {
        const int a = clamp_index(group_start[j], 0, n);
        const int b = clamp_index(group_start[j + 1], a, n);
        const int pa = prefix[a], pb = prefix[b];
        const int nj = n - a, n1 = N1 - (pa & 0xffff);
        const int d = deaths[j], d1 = (pb >> 16) - (pa >> 16);
        const int ng[2] = {n1, nj - n1}, dg[2] = {d1, d - d1};
#pragma unroll
        for (int g = 0; g < 2; ++g) fac[g] = ng[g] > 0 ? (double)(ng[g] - dg[g]) / (double)ng[g] : 1.0;
      }
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        c[g] *= fac[g];                                            // (times 1.0 is exact)
        pr[g][k] = c[g];
      }
    }
    double before[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      double inc = c[g];
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const double v = __shfl_up(inc, o);
        if (lane >= o) inc = v * inc;
      }
      if (lane == kWave - 1) wave_prod[g][wave] = inc;
      const double prev = __shfl_up(inc, 1);
      before[g] = lane > 0 ? prev : 1.0;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      double lead = 1.0;
      for (int w = 0; w < wave; ++w) lead *= wave_prod[g][w];
      const double start = lead * before[g];
      double* out = km + ((size_t)r * 2 + g) * (size_t)M;
#pragma unroll
      for (int k = 0; k < kChunk; ++k) {
        const int j = first + k;
        if (j < M) out[j] = start * pr[g][k];
      }
    }
  }

  if (tid == 0) {
    const double e1 = acc[0], v = acc[1];
    const double diff = (double)O1 - e1;
    double* f = out_f64 + (size_t)r * 4;
    long long* o = out_i64 + (size_t)r * 5;
    f[0] = thr;
    f[1] = e1;
    f[2] = v;
    f[3] = v > 0.0 ? diff * diff / v : __builtin_nan("");
    o[0] = N1;
    o[1] = n - N1;
    o[2] = O1;
    o[3] = all_deaths - O1;
    o[4] = n_nonfinite;
  }
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_survival_screen_supported(int64_t R, int64_t n, int64_t M, int want_km) {
  return screen_shape(R, n, M, want_km) ? 1 : 0;
}

extern "C" int64_t mlgnn_survival_screen_workspace_bytes(int64_t R, int64_t n, int64_t M, int want_km) {
  return screen_shape(R, n, M, want_km) ? 0 : MLGNN_E_SHAPE;
}

extern "C" int mlgnn_survival_screen(const void* scores, int score_is_f64, int64_t row_stride, int64_t patient_stride,
                                     const int32_t* order, const int32_t* event_sorted, const int32_t* group_start,
                                     const int32_t* deaths, const double* threshold, int64_t R, int64_t n, int64_t M,
                                     int want_km, double* out_f64, int64_t* out_i64, double* km, void* work,
                                     int64_t work_bytes, void* stream) {
  if (!scores || !order || !event_sorted || !group_start || !deaths || !out_f64 || !out_i64 || (want_km && !km))
    return MLGNN_E_NULL;
  if (!screen_shape(R, n, M, want_km)) return MLGNN_E_SHAPE;
  if (row_stride < 0 || row_stride >= kScreenMaxStride || patient_stride < 0 || patient_stride >= kScreenMaxStride)
    return MLGNN_E_SHAPE;
  if (score_is_f64 != 0 && score_is_f64 != 1) return MLGNN_E_DTYPE;
  if (!(score_is_f64 ? aligned<8>(scores) : aligned<4>(scores)) || !aligned<8>(threshold, out_f64, out_i64, km) ||
      !aligned<4>(order, event_sorted, group_start, deaths))
    return MLGNN_E_ALIGN;
  if (work_bytes < 0) return MLGNN_E_WORKSPACE;                     // the op needs none; `work` may be NULL
  (void)work;
  hipStream_t st = as_stream(stream);
  const bool launched = ScreenPads::dispatch(screen_pad(n), [&](auto np) {
    hipLaunchKernelGGL(survival_screen_kernel<decltype(np)::value>, dim3((unsigned)R), dim3(kBlock), 0, st, scores,
                       score_is_f64, (long long)row_stride, (long long)patient_stride, order, event_sorted, group_start,
                       deaths, threshold, (int)n, (int)M, want_km, out_f64, reinterpret_cast<long long*>(out_i64), km);
  });
  if (!launched) return MLGNN_E_SHAPE;
  return (int)hipGetLastError();
}
