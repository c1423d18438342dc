// Batched PCA over ragged column segments, fp64: sklearn.decomposition.PCA(svd_solver='full') for every (pathway, omics)
// segment of a fold in one launch, one workgroup of 16 waves per segment.
//
//   Xc = x[:, cols of the segment] - column means = U diag(sigma) V^T
//
// by one-sided (Hestenes) Jacobi: rotate pairs of columns of the working matrix W until all are orthogonal; the column
// norms are then the sigma, the accumulated rotation R holds the singular vectors of the other side.  W = Xc (g columns
// of length N, "tall") when g <= N and W = Xc^T (N columns of length g, "wide") otherwise, so W has m = min(N, g) <= 512
// columns of length L = max(N, g) and R is m x m.  The covariance is never formed.
//
//   tall:  v_j = R[:, j],          scores[:, j] = W[:, j]               (= Xc v_j = u_j sigma_j)
//   wide:  v_j = W[:, j] / sigma_j, scores[:, j] = R[:, j] sigma_j      (Xc^T = V diag(sigma) U^T: R accumulates U)
//
// A sweep visits all m (m - 1) / 2 pairs in round-robin order (the circle method over m rounded up to even: m' - 1 steps
// of m' / 2 disjoint pairs, the pair with the odd m's dummy column is a bye).  One wave per pair: alpha = |w_i|^2,
// beta = |w_j|^2, gamma = w_i . w_j, each lane adding its elements l, l + 64, ... in that order and the 64 lanes by an
// xor butterfly (every lane ends with the same bits); a rotation when |gamma| > 1e-15 sqrt(alpha beta) -- false for NaN,
// so a non-finite segment just stops rotating --
//   zeta = (beta - alpha) / (2 gamma),  t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)),  c = 1 / sqrt(1 + t^2),  s = c t
//   w_i' = c w_i - s w_j,  w_j' = s w_i + c w_j        (and the same on columns i, j of R)
// and a workgroup barrier between steps (the pairs of a step are disjoint, so no two waves touch one column).  The loop
// ends after the first sweep without a rotation, at most 60 sweeps.  W and R live in the caller's workspace (they stay in
// L2 at the workload's sizes: 300 x 57 doubles per segment); the workgroup is its only reader and writer.
//
// Then: sigma_j^2 = |w_j|^2 (one wave per column), wave 0 picks the k_s largest (ties to the lower column; the choice is
// the only index that depends on a value: NaN norms rank below every number and a column is picked once, so it is
// always one of [0, m)), one wave per picked component finds the entry of largest |v| (first on ties) for the sign and
// writes its column of `components`, `scores` and `variance`.  Padding columns k_s <= j < k are written as zeros first.
// No atomics, every sum in a fixed order, nothing depends on the segment's position: bitwise reproducible.
#include <math.h>

#include "common.h"
#include "launch.h"
#include "mlgnn.h"

namespace mlgnn {
namespace {

constexpr int kPcaBlock = 1024;                  // 16 waves: 16 pairs of a step at a time
constexpr int kPcaWaves = kPcaBlock / kWave;
constexpr int64_t kPcaMaxRows = 2048;            // N
constexpr int64_t kPcaMaxCols = 2048;            // g
constexpr int kPcaMaxSmall = 512;                // min(N, g): the norms of the working columns live in LDS
constexpr int kPcaMaxK = 8;
constexpr int kPcaMaxSweeps = 60;
constexpr double kPcaRotate = 1e-15;
constexpr double kPcaEps = 2.220446049250313e-16;  // 2^-52
constexpr int64_t kPcaMaxDoubles = ((int64_t)1 << 29) - 1;   // an array of doubles below 4 GiB

bool below_4gib(int64_t a, int64_t b) { return a == 0 || b <= kPcaMaxDoubles / a; }

bool pca_shape_ok(int64_t n, int64_t T, int64_t S, int64_t max_cols, int64_t k) {
  if (n < 2 || n > kPcaMaxRows || max_cols < 0 || max_cols > kPcaMaxCols || T < 0 || S < 0) return false;
  if ((n < max_cols ? n : max_cols) > kPcaMaxSmall || k < 1 || k > kPcaMaxK) return false;
  return below_4gib(n, T) && below_4gib(n * k, S) && below_4gib(k, T);
}

int64_t pca_workspace_doubles(int64_t n, int64_t T, int64_t max_cols) {
  return n * T + T * (n < max_cols ? n : max_cols);            // W of every segment, then R of every segment
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// (larger value, then lower index) over the wave; every lane ends with the winner
__device__ __forceinline__ void wave_argmax_f64(double& v, int& i) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

__global__ __launch_bounds__(kPcaBlock) void pathway_pca_kernel(
    const double* __restrict__ xt, const int32_t* __restrict__ cols, const int64_t* __restrict__ seg_ptr,
    const int32_t* __restrict__ k_seg, double* __restrict__ components, double* __restrict__ scores,
    double* __restrict__ variance, double* __restrict__ mean_out, int32_t* __restrict__ info, double* ws, int N, int F,
    int64_t T, int S, int max_cols, int k, int small_cap) {
  __shared__ double s2[kPcaMaxSmall];            // |w_j|^2
  __shared__ int rotations[kPcaWaves];
  __shared__ int picked[kPcaMaxK];
  const int s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);

  int64_t t0 = seg_ptr[s], t1 = seg_ptr[s + 1];
  t0 = t0 < 0 ? 0 : (t0 > T ? T : t0);                                  // (a malformed table stays inside [0, T])
  t1 = t1 < t0 ? t0 : (t1 > T ? T : t1);
  const int g = (int)(t1 - t0 < (int64_t)max_cols ? t1 - t0 : (int64_t)max_cols);
  const int k_most = min(min(k, N), g);
  const int ks = k_seg ? min(max((int)k_seg[s], 0), k_most) : k_most;

  // the padding columns k_s <= j < k
  const int pad = k - ks;
  for (int e = tid; e < g * pad; e += kPcaBlock) components[(size_t)(t0 + e / pad) * k + ks + e % pad] = 0.0;
  for (int e = tid; e < N * pad; e += kPcaBlock) scores[((size_t)(e / pad) * S + s) * k + ks + e % pad] = 0.0;
  if (tid < pad) variance[(size_t)s * k + ks + tid] = 0.0;
  if (g == 0) {                                                         // uniform: the whole workgroup leaves
    if (tid == 0) { info[2 * (size_t)s] = 0; info[2 * (size_t)s + 1] = 0; }
    return;
  }

  const bool tall = g <= N;
  const int m = tall ? g : N, L = tall ? N : g;                         // m <= min(N, max_cols) = small_cap <= 512
  double* W = ws + (size_t)N * t0;                                      // [m][L]
  double* R = ws + (size_t)N * T + (size_t)t0 * small_cap;              // [m][m]; m * m <= g * small_cap

  // centre: one wave per data column
  for (int t = wave; t < g; t += kPcaWaves) {
    int c = cols[t0 + t];
    c = c < 0 ? 0 : (c >= F ? F - 1 : c);
    const double* col = xt + (size_t)c * N;
    double acc = 0.0;
    for (int i = lane; i < N; i += kWave) acc += col[i];
    const double mu = wave_sum_f64(acc) / (double)N;
    if (lane == 0) mean_out[t0 + t] = mu;
    if (tall) {
      for (int i = lane; i < N; i += kWave) W[(size_t)t * L + i] = col[i] - mu;
    } else {
      for (int i = lane; i < N; i += kWave) W[(size_t)i * L + t] = col[i] - mu;
    }
  }
  for (int e = tid; e < m * m; e += kPcaBlock) R[e] = (e / m == e % m) ? 1.0 : 0.0;
  __syncthreads();

  const int half = (m + 1) >> 1, ring = 2 * half - 1;                   // m' = 2 half players, m' - 1 steps
  int sweeps = 0;
  bool converged = false;
  for (int sweep = 0; sweep < kPcaMaxSweeps; ++sweep) {
    int rotated = 0;
    for (int step = 0; step < ring; ++step) {
      for (int p = wave; p < half; p += kPcaWaves) {
        const int a = p == 0 ? ring : (step + p) % ring;
        const int b = p == 0 ? step : (step - p + ring) % ring;
        const int i = min(a, b), j = max(a, b);
        if (j >= m) continue;                                           // the bye of an odd m
        double* wi = W + (size_t)i * L;
        double* wj = W + (size_t)j * L;
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int q = lane; q < L; q += kWave) {
          const double x = wi[q], y = wj[q];
          alpha += x * x;
          beta += y * y;
          gamma += x * y;
        }
        alpha = wave_sum_f64(alpha);
        beta = wave_sum_f64(beta);
        gamma = wave_sum_f64(gamma);
        if (fabs(gamma) > kPcaRotate * sqrt(alpha * beta)) {            // wave-uniform; false for NaN
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
          for (int q = lane; q < L; q += kWave) {
            const double x = wi[q], y = wj[q];
            wi[q] = cs * x - sn * y;
            wj[q] = sn * x + cs * y;
          }
          double* ri = R + (size_t)i * m;
          double* rj = R + (size_t)j * m;
          for (int q = lane; q < m; q += kWave) {
            const double x = ri[q], y = rj[q];
            ri[q] = cs * x - sn * y;
            rj[q] = sn * x + cs * y;
          }
          ++rotated;
        }
      }
      __syncthreads();
    }
    if (lane == 0) rotations[wave] = rotated;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < kPcaWaves; ++w) total += rotations[w];
    __syncthreads();
    sweeps = sweep + 1;
    if (total == 0) { converged = true; break; }                        // uniform
  }

  for (int j = wave; j < m; j += kPcaWaves) {
    const double* wj = W + (size_t)j * L;
    double acc = 0.0;
    for (int q = lane; q < L; q += kWave) acc += wj[q] * wj[q];
    acc = wave_sum_f64(acc);
    if (lane == 0) s2[j] = acc;
  }
  __syncthreads();

  if (wave == 0) {
    int pk[kPcaMaxK];
#pragma unroll
    for (int r = 0; r < kPcaMaxK; ++r) pk[r] = -1;
    double top = 0.0;
#pragma unroll
    for (int r = 0; r < kPcaMaxK; ++r) {
      if (r < ks) {                                                     // uniform
        double bv = -2.0;
        int bi = 0x7fffffff;
        for (int j = lane; j < m; j += kWave) {
          bool taken = false;
#pragma unroll
          for (int r2 = 0; r2 < kPcaMaxK; ++r2) taken = taken || pk[r2] == j;
          const double v = s2[j];
          const double key = v == v ? v : -1.0;                         // NaN ranks below every number
          if (!taken && key > bv) { bv = key; bi = j; }                 // ascending j: the first of equals stays
        }
        wave_argmax_f64(bv, bi);
        bi = bi < 0 ? 0 : (bi >= m ? m - 1 : bi);                       // (ks <= m: some lane always holds a column)
        pk[r] = bi;
        if (r == 0) top = s2[bi];
        if (lane == 0) picked[r] = bi;
      }
    }
    if (ks == 0) {                                                      // sigma_0 for the rank all the same
      double bv = -2.0;
      int bi = 0;
      for (int j = lane; j < m; j += kWave) {
        const double v = s2[j];
        if (v > bv) { bv = v; bi = j; }
      }
      wave_argmax_f64(bv, bi);
      top = bv;
    }
    const double bound = (double)N * (double)g * kPcaEps * sqrt(top);
    int rank = 0;
    for (int j = lane; j < m; j += kWave) rank += sqrt(s2[j]) > bound ? 1 : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) rank += __shfl_xor(rank, o);
    if (lane == 0) {
      info[2 * (size_t)s] = converged ? sweeps : -1;
      info[2 * (size_t)s + 1] = rank;
    }
  }
  __syncthreads();

  for (int r = wave; r < ks; r += kPcaWaves) {
    const int q = picked[r];
    const double sig2 = s2[q], sigma = sqrt(sig2);
    const double* v = tall ? R + (size_t)q * m : W + (size_t)q * L;     // [g], up to the positive factor 1 / sigma
    const double* u = tall ? W + (size_t)q * L : R + (size_t)q * m;     // [N]
    double bv = -1.0;
    int bi = 0;
    for (int t = lane; t < g; t += kWave) {
      const double a = fabs(v[t]);
      if (a > bv) { bv = a; bi = t; }
    }
    wave_argmax_f64(bv, bi);
    bi = bi < 0 ? 0 : (bi >= g ? g - 1 : bi);
    const double sign = v[bi] < 0.0 ? -1.0 : 1.0;
    if (tall) {
      for (int t = lane; t < g; t += kWave) components[(size_t)(t0 + t) * k + r] = sign * v[t];
      for (int i = lane; i < N; i += kWave) scores[((size_t)i * S + s) * k + r] = sign * u[i];
    } else {
      for (int t = lane; t < g; t += kWave) components[(size_t)(t0 + t) * k + r] = sigma > 0.0 ? sign * v[t] / sigma : 0.0;
      for (int i = lane; i < N; i += kWave) scores[((size_t)i * S + s) * k + r] = sign * u[i] * sigma;
    }
    if (lane == 0) variance[(size_t)s * k + r] = sig2 / (double)(N - 1);
  }
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_pathway_pca_supported(int64_t n, int64_t total_cols, int64_t n_segments, int64_t max_cols, int k) {
  return pca_shape_ok(n, total_cols, n_segments, max_cols, k) ? 1 : 0;
}

extern "C" int64_t mlgnn_pathway_pca_workspace_bytes(int64_t n, int64_t total_cols, int64_t n_segments, int64_t max_cols) {
  if (!pca_shape_ok(n, total_cols, n_segments, max_cols, 1)) return MLGNN_E_SHAPE;
  return (int64_t)align256((size_t)pca_workspace_doubles(n, total_cols, max_cols) * sizeof(double));
}

extern "C" int mlgnn_pathway_pca(const double* xt, const int32_t* cols, const int64_t* seg_ptr, const int32_t* k_seg,
                                 double* components, double* scores, double* variance, double* mean, int32_t* info,
                                 void* workspace, int64_t workspace_bytes, int64_t n, int64_t n_features,
                                 int64_t total_cols, int64_t n_segments, int64_t max_cols, int k, void* stream) {
  if (!xt || !cols || !seg_ptr || !components || !scores || !variance || !mean || !info || !workspace) return MLGNN_E_NULL;
  if (!pca_shape_ok(n, total_cols, n_segments, max_cols, k) || n_features < 0 || !below_4gib(n, n_features) ||
      (total_cols > 0 && n_features < 1))
    return MLGNN_E_SHAPE;
  if (!aligned<8>(xt, seg_ptr, components, scores, variance, mean, static_cast<const char*>(workspace))) return MLGNN_E_ALIGN;
  if (workspace_bytes < mlgnn_pathway_pca_workspace_bytes(n, total_cols, n_segments, max_cols)) return MLGNN_E_WORKSPACE;
  if (total_cols == 0 || n_segments == 0) return 0;
  const int small_cap = (int)(n < max_cols ? n : max_cols);
  hipLaunchKernelGGL(pathway_pca_kernel, dim3((unsigned)n_segments), dim3(kPcaBlock), 0, as_stream(stream), xt, cols,
                     seg_ptr, k_seg, components, scores, variance, mean, info, static_cast<double*>(workspace), (int)n,
                     (int)n_features, total_cols, (int)n_segments, (int)max_cols, k, small_cap);
  return (int)hipGetLastError();
}
