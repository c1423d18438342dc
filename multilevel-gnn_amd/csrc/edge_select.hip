// The --edge_select test of the fold preparation (the reference's valid_pca_mutual_info, multiloader.py:828-874) for all
// PPI edges of a fold at once: one workgroup per PAIR of nodes, fp64 throughout.  Per pair (s, t), on the N training
// patients, what the reference computes with PCA(n_components=1) and mutual_info_classif(score, y, random_state):
//
//   1. means of both columns, then the centred sums a = sum dx^2, b = sum dx dy, c = sum dy^2 (two passes over global
//      memory, both rows read coalesced; dx and dy stay in LDS);
//   2. the leading eigenvector v of [[a, b], [b, c]] in closed form: for b != 0, lambda = (a + c) / 2 +
//      hypot((a - c) / 2, b) and the longer of (b, lambda - a) and (lambda - c, b), normalised; for b = 0 the axis of the
//      larger variance, axis 0 on equality.  Sign: the component of larger magnitude is positive, the first on a tie
//      (scikit-learn's svd_flip(u_based_decision=False), the rule of csrc/pathway_pca.hip);
//   3. score_i = dx_i v0 + dy_i v1;
//   4. scikit-learn's scale(with_mean=False): score / std, the population standard deviation (two passes); a deviation
//      below 10 eps is replaced by 1 (_handle_zeros_in_scale);
//   5. the noise: value_i = score_i / std + (1e-10 max(1, mean|score / std|)) noise_i -- ONE noise vector per fold: with
//      a fixed random_state every call of the reference seeds a fresh generator and draws the same N values;
//   6. the estimator of csrc/mutual_info_cd.h on that column.
// t < 0 selects the single-column mode: score_i = x_s[i], uncentred, then steps 4-6: the end-node value
// mutual_info_classif(column[:, None], y, random_state).
//
// Every sum in the fixed order of the other kernels: a lane adds its positions i = t, t + 256, ... in that order, then
// the 64 lanes of a wave (xor butterfly), then the four waves in wave order; every reduction has LDS scratch of its own,
// so each costs one barrier.  No atomics, no fused multiply-add (contraction is off in this file: a product and the sum
// that takes it round separately, as in the numpy restatement of the tests): bitwise reproducible, and a pair's bits do
// not depend on the other pairs.  Node indices are clamped to [0, n_nodes), so a wrong value cannot read outside xt; no
// other index depends on a value (mutual_info_cd.h).
//
// LDS: 24 NP bytes of the column (mutual_info_cd.h; dx lies in `key` and dy in `lkey` until the score replaces them) +
// 288 of static reduction scratch: 49 440 bytes at N = 2048, 12 576 at N = 300.  Barriers: 2 in pair mode (means,
// centred sums) + 3 (mean, deviation, mean magnitude of the score) before the estimator's own.
#include <math.h>

#include "block_sums.h"
#include "common.h"
#include "launch.h"
#include "mlgnn.h"
#include "mutual_info_cd.h"

#pragma clang fp contract(off)

namespace mlgnn {
namespace {

bool shape_ok(int64_t n, int64_t n_nodes, int64_t P, int64_t k, int64_t n_labels, bool with_score) {
  if (n < 2 || n > kMiMaxSamples || k < 1 || n_labels < 1 || n_labels > n) return false;
  const int64_t most = (((int64_t)1 << 29) - 1) / n;                    // rows of N doubles below 4 GiB
  if (n_nodes < 0 || n_nodes > most || P < 0 || P >= ((int64_t)1 << 31)) return false;
  if (P > 0 && n_nodes < 1) return false;
  return !with_score || P <= most;
}

constexpr int kScratchDoubles = (2 + 3 + 1 + 1 + 1) * kWavesPerBlock;   // means, centred sums, mean, deviation, magnitude

__global__ __launch_bounds__(kBlock) void edge_mi_kernel(const double* __restrict__ xt, const int32_t* __restrict__ pairs,
                                                        const double* __restrict__ noise,
                                                        const int32_t* __restrict__ labels, const double* __restrict__ psi,
                                                        double base, double* __restrict__ mi, double* __restrict__ score,
                                                        int32_t* __restrict__ counts, int N, int NP, int n_nodes, int k,
                                                        int n_labels) {
  extern __shared__ double lds[];
  __shared__ double scratch[kScratchDoubles];
  __shared__ double red[kWavesPerBlock];
  const MiColumn col = mi_column(lds, NP);
  double* key = col.key;
  double* lkey = col.lkey;
  const int tid = threadIdx.x;
  const size_t pair = blockIdx.x;
  const double n_d = (double)N;
  int s = pairs[2 * pair], t = pairs[2 * pair + 1];
  const bool single = t < 0;                                            // uniform over the workgroup
  s = min(max(s, 0), n_nodes - 1);
  t = single ? s : min(t, n_nodes - 1);
  const double* xs = xt + (size_t)s * N;
  const double* xq = xt + (size_t)t * N;

  // steps 1-3: key[i] = score_i.  A lane reads and writes its own positions i = tid, tid + 256, ... only.
  if (single) {
    for (int i = tid; i < N; i += kBlock) key[i] = xs[i];
  } else {
    double m[2] = {0.0, 0.0};
    for (int i = tid; i < N; i += kBlock) {
      m[0] += xs[i];
      m[1] += xq[i];
    }
    block_sums(m, scratch);
    const double mx = m[0] / n_d, my = m[1] / n_d;
    double q[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < N; i += kBlock) {
      const double dx = xs[i] - mx, dy = xq[i] - my;
      key[i] = dx;
      lkey[i] = dy;
      q[0] += dx * dx;
      q[1] += dx * dy;
      q[2] += dy * dy;
    }
    block_sums(q, scratch + 2 * kWavesPerBlock);
    const double a = q[0], b = q[1], c = q[2];
    double v0, v1;
    if (b != 0.0) {
      const double lambda = (a + c) / 2.0 + hypot((a - c) / 2.0, b);
      const double u0 = b, u1 = lambda - a, w0 = lambda - c, w1 = b;
      const double nu = hypot(u0, u1), nw = hypot(w0, w1);
      if (nw > nu) { v0 = w0 / nw; v1 = w1 / nw; } else { v0 = u0 / nu; v1 = u1 / nu; }
    } else {
      v0 = a >= c ? 1.0 : 0.0;
      v1 = 1.0 - v0;
    }
    if (fabs(v0) >= fabs(v1) ? v0 < 0.0 : v1 < 0.0) { v0 = -v0; v1 = -v1; }
    for (int i = tid; i < N; i += kBlock) key[i] = key[i] * v0 + lkey[i] * v1;
  }

  // step 4: the population standard deviation of the score, two passes
  double sum[1] = {0.0};
  for (int i = tid; i < N; i += kBlock) sum[0] += key[i];
  block_sums(sum, scratch + 5 * kWavesPerBlock);
  const double mean = sum[0] / n_d;
  double dev[1] = {0.0};
  for (int i = tid; i < N; i += kBlock) {
    const double d = key[i] - mean;
    dev[0] += d * d;
  }
  block_sums(dev, scratch + 6 * kWavesPerBlock);
  double sd = sqrt(dev[0] / n_d);
  if (sd < 10.0 * 2.220446049250313e-16) sd = 1.0;                      // (a NaN stays)
  // step 5: the noise's scale from the mean magnitude of the scaled score
  double mag[1] = {0.0};
  for (int i = tid; i < N; i += kBlock) {
    const double z = key[i] / sd;
    key[i] = z;
    mag[0] += fabs(z);
  }
  block_sums(mag, scratch + 7 * kWavesPerBlock);
  const double mean_mag = mag[0] / n_d;
  const double amp = 1e-10 * (mean_mag > 1.0 ? mean_mag : 1.0);        // numpy's maximum(1, .) apart from NaN
  const double inf = __builtin_huge_val();
  for (int i = tid; i < NP; i += kBlock) {
    double v = inf;
    uint32_t tg = kMiPadTag;
    if (i < N) {
      v = key[i] + amp * noise[i];
      tg = mi_tag(labels[i], n_labels, i);
      if (score) score[pair * N + i] = v;
    }
    key[i] = v;
    lkey[i] = v;
    col.tag[i] = tg;
  }
  // step 6
  const double v = mi_cd_estimate(col, red, psi, base, counts ? counts + pair * N : nullptr, N, NP, k);
  if (tid == 0) mi[pair] = v;
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_edge_mi_supported(int64_t n, int64_t n_nodes, int64_t n_pairs, int k, int n_labels, int with_score) {
  return shape_ok(n, n_nodes, n_pairs, k, n_labels, with_score != 0) ? 1 : 0;
}

extern "C" int mlgnn_edge_mi(const double* xt, const int32_t* pairs, const double* noise, const int32_t* labels,
                             const double* psi, double base, double* mi, double* score, int32_t* counts, int64_t n,
                             int64_t n_nodes, int64_t n_pairs, int k, int n_labels, void* stream) {
  if (!xt || !pairs || !noise || !labels || !psi || !mi) return MLGNN_E_NULL;
  if (!shape_ok(n, n_nodes, n_pairs, k, n_labels, score != nullptr)) return MLGNN_E_SHAPE;
  if (n_pairs == 0) return 0;
  const int NP = mi_pow2_at_least(n);
  const size_t bytes = (size_t)NP * 24;                                // at most 48 KiB: below the default limit
  hipLaunchKernelGGL(edge_mi_kernel, dim3((unsigned)n_pairs), dim3(kBlock), bytes, as_stream(stream), xt, pairs, noise,
                     labels, psi, base, mi, score, counts, (int)n, NP, (int)n_nodes, k, n_labels);
  return (int)hipGetLastError();
}
