// The per-pair preparation of the fold preparation's edge tests: what the reference's valid_pca_mutual_info hands to its
// estimator for a pair of nodes (s, t) -- the score of PCA(n_components=1) on the two end columns, scaled as scikit-learn's
// mutual_info_classif and mutual_info_regression scale a feature.  Shared by csrc/edge_select.hip (the classification
// estimator follows) and csrc/edge_select_cc.hip (the regression estimator follows).  Per pair, on the N training patients:
//
//   1. means of both columns, then the centred sums a = sum dx^2, b = sum dx dy, c = sum dy^2 (two passes over global
//      memory, both rows read coalesced; dx and dy stay in LDS);
//   2. the leading eigenvector v of [[a, b], [b, c]] in closed form: for b != 0, lambda = (a + c) / 2 +
//      hypot((a - c) / 2, b) and the longer of (b, lambda - a) and (lambda - c, b), normalised; for b = 0 the axis of the
//      larger variance, axis 0 on equality.  Sign: the component of larger magnitude is positive, the first on a tie
//      (scikit-learn's svd_flip(u_based_decision=False), the rule of csrc/pathway_pca.hip);
//   3. score_i = dx_i v0 + dy_i v1;
//   4. scikit-learn's scale(with_mean=False): z = score / std, the population standard deviation (two passes); a deviation
//      below 10 eps is replaced by 1 (_handle_zeros_in_scale);
//   5. the noise's amplitude 1e-10 max(1, mean|z|).
// t < 0 selects the single-column mode: score_i = x_s[i], uncentred, then steps 4 and 5.
//
// Every sum in the fixed order of block_sums.h, each with LDS scratch of its own (one barrier each).  No fused
// multiply-add: contraction is off inside the function, whatever the including file says (a product and the sum that takes
// it round separately, as in the numpy restatement of the tests).  Node indices are clamped to [0, n_nodes) (pair_list.h),
// so a wrong value cannot read outside xt.  Barriers: 2 in pair mode (means, centred sums) + 3 (mean, deviation, mean magnitude).
#pragma once
#include <math.h>

#include "block_sums.h"
#include "common.h"
#include "pair_list.h"

namespace mlgnn {

// means, centred sums, mean, deviation, magnitude
constexpr int kEdgePrepareScratchDoubles = (2 + 3 + 1 + 1 + 1) * kWavesPerBlock;

// Row `pair` of pairs [P, 2] -> key[i] = z_i for i < N; the value is the noise's amplitude, in every lane.  `key`, `lkey`:
// N doubles of LDS each (dx and dy on the way; `lkey` is free afterwards); `scratch`: kEdgePrepareScratchDoubles doubles
// of LDS.  A lane reads and writes its own positions i = tid, tid + 256, ... only, so the caller needs no barrier before
// it goes on with its own positions of `key`.  All kBlock threads call.
__device__ __forceinline__ double edge_prepare_column(const double* __restrict__ xt, const int32_t* __restrict__ pairs,
                                                      size_t pair, int N, int n_nodes, double* key, double* lkey,
                                                      double* scratch) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const double n_d = (double)N;
  const double *xs, *xq;
  const bool single = pair_rows(xt, pairs, pair, N, n_nodes, xs, xq);   // uniform over the workgroup

  // steps 1-3: key[i] = score_i
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
  return 1e-10 * (mean_mag > 1.0 ? mean_mag : 1.0);                     // numpy's maximum(1, .) apart from NaN
}

}  // namespace mlgnn
