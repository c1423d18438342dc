// The --edge_select test of the fold preparation under mutual_info_regression -- the reference's default: its
// valid_pca_mutual_info (multiloader.py:828-874) with mutual_classif false -- for all PPI edges of a fold at once: one
// workgroup per PAIR of nodes, fp64 throughout.  Per pair (s, t), on the N training patients, what the reference computes
// with PCA(n_components=1) and mutual_info_regression(score, y):
//
//   1.-5. the preparation of edge_prepare.h: the score of the pair's closed-form 2 x 2 PCA with scikit-learn's sign rule,
//      scale(with_mean=False) -> z, and the noise's amplitude 1e-10 max(1, mean|z|);
//   the noise: value_i = z_i + amplitude noise_x[i] -- ONE feature-noise vector per launch: with a fixed random_state
//      every call of the reference seeds a fresh generator, draws the same N values for its single feature and then the
//      same N for the target, so the prepared target y_prepared comes from the host and is the same for every pair;
//   6. the estimator of csrc/mutual_info_cc.h on that column against y_prepared.
// t < 0 selects the single-column mode: score_i = x_s[i], uncentred, then steps 4-6: the end-node value
// mutual_info_regression(column[:, None], y).
//
// The preparation runs in two of the estimator's LDS arrays, which are free until its sort: dx and z in `xs`, dy in `yx`.
// Every sum in the fixed order of block_sums.h; no atomics, no fused multiply-add (contraction is off in this file and in
// edge_prepare.h): bitwise reproducible, and a pair's bits do not depend on the other pairs.  Node indices are clamped to
// [0, n_nodes), so a wrong value cannot read outside xt; no other index depends on a value (mutual_info_cc.h).
//
// LDS: 28 NP + 8 k kBlock bytes of the column and the lists (mutual_info_cc.h) + 320 of static reduction scratch:
// 123 200 bytes at N = 2048, k = 32 (above the 64 KiB default: opted in at the launch), 20 800 at N = 300, k = 3 (seven
// workgroups per CU).  Barriers: 2 in pair mode + 3 of the preparation, then the estimator's own (1 + the sort's
// log2 NP (log2 NP + 1) / 2 + 2).
#include <math.h>

#include "common.h"
#include "edge_prepare.h"
#include "launch.h"
#include "mlgnn.h"
#include "mutual_info_cc.h"
#include "pair_list.h"

#pragma clang fp contract(off)

namespace mlgnn {
namespace {

bool edge_cc_shape_ok(int64_t n, int64_t n_nodes, int64_t P, int64_t k, bool with_score) {
  if (n < 2 || n > kCcMaxSamples || k < 1 || k > kCcMaxNeighbors || k > n - 1) return false;
  return pair_list_shape_ok(n, n_nodes, P, with_score);
}

__global__ __launch_bounds__(kBlock) void edge_mi_cc_kernel(const double* __restrict__ xt, const int32_t* __restrict__ pairs,
                                                           const double* __restrict__ noise_x,
                                                           const double* __restrict__ y_prepared,
                                                           const double* __restrict__ psi, double base,
                                                           double* __restrict__ mi, double* __restrict__ score,
                                                           int32_t* __restrict__ nx_out, int32_t* __restrict__ ny_out, int N,
                                                           int NP, int n_nodes, int k) {
  extern __shared__ double lds[];
  __shared__ double scratch[kEdgePrepareScratchDoubles];
  __shared__ double red[2 * kWavesPerBlock];
  const CcColumn col = cc_column(lds, NP);
  const int tid = threadIdx.x;
  const size_t pair = blockIdx.x;
  // steps 1-5: xs[i] = z_i, the scaled score, and the noise's amplitude (edge_prepare.h); dy passes through yx
  const double amp = edge_prepare_column(xt, pairs, pair, N, n_nodes, col.xs, col.yx, scratch);
  const double inf = __builtin_huge_val();
  for (int i = tid; i < NP; i += kBlock) {                              // a lane's own positions, as in the preparation
    double v = inf, t = inf;
    uint32_t at = kCcPad;
    if (i < N) {
      v = col.xs[i] + amp * noise_x[i];
      t = y_prepared[i];
      at = (uint32_t)i;
      if (score) score[pair * N + i] = v;
    }
    col.xs[i] = v;
    col.ys[i] = t;
    col.idx[i] = at;
  }
  // step 6
  const double v = mi_cc_estimate(col, red, y_prepared, psi, base, nx_out ? nx_out + pair * N : nullptr,
                                  ny_out ? ny_out + pair * N : nullptr, N, NP, k);
  if (tid == 0) mi[pair] = v;
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_edge_mi_cc_supported(int64_t n, int64_t n_nodes, int64_t n_pairs, int k, int with_score) {
  return edge_cc_shape_ok(n, n_nodes, n_pairs, k, with_score != 0) ? 1 : 0;
}

extern "C" int mlgnn_edge_mi_cc(const double* xt, const int32_t* pairs, const double* noise_x, const double* y_prepared,
                                const double* psi, double base, double* mi, double* score, int32_t* nx, int32_t* ny,
                                int64_t n, int64_t n_nodes, int64_t n_pairs, int k, void* stream) {
  if (!xt || !pairs || !noise_x || !y_prepared || !psi || !mi) return MLGNN_E_NULL;
  if (!edge_cc_shape_ok(n, n_nodes, n_pairs, k, score != nullptr)) return MLGNN_E_SHAPE;
  if (n_pairs == 0) return 0;
  const int NP = cc_pow2_at_least(n);
  const size_t bytes = cc_lds_bytes(NP, k);                            // at most 122 880
  if (bytes > 64 * 1024)
    if (const hipError_t e = allow_dynamic_lds(&edge_mi_cc_kernel, (int)bytes); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(edge_mi_cc_kernel, dim3((unsigned)n_pairs), dim3(kBlock), bytes, as_stream(stream), xt, pairs,
                     noise_x, y_prepared, psi, base, mi, score, nx, ny, (int)n, NP, (int)n_nodes, k);
  return (int)hipGetLastError();
}
