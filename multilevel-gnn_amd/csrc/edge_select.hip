// The --edge_select test of the fold preparation (the reference's valid_pca_mutual_info, multiloader.py:828-874) for all
// PPI edges of a fold at once: one workgroup per PAIR of nodes, fp64 throughout.  Per pair (s, t), on the N training
// patients, what the reference computes with PCA(n_components=1) and mutual_info_classif(score, y, random_state):
//
//   1.-5. the preparation of edge_prepare.h: the score of the pair's closed-form 2 x 2 PCA with scikit-learn's sign rule,
//      scale(with_mean=False) -> z, and the noise's amplitude 1e-10 max(1, mean|z|);
//   the noise: value_i = z_i + amplitude noise_i -- ONE noise vector per fold: with a fixed random_state every call of
//      the reference seeds a fresh generator and draws the same N values;
//   6. the estimator of csrc/mutual_info_cd.h on that column.
// t < 0 selects the single-column mode: score_i = x_s[i], uncentred, then steps 4-6: the end-node value
// mutual_info_classif(column[:, None], y, random_state).
//
// Every sum in the fixed order of the other kernels: a lane adds its positions i = t, t + 256, ... in that order, then
// the 64 lanes of a wave (xor butterfly), then the four waves in wave order; every reduction has LDS scratch of its own,
// so each costs one barrier.  No atomics, no fused multiply-add (contraction is off in this file and in edge_prepare.h: a product and the sum
// that takes it round separately, as in the numpy restatement of the tests): bitwise reproducible, and a pair's bits do
// not depend on the other pairs.  Node indices are clamped to [0, n_nodes), so a wrong value cannot read outside xt; no
// other index depends on a value (mutual_info_cd.h).
//
// LDS: 24 NP bytes of the column (mutual_info_cd.h; dx lies in `key` and dy in `lkey` until the score replaces them) +
// 288 of static reduction scratch: 49 440 bytes at N = 2048, 12 576 at N = 300.  Barriers: 2 in pair mode (means,
// centred sums) + 3 (mean, deviation, mean magnitude of the score) before the estimator's own.
#include <math.h>

#include "common.h"
#include "edge_prepare.h"
#include "launch.h"
#include "mlgnn.h"
#include "mutual_info_cd.h"
#include "pair_list.h"

#pragma clang fp contract(off)

namespace mlgnn {
namespace {

bool shape_ok(int64_t n, int64_t n_nodes, int64_t P, int64_t k, int64_t n_labels, bool with_score) {
  if (n < 2 || n > kMiMaxSamples || k < 1 || n_labels < 1 || n_labels > n) return false;
  return pair_list_shape_ok(n, n_nodes, P, with_score);
}

__global__ __launch_bounds__(kBlock) void edge_mi_kernel(const double* __restrict__ xt, const int32_t* __restrict__ pairs,
                                                        const double* __restrict__ noise,
                                                        const int32_t* __restrict__ labels, const double* __restrict__ psi,
                                                        double base, double* __restrict__ mi, double* __restrict__ score,
                                                        int32_t* __restrict__ counts, int N, int NP, int n_nodes, int k,
                                                        int n_labels) {
  extern __shared__ double lds[];
  __shared__ double scratch[kEdgePrepareScratchDoubles];
  __shared__ double red[kWavesPerBlock];
  const MiColumn col = mi_column(lds, NP);
  double* key = col.key;
  double* lkey = col.lkey;
  const int tid = threadIdx.x;
  const size_t pair = blockIdx.x;
  // steps 1-5: key[i] = z_i, the scaled score, and the noise's amplitude (edge_prepare.h)
  const double amp = edge_prepare_column(xt, pairs, pair, N, n_nodes, key, lkey, scratch);
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
