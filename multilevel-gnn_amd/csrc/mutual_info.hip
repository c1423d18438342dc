// Mutual information between continuous features and a discrete target (Ross 2014, as scikit-learn's _compute_mi_cd
// evaluates it) for all features at once: one workgroup per feature, the feature's column in LDS, fp64 throughout.  The
// estimator itself -- the double bitonic sort, the label runs, the outward walk, the two binary searches, the psi sum and
// its fixed-order reduction -- is mi_cd_estimate of csrc/mutual_info_cd.h (shared with csrc/edge_select.hip); this file
// loads the prepared column into LDS and owns the entry points.
//
// LDS: NP = N rounded up to a power of two, 24 NP bytes + 32 of static reduction scratch (mutual_info_cd.h).
#include <math.h>

#include "common.h"
#include "launch.h"
#include "mlgnn.h"
#include "mutual_info_cd.h"

namespace mlgnn {
namespace {

bool shape_ok(int64_t n, int64_t F, int64_t k, int64_t n_labels) {
  if (n < 2 || n > kMiMaxSamples || F < 0 || k < 1 || n_labels < 1 || n_labels > n) return false;
  return F <= (((int64_t)1 << 29) - 1) / n;                             // F * N doubles below 4 GiB
}

__global__ __launch_bounds__(kBlock) void mutual_info_kernel(const double* __restrict__ x, const int32_t* __restrict__ labels,
                                                            const double* __restrict__ psi, double base,
                                                            double* __restrict__ mi, int32_t* __restrict__ counts, int N,
                                                            int NP, int k, int n_labels) {
  extern __shared__ double lds[];
  __shared__ double red[kWavesPerBlock];
  const MiColumn c = mi_column(lds, NP);
  const int tid = threadIdx.x;
  const double* col = x + (size_t)blockIdx.x * N;
  const double inf = __builtin_huge_val();

  for (int i = tid; i < NP; i += kBlock) {
    double v = inf;
    uint32_t t = kMiPadTag;
    if (i < N) {
      v = col[i];
      t = mi_tag(labels[i], n_labels, i);
    }
    c.key[i] = v;
    c.lkey[i] = v;
    c.tag[i] = t;
  }
  const double v = mi_cd_estimate(c, red, psi, base, counts ? counts + (size_t)blockIdx.x * N : nullptr, N, NP, k);
  if (tid == 0) mi[blockIdx.x] = v;
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_mutual_info_supported(int64_t n, int64_t n_features, int k, int n_labels) {
  return shape_ok(n, n_features, k, n_labels) ? 1 : 0;
}

extern "C" int mlgnn_mutual_info_cd(const double* x, const int32_t* labels, const double* psi, double base, double* mi,
                                    int32_t* counts, int64_t n, int64_t n_features, int k, int n_labels, void* stream) {
  if (!x || !labels || !psi || !mi) return MLGNN_E_NULL;
  if (!shape_ok(n, n_features, k, n_labels)) return MLGNN_E_SHAPE;
  if (n_features == 0) return 0;
  const int NP = mi_pow2_at_least(n);
  const size_t bytes = (size_t)NP * 24;                                // at most 48 KiB: below the default limit
  hipLaunchKernelGGL(mutual_info_kernel, dim3((unsigned)n_features), dim3(kBlock), bytes, as_stream(stream), x, labels,
                     psi, base, mi, counts, (int)n, NP, k, n_labels);
  return (int)hipGetLastError();
}
