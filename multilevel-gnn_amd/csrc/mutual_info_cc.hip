// Mutual information between continuous features and a continuous target (Kraskov, Stoegbauer, Grassberger 2004, as
// scikit-learn's _compute_mi_cc evaluates it) for all features at once: one workgroup per feature, the feature's column
// and the target in LDS, fp64 throughout.  The kernel stages the prepared column, the target and the sample indices;
// everything after that -- the sort, the walk, the counts, the fixed-order sums -- is the body of mutual_info_cc.h, which
// also states the LDS (28 NP + 8 k kBlock bytes + 64 of static reduction scratch: 122 944 bytes at N = 2048, k = 32,
// above the 64 KiB default and opted in at the launch; 45 120 at the N = 300, k = 15 of the shipped configurations).
#include <math.h>

#include "common.h"
#include "launch.h"
#include "mlgnn.h"
#include "mutual_info_cc.h"

namespace mlgnn {
namespace {

bool cc_shape_ok(int64_t n, int64_t F, int64_t k) {
  if (n < 2 || n > kCcMaxSamples || F < 0 || k < 1 || k > kCcMaxNeighbors || k > n - 1) return false;
  return F <= (((int64_t)1 << 29) - 1) / n;                             // F * N doubles below 4 GiB
}

__global__ __launch_bounds__(kBlock) void mutual_info_cc_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                               const double* __restrict__ psi, double base,
                                                               double* __restrict__ mi, int32_t* __restrict__ nx_out,
                                                               int32_t* __restrict__ ny_out, int N, int NP, int k) {
  extern __shared__ double lds[];
  __shared__ double red[2 * kWavesPerBlock];
  const CcColumn c = cc_column(lds, NP);
  const int tid = threadIdx.x;
  const double* col = x + (size_t)blockIdx.x * N;
  const double inf = __builtin_huge_val();

  for (int i = tid; i < NP; i += kBlock) {
    c.xs[i] = i < N ? col[i] : inf;
    c.ys[i] = i < N ? y[i] : inf;
    c.idx[i] = i < N ? (uint32_t)i : kCcPad;
  }
  const double v = mi_cc_estimate(c, red, y, psi, base, nx_out ? nx_out + (size_t)blockIdx.x * N : nullptr,
                                  ny_out ? ny_out + (size_t)blockIdx.x * N : nullptr, N, NP, k);
  if (tid == 0) mi[blockIdx.x] = v;
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_mutual_info_cc_supported(int64_t n, int64_t n_features, int k) {
  return cc_shape_ok(n, n_features, k) ? 1 : 0;
}

extern "C" int mlgnn_mutual_info_cc(const double* x, const double* y, const double* psi, double base, double* mi,
                                    int32_t* nx, int32_t* ny, int64_t n, int64_t n_features, int k, void* stream) {
  if (!x || !y || !psi || !mi) return MLGNN_E_NULL;
  if (!cc_shape_ok(n, n_features, k)) return MLGNN_E_SHAPE;
  if (n_features == 0) return 0;
  const int NP = cc_pow2_at_least(n);
  const size_t bytes = cc_lds_bytes(NP, k);                            // at most 122 880
  if (bytes > 64 * 1024)
    if (const hipError_t e = allow_dynamic_lds(&mutual_info_cc_kernel, (int)bytes); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(mutual_info_cc_kernel, dim3((unsigned)n_features), dim3(kBlock), bytes, as_stream(stream), x, y, psi,
                     base, mi, nx, ny, (int)n, NP, k);
  return (int)hipGetLastError();
}
