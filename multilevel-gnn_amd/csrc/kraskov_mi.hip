// The --knn_mutual_info form of the fold preparation's edge test (the reference's utils/knnie.py::kraskov_mi as
// valid_pca_mutual_info calls it, multiloader.py:838-839, 853-854, 863-864) for all node pairs of a fold at once: one
// workgroup per PAIR of nodes, fp64 throughout.  Per pair (s, t) on the N training patients, with the raw columns
// x_s, x_t (no PCA, no scaling, no noise) and the label column y, what the reference computes on three KD-trees:
//
//   d_ij = max(fl|x_s[i] - x_s[j]|, fl|x_t[i] - x_t[j]|, fl|y[i] - y[j]|)           Chebyshev, one IEEE subtraction each
//   kd_i = the (k + 1)-th smallest d_ij over ALL j, self included, duplicates counted  tree_xy.query(p, k + 1, p=inf)[0][k]
//   r_i  = fl(kd_i - 1e-15)                                                            exactly as the reference writes it
//   nx_i = #{ j : max(fl|x_s[i] - x_s[j]|, fl|x_t[i] - x_t[j]|) <= r_i }               query_ball_point, self included
//   ny_i = #{ j : fl|y[i] - y[j]| <= r_i }
//   mi   = (base - (1 / N) sum_i psi(nx_i)) - (1 / N) sum_i psi(ny_i)                  base = psi(k) + psi(N), psi: the host's
//
// The reference's three sums of log(kd_i) cancel identically and are left out.  Where some kd_i is 0 or not finite the
// reference takes log(0) and stops; here that pair's mi is NaN.  t < 0 selects the single-column form (d_x = 1): the
// x_t terms are left out (a branch that is uniform over the workgroup picks the instantiation without them).
//
// The three columns lie in LDS (24 N bytes; two of them in the single-column form).  A lane owns the samples i = tid, tid + 256, ... and walks all j for each of
// them, twice: every lane reads the same j, and an identical LDS address is a broadcast.  Pass 1 keeps the k + 1 smallest
// d_ij as an ascending list in registers: the list length L = k + 1 is a template parameter, so every index into it is a
// compile-time constant after unrolling and nothing goes to scratch memory; an insertion is one chain of L
// compare-exchanges and happens only where d_ij is below the list's largest.  Pass 2 counts.  2 N^2 distance evaluations
// per pair.
//
// Sums in the fixed order of block_sums.h: a lane adds its samples in the order i = tid, tid + 256, ..., then the 64 lanes
// of a wave, then the four waves.  No atomics: bitwise reproducible, and a pair's bits do not depend on the other pairs.
// Node indices are clamped to [0, n_nodes) and table indices to [1, N]; no other address depends on a value.
//
// LDS: 24 N bytes + 96 of static reduction scratch: 49 248 bytes at N = 2048, 7 296 at N = 300.  Barriers: 2 (columns
// staged; the sums).
#include <math.h>

#include <array>
#include <utility>

#include "block_sums.h"
#include "common.h"
#include "launch.h"
#include "mlgnn.h"
#include "pair_list.h"

#pragma clang fp contract(off)

namespace mlgnn {
namespace {

constexpr int64_t kKsgMaxSamples = 2048;
constexpr int kKsgMaxNeighbors = MLGNN_KRASKOV_MAX_NEIGHBORS;

bool ksg_shape_ok(int64_t n, int64_t n_nodes, int64_t P, int64_t k, bool with_details) {
  if (k < 1 || k > kKsgMaxNeighbors || n < k + 1 || n > kKsgMaxSamples) return false;
  return pair_list_shape_ok(n, n_nodes, P, with_details);
}

__device__ __forceinline__ double larger(double a, double b) { return a > b ? a : b; }

// The samples i = tid, tid + 256, ... of one pair: both passes, the details, and the lane's three partial sums.  PAIR:
// whether the second column takes part (false: the single-column form, which neither stages nor reads it).
template <int L, bool PAIR>
__device__ __forceinline__ void ksg_samples(const double* xs, const double* xq, const double* ys,
                                            const double* __restrict__ psi, double* __restrict__ kd_out,
                                            int32_t* __restrict__ nx_out, int32_t* __restrict__ ny_out, size_t row, int N,
                                            double (&acc)[3]) {
  const double inf = __builtin_huge_val();
  for (int i = threadIdx.x; i < N; i += kBlock) {
    const double cs = xs[i], cq = PAIR ? xq[i] : 0.0, cy = ys[i];
    // pass 1: the L smallest d_ij, ascending
    double list[L];
#pragma unroll
    for (int q = 0; q < L; ++q) list[q] = inf;
    for (int j = 0; j < N; ++j) {
      double dx = fabs(cs - xs[j]);
      if (PAIR) dx = larger(dx, fabs(cq - xq[j]));
      const double d = larger(dx, fabs(cy - ys[j]));
      if (d < list[L - 1]) {
        double c = d;                                                   // carried up the list; the last carry drops out
#pragma unroll
        for (int q = 0; q < L; ++q) {
          const double held = list[q];
          const bool below = c < held;
          list[q] = below ? c : held;
          c = below ? held : c;
        }
      }
    }
    const double kd = list[L - 1];
    // pass 2: the two counts inside r
    const double r = kd - 1e-15;
    int nx = 0, ny = 0;
    for (int j = 0; j < N; ++j) {
      double dx = fabs(cs - xs[j]);
      if (PAIR) dx = larger(dx, fabs(cq - xq[j]));
      nx += dx <= r ? 1 : 0;
      ny += fabs(cy - ys[j]) <= r ? 1 : 0;
    }
    acc[0] += psi[min(max(nx, 1), N)];
    acc[1] += psi[min(max(ny, 1), N)];
    acc[2] += (kd > 0.0 && kd < inf) ? 0.0 : 1.0;
    if (kd_out) kd_out[row + i] = kd;
    if (nx_out) nx_out[row + i] = nx;
    if (ny_out) ny_out[row + i] = ny;
  }
}

template <int L>
__global__ __launch_bounds__(kBlock) void kraskov_mi_kernel(const double* __restrict__ xt, const int32_t* __restrict__ pairs,
                                                           const double* __restrict__ y, const double* __restrict__ psi,
                                                           double base, double* __restrict__ mi, double* __restrict__ kd_out,
                                                           int32_t* __restrict__ nx_out, int32_t* __restrict__ ny_out, int N,
                                                           int n_nodes) {
  extern __shared__ double lds[];
  __shared__ double scratch[3 * kWavesPerBlock];
  double* xs = lds;                                                     // [N] the source node's column
  double* xq = lds + N;                                                 // [N] the target node's (unused: single)
  double* ys = lds + 2 * N;                                             // [N] the label
  const int tid = threadIdx.x;
  const size_t pair = blockIdx.x;
  const double *gs, *gq;
  const bool single = pair_rows(xt, pairs, pair, N, n_nodes, gs, gq);   // uniform over the workgroup
  for (int i = tid; i < N; i += kBlock) {
    xs[i] = gs[i];
    if (!single) xq[i] = gq[i];
    ys[i] = y[i];
  }
  __syncthreads();

  double acc[3] = {0.0, 0.0, 0.0};                                      // sum psi(nx), sum psi(ny), samples with a bad kd
  if (single)
    ksg_samples<L, false>(xs, xq, ys, psi, kd_out, nx_out, ny_out, pair * N, N, acc);
  else
    ksg_samples<L, true>(xs, xq, ys, psi, kd_out, nx_out, ny_out, pair * N, N, acc);
  block_sums(acc, scratch);
  if (tid == 0) {
    const double n_d = (double)N;
    const double v = (base - acc[0] / n_d) - acc[1] / n_d;
    mi[pair] = acc[2] == 0.0 ? v : __builtin_nan("");
  }
}

using KsgKernel = void (*)(const double*, const int32_t*, const double*, const double*, double, double*, double*, int32_t*,
                           int32_t*, int, int);

// entry k - 1: the instantiation with the list length k + 1
template <int... K>
constexpr std::array<KsgKernel, sizeof...(K)> ksg_table(std::integer_sequence<int, K...>) {
  return {{kraskov_mi_kernel<K + 2>...}};
}

constexpr auto kKsgKernels = ksg_table(std::make_integer_sequence<int, kKsgMaxNeighbors>{});

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_kraskov_mi_supported(int64_t n, int64_t n_nodes, int64_t n_pairs, int k, int with_details) {
  return ksg_shape_ok(n, n_nodes, n_pairs, k, with_details != 0) ? 1 : 0;
}

extern "C" int mlgnn_kraskov_mi(const double* xt, const int32_t* pairs, const double* y, const double* psi, double base,
                                double* mi, double* kd, int32_t* nx, int32_t* ny, int64_t n, int64_t n_nodes,
                                int64_t n_pairs, int k, void* stream) {
  if (!xt || !pairs || !y || !psi || !mi) return MLGNN_E_NULL;
  if (!ksg_shape_ok(n, n_nodes, n_pairs, k, kd || nx || ny)) return MLGNN_E_SHAPE;
  if (n_pairs == 0) return 0;
  const size_t bytes = (size_t)n * 24;                                  // at most 48 KiB: below the default limit
  hipLaunchKernelGGL(kKsgKernels[k - 1], dim3((unsigned)n_pairs), dim3(kBlock), bytes, as_stream(stream), xt, pairs, y, psi,
                     base, mi, kd, nx, ny, (int)n, (int)n_nodes);
  return (int)hipGetLastError();
}
