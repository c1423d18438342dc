// Mutual information between continuous features and a discrete target (Ross 2014, as scikit-learn's _compute_mi_cd
// evaluates it) for all features at once: one workgroup per feature, the feature's column in LDS, fp64 throughout.
//
//   k_i = min(k, count(d_i) - 1)
//   r_i = the k_i-th smallest of fl|c_j - c_i| over j != i with d_j = d_i         one IEEE subtraction
//   m_i = #{ j : fl|c_j - c_i| <= nextafter(r_i, 0) } over all N samples, self included
//   mi  = max(0, base - (1 / N) sum_i psi(m_i))                                    base, psi: from the host
//
// The column is sorted twice by the same bitonic network (both arrays move in one pass over its stages): `key` by value
// over all samples, and `lkey` / `tag` by (label, value, sample index) -- the index makes that order total, so the order
// of the final sum does not depend on how the network treats ties.  Then one lane per position p of the label order:
//   * r: at most k_i steps outward from p inside the label's run [rs, re) of `lkey`, taking the nearer of the two
//     candidates at every step (differences to the left and to the right are non-decreasing outward, because fl(a - b)
//     is monotone in both operands: a merge of two sorted sequences);
//   * m: two binary searches in `key` on the predicate fl(c - key[a]) <= rr (left of c) and fl(key[b] - c) <= rr (right
//     of c), which is monotone along the sorted order for the same reason -- not on c -+ rr, which rounds differently;
//   * psi(m) from the table; lanes add their positions p = t, t + 256, ... in that order, then the 64 lanes of a wave
//     (xor butterfly), then the four waves in wave order.
// No atomics: bitwise reproducible.  Every index is bounded by construction whatever the values are (NaN included: the
// searches run over [0, N) and every walk step checks its run's ends); labels outside [0, n_labels) are read as 0.
//
// LDS: NP = N rounded up to a power of two, 24 NP bytes (key 8, lkey 8, tag 4, run begin 2, run end 2) + 32 of static
// reduction scratch: 49 184 bytes at N = 2048, 12 320 at the N = 300 of the shipped configurations.
#include <math.h>

#include "common.h"
#include "launch.h"
#include "mlgnn.h"

namespace mlgnn {
namespace {

constexpr int64_t kMiMaxSamples = 2048;
constexpr uint32_t kPadTag = 0xffffffffu;      // label 0xffff: behind every real label (labels < 2048)

bool shape_ok(int64_t n, int64_t F, int64_t k, int64_t n_labels) {
  if (n < 2 || n > kMiMaxSamples || F < 0 || k < 1 || n_labels < 1 || n_labels > n) return false;
  return F <= (((int64_t)1 << 29) - 1) / n;                             // F * N doubles below 4 GiB
}

int pow2_at_least(int64_t n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

// (label, value, sample index) order; tag = label << 16 | index, so equal labels compare their indices through the tags
__device__ __forceinline__ bool tagged_less(double va, uint32_t ta, double vb, uint32_t tb) {
  const uint32_t la = ta >> 16, lb = tb >> 16;
  if (la != lb) return la < lb;
  if (va != vb) return va < vb;
  return ta < tb;
}

__global__ __launch_bounds__(kBlock) void mutual_info_kernel(const double* __restrict__ x, const int32_t* __restrict__ labels,
                                                            const double* __restrict__ psi, double base,
                                                            double* __restrict__ mi, int32_t* __restrict__ counts, int N,
                                                            int NP, int k, int n_labels) {
  extern __shared__ double lds[];
  __shared__ double red[kWavesPerBlock];
  double* key = lds;                                                   // [NP] all samples by value
  double* lkey = lds + NP;                                             // [NP] by (label, value, index)
  uint32_t* tag = reinterpret_cast<uint32_t*>(lds + 2 * NP);           // [NP] label << 16 | sample index, in lkey's order
  uint16_t* rs = reinterpret_cast<uint16_t*>(tag + NP);                // [NP] first position of a label's run
  uint16_t* re = rs + NP;                                              // [NP] one past its last
  const int tid = threadIdx.x;
  const double* col = x + (size_t)blockIdx.x * N;
  const double inf = __builtin_huge_val();

  for (int i = tid; i < NP; i += kBlock) {
    double v = inf;
    uint32_t t = kPadTag;
    if (i < N) {
      v = col[i];
      const int32_t l = labels[i];
      t = ((uint32_t)l < (uint32_t)n_labels ? (uint32_t)l << 16 : 0u) | (uint32_t)i;
    }
    key[i] = v;
    lkey[i] = v;
    tag[i] = t;
  }
  __syncthreads();

  // bitonic network, ascending; thread t owns the pairs (i, i | j) with i = t's bits with a 0 inserted at bit j
  for (int kk = 2; kk <= NP; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (NP >> 1); t += kBlock) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int p = i | j;
        const bool up = (i & kk) == 0;
        const double a = key[i], b = key[p];
        if (up ? b < a : a < b) { key[i] = b; key[p] = a; }
        const double la = lkey[i], lb = lkey[p];
        const uint32_t ta = tag[i], tb = tag[p];
        if (up ? tagged_less(lb, tb, la, ta) : tagged_less(la, ta, lb, tb)) {
          lkey[i] = lb; lkey[p] = la;
          tag[i] = tb; tag[p] = ta;
        }
      }
      __syncthreads();
    }
  }

  // the runs of the labels (labels < n_labels <= N <= NP)
  for (int p = tid; p < N; p += kBlock) {
    const uint32_t l = tag[p] >> 16;
    if (p == 0 || (tag[p - 1] >> 16) != l) rs[l] = (uint16_t)p;
    if (p == N - 1 || (tag[p + 1] >> 16) != l) re[l] = (uint16_t)(p + 1);
  }
  __syncthreads();

  double acc = 0.0;
  for (int p = tid; p < N; p += kBlock) {
    const double c = lkey[p];
    const uint32_t t = tag[p];
    const int s = rs[t >> 16], e = re[t >> 16];
    const int ki = min(k, e - s - 1);
    int lo = p - 1, hi = p + 1;
    double r = 0.0;
    for (int step = 0; step < ki; ++step) {
      const double dl = lo >= s ? c - lkey[lo] : inf;
      const double dh = hi < e ? lkey[hi] - c : inf;
      if (dl <= dh) { r = dl; --lo; } else { r = dh; ++hi; }
    }
    // nextafter(r, 0) of a finite r >= 0
    const double rr = r > 0.0 ? __longlong_as_double(__double_as_longlong(r) - 1) : r;
    int a = 0, n = N;                                                  // first a with key[a] >= c or c - key[a] <= rr
    while (n > 0) {
      const int h = n >> 1;
      const double v = key[a + h];
      if (v >= c || c - v <= rr) { n = h; } else { a += h + 1; n -= h + 1; }
    }
    int b = 0;                                                         // first b with key[b] > c and key[b] - c > rr
    n = N;
    while (n > 0) {
      const int h = n >> 1;
      const double v = key[b + h];
      if (v <= c || v - c <= rr) { b += h + 1; n -= h + 1; } else { n = h; }
    }
    int m = b - a;
    m = m < 0 ? 0 : m;                                                 // (NaN input only)
    acc += psi[m];
    if (counts) counts[(size_t)blockIdx.x * N + (t & 0xffffu)] = m;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
  if ((tid & (kWave - 1)) == 0) red[tid / kWave] = acc;
  __syncthreads();
  if (tid == 0) {
    const double sum = ((red[0] + red[1]) + red[2]) + red[3];
    const double v = base - sum / (double)N;
    mi[blockIdx.x] = v > 0.0 ? v : (v == v ? 0.0 : v);                 // max(0, v); a NaN stays
  }
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
  const int NP = pow2_at_least(n);
  const size_t bytes = (size_t)NP * 24;                                // at most 48 KiB: below the default limit
  hipLaunchKernelGGL(mutual_info_kernel, dim3((unsigned)n_features), dim3(kBlock), bytes, as_stream(stream), x, labels,
                     psi, base, mi, counts, (int)n, NP, k, n_labels);
  return (int)hipGetLastError();
}
