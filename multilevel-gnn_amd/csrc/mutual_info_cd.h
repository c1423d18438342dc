// The estimator body of the mutual-information kernels (Ross 2014, as scikit-learn's _compute_mi_cd evaluates it) on ONE
// column that already lies in LDS: shared by csrc/mutual_info.hip (the column comes prepared from the host) and
// csrc/edge_select.hip (the column is prepared in the kernel).
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
// LDS: NP = N rounded up to a power of two, 24 NP bytes (key 8, lkey 8, tag 4, run begin 2, run end 2) + 32 of
// reduction scratch (`red`, the caller's): 49 184 bytes at N = 2048, 12 320 at the N = 300 of the shipped configurations.
#pragma once
#include "common.h"

namespace mlgnn {

constexpr int64_t kMiMaxSamples = 2048;
constexpr uint32_t kMiPadTag = 0xffffffffu;    // label 0xffff: behind every real label (labels < 2048)

inline int mi_pow2_at_least(int64_t n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

// the carve of the dynamic LDS of one column: 24 NP bytes
struct MiColumn {
  double* key;                                                         // [NP] all samples by value
  double* lkey;                                                        // [NP] by (label, value, index)
  uint32_t* tag;                                                       // [NP] label << 16 | sample index, in lkey's order
  uint16_t* rs;                                                        // [NP] first position of a label's run
  uint16_t* re;                                                        // [NP] one past its last
};

__device__ __forceinline__ MiColumn mi_column(double* lds, int NP) {
  MiColumn c;
  c.key = lds;
  c.lkey = lds + NP;
  c.tag = reinterpret_cast<uint32_t*>(lds + 2 * NP);
  c.rs = reinterpret_cast<uint16_t*>(c.tag + NP);
  c.re = c.rs + NP;
  return c;
}

// the tag of sample i: a label outside [0, n_labels) is read as 0
__device__ __forceinline__ uint32_t mi_tag(int32_t label, int n_labels, int i) {
  return ((uint32_t)label < (uint32_t)n_labels ? (uint32_t)label << 16 : 0u) | (uint32_t)i;
}

// (label, value, sample index) order; tag = label << 16 | index, so equal labels compare their indices through the tags
__device__ __forceinline__ bool mi_tagged_less(double va, uint32_t ta, double vb, uint32_t tb) {
  const uint32_t la = ta >> 16, lb = tb >> 16;
  if (la != lb) return la < lb;
  if (va != vb) return va < vb;
  return ta < tb;
}

// The estimate of the column the caller has written: key[i] = lkey[i] = c_i and tag[i] = mi_tag(label_i, n_labels, i)
// for i < N, +inf and kMiPadTag for N <= i < NP (no barrier needed after the fill: the first one is here).  `red`:
// kWavesPerBlock doubles of LDS.  counts_row [N]: m_i in sample order, or NULL.  The value is valid in thread 0; all
// kBlock threads call.
__device__ __forceinline__ double mi_cd_estimate(const MiColumn& col, double* red, const double* __restrict__ psi,
                                                 double base, int32_t* __restrict__ counts_row, int N, int NP, int k) {
  double* key = col.key;
  double* lkey = col.lkey;
  uint32_t* tag = col.tag;
  uint16_t* rs = col.rs;
  uint16_t* re = col.re;
  const int tid = threadIdx.x;
  const double inf = __builtin_huge_val();
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
        if (up ? mi_tagged_less(lb, tb, la, ta) : mi_tagged_less(la, ta, lb, tb)) {
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
    if (counts_row) counts_row[t & 0xffffu] = m;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
  if ((tid & (kWave - 1)) == 0) red[tid / kWave] = acc;
  __syncthreads();
  double v = 0.0;
  if (tid == 0) {
    const double sum = ((red[0] + red[1]) + red[2]) + red[3];
    v = base - sum / (double)N;
    v = v > 0.0 ? v : (v == v ? 0.0 : v);                              // max(0, v); a NaN stays
  }
  return v;
}

}  // namespace mlgnn
