// The estimator body of the regression mutual-information kernels (Kraskov, Stoegbauer, Grassberger 2004, as scikit-learn's
// _compute_mi_cc evaluates it) on ONE column that already lies in LDS: shared by csrc/mutual_info_cc.hip (the column comes
// prepared from the host) and csrc/edge_select_cc.hip (the column is prepared in the kernel).
//
//   d_ij = max(fl|x_j - x_i|, fl|y_j - y_i|)                                       Chebyshev, one IEEE subtraction each
//   r_i  = the k-th smallest d_ij over j != i
//   nx_i = #{ j != i : fl|x_j - x_i| <= nextafter(r_i, 0) },  ny_i likewise in y
//   mi   = max(0, (base - (1 / N) sum_i psi(nx_i + 1)) - (1 / N) sum_i psi(ny_i + 1))      base, psi: from the host
//
// One pass over the stages of the bitonic network of mutual_info_cd.h sorts two arrays: `xs` / `idx` by (value, sample
// index) -- the index makes that order total and carries the sample along, so `yx` = y in x-order follows -- and `ys` by
// value (it does not depend on the column; sorting it per workgroup rides on the same barriers and keeps the ABI at
// one y).  Then one lane per position p of the x-order, in passes of kBlock positions:
//   * r: walk outward from p in `xs`, taking the nearer of the left and the right candidate at every step (fl(a - b) is
//     monotone in both operands, so dx is non-decreasing along the walk: the merge of mutual_info_cd.h).  Each candidate
//     q contributes max(dx, fl|yx[q] - yx[p]|) to the lane's list of the k smallest values seen, kept in LDS as
//     list[slot][lane] (lanes on distinct banks; k is a run-time value, so registers cannot hold it).  The list is not
//     ordered: its largest value and that value's slot live in registers, a smaller candidate overwrites that slot and
//     one scan of the k slots (independent reads) finds the next largest -- a sorted list would pay a chain of
//     dependent read-write pairs per insertion instead, because with a two-valued target the other class's far
//     candidates are held until the own class's near ones push them out.  The walk stops when k values are held and
//     the next dx is not below the largest -- nothing further out can be nearer -- or when the column is exhausted.
//     With a two-valued target that is about k / (class share) candidates; with a continuous one it can be the whole
//     column.
//   * nx, ny: two binary searches each, in `xs` and in `ys`, on the predicates fl(c - key[a]) <= rr and
//     fl(key[b] - c) <= rr (monotone along the sorted order) -- not on c -+ rr, which rounds differently; minus the
//     sample itself.
//   * psi from the table; lanes add their positions p = t, t + 256, ... in that order, then the 64 lanes of a wave (xor
//     butterfly), then the four waves in wave order -- the x sum and the y sum apart, as scikit-learn subtracts them.
// No atomics: bitwise reproducible.  Every index is bounded by construction whatever the values are (NaN included: the
// walk moves one of two cursors inside [0, N) at every step, the searches run over [0, N), the table index is clamped,
// a position whose sample index is a padding's is skipped).
//
// LDS: NP = N rounded up to a power of two, 28 NP bytes (xs 8, yx 8, ys 8, idx 4) + 8 k kBlock of lists + 64 of
// reduction scratch (`red`, the caller's): 122 944 bytes at N = 2048, k = 32 (above the 64 KiB default: the caller opts
// in at the launch), 45 120 at N = 300, k = 15 (three workgroups per CU).
#pragma once
#include "common.h"
#include "mlgnn.h"

namespace mlgnn {

constexpr int64_t kCcMaxSamples = 2048;
constexpr int kCcMaxNeighbors = MLGNN_MI_CC_MAX_NEIGHBORS;
constexpr uint32_t kCcPad = 0xffffffffu;       // sample index of the padding: behind every real one

inline int cc_pow2_at_least(int64_t n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

inline size_t cc_lds_bytes(int NP, int k) { return (size_t)NP * 28 + (size_t)k * kBlock * sizeof(double); }

// the carve of the dynamic LDS of one column: cc_lds_bytes(NP, k)
struct CcColumn {
  double* xs;                                                          // [NP] the column by (value, index)
  double* yx;                                                          // [NP] y in that order
  double* ys;                                                          // [NP] y by value
  uint32_t* idx;                                                       // [NP] sample index, in xs's order
  double* list;                                                        // [k][kBlock], at this lane's column (NP is even)
};

__device__ __forceinline__ CcColumn cc_column(double* lds, int NP) {
  CcColumn c;
  c.xs = lds;
  c.yx = lds + NP;
  c.ys = lds + 2 * NP;
  c.idx = reinterpret_cast<uint32_t*>(lds + 3 * NP);
  c.list = reinterpret_cast<double*>(c.idx + NP) + threadIdx.x;
  return c;
}

// (value, sample index) order
__device__ __forceinline__ bool indexed_less(double va, uint32_t ia, double vb, uint32_t ib) {
  if (va != vb) return va < vb;
  return ia < ib;
}

// #{ j : fl|key[j] - c| <= rr } over the ascending key[0, N), c itself included where it is one of them
__device__ __forceinline__ int count_within(const double* key, int N, double c, double rr) {
  int a = 0, n = N;                                                    // first a with key[a] >= c or c - key[a] <= rr
  while (n > 0) {
    const int h = n >> 1;
    const double v = key[a + h];
    if (v >= c || c - v <= rr) { n = h; } else { a += h + 1; n -= h + 1; }
  }
  int b = 0;                                                           // first b with key[b] > c and key[b] - c > rr
  n = N;
  while (n > 0) {
    const int h = n >> 1;
    const double v = key[b + h];
    if (v <= c || v - c <= rr) { b += h + 1; n -= h + 1; } else { n = h; }
  }
  return b - a;
}

// The estimate of the column the caller has written: xs[i] = x_i, ys[i] = y[i] and idx[i] = i for i < N, +inf, +inf and
// kCcPad for N <= i < NP (no barrier needed after the fill: the first one is here; `yx` and the lists may hold anything).
// `y` [N]: the target in sample order, in global memory.  `red`: 2 kWavesPerBlock doubles of LDS.  nx_row, ny_row [N]:
// the counts in sample order, or NULL.  The value is valid in thread 0; all kBlock threads call.
__device__ __forceinline__ double mi_cc_estimate(const CcColumn& col, double* red, const double* __restrict__ y,
                                                 const double* __restrict__ psi, double base,
                                                 int32_t* __restrict__ nx_row, int32_t* __restrict__ ny_row, int N, int NP,
                                                 int k) {
  double* xs = col.xs;
  double* yx = col.yx;
  double* ys = col.ys;
  uint32_t* idx = col.idx;
  double* list = col.list;
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
        const double a = ys[i], b = ys[p];
        if (up ? b < a : a < b) { ys[i] = b; ys[p] = a; }
        const double xa = xs[i], xb = xs[p];
        const uint32_t ia = idx[i], ib = idx[p];
        if (up ? indexed_less(xb, ib, xa, ia) : indexed_less(xa, ia, xb, ib)) {
          xs[i] = xb; xs[p] = xa;
          idx[i] = ib; idx[p] = ia;
        }
      }
      __syncthreads();
    }
  }

  for (int p = tid; p < NP; p += kBlock) {
    const uint32_t s = idx[p];
    yx[p] = s < (uint32_t)N ? y[s] : inf;
  }
  __syncthreads();

  double acc_x = 0.0, acc_y = 0.0;
  for (int p = tid; p < N; p += kBlock) {
    const double c = xs[p], yc = yx[p];
    int lo = p - 1, hi = p + 1, held = 0, worst = 0;
    double dl = lo >= 0 ? c - xs[lo] : inf, dh = hi < N ? xs[hi] - c : inf;
    double top = -inf;                                                 // the largest value held; list[worst] is it
    while (lo >= 0 || hi < N) {                                        // every step moves one cursor: at most N - 1 steps
      const bool left = lo >= 0 && (hi >= N || dl <= dh);
      const double dx = left ? dl : dh;
      const bool full = held == k;
      if (full && !(dx < top)) break;
      const int q = left ? lo : hi;
      if (left) { --lo; dl = lo >= 0 ? c - xs[lo] : inf; } else { ++hi; dh = hi < N ? xs[hi] - c : inf; }
      const double dy = fabs(yx[q] - yc);
      const double d = dx > dy ? dx : dy;                              // dx >= 0 along the walk
      if (!full) {
        list[held * kBlock] = d;
        if (d > top) { top = d; worst = held; }
        ++held;
      } else if (d < top) {                                            // d takes the place of the largest; find the next
        list[worst * kBlock] = d;
        top = -inf;
        worst = 0;
#pragma unroll 4
        for (int s = 0; s < k; ++s) {
          const double v = list[s * kBlock];
          if (v > top) { top = v; worst = s; }
        }
      }
    }
    const double r = held > 0 ? top : 0.0;                             // held == k: k <= N - 1 candidates exist
    // nextafter(r, 0) of a finite r >= 0
    const double rr = r > 0.0 ? __longlong_as_double(__double_as_longlong(r) - 1) : r;
    int nx = count_within(xs, N, c, rr) - 1;                           // minus the sample itself
    int ny = count_within(ys, N, yc, rr) - 1;
    nx = nx < 0 ? 0 : (nx > N - 1 ? N - 1 : nx);                       // (NaN input only)
    ny = ny < 0 ? 0 : (ny > N - 1 ? N - 1 : ny);
    acc_x += psi[nx + 1];
    acc_y += psi[ny + 1];
    const uint32_t s = idx[p];
    if (s < (uint32_t)N) {                                             // (a padding's index here: NaN input only)
      if (nx_row) nx_row[s] = nx;
      if (ny_row) ny_row[s] = ny;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    acc_x += __shfl_xor(acc_x, o);
    acc_y += __shfl_xor(acc_y, o);
  }
  if ((tid & (kWave - 1)) == 0) {
    red[tid / kWave] = acc_x;
    red[kWavesPerBlock + tid / kWave] = acc_y;
  }
  __syncthreads();
  double v = 0.0;
  if (tid == 0) {
    const double sx = ((red[0] + red[1]) + red[2]) + red[3];
    const double* ry = red + kWavesPerBlock;
    const double sy = ((ry[0] + ry[1]) + ry[2]) + ry[3];
    v = (base - sx / (double)N) - sy / (double)N;
    v = v > 0.0 ? v : (v == v ? 0.0 : v);                              // max(0, v); a NaN stays
  }
  return v;
}

}  // namespace mlgnn
