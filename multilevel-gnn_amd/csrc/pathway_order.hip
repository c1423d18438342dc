// Pathway reordering (the reference's dataloader/multiloader.py:512-528), fp64: the correlation matrix of R rows
// (np.corrcoef - I) and the greedy nearest-neighbour chain over it, in three launches with no host step between them.
//
//   x [R, A, B]: row r, outer block a, inner b at x[r * row_stride + a * outer_stride + b]; the L = A B values of a row
//   are the observations of one variable in the order l = a B + b.  (The PCA scores [N, 3 R, k] are R rows with A = N,
//   B = 3 k, row_stride = 3 k, outer_stride = 3 R k: no transposing copy.)
//
// 1. pathway_order_mean_kernel, one workgroup per row: mean_r = (sum_l x[r, l]) / L.  Thread t adds its elements
//    t, t + 256, ... in that order, the 256 partial sums are folded by halves in LDS.
// 2. pathway_order_gram_kernel, one workgroup of 16 waves per chunk of 256 columns: the chunk's share of the centred
//    Gram matrix  C = (x - mean)(x - mean)^T  on v_mfma_f64_16x16x4_f64, upper-triangular 16 x 16 tiles only.  The chunk
//    is staged 64 columns at a time: lanes along the contiguous axis read x, subtract the row's mean (numpy centres
//    first and multiplies then; so does this) and store [Rp][64] doubles in LDS with a row stride of 66 (Rp = R rounded
//    up to 16; rows past R and columns past L are zeros; 66 doubles = 4 banks mod 64, so the 16 rows x 2 k of a
//    half-wave's operand read hit 32 distinct bank pairs).  Wave w owns the tiles w, w + 16, ... and keeps their
//    accumulators in registers across the four stagings, then writes them to part[chunk][tile][16][16].
//      operand maps: lane l gives A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], one double each;
//      result: register q of lane l is C[row (l >> 4) + 4 q][col l & 15]   (NOT the f32 shapes' 4 (l >> 4) + q).
// 3. pathway_order_chain_kernel, one workgroup:
//    a. gram[tile][16][16] = (sum over chunks, in chunk order, of part) * (1 / (L - 1));
//    b. s_i = sqrt(gram_ii); info[0] = the number of rows whose gram_ii is not a positive finite number;
//    c. corr[i, j] = corr[j, i] = clip((gram_ij / s_i) / s_j, -1, 1) for i < j (one value, written twice: the mirror
//       is bit for bit), corr[i, i] = gram_ii / s_i / s_i - 1; clip keeps a NaN;
//    d. the start pair: the largest corr[i, j] over i < j, the first in row-major order among equal values;
//    e. wave 0 runs the R - 2 steps: the not-yet-used t with the largest corr[last, t], the highest t among equal values.
//    In d and e a NaN ranks as -inf, so every index stays in [0, R) and `order` is a permutation whatever x holds.
// No float atomics, every sum in a fixed order: bitwise reproducible.
#include <math.h>

#include "common.h"
#include "launch.h"
#include "mlgnn.h"

namespace mlgnn {
namespace {

constexpr int kOrdMaxRows = 256;
constexpr int kOrdTile = 16;
constexpr int kOrdMaxTilesPerWave = 9;           // 16 x 17 / 2 = 136 tiles at 256 rows over 16 waves
constexpr int kOrdBlock = 1024;
constexpr int kOrdWaves = kOrdBlock / kWave;
constexpr int kOrdSub = 64;                      // columns staged at a time
constexpr int kOrdLds = kOrdSub + 2;             // padded LDS row stride, doubles
constexpr int kOrdChunk = 4 * kOrdSub;           // columns per workgroup
constexpr int kOrdMeanBlock = 256;
constexpr int64_t kOrdMaxDoubles = ((int64_t)1 << 29) - 1;   // an array of doubles below 4 GiB

using f64x4 = __attribute__((ext_vector_type(4))) double;

struct OrderShape {
  int64_t L, chunks, tiles, rp;
};

bool order_shape(int64_t rows, int64_t outer, int64_t inner, OrderShape* s) {
  if (rows < 2 || rows > kOrdMaxRows || outer < 1 || inner < 1) return false;
  if (outer > kOrdMaxDoubles / inner) return false;
  const int64_t L = outer * inner;
  if (L < 2 || L > kOrdMaxDoubles / rows) return false;
  const int64_t nt = (rows + kOrdTile - 1) / kOrdTile;
  s->L = L;
  s->chunks = (L + kOrdChunk - 1) / kOrdChunk;
  s->tiles = nt * (nt + 1) / 2;
  s->rp = nt * kOrdTile;
  return s->chunks <= kOrdMaxDoubles / (s->tiles * 256);
}

// workspace: mean [Rp] | gram [tiles][256] | part [chunks][tiles][256], each on a 256-byte boundary
size_t order_mean_bytes(const OrderShape& s) { return align256((size_t)s.rp * sizeof(double)); }
size_t order_gram_bytes(const OrderShape& s) { return align256((size_t)s.tiles * 256 * sizeof(double)); }
size_t order_part_bytes(const OrderShape& s) { return align256((size_t)s.chunks * s.tiles * 256 * sizeof(double)); }

// the l-th observation of a row, as an offset from the row's first
__device__ __forceinline__ size_t obs_offset(unsigned l, unsigned inner, size_t outer_stride) {
  const unsigned a = l / inner;
  return (size_t)a * outer_stride + (l - a * inner);
}

__global__ __launch_bounds__(kOrdMeanBlock) void pathway_order_mean_kernel(
    const double* __restrict__ x, double* __restrict__ mean, int L, int inner, size_t row_stride, size_t outer_stride) {
  __shared__ double part[kOrdMeanBlock];
  const double* row = x + (size_t)blockIdx.x * row_stride;
  double s = 0.0;
  for (int l = threadIdx.x; l < L; l += kOrdMeanBlock) s += row[obs_offset(l, inner, outer_stride)];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int h = kOrdMeanBlock / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) mean[blockIdx.x] = part[0] / (double)L;
}

// tile t of the upper triangle in row-major order -> (ti, tj), ti <= tj < nt
__device__ __forceinline__ void tile_of(int t, int nt, int& ti, int& tj) {
  ti = 0;
  while (t >= nt - ti) { t -= nt - ti; ++ti; }
  tj = ti + t;
}

__global__ __launch_bounds__(kOrdBlock) void pathway_order_gram_kernel(
    const double* __restrict__ x, const double* __restrict__ mean, double* __restrict__ part, int R, int L, int inner,
    size_t row_stride, size_t outer_stride, int nt, int tiles) {
  extern __shared__ double lds[];                // [Rp][kOrdLds]
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int rp = nt * kOrdTile;

  int ti[kOrdMaxTilesPerWave], tj[kOrdMaxTilesPerWave];
  f64x4 acc[kOrdMaxTilesPerWave];
#pragma unroll
  for (int i = 0; i < kOrdMaxTilesPerWave; ++i) {
    const int t = wave + kOrdWaves * i;
    ti[i] = tj[i] = 0;
    if (t < tiles) tile_of(t, nt, ti[i], tj[i]);
    acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
  }

  const int col = tid & (kOrdSub - 1), rg = tid / kOrdSub;       // staging: 16 rows x 64 columns per pass
  const int arow = lane & 15, ak = lane >> 4;                     // operands
  for (int sub = 0; sub < kOrdChunk / kOrdSub; ++sub) {
    const int l = blockIdx.x * kOrdChunk + sub * kOrdSub + col;
    const bool live = l < L;
    const size_t off = live ? obs_offset(l, inner, outer_stride) : 0;
    __syncthreads();                                              // the previous staging has been read
    for (int r = rg; r < rp; r += kOrdBlock / kOrdSub)
      lds[r * kOrdLds + col] = (live && r < R) ? x[(size_t)r * row_stride + off] - mean[r] : 0.0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kOrdMaxTilesPerWave; ++i) {
      if (wave + kOrdWaves * i < tiles) {                         // wave-uniform
        const double* pa = lds + (ti[i] * kOrdTile + arow) * kOrdLds + ak;
        const double* pb = lds + (tj[i] * kOrdTile + arow) * kOrdLds + ak;
#pragma unroll
        for (int k0 = 0; k0 < kOrdSub; k0 += 4)
          acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k0], pb[k0], acc[i], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kOrdMaxTilesPerWave; ++i) {
    const int t = wave + kOrdWaves * i;
    if (t < tiles) {
      double* out = part + ((size_t)blockIdx.x * tiles + t) * 256;
#pragma unroll
      for (int q = 0; q < 4; ++q) out[((lane >> 4) + 4 * q) * kOrdTile + (lane & 15)] = acc[i][q];
    }
  }
}

__global__ __launch_bounds__(kOrdBlock) void pathway_order_chain_kernel(
    const double* __restrict__ part, double* __restrict__ gram, double* corr, int32_t* __restrict__ order,
    int32_t* __restrict__ info, int R, int L, int chunks, int nt, int tiles) {
  __shared__ double sd[kOrdMaxRows];
  __shared__ double best_v[kOrdBlock];
  __shared__ int best_i[kOrdBlock];
  __shared__ unsigned char tile_i[kOrdMaxRows / kOrdTile * (kOrdMaxRows / kOrdTile + 1) / 2];
  __shared__ unsigned char tile_j[kOrdMaxRows / kOrdTile * (kOrdMaxRows / kOrdTile + 1) / 2];
  const int tid = threadIdx.x;
  const double scale = 1.0 / (double)(L - 1);

  for (int t = tid; t < tiles; t += kOrdBlock) {
    int a, b;
    tile_of(t, nt, a, b);
    tile_i[t] = (unsigned char)a;
    tile_j[t] = (unsigned char)b;
  }
  for (int e = tid; e < tiles * 256; e += kOrdBlock) {            // a. the chunks in chunk order
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * tiles * 256 + e];
    gram[e] = s * scale;
  }
  __syncthreads();

  int degenerate = 0;                                             // b.
  if (tid < R) {
    const int a = tid / kOrdTile, w = tid % kOrdTile;
    const double v = gram[(size_t)(a * nt - a * (a - 1) / 2) * 256 + w * kOrdTile + w];
    sd[tid] = sqrt(v);
    degenerate = !(v > 0.0 && v < INFINITY);
  }
  const int n_degenerate = __syncthreads_count(degenerate);
  if (tid == 0) info[0] = n_degenerate;

  double bv = -INFINITY;                                          // c. and this thread's share of d.
  int bi = 0x7fffffff;
  for (int e = tid; e < tiles * 256; e += kOrdBlock) {
    const int t = e >> 8;
    const int i = tile_i[t] * kOrdTile + ((e >> 4) & 15), j = tile_j[t] * kOrdTile + (e & 15);
    if (i >= R || j >= R || i > j) continue;
    const double g = gram[e];
    if (i == j) {
      corr[(size_t)i * R + i] = g / sd[i] / sd[i] - 1.0;
      continue;
    }
    double r = g / sd[i] / sd[j];
    r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    corr[(size_t)i * R + j] = r;
    corr[(size_t)j * R + i] = r;
    const double key = r == r ? r : -INFINITY;
    const int idx = i * R + j;
    if (key > bv || (key == bv && idx < bi)) { bv = key; bi = idx; }
  }
  best_v[tid] = bv;
  best_i[tid] = bi;
  __syncthreads();                                                // (corr is read below by wave 0)
  for (int h = kOrdBlock / 2; h >= 1; h >>= 1) {
    if (tid < h) {
      const double ov = best_v[tid + h];
      const int oi = best_i[tid + h];
      if (ov > best_v[tid] || (ov == best_v[tid] && oi < best_i[tid])) { best_v[tid] = ov; best_i[tid] = oi; }
    }
    __syncthreads();
  }
  if (tid >= kWave) return;

  const int lane = tid;                                           // e. lane owns t = lane + 64 q
  const int first = best_i[0] / R, second = best_i[0] % R;        // (R >= 2: some pair i < j was seen)
  unsigned used = 0;
#pragma unroll
  for (int q = 0; q < kOrdMaxRows / kWave; ++q) {
    const int t = lane + kWave * q;
    if (t >= R || t == first || t == second) used |= 1u << q;
  }
  if (lane == 0) { order[0] = first; order[1] = second; }
  int last = second;
  for (int step = 2; step < R; ++step) {
    const double* row = corr + (size_t)last * R;
    double v = -INFINITY;
    int at = -1;
#pragma unroll
    for (int q = 0; q < kOrdMaxRows / kWave; ++q) {               // ascending t: >= keeps the highest of equal values
      const int t = lane + kWave * q;
      if (used >> q & 1u) continue;
      const double c = row[t];
      const double key = c == c ? c : -INFINITY;
      if (key >= v) { v = key; at = t; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double ov = __shfl_xor(v, o);
      const int oa = __shfl_xor(at, o);
      if (ov > v || (ov == v && oa > at)) { v = ov; at = oa; }
    }
    at = at < 0 ? 0 : at;                                          // (never: R - step >= 1 rows are unused)
    if ((at & (kWave - 1)) == lane) used |= 1u << (at / kWave);
    if (lane == 0) order[step] = at;
    last = at;
  }
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_pathway_order_supported(int64_t rows, int64_t outer, int64_t inner) {
  OrderShape s;
  return order_shape(rows, outer, inner, &s) ? 1 : 0;
}

extern "C" int64_t mlgnn_pathway_order_workspace_bytes(int64_t rows, int64_t outer, int64_t inner) {
  OrderShape s;
  if (!order_shape(rows, outer, inner, &s)) return MLGNN_E_SHAPE;
  return (int64_t)(order_mean_bytes(s) + order_gram_bytes(s) + order_part_bytes(s));
}

extern "C" int mlgnn_pathway_order(const double* x, int64_t rows, int64_t outer, int64_t inner, int64_t row_stride,
                                   int64_t outer_stride, double* corr, int32_t* order, int32_t* info, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  if (!x || !corr || !order || !info || !workspace) return MLGNN_E_NULL;
  OrderShape s;
  if (!order_shape(rows, outer, inner, &s) || row_stride < 0 || outer_stride < 0) return MLGNN_E_SHAPE;
  // the last element read: (rows - 1) row_stride + (outer - 1) outer_stride + inner - 1, below 4 GiB of doubles
  if (row_stride > kOrdMaxDoubles || outer_stride > kOrdMaxDoubles ||       // (so the sum below cannot overflow)
      (rows - 1) * row_stride + (outer - 1) * outer_stride + inner > kOrdMaxDoubles)
    return MLGNN_E_SHAPE;
  if (!aligned<8>(x, corr, static_cast<const char*>(workspace)) || !aligned<4>(order, info)) return MLGNN_E_ALIGN;
  if (workspace_bytes < mlgnn_pathway_order_workspace_bytes(rows, outer, inner)) return MLGNN_E_WORKSPACE;
  char* base = static_cast<char*>(workspace);
  double* mean = reinterpret_cast<double*>(base);
  double* gram = reinterpret_cast<double*>(base + order_mean_bytes(s));
  double* part = reinterpret_cast<double*>(base + order_mean_bytes(s) + order_gram_bytes(s));
  const int R = (int)rows, L = (int)s.L, nt = (int)(s.rp / kOrdTile), tiles = (int)s.tiles;
  const int lds_bytes = (int)(s.rp * kOrdLds * sizeof(double));
  hipError_t err = allow_dynamic_lds(pathway_order_gram_kernel, lds_bytes);
  if (err != hipSuccess) return (int)err;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(pathway_order_mean_kernel, dim3((unsigned)R), dim3(kOrdMeanBlock), 0, st, x, mean, L, (int)inner,
                     (size_t)row_stride, (size_t)outer_stride);
  hipLaunchKernelGGL(pathway_order_gram_kernel, dim3((unsigned)s.chunks), dim3(kOrdBlock), lds_bytes, st, x, mean, part,
                     R, L, (int)inner, (size_t)row_stride, (size_t)outer_stride, nt, tiles);
  hipLaunchKernelGGL(pathway_order_chain_kernel, dim3(1), dim3(kOrdBlock), 0, st, part, gram, corr, order, info, R, L,
                     (int)s.chunks, nt, tiles);
  return (int)hipGetLastError();
}
