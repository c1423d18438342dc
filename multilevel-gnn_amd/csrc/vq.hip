// The VQ-VAE quantiser (models/vae.py: VectorQuantizer.forward): nearest code word of every latent row, the
// straight-through output, the commitment + embedding loss and both gradients, without the [N, K] distance matrix.
//
//   z        [N, D]   the latent rows (N = B * 438, D = final_channels * pca_dim)
//   codebook [K, D]
//   index    [N]      argmin_k |z_n - w_k|^2 (int32)
//   out      [N, D]   z_n + (w_index[n] - z_n): two fp32 roundings, as `latents + (quantized - latents).detach()`
//   partials [ceil(N / 64)]  sum over a workgroup's rows of (w_index[n] - z_n)^2;  loss = m beta + m, m = sum / (N D)
//
// Forward, one launch: a workgroup owns 64 rows, one lane per row, the row in DP registers (D rounded up to a power of
// two, the tail zero).  The codebook passes through LDS in slabs of at most 48 KiB (rows padded to DP with zeros, so a
// pad term adds (0 - 0)^2 = 0); the four waves share a slab's codes by quarters and read them with broadcast reads (all
// lanes one address: no bank conflicts).  A distance is the fp32 sum of (z_d - w_d)^2: the even and the odd columns each
// in index order in the two halves of a packed fma chain, the two sums added -- a pure function of the two rows,
// whichever wave or loop computes it.  Every lane keeps its running minimum
// and index in registers across slabs; the four waves' candidates meet in LDS at the end.  Order of torch.argmin: a NaN
// distance is below every number, the first NaN wins, the lowest index wins a tie.  Then the 256 threads write
// out and sum the loss terms, reduced over lanes (xor butterfly) and over the waves in wave order.  A second,
// one-workgroup launch adds the partials in a fixed order.  No atomics.
// Backward: grad_z is one elementwise pass.  grad_codebook is a by-code pass: one wave per code scans the saved index
// vector (ballot over 64 rows at a time) and adds (w_k - z_n) over its members in ascending n, lane d owning column d
// (and d + 64); every element of [K, D] is written once, unused codes get zeros.
#include <climits>
#include <cmath>
#include "common.h"
#include "launch.h"
#include "mlgnn.h"

namespace mlgnn {
namespace {

constexpr int kVqRows = MLGNN_VQ_ROWS;        // rows per workgroup of the forward: one lane per row
constexpr int kVqSlabFloats = 12288;          // 48 KiB of code words per slab (three workgroups per CU)
constexpr int64_t kVqMaxCodes = 65536;
constexpr int64_t kVqMaxWidth = 128;          // two columns per lane in the by-code pass
static_assert(kVqRows == kWave, "one lane per row");

struct VqArgs {
  int N, K, D;
  int SK;           // codes per slab
  int vec;          // D == DP, D % 4 == 0 and 16-byte aligned operands: 16-byte loads of rows and code words
};

bool shape_ok(int64_t N, int64_t K, int64_t D) {
  if (N < 0 || K < 1 || K > kVqMaxCodes || D < 1 || D > kVqMaxWidth) return false;
  return N <= (((int64_t)1 << 30) - 1) / D;                                  // N * D floats below 4 GiB
}

int padded_width(int64_t D) {
  int dp = 2;
  while (dp < D) dp *= 2;
  return dp;
}

// torch.argmin's order on (distance, index): NaN below every number, the first NaN, the lowest index of a tie
__device__ __forceinline__ bool comes_before(float d, int k, float bd, int bk) {
  const bool dn = d != d, bn = bd != bd;
  if (dn || bn) return dn && (!bn || k < bk);
  return d < bd || (d == bd && k < bk);
}

typedef float f2 __attribute__((ext_vector_type(2)));

// |z - w_c|^2 for the C code words at w, w + DP, ...: even and odd columns run in the two halves of one packed chain
// (v_pk_add_f32, v_pk_fma_f32) and are added at the end -- the same operations in the same order for every (row, code),
// however many codes are in flight
template <int DP, int C>
__device__ __forceinline__ void distances_to(const f2 (&zr)[DP / 2], const float* w, float (&dist)[C]) {
  constexpr int V = DP < 4 ? DP : 4;
  f2 acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = f2{0.f, 0.f};
#pragma unroll
  for (int d = 0; d < DP; d += V) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float wv[V];
      load_vec<V>(wv, w + c * DP + d);
#pragma unroll
      for (int v = 0; v < V; v += 2) {
        const f2 t = zr[(d + v) / 2] - f2{wv[v], wv[v + 1]};
        acc[c] = __builtin_elementwise_fma(t, t, acc[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) dist[c] = acc[c].x + acc[c].y;
}

template <int DP>
__global__ __launch_bounds__(kBlock, DP < 128 ? 2 : 1) void vq_fwd_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                       int* __restrict__ index, float* __restrict__ out,
                                                       float* __restrict__ partials, VqArgs a) {
  constexpr int C = DP < 64 ? 4 : 2;                  // codes in flight: independent chains (two at the widest rows: registers)
  extern __shared__ float4 vq_lds[];
  __shared__ float cand_d[kWavesPerBlock][kVqRows];
  __shared__ int cand_k[kWavesPerBlock][kVqRows];
  __shared__ int best_k[kVqRows];
  __shared__ float red[kWavesPerBlock];
  float* slab = reinterpret_cast<float*>(vq_lds);

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int row0 = blockIdx.x * kVqRows;
  const int rows = a.N - row0 < kVqRows ? a.N - row0 : kVqRows;
  const bool live = lane < rows;

  f2 zr[DP / 2];
  {
    const float* zp = z + (size_t)(row0 + (live ? lane : 0)) * a.D;
    bool loaded = false;
    if constexpr (DP >= 4) {
      if (a.vec) {
#pragma unroll
        for (int d = 0; d < DP; d += 4) {
          float r[4];
          load_vec<4>(r, zp + d);
#pragma unroll
          for (int v = 0; v < 4; v += 2) zr[(d + v) / 2] = live ? f2{r[v], r[v + 1]} : f2{0.f, 0.f};
        }
        loaded = true;
      }
    }
    if (!loaded) {
#pragma unroll
      for (int d = 0; d < DP; d += 2)
        zr[d / 2] = f2{(live && d < a.D) ? zp[d] : 0.f, (live && d + 1 < a.D) ? zp[d + 1] : 0.f};
    }
  }

  float bd = INFINITY;
  int bk = INT_MAX;                                   // "no code yet": loses every tie
  for (int k0 = 0; k0 < a.K; k0 += a.SK) {
    const int cnt = a.K - k0 < a.SK ? a.K - k0 : a.SK;
    __syncthreads();                                  // the previous slab has been read
    if (a.vec) {
      for (int e = threadIdx.x * 4; e < cnt * DP; e += kBlock * 4) {
        float r[4];
        load_vec<4>(r, cb + (size_t)k0 * DP + e);
        store_vec<4>(slab + e, r);
      }
    } else {
      for (int e = threadIdx.x; e < cnt * DP; e += kBlock) {
        const int k = e / DP, d = e - k * DP;
        slab[e] = d < a.D ? cb[(size_t)(k0 + k) * a.D + d] : 0.f;
      }
    }
    __syncthreads();

    const int share = (cnt + kWavesPerBlock - 1) / kWavesPerBlock;
    const int kb = wave * share;
    const int ke = kb + share < cnt ? kb + share : cnt;
    int k = kb;
    for (; k + C <= ke; k += C) {
      float dist[C];
      distances_to<DP, C>(zr, slab + k * DP, dist);
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (comes_before(dist[c], k0 + k + c, bd, bk)) { bd = dist[c]; bk = k0 + k + c; }
    }
    for (; k < ke; ++k) {
      float dist[1];
      distances_to<DP, 1>(zr, slab + k * DP, dist);
      if (comes_before(dist[0], k0 + k, bd, bk)) { bd = dist[0]; bk = k0 + k; }
    }
  }

  cand_d[wave][lane] = bd;
  cand_k[wave][lane] = bk;
  __syncthreads();
  if (wave == 0) {                                    // K >= 1: wave 0 has seen code 0, so bk is a code
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) {
      const float d = cand_d[w][lane];
      const int kk = cand_k[w][lane];
      if (comes_before(d, kk, bd, bk)) { bd = d; bk = kk; }
    }
    best_k[lane] = bk;
    if (live) index[row0 + lane] = bk;
  }
  __syncthreads();

  float s = 0.f;
  const size_t base = (size_t)row0 * a.D;
  for (int e = threadIdx.x; e < rows * a.D; e += kBlock) {
    const int r = e / a.D, d = e - r * a.D;
    const float zv = z[base + e];
    const float t = cb[(size_t)best_k[r] * a.D + d] - zv;
    out[base + e] = zv + t;
    s = fmaf(t, t, s);
  }
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = red[0];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) t += red[w];
    partials[blockIdx.x] = t;
  }
}

// loss = m beta + m, m = (sum of the partials) / count: one workgroup, fixed order
__global__ __launch_bounds__(kBlock) void vq_loss_kernel(const float* __restrict__ partials, int nblk, float count, float beta,
                                                        float* __restrict__ loss) {
  __shared__ float red[kWavesPerBlock];
  float s = 0.f;
  for (int i = threadIdx.x; i < nblk; i += kBlock) s += partials[i];
  s = wave_sum(s);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = red[0];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) t += red[w];
    const float m = t / count;
    *loss = __fmul_rn(m, beta) + m;
  }
}

// grad_z = g_out + g_loss * coef * (z - w_index), coef = 2 beta / (N D); an absent cotangent is zero
__global__ __launch_bounds__(kBlock) void vq_grad_z_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                          const int* __restrict__ index, const float* __restrict__ g_out,
                                                          const float* __restrict__ g_loss, float* __restrict__ grad_z,
                                                          float coef, size_t total, int D) {
  const float scale = g_loss ? *g_loss * coef : 0.f;
  for (size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kBlock) {
    float g = g_out ? g_out[e] : 0.f;
    if (g_loss) {
      const size_t n = e / D;
      const int d = (int)(e - n * D);
      g = fmaf(scale, z[e] - cb[(size_t)index[n] * D + d], g);
    }
    grad_z[e] = g;
  }
}

// grad_codebook[k] = g_loss * coef * sum over {n : index[n] == k}, ascending, of (w_k - z_n), coef = 2 / (N D)
__global__ __launch_bounds__(kBlock) void vq_grad_codebook_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                                 const int* __restrict__ index,
                                                                 const float* __restrict__ g_loss,
                                                                 float* __restrict__ grad_cb, float coef, int N, int K, int D) {
  const int lane = threadIdx.x & (kWave - 1);
  const int k = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + threadIdx.x / kWave));
  if (k >= K) return;                                 // (no barrier below)
  constexpr int G = 16;                               // index loads in flight: the scan is bound by their latency
  const bool c0 = lane < D, c1 = lane + kWave < D;
  const float w0 = c0 ? cb[(size_t)k * D + lane] : 0.f;
  const float w1 = c1 ? cb[(size_t)k * D + lane + kWave] : 0.f;
  float a0 = 0.f, a1 = 0.f;
  for (int n0 = 0; n0 < N; n0 += G * kWave) {
    unsigned long long member[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int n = n0 + j * kWave + lane;
      member[j] = __ballot(n < N && index[n] == k);
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      unsigned long long m = member[j];
      while (m) {                                     // up to four member rows in flight, added in ascending n
        int nn[4];
        float v0[4], v1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          nn[u] = -1;
          if (m) {
            nn[u] = n0 + j * kWave + (__ffsll((long long)m) - 1);
            m &= m - 1;
            const float* row = z + (size_t)nn[u] * D;
            v0[u] = c0 ? row[lane] : 0.f;
            v1[u] = c1 ? row[lane + kWave] : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (nn[u] >= 0) { a0 += w0 - v0[u]; a1 += w1 - v1[u]; }
      }
    }
  }
  const float scale = *g_loss * coef;
  if (c0) grad_cb[(size_t)k * D + lane] = scale * a0;
  if (c1) grad_cb[(size_t)k * D + lane + kWave] = scale * a1;
}

template <int DP>
int launch_fwd(const float* z, const float* cb, int* index, float* out, float* partials, const VqArgs& a, int nblk,
               hipStream_t st) {
  const size_t lds = (size_t)a.SK * DP * sizeof(float);
  hipLaunchKernelGGL((vq_fwd_kernel<DP>), dim3((unsigned)nblk), dim3(kBlock), lds, st, z, cb, index, out, partials, a);
  return (int)hipGetLastError();
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_vq_supported(int64_t N, int64_t K, int64_t D) { return shape_ok(N, K, D) ? 1 : 0; }

extern "C" int mlgnn_vq_fwd(const float* z, const float* codebook, int32_t* index, float* out, float* partials, float* loss,
                            float beta, int64_t N, int64_t K, int64_t D, void* stream) {
  if (!shape_ok(N, K, D)) return MLGNN_E_SHAPE;
  if (N == 0) return 0;
  if (!z || !codebook || !index || !out || !partials) return MLGNN_E_NULL;
  const int dp = padded_width(D);
  VqArgs a;
  a.N = (int)N; a.K = (int)K; a.D = (int)D;
  const int most = kVqSlabFloats / dp;                                      // >= 96 codes
  a.SK = K < most ? (int)K : most;
  a.vec = (dp == D && D % 4 == 0 && aligned(z, codebook)) ? 1 : 0;
  const int nblk = (int)((N + kVqRows - 1) / kVqRows);
  hipStream_t st = as_stream(stream);
  int rc = MLGNN_E_SHAPE;
  dispatch_int<2, 4, 8, 16, 32, 64, 128>(dp, [&](auto w) {
    rc = launch_fwd<decltype(w)::value>(z, codebook, index, out, partials, a, nblk, st);
  });
  if (rc != 0 || !loss) return rc;
  hipLaunchKernelGGL(vq_loss_kernel, dim3(1), dim3(kBlock), 0, st, partials, nblk, (float)((double)N * (double)D), beta, loss);
  return (int)hipGetLastError();
}

extern "C" int mlgnn_vq_bwd(const float* z, const float* codebook, const int32_t* index, const float* g_out,
                            const float* g_loss, float* grad_z, float* grad_codebook, float beta, int64_t N, int64_t K,
                            int64_t D, void* stream) {
  if (!shape_ok(N, K, D)) return MLGNN_E_SHAPE;
  if (N == 0) return 0;
  if (!z || !codebook || !index) return MLGNN_E_NULL;
  hipStream_t st = as_stream(stream);
  const double count = (double)N * (double)D;
  if (grad_z) {
    const size_t total = (size_t)N * (size_t)D;
    size_t blocks = (total + kBlock - 1) / kBlock;
    if (blocks > (size_t)kMaxBlocks) blocks = kMaxBlocks;
    hipLaunchKernelGGL(vq_grad_z_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, z, codebook, index, g_out, g_loss, grad_z,
                       (float)(2.0 * (double)beta / count), total, (int)D);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
  }
  if (grad_codebook) {
    if (!g_loss)                                                            // the straight-through output sends nothing here
      return (int)hipMemsetAsync(grad_codebook, 0, (size_t)K * (size_t)D * sizeof(float), st);
    const int blocks = (int)((K + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(vq_grad_codebook_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, z, codebook, index, g_loss,
                       grad_codebook, (float)(2.0 / count), (int)N, (int)K, (int)D);
    return (int)hipGetLastError();
  }
  return 0;
}
