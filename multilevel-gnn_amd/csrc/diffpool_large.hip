// DiffPool soft-assignment contraction for LARGE pooled graphs (BASELINE configs[4]: 4096 nodes, 1024 clusters, 256
// channels, bf16 storage / fp32 accumulation): the chain of big dense products on the bf16 matrix cores
// (csrc/gemm_nt.hip) with everything around them fused into producers / epilogues.
//
// Reference: torch_geometric.nn.dense_diff_pool as called from DiffPoolLayer.forward (models/diff_pooling.py:59-65):
//     S = softmax(s, -1);  X' = S^T Z;  A' = S^T A S;  link = ||A - S S^T||_F / numel(A);
//     ent = mean_n( sum_k -S log(S + 1e-15) )
//
// What is computed (one pooled graph; all big operands bf16, every sum in fp32):
//   * S~ = bf16(softmax(logits)) [N,K] and its transpose; entropy from the fp32 softmax in the same pass.
//   * T = A S~ [N,K] (34 GFLOP at configs[4]) -- written as T and as T^T by the product's epilogue, which also
//     accumulates <S~, T> from the fp32 accumulators.
//   * [A' | G] = S~^T [T | S~]  (G = S~^T S~, [K,K]) as ONE split-K product, X' = S~^T Z as another.
//   * The link term never forms the [N,N] matrix S S^T (another 34 GFLOP):
//         ||A - S S^T||_F^2 = ||A||_F^2 - 2 <A, S S^T> + ||S S^T||_F^2 = ||A||_F^2 - 2 <S, A S> + ||S^T S||_F^2
//     (exact identities; <A, S S^T> = sum_ik S_ik (A S)_ik needs no symmetry of A).  All three terms are sums of
//     fp32 partials in a fixed order.  The subtraction cancels when S S^T ~ A: the relative error of link^2 is
//     ~1e-6 * ||A||_F^2 / ||A - S S^T||_F^2 -- negligible unless the assignment reproduces the adjacency to
//     better than 1 %, where link (a regulariser) is ~0 anyway.  Its gradient is formed the same way:
//         d link / dS = c (-(A + A^T) S + 2 S G),   c = grad_link / (numel(A) * ||A - S S^T||_F)
//   * backward:  dS = Z dX'^T + T (dA' - cI)^T... all four terms summed by ONE multi-term product
//         dS = [Z | T | T2 | S~] [dX' | dA' - cI | dA'^T - cI | 2c G]^T,      T2 = A^T S~
//     then the softmax backward (with the entropy term) as one streaming pass; dZ = S~ dX'.
// No atomics; every reduction is a fixed-order sum of per-workgroup partials: bitwise reproducible.
// The split-K reduce is csrc/gemm_chain.hip; the fp32 three-term form of this chain is csrc/diffpool_large_f32.hip.
#include "common.h"
#include "launch.h"
#include "gemm_chain.h"

namespace mlgnn {

constexpr int kDplSqBlocks = 256;        // workgroups (= partial sums) of ||A||_F^2
constexpr int kProRows = 32;             // rows of the logits one softmax workgroup owns
constexpr int kProCols = 128;            // columns per transposed write-out
constexpr int kProPitch = kProCols + 2;  // LDS pitch of the staging image (bf16 elements)

template <typename T>
__device__ __forceinline__ float dpl_load(const T* p, size_t i) {
  if constexpr (sizeof(T) == 4) return reinterpret_cast<const float*>(p)[i];
  else return bf16_to_f32(reinterpret_cast<const uint16_t*>(p)[i]);
}
__device__ __forceinline__ float dpl_load_dt(const void* p, size_t i, int f32) {
  return f32 ? reinterpret_cast<const float*>(p)[i] : bf16_to_f32(reinterpret_cast<const uint16_t*>(p)[i]);
}

// 64 x 64 bf16 tile transpose through LDS: in [.., ld_in] -> out [.., ld_out]; 256 threads; tile = [64][66]
__device__ __forceinline__ void dpl_transpose_tile(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                   int64_t ld_in, int64_t ld_out, int r0, int c0, uint16_t (*tile)[66],
                                                   int tid) {
  // 64 rows x 128 B: 8 lanes per row, 16 bytes each; 256 threads = 32 rows per pass
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int r = pass * 32 + (tid >> 3), ch = tid & 7;
    const uint4 v = *reinterpret_cast<const uint4*>(in + (size_t)(r0 + r) * ld_in + c0 + ch * 8);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      tile[r][ch * 8 + 2 * i] = (uint16_t)(w[i] & 0xffff);
      tile[r][ch * 8 + 2 * i + 1] = (uint16_t)(w[i] >> 16);
    }
  }
  __syncthreads();
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int c = pass * 32 + (tid >> 3), ch = tid & 7;
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)tile[ch * 8 + 2 * i][c] | ((uint32_t)tile[ch * 8 + 2 * i + 1][c] << 16);
    *reinterpret_cast<uint4*>(out + (size_t)(c0 + c) * ld_out + r0 + ch * 8) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// sum of squares of a bf16 matrix (contiguous, n8 groups of 8) over workgroup `b` of `nb`
__device__ __forceinline__ float dpl_sumsq_part(const uint4* __restrict__ x, int64_t n8, int b, int nb) {
  float acc = 0.f;
  for (int64_t i = (int64_t)b * blockDim.x + threadIdx.x; i < n8; i += (int64_t)nb * blockDim.x) {
    const uint4 v = x[i];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = __builtin_bit_cast(float, w[j] << 16), c = __builtin_bit_cast(float, w[j] & 0xffff0000u);
      acc += a * a + c * c;
    }
  }
  return acc;
}

// ---- forward prologue: ONE launch, workgroups by role ------------------------------------------------------------
//   [0, nb_sm)           32 rows of the logits each: S~ = bf16(softmax) written as S [N,K] AND as S^T [K,N] (128-column
//                        slabs staged in LDS, 64-byte runs of S^T per column), entropy partial from the fp32 softmax
//   [nb_sm, +nb_zt)      64 x 64 tiles of Z -> Z^T
//   [.., +nb_sq)         ||A||_F^2 partials
// (round 2 ran these as four launches: softmax, two transposes, sum of squares.)
struct DplProArgs {
  const void* logits; uint16_t* S; uint16_t* St; float* ent_partial;
  const uint16_t* z; uint16_t* Zt;
  const uint4* adj; int64_t adj_n8; float* a2_partial;
  int N, K, C, nb_sm, nb_zt, nb_sq;
  // grouped launch: graph blockIdx.y of the batch; strides in elements of each pointer's type (ws: bytes between the
  // per-graph workspaces that hold St, Zt and the partial sums); adj_batch graphs have an adjacency of their own
  int64_t s_rowsK, s_z, s_adj8, ws_stride; int adj_batch;
};

constexpr int kProThreads = 1024;        // 16 wavefronts: two rows of the softmax each
constexpr int kProWaves = kProThreads / 64;
constexpr int kProRowsPerWave = kProRows / kProWaves;

constexpr int kProWide = 512, kProWidePitch = kProWide + 8;      // CH > 0: 512-column slabs, rows held in registers

// CH = K / 512 in {1, 2, 4}: the two rows of a wavefront stay in registers (one read of the logits, 16-byte accesses,
// K / 512 slabs of 512 columns); CH = 0: any K (multiple of 128), rows re-read from the cache, 128-column slabs.
template <typename T, int CH>
__global__ __launch_bounds__(kProThreads) void dpl_prologue_kernel(const DplProArgs p_in) {
  constexpr int kLdsElems = 4 * 64 * 66 + 64;
  static_assert(kLdsElems >= kProRows * kProWidePitch && kLdsElems >= kProRows * kProPitch, "staging image");
  __shared__ __attribute__((aligned(16))) uint16_t lds_all[kLdsElems];
  uint16_t (*lds)[64 * 66] = reinterpret_cast<uint16_t(*)[64 * 66]>(lds_all);    // four transpose tiles
  __shared__ float wsum[kProWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x;
  DplProArgs p = p_in;
  {
    const int64_t bz = blockIdx.y;
    p.logits = static_cast<const T*>(p.logits) + bz * p.s_rowsK;
    p.S += bz * p.s_rowsK;
    p.St += bz * (p.ws_stride / 2);
    p.Zt += bz * (p.ws_stride / 2);
    p.z += bz * p.s_z;
    p.adj += bz * p.s_adj8;
    p.ent_partial += bz * (p.ws_stride / 4);
    p.a2_partial += bz * (p.ws_stride / 4);
    if (b >= p.nb_sm + p.nb_zt && bz >= p.adj_batch) return;        // a shared adjacency is summed once
  }
  if (b >= p.nb_sm + p.nb_zt) {
    float acc = wave_sum(dpl_sumsq_part(p.adj, p.adj_n8, b - p.nb_sm - p.nb_zt, p.nb_sq));
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      float tot = 0.f;
#pragma unroll
      for (int i = 0; i < kProWaves; ++i) tot += wsum[i];
      p.a2_partial[b - p.nb_sm - p.nb_zt] = tot;
    }
    return;
  }
  if (b >= p.nb_sm) {
    // four 64 x 64 tiles of Z per workgroup, one per group of 256 threads (a group past the last tile repeats it)
    const int tiles_c = p.C / 64, tiles = (p.N / 64) * tiles_c;
    const int t = min((b - p.nb_sm) * 4 + (int)(threadIdx.x >> 8), tiles - 1);
    dpl_transpose_tile(p.z, p.Zt, p.C, p.N, (t / tiles_c) * 64, (t % tiles_c) * 64,
                       reinterpret_cast<uint16_t(*)[66]>(lds[threadIdx.x >> 8]), threadIdx.x & 255);
    return;
  }
  const T* logits = static_cast<const T*>(p.logits);
  const int K = p.K;
  const int row0 = b * kProRows + wave * kProRowsPerWave;
  if constexpr (CH > 0) {
    float v[kProRowsPerWave][CH][8];
    float ent = 0.f;
#pragma unroll
    for (int j = 0; j < kProRowsPerWave; ++j) {
      const T* lr = logits + (size_t)(row0 + j) * K;
      float m = -3.0e38f;
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        load_t<T, 8>(v[j][q], lr + q * kProWide + lane * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) m = fmaxf(m, v[j][q][i]);
      }
      m = wave_max(m);
      float sum = 0.f;
#pragma unroll
      for (int q = 0; q < CH; ++q)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          v[j][q][i] = __expf(v[j][q][i] - m);
          sum += v[j][q][i];
        }
      const float inv = 1.0f / wave_sum(sum);
#pragma unroll
      for (int q = 0; q < CH; ++q)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          v[j][q][i] *= inv;
          ent -= v[j][q][i] * __logf(v[j][q][i] + kDplEps);
        }
    }
#pragma unroll
    for (int q = 0; q < CH; ++q) {
#pragma unroll
      for (int j = 0; j < kProRowsPerWave; ++j) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = pack2_bf16(v[j][q][2 * i], v[j][q][2 * i + 1]);
        const uint4 pk = make_uint4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<uint4*>(p.S + (size_t)(row0 + j) * K + q * kProWide + lane * 8) = pk;
        *reinterpret_cast<uint4*>(lds_all + (wave * kProRowsPerWave + j) * kProWidePitch + lane * 8) = pk;
      }
      __syncthreads();
      {
        // 512 columns x 32 rows: thread -> (column, 16 rows) = one 32-byte run of S^T
        const int col = threadIdx.x >> 1, half = threadIdx.x & 1;
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int r = half * 16 + 2 * i;
          w[i] = (uint32_t)lds_all[r * kProWidePitch + col] | ((uint32_t)lds_all[(r + 1) * kProWidePitch + col] << 16);
        }
        uint16_t* dst = p.St + (size_t)(q * kProWide + col) * p.N + b * kProRows + half * 16;
        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<uint4*>(dst + 8) = make_uint4(w[4], w[5], w[6], w[7]);
      }
      if (q + 1 < CH) __syncthreads();
    }
    ent = wave_sum(ent);
    if (lane == 0) wsum[wave] = ent;
    __syncthreads();
    if (threadIdx.x == 0) {
      float tot = 0.f;
#pragma unroll
      for (int i = 0; i < kProWaves; ++i) tot += wsum[i];
      p.ent_partial[b] = tot;
    }
    return;
  }
  float mx[kProRowsPerWave], inv[kProRowsPerWave];
#pragma unroll
  for (int j = 0; j < kProRowsPerWave; ++j) {
    const T* lr = logits + (size_t)(row0 + j) * K;
    float m = -3.0e38f;
    for (int k = lane * 8; k < K; k += 512) {
      float v[8];
      load_t<T, 8>(v, lr + k);
#pragma unroll
      for (int i = 0; i < 8; ++i) m = fmaxf(m, v[i]);
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
      float v[8];
      load_t<T, 8>(v, lr + k);
#pragma unroll
      for (int i = 0; i < 8; ++i) sum += __expf(v[i] - m);
    }
    sum = wave_sum(sum);
    mx[j] = m;
    inv[j] = 1.0f / sum;
  }
  float ent = 0.f;
  uint16_t* img = lds[0];
  for (int c0 = 0; c0 < K; c0 += kProCols) {
#pragma unroll
    for (int j = 0; j < kProRowsPerWave; ++j) {
      const size_t at = (size_t)(row0 + j) * K + c0 + lane * 2;
      const float s0 = __expf(dpl_load(logits, at) - mx[j]) * inv[j];
      const float s1 = __expf(dpl_load(logits, at + 1) - mx[j]) * inv[j];
      ent -= s0 * __logf(s0 + kDplEps) + s1 * __logf(s1 + kDplEps);
      const uint32_t w = pack2_bf16(s0, s1);
      *reinterpret_cast<uint32_t*>(p.S + at) = w;
      *reinterpret_cast<uint32_t*>(img + (wave * kProRowsPerWave + j) * kProPitch + lane * 2) = w;
    }
    __syncthreads();
    {
      // 128 columns x 32 rows: thread -> (column, 4 rows) = one 8-byte run of S^T
      const int col = threadIdx.x >> 3, part = threadIdx.x & 7;
      uint32_t w[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int r = part * 4 + 2 * i;
        w[i] = (uint32_t)img[r * kProPitch + col] | ((uint32_t)img[(r + 1) * kProPitch + col] << 16);
      }
      *reinterpret_cast<uint2*>(p.St + (size_t)(c0 + col) * p.N + b * kProRows + part * 4) = make_uint2(w[0], w[1]);
    }
    __syncthreads();
  }
  ent = wave_sum(ent);
  if (lane == 0) wsum[wave] = ent;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < kProWaves; ++i) tot += wsum[i];
    p.ent_partial[b] = tot;
  }
}

// dlogits = S (ds - <ds, S>),  ds = dS + c_ent * d/dS(-S log(S + eps)),   S recomputed in fp32 from the logits.
// One wavefront per row, 8 consecutive elements per lane and pass (16-byte loads of the bf16 logits, 2 x 16 of dS);
// the four passes over a row re-read it from the cache.
template <typename T>
__global__ __launch_bounds__(256) void dpl_softmax_bwd_kernel(const T* __restrict__ logits, const float* __restrict__ ds_in,
                                                              const float* __restrict__ coef, T* __restrict__ dlogits,
                                                              int N, int K, int64_t ds_stride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float c_ent = coef[1];
  logits += (size_t)blockIdx.y * N * K;                             // graph of a grouped launch
  dlogits += (size_t)blockIdx.y * N * K;
  ds_in += (size_t)blockIdx.y * ds_stride;
  for (int row = blockIdx.x * 4 + wave; row < N; row += gridDim.x * 4) {
    const T* lr = logits + (size_t)row * K;
    const float* dr = ds_in + (size_t)row * K;
    float mx = -3.0e38f;
    for (int k = lane * 8; k < K; k += 512) {
      float v[8];
      load_t<T, 8>(v, lr + k);
#pragma unroll
      for (int i = 0; i < 8; ++i) mx = fmaxf(mx, v[i]);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
      float v[8];
      load_t<T, 8>(v, lr + k);
#pragma unroll
      for (int i = 0; i < 8; ++i) sum += __expf(v[i] - mx);
    }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    float dot = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
      float v[8], d[8];
      load_t<T, 8>(v, lr + k);
      load_vec<8>(d, dr + k);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float s = __expf(v[i] - mx) * inv;
        const float g = d[i] - c_ent * (__logf(s + kDplEps) + s / (s + kDplEps));
        dot += g * s;
      }
    }
    dot = wave_sum(dot);
    for (int k = lane * 8; k < K; k += 512) {
      float v[8], d[8], o[8];
      load_t<T, 8>(v, lr + k);
      load_vec<8>(d, dr + k);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float s = __expf(v[i] - mx) * inv;
        const float g = d[i] - c_ent * (__logf(s + kDplEps) + s / (s + kDplEps));
        o[i] = s * (g - dot);
      }
      store_t<T, 8>(dlogits + (size_t)row * K + k, o);
    }
  }
}

__device__ float dpl_block_sum(const float* p, int n, float* sh) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += p[i];
  acc = wave_sum(acc);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ void dpl_final(const DplFinalArgs& p, float* sh) {
  float sq = 0.f, ent = 0.f;
  for (int b = 0; b < p.batch; ++b) {
    const int64_t o = (int64_t)b * p.ws_floats;
    const float a2 = dpl_block_sum(p.a2 + (b < p.adj_batch ? o : 0), p.n_a2, sh);
    const float dot = dpl_block_sum(p.dot + o, p.n_dot, sh);
    const float g2 = dpl_block_sum(p.g2 + o, p.n_g2, sh);
    ent += dpl_block_sum(p.ent + o, p.n_ent, sh);
    sq += fmaxf(a2 - 2.f * dot + g2, 0.f);
  }
  if (threadIdx.x == 0) {
    const float norm = sqrtf(sq);
    p.stats[0] = norm * p.inv_numel;
    p.stats[1] = ent * p.inv_rows;
    p.stats[2] = norm;
    if (p.scal_f32) {
      reinterpret_cast<float*>(p.scal_out)[0] = p.stats[0];
      reinterpret_cast<float*>(p.scal_out)[1] = p.stats[1];
    } else {
      reinterpret_cast<uint16_t*>(p.scal_out)[0] = f32_to_bf16(p.stats[0]);
      reinterpret_cast<uint16_t*>(p.scal_out)[1] = f32_to_bf16(p.stats[1]);
    }
  }
}

__global__ __launch_bounds__(256) void dpl_final_kernel(const DplFinalArgs p) {
  __shared__ float sh[4];
  dpl_final(p, sh);
}

// ---- backward operand preparation: ONE launch, workgroups by role --------------------------------------------------
// coef = { c = grad_link / (numel(adj) * ||adj - S S^T||_F),  grad_ent / N }  from the scalar cotangents (device)
//   [0, nb_ga)        64 x 64 tiles of  b1 = ga - cI,  b2 = ga^T - cI (the transposed tile through LDS),  b3 = 2c G
//   [nb_ga, +nb_gx)   64 x 64 tiles of gx [K,C] -> bf16 copy and its transpose [C,K]
//   [.., +nb_at)      64 x 64 tiles of A -> A^T (only when adj is not promised symmetric)
// (round 2: coef, prep_ga, to_bf16 and one or two transposes as separate launches.)
struct DplPrepArgs {
  const void* g_link; const void* g_ent; int scal_f32; const float* stats; float* coef; float inv_numel, inv_rows;
  const void* ga; const void* gx; int g_f32; const uint16_t* G;
  uint16_t *b1, *b2, *b3, *gxb, *gxt;
  const uint16_t* adj; uint16_t* At;
  int N, K, C, nb_ga, nb_gx, nb_at;
  // grouped launch: bytes between the per-graph forward (G) / backward (b1 .. At) workspaces; element stride of adj
  int64_t fws_stride, bws_stride, s_adj;
};

__global__ __launch_bounds__(256) void dpl_prep_kernel(const DplPrepArgs p_in) {
  __shared__ __attribute__((aligned(16))) float ldsf[64 * 65];
  const int b = blockIdx.x;
  DplPrepArgs p = p_in;
  {
    const int64_t bz = blockIdx.y;
    const int64_t kk = (int64_t)p.K * p.K, kc = (int64_t)p.K * p.C;
    p.ga = p.g_f32 ? (const void*)(static_cast<const float*>(p.ga) + bz * kk) : (const void*)(static_cast<const uint16_t*>(p.ga) + bz * kk);
    p.gx = p.g_f32 ? (const void*)(static_cast<const float*>(p.gx) + bz * kc) : (const void*)(static_cast<const uint16_t*>(p.gx) + bz * kc);
    p.G += bz * (p.fws_stride / 2);
    const int64_t o = bz * (p.bws_stride / 2);
    p.b1 += o; p.b2 += o; p.b3 += o; p.gxb += o; p.gxt += o;
    p.adj += bz * p.s_adj;
    if (p.At) p.At += o;
  }
  const float c = dpl_load_dt(p.g_link, 0, p.scal_f32) * p.inv_numel / p.stats[2];
  if (b == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    p.coef[0] = c;
    p.coef[1] = dpl_load_dt(p.g_ent, 0, p.scal_f32) * p.inv_rows;
  }
  // tile roles: thread -> (row r = pass * 32 + tid / 8, 8 consecutive columns ch * 8 ..) as in dpl_transpose_tile
  const int trow = threadIdx.x >> 3, ch = threadIdx.x & 7;
  if (b < p.nb_ga) {
    const int tiles = p.K / 64, tr = b / tiles, tc = b % tiles;
    // the source tile of ga^T: rows of block tc, columns of block tr
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int r = pass * 32 + trow;
      float v[8];
      const size_t at = (size_t)(tc * 64 + r) * p.K + tr * 64 + ch * 8;
      if (p.g_f32) load_vec<8>(v, reinterpret_cast<const float*>(p.ga) + at);
      else load_t<bf16_t, 8>(v, reinterpret_cast<const bf16_t*>(p.ga) + at);
#pragma unroll
      for (int i = 0; i < 8; ++i) ldsf[r * 65 + ch * 8 + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int r = pass * 32 + trow;
      const int row = tr * 64 + r, col = tc * 64 + ch * 8;
      const size_t at = (size_t)row * p.K + col;
      float v[8], g[8], o1[8], o2[8], o3[8];
      if (p.g_f32) load_vec<8>(v, reinterpret_cast<const float*>(p.ga) + at);
      else load_t<bf16_t, 8>(v, reinterpret_cast<const bf16_t*>(p.ga) + at);
      load_t<bf16_t, 8>(g, reinterpret_cast<const bf16_t*>(p.G) + at);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = row == col + i ? c : 0.f;
        o1[i] = v[i] - d;
        o2[i] = ldsf[(ch * 8 + i) * 65 + r] - d;
        o3[i] = 2.f * c * g[i];
      }
      store_t<bf16_t, 8>(reinterpret_cast<bf16_t*>(p.b1) + at, o1);
      store_t<bf16_t, 8>(reinterpret_cast<bf16_t*>(p.b2) + at, o2);
      store_t<bf16_t, 8>(reinterpret_cast<bf16_t*>(p.b3) + at, o3);
    }
    return;
  }
  if (b < p.nb_ga + p.nb_gx) {
    const int t = b - p.nb_ga, tiles_c = p.C / 64, r0 = (t / tiles_c) * 64, c0 = (t % tiles_c) * 64;
    uint16_t* tile = reinterpret_cast<uint16_t*>(ldsf);                // [64][66]
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int r = pass * 32 + trow;
      const size_t at = (size_t)(r0 + r) * p.C + c0 + ch * 8;
      float v[8];
      if (p.g_f32) load_vec<8>(v, reinterpret_cast<const float*>(p.gx) + at);
      else load_t<bf16_t, 8>(v, reinterpret_cast<const bf16_t*>(p.gx) + at);
      store_t<bf16_t, 8>(reinterpret_cast<bf16_t*>(p.gxb) + at, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) tile[r * 66 + ch * 8 + i] = f32_to_bf16(v[i]);
    }
    __syncthreads();
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int cc = pass * 32 + trow;                                 // column of the tile = row of the transpose
      uint32_t w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        w[i] = (uint32_t)tile[(ch * 8 + 2 * i) * 66 + cc] | ((uint32_t)tile[(ch * 8 + 2 * i + 1) * 66 + cc] << 16);
      *reinterpret_cast<uint4*>(p.gxt + (size_t)(c0 + cc) * p.K + r0 + ch * 8) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return;
  }
  const int t = b - p.nb_ga - p.nb_gx, tiles_c = p.N / 64;
  dpl_transpose_tile(p.adj, p.At, p.N, p.N, (t / tiles_c) * 64, (t % tiles_c) * 64, reinterpret_cast<uint16_t(*)[66]>(ldsf),
                     threadIdx.x);
}

struct DplLayout {       // byte offsets into the forward workspace (kept for the backward) and scratch
  size_t stack, T, G, scratch, total;      // stack [2K + C, N]: T^T, S~^T, Z^T;  T [N,K];  G [K,K]
  size_t slab, part_a2, part_dot, part_g2, part_ent;
  int splits_ag;
};

DplLayout dpl_layout(int64_t N, int64_t K, int64_t C) {
  DplLayout L;
  size_t o = 0;
  L.stack = o; o += align256((size_t)(2 * K + C) * N * 2);
  L.T = o; o += align256((size_t)N * K * 2);
  L.G = o; o += align256((size_t)K * K * 2);
  L.scratch = o;
  // [A' | G | X'] = S~^T [T | S~ | Z] is ONE product over the whole stack, split along K into about 1.5 workgroups
  // per CU (measured at 4096 / 1024 / 256, 144 tiles: 2 / 3 / 4 / 6 splits 0.110 / 0.104 / 0.109 / 0.113 ms forward)
  const int tiles_agx = (int)((K / kGemmTile) * ((2 * K + C) / kGemmTile));
  int sp = (384 + tiles_agx / 2) / tiles_agx;
  if (sp > (int)(N / kGemmBK)) sp = (int)(N / kGemmBK);
  L.splits_ag = sp < 1 ? 1 : sp;
  L.slab = o; o += align256((size_t)L.splits_ag * K * (2 * K + C) * 4);
  L.part_a2 = o; o += align256(kReducePartials * 4);
  L.part_dot = o; o += align256((size_t)(N / kGemmTile) * (K / kGemmTile) * 4);
  L.part_g2 = o; o += align256(kReducePartials * 4);
  L.part_ent = o; o += align256(kReducePartials * 4);
  L.total = o;
  return L;
}

void dpl_final_launch(const DplFinalArgs& f, hipStream_t st) {
  hipLaunchKernelGGL(dpl_final_kernel, dim3(1), dim3(256), 0, st, f);
}

// four rows (one per wavefront) per workgroup and pass
template <typename T>
static void dpl_softmax_bwd_launch(const T* logits, const float* ds, const float* coef, T* dlogits, int N, int K,
                                   int64_t ds_stride, int batch, hipStream_t st) {
  const int sm_blocks = (N + 3) / 4 < 1024 ? (N + 3) / 4 : 1024;
  hipLaunchKernelGGL(dpl_softmax_bwd_kernel<T>, dim3(sm_blocks, batch), dim3(256), 0, st, logits, ds, coef, dlogits, N, K,
                     ds_stride);
}

void dpl_softmax_bwd_f32_launch(const float* logits, const float* ds, const float* coef, float* dlogits, int N, int K,
                                int64_t ds_stride, int batch, hipStream_t st) {
  dpl_softmax_bwd_launch<float>(logits, ds, coef, dlogits, N, K, ds_stride, batch, st);
}

}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_diffpool_large_supported(int64_t N, int64_t K, int64_t C) { return dpl_supported(N, K, C) ? 1 : 0; }

extern "C" int64_t mlgnn_diffpool_large_workspace_bytes(int64_t N, int64_t K, int64_t C) {
  if (!dpl_supported(N, K, C)) return MLGNN_E_SHAPE;
  return (int64_t)dpl_layout(N, K, C).total;
}

extern "C" int64_t mlgnn_diffpool_large_saved_bytes(int64_t N, int64_t K, int64_t C) {
  if (!dpl_supported(N, K, C)) return MLGNN_E_SHAPE;
  return (int64_t)dpl_layout(N, K, C).scratch;
}

// Forward: FIVE launches for a whole batch of B pooled graphs of one shape (grid.y = graph) -- prologue (softmax + S^T,
// Z^T, ||A||^2), T = A S~, [A' | G | X'] split along K, its reduce, the scalars (ONE Frobenius norm over the batch and
// the mean entropy over all its nodes, as the reference computes them on a batched call).
// z [B,N,C], s_logits / s_out [B,N,K], adj [B,N,N] (adj_batched) or [N,N] shared by the batch, x_out [B,K,C],
// adj_out [B,K,K]; workspace: B consecutive blocks of mlgnn_diffpool_large_workspace_bytes(N, K, C) bytes.
extern "C" int mlgnn_diffpool_large_fwd(const void* z, const void* adj, const void* s_logits, int logits_dtype,
                                        void* s_out, void* x_out, void* adj_out, void* scal_out, int out_dtype,
                                        float* stats, void* workspace, int64_t workspace_bytes, int64_t N, int64_t K, int64_t C,
                                        int64_t B, int adj_batched, void* stream) {
  if (!dpl_supported(N, K, C) || B < 1 || B > 65535) return MLGNN_E_SHAPE;
  if (!z || !adj || !s_logits || !s_out || !x_out || !adj_out || !scal_out || !stats || !workspace) return MLGNN_E_NULL;
  if ((logits_dtype != MLGNN_DTYPE_F32 && logits_dtype != MLGNN_DTYPE_BF16) ||
      (out_dtype != MLGNN_DTYPE_F32 && out_dtype != MLGNN_DTYPE_BF16)) return MLGNN_E_DTYPE;
  const DplLayout L = dpl_layout(N, K, C);
  if (workspace_bytes < (int64_t)L.total * B) return MLGNN_E_WORKSPACE;
  if (!aligned(z, adj, s_out, workspace, s_logits)) return MLGNN_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  const int64_t WS = (int64_t)L.total;                // bytes between the per-graph workspaces (a multiple of 256)
  const int batch = (int)B, adj_batch = adj_batched ? (int)B : 1;
  uint16_t* stack = (uint16_t*)(ws + L.stack);
  uint16_t* Tt = stack;                               // [K,N]
  uint16_t* St = stack + (size_t)K * N;               // [K,N]
  uint16_t* Zt = stack + (size_t)2 * K * N;           // [C,N]
  uint16_t* T = (uint16_t*)(ws + L.T);
  uint16_t* G = (uint16_t*)(ws + L.G);
  float* slab = (float*)(ws + L.slab);
  float* p_a2 = (float*)(ws + L.part_a2);
  float* p_dot = (float*)(ws + L.part_dot);
  float* p_g2 = (float*)(ws + L.part_g2);
  float* p_ent = (float*)(ws + L.part_ent);
  uint16_t* S = (uint16_t*)s_out;
  const int n = (int)N, k = (int)K, c = (int)C;

  // 1. S~ = softmax(logits) as S and S^T, entropy partials; Z^T; ||A||_F^2 partials
  DplProArgs pro;
  pro.logits = s_logits; pro.S = S; pro.St = St; pro.ent_partial = p_ent;
  pro.z = (const uint16_t*)z; pro.Zt = Zt;
  pro.adj = (const uint4*)adj; pro.adj_n8 = (int64_t)N * N / 8; pro.a2_partial = p_a2;
  pro.N = n; pro.K = k; pro.C = c;
  pro.nb_sm = n / kProRows; pro.nb_zt = ((n / 64) * (c / 64) + 3) / 4; pro.nb_sq = kDplSqBlocks;
  pro.s_rowsK = N * K; pro.s_z = N * C; pro.s_adj8 = adj_batched ? N * N / 8 : 0; pro.ws_stride = WS; pro.adj_batch = adj_batch;
  const dim3 pro_grid(pro.nb_sm + pro.nb_zt + pro.nb_sq, batch);
  {
    const bool f32 = logits_dtype == MLGNN_DTYPE_F32;
    const dim3 blk(kProThreads);
#define DPL_PRO(CH)                                                                                   \
  do {                                                                                                \
    if (f32) hipLaunchKernelGGL((dpl_prologue_kernel<float, CH>), pro_grid, blk, 0, st, pro);        \
    else hipLaunchKernelGGL((dpl_prologue_kernel<bf16_t, CH>), pro_grid, blk, 0, st, pro);           \
  } while (0)
    if (k == 512) DPL_PRO(1);
    else if (k == 1024) DPL_PRO(2);
    else if (k == 2048) DPL_PRO(4);
    else DPL_PRO(0);
#undef DPL_PRO
  }
  // 2. T = A S~ (and T^T, <S~, T>)
  {
    GemmDesc d{};
    d.nseg = 1;
    d.seg[0] = GemmSeg{(const uint16_t*)adj, St, N, N, n, adj_batched ? N * N : 0, WS / 2};
    d.M = n; d.N = k; d.splits = 1;
    d.c = T; d.ldc = K; d.c_f32 = 0;
    d.ct = Tt; d.ldct = N;
    d.dot = S; d.lddot = K; d.dot_partial = p_dot;
    d.batch = batch; d.s_c = WS / 2; d.s_ct = WS / 2; d.s_dot = N * K; d.s_part = WS / 4;
    DPL_CHECK(gemm_nt_launch(d, st));
  }
  // 3. [A' | G | X'] = S~^T [T | S~ | Z]: one product over the whole stack (T^T, S~^T, Z^T are its rows), one reduce
  {
    GemmDesc d{};
    d.nseg = 1;
    d.seg[0] = GemmSeg{St, Tt, N, N, n, WS / 2, WS / 2};
    d.M = k; d.N = 2 * k + c; d.splits = L.splits_ag; d.slab = slab;
    d.batch = batch; d.s_slab = WS / 4;
    DPL_CHECK(gemm_nt_launch(d, st));
    SlabReduceArgs r{};
    r.slab = slab; r.splits = L.splits_ag; r.M = k; r.N = 2 * k + c; r.n_a = k; r.n_b = 2 * k;
    r.ca = adj_out; r.lda = K; r.ca_f32 = out_dtype == MLGNN_DTYPE_F32;
    r.cb = G; r.ldb = K; r.sq_partial = p_g2;
    r.cc = x_out; r.ldc = C; r.cc_f32 = out_dtype == MLGNN_DTYPE_F32;
    r.s_ca = K * K; r.s_cc = K * C; r.ws_stride = WS;
    slab_reduce_launch(r, batch, st);
  }
  // 4. link / entropy from the partial sums of the whole batch; numel(adj) is the ARGUMENT's element count
  DplFinalArgs f{p_a2, kDplSqBlocks, p_dot, (int)((N / kGemmTile) * (K / kGemmTile)), p_g2, kReducePartials, p_ent, pro.nb_sm,
                 stats, scal_out, out_dtype == MLGNN_DTYPE_F32, (float)(1.0 / ((double)adj_batch * (double)N * (double)N)),
                 (float)(1.0 / ((double)B * (double)N)), batch, adj_batch, WS / 4};
  dpl_final_launch(f, st);
  return (int)hipGetLastError();
}

extern "C" int64_t mlgnn_diffpool_large_bwd_workspace_bytes(int64_t N, int64_t K, int64_t C, int adj_symmetric) {
  if (!dpl_supported(N, K, C)) return MLGNN_E_SHAPE;
  size_t o = 0;
  o += align256(16);                                           // coef
  o += 3 * align256((size_t)K * K * 2);                        // b1, b2, b3
  o += 2 * align256((size_t)K * C * 2);                        // gx bf16, its transpose
  o += align256((size_t)N * K * 4);                            // dS fp32
  if (!adj_symmetric) o += align256((size_t)N * N * 2) + align256((size_t)N * K * 2);   // A^T, T2
  o += align256((size_t)N * K * 2);                            // P = S~ (dA' - cI) of the adjacency gradient
  return (int64_t)o;
}

// Backward: FOUR launches for the whole batch when adj is promised symmetric (operand preparation, the four-term dS
// product, softmax backward, dZ), one more product (T2 = A^T S~) otherwise, two more for the adjacency gradient.
// grad_x [B,K,C], grad_adj_out [B,K,K], grad_z [B,N,C], grad_logits [B,N,K], grad_adj [B,N,N] or NULL (one [N,N] block per
// graph also for a shared adjacency: the caller sums them); saved / workspace: B consecutive per-graph blocks.
extern "C" int mlgnn_diffpool_large_bwd(const void* z, const void* adj, const void* s_logits, int logits_dtype,
                                        const void* s_soft, const void* saved, const void* grad_x,
                                        const void* grad_adj_out, int grad_dtype, const void* grad_link,
                                        const void* grad_ent, int scalar_dtype, const float* stats, void* grad_z,
                                        void* grad_logits, void* grad_adj, int adj_symmetric, void* workspace,
                                        int64_t workspace_bytes, int64_t N, int64_t K, int64_t C, int64_t B, int adj_batched,
                                        void* stream) {
  if (!dpl_supported(N, K, C) || B < 1 || B > 65535) return MLGNN_E_SHAPE;
  if (!z || !adj || !s_logits || !s_soft || !saved || !grad_x || !grad_adj_out || !grad_link || !grad_ent || !stats ||
      !grad_z || !grad_logits || !workspace) return MLGNN_E_NULL;
  if (scalar_dtype != MLGNN_DTYPE_F32 && scalar_dtype != MLGNN_DTYPE_BF16) return MLGNN_E_DTYPE;
  if ((logits_dtype != MLGNN_DTYPE_F32 && logits_dtype != MLGNN_DTYPE_BF16) ||
      (grad_dtype != MLGNN_DTYPE_F32 && grad_dtype != MLGNN_DTYPE_BF16)) return MLGNN_E_DTYPE;
  const int64_t W = mlgnn_diffpool_large_bwd_workspace_bytes(N, K, C, adj_symmetric);
  if (workspace_bytes < W * B) return MLGNN_E_WORKSPACE;
  if (!aligned(s_logits, grad_logits, workspace, adj, grad_x, grad_adj_out, grad_z)) return MLGNN_E_ALIGN;
  const DplLayout L = dpl_layout(N, K, C);
  const int64_t WS = (int64_t)L.total;
  const int batch = (int)B;
  const int64_t s_adj = adj_batched ? N * N : 0;
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* sv = (const unsigned char*)saved;
  const uint16_t* stack = (const uint16_t*)(sv + L.stack);
  const uint16_t* St = stack + (size_t)K * N;
  const uint16_t* T = (const uint16_t*)(sv + L.T);
  const uint16_t* G = (const uint16_t*)(sv + L.G);
  const uint16_t* S = (const uint16_t*)s_soft;
  const int n = (int)N, k = (int)K, c = (int)C;
  unsigned char* ws = (unsigned char*)workspace;
  size_t o = 0;
  auto take = [&](size_t bytes) { unsigned char* p = ws + o; o += align256(bytes); return p; };
  float* coef = (float*)take(16);                     // (the first graph's block; one pair of coefficients for the batch)
  uint16_t* b1 = (uint16_t*)take((size_t)K * K * 2);
  uint16_t* b2 = (uint16_t*)take((size_t)K * K * 2);
  uint16_t* b3 = (uint16_t*)take((size_t)K * K * 2);
  uint16_t* gxb = (uint16_t*)take((size_t)K * C * 2);
  uint16_t* gxt = (uint16_t*)take((size_t)K * C * 2);
  float* dS = (float*)take((size_t)N * K * 4);
  uint16_t* At = nullptr;
  uint16_t* t2 = nullptr;
  if (!adj_symmetric) {
    At = (uint16_t*)take((size_t)N * N * 2);
    t2 = (uint16_t*)take((size_t)N * K * 2);
  }
  const int adj_batch = adj_batched ? batch : 1;
  // 1. operands derived from the incoming gradients (+ A^T)
  {
    DplPrepArgs q;
    q.g_link = grad_link; q.g_ent = grad_ent; q.scal_f32 = scalar_dtype == MLGNN_DTYPE_F32; q.stats = stats; q.coef = coef;
    q.inv_numel = (float)(1.0 / ((double)adj_batch * (double)N * (double)N)); q.inv_rows = (float)(1.0 / ((double)B * (double)N));
    q.ga = grad_adj_out; q.gx = grad_x; q.g_f32 = grad_dtype == MLGNN_DTYPE_F32; q.G = G;
    q.b1 = b1; q.b2 = b2; q.b3 = b3; q.gxb = gxb; q.gxt = gxt;
    q.adj = (const uint16_t*)adj; q.At = At;
    q.N = n; q.K = k; q.C = c;
    q.nb_ga = (k / 64) * (k / 64); q.nb_gx = (k / 64) * (c / 64); q.nb_at = At ? (n / 64) * (n / 64) : 0;
    q.fws_stride = WS; q.bws_stride = W; q.s_adj = s_adj;
    hipLaunchKernelGGL(dpl_prep_kernel, dim3(q.nb_ga + q.nb_gx + q.nb_at, batch), dim3(256), 0, st, q);
  }
  const uint16_t* T2 = T;
  int64_t s_T2 = WS / 2;
  if (!adj_symmetric) {
    GemmDesc d{};
    d.nseg = 1;
    d.seg[0] = GemmSeg{At, St, N, N, n, W / 2, WS / 2};
    d.M = n; d.N = k; d.splits = 1;
    d.c = t2; d.ldc = K; d.c_f32 = 0;
    d.batch = batch; d.s_c = W / 2;
    DPL_CHECK(gemm_nt_launch(d, st));
    T2 = t2; s_T2 = W / 2;
  }
  // dS = Z gx^T + T (ga - cI)^T + T2 (ga^T - cI)^T + S~ (2cG)^T    (one product over the concatenated contraction range)
  {
    GemmDesc d{};
    d.nseg = 4;
    d.seg[0] = GemmSeg{(const uint16_t*)z, gxb, C, C, c, N * C, W / 2};
    d.seg[1] = GemmSeg{T, b1, K, K, k, WS / 2, W / 2};
    d.seg[2] = GemmSeg{T2, b2, K, K, k, s_T2, W / 2};
    d.seg[3] = GemmSeg{S, b3, K, K, k, N * K, W / 2};
    d.M = n; d.N = k; d.splits = 1;
    d.c = dS; d.ldc = K; d.c_f32 = 1;
    d.batch = batch; d.s_c = W / 4;
    DPL_CHECK(gemm_nt_launch(d, st));
  }
  if (logits_dtype == MLGNN_DTYPE_F32)
    dpl_softmax_bwd_launch(static_cast<const float*>(s_logits), dS, coef, static_cast<float*>(grad_logits), n, k, W / 4, batch, st);
  else
    dpl_softmax_bwd_launch(static_cast<const bf16_t*>(s_logits), dS, coef, static_cast<bf16_t*>(grad_logits), n, k, W / 4, batch, st);
  // dZ = S~ gx, written in the dtype of z (= the dtype of the logits).  One workgroup per output tile: at
  // 4096 x 256 x 1024 that is 64 workgroups for 16 K-steps -- a split along K with its slabs and reduce launch
  // (round 2) took longer than the quarter-filled chip does.
  {
    GemmDesc d{};
    d.nseg = 1;
    d.seg[0] = GemmSeg{S, gxt, K, K, k, N * K, W / 2};
    d.M = n; d.N = c; d.splits = 1;
    d.c = grad_z; d.ldc = C; d.c_f32 = logits_dtype == MLGNN_DTYPE_F32;
    d.batch = batch; d.s_c = N * C;
    DPL_CHECK(gemm_nt_launch(d, st));
  }
  // dA = S~ dA' S~^T  (through A' = S^T A S)  +  c (A - S~ S~^T)  (through the link term)
  //    = P S~^T + c A,   P = S~ (dA' - cI)   -- two products, the second with the `+ c A` in its epilogue (c read on
  // the device).  The adjacency of the next pooling level is this level's A' (models/diff_pooling.py:116-127).
  if (grad_adj) {
    uint16_t* P = (uint16_t*)take((size_t)N * K * 2);
    GemmDesc d{};
    d.nseg = 1;
    d.seg[0] = GemmSeg{S, b2, K, K, k, N * K, W / 2};         // S~ [N,K] x (dA'^T - cI)[K,K]^T = S~ (dA' - cI)
    d.M = n; d.N = k; d.splits = 1;
    d.c = P; d.ldc = K; d.c_f32 = 0;
    d.batch = batch; d.s_c = W / 2;
    DPL_CHECK(gemm_nt_launch(d, st));
    GemmDesc e{};
    e.nseg = 1;
    e.seg[0] = GemmSeg{P, S, K, K, k, W / 2, N * K};          // P [N,K] x S~[N,K]^T
    e.M = n; e.N = n; e.splits = 1;
    e.c = grad_adj; e.ldc = N; e.c_f32 = logits_dtype == MLGNN_DTYPE_F32;
    e.aux = adj; e.ldaux = N; e.aux_f32 = 0; e.alpha = 0.f; e.alpha_dev = coef;
    e.batch = batch; e.s_c = N * N; e.s_aux = s_adj;
    DPL_CHECK(gemm_nt_launch(e, st));
  }
  return (int)hipGetLastError();
}
