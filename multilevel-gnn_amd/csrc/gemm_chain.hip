// Kernels shared by the chains of big bf16 products (csrc/gemm_chain.h): the split-K reduce and the fp32 -> hi / lo
// bf16 split.  No atomics; every reduction is a fixed-order sum of per-workgroup partials.
#include "common.h"
#include "gemm_chain.h"

namespace mlgnn {

__global__ __launch_bounds__(256) void slab_reduce_kernel(const SlabReduceArgs p_in) {
  SlabReduceArgs p = p_in;
  {
    const int64_t bz = blockIdx.y;
    p.slab += bz * (p.ws_stride / 4);
    p.cb = reinterpret_cast<uint16_t*>(reinterpret_cast<unsigned char*>(p.cb) + bz * p.ws_stride);
    p.sq_partial += bz * (p.ws_stride / 4);
    p.ca = p.ca_f32 ? (void*)(static_cast<float*>(p.ca) + bz * p.s_ca) : (void*)(static_cast<uint16_t*>(p.ca) + bz * p.s_ca);
    p.cc = p.cc_f32 ? (void*)(static_cast<float*>(p.cc) + bz * p.s_cc) : (void*)(static_cast<uint16_t*>(p.cc) + bz * p.s_cc);
  }
  __shared__ float wsum[4];
  const int per_row = p.N / 4;
  const int64_t total = (int64_t)p.M * per_row;
  float sq = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(i / per_row), col = (int)(i % per_row) * 4;
    float4 s = reinterpret_cast<const float4*>(p.slab)[i];
    for (int z = 1; z < p.splits; ++z) {
      const float4 v = reinterpret_cast<const float4*>(p.slab + (size_t)z * p.M * p.N)[i];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (col < p.n_a || col >= p.n_b) {
      const bool first = col < p.n_a;
      void* dst = first ? p.ca : p.cc;
      const size_t at = first ? (size_t)row * p.lda + col : (size_t)row * p.ldc + (col - p.n_b);
      if (first ? p.ca_f32 : p.cc_f32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(dst) + at) = s;
      } else {
        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(dst) + at) = make_uint2(pack2_bf16(s.x, s.y), pack2_bf16(s.z, s.w));
      }
    } else {
      sq += s.x * s.x + s.y * s.y + s.z * s.z + s.w * s.w;
      if (p.cb_f32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.cb) + (size_t)row * p.ldb + (col - p.n_a)) = s;
      else *reinterpret_cast<uint2*>(p.cb + (size_t)row * p.ldb + (col - p.n_a)) = make_uint2(pack2_bf16(s.x, s.y), pack2_bf16(s.z, s.w));
    }
  }
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) p.sq_partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__device__ __forceinline__ void split2(float v, uint16_t& h, uint16_t& l) {
  h = f32_to_bf16(v);
  l = f32_to_bf16(v - bf16_to_f32(h));
}

__global__ __launch_bounds__(256) void dpl32_split_kernel(const SplitArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t th[64][66];
  __shared__ __attribute__((aligned(16))) uint16_t tl[64][66];
  __shared__ float wsum[4];
  __shared__ float cs_lds[16][64];
  int t = blockIdx.x, j = 0;
#pragma unroll
  for (int i = 0; i + 1 < kSplitMaxJobs; ++i)
    if (j == i && i + 1 < a.njobs && t >= a.job[i].tiles) { t -= a.job[i].tiles; j = i + 1; }
  SplitJob q;
  // (a uniform select over the by-value argument: no dynamic indexing of the kernel argument segment)
  q = a.job[0];
  if (j == 1) q = a.job[1];
  if (j == 2) q = a.job[2];
  if (j == 3) q = a.job[3];
  const int64_t bz = blockIdx.y;
  if (bz >= q.nb) return;
  const int tiles_c = q.Cc / 64, r0 = (t / tiles_c) * 64, c0 = (t % tiles_c) * 64;
  const float* src = q.src + bz * q.s_src;
  const float* dot = q.dot ? q.dot + bz * q.s_dot : nullptr;
  const int tid = threadIdx.x;
  float part = 0.f;
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
  // 64 rows x 256 B: 16 lanes per row, 16 bytes each; 256 threads = 16 rows per pass
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int r = pass * 16 + (tid >> 4), ch = tid & 15;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r0 + r < q.rows_valid) load_vec<4>(v, src + (size_t)(r0 + r) * q.ld + c0 + ch * 4);
    if (dot) {
      float d[4];
      load_vec<4>(d, dot + (size_t)(r0 + r) * q.lddot + c0 + ch * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) part += v[i] * d[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) cs[i] += v[i];
    uint16_t h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split2(v[i], h[i], l[i]);
    if (q.hi) {
      const size_t at = (size_t)(bz * q.s_out) + (size_t)(r0 + r) * q.ldo + c0 + ch * 4;
      *reinterpret_cast<uint2*>(q.hi + at) = make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
      *reinterpret_cast<uint2*>(q.lo + at) = make_uint2((uint32_t)l[0] | ((uint32_t)l[1] << 16), (uint32_t)l[2] | ((uint32_t)l[3] << 16));
    }
    if (q.hit) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        th[r][ch * 4 + i] = h[i];
        tl[r][ch * 4 + i] = l[i];
      }
    }
  }
  if (q.hit) {
    __syncthreads();
    uint16_t* oh = q.hit + bz * q.s_outt;
    uint16_t* ol = q.lot + bz * q.s_outt;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int c = pass * 32 + (tid >> 3), ch = tid & 7;                  // column of the tile = row of the transpose
      uint32_t wh[4], wl[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        wh[i] = (uint32_t)th[ch * 8 + 2 * i][c] | ((uint32_t)th[ch * 8 + 2 * i + 1][c] << 16);
        wl[i] = (uint32_t)tl[ch * 8 + 2 * i][c] | ((uint32_t)tl[ch * 8 + 2 * i + 1][c] << 16);
      }
      const size_t at = (size_t)(c0 + c) * q.ldt + r0 + ch * 8;
      *reinterpret_cast<uint4*>(oh + at) = make_uint4(wh[0], wh[1], wh[2], wh[3]);
      *reinterpret_cast<uint4*>(ol + at) = make_uint4(wl[0], wl[1], wl[2], wl[3]);
    }
  }
  if (q.colsum) {                                     // fixed order: a thread's four rows, then the 16 row lanes in order
#pragma unroll
    for (int i = 0; i < 4; ++i) cs_lds[tid >> 4][(tid & 15) * 4 + i] = cs[i];
    __syncthreads();
    if (tid < 64) {
      float acc = cs_lds[0][tid];
#pragma unroll
      for (int k = 1; k < 16; ++k) acc += cs_lds[k][tid];
      q.colsum[(size_t)(t / tiles_c) * q.Cc + c0 + tid] = acc;
    }
  }
  if (dot) {
    part = wave_sum(part);
    if ((tid & 63) == 0) wsum[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) q.partial[bz * q.s_part + t] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
  }
}

void slab_reduce_launch(const SlabReduceArgs& r, int batch, hipStream_t st) {
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(kReducePartials, batch), dim3(256), 0, st, r);
}

int split_launch(const SplitArgs& a, int batch, hipStream_t st) {
  int tiles = 0;
  for (int i = 0; i < a.njobs; ++i) tiles += a.job[i].tiles;
  hipLaunchKernelGGL(dpl32_split_kernel, dim3(tiles, batch), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace mlgnn
