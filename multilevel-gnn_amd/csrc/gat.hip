// Graph attention convolution (PyG GATConv as wrapped by the reference's models/gcn_lib/sparse/torch_vertex.py:207-223)
// as CSR edge-softmax kernels: fp32, atomic-free, every sum in a fixed order (bitwise reproducible).
//
//   z [N, H, C] = lin_src(x)                      (a separate GEMM node: mlgnn.dense.linear)
//   a_src[n,h] = <z[n,h,:], att_src[h,:]>,  a_dst likewise                        gat_scores_kernel
//   e(j->i,h)  = leaky_relu(a_src[j,h] + a_dst[i,h], negative_slope)
//   alpha      = softmax of e over the incoming edges of i (row maximum subtracted)
//   y[i,h,:]   = act(sum_j alpha z[j,h,:] + bias)                                 gat_fwd_kernel
//
// Layout (that of csr_aggregate_fwd_kernel): one wavefront owns one CSR row, its 64 lanes are G = 64 / LPR groups of
// LPR lanes, a group streams one whole neighbour row per step with VEC floats per lane (16-byte loads when C % 4 == 0);
// `col` is loaded coalesced once per 64 edges and broadcast with shuffles.  A lane holds Q "slots" of VEC consecutive
// channels (slot q = unit cl + q * LPR); VEC divides C, so a slot lies inside ONE head and the per-head quantities
// (logit, running maximum, sum) are per slot.  Instantiations: <4,1> (C % 4 == 0), <1,1> (d <= 64) and <1,4>.
//
// Reductions over the lanes of one head (the scores, D, and the backward's <g_i, z_j>): an xor butterfly when the head
// spans an aligned power-of-two run of lanes, else through a per-wave LDS strip summed in channel order.
//
// Algorithmic bytes, forward: E*d*4 (z rows) + E*4 (col) + E*H*4 (a_src; a 32..64-byte sector per edge) + N*d*4 (y)
// + 3*N*H*4 + N*4.  Backward main pass: E*d*4 (g rows) + E*H*16 (packed a_dst / lse / D) + E*8 (col_t, pos_t)
// + E*H*4 (per-edge d logit, written once) + 2*N*d*4.
#include <type_traits>
#include "common.h"
#include "launch.h"
#include "mlgnn.h"

namespace mlgnn {
namespace {

constexpr int kGatUnroll = 4;              // neighbour rows in flight per lane group
constexpr int kGatRowsPerWave = 4;         // rows per wave of the chunked row walk (as the aggregation forward)
constexpr int kGatStreamBlocks = 1024;     // most workgroups of a streaming pass (= rows of its partial sums)
constexpr float kGatNegBig = -3.0e38f;

struct GatShape {
  int N, H, C, d;
  int lpr_log2;      // lanes per row (log2)
  int upl;           // units (lanes x slots) per head = C / VEC
  int butterfly;     // heads are aligned power-of-two lane runs
  float neg_slope, act_slope;
};

template <int VEC, int Q>
struct Lay {
  int lane, lpr, groups, sub, cl;
  int c0[Q];         // first channel of slot q, clamped into the row (lanes past the row re-read its last chunk)
  int head[Q];
  bool act[Q];       // slot q holds channels of the row
  bool lead[Q];      // ... and the first channel of its head
};

template <int VEC, int Q>
__device__ __forceinline__ Lay<VEC, Q> make_lay(const GatShape& s) {
  Lay<VEC, Q> L;
  L.lane = threadIdx.x & (kWave - 1);
  L.lpr = 1 << s.lpr_log2;
  L.groups = kWave >> s.lpr_log2;
  L.sub = L.lane >> s.lpr_log2;
  L.cl = L.lane & (L.lpr - 1);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int c = (L.cl + q * L.lpr) * VEC;
    L.act[q] = c < s.d;
    L.c0[q] = min(c, s.d - VEC);
    L.head[q] = L.c0[q] / s.C;
    L.lead[q] = L.act[q] && L.c0[q] == L.head[q] * s.C;
  }
  return L;
}

// p[q] <- sum of p over the units of slot q's head (every lane of the wave calls this together).  wl: this wave's
// 64 * Q floats of LDS.  Both forms add in a fixed order.
template <int VEC, int Q>
__device__ __forceinline__ void head_sum(float (&p)[Q], const Lay<VEC, Q>& L, const GatShape& s, float* wl) {
  if (s.butterfly) {
    for (int off = 1; off < s.upl; off <<= 1) {
#pragma unroll
      for (int q = 0; q < Q; ++q) p[q] += __shfl_xor(p[q], off);
    }
    return;
  }
  const int base = L.sub * (L.lpr * Q);
#pragma unroll
  for (int q = 0; q < Q; ++q) wl[base + L.cl + q * L.lpr] = p[q];
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int b = base + L.head[q] * s.upl;
    float t = 0.f;
    for (int k = 0; k < s.upl; ++k) t += wl[b + k];
    p[q] = t;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float leaky(float x, float slope) { return x > 0.f ? x : x * slope; }

// per-lane sums [Q][VEC] over the rows a workgroup streamed -> row `blockIdx.x` of ws [gridDim.x, d]: lane groups by
// xor shuffles, the four waves through LDS in wave order
template <int VEC, int Q>
__device__ __forceinline__ void block_partial(float (&acc)[Q][VEC], const Lay<VEC, Q>& L, const GatShape& s,
                                              float* red /* [4][64 * Q * VEC] */, float* __restrict__ ws) {
  for (int off = L.lpr; off < kWave; off <<= 1) {
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[q][i] += __shfl_xor(acc[q][i], off);
  }
  constexpr int kSpan = kWave * Q * VEC;
  const int wave = threadIdx.x / kWave;
  __syncthreads();
  if (L.sub == 0) {
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (L.act[q]) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) red[wave * kSpan + L.c0[q] + i] = acc[q][i];
      }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < s.d; c += kBlock) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) t += red[w * kSpan + c];
    ws[(size_t)blockIdx.x * s.d + c] = t;
  }
}

// ---- scores: a_src / a_dst [N, H] -------------------------------------------------------------------------------
template <int VEC, int Q>
__global__ __launch_bounds__(kBlock) void gat_scores_kernel(const float* __restrict__ z, const float* __restrict__ att_src,
                                                            const float* __restrict__ att_dst, float* __restrict__ a_src,
                                                            float* __restrict__ a_dst, const GatShape s) {
  __shared__ float lds[kWavesPerBlock][kWave * Q];
  const Lay<VEC, Q> L = make_lay<VEC, Q>(s);
  const int wave = threadIdx.x / kWave;
  float as[Q][VEC], ad[Q][VEC];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    load_vec<VEC>(as[q], att_src + L.c0[q]);
    load_vec<VEC>(ad[q], att_dst + L.c0[q]);
  }
  const int step = gridDim.x * kWavesPerBlock * L.groups;
  for (int r0 = (blockIdx.x * kWavesPerBlock + wave) * L.groups; r0 < s.N; r0 += step) {
    const int r = r0 + L.sub;
    const bool ok = r < s.N;
    const int rr = ok ? r : s.N - 1;
    float ps[Q], pd[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      float zv[VEC];
      load_vec<VEC>(zv, z + (size_t)rr * s.d + L.c0[q]);
      ps[q] = 0.f; pd[q] = 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) { ps[q] = fmaf(zv[i], as[q][i], ps[q]); pd[q] = fmaf(zv[i], ad[q][i], pd[q]); }
    }
    head_sum<VEC, Q>(ps, L, s, lds[wave]);
    head_sum<VEC, Q>(pd, L, s, lds[wave]);
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (ok && L.lead[q]) {
        a_src[(size_t)r * s.H + L.head[q]] = ps[q];
        a_dst[(size_t)r * s.H + L.head[q]] = pd[q];
      }
  }
}

// ---- forward: one wavefront per destination row ----------------------------------------------------------------
struct GatFwdArgs {
  const float* z; const float* a_src; const float* a_dst; const float* bias;
  const int* rowptr; const int* col;
  float* y; float* lse; float* rowmax;
};

template <int VEC, int Q>
__global__ __launch_bounds__(kBlock) void gat_fwd_kernel(const GatFwdArgs a, const GatShape s) {
  const Lay<VEC, Q> L = make_lay<VEC, Q>(s);
  const RowWalk walk = make_chunk_walk(s.N);
  float b[Q][VEC];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) b[q][i] = 0.f;
    if (a.bias) load_vec<VEC>(b[q], a.bias + L.c0[q]);
  }
  for (int r = walk.first; r < walk.r_end; r += walk.stride) {
    const int beg = a.rowptr[r], end = a.rowptr[r + 1];
    float adst[Q], mx[Q], sum[Q], acc[Q][VEC];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      adst[q] = a.a_dst[(size_t)r * s.H + L.head[q]];
      mx[q] = kGatNegBig; sum[q] = 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[q][i] = 0.f;
    }
    for (int base = beg; base < end; base += kWave) {
      const int cnt = min(kWave, end - base);
      const int my_col = L.lane < cnt ? a.col[base + L.lane] : 0;
      for (int k = 0; k < cnt; k += L.groups * kGatUnroll) {
        float zv[kGatUnroll][Q][VEC], e[kGatUnroll][Q];
        bool valid[kGatUnroll];
#pragma unroll
        for (int u = 0; u < kGatUnroll; ++u) {
          const int idx = k + u * L.groups + L.sub;
          valid[u] = idx < cnt;
          const int j = __shfl(my_col, idx & (kWave - 1));
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            e[u][q] = kGatNegBig;
#pragma unroll
            for (int i = 0; i < VEC; ++i) zv[u][q][i] = 0.f;
            if (valid[u]) {
              load_vec<VEC>(zv[u][q], a.z + (uint32_t)j * (uint32_t)s.d + (uint32_t)L.c0[q]);
              e[u][q] = leaky(a.a_src[(uint32_t)j * (uint32_t)s.H + (uint32_t)L.head[q]] + adst[q], s.neg_slope);
            }
          }
        }
        // online softmax, one rescale per batch; the running maximum is kept (logits are unbounded)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          float nm = mx[q];
#pragma unroll
          for (int u = 0; u < kGatUnroll; ++u) nm = fmaxf(nm, e[u][q]);
          const float rs = fast_exp2((mx[q] - nm) * kLog2e);      // 0 on the first batch; 1 when nothing was seen yet
          float t = sum[q] * rs;
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[q][i] *= rs;
#pragma unroll
          for (int u = 0; u < kGatUnroll; ++u) {
            const float p = valid[u] ? fast_exp2((e[u][q] - nm) * kLog2e) : 0.f;
            t += p;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[q][i] = fmaf(p, zv[u][q][i], acc[q][i]);
          }
          sum[q] = t; mx[q] = nm;
        }
      }
    }
    // combine the lane groups; a group that saw no edge holds (kGatNegBig, 0, 0)
    for (int off = L.lpr; off < kWave; off <<= 1) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const float om = __shfl_xor(mx[q], off), os = __shfl_xor(sum[q], off);
        const float nm = fmaxf(mx[q], om);
        const float sa = fast_exp2((mx[q] - nm) * kLog2e), sb = fast_exp2((om - nm) * kLog2e);
        sum[q] = sum[q] * sa + os * sb;
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[q][i] = acc[q][i] * sa + __shfl_xor(acc[q][i], off) * sb;
        mx[q] = nm;
      }
    }
    float amax = 0.f;
    if (L.sub == 0) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (!L.act[q]) continue;
        // the reference adds 1e-16 to the sum of exp(e - max) >= 1: below fp32 resolution, kept for the record
        const float inv = sum[q] > 0.f ? 1.0f / (sum[q] + 1e-16f) : 0.f;
        float o[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          o[i] = leaky(fmaf(acc[q][i], inv, b[q][i]), s.act_slope);
          amax = fmaxf(amax, fabsf(o[i]));
        }
        store_t_stream<float, VEC>(a.y + (size_t)r * s.d + L.c0[q], o);
        if (L.lead[q]) a.lse[(size_t)r * s.H + L.head[q]] = sum[q] > 0.f ? mx[q] + fast_log2(sum[q]) * kLn2 : 0.f;
      }
    }
    if (a.rowmax) {
      amax = wave_max(amax);
      if (L.lane == 0) a.rowmax[r] = amax;
    }
  }
}

// ---- backward (a): g = dY act'(y), D[i,h] = sum_c g (pre - bias), packed row scalars, bias-gradient partials -------
struct GatPreArgs {
  const float* gy; const float* y; const float* bias; const float* a_dst; const float* lse;
  float* g; float* pack; float* ws_db;
};

template <int VEC, int Q>
__global__ __launch_bounds__(kBlock) void gat_bwd_pre_kernel(const GatPreArgs a, const GatShape s) {
  __shared__ float lds[kWavesPerBlock][kWave * Q];
  __shared__ float red[kWavesPerBlock * kWave * Q * VEC];
  const Lay<VEC, Q> L = make_lay<VEC, Q>(s);
  const int wave = threadIdx.x / kWave;
  float b[Q][VEC], db[Q][VEC];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) { b[q][i] = 0.f; db[q][i] = 0.f; }
    if (a.bias) load_vec<VEC>(b[q], a.bias + L.c0[q]);
  }
  const float inv_slope = s.act_slope != 0.f ? 1.0f / s.act_slope : 0.f;
  const int step = gridDim.x * kWavesPerBlock * L.groups;
  for (int r0 = (blockIdx.x * kWavesPerBlock + wave) * L.groups; r0 < s.N; r0 += step) {
    const int r = r0 + L.sub;
    const bool ok = r < s.N;
    const int rr = ok ? r : s.N - 1;
    float pD[Q], gv[Q][VEC];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      float go[VEC], yv[VEC];
      load_vec<VEC>(go, a.gy + (size_t)rr * s.d + L.c0[q]);
      load_vec<VEC>(yv, a.y + (size_t)rr * s.d + L.c0[q]);
      pD[q] = 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const bool pos = yv[i] > 0.f;
        gv[q][i] = pos ? go[i] : go[i] * s.act_slope;
        // (relu's flat side: the pre-activation is lost, and g = 0 there)
        const float pre = pos ? yv[i] : yv[i] * inv_slope;
        pD[q] = fmaf(gv[q][i], (pos || s.act_slope != 0.f) ? pre - b[q][i] : 0.f, pD[q]);
        db[q][i] += (ok && L.act[q]) ? gv[q][i] : 0.f;
      }
    }
    head_sum<VEC, Q>(pD, L, s, lds[wave]);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      if (!ok || !L.act[q]) continue;
      store_vec<VEC>(a.g + (size_t)r * s.d + L.c0[q], gv[q]);
      if (L.lead[q]) {
        const size_t rh = (size_t)r * s.H + L.head[q];
        *reinterpret_cast<float4*>(a.pack + rh * 4) = make_float4(a.a_dst[rh], a.lse[rh], pD[q], 0.f);
      }
    }
  }
  block_partial<VEC, Q>(db, L, s, red, a.ws_db);
}

// ---- backward (b): one wavefront per source row of the transposed CSR ------------------------------------------
struct GatBwdArgs {
  const float* z; const float* a_src; const float* g; const float* pack;
  const int* rowptr_t; const int* col_t; const int* pos_t;
  float* dz; float* da_src; float* dlogit;
};

template <int VEC, int Q>
__global__ __launch_bounds__(kBlock) void gat_bwd_kernel(const GatBwdArgs a, const GatShape s) {
  __shared__ float lds[kWavesPerBlock][kWave * Q];
  const Lay<VEC, Q> L = make_lay<VEC, Q>(s);
  const int wave = threadIdx.x / kWave;
  const RowWalk walk = make_chunk_walk(s.N);
  for (int r = walk.first; r < walk.r_end; r += walk.stride) {
    const int beg = a.rowptr_t[r], end = a.rowptr_t[r + 1];
    float zj[Q][VEC], asj[Q], dz[Q][VEC], das[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      load_vec<VEC>(zj[q], a.z + (size_t)r * s.d + L.c0[q]);
      asj[q] = a.a_src[(size_t)r * s.H + L.head[q]];
      das[q] = 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) dz[q][i] = 0.f;
    }
    for (int base = beg; base < end; base += kWave) {
      const int cnt = min(kWave, end - base);
      const int my_i = L.lane < cnt ? a.col_t[base + L.lane] : 0;
      const int my_pos = L.lane < cnt ? a.pos_t[base + L.lane] : 0;
      for (int k = 0; k < cnt; k += L.groups * kGatUnroll) {
#pragma unroll
        for (int u = 0; u < kGatUnroll; ++u) {
          if (k + u * L.groups >= cnt) break;                    // wave-uniform: no lane group has an edge left
          const int idx = k + u * L.groups + L.sub;
          const bool valid = idx < cnt;
          const int i_row = __shfl(my_i, idx & (kWave - 1));
          const int pos = __shfl(my_pos, idx & (kWave - 1));
          float gv[Q][VEC], pd[Q], alpha[Q], dsc[Q], lk[Q];
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            pd[q] = 0.f; alpha[q] = 0.f; dsc[q] = 0.f; lk[q] = 0.f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) gv[q][i] = 0.f;
            if (valid) {
              load_vec<VEC>(gv[q], a.g + (uint32_t)i_row * (uint32_t)s.d + (uint32_t)L.c0[q]);
              const float4 pk = *reinterpret_cast<const float4*>(a.pack + ((size_t)i_row * s.H + L.head[q]) * 4);
              const float raw = asj[q] + pk.x;
              alpha[q] = fast_exp2((leaky(raw, s.neg_slope) - pk.y) * kLog2e);
              dsc[q] = pk.z;
              lk[q] = raw > 0.f ? 1.0f : s.neg_slope;
#pragma unroll
              for (int i = 0; i < VEC; ++i) pd[q] = fmaf(gv[q][i], zj[q][i], pd[q]);
            }
          }
          head_sum<VEC, Q>(pd, L, s, lds[wave]);                 // d alpha = <g[i,h,:], z[j,h,:]>
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            const float dl = alpha[q] * (pd[q] - dsc[q]) * lk[q];
            das[q] += dl;
#pragma unroll
            for (int i = 0; i < VEC; ++i) dz[q][i] = fmaf(alpha[q], gv[q][i], dz[q][i]);
            if (valid && L.lead[q]) a.dlogit[(size_t)pos * s.H + L.head[q]] = dl;
          }
        }
      }
    }
    for (int off = L.lpr; off < kWave; off <<= 1) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        das[q] += __shfl_xor(das[q], off);
#pragma unroll
        for (int i = 0; i < VEC; ++i) dz[q][i] += __shfl_xor(dz[q][i], off);
      }
    }
    if (L.sub == 0) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        if (!L.act[q]) continue;
        if (a.dz) store_vec<VEC>(a.dz + (size_t)r * s.d + L.c0[q], dz[q]);
        if (L.lead[q]) a.da_src[(size_t)r * s.H + L.head[q]] = das[q];
      }
    }
  }
}

// ---- backward (c) + (d): da_dst by rowptr, the scores' chain rule into dz, attention-vector gradient partials ----
struct GatFinArgs {
  const float* z; const float* att_src; const float* att_dst; const float* da_src; const float* dlogit;
  const int* rowptr;
  float* dz; float* ws_src; float* ws_dst;
};

template <int VEC, int Q>
__global__ __launch_bounds__(kBlock) void gat_bwd_finish_kernel(const GatFinArgs a, const GatShape s) {
  __shared__ float red[kWavesPerBlock * kWave * Q * VEC];
  const Lay<VEC, Q> L = make_lay<VEC, Q>(s);
  const int wave = threadIdx.x / kWave;
  float as[Q][VEC], ad[Q][VEC], ps[Q][VEC], pd[Q][VEC];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    load_vec<VEC>(as[q], a.att_src + L.c0[q]);
    load_vec<VEC>(ad[q], a.att_dst + L.c0[q]);
#pragma unroll
    for (int i = 0; i < VEC; ++i) { ps[q][i] = 0.f; pd[q][i] = 0.f; }
  }
  const int step = gridDim.x * kWavesPerBlock * L.groups;
  for (int r0 = (blockIdx.x * kWavesPerBlock + wave) * L.groups; r0 < s.N; r0 += step) {
    const int r = r0 + L.sub;
    if (r >= s.N) continue;
    const int beg = a.rowptr[r], end = a.rowptr[r + 1];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      if (!L.act[q]) continue;
      const float das = a.da_src[(size_t)r * s.H + L.head[q]];
      float dad = 0.f;                                       // the row's edges in by-destination order
      for (int e = beg; e < end; ++e) dad += a.dlogit[(size_t)e * s.H + L.head[q]];
      float zv[VEC];
      load_vec<VEC>(zv, a.z + (size_t)r * s.d + L.c0[q]);
#pragma unroll
      for (int i = 0; i < VEC; ++i) { ps[q][i] = fmaf(das, zv[i], ps[q][i]); pd[q][i] = fmaf(dad, zv[i], pd[q][i]); }
      if (a.dz) {
        float dv[VEC];
        load_vec<VEC>(dv, a.dz + (size_t)r * s.d + L.c0[q]);
#pragma unroll
        for (int i = 0; i < VEC; ++i) dv[i] = fmaf(das, as[q][i], fmaf(dad, ad[q][i], dv[i]));
        store_vec<VEC>(a.dz + (size_t)r * s.d + L.c0[q], dv);
      }
    }
  }
  block_partial<VEC, Q>(ps, L, s, red, a.ws_src);
  block_partial<VEC, Q>(pd, L, s, red, a.ws_dst);
}

// ---- host side -------------------------------------------------------------------------------------------------
bool shape_ok(int64_t N, int64_t H, int64_t C) {
  return N >= 0 && H >= 1 && H <= 16 && C >= 1 && H * C <= 256 && N * H * C * 4 < ((int64_t)1 << 32);
}

int vec_of(int64_t C) { return C % 4 == 0 ? 4 : 1; }

GatShape make_shape(int64_t N, int64_t H, int64_t C, float neg_slope, float act_slope) {
  GatShape s;
  s.N = (int)N; s.H = (int)H; s.C = (int)C; s.d = (int)(H * C);
  const int vec = vec_of(C);
  const bool q4 = vec == 1 && s.d > kWave;
  s.lpr_log2 = q4 ? 6 : lanes_per_row_log2(s.d, vec);
  s.upl = s.C / vec;
  s.butterfly = ((s.upl & (s.upl - 1)) == 0 && s.upl <= (1 << s.lpr_log2)) ? 1 : 0;
  s.neg_slope = neg_slope; s.act_slope = act_slope;
  return s;
}

template <typename F>
void for_layout(const GatShape& s, F&& f) {
  if (s.C % 4 == 0) f(IC<4>{}, IC<1>{});
  else if (s.d <= kWave) f(IC<1>{}, IC<1>{});
  else f(IC<1>{}, IC<4>{});
}

int stream_blocks(const GatShape& s) {
  const int64_t rows_per_block = (int64_t)kWavesPerBlock * (kWave >> s.lpr_log2) * 4;
  int64_t b = (s.N + rows_per_block - 1) / rows_per_block;
  return (int)(b < 1 ? 1 : (b > kGatStreamBlocks ? kGatStreamBlocks : b));
}

int64_t pad64(int64_t floats) { return (floats + 63) / 64 * 64; }

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_gat_supported(int64_t N, int64_t H, int64_t C) { return shape_ok(N, H, C) ? 1 : 0; }

extern "C" int mlgnn_gat_scores(const float* z, const float* att_src, const float* att_dst, float* a_src, float* a_dst,
                                int64_t N, int64_t H, int64_t C, void* stream) {
  if (!shape_ok(N, H, C)) return MLGNN_E_SHAPE;
  if (N == 0) return 0;
  if (!z || !att_src || !att_dst || !a_src || !a_dst) return MLGNN_E_NULL;
  if (vec_of(C) == 4 && !aligned(z, att_src, att_dst)) return MLGNN_E_ALIGN;
  const GatShape s = make_shape(N, H, C, 0.f, 1.f);
  hipStream_t st = static_cast<hipStream_t>(stream);
  for_layout(s, [&](auto vec, auto q) {
    hipLaunchKernelGGL((gat_scores_kernel<decltype(vec)::value, decltype(q)::value>), dim3(stream_blocks(s)), dim3(kBlock),
                       0, st, z, att_src, att_dst, a_src, a_dst, s);
  });
  return (int)hipGetLastError();
}

extern "C" int mlgnn_gat_aggregate_fwd(const float* z, const float* a_src, const float* a_dst, const float* bias,
                                       const int32_t* rowptr, const int32_t* col, float* y, float* lse, float* row_max,
                                       int64_t N, int64_t E, int64_t H, int64_t C, float negative_slope, float act_slope,
                                       void* stream) {
  if (!shape_ok(N, H, C) || E < 0 || E >= ((int64_t)1 << 31) || !(act_slope >= 0.f)) return MLGNN_E_SHAPE;
  if (N == 0) return 0;
  if (!z || !a_src || !a_dst || !rowptr || !y || !lse || (E > 0 && !col)) return MLGNN_E_NULL;
  if (vec_of(C) == 4 && !aligned(z, y, bias)) return MLGNN_E_ALIGN;
  const GatShape s = make_shape(N, H, C, negative_slope, act_slope);
  const GatFwdArgs a{z, a_src, a_dst, bias, rowptr, col, y, lse, row_max};
  hipStream_t st = static_cast<hipStream_t>(stream);
  for_layout(s, [&](auto vec, auto q) {
    hipLaunchKernelGGL((gat_fwd_kernel<decltype(vec)::value, decltype(q)::value>), dim3(grid_for_chunks(N, kGatRowsPerWave)),
                       dim3(kBlock), 0, st, a, s);
  });
  return (int)hipGetLastError();
}

// workspace (floats): g [N,d] | packed (a_dst, lse, D, 0) [N,H,4] | da_src [N,H] | d logit [E,H] | 3 x partials [blocks, d]
extern "C" int64_t mlgnn_gat_bwd_workspace_floats(int64_t N, int64_t E, int64_t H, int64_t C) {
  if (!shape_ok(N, H, C) || E < 0 || E >= ((int64_t)1 << 31)) return MLGNN_E_SHAPE;
  const GatShape s = make_shape(N, H, C, 0.f, 1.f);
  return pad64(N * H * C) + pad64(N * H * 4) + pad64(N * H) + pad64(E * H) + 3 * pad64((int64_t)stream_blocks(s) * H * C);
}

extern "C" int mlgnn_gat_aggregate_bwd(const float* grad_y, const float* y, const float* z, const float* a_src,
                                       const float* a_dst, const float* lse, const float* att_src, const float* att_dst,
                                       const float* bias, const int32_t* rowptr, const int32_t* rowptr_t,
                                       const int32_t* col_t, const int32_t* pos_t, float* grad_z, float* grad_att_src,
                                       float* grad_att_dst, float* grad_bias, float* workspace, int64_t workspace_floats,
                                       int64_t N, int64_t E, int64_t H, int64_t C, float negative_slope, float act_slope,
                                       void* stream) {
  if (!shape_ok(N, H, C) || E < 0 || E >= ((int64_t)1 << 31) || !(act_slope >= 0.f)) return MLGNN_E_SHAPE;
  if (N == 0) return 0;
  if (!grad_y || !y || !z || !a_src || !a_dst || !lse || !att_src || !att_dst || !rowptr || !rowptr_t || !workspace ||
      (E > 0 && (!col_t || !pos_t)) || (!grad_att_src) != (!grad_att_dst))
    return MLGNN_E_NULL;
  if (workspace_floats < mlgnn_gat_bwd_workspace_floats(N, E, H, C)) return MLGNN_E_WORKSPACE;
  if (!aligned(workspace)) return MLGNN_E_ALIGN;
  if (vec_of(C) == 4 && !aligned(grad_y, y, z, att_src, att_dst, bias, grad_z))
    return MLGNN_E_ALIGN;
  const GatShape s = make_shape(N, H, C, negative_slope, act_slope);
  const int d = s.d, blocks = stream_blocks(s);
  float* g = workspace;
  float* pack = g + pad64(N * d);
  float* da_src = pack + pad64(N * H * 4);
  float* dlogit = da_src + pad64(N * H);
  float* ws_db = dlogit + pad64(E * H);
  float* ws_src = ws_db + pad64((int64_t)blocks * d);
  float* ws_dst = ws_src + pad64((int64_t)blocks * d);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool edges = grad_z || grad_att_src;      // anything past the bias gradient
  const GatPreArgs pa{grad_y, y, bias, a_dst, lse, g, pack, ws_db};
  const GatBwdArgs ba{z, a_src, g, pack, rowptr_t, col_t, pos_t, grad_z, da_src, dlogit};
  const GatFinArgs fa{z, att_src, att_dst, da_src, dlogit, rowptr, grad_z, ws_src, ws_dst};
  for_layout(s, [&](auto vec, auto q) {
    constexpr int V = decltype(vec)::value, QQ = decltype(q)::value;
    hipLaunchKernelGGL((gat_bwd_pre_kernel<V, QQ>), dim3(blocks), dim3(kBlock), 0, st, pa, s);
    if (edges) {
      hipLaunchKernelGGL((gat_bwd_kernel<V, QQ>), dim3(grid_for_chunks(N, kGatRowsPerWave)), dim3(kBlock), 0, st, ba, s);
      hipLaunchKernelGGL((gat_bwd_finish_kernel<V, QQ>), dim3(blocks), dim3(kBlock), 0, st, fa, s);
    }
  });
  int err = (int)hipGetLastError();
  if (!err && grad_bias) launch_reduce_partials(ws_db, grad_bias, blocks, d, st);
  if (!err && grad_att_src) {
    launch_reduce_partials(ws_src, grad_att_src, blocks, d, st);
    launch_reduce_partials(ws_dst, grad_att_dst, blocks, d, st);
  }
  return err ? err : (int)hipGetLastError();
}
