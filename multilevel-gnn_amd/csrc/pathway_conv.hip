// PathwayConv's message + aggregation (the reference's models/gcn_lib/sparse/torch_vertex.py:107-178 over
// torch_message.py:88-165) for the `max` and `softmax` aggregators: fp32, atomic-free, every sum in a fixed order
// (bitwise reproducible), no per-edge tensor in memory.
//
//   msg_e[c] = a_e0 * Y0[j, c] + a_e1 * Y1[j, c]  (+ b[c])      edge j -> i, Y = [Y0 | Y1] = x [W[:, 0::2] | W[:, 1::2]]^T
//   max:      m[i, c] = max_e msg_e[c], the first maximal edge of the by-destination order wins
//   softmax:  m[i, c] = sum_e w_e msg_e[c],  w = softmax_e(t msg_e[c])
//
// The bias shifts every message of a (row, channel) alike: it is added once per row, after the aggregation.
//
// Forward: ONE workgroup (four waves) per destination row of the compact list rows[R] -- the membership rows hold tens
// to hundreds of edges.  The 256 lanes are G = 256 / LPR groups of LPR lanes; a group streams the two d-wide halves of
// one source row per step with VEC floats per lane (16-byte loads when d % 4 == 0, else one float per lane) and takes the
// edges beg + g, beg + g + G, ...; the aggregator states (maximum + position; running maximum, sum, weighted sum) stay
// in registers.  The G partial states meet in LDS and are combined in group order by the lanes of group 0.
//
// Backward: by SOURCE row over the transposed CSR, one lane group per row (the rows are short: a gene belongs to a few
// pathways).  The row's own Y[j] is all the messages need, so they are recomputed; the per-(row, channel) quantities of
// the destination (winner position / log-sum, output, cotangent) are gathered from the compact [R, d] arrays through
// row_of[N].  Every row of grad_Y is written.
//
// Algorithmic bytes, forward: E*2d*4 (Y rows) + E*12 (col, attributes) + R*d*8 (+4: rows, rowptr).  Backward:
// E*d*8 .. E*d*16 (cotangent + winner / log-sum (+ output) rows) + E*20 + N*2d*8 (Y read, grad_Y written).
#include "common.h"
#include "launch.h"
#include "mlgnn.h"

namespace mlgnn {
namespace {

constexpr int kPwUnroll = 4;               // source rows in flight per lane group (forward)
constexpr float kPwNegBig = -3.0e38f;
constexpr int kPwMaxBlocks = 1 << 16;      // most workgroups of the forward (rows are dealt round-robin past that)
constexpr int kPwColsumBlocks = 256;

struct PwShape {
  int N, R, d;
  int lpr_log2;      // lanes per row (log2): 256 >= LPR >= ceil(d / VEC)
};

__device__ __forceinline__ float pw_msg(float a0, float a1, float y0, float y1) { return fmaf(a0, y0, a1 * y1); }

struct PwFwdArgs {
  const float* Y; const int* rowptr; const int* col; const float* attr; const int* rows; const float* bias;
  float* out; int* winner; float* lse; float t; const float* t_ptr;
};

template <int VEC, int AGGR>
__global__ __launch_bounds__(kBlock) void pathway_fwd_kernel(const PwFwdArgs a, const PwShape s) {
  // partial states of the lane groups: [3][256 lanes][VEC]
  __shared__ float part[3 * kBlock * VEC];
  const int lpr = 1 << s.lpr_log2, groups = kBlock >> s.lpr_log2;
  const int g = threadIdx.x >> s.lpr_log2, u = threadIdx.x & (lpr - 1);
  const bool act = u * VEC < s.d;
  const int c0 = act ? u * VEC : 0;                      // (idle lanes re-read the first chunk and write nothing)
  const size_t row_floats = (size_t)2 * s.d;
  const float t2 = (a.t_ptr ? *a.t_ptr : a.t) * kLog2e;
  float b[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) b[i] = 0.f;
  if (a.bias) load_vec<VEC>(b, a.bias + c0);

  for (int r = blockIdx.x; r < s.R; r += gridDim.x) {
    const int row = a.rows[r];
    const int beg = a.rowptr[row], end = a.rowptr[row + 1];
    float best[VEC], sum[VEC], acc[VEC];                 // max: best = maximum; softmax: best = running maximum (log2 units)
    int pos[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) { best[i] = kPwNegBig; sum[i] = 0.f; acc[i] = 0.f; pos[i] = -1; }

    for (int e0 = beg + g; e0 < end; e0 += groups * kPwUnroll) {
      float m[kPwUnroll][VEC];
      bool valid[kPwUnroll];
#pragma unroll
      for (int k = 0; k < kPwUnroll; ++k) {
        const int e = e0 + k * groups;
        valid[k] = e < end;
#pragma unroll
        for (int i = 0; i < VEC; ++i) m[k][i] = kPwNegBig;
        if (valid[k]) {
          const int j = a.col[e];
          const float2 at = *reinterpret_cast<const float2*>(a.attr + (size_t)e * 2);
          float y0[VEC], y1[VEC];
          load_vec<VEC>(y0, a.Y + (size_t)j * row_floats + c0);
          load_vec<VEC>(y1, a.Y + (size_t)j * row_floats + s.d + c0);
#pragma unroll
          for (int i = 0; i < VEC; ++i) m[k][i] = pw_msg(at.x, at.y, y0[i], y1[i]);
        }
      }
      if constexpr (AGGR == MLGNN_AGGR_MAX) {
#pragma unroll
        for (int k = 0; k < kPwUnroll; ++k) {
          if (!valid[k]) continue;
#pragma unroll
          for (int i = 0; i < VEC; ++i)
            if (m[k][i] > best[i]) { best[i] = m[k][i]; pos[i] = e0 + k * groups; }      // strict: the first edge keeps a tie
        }
      } else {
        // online softmax, one rescale per batch
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          float nm = best[i];
#pragma unroll
          for (int k = 0; k < kPwUnroll; ++k)
            if (valid[k]) nm = fmaxf(nm, t2 * m[k][i]);
          const float rs = fast_exp2(best[i] - nm);
          float sm = sum[i] * rs, ac = acc[i] * rs;
#pragma unroll
          for (int k = 0; k < kPwUnroll; ++k) {
            if (!valid[k]) continue;
            const float p = fast_exp2(t2 * m[k][i] - nm);
            sm += p;
            ac = fmaf(p, m[k][i], ac);
          }
          best[i] = nm; sum[i] = sm; acc[i] = ac;
        }
      }
    }

    // the lane groups' partial states, combined in group order
    float* p0 = part;
    float* p1 = part + kBlock * VEC;
    float* p2 = part + 2 * kBlock * VEC;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const int at = threadIdx.x * VEC + i;
      p0[at] = best[i];
      if constexpr (AGGR == MLGNN_AGGR_MAX) {
        p1[at] = __int_as_float(pos[i]);
      } else {
        p1[at] = sum[i];
        p2[at] = acc[i];
      }
    }
    __syncthreads();
    if (g == 0 && act) {
      float o[VEC];
      if constexpr (AGGR == MLGNN_AGGR_MAX) {
        int w[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          float v = best[i];
          int p = pos[i];
          for (int k = 1; k < groups; ++k) {
            const int at = (k * lpr + u) * VEC + i;
            const float vk = p0[at];
            const int pk = __float_as_int(p1[at]);
            if (pk >= 0 && (p < 0 || vk > v || (vk == v && pk < p))) { v = vk; p = pk; }
          }
          o[i] = v + b[i];
          w[i] = p;
        }
        store_vec<VEC>(a.winner + (size_t)r * s.d + c0, w);
      } else {
        float l[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          float mx = best[i], sm = sum[i], ac = acc[i];
          for (int k = 1; k < groups; ++k) {
            const int at = (k * lpr + u) * VEC + i;
            const float mk = p0[at];
            const float nm = fmaxf(mx, mk);
            const float sa = fast_exp2(mx - nm), sb = fast_exp2(mk - nm);
            sm = sm * sa + p1[at] * sb;
            ac = ac * sa + p2[at] * sb;
            mx = nm;
          }
          o[i] = (sm > 0.f ? ac / sm : 0.f) + b[i];
          l[i] = sm > 0.f ? mx + fast_log2(sm) : 0.f;
        }
        store_vec<VEC>(a.lse + (size_t)r * s.d + c0, l);
      }
      store_vec<VEC>(a.out + (size_t)r * s.d + c0, o);
    }
    __syncthreads();
  }
}

struct PwBwdArgs {
  const float* go; const float* Y; const float* out; const float* bias; const int* winner; const float* lse;
  const int* rowptr_t; const int* col_t; const int* pos_t; const float* attr_t; const int* row_of;
  float* gY; float* ws_t; float t; const float* t_ptr;
};

template <int VEC, int AGGR, bool LEARN_T>
__global__ __launch_bounds__(kBlock) void pathway_bwd_kernel(const PwBwdArgs a, const PwShape s) {
  __shared__ float red[kWavesPerBlock];
  const int lpr = 1 << s.lpr_log2, groups = kBlock >> s.lpr_log2;
  const int g = threadIdx.x >> s.lpr_log2, u = threadIdx.x & (lpr - 1);
  const bool act = u * VEC < s.d;
  const int c0 = act ? u * VEC : 0;
  const size_t row_floats = (size_t)2 * s.d;
  const float t = a.t_ptr ? *a.t_ptr : a.t;
  const float t2 = t * kLog2e;
  const int64_t j = (int64_t)blockIdx.x * groups + g;
  float gt = 0.f;
  if (j < s.N) {
    float y0[VEC], y1[VEC], g0[VEC], g1[VEC], b[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) { y0[i] = 0.f; y1[i] = 0.f; g0[i] = 0.f; g1[i] = 0.f; b[i] = 0.f; }
    const int beg = a.rowptr_t[j], end = a.rowptr_t[j + 1];
    if (AGGR == MLGNN_AGGR_SOFTMAX && beg < end) {
      load_vec<VEC>(y0, a.Y + (size_t)j * row_floats + c0);
      load_vec<VEC>(y1, a.Y + (size_t)j * row_floats + s.d + c0);
      if (LEARN_T && a.bias) load_vec<VEC>(b, a.bias + c0);
    }
    for (int e = beg; e < end; ++e) {
      const int r = a.row_of[a.col_t[e]];
      if (r < 0) continue;                                  // (never: a destination with an edge is in rows[])
      const float2 at = *reinterpret_cast<const float2*>(a.attr_t + (size_t)e * 2);
      const size_t o = (size_t)r * s.d + c0;
      float gv[VEC], gm[VEC];
      load_vec<VEC>(gv, a.go + o);
      if constexpr (AGGR == MLGNN_AGGR_MAX) {
        const int p = a.pos_t[e];
        int w[VEC];
        load_vec<VEC>(w, a.winner + o);
#pragma unroll
        for (int i = 0; i < VEC; ++i) gm[i] = w[i] == p ? gv[i] : 0.f;
      } else {
        float l[VEC], ov[VEC];
        load_vec<VEC>(l, a.lse + o);
        if constexpr (LEARN_T) load_vec<VEC>(ov, a.out + o);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float m = pw_msg(at.x, at.y, y0[i], y1[i]);
          const float w = fast_exp2(t2 * m - l[i]);
          if constexpr (LEARN_T) {
            const float dm = m - (ov[i] - b[i]);
            gm[i] = w * fmaf(t, dm, 1.0f) * gv[i];
            gt = fmaf(gv[i] * w, m * dm, gt);
          } else {
            gm[i] = w * gv[i];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) { g0[i] = fmaf(at.x, gm[i], g0[i]); g1[i] = fmaf(at.y, gm[i], g1[i]); }
    }
    if (act) {
      store_vec<VEC>(a.gY + (size_t)j * row_floats + c0, g0);
      store_vec<VEC>(a.gY + (size_t)j * row_floats + s.d + c0, g1);
    }
  }
  if constexpr (LEARN_T) {
    // this workgroup's share of g_t: lanes by the xor butterfly, the four waves in wave order
    gt = wave_sum(act ? gt : 0.f);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = gt;
    __syncthreads();
    if (threadIdx.x == 0) {
      float tsum = 0.f;
#pragma unroll
      for (int w = 0; w < kWavesPerBlock; ++w) tsum += red[w];
      a.ws_t[blockIdx.x] = tsum;
    }
  }
}

// column sums of the cotangent [R, d] -> ws [gridDim.x, d] (each workgroup a contiguous run of rows, in row order)
__global__ __launch_bounds__(kBlock) void pathway_colsum_kernel(const float* __restrict__ go, float* __restrict__ ws,
                                                                int R, int d) {
  const int per = (R + gridDim.x - 1) / gridDim.x;
  const int r0 = blockIdx.x * per, r1 = min(R, r0 + per);
  for (int c = threadIdx.x; c < d; c += kBlock) {
    float t = 0.f;
    for (int r = r0; r < r1; ++r) t += go[(size_t)r * d + c];
    ws[(size_t)blockIdx.x * d + c] = t;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
bool pw_shape_ok(int64_t N, int64_t E, int64_t d) {
  return N >= 0 && E >= 0 && E < ((int64_t)1 << 31) && d >= 1 && d <= 256 && N * d * 8 < ((int64_t)1 << 32);
}

int pw_vec(int64_t d) { return d % 4 == 0 ? 4 : 1; }

PwShape pw_make_shape(int64_t N, int64_t R, int64_t d) {
  PwShape s;
  s.N = (int)N; s.R = (int)R; s.d = (int)d;
  const int64_t need = (d + pw_vec(d) - 1) / pw_vec(d);
  int l = 0;
  while ((1 << l) < need) ++l;                             // need <= 256: l <= 8
  s.lpr_log2 = l;
  return s;
}

int64_t pw_pad64(int64_t floats) { return (floats + 63) / 64 * 64; }

int pw_colsum_blocks(int64_t R) {
  const int64_t b = (R + 63) / 64;
  return (int)(b < 1 ? 1 : (b > kPwColsumBlocks ? kPwColsumBlocks : b));
}

int64_t pw_bwd_blocks(const PwShape& s) {
  const int64_t groups = kBlock >> s.lpr_log2;
  return ((int64_t)s.N + groups - 1) / groups;
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_pathway_conv_supported(int64_t N, int64_t E, int64_t d) { return pw_shape_ok(N, E, d) ? 1 : 0; }

extern "C" int mlgnn_pathway_conv_fwd(const float* Y, const int32_t* rowptr, const int32_t* col, const float* attr,
                                      const int32_t* rows, const float* bias, float* out, int32_t* winner, float* lse,
                                      int64_t N, int64_t E, int64_t R, int64_t d, int aggr, float t, const float* t_ptr,
                                      void* stream) {
  if (!pw_shape_ok(N, E, d) || R < 0 || R > N) return MLGNN_E_SHAPE;
  if (aggr != MLGNN_AGGR_MAX && aggr != MLGNN_AGGR_SOFTMAX) return MLGNN_E_MODE;
  if (R == 0) return 0;
  if (!Y || !rowptr || !col || !attr || !rows || !out || (aggr == MLGNN_AGGR_MAX ? !winner : !lse)) return MLGNN_E_NULL;
  if (!aligned<8>(attr) || (pw_vec(d) == 4 && !aligned(Y, bias, out, winner, lse))) return MLGNN_E_ALIGN;
  const PwShape s = pw_make_shape(N, R, d);
  const PwFwdArgs a{Y, rowptr, col, attr, rows, bias, out, winner, lse, t, t_ptr};
  const dim3 grid((unsigned)(R < kPwMaxBlocks ? R : kPwMaxBlocks)), block(kBlock);
  hipStream_t st = as_stream(stream);
  if (pw_vec(d) == 4) {
    if (aggr == MLGNN_AGGR_MAX) hipLaunchKernelGGL((pathway_fwd_kernel<4, MLGNN_AGGR_MAX>), grid, block, 0, st, a, s);
    else hipLaunchKernelGGL((pathway_fwd_kernel<4, MLGNN_AGGR_SOFTMAX>), grid, block, 0, st, a, s);
  } else {
    if (aggr == MLGNN_AGGR_MAX) hipLaunchKernelGGL((pathway_fwd_kernel<1, MLGNN_AGGR_MAX>), grid, block, 0, st, a, s);
    else hipLaunchKernelGGL((pathway_fwd_kernel<1, MLGNN_AGGR_SOFTMAX>), grid, block, 0, st, a, s);
  }
  return (int)hipGetLastError();
}

// workspace (floats): bias-gradient partials [colsum blocks, d] | g_t partials [backward workgroups] (learn_t)
extern "C" int64_t mlgnn_pathway_conv_bwd_workspace_floats(int64_t N, int64_t E, int64_t R, int64_t d, int learn_t) {
  if (!pw_shape_ok(N, E, d) || R < 0 || R > N) return MLGNN_E_SHAPE;
  const PwShape s = pw_make_shape(N, R, d);
  return pw_pad64((int64_t)pw_colsum_blocks(R) * d) + (learn_t ? pw_pad64(pw_bwd_blocks(s)) : 0);
}

extern "C" int mlgnn_pathway_conv_bwd(const float* grad_out, const float* Y, const float* out, const float* bias,
                                      const int32_t* winner, const float* lse, const int32_t* rowptr_t,
                                      const int32_t* col_t, const int32_t* pos_t, const float* attr_t,
                                      const int32_t* row_of, float* grad_Y, float* grad_bias, float* grad_t,
                                      float* workspace, int64_t workspace_floats, int64_t N, int64_t E, int64_t R,
                                      int64_t d, int aggr, float t, const float* t_ptr, int learn_t, void* stream) {
  if (!pw_shape_ok(N, E, d) || R < 0 || R > N) return MLGNN_E_SHAPE;
  if (aggr != MLGNN_AGGR_MAX && aggr != MLGNN_AGGR_SOFTMAX) return MLGNN_E_MODE;
  if (learn_t && aggr != MLGNN_AGGR_SOFTMAX) return MLGNN_E_MODE;
  if (N == 0) return 0;
  if (!grad_Y || !rowptr_t || !workspace || (learn_t && (!grad_t || !out))) return MLGNN_E_NULL;
  if (R > 0 && (!grad_out || !Y || !row_of || (aggr == MLGNN_AGGR_MAX ? !winner : !lse))) return MLGNN_E_NULL;
  if (E > 0 && (!col_t || !pos_t || !attr_t)) return MLGNN_E_NULL;
  if (workspace_floats < mlgnn_pathway_conv_bwd_workspace_floats(N, E, R, d, learn_t)) return MLGNN_E_WORKSPACE;
  if (!aligned<8>(attr_t) || (pw_vec(d) == 4 && !aligned(grad_out, Y, out, bias, winner, lse, grad_Y)))
    return MLGNN_E_ALIGN;
  const PwShape s = pw_make_shape(N, R, d);
  const int cs_blocks = pw_colsum_blocks(R);
  float* ws_b = workspace;
  float* ws_t = workspace + pw_pad64((int64_t)cs_blocks * d);
  const int64_t blocks = pw_bwd_blocks(s);
  const PwBwdArgs a{grad_out, Y, out, bias, winner, lse, rowptr_t, col_t, pos_t, attr_t, row_of, grad_Y, ws_t, t, t_ptr};
  const dim3 grid((unsigned)blocks), block(kBlock);
  hipStream_t st = as_stream(stream);
  const bool v4 = pw_vec(d) == 4;
  if (aggr == MLGNN_AGGR_MAX) {
    if (v4) hipLaunchKernelGGL((pathway_bwd_kernel<4, MLGNN_AGGR_MAX, false>), grid, block, 0, st, a, s);
    else hipLaunchKernelGGL((pathway_bwd_kernel<1, MLGNN_AGGR_MAX, false>), grid, block, 0, st, a, s);
  } else if (learn_t) {
    if (v4) hipLaunchKernelGGL((pathway_bwd_kernel<4, MLGNN_AGGR_SOFTMAX, true>), grid, block, 0, st, a, s);
    else hipLaunchKernelGGL((pathway_bwd_kernel<1, MLGNN_AGGR_SOFTMAX, true>), grid, block, 0, st, a, s);
  } else {
    if (v4) hipLaunchKernelGGL((pathway_bwd_kernel<4, MLGNN_AGGR_SOFTMAX, false>), grid, block, 0, st, a, s);
    else hipLaunchKernelGGL((pathway_bwd_kernel<1, MLGNN_AGGR_SOFTMAX, false>), grid, block, 0, st, a, s);
  }
  int err = (int)hipGetLastError();
  if (!err && learn_t) {
    launch_reduce_partials(ws_t, grad_t, (int)blocks, 1, st);
    err = (int)hipGetLastError();
  }
  if (!err && grad_bias) {
    hipLaunchKernelGGL(pathway_colsum_kernel, dim3(cs_blocks), block, 0, st, grad_out, ws_b, (int)R, (int)d);
    launch_reduce_partials(ws_b, grad_bias, cs_blocks, (int)d, st);
    err = (int)hipGetLastError();
  }
  return err;
}
