// The per-pathway decoders of the pre-training models (models/vae.py: foreach_decoder) for every (pathway, omics)
// segment at once: one launch forward, one backward, one workgroup per segment.
//
//   h    [B, P, H]                      segment p decodes the B rows h[:, p, :]
//   w1   blocks [hid_p, H] row-major    block p at H * hid_off[p];  b1 at hid_off[p]
//   w2   blocks [n_p, hid_p] row-major  block p at w2_off[p];       b2 at out_off[p]
//   out  [B, N], N = out_off[P]:        out[:, out_off[p] : out_off[p + 1]] = relu(h_p W1_p^T + b1_p) W2_p^T + b2_p
//
// LDS (floats; Hp, hp = H, hid rounded up to 4 so that a row is read 16 bytes at a time; the padding is zero):
//   forward   hs [B][Hp] | hid [B][hp] | ws [64][33]
//   backward  r0 [B][max(Hp, NC)] | hid [B][hp] | dhid [B][hp]   (r0: hs, then the cotangent chunk gs [B][NC], then hs
//             again; ws lies over dhid while hid is recomputed)
// Three products, each with lanes across 64 output columns, the four waves across rows and 16 accumulators per thread:
//   nt  X W^T, W global with the reduction along its rows (hid, out): 64 x 32 tiles of W go through ws (row stride 33:
//       lanes read down a column without a bank conflict); every weight is read from global memory once
//   nn  X W, W global with the output along its rows (dhid += g W2, dh = dhid W1): lanes read W rows directly
//   tn  A^T Y, both in LDS, reduced over the batch (dW2 = g^T hid, dW1 = dhid^T h)
// Every sum runs in index order inside one thread, every output element has one owner: no atomics, bitwise
// reproducible.  The backward recomputes hid; a unit with hid == 0 gets no gradient (torch's relu backward).
#include "common.h"
#include "launch.h"
#include "mlgnn.h"

namespace mlgnn {
namespace {

constexpr int kDecRows = 16;                            // accumulators (rows) per thread
constexpr int kDecRowTile = kWavesPerBlock * kDecRows;  // 64 rows per pass
constexpr int kDecKC = 32;                              // reduction chunk of a staged weight tile
constexpr int kDecWS = kDecKC + 1;                      // its row stride
constexpr int64_t kDecTileFloats = kWave * kDecWS;      // 2112
constexpr int64_t kDecLdsFloats = 40960;                // 160 KiB
constexpr int64_t kDecMaxBatch = 256, kDecMaxWidth = 128, kDecMaxHidden = 256;
constexpr int64_t kDecMinChunk = 16;                    // the narrowest cotangent chunk the rule leaves room for

struct DecArgs {
  int B, P, H, Hp;
  int max_hid;
  int NC;                 // backward: columns per cotangent chunk (a multiple of 4)
  int r0, hid_floats;     // backward: floats of the first two LDS regions; forward: r0 = B * Hp
  int64_t N;
};

int64_t ceil4(int64_t v) { return (v + 3) / 4 * 4; }

int64_t bwd_floats(int64_t B, int64_t H, int64_t max_hid, int64_t nc) {
  const int64_t Hp = ceil4(H), hp = ceil4(max_hid);
  const int64_t dh = B * hp > kDecTileFloats ? B * hp : kDecTileFloats;
  return B * ((Hp > nc ? Hp : nc) + hp) + dh;
}

bool shape_ok(int64_t B, int64_t P, int64_t H, int64_t max_hid, int64_t max_out, int64_t total_out) {
  if (B < 0 || P < 0 || H < 1 || max_hid < 1 || max_out < 0 || total_out < max_out) return false;
  if (B > kDecMaxBatch || H > kDecMaxWidth || max_hid > kDecMaxHidden) return false;
  if (bwd_floats(B, H, max_hid, kDecMinChunk) > kDecLdsFloats) return false;
  const int64_t lim = ((int64_t)1 << 31) - 1;             // every tensor below 2^31 elements
  if (P > lim / (max_hid * H) || total_out > lim / max_hid) return false;       // w1, w2 (bounded by their widest block)
  return B == 0 || (P <= lim / (B * H) && total_out <= lim / B);               // h, out
}

DecArgs make_args(int64_t B, int64_t P, int64_t H, int64_t max_hid, int64_t total_out) {
  DecArgs a;
  a.B = (int)B; a.P = (int)P; a.H = (int)H; a.Hp = (int)ceil4(H);
  a.max_hid = (int)max_hid;
  a.NC = 64;
  while (a.NC > kDecMinChunk && bwd_floats(B, H, max_hid, a.NC) > kDecLdsFloats) a.NC /= 2;
  a.r0 = (int)(B * (a.Hp > a.NC ? a.Hp : a.NC));
  a.hid_floats = (int)(B * ceil4(max_hid));
  a.N = total_out;
  return a;
}

size_t fwd_bytes(const DecArgs& a) { return ((size_t)a.B * a.Hp + a.hid_floats + kDecTileFloats) * sizeof(float); }
size_t bwd_bytes(int64_t B, int64_t H, int64_t max_hid, int nc) { return (size_t)bwd_floats(B, H, max_hid, nc) * sizeof(float); }

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// h[:, p, :] -> hs [B][Hp], padding columns zero
__device__ __forceinline__ void stage_h(const float* __restrict__ h, float* hs, int p, const DecArgs& a) {
  if (a.H % 4 == 0 && aligned16(h)) {
    const int hv = a.H / 4;
    for (int e = threadIdx.x; e < a.B * hv; e += kBlock) {
      const int b = e / hv, d = (e - b * hv) * 4;
      float r[4];
      load_vec<4>(r, h + ((size_t)b * a.P + p) * a.H + d);
      store_vec<4>(hs + b * a.Hp + d, r);
    }
  } else {
    for (int e = threadIdx.x; e < a.B * a.Hp; e += kBlock) {
      const int b = e / a.Hp, d = e - b * a.Hp;
      hs[e] = d < a.H ? h[((size_t)b * a.P + p) * a.H + d] : 0.f;
    }
  }
}

// epi(b, j, sum_k X[b][k] W[j][k]) for b < B, j < J.  X: LDS, row stride sx (a multiple of 4, zero beyond K); W: global,
// [J][K] row-major; ws: the [64][33] staging tile.  Ends without a barrier.
template <class Epi>
__device__ __forceinline__ void gemm_nt(const float* X, int sx, int B, const float* __restrict__ W, int J, int K, float* ws,
                                        Epi epi) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const bool vec = K % 4 == 0 && aligned16(W);
  for (int j0 = 0; j0 < J; j0 += kWave) {
    for (int b0 = 0; b0 < B; b0 += kDecRowTile) {
      float acc[kDecRows];
#pragma unroll
      for (int r = 0; r < kDecRows; ++r) acc[r] = 0.f;
      for (int k0 = 0; k0 < K; k0 += kDecKC) {
        __syncthreads();                                                     // the tile's readers (and X's writers) are done
        if (vec) {
          for (int e = threadIdx.x; e < kWave * (kDecKC / 4); e += kBlock) {
            const int jj = e / (kDecKC / 4), kk = (e - jj * (kDecKC / 4)) * 4;
            float r[4] = {0.f, 0.f, 0.f, 0.f};
            if (j0 + jj < J && k0 + kk < K) load_vec<4>(r, W + (size_t)(j0 + jj) * K + k0 + kk);
#pragma unroll
            for (int c = 0; c < 4; ++c) ws[jj * kDecWS + kk + c] = r[c];
          }
        } else {
          for (int e = threadIdx.x; e < kWave * kDecKC; e += kBlock) {
            const int jj = e / kDecKC, kk = e - jj * kDecKC;
            ws[jj * kDecWS + kk] = (j0 + jj < J && k0 + kk < K) ? W[(size_t)(j0 + jj) * K + k0 + kk] : 0.f;
          }
        }
        __syncthreads();
        const int kend = K - k0 < kDecKC ? (K - k0 + 3) / 4 * 4 : kDecKC;
        const float* wr = ws + lane * kDecWS;
        for (int kk = 0; kk < kend; kk += 4) {
          const float w0 = wr[kk], w1 = wr[kk + 1], w2 = wr[kk + 2], w3 = wr[kk + 3];
#pragma unroll
          for (int r = 0; r < kDecRows; ++r) {
            const int row = b0 + wave + kWavesPerBlock * r;
            const float4 x = *reinterpret_cast<const float4*>(X + (row < B ? row : B - 1) * sx + k0 + kk);
            acc[r] = fmaf(x.x, w0, acc[r]); acc[r] = fmaf(x.y, w1, acc[r]);
            acc[r] = fmaf(x.z, w2, acc[r]); acc[r] = fmaf(x.w, w3, acc[r]);
          }
        }
      }
      if (j0 + lane < J) {
#pragma unroll
        for (int r = 0; r < kDecRows; ++r) {
          const int row = b0 + wave + kWavesPerBlock * r;
          if (row < B) epi(row, j0 + lane, acc[r]);
        }
      }
    }
  }
}

// epi(b, j, sum_k X[b][k] W[k][j]) for b < B, j < J.  X: LDS, row stride sx (a multiple of 4, zero beyond K); W: global,
// [K][J] row-major, read row by row (lanes along j).  No barrier inside.
template <class Epi>
__device__ __forceinline__ void gemm_nn(const float* X, int sx, int B, const float* __restrict__ W, int K, int J, Epi epi) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int j0 = 0; j0 < J; j0 += kWave) {
    const int j = j0 + lane, jc = j < J ? j : J - 1;
    for (int b0 = 0; b0 < B; b0 += kDecRowTile) {
      if (b0 + wave >= B) continue;                                          // (wave-uniform)
      float acc[kDecRows];
#pragma unroll
      for (int r = 0; r < kDecRows; ++r) acc[r] = 0.f;
      for (int k = 0; k < K; k += 4) {
        float w[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = k + c < K ? W[(size_t)(k + c) * J + jc] : 0.f;
#pragma unroll
        for (int r = 0; r < kDecRows; ++r) {
          const int row = b0 + wave + kWavesPerBlock * r;
          const float4 x = *reinterpret_cast<const float4*>(X + (row < B ? row : B - 1) * sx + k);
          acc[r] = fmaf(x.x, w[0], acc[r]); acc[r] = fmaf(x.y, w[1], acc[r]);
          acc[r] = fmaf(x.z, w[2], acc[r]); acc[r] = fmaf(x.w, w[3], acc[r]);
        }
      }
      if (j < J) {
#pragma unroll
        for (int r = 0; r < kDecRows; ++r) {
          const int row = b0 + wave + kWavesPerBlock * r;
          if (row < B) epi(row, j, acc[r]);
        }
      }
    }
  }
}

// epi(m, n, sum_b A[b][m] Y[b][n]) for m < M, n < Nn.  A, Y: LDS, row strides sa (a multiple of 4, >= M rounded up to 4)
// and sy.  Lanes along n, a wave owns 16 consecutive m.  No barrier inside.
template <class Epi>
__device__ __forceinline__ void gemm_tn(const float* A, int sa, int M, const float* Y, int sy, int Nn, int B, Epi epi) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int n0 = 0; n0 < Nn; n0 += kWave) {
    const int n = n0 + lane, nc = n < Nn ? n : Nn - 1;
    for (int m0 = 0; m0 < M; m0 += kDecRowTile) {
      const int mb = m0 + wave * kDecRows;
      if (mb >= M) continue;                                                 // (wave-uniform)
      float acc[kDecRows];
#pragma unroll
      for (int r = 0; r < kDecRows; ++r) acc[r] = 0.f;
      for (int b = 0; b < B; ++b) {
        const float y = Y[b * sy + nc];
#pragma unroll
        for (int q = 0; q < kDecRows / 4; ++q) {
          if (mb + 4 * q < M) {
            const float4 x = *reinterpret_cast<const float4*>(A + b * sa + mb + 4 * q);
            acc[4 * q] = fmaf(x.x, y, acc[4 * q]); acc[4 * q + 1] = fmaf(x.y, y, acc[4 * q + 1]);
            acc[4 * q + 2] = fmaf(x.z, y, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(x.w, y, acc[4 * q + 3]);
          }
        }
      }
      if (n < Nn) {
#pragma unroll
        for (int r = 0; r < kDecRows; ++r)
          if (mb + r < M) epi(mb + r, n, acc[r]);
      }
    }
  }
}

// out[j] = sum_b S[b][j], j < J
__device__ __forceinline__ void column_sums(const float* S, int ss, int B, int J, float* __restrict__ out) {
  for (int j = threadIdx.x; j < J; j += kBlock) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += S[b * ss + j];
    out[j] = s;
  }
}

struct DecBlock {
  int hid, hp, n;
  int64_t ho, oo, wo;
  bool ok;
};

// the tables are data: a block whose entries do not fit the launch (hid_p outside 1 .. max_hid, a negative length, columns
// past N) is left alone instead of read
__device__ __forceinline__ DecBlock block_of(const int64_t* __restrict__ hid_off, const int64_t* __restrict__ out_off,
                                             const int64_t* __restrict__ w2_off, int p, const DecArgs& a) {
  DecBlock k;
  k.ho = hid_off[p]; k.oo = out_off[p]; k.wo = w2_off[p];
  const int64_t hid = hid_off[p + 1] - k.ho, n = out_off[p + 1] - k.oo;
  k.ok = hid >= 1 && hid <= a.max_hid && n >= 0 && k.ho >= 0 && k.oo >= 0 && k.wo >= 0 && k.oo + n <= a.N;
  k.hid = (int)hid; k.hp = (int)((hid + 3) / 4 * 4); k.n = (int)n;
  return k;
}

// hs -> hid [B][hp] = relu(hs W1^T + b1), padding columns zero; ends with a barrier
__device__ __forceinline__ void hidden_rows(const float* hs, float* hid, float* ws, const float* __restrict__ w1,
                                            const float* __restrict__ b1, const DecBlock& k, const DecArgs& a) {
  if (k.hp != k.hid)
    for (int e = threadIdx.x; e < a.B * (k.hp - k.hid); e += kBlock) {
      const int b = e / (k.hp - k.hid);
      hid[b * k.hp + k.hid + (e - b * (k.hp - k.hid))] = 0.f;
    }
  const float* bias = b1 + k.ho;
  const int hp = k.hp;
  gemm_nt(hs, a.Hp, a.B, w1 + (size_t)k.ho * a.H, k.hid, a.H, ws,
          [=](int b, int j, float s) { hid[b * hp + j] = relu_keep_nan(s + bias[j]); });
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void pathway_decoder_fwd_kernel(
    const float* __restrict__ h, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, const int64_t* __restrict__ hid_off, const int64_t* __restrict__ out_off,
    const int64_t* __restrict__ w2_off, float* __restrict__ out, DecArgs a) {
  extern __shared__ float4 dec_lds[];
  const int p = blockIdx.x;
  const DecBlock k = block_of(hid_off, out_off, w2_off, p, a);
  if (!k.ok || k.n == 0) return;
  float* hs = reinterpret_cast<float*>(dec_lds);
  float* hid = hs + a.r0;
  float* ws = hid + a.hid_floats;
  stage_h(h, hs, p, a);
  hidden_rows(hs, hid, ws, w1, b1, k, a);
  const float* bias = b2 + k.oo;
  float* o = out + k.oo;
  const int64_t N = a.N;
  gemm_nt(hid, k.hp, a.B, w2 + k.wo, k.n, k.hid, ws, [=](int b, int j, float s) { o[(size_t)b * N + j] = s + bias[j]; });
}

__global__ __launch_bounds__(kBlock) void pathway_decoder_bwd_kernel(
    const float* __restrict__ h, const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ g, const int64_t* __restrict__ hid_off, const int64_t* __restrict__ out_off,
    const int64_t* __restrict__ w2_off, float* __restrict__ dh, float* __restrict__ dw1, float* __restrict__ db1,
    float* __restrict__ dw2, float* __restrict__ db2, DecArgs a) {
  extern __shared__ float4 dec_lds[];
  const int p = blockIdx.x;
  const DecBlock k = block_of(hid_off, out_off, w2_off, p, a);
  if (!k.ok) return;
  float* r0 = reinterpret_cast<float*>(dec_lds);
  float* hid = r0 + a.r0;
  float* dhid = hid + a.hid_floats;
  const bool want_dhid = dh || dw1 || db1;
  const int hp = k.hp, B = a.B;

  if (want_dhid || dw2) {
    stage_h(h, r0, p, a);
    hidden_rows(r0, hid, dhid, w1, b1, k, a);                                // (the staging tile lies over dhid)
  }
  if (want_dhid) {
    for (int e = threadIdx.x; e < B * hp; e += kBlock) dhid[e] = 0.f;
  }
  // the cotangent, NC columns at a time: dW2, db2 and dhid += g W2
  for (int c0 = 0; c0 < k.n; c0 += a.NC) {
    const int nc = k.n - c0 < a.NC ? k.n - c0 : a.NC, ncp = (nc + 3) / 4 * 4;
    __syncthreads();                                                         // r0's readers are done
    for (int e = threadIdx.x; e < B * ncp; e += kBlock) {
      const int b = e / ncp, jj = e - b * ncp;
      r0[e] = jj < nc ? g[(size_t)b * a.N + k.oo + c0 + jj] : 0.f;
    }
    __syncthreads();
    if (dw2) {
      float* o = dw2 + k.wo + (size_t)c0 * k.hid;
      const int ld = k.hid;
      gemm_tn(r0, ncp, nc, hid, hp, k.hid, B, [=](int m, int n, float s) { o[(size_t)m * ld + n] = s; });
    }
    if (db2) column_sums(r0, ncp, B, nc, db2 + k.oo + c0);
    if (want_dhid)
      gemm_nn(r0, ncp, B, w2 + k.wo + (size_t)c0 * k.hid, nc, k.hid, [=](int b, int j, float s) { dhid[b * hp + j] += s; });
  }
  if (!want_dhid) return;
  __syncthreads();
  for (int e = threadIdx.x; e < B * hp; e += kBlock)
    if (!(hid[e] > 0.f)) dhid[e] = 0.f;                                      // relu: result > 0 (the padding is 0 already)
  if (dw1) stage_h(h, r0, p, a);
  __syncthreads();
  if (dh) {
    const int P = a.P, H = a.H;
    gemm_nn(dhid, hp, B, w1 + (size_t)k.ho * a.H, k.hid, a.H,
            [=](int b, int j, float s) { dh[((size_t)b * P + p) * H + j] = s; });
  }
  if (db1) column_sums(dhid, hp, B, k.hid, db1 + k.ho);
  if (dw1) {
    float* o = dw1 + (size_t)k.ho * a.H;
    const int H = a.H;
    gemm_tn(dhid, hp, k.hid, r0, a.Hp, a.H, B, [=](int m, int n, float s) { o[(size_t)m * H + n] = s; });
  }
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_pathway_decoder_supported(int64_t B, int64_t P, int64_t H, int64_t max_hid, int64_t max_out,
                                               int64_t total_out) {
  return shape_ok(B, P, H, max_hid, max_out, total_out) ? 1 : 0;
}

extern "C" int mlgnn_pathway_decoder_fwd(const float* h, const float* w1, const float* b1, const float* w2, const float* b2,
                                         const int64_t* hid_off, const int64_t* out_off, const int64_t* w2_off, float* out,
                                         int64_t B, int64_t P, int64_t H, int64_t max_hid, int64_t max_out, int64_t total_out,
                                         void* stream) {
  if (!shape_ok(B, P, H, max_hid, max_out, total_out)) return MLGNN_E_SHAPE;
  if (B == 0 || P == 0 || total_out == 0) return 0;
  if (!h || !w1 || !b1 || !w2 || !b2 || !hid_off || !out_off || !w2_off || !out) return MLGNN_E_NULL;
  DecArgs a = make_args(B, P, H, max_hid, total_out);
  a.r0 = a.B * a.Hp;
  const size_t lds = fwd_bytes(a);
  if (lds > 64 * 1024)
    if (const hipError_t e = allow_dynamic_lds(&pathway_decoder_fwd_kernel, (int)lds); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(pathway_decoder_fwd_kernel, dim3((unsigned)P), dim3(kBlock), lds, as_stream(stream), h, w1, b1, w2, b2,
                     hid_off, out_off, w2_off, out, a);
  return (int)hipGetLastError();
}

extern "C" int mlgnn_pathway_decoder_bwd(const float* h, const float* w1, const float* b1, const float* w2, const float* g,
                                         const int64_t* hid_off, const int64_t* out_off, const int64_t* w2_off, float* dh,
                                         float* dw1, float* db1, float* dw2, float* db2, int64_t B, int64_t P, int64_t H,
                                         int64_t max_hid, int64_t max_out, int64_t total_out, void* stream) {
  if (!shape_ok(B, P, H, max_hid, max_out, total_out)) return MLGNN_E_SHAPE;
  if (B == 0 || P == 0) return 0;
  if (!dh && !dw1 && !db1 && !dw2 && !db2) return 0;
  if (!h || !w1 || !b1 || !w2 || !hid_off || !out_off || !w2_off || (!g && total_out > 0)) return MLGNN_E_NULL;
  const DecArgs a = make_args(B, P, H, max_hid, total_out);
  const size_t lds = bwd_bytes(B, H, max_hid, a.NC);
  if (lds > 64 * 1024)
    if (const hipError_t e = allow_dynamic_lds(&pathway_decoder_bwd_kernel, (int)lds); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(pathway_decoder_bwd_kernel, dim3((unsigned)P), dim3(kBlock), lds, as_stream(stream), h, w1, b1, w2, g,
                     hid_off, out_off, w2_off, dh, dw1, db1, dw2, db2, a);
  return (int)hipGetLastError();
}
