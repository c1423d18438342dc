// The MMD term of the VAE's pre-training loss (models/vae.py: compute_kernel ... compute_mmd) for every pathway at once:
// one launch forward, one backward, one workgroup per pathway.
//
//   z, prior  [B, P, H]   the latent and the prior draw; pathway p owns the n = B rows z[:, p, :] / prior[:, p, :]
//   terms     [P, 3]      (T_pp, T_zz, T_pz), the three kernel sums;  mmd [P] = T_pp + T_zz - 2 T_pz
//
//   imq:  k(a, b) = c / (c_eps + |a - b|^2),      T = sum over the pairs i != j
//   rbf:  k(a, b) = exp(-(|a - b|^2 / H) / c),    T = mean over all n^2 pairs (so T_pz has a gradient through i == j)
//
// Both operands of a pathway (2 n H floats, at most 64 KiB before padding) are staged in LDS straight from the [B, P, H]
// tensors.  Lanes walk rows, so the row stride is padded to an odd number of floats (ds_read_b32, banks mod 32) or, when
// H % 4 == 0 and the operands are 16-byte aligned, to an odd number of 16-byte slots (ds_read_b128, 16 lanes over the
// 64 banks): conflict-free either way.  Squared distances are sums of (a_d - b_d)^2 in fp32 -- the mmd is a difference
// of nearly equal sums, the norm expansion would lose it.
//
// Forward: thread (i, js) takes row i against the rows j = js, js + step, ...; its three sums are reduced over the
// lanes (xor butterfly) and then over the four waves in wave order.  The imq diagonal adds k - k (0, or NaN when k is
// NaN) as the torch lines' `kernel.sum() - kernel.diag().sum()` does.
// Backward: nothing but the inputs is read; for a tile of rows m the weights w_zz(m, j), w_pz(j, m) (k^2 for imq, k for
// rbf) of all j go to LDS, then one thread per (m, d) sums w_zz (z_j - z_m) - w_pz (p_j - z_m) over j in index order and
// writes grad_z[m, p, d] once.  No atomics in either direction: bitwise reproducible.
#include "common.h"
#include "launch.h"
#include "mlgnn.h"

namespace mlgnn {
namespace {

constexpr int64_t kMmdMaxRows = 256;       // n <= kBlock: one lane per row
constexpr int64_t kMmdMaxWidth = 256;
constexpr int64_t kMmdMaxFloats = 8192;    // n * H: 64 KiB for both operands, unpadded
constexpr int kMmdWeightPairs = 4352;      // the backward's weight tile: (w_zz, w_pz) pairs, 34 KiB (64 rows x 65: one tile)

struct MmdArgs {
  int n, P, H;
  int S;            // LDS row stride in floats
  int rshift;       // log2 of the lanes that walk rows (the next power of two >= n)
  int MT, WS;       // backward: rows per weight tile, its row stride in pairs
  float c_eps, c;
  float coef;       // backward: 4 / c (imq), 4 / (n^2 H c) (rbf)
};

bool shape_ok(int64_t B, int64_t P, int64_t H) {
  if (B < 0 || P < 0 || H < 1 || H > kMmdMaxWidth || B > kMmdMaxRows || B * H > kMmdMaxFloats) return false;
  return B == 0 || P <= (((int64_t)1 << 30) - 1) / (B * H);   // B * P * H floats below 4 GiB (an empty z is)
}

MmdArgs make_args(int64_t B, int64_t P, int64_t H, int vec, int kind, float c_eps, float c) {
  MmdArgs a;
  a.n = (int)B; a.P = (int)P; a.H = (int)H;
  a.S = vec == 4 ? 4 * (int)((H / 4) | 1) : (int)(H | 1);
  a.rshift = 0;
  while ((1 << a.rshift) < a.n) ++a.rshift;
  a.WS = a.n | 1;
  const int most = kMmdWeightPairs / a.WS;                 // >= 16 rows; tiles of equal height
  const int tiles = (a.n + most - 1) / most;
  a.MT = tiles ? (a.n + tiles - 1) / tiles : 0;
  a.c_eps = c_eps; a.c = c;
  a.coef = kind == 0 ? 4.f / c : 4.f / ((float)(a.n * a.n) * (float)a.H * c);
  return a;
}

size_t operand_bytes(const MmdArgs& a) { return (size_t)2 * a.n * a.S * sizeof(float); }
size_t weight_bytes(const MmdArgs& a) { return (size_t)a.MT * a.WS * sizeof(float2); }

template <int KIND>
__device__ __forceinline__ float kernel_value(float dist, const MmdArgs& a) {
  if constexpr (KIND == 0) return a.c / (a.c_eps + dist);
  else return expf(-(dist / (float)a.H / a.c));
}

// rows z[:, p, :] and prior[:, p, :] -> zs, ps (row stride a.S)
template <int VEC>
__device__ __forceinline__ void stage_rows(const float* __restrict__ z, const float* __restrict__ prior, float* zs, float* ps,
                                           const MmdArgs& a) {
  const int hv = a.H / VEC;
  for (int e = threadIdx.x; e < a.n * hv; e += kBlock) {
    const int b = e / hv, d = (e - b * hv) * VEC;
    const size_t g = ((size_t)b * a.P + blockIdx.x) * a.H + d;
    float r[VEC];
    load_vec<VEC>(r, z + g);
    store_vec<VEC>(zs + b * a.S + d, r);
    load_vec<VEC>(r, prior + g);
    store_vec<VEC>(ps + b * a.S + d, r);
  }
}

template <int VEC, int KIND>
__global__ __launch_bounds__(kBlock) void mmd_fwd_kernel(const float* __restrict__ z, const float* __restrict__ prior,
                                                        float* __restrict__ terms, float* __restrict__ mmd, MmdArgs a) {
  extern __shared__ float4 mmd_lds[];
  __shared__ float red[3][kWavesPerBlock];
  float* zs = reinterpret_cast<float*>(mmd_lds);
  float* ps = zs + a.n * a.S;
  stage_rows<VEC>(z, prior, zs, ps, a);
  __syncthreads();

  const int i = threadIdx.x & ((1 << a.rshift) - 1), js = threadIdx.x >> a.rshift, jstep = kBlock >> a.rshift;
  float spp = 0.f, szz = 0.f, spz = 0.f;
  if (i < a.n) {
    const float* zi = zs + i * a.S;
    const float* pi = ps + i * a.S;
    for (int j = js; j < a.n; j += jstep) {
      const float* zj = zs + j * a.S;
      const float* pj = ps + j * a.S;
      float dpp = 0.f, dzz = 0.f, dpz = 0.f;
      for (int d = 0; d < a.H; d += VEC) {
        float vzi[VEC], vpi[VEC], vzj[VEC], vpj[VEC];
        load_vec<VEC>(vzi, zi + d); load_vec<VEC>(vpi, pi + d);
        load_vec<VEC>(vzj, zj + d); load_vec<VEC>(vpj, pj + d);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const float tpp = vpi[v] - vpj[v], tzz = vzi[v] - vzj[v], tpz = vpi[v] - vzj[v];
          dpp = fmaf(tpp, tpp, dpp); dzz = fmaf(tzz, tzz, dzz); dpz = fmaf(tpz, tpz, dpz);
        }
      }
      float kpp = kernel_value<KIND>(dpp, a), kzz = kernel_value<KIND>(dzz, a), kpz = kernel_value<KIND>(dpz, a);
      if (KIND == 0 && i == j) { kpp -= kpp; kzz -= kzz; kpz -= kpz; }       // off-diagonal sum; a NaN stays
      spp += kpp; szz += kzz; spz += kpz;
    }
  }
  spp = wave_sum(spp); szz = wave_sum(szz); spz = wave_sum(spz);
  const int wave = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) { red[0][wave] = spp; red[1][wave] = szz; red[2][wave] = spz; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t[k] = red[k][0];
#pragma unroll
      for (int w = 1; w < kWavesPerBlock; ++w) t[k] += red[k][w];
      if (KIND == 1) t[k] = t[k] / (float)(a.n * a.n);
      if (terms) terms[(size_t)blockIdx.x * 3 + k] = t[k];
    }
    mmd[blockIdx.x] = t[0] + t[1] - 2.f * t[2];
  }
}

template <int VEC, int KIND>
__global__ __launch_bounds__(kBlock) void mmd_bwd_kernel(const float* __restrict__ z, const float* __restrict__ prior,
                                                        const float* __restrict__ grad_mmd, float* __restrict__ grad_z,
                                                        MmdArgs a) {
  extern __shared__ float4 mmd_lds[];
  float* zs = reinterpret_cast<float*>(mmd_lds);
  float* ps = zs + a.n * a.S;
  float2* wt = reinterpret_cast<float2*>(ps + a.n * a.S);                    // [MT][WS]: (w_zz(m, j), w_pz(j, m))
  stage_rows<VEC>(z, prior, zs, ps, a);
  __syncthreads();

  const float scale = grad_mmd[blockIdx.x] * a.coef;
  const int j = threadIdx.x & ((1 << a.rshift) - 1), ms = threadIdx.x >> a.rshift, mstep = kBlock >> a.rshift;
  for (int m0 = 0; m0 < a.n; m0 += a.MT) {
    const int rows = a.n - m0 < a.MT ? a.n - m0 : a.MT;
    if (j < a.n) {
      const float* zj = zs + j * a.S;
      const float* pj = ps + j * a.S;
      for (int mm = ms; mm < rows; mm += mstep) {
        const float* zm = zs + (m0 + mm) * a.S;
        float dzz = 0.f, dpz = 0.f;
        for (int d = 0; d < a.H; d += VEC) {
          float vzm[VEC], vzj[VEC], vpj[VEC];
          load_vec<VEC>(vzm, zm + d); load_vec<VEC>(vzj, zj + d); load_vec<VEC>(vpj, pj + d);
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const float tzz = vzm[v] - vzj[v], tpz = vpj[v] - vzm[v];
            dzz = fmaf(tzz, tzz, dzz); dpz = fmaf(tpz, tpz, dpz);
          }
        }
        float wzz = kernel_value<KIND>(dzz, a), wpz = kernel_value<KIND>(dpz, a);
        if (KIND == 0) {
          wzz *= wzz;
          wpz = (j == m0 + mm) ? 0.f : wpz * wpz;                            // the imq sums leave the pair i == j out
        }
        wt[mm * a.WS + j] = make_float2(wzz, wpz);
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < rows * a.H; e += kBlock) {
      const int mm = e / a.H, d = e - mm * a.H;
      const float zm = zs[(m0 + mm) * a.S + d];
      const float2* w = wt + mm * a.WS;
      float acc = 0.f;
      for (int jj = 0; jj < a.n; ++jj) {
        const float2 wj = w[jj];
        acc = fmaf(wj.x, zs[jj * a.S + d] - zm, acc);
        acc = fmaf(-wj.y, ps[jj * a.S + d] - zm, acc);
      }
      grad_z[((size_t)(m0 + mm) * a.P + blockIdx.x) * a.H + d] = scale * acc;
    }
    __syncthreads();                                                         // the next tile overwrites wt
  }
}

template <int VEC, int KIND>
int launch_fwd(const float* z, const float* prior, float* terms, float* mmd, const MmdArgs& a, hipStream_t st) {
  const size_t lds = operand_bytes(a);
  if (lds > 64 * 1024)
    if (const hipError_t e = allow_dynamic_lds(&mmd_fwd_kernel<VEC, KIND>, (int)lds); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((mmd_fwd_kernel<VEC, KIND>), dim3((unsigned)a.P), dim3(kBlock), lds, st, z, prior, terms, mmd, a);
  return (int)hipGetLastError();
}

template <int VEC, int KIND>
int launch_bwd(const float* z, const float* prior, const float* grad_mmd, float* grad_z, const MmdArgs& a, hipStream_t st) {
  const size_t lds = operand_bytes(a) + weight_bytes(a);
  if (lds > 64 * 1024)
    if (const hipError_t e = allow_dynamic_lds(&mmd_bwd_kernel<VEC, KIND>, (int)lds); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((mmd_bwd_kernel<VEC, KIND>), dim3((unsigned)a.P), dim3(kBlock), lds, st, z, prior, grad_mmd, grad_z, a);
  return (int)hipGetLastError();
}

// 16-byte rows: the vector loads of the staging and the ds_read_b128 of the pair loops
int vec_for(const float* z, const float* prior, int64_t H) { return (H % 4 == 0 && aligned(z, prior)) ? 4 : 1; }

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_mmd_supported(int64_t B, int64_t P, int64_t H) { return shape_ok(B, P, H) ? 1 : 0; }

extern "C" int mlgnn_mmd_fwd(const float* z, const float* prior, float* terms, float* mmd, int kind, float c_eps, float c,
                             int64_t B, int64_t P, int64_t H, void* stream) {
  if (!shape_ok(B, P, H)) return MLGNN_E_SHAPE;
  if (kind != 0 && kind != 1) return MLGNN_E_MODE;
  if (B == 0 || P == 0) return 0;
  if (!z || !prior || !mmd) return MLGNN_E_NULL;
  const int vec = vec_for(z, prior, H);
  const MmdArgs a = make_args(B, P, H, vec, kind, c_eps, c);
  hipStream_t st = as_stream(stream);
  if (vec == 4) return kind == 0 ? launch_fwd<4, 0>(z, prior, terms, mmd, a, st) : launch_fwd<4, 1>(z, prior, terms, mmd, a, st);
  return kind == 0 ? launch_fwd<1, 0>(z, prior, terms, mmd, a, st) : launch_fwd<1, 1>(z, prior, terms, mmd, a, st);
}

extern "C" int mlgnn_mmd_bwd(const float* z, const float* prior, const float* grad_mmd, float* grad_z, int kind, float c_eps,
                             float c, int64_t B, int64_t P, int64_t H, void* stream) {
  if (!shape_ok(B, P, H)) return MLGNN_E_SHAPE;
  if (kind != 0 && kind != 1) return MLGNN_E_MODE;
  if (B == 0 || P == 0) return 0;
  if (!z || !prior || !grad_mmd || !grad_z) return MLGNN_E_NULL;
  const int vec = vec_for(z, prior, H);
  const MmdArgs a = make_args(B, P, H, vec, kind, c_eps, c);
  hipStream_t st = as_stream(stream);
  if (vec == 4) return kind == 0 ? launch_bwd<4, 0>(z, prior, grad_mmd, grad_z, a, st) : launch_bwd<4, 1>(z, prior, grad_mmd, grad_z, a, st);
  return kind == 0 ? launch_bwd<1, 0>(z, prior, grad_mmd, grad_z, a, st) : launch_bwd<1, 1>(z, prior, grad_mmd, grad_z, a, st);
}
