// The latent head of the VAE and its loss terms (models/vae.py: VAE.encoder behind the projection pooling, and the KL
// term of VAE.vae_loss) for every pathway at once: one launch forward, one backward plus one that adds the per-pathway
// parameter-gradient partials; one workgroup per pathway.
//
//   x [B, P, H]           the pooled latent; pathway p owns the n = B rows x[:, p, :]
//   w_mu, w_ls [H, H]     enc_mu / enc_log_sigma (row o = output o), b_mu, b_ls [H]; shared by all pathways, read from
//                         global memory (at most 64 KiB each: L2-resident across the workgroups)
//   mu    = x_p w_mu^T + b_mu,  sigma = exp(x_p w_ls^T + b_ls)                                   [B, P, H]
//   std_sum[p]  = sum_h std_b(mu[:, p, h])                 unbiased, two passes, the second on centred values
//   corr_sum[p] = sum_{i != j} |clamp(c_ij / d_i / d_j, -1, 1)|,  c = m~^T m~ / (B - 1), d_i = sqrt(c_ii)
//   kld_sum[p]  = sum_{b, h} (s^2 + mu^2 - 1) / 2 - log s,  s = sigma + 1e-7
//
// LDS image (floats; row stride S = H | 1, so lanes that walk rows of one column, or columns of one row, hit distinct
// banks with ds_read_b32): forward  xs | ms | ss (3 n S) + mean, dev (2 H) + red (8); backward  xs | ms | dm | ss (4 n S)
// + mean, dev, qs (3 H) + at, qt (2 * 16 H) + red (8).  n S <= 8192 + 256: at most 100 KiB forward, 150 KiB backward.
//
// Forward: stage x_p; thread (o, b) -- lanes walk rows, so the weight row is wave-uniform -- forms mu and sigma into LDS
// and its share of the KL sum; both are written out with h fastest; one thread per column takes mean and std; the rows
// are centred in place; thread (i, part) walks its share of the columns j for column i.
// Backward: d mu = g_mu + g_kld mu + the std and corr streams.  The corr stream goes by tiles of 16 columns j: thread
// (i, jj) forms c_ij and leaves a_ij = 2 g_corr sgn(r_ij) / ((B - 1) d_i d_j) in LDS, thread (b, i) adds
// sum_jj a_ij m~_bj to dm in jj order; the -r_ij m~_bi / d_i^2 halves are collected per column and applied once with the
// std stream, then the centring's backward.  d log-sigma = (g_sigma + g_kld (s - 1 / s)) sigma overwrites ss.
// grad_x = dmu w_mu + dls w_ls; the weight and bias gradients of the pathway (sums over its rows in row order) go to
// the caller's workspace and are added over the pathways in index order by the second launch.
// No atomics, every sum in a fixed order: bitwise reproducible.
#include <math.h>

#include "common.h"
#include "launch.h"
#include "mlgnn.h"

namespace mlgnn {
namespace {

constexpr int64_t kLatMaxRows = 256;
constexpr int64_t kLatMaxWidth = 128;
constexpr int64_t kLatMaxFloats = 8192;    // n * H: one row set of a pathway, unpadded, is 32 KiB
constexpr int kLatTile = 16;               // the backward's corr stream: columns j per tile
constexpr float kLatEps = 1e-7f;

struct LatArgs {
  int n, P, H;
  int S;            // LDS row stride in floats
};

bool shape_ok(int64_t B, int64_t P, int64_t H) {
  if (B < 2 || B > kLatMaxRows || P < 0 || H < 1 || H > kLatMaxWidth || B * H > kLatMaxFloats) return false;
  return P <= (((int64_t)1 << 30) - 1) / (B * H);           // B * P * H floats below 4 GiB
}

LatArgs make_args(int64_t B, int64_t P, int64_t H) {
  LatArgs a;
  a.n = (int)B; a.P = (int)P; a.H = (int)H;
  a.S = (int)(H | 1);
  return a;
}

int tile_cols(const LatArgs& a) { return a.H < kLatTile ? a.H : kLatTile; }
size_t fwd_lds_bytes(const LatArgs& a) { return ((size_t)3 * a.n * a.S + 2 * a.H + 8) * sizeof(float); }
size_t bwd_lds_bytes(const LatArgs& a) {
  return ((size_t)4 * a.n * a.S + 3 * a.H + 2 * (size_t)tile_cols(a) * a.H + 8) * sizeof(float);
}
// the backward's workspace: per pathway  grad_w_mu [H, H] | grad_b_mu [H] | grad_w_ls [H, H] | grad_b_ls [H]
int64_t partial_cols(int64_t H) { return 2 * H * H + 2 * H; }

// sum over the workgroup: lanes by the xor butterfly, then the four waves in wave order; every thread gets it
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int w = 1; w < kWavesPerBlock; ++w) t += red[w];
  __syncthreads();                                                           // red may be written again
  return t;
}

// rows src[:, p, :] -> dst (row stride a.S), h fastest
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, float* dst, const LatArgs& a) {
  for (int e = threadIdx.x; e < a.n * a.H; e += kBlock) {
    const int b = e / a.H, h = e - b * a.H;
    dst[b * a.S + h] = src[((size_t)b * a.P + blockIdx.x) * a.H + h];
  }
}

// one thread per column: mean[h], dev[h] = sqrt(sum_b (m_bh - mean_h)^2 / (n - 1))
__device__ __forceinline__ void column_stats(const float* ms, float* mean, float* dev, const LatArgs& a) {
  if ((int)threadIdx.x < a.H) {
    const int h = threadIdx.x;
    float s = 0.f;
    for (int b = 0; b < a.n; ++b) s += ms[b * a.S + h];
    const float m = s / (float)a.n;
    float q = 0.f;
    for (int b = 0; b < a.n; ++b) {
      const float d = ms[b * a.S + h] - m;
      q = fmaf(d, d, q);
    }
    mean[h] = m;
    dev[h] = sqrtf(q / (float)(a.n - 1));
  }
}

__device__ __forceinline__ void centre_rows(float* ms, const float* mean, const LatArgs& a) {
  for (int e = threadIdx.x; e < a.n * a.H; e += kBlock) {
    const int b = e / a.H, h = e - b * a.H;
    ms[b * a.S + h] -= mean[h];
  }
}

// c_ij / (n - 1) / d_i / d_j over the centred rows
__device__ __forceinline__ float corr_of(const float* ms, int i, int j, float di, float dj, const LatArgs& a) {
  float c = 0.f;
  for (int b = 0; b < a.n; ++b) c = fmaf(ms[b * a.S + i], ms[b * a.S + j], c);
  return c / (float)(a.n - 1) / di / dj;
}

__global__ __launch_bounds__(kBlock) void vae_latent_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ w_mu, const float* __restrict__ b_mu,
    const float* __restrict__ w_ls, const float* __restrict__ b_ls, float* __restrict__ mu, float* __restrict__ sigma,
    float* __restrict__ std_sum, float* __restrict__ corr_sum, float* __restrict__ kld_sum, LatArgs a) {
  extern __shared__ float4 lat_lds[];
  float* xs = reinterpret_cast<float*>(lat_lds);
  float* ms = xs + a.n * a.S;
  float* ss = ms + a.n * a.S;
  float* mean = ss + a.n * a.S;
  float* dev = mean + a.H;
  float* red = dev + a.H;
  stage_rows(x, xs, a);
  __syncthreads();

  float kld = 0.f;
  for (int e = threadIdx.x; e < a.n * a.H; e += kBlock) {
    const int o = e / a.n, b = e - o * a.n;
    const float* xr = xs + b * a.S;
    const float* wm = w_mu + (size_t)o * a.H;
    const float* wl = w_ls + (size_t)o * a.H;
    float am = b_mu[o], al = b_ls[o];
    for (int k = 0; k < a.H; ++k) {
      const float xv = xr[k];
      am = fmaf(xv, wm[k], am);
      al = fmaf(xv, wl[k], al);
    }
    const float sg = expf(al);
    ms[b * a.S + o] = am;
    ss[b * a.S + o] = sg;
    if (kld_sum) {
      const float s = sg + kLatEps;
      kld += 0.5f * (s * s + am * am - 1.f) - logf(s);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < a.n * a.H; e += kBlock) {
    const int b = e / a.H, h = e - b * a.H;
    const size_t g = ((size_t)b * a.P + blockIdx.x) * a.H + h;
    mu[g] = ms[b * a.S + h];
    sigma[g] = ss[b * a.S + h];
  }
  if (kld_sum) {
    const float t = block_sum(kld, red);
    if (threadIdx.x == 0) kld_sum[blockIdx.x] = t;
  }
  if (!std_sum && !corr_sum) return;

  column_stats(ms, mean, dev, a);
  __syncthreads();
  if (std_sum) {
    const float t = block_sum((int)threadIdx.x < a.H ? dev[threadIdx.x] : 0.f, red);
    if (threadIdx.x == 0) std_sum[blockIdx.x] = t;
  }
  if (!corr_sum) return;

  centre_rows(ms, mean, a);                      // (mu has left for global memory: the loop above, then a barrier)
  __syncthreads();
  const int parts = kBlock / a.H;                // >= 2: thread (i, part) takes the columns j = part, part + parts, ...
  const int i = threadIdx.x % a.H, part = threadIdx.x / a.H;
  float acc = 0.f;
  if (part < parts) {
    const float di = dev[i];
    for (int j = part; j < a.H; j += parts) {
      if (j == i) continue;
      float r = corr_of(ms, i, j, di, dev[j], a);
      r = r < -1.f ? -1.f : (r > 1.f ? 1.f : r);                             // a NaN stays, as through torch.clamp
      acc += fabsf(r);
    }
  }
  const float t = block_sum(acc, red);
  if (threadIdx.x == 0) corr_sum[blockIdx.x] = t;
}

struct LatWant {
  int x, w_mu, b_mu, w_ls, b_ls;     // which outputs of the backward are wanted
};

__global__ __launch_bounds__(kBlock) void vae_latent_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ w_mu, const float* __restrict__ w_ls,
    const float* __restrict__ mu, const float* __restrict__ sigma, const float* __restrict__ g_mu,
    const float* __restrict__ g_sigma, const float* __restrict__ g_std, const float* __restrict__ g_corr,
    const float* __restrict__ g_kld, float* __restrict__ grad_x, float* __restrict__ ws, LatWant want, LatArgs a) {
  extern __shared__ float4 lat_lds[];
  const int JT = a.H < kLatTile ? a.H : kLatTile;
  float* xs = reinterpret_cast<float*>(lat_lds);
  float* ms = xs + a.n * a.S;
  float* dm = ms + a.n * a.S;
  float* ss = dm + a.n * a.S;
  float* mean = ss + a.n * a.S;
  float* dev = mean + a.H;
  float* qs = dev + a.H;
  float* at = qs + a.H;              // [JT][H]
  float* qt = at + JT * a.H;         // [JT][H]
  const int p = blockIdx.x;
  const int nh = a.n * a.H;
  const bool want_dmu = want.x || want.w_mu || want.b_mu, want_dls = want.x || want.w_ls || want.b_ls;
  const bool stats = want_dmu && (g_std || g_corr);

  if (want.w_mu || want.w_ls) stage_rows(x, xs, a);
  if (want_dls) stage_rows(sigma, ss, a);
  if (stats) {
    stage_rows(mu, ms, a);
    __syncthreads();
    column_stats(ms, mean, dev, a);
    __syncthreads();
    centre_rows(ms, mean, a);
    for (int e = threadIdx.x; e < nh; e += kBlock) dm[(e / a.H) * a.S + e % a.H] = 0.f;
    if ((int)threadIdx.x < a.H) qs[threadIdx.x] = 0.f;
    __syncthreads();

    const float inv = 1.f / (float)(a.n - 1);
    if (g_corr && a.H > 1) {
      const float gc2 = 2.f * g_corr[p];
      for (int j0 = 0; j0 < a.H; j0 += JT) {
        const int cols = a.H - j0 < JT ? a.H - j0 : JT;
        for (int e = threadIdx.x; e < cols * a.H; e += kBlock) {
          const int jj = e / a.H, i = e - jj * a.H, j = j0 + jj;
          float av = 0.f, qv = 0.f;
          if (i != j) {
            const float di = dev[i], dj = dev[j];
            const float r = corr_of(ms, i, j, di, dj, a);
            float sgn = r > 0.f ? 1.f : (r < 0.f ? -1.f : r);                // sign(r); a NaN stays
            if (fabsf(r) > 1.f) sgn = 0.f;                                   // clamp passes gradient on [-1, 1]
            av = gc2 * sgn * inv / di / dj;
            qv = gc2 * sgn * r * inv / di / di;
          }
          at[jj * a.H + i] = av;
          qt[jj * a.H + i] = qv;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nh; e += kBlock) {
          const int b = e / a.H, i = e - b * a.H;
          float acc = dm[b * a.S + i];
          for (int jj = 0; jj < cols; ++jj) acc = fmaf(at[jj * a.H + i], ms[b * a.S + j0 + jj], acc);
          dm[b * a.S + i] = acc;
        }
        if ((int)threadIdx.x < a.H) {
          float q = qs[threadIdx.x];
          for (int jj = 0; jj < cols; ++jj) q += qt[jj * a.H + threadIdx.x];
          qs[threadIdx.x] = q;
        }
        __syncthreads();                                                     // the next tile overwrites at, qt
      }
    }
    // the column's own share: the std stream and the r_ij halves of the corr stream; then the centring's backward
    if ((int)threadIdx.x < a.H) {
      const int i = threadIdx.x;
      const float own = (g_std ? g_std[p] * inv / dev[i] : 0.f) - qs[i];
      float s = 0.f;
      for (int b = 0; b < a.n; ++b) {
        const float v = fmaf(own, ms[b * a.S + i], dm[b * a.S + i]);
        dm[b * a.S + i] = v;
        s += v;
      }
      const float m = s / (float)a.n;
      for (int b = 0; b < a.n; ++b) dm[b * a.S + i] -= m;
    }
  }
  __syncthreads();

  const float gk = g_kld ? g_kld[p] : 0.f;
  for (int e = threadIdx.x; e < nh; e += kBlock) {
    const int b = e / a.H, h = e - b * a.H;
    const size_t g = ((size_t)b * a.P + p) * a.H + h;
    if (want_dmu) {
      float d = stats ? dm[b * a.S + h] : 0.f;
      if (g_mu) d += g_mu[g];
      if (g_kld) d = fmaf(gk, mu[g], d);
      dm[b * a.S + h] = d;
    }
    if (want_dls) {
      const float sg = ss[b * a.S + h];
      float d = g_sigma ? g_sigma[g] : 0.f;
      if (g_kld) {
        const float s = sg + kLatEps;
        d = fmaf(gk, s - 1.f / s, d);
      }
      ss[b * a.S + h] = d * sg;
    }
  }
  __syncthreads();

  if (want.x) {
    for (int e = threadIdx.x; e < nh; e += kBlock) {
      const int b = e / a.H, k = e - b * a.H;
      float acc = 0.f;
      for (int o = 0; o < a.H; ++o) {
        acc = fmaf(dm[b * a.S + o], w_mu[(size_t)o * a.H + k], acc);
        acc = fmaf(ss[b * a.S + o], w_ls[(size_t)o * a.H + k], acc);
      }
      grad_x[((size_t)b * a.P + p) * a.H + k] = acc;
    }
  }
  if (!ws) return;
  const int hh = a.H * a.H;
  float* out = ws + (size_t)p * (2 * hh + 2 * a.H);
  if (want.w_mu || want.w_ls) {
    for (int e = threadIdx.x; e < hh; e += kBlock) {
      const int o = e / a.H, k = e - o * a.H;
      float am = 0.f, al = 0.f;
      for (int b = 0; b < a.n; ++b) {
        const float xv = xs[b * a.S + k];
        if (want.w_mu) am = fmaf(dm[b * a.S + o], xv, am);
        if (want.w_ls) al = fmaf(ss[b * a.S + o], xv, al);
      }
      if (want.w_mu) out[e] = am;
      if (want.w_ls) out[hh + a.H + e] = al;
    }
  }
  if ((int)threadIdx.x < a.H) {
    const int o = threadIdx.x;
    float am = 0.f, al = 0.f;
    for (int b = 0; b < a.n; ++b) {
      if (want.b_mu) am += dm[b * a.S + o];
      if (want.b_ls) al += ss[b * a.S + o];
    }
    if (want.b_mu) out[hh + o] = am;
    if (want.b_ls) out[2 * hh + a.H + o] = al;
  }
}

// ws [P][2 H H + 2 H] -> the four parameter gradients: one thread per element, the pathways added in index order
__global__ __launch_bounds__(kBlock) void vae_latent_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw_mu,
                                                                  float* __restrict__ gb_mu, float* __restrict__ gw_ls,
                                                                  float* __restrict__ gb_ls, int P, int H) {
  const int hh = H * H, cols = 2 * hh + 2 * H;
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= cols) return;
  float* dst;
  if (c < hh) dst = gw_mu ? gw_mu + c : nullptr;
  else if (c < hh + H) dst = gb_mu ? gb_mu + (c - hh) : nullptr;
  else if (c < 2 * hh + H) dst = gw_ls ? gw_ls + (c - hh - H) : nullptr;
  else dst = gb_ls ? gb_ls + (c - 2 * hh - H) : nullptr;
  if (!dst) return;                                                          // not wanted: its partials were not written
  float s = 0.f;
  for (int p = 0; p < P; ++p) s += ws[(size_t)p * cols + c];
  *dst = s;
}

}  // namespace
}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_vae_latent_supported(int64_t B, int64_t P, int64_t H) { return shape_ok(B, P, H) ? 1 : 0; }

extern "C" int mlgnn_vae_latent_fwd(const float* x, const float* w_mu, const float* b_mu, const float* w_ls, const float* b_ls,
                                    float* mu, float* sigma, float* std_sum, float* corr_sum, float* kld_sum, int64_t B,
                                    int64_t P, int64_t H, void* stream) {
  if (!shape_ok(B, P, H)) return MLGNN_E_SHAPE;
  if (P == 0) return 0;
  if (!x || !w_mu || !b_mu || !w_ls || !b_ls || !mu || !sigma) return MLGNN_E_NULL;
  const LatArgs a = make_args(B, P, H);
  const size_t lds = fwd_lds_bytes(a);
  if (lds > 64 * 1024)
    if (const hipError_t e = allow_dynamic_lds(&vae_latent_fwd_kernel, (int)lds); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(vae_latent_fwd_kernel, dim3((unsigned)a.P), dim3(kBlock), lds, as_stream(stream), x, w_mu, b_mu, w_ls,
                     b_ls, mu, sigma, std_sum, corr_sum, kld_sum, a);
  return (int)hipGetLastError();
}

extern "C" int mlgnn_vae_latent_bwd(const float* x, const float* w_mu, const float* w_ls, const float* mu, const float* sigma,
                                    const float* g_mu, const float* g_sigma, const float* g_std, const float* g_corr,
                                    const float* g_kld, float* grad_x, float* grad_w_mu, float* grad_b_mu, float* grad_w_ls,
                                    float* grad_b_ls, float* workspace, int64_t workspace_floats, int64_t B, int64_t P,
                                    int64_t H, void* stream) {
  if (!shape_ok(B, P, H)) return MLGNN_E_SHAPE;
  if (P == 0) return 0;
  const bool want_par = grad_w_mu || grad_b_mu || grad_w_ls || grad_b_ls;
  if (!grad_x && !want_par) return 0;
  if (!x || !w_mu || !w_ls || !mu || !sigma) return MLGNN_E_NULL;
  if (want_par && (!workspace || workspace_floats < P * partial_cols(H))) return MLGNN_E_WORKSPACE;
  const LatArgs a = make_args(B, P, H);
  const LatWant want = {grad_x != nullptr, grad_w_mu != nullptr, grad_b_mu != nullptr, grad_w_ls != nullptr,
                        grad_b_ls != nullptr};
  const size_t lds = bwd_lds_bytes(a);
  hipStream_t st = as_stream(stream);
  if (lds > 64 * 1024)
    if (const hipError_t e = allow_dynamic_lds(&vae_latent_bwd_kernel, (int)lds); e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(vae_latent_bwd_kernel, dim3((unsigned)a.P), dim3(kBlock), lds, st, x, w_mu, w_ls, mu, sigma, g_mu,
                     g_sigma, g_std, g_corr, g_kld, grad_x, want_par ? workspace : nullptr, want, a);
  if (const int e = (int)hipGetLastError(); e != 0 || !want_par) return e;
  const int cols = (int)partial_cols(H);
  hipLaunchKernelGGL(vae_latent_reduce_kernel, dim3((unsigned)((cols + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, workspace,
                     grad_w_mu, grad_b_mu, grad_w_ls, grad_b_ls, a.P, a.H);
  return (int)hipGetLastError();
}
