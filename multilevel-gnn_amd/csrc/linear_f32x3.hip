// fp32 nn.Linear on tall inputs whose widths are past the fp32 tall kernels (csrc/tallgemm.hip: weight image <= 128 KB,
// i.e. hidden width 512 at BASELINE configs[4]'s d = 256): the three-term bf16 products of csrc/diffpool_large_f32.hip
// (x y^T ~= x_hi y_hi^T + x_hi y_lo^T + x_lo y_hi^T; split and reduce kernels: csrc/gemm_chain.hip) -- the library's
// fp32 GEMMs for these shapes (200 000 x 256 x 512) run at ~40 TFLOP/s, 1.35 ms each.
//     forward   y  = x W^T + b          x [N,R], W [J,R]:  split {x, W}, one three-segment product (bias through aux, ld 0)
//     backward  dx = go W               split {go (+ go^T), x^T, W^T}, one product
//               dW = go^T x             one product over the row index, split along it, one reduce
// Reference: torch_nn.py:54-75 (the Linears of MLP).  R, J multiples of 128; the rows are padded to a multiple of 128
// inside the workspace (zero rows), y / dx are [Npad, .] buffers whose first N rows are the result.
#include "common.h"
#include "launch.h"
#include "gemm_chain.h"

namespace mlgnn {

inline int64_t lin3_pad(int64_t N) { return (N + 127) / 128 * 128; }
inline bool lin3_ok(int64_t N, int64_t R, int64_t J) {
  return N > 0 && N <= (int64_t)1 << 26 && R >= 128 && J >= 128 && R % 128 == 0 && J % 128 == 0 && R <= 8192 && J <= 8192;
}
inline int lin3_splits(int64_t Np, int64_t R, int64_t J) {
  const int tiles = (int)((J / kGemmTile) * (R / kGemmTile));
  int sp = 512 / tiles;
  const int64_t ktiles = 3 * Np / kGemmBK;
  if (sp > ktiles / 8) sp = (int)(ktiles / 8);
  return sp < 1 ? 1 : sp;
}

}  // namespace mlgnn

using namespace mlgnn;

extern "C" int mlgnn_linear_f32x3_supported(int64_t N, int64_t R, int64_t J) { return lin3_ok(N, R, J) ? 1 : 0; }

extern "C" int64_t mlgnn_linear_f32x3_padded_rows(int64_t N) { return N > 0 ? lin3_pad(N) : 0; }

extern "C" int64_t mlgnn_linear_f32x3_fwd_workspace_bytes(int64_t N, int64_t R, int64_t J) {
  if (!lin3_ok(N, R, J)) return MLGNN_E_SHAPE;
  const int64_t Np = lin3_pad(N);
  return (int64_t)(2 * align256((size_t)Np * R * 2) + 2 * align256((size_t)J * R * 2));
}

extern "C" int mlgnn_linear_f32x3_fwd(const float* x, const float* w, const float* bias, float* y, void* workspace,
                                      int64_t workspace_bytes, int64_t N, int64_t R, int64_t J, void* stream) {
  if (!lin3_ok(N, R, J)) return MLGNN_E_SHAPE;
  if (!x || !w || !y || !workspace) return MLGNN_E_NULL;
  if (workspace_bytes < mlgnn_linear_f32x3_fwd_workspace_bytes(N, R, J)) return MLGNN_E_WORKSPACE;
  if (!aligned(x, w, y, workspace, bias)) return MLGNN_E_ALIGN;
  const int64_t Np = lin3_pad(N);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  size_t o = 0;
  auto take = [&](size_t bytes) { unsigned char* p = ws + o; o += align256(bytes); return (uint16_t*)p; };
  uint16_t *xh = take((size_t)Np * R * 2), *xl = take((size_t)Np * R * 2);
  uint16_t *wh = take((size_t)J * R * 2), *wl = take((size_t)J * R * 2);
  SplitArgs a{};
  a.njobs = 2;
  a.job[0] = split_job(x, R, (int)Np, (int)R, 1, 0);
  a.job[0].rows_valid = (int)N; a.job[0].hi = xh; a.job[0].lo = xl; a.job[0].ldo = R;
  a.job[1] = split_job(w, R, (int)J, (int)R, 1, 0);
  a.job[1].hi = wh; a.job[1].lo = wl; a.job[1].ldo = R;
  DPL_CHECK(split_launch(a, 1, st));
  GemmDesc d{};
  d.nseg = 3;
  seg3(d, 0, xh, xl, wh, wl, R, R, (int)R, 0, 0);
  d.M = (int)Np; d.N = (int)J; d.splits = 1;
  d.c = y; d.ldc = J; d.c_f32 = 1;
  if (bias) { d.aux = bias; d.ldaux = 0; d.aux_f32 = 1; d.alpha = 1.f; }      // leading dimension 0: one row for all
  d.batch = 1;
  return gemm_nt_launch(d, st);
}

extern "C" int64_t mlgnn_linear_f32x3_bwd_workspace_bytes(int64_t N, int64_t R, int64_t J) {
  if (!lin3_ok(N, R, J)) return MLGNN_E_SHAPE;
  const int64_t Np = lin3_pad(N);
  size_t o = 0;
  o += 4 * align256((size_t)Np * J * 2);             // go hi / lo, go^T hi / lo
  o += 2 * align256((size_t)Np * R * 2);             // x^T hi / lo
  o += 2 * align256((size_t)J * R * 2);              // W^T hi / lo
  o += align256((size_t)lin3_splits(Np, R, J) * J * R * 4);
  o += align256(kReducePartials * 4);
  o += align256((size_t)(Np / 64) * J * 4);          // column sums of grad_out per tile row (the bias gradient's partials)
  return (int64_t)o;
}

// grad_x [Npad, R] (first N rows = the gradient; NULL: not wanted), grad_w [J, R], grad_bias [J] or NULL (the column
// sums of grad_out: partial sums per 64 rows from the split launch that reads grad_out anyway, fixed-order reduce).
extern "C" int mlgnn_linear_f32x3_bwd(const float* grad_out, const float* x, const float* w, float* grad_x, float* grad_w,
                                      float* grad_bias, void* workspace, int64_t workspace_bytes, int64_t N, int64_t R,
                                      int64_t J, void* stream) {
  if (!lin3_ok(N, R, J)) return MLGNN_E_SHAPE;
  if (!grad_out || !x || !w || !grad_w || !workspace) return MLGNN_E_NULL;
  if (workspace_bytes < mlgnn_linear_f32x3_bwd_workspace_bytes(N, R, J)) return MLGNN_E_WORKSPACE;
  if (!aligned(grad_out, x, w, grad_x, grad_w, workspace)) return MLGNN_E_ALIGN;
  const int64_t Np = lin3_pad(N);
  const int splits = lin3_splits(Np, R, J);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  size_t o = 0;
  auto take = [&](size_t bytes) { unsigned char* p = ws + o; o += align256(bytes); return p; };
  uint16_t *gh = (uint16_t*)take((size_t)Np * J * 2), *gl = (uint16_t*)take((size_t)Np * J * 2);
  uint16_t *gth = (uint16_t*)take((size_t)Np * J * 2), *gtl = (uint16_t*)take((size_t)Np * J * 2);
  uint16_t *xth = (uint16_t*)take((size_t)Np * R * 2), *xtl = (uint16_t*)take((size_t)Np * R * 2);
  uint16_t *wth = (uint16_t*)take((size_t)J * R * 2), *wtl = (uint16_t*)take((size_t)J * R * 2);
  float* slab = (float*)take((size_t)splits * J * R * 4);
  float* scratch = (float*)take(kReducePartials * 4);
  float* colsum = (float*)take((size_t)(Np / 64) * J * 4);
  {
    SplitArgs a{};
    a.njobs = 3;
    SplitJob& g = a.job[0];
    g = split_job(grad_out, J, (int)Np, (int)J, 1, 0);
    g.rows_valid = (int)N; g.hi = gh; g.lo = gl; g.ldo = J; g.hit = gth; g.lot = gtl; g.ldt = Np;
    g.colsum = grad_bias ? colsum : nullptr;
    SplitJob& xj = a.job[1];
    xj = split_job(x, R, (int)Np, (int)R, 1, 0);
    xj.rows_valid = (int)N; xj.hit = xth; xj.lot = xtl; xj.ldt = Np;
    SplitJob& wj = a.job[2];
    wj = split_job(w, R, (int)J, (int)R, 1, 0);
    wj.hit = wth; wj.lot = wtl; wj.ldt = J;
    DPL_CHECK(split_launch(a, 1, st));
  }
  if (grad_x) {                                        // dx = go W:  go [Np, J] x (W^T [R, J])^T
    GemmDesc d{};
    d.nseg = 3;
    seg3(d, 0, gh, gl, wth, wtl, J, J, (int)J, 0, 0);
    d.M = (int)Np; d.N = (int)R; d.splits = 1;
    d.c = grad_x; d.ldc = R; d.c_f32 = 1;
    d.batch = 1;
    DPL_CHECK(gemm_nt_launch(d, st));
  }
  {                                                    // dW = go^T x:  go^T [J, Np] x (x^T [R, Np])^T, split along the rows
    GemmDesc d{};
    d.nseg = 3;
    seg3(d, 0, gth, gtl, xth, xtl, Np, Np, (int)Np, 0, 0);
    d.M = (int)J; d.N = (int)R; d.splits = splits; d.slab = slab;
    d.batch = 1;
    DPL_CHECK(gemm_nt_launch(d, st));
    SlabReduceArgs r{};
    r.slab = slab; r.splits = splits; r.M = (int)J; r.N = (int)R; r.n_a = (int)R; r.n_b = (int)R;
    r.ca = grad_w; r.lda = R; r.ca_f32 = 1;
    r.cb = (uint16_t*)scratch; r.ldb = R; r.sq_partial = scratch;
    r.cc = grad_w; r.ldc = R; r.cc_f32 = 1;
    slab_reduce_launch(r, 1, st);
  }
  if (grad_bias) launch_reduce_partials(colsum, grad_bias, (int)(Np / 64), (int)J, st);
  return (int)hipGetLastError();
}
