// Host-side vocabulary shared by the chains of big bf16 "NT" products (csrc/gemm_nt.hip): the bf16 DiffPool chain
// (csrc/diffpool_large.hip), its fp32 three-term form (csrc/diffpool_large_f32.hip) and the fp32 three-term nn.Linear
// (csrc/linear_f32x3.hip).  The kernels behind slab_reduce_launch / split_launch are in csrc/gemm_chain.hip, those behind
// dpl_final_launch / dpl_softmax_bwd_f32_launch in csrc/diffpool_large.hip.
#pragma once
#include "gemm_nt.h"
#include "mlgnn.h"

// early return of a launcher's error code
#define DPL_CHECK(expr)       \
  do {                        \
    const int rc_ = (expr);   \
    if (rc_ != 0) return rc_; \
  } while (0)

namespace mlgnn {

constexpr float kDplEps = 1e-15f;
constexpr int kReducePartials = 1024;    // workgroups of the split-K reduce (= partial sums of its middle column range)

inline bool dpl_supported(int64_t N, int64_t K, int64_t C) {
  return N >= kGemmTile && K >= kGemmTile && C >= kGemmTile && N % kGemmTile == 0 && K % kGemmTile == 0 &&
         C % kGemmTile == 0 && N <= 32768 && K <= 8192 && C <= 8192;
}

// ---- split-K reduce of [A' | G | X'] -------------------------------------------------------------------------------
// out[i] = sum_z slab[z][i]  in a fixed order; columns [0, n_a) of every row go to `ca` (bf16 or fp32, leading
// dimension lda), columns [n_a, n_b) to `cb` (bf16, leading dimension ldb) with their squares summed per workgroup
// into sq_partial (||.||_F^2 of that column range), columns [n_b, N) to `cc`.
// (Measured and not kept: the forward scalars computed by the workgroup that finishes last, found through a completion
// counter.  The device-scope release in front of the counter writes back the XCD's whole L2 on this part -- 1024
// workgroups doing that took the reduce from 6 to 34 us; the separate one-workgroup launch costs 5.)
struct SlabReduceArgs {
  const float* slab; int splits; int M, N, n_a, n_b;
  void* ca; int64_t lda; int ca_f32;
  uint16_t* cb; int64_t ldb; float* sq_partial;
  void* cc; int64_t ldc; int cc_f32;
  int cb_f32;                          // the middle column range is kept in fp32 (the three-term fp32 chain)
  int64_t s_ca, s_cc, ws_stride;       // grouped launch: element strides of ca / cc, bytes between per-graph workspaces
};

// kReducePartials workgroups per graph of the batch (sq_partial holds that many sums per graph)
void slab_reduce_launch(const SlabReduceArgs& r, int batch, hipStream_t st);

// One job of a split launch: src [R, Cc] fp32 (leading dimension ld; R, Cc multiples of 64) ->
//   hi / lo   [R, Cc] bf16 (leading dimension ldo), when hi != NULL
//   hit / lot [Cc, R] bf16 (leading dimension ldt), when hit != NULL  (64 x 64 tiles through LDS)
//   partial[tile] = sum over the tile of src * dot (dot == src: the sum of squares), when dot != NULL
// Batch: graph blockIdx.y < nb runs the job on pointers advanced by the s_* strides (elements of each pointer's type).
struct SplitJob {
  const float* src; int64_t ld; int R, Cc;
  uint16_t *hi, *lo; int64_t ldo;
  uint16_t *hit, *lot; int64_t ldt;
  const float* dot; int64_t lddot; float* partial;
  int64_t s_src, s_out, s_outt, s_dot, s_part;
  int nb, tiles;
  int rows_valid;            // rows >= rows_valid of src do not exist: they split to zeros (a tall operand padded to R rows)
  float* colsum;             // non-NULL: colsum[tile row][Cc] = column sums of src over the 64 rows of each tile row
};
constexpr int kSplitMaxJobs = 4;
struct SplitArgs { SplitJob job[kSplitMaxJobs]; int njobs; };

inline SplitJob split_job(const float* src, int64_t ld, int R, int Cc, int nb, int64_t s_src) {
  SplitJob q{};
  q.src = src; q.ld = ld; q.R = R; q.Cc = Cc; q.nb = nb; q.s_src = s_src;
  q.tiles = (R / 64) * (Cc / 64);
  q.rows_valid = R;
  return q;
}

int split_launch(const SplitArgs& a, int batch, hipStream_t st);

// three-term product: (a_hi, b_hi), (a_hi, b_lo), (a_lo, b_hi) as segments i0 .. i0 + 2 of a descriptor
inline void seg3(GemmDesc& d, int i0, const uint16_t* ah, const uint16_t* al, const uint16_t* bh, const uint16_t* bl,
                 int64_t lda, int64_t ldb, int K, int64_t sa, int64_t sb) {
  d.seg[i0] = GemmSeg{ah, bh, lda, ldb, K, sa, sb};
  d.seg[i0 + 1] = GemmSeg{ah, bl, lda, ldb, K, sa, sb};
  d.seg[i0 + 2] = GemmSeg{al, bh, lda, ldb, K, sa, sb};
}

// ---- forward scalars: stats = {link, ent, ||A - S S^T||_F} from the partial sums, fixed order ---------------------
struct DplFinalArgs {
  const float* a2; int n_a2;          // ||A||_F^2 partials
  const float* dot; int n_dot;        // <S, A S> partials
  const float* g2; int n_g2;          // ||S^T S||_F^2 partials
  const float* ent; int n_ent;        // entropy partials
  float* stats; void* scal_out; int scal_f32; float inv_numel; float inv_rows;
  // a batch: the partial sums of graph b sit ws_floats further on (a2: only the first adj_batch graphs have their own);
  // the reference takes ONE Frobenius norm over the whole batch and the mean entropy over all its nodes
  int batch, adj_batch; int64_t ws_floats;
};

// one workgroup for the whole batch
void dpl_final_launch(const DplFinalArgs& f, hipStream_t st);

// softmax backward (with the entropy term) of fp32 logits [batch, N, K]; ds_stride: floats between the graphs' ds
void dpl_softmax_bwd_f32_launch(const float* logits, const float* ds, const float* coef, float* dlogits, int N, int K,
                                int64_t ds_stride, int batch, hipStream_t st);

}  // namespace mlgnn
