// bf16-storage halves of the tall dense kernels, called from the fp32 files that own the exported entry points:
// csrc/tallgemm_bf16.hip (from csrc/tallgemm.hip) and csrc/wgrad_bf16.hip (from csrc/wgrad.hip).
#pragma once
#include "common.h"

namespace mlgnn {

// tiles per column slice of the weight; 0 = shape not covered
int tb_tiles_per_slice(int64_t R, int64_t J);
int tallgemm_bf16(const void* a, const void* bt, const float* bias, const void* residual, void* c, void* workspace,
                  int64_t N, int64_t R, int64_t J, hipStream_t s, const float* lse = nullptr, void* gt = nullptr,
                  int* spread = nullptr);

// row slabs (= fp32 partial results in the workspace) of the weight gradient; 0 = shape not covered
int wb_slabs(int64_t N, int64_t M, int64_t K);
int linear_wgrad_bf16(const void* grad_out, const void* x, float* grad_w_b, float* workspace, int64_t N, int64_t M,
                      int64_t K, hipStream_t s);

}  // namespace mlgnn
