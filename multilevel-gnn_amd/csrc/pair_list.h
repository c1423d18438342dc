// The pair list of the fold preparation's edge tests: rows (s, t) of pairs [P, 2] select two rows of xt [n_nodes, N], a
// row (s, -1) the single row s.  Shared by csrc/edge_select.hip, csrc/edge_select_cc.hip (through edge_prepare.h) and
// csrc/kraskov_mi.hip: the host's shape rule for the list and the device's decode of one row.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "common.h"

namespace mlgnn {

// What every pair-list entry point asks of its sizes apart from its own conditions on n and k (n >= 1 is the caller's):
// xt and, where a [P, N] output is asked for, that output as rows of N doubles below 4 GiB; P below 2^31 (the grid); no
// pair without a node.
inline bool pair_list_shape_ok(int64_t n, int64_t n_nodes, int64_t P, bool with_rows_out) {
  const int64_t most = (((int64_t)1 << 29) - 1) / n;                    // rows of N doubles below 4 GiB
  if (n_nodes < 0 || n_nodes > most || P < 0 || P >= ((int64_t)1 << 31)) return false;
  if (P > 0 && n_nodes < 1) return false;
  return !with_rows_out || P <= most;
}

// Row `pair` of the list -> the two rows of xt and whether the pair is a single column (uniform over the workgroup; xq is
// xs then).  Node indices are clamped to [0, n_nodes), so a wrong value cannot read outside xt.
__device__ __forceinline__ bool pair_rows(const double* __restrict__ xt, const int32_t* __restrict__ pairs, size_t pair,
                                          int N, int n_nodes, const double*& xs, const double*& xq) {
  int s = pairs[2 * pair], t = pairs[2 * pair + 1];
  const bool single = t < 0;
  s = min(max(s, 0), n_nodes - 1);
  t = single ? s : min(t, n_nodes - 1);
  xs = xt + (size_t)s * N;
  xq = xt + (size_t)t * N;
  return single;
}

}  // namespace mlgnn
