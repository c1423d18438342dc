"""csrc/dispatch.h on the host: ``dispatch_int`` reaches the listed constant exactly once and nothing else, ``IntList``
answers ``has`` for exactly the values it dispatches, ``aligned`` accepts null and multiples of the alignment only.
csrc/wgrad_plan.h: the plan of every tile count is the one the hand-written search gave, and a row of the launch table.
Small C++17 programs with their own ``main`` are compiled with the clang of the ROCm toolchain (host only, no HIP) and
run; they need no GPU.  The shape predicates of the tall-Linear entry points are swept through ``ctypes`` (no launch)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilevel-gnn_amd"))

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "dispatch.h"
using namespace mlgnn;

static int failures = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("line %d: %s\n", __LINE__, #__VA_ARGS__); ++failures; } } while (0)

// every v in [lo, hi]: a listed v reaches f once, with IC<v>; any other v returns false and calls nothing
template <int... Vs>
static void sweep(int lo, int hi) {
  const std::vector<int> listed{Vs...};
  for (int v = lo; v <= hi; ++v) {
    int calls = 0, seen = -12345;
    const bool hit = dispatch_int<Vs...>(v, [&](auto c) {
      static_assert(((decltype(c)::value == Vs) || ...), "a constant that is not in the list");
      ++calls;
      seen = c();
    });
    bool in_list = false;
    for (int l : listed) in_list = in_list || l == v;
    CHECK(hit == in_list);
    CHECK(calls == (in_list ? 1 : 0));
    if (in_list) CHECK(seen == v);
  }
}

// IntList: has() says yes exactly where dispatch() reaches a constant
template <int... Vs>
static void sweep_list(IntList<Vs...>, int lo, int hi) {
  sweep<Vs...>(lo, hi);
  for (int v = lo; v <= hi; ++v) {
    int seen = -12345;
    const bool hit = IntList<Vs...>::dispatch(v, [&](auto c) { seen = c(); });
    CHECK(hit == IntList<Vs...>::has(v));
    if (hit) CHECK(seen == v);
  }
  static_assert((IntList<Vs...>::has(Vs) && ...), "has() is usable in constant expressions");
  CHECK(!IntList<Vs...>::has(int64_t{1} << 40));
}

int main() {
  // the value lists of the sources: LayerNorm lanes-per-row log2, lanes per row, narrow-linear R, narrow-linear lanes,
  // projection K, short-row lanes, bf16 tall GEMM tiles per slice
  sweep<0, 1, 2, 3, 4, 5, 6>(-3, 10);
  sweep<1, 2, 4, 8, 16, 32, 64>(-1, 130);
  sweep<1, 2, 3, 4, 5, 6, 7, 8>(-2, 12);
  sweep<8, 16, 32, 64>(0, 130);
  sweep<1, 2, 3, 4>(-2, 8);
  sweep<1, 2, 4, 8, 16>(-1, 40);
  sweep<1, 2, 4, 8>(-1, 20);
  // fp32 tall GEMM (csrc/tallgemm.hip): column tiles and k-steps of the plain, LayerNorm, POST / SHIFT and DUAL
  // families; bf16 weight gradient (csrc/wgrad_bf16.hip): tiles per wave along M and K
  sweep_list(IntList<1, 2, 4, 8>{}, -1, 20);
  sweep_list(IntList<1, 2, 4, 8, 16>{}, -1, 40);
  sweep_list(IntList<2, 4, 8>{}, -1, 20);
  sweep_list(IntList<4, 8, 16>{}, -1, 40);
  sweep_list(IntList<2, 4>{}, -1, 20);
  sweep_list(IntList<1, 2, 4>{}, -1, 20);
  sweep_list(IntList<2, 4, 8, 16>{}, -1, 40);
  sweep_list(IntList<1, 2>{}, -1, 20);
  CHECK(!dispatch_int<1, 2, 4>(0x7fffffff, [](auto) {}));
  CHECK(!dispatch_int<1, 2, 4>(-0x7fffffff - 1, [](auto) {}));

  alignas(64) static char buf[256];
  const char* null_c = nullptr;
  const float* null_f = nullptr;
  CHECK(aligned(null_c) && aligned<8>(null_c) && aligned<4>(null_c));
  CHECK(aligned(null_c, null_f));
  CHECK(aligned(buf) && aligned(buf + 16) && aligned(buf + 32) && aligned<16>(buf + 48));
  CHECK(aligned<8>(buf) && aligned<8>(buf + 8) && aligned<8>(buf + 16));
  CHECK(aligned<4>(buf) && aligned<4>(buf + 4) && aligned<4>(buf + 8) && aligned<4>(buf + 16));
  CHECK(!aligned(buf + 1) && !aligned(buf + 4) && !aligned(buf + 8));
  CHECK(!aligned<8>(buf + 1) && !aligned<8>(buf + 4) && aligned<8>(buf + 8));
  CHECK(!aligned<4>(buf + 1) && aligned<4>(buf + 4) && aligned<4>(buf + 8));
  // mixed packs: pointer types differ, null among them, one offender anywhere in the pack
  const float* f = reinterpret_cast<const float*>(buf + 32);
  const void* v = buf + 64;
  const unsigned char* u = reinterpret_cast<const unsigned char*>(buf + 96);
  CHECK(aligned(f, v, u) && aligned(f, null_c, v, null_f, u));
  CHECK(!aligned(buf + 1, v, u) && !aligned(f, buf + 4, u) && !aligned(f, v, buf + 8) && !aligned(null_c, buf + 8));
  CHECK(aligned<8>(f, buf + 8, null_f) && !aligned<8>(f, buf + 4, null_f));
  CHECK(aligned<4>(f, buf + 4, buf + 8) && !aligned<4>(f, buf + 4, buf + 1));
  CHECK(aligned());                                     // the empty pack
  if (failures == 0) std::printf("dispatch ok\n");
  return failures == 0 ? 0 : 1;
}
"""


def host_compiler():
    import build_native
    bindir = os.path.dirname(os.path.realpath(build_native.HIPCC))
    for cxx in (os.path.join(os.path.dirname(bindir), "llvm", "bin", "clang++"), os.path.join(bindir, "amdclang++")):
        if os.path.exists(cxx):
            return cxx
    pytest.fail("no clang++ next to %s" % build_native.HIPCC)


def _build_and_run(tmp_path, name, program):
    import build_native
    src, exe = tmp_path / (name + ".cpp"), tmp_path / name
    src.write_text(program)
    cmd = [host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + build_native.CSRC, str(src), "-o", str(exe)]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert ran.returncode == 0, ran.stdout
    return ran.stdout


def test_dispatch_int_and_aligned(tmp_path):
    assert "dispatch ok" in _build_and_run(tmp_path, "dispatch_host", PROGRAM)


# ---- csrc/wgrad_plan.h ------------------------------------------------------------------------------------------------

_ = None
# PLANS_BEFORE[tiles_m - 1][tiles_k - 1] = (nw, wm, wk, tm, tk), or None where no plan covers the output
PLANS_BEFORE = [
    [(4, 2, 2, 1, 1), (4, 2, 2, 1, 1), (4, 1, 4, 1, 1), (4, 1, 4, 1, 1), (4, 1, 4, 1, 2), (4, 1, 4, 1, 2), (4, 1, 4, 1, 2), (4, 1, 4, 1, 2), (4, 1, 4, 1, 4)],
    [(4, 2, 2, 1, 1), (4, 2, 2, 1, 1), (4, 2, 2, 1, 2), (4, 2, 2, 1, 2), (4, 1, 4, 2, 2), (4, 1, 4, 2, 2), (4, 1, 4, 2, 2), (4, 1, 4, 2, 2), (8, 1, 8, 2, 2)],
    [(4, 4, 1, 1, 1), (4, 2, 2, 2, 1), (4, 2, 2, 2, 2), (4, 2, 2, 2, 2), (8, 2, 4, 2, 2), (8, 2, 4, 2, 2), (8, 2, 4, 2, 2), (8, 2, 4, 2, 2), _],
    [(4, 4, 1, 1, 1), (4, 2, 2, 2, 1), (4, 2, 2, 2, 2), (4, 2, 2, 2, 2), (8, 2, 4, 2, 2), (8, 2, 4, 2, 2), (8, 2, 4, 2, 2), (8, 2, 4, 2, 2), _],
    [(4, 4, 1, 2, 1), (4, 4, 1, 2, 2), (8, 4, 2, 2, 2), (8, 4, 2, 2, 2), _, _, _, _, _],
    [(4, 4, 1, 2, 1), (4, 4, 1, 2, 2), (8, 4, 2, 2, 2), (8, 4, 2, 2, 2), _, _, _, _, _],
    [(4, 4, 1, 2, 1), (4, 4, 1, 2, 2), (8, 4, 2, 2, 2), (8, 4, 2, 2, 2), _, _, _, _, _],
    [(4, 4, 1, 2, 1), (4, 4, 1, 2, 2), (8, 4, 2, 2, 2), (8, 4, 2, 2, 2), _, _, _, _, _],
    [(4, 4, 1, 4, 1), (8, 8, 1, 2, 2), _, _, _, _, _, _, _],
]

PLAN_PROGRAM = r"""
#include <cstdio>
#include "wgrad_plan.h"
using namespace mlgnn;

// usable in constant expressions: the launcher instantiates kernels from the rows
static_assert(kWgradRows == 28, "18 four-wave rows + 10 eight-wave rows");
static_assert(plan_wgrad(4, 8) >= 0 && kWgradTable.row[plan_wgrad(4, 8)].nw == 8, "the flagship 128 x 256 gradient");
static_assert(plan_wgrad(9, 9) == -1, "");

int main() {
  // every row obeys the two rules that admit it, exactly once
  for (int i = 0; i < kWgradRows; ++i) {
    const WgradPlan& p = kWgradTable.row[i];
    const bool ok = p.nw == p.wm * p.wk && (p.nw == 4 || (p.nw == 8 && p.tm * p.tk == 4)) && p.tm * p.tk <= 4 &&
                    lds_fits((p.wm * p.tm + p.wk * p.tk) * kTile, p.nw == 8);
    if (!ok) { std::printf("row %d breaks a rule\n", i); return 1; }
    for (int j = 0; j < i; ++j) {
      const WgradPlan& q = kWgradTable.row[j];
      if (q.nw == p.nw && q.wm == p.wm && q.wk == p.wk && q.tm == p.tm && q.tk == p.tk) { std::printf("row %d twice\n", i); return 1; }
    }
  }
  for (int m = 1; m <= 9; ++m)
    for (int k = 1; k <= 9; ++k) {
      const int row = plan_wgrad(m, k);
      if (row < -1 || row >= kWgradRows) { std::printf("%d %d: row %d is outside the launch table\n", m, k, row); return 1; }
      if (row < 0) { std::printf("%d %d none\n", m, k); continue; }
      const WgradPlan& p = kWgradTable.row[row];
      std::printf("%d %d %d %d %d %d %d\n", m, k, p.nw, p.wm, p.wk, p.tm, p.tk);
    }
  return 0;
}
"""


def test_wgrad_plan_is_the_plan_of_the_search_it_replaces(tmp_path):
    """``plan_wgrad`` of csrc/wgrad_plan.h over tiles_m, tiles_k in 1..9: a plan exists exactly where ``PLANS_BEFORE`` has
    one, it is the same five numbers, and it is a row of ``kWgradTable`` (the program indexes the table with the answer).
    ``PLANS_BEFORE`` was generated by compiling, in a host program, the ``plan_wgrad`` that csrc/wgrad.hip had before the
    table existed (its own walk over ``layouts[7][3] x shapes[6][2]``) and printing its 81 answers."""
    got = {}
    for line in _build_and_run(tmp_path, "wgrad_plan_host", PLAN_PROGRAM).splitlines():
        f = line.split()
        got[(int(f[0]), int(f[1]))] = None if f[2] == "none" else tuple(int(v) for v in f[2:])
    want = {(m, k): PLANS_BEFORE[m - 1][k - 1] for m in range(1, 10) for k in range(1, 10)}
    assert got == want


# ---- the shape predicates of the tall-Linear entry points ------------------------------------------------------------
# The "yes" sets the library answered before the predicates read the launchers' value lists, over R in 16..512 step 16 and
# J in 32..512 step 32 (N = 1000), recorded from that library through the same ctypes calls.

SWEEP_R, SWEEP_J = range(16, 513, 16), range(32, 513, 32)
YES_TALLGEMM = {(R, J) for R in (16, 32, 64, 128, 256) for J in (32, 64, 128, 256)} - {(256, 256)}
YES_SHIFT = YES_POST = {(R, J) for R in (64, 128, 256) for J in (64, 128)}
YES_LNBWD = {(R, J) for R in (64, 128, 256) for J in (64, 128, 256)} - {(256, 256)}
YES_DUAL = {(R1, R2, J) for R1, R2 in ((16, 16), (32, 0), (48, 16), (64, 0), (64, 64), (112, 16), (128, 0), (192, 64),
                                      (240, 16), (256, 0)) for J in (32, 64, 128)}
YES_LINEAR_BWD = {(128, 256, 0), (256, 128, 1), (256, 128, 2)}                  # (M, K, epilogue)
# fp32 weight gradient, (M, K) = (R, J) of the sweep: widest K by the number of 32-row tiles of M
YES_WGRAD = {(M, K) for M in SWEEP_R for K in SWEEP_J
             if K <= {1: 512, 2: 512, 3: 256, 4: 256}.get((M + 31) // 32, 128 if M <= 256 else 64)}


def test_shape_predicates_answer_as_before():
    from mlgnn import _lib
    lib, N = _lib.lib, 1000
    grid = [(R, J) for R in SWEEP_R for J in SWEEP_J]
    assert {(R, J) for R, J in grid if lib.mlgnn_tallgemm_supported(N, R, J, 0)} == YES_TALLGEMM
    assert {(R, J) for R, J in grid if lib.mlgnn_tallgemm_nt_shift_supported(N, R, J)} == YES_SHIFT
    assert {(R, J) for R, J in grid if lib.mlgnn_tallgemm_lnin_postln_supported(N, R, J)} == YES_POST
    assert {(R, J) for R, J in grid if lib.mlgnn_tallgemm_lnbwd_supported(N, R, J)} == YES_LNBWD
    assert {(R, R2, J) for R, J in grid for R2 in (0, 16, 64) if lib.mlgnn_tallgemm_dual_supported(N, R, R2, J)} == YES_DUAL
    assert {(R, J, e) for R, J in grid for e in (0, 1, 2) if lib.mlgnn_linear_bwd_supported(N, R, J, e)} == YES_LINEAR_BWD
    assert {(R, J) for R, J in grid if lib.mlgnn_linear_wgrad_workspace_floats(N, R, J, 0) >= 0} == YES_WGRAD
    for name in ("tallgemm_nt_shift", "tallgemm_lnin_postln", "tallgemm_lnbwd"):       # every predicate refuses N = 0
        assert getattr(lib, "mlgnn_%s_supported" % name)(0, 128, 128) == 0
