"""csrc/dispatch.h on the host: ``dispatch_int`` reaches the listed constant exactly once and nothing else, ``aligned``
accepts null and multiples of the alignment only.  A small C++17 program with its own ``main`` is compiled with the clang of
the ROCm toolchain (host only, no HIP) and run; it needs no GPU."""
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


def test_dispatch_int_and_aligned(tmp_path):
    import build_native
    src, exe = tmp_path / "dispatch_host.cpp", tmp_path / "dispatch_host"
    src.write_text(PROGRAM)
    cmd = [host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + build_native.CSRC, str(src), "-o", str(exe)]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert ran.returncode == 0 and "dispatch ok" in ran.stdout, ran.stdout
