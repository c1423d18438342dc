// Which instantiation of linear_wgrad_kernel (csrc/wgrad.hip) covers an output of tiles_m x tiles_k 32x32 tiles.
// No HIP types: a plain C++17 program can include this file (tests/test_dispatch_host.py does).
#pragma once

namespace mlgnn {

constexpr int kTile = 32;

// NW waves per workgroup laid out WM x WK over the output, TM x TK tiles per wave
struct WgradPlan { int nw, wm, wk, tm, tk; };

// Stage = 32 rows when the operand tiles fit the LDS budget (64 KB single buffered, 144 KB double buffered),
// 16 rows for the widest layouts.  W = padded width of both operands, db = double buffered (the 8-wave kernels).
constexpr int stage_rows(int W, bool db) { return db ? (W <= 384 ? 32 : 16) : (W <= 320 ? 32 : 16); }
constexpr bool lds_fits(int W, bool db) { return (db ? 12 : 6) * stage_rows(W, db) * W <= 160 * 1024; }

constexpr int kWgradLayouts[7][3] = {{4, 2, 2}, {4, 4, 1}, {4, 1, 4}, {8, 4, 2}, {8, 2, 4}, {8, 8, 1}, {8, 1, 8}};
constexpr int kWgradShapes[6][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {1, 4}, {4, 1}};      // <= 4 tiles: 64 accumulator registers

// a (layout, shape) pair is instantiated when its operand tiles fit the LDS; 8 waves (double buffered, one workgroup
// per CU) only at 4 tiles per wave, i.e. only where 4 waves run out of registers
constexpr bool wgrad_row_valid(int layout, int shape) {
  const int nw = kWgradLayouts[layout][0], tm = kWgradShapes[shape][0], tk = kWgradShapes[shape][1];
  if (nw == 8 && tm * tk != 4) return false;
  return lds_fits((kWgradLayouts[layout][1] * tm + kWgradLayouts[layout][2] * tk) * kTile, nw == 8);
}
constexpr int wgrad_count_rows() {
  int n = 0;
  for (int l = 0; l < 7; ++l)
    for (int s = 0; s < 6; ++s) n += wgrad_row_valid(l, s);
  return n;
}
constexpr int kWgradRows = wgrad_count_rows();

// The launch table: every valid pair, layout-major.  plan_wgrad picks a row of it, launch_wgrad instantiates from it.
struct WgradTable { WgradPlan row[kWgradRows]; };
constexpr WgradTable wgrad_make_table() {
  WgradTable t{};
  int n = 0;
  for (int l = 0; l < 7; ++l)
    for (int s = 0; s < 6; ++s)
      if (wgrad_row_valid(l, s))
        t.row[n++] = {kWgradLayouts[l][0], kWgradLayouts[l][1], kWgradLayouts[l][2], kWgradShapes[s][0], kWgradShapes[s][1]};
  return t;
}
constexpr WgradTable kWgradTable = wgrad_make_table();

// Row of the cheapest plan that covers tiles_m x tiles_k, or -1: 4 waves up to 16 tiles, 8 waves up to 32.  Cost =
// padded MFMA work, then operand loads per wave, then the smaller workgroup; ties go to the earlier row.
constexpr int plan_wgrad(int tiles_m, int tiles_k) {
  int best = 1 << 30, row = -1;
  for (int i = 0; i < kWgradRows; ++i) {
    const WgradPlan& p = kWgradTable.row[i];
    if (p.wm * p.tm < tiles_m || p.wk * p.tk < tiles_k) continue;
    const int cost = ((p.wm * p.tm) * (p.wk * p.tk) * 16 + (p.tm + p.tk)) * 2 + (p.nw == 8);
    if (cost < best) { best = cost; row = i; }
  }
  return row;
}

}  // namespace mlgnn
