// Host side of a launcher: argument checks, grids and dispatch shared by the kernel files.  Include after common.hpp.
// Nothing here is device code; every helper does the arithmetic the launchers used to spell out one by one.
#pragma once
#include "common.hpp"

// compute units the grids are sized for; the only place the fallback for an unknown device is written
inline int spr_cus_or_default() {
  const int cus = spr_cached_cus();
  return cus > 0 ? cus : 256;
}

// ---- feature layout and row-shard plan --------------------------------------------------------------------------------
inline bool spr_layout_ok(int64_t row0, int64_t n_rows, int64_t n_points, int32_t n_features) {
  return n_points > 0 && n_features > 0 && row0 >= 0 && row0 + n_rows <= n_points * (int64_t)n_features;
}
#define SPR_REQUIRE_LAYOUT(name, row0, n_rows, n_points, n_features) \
  SPR_REQUIRE(spr_layout_ok(row0, n_rows, n_points, n_features), SPR_E_INVALID, "%s: bad feature layout", name)

inline SegPlan spr_make_plan(int64_t row0, int64_t n_rows, int64_t n_points, int32_t n_features, int32_t chunk_rows) {
  SegPlan plan;
  plan.row0 = row0; plan.n_rows = n_rows; plan.n_points = n_points; plan.n_features = n_features;
  plan.total_wg = 0; plan.chunk_rows = chunk_rows;
  return plan;
}

// per_cu workgroups per compute unit, each consuming chunk_rows rows per step; returns the grid
inline int spr_plan_grid(SegPlan &plan, int per_cu, int chunk_rows) {
  plan.total_wg = per_cu * spr_cus_or_default();
  plan.chunk_rows = chunk_rows;
  return seg_total_wgs(plan);
}

// ... with the chunk_rows the plan was made with
inline int spr_plan_grid(SegPlan &plan, int per_cu) { return spr_plan_grid(plan, per_cu, plan.chunk_rows); }

// workgroups per CU of the vector-stationary panel kernels (reconstruct, bound sweep, field error, field_std), by LDS: 2 x 64 x (16 mtr + 2) doubles per workgroup of
// the 160 KB -> 6 / 4 / 3 / 2 / 1 / 1 for mtr = 1, 2, 3, 4, 6, 8
// (tests/test_panel_sweep_gpu.py sizes its blocks from a copy of this table: change both)
constexpr int spr_panel_per_cu(int mtr) { return mtr <= 1 ? 6 : mtr == 2 ? 4 : mtr == 3 ? 3 : mtr == 4 ? 2 : 1; }

// a grid whose workgroups each own a slot of the caller's workspace
#define SPR_REQUIRE_GRID(name, grid, max_slots) \
  SPR_REQUIRE((grid) > 0 && (grid) <= (max_slots), SPR_E_INVALID, "%s: grid of %d exceeds the workspace", name, grid)

// ---- 16-byte loads ----------------------------------------------------------------------------------------------------
// rows of `cols` elements with leading dimension `ld` can be read as aligned pairs of T
template <typename T>
inline bool spr_pair_aligned(const T *p, int64_t cols, int64_t ld) {
  return (cols % 2 == 0) && (ld % 2 == 0) && ((reinterpret_cast<uintptr_t>(p) & (2 * sizeof(T) - 1)) == 0);
}

// every row of row_bytes bytes starts on a 16-byte boundary
inline bool spr_rows_aligned16(const void *p, size_t row_bytes) {
  return row_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// load mode of the row-tile kernels: 0 scalar, 1 pairs, 2 pairs with no column tail (r fills its MTR tiles)
inline int spr_load_mode(bool pair_aligned, int r, int mtr) { return pair_aligned ? (r == 16 * mtr ? 2 : 1) : 0; }

// ---- dispatch on a padded tile count --------------------------------------------------------------------------------------
// SPR_DISPATCH_*(sel, name, r, stmt): runs stmt with the compile-time constant RUNG equal to sel, for the widths the kernels
// of the file are instantiated for; any other value is refused as "no kernel".  stmt names RUNG where the rungs used to differ.
#define SPR_RUNG_(N, ...) \
  case N: {               \
    constexpr int RUNG = N; \
    __VA_ARGS__;          \
  } break;
#define SPR_NO_RUNG_(name, r) \
  default: SPR_REQUIRE(false, SPR_E_UNSUPPORTED, "%s: no kernel for the padded width of r = %d", name, (int)(r));

#define SPR_DISPATCH_MT(sel, name, r, ...) /* spr_round_mt up to SPR_MAX_R: 1, 2, 3, 4, 6, 8 */                  \
  switch (sel) {                                                                                                  \
    SPR_RUNG_(1, __VA_ARGS__) SPR_RUNG_(2, __VA_ARGS__) SPR_RUNG_(3, __VA_ARGS__) SPR_RUNG_(4, __VA_ARGS__)       \
    SPR_RUNG_(6, __VA_ARGS__) SPR_RUNG_(8, __VA_ARGS__) SPR_NO_RUNG_(name, r)                                     \
  }
#define SPR_DISPATCH_POW2(sel, name, r, ...) /* en_round_mtr, gp_round_mtr: 1, 2, 4, 8 */                        \
  switch (sel) {                                                                                                  \
    SPR_RUNG_(1, __VA_ARGS__) SPR_RUNG_(2, __VA_ARGS__) SPR_RUNG_(4, __VA_ARGS__) SPR_RUNG_(8, __VA_ARGS__)       \
    SPR_NO_RUNG_(name, r)                                                                                         \
  }
#define SPR_DISPATCH_1TO8(sel, name, r, ...) /* whole 16-column groups: 1 ... 8 */                                \
  switch (sel) {                                                                                                  \
    SPR_RUNG_(1, __VA_ARGS__) SPR_RUNG_(2, __VA_ARGS__) SPR_RUNG_(3, __VA_ARGS__) SPR_RUNG_(4, __VA_ARGS__)       \
    SPR_RUNG_(5, __VA_ARGS__) SPR_RUNG_(6, __VA_ARGS__) SPR_RUNG_(7, __VA_ARGS__) SPR_RUNG_(8, __VA_ARGS__)       \
    SPR_NO_RUNG_(name, r)                                                                                         \
  }

#define SPR_DISPATCH_NT(sel, name, r, ...) /* spr_round_nt: 1, 2, 3, 5, 9 */                                      \
  switch (sel) {                                                                                                  \
    SPR_RUNG_(1, __VA_ARGS__) SPR_RUNG_(2, __VA_ARGS__) SPR_RUNG_(3, __VA_ARGS__) SPR_RUNG_(5, __VA_ARGS__)       \
    SPR_RUNG_(9, __VA_ARGS__) SPR_NO_RUNG_(name, r)                                                               \
  }
// 16-column tiles across the augmented Gram of the dense solvers (solve.hip, assimilate.hip), `cols` columns wide
inline int spr_round_nt(int cols) {
  const int need = (cols + 15) / 16;
  return need <= 3 ? need : need <= 5 ? 5 : need <= 9 ? 9 : -1;
}

// ---- exported entry points ----------------------------------------------------------------------------------------------
// SPR_ENTRY(name, (parameters), (implementation), arguments...): extern "C" int name(parameters), which hands its own name and
// the arguments to the templated implementation.  A file wraps it once per family, with the storage types as parameters.
#define SPR_ENTRY(NAME, PARAMS, IMPL, ...) \
  extern "C" int NAME PARAMS { return IMPL(#NAME, __VA_ARGS__); }
