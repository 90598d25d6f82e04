// One field value  x = X_scl (u . a) + X_cnt  from one basis row held in the accumulator layout of the 16x16 MFMA tiles:
// the 16 lanes li of a group hold the row's columns 16 ct + li, ct = 0 .. NT-1, one double per column tile.
//
// Shared by the field epilogue of the W-stationary projection (project_ws.hip), which has the row in its accumulators, and
// by the stand-alone row-dot kernel (reconstruct.hip), which loads it from HBM: the same operations in the same order,
// so reconstruct(a) returns the same bits whether the projection emitted the field or the basis was read again.
#pragma once
#include "common.hpp"

// coefficient vectors one launch serves (the NF the kernels are built for)
constexpr int SPR_FIELD_NF = 1;

// v[ct]: the row's entries AS STORED (rounded to the storage type of the basis first), a[ct]: entry 16 ct + li of the
// coefficient vector (0 past r).  Per lane one fused multiply-add per column tile in ascending order, then the butterfly
// over the 16 lanes of the row (every lane ends with the same bits), then one fused multiply-add for scale and centre.
// Trailing tiles of zeros leave the sum as it is (it starts at +0 and can never become -0), so callers built for different
// NT agree on a row they both hold.  All 64 lanes must be active (DPP moves).
template <int NT>
__device__ inline double field_row_value(const double (&v)[NT], const double (&a)[NT], double scale, double mean) {
  double d = 0.0;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) d = fma(v[ct], a[ct], d);
  return fma(scale, group_sum_t<16>(d), mean);
}

// Four rows of one lane group at once (the four accumulator registers of the MFMA tiles): the value of row
// group_sum4_slot(li), li the lane's index in its group, so lanes 0..3 hold rows 0..3.  The per-lane sums and the last
// fused multiply-add are those of field_row_value and the butterfly adds the same pairs (group_sum4_t): the same bits.
template <int NT>
__device__ inline double field_row4_value(const double (&v)[4][NT], const double (&a)[NT], double scale, double mean0,
                                          double mean1, double mean2, double mean3, int li) {
  double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    d0 = fma(v[0][ct], a[ct], d0); d1 = fma(v[1][ct], a[ct], d1);
    d2 = fma(v[2][ct], a[ct], d2); d3 = fma(v[3][ct], a[ct], d3);
  }
  const int slot = group_sum4_slot(li);
  const double mu_lo = (slot & 1) ? mean1 : mean0, mu_hi = (slot & 1) ? mean3 : mean2;
  return fma(scale, group_sum4_t(d0, d1, d2, d3, li), (slot & 2) ? mu_hi : mu_lo);
}
