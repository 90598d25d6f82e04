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
