// The running worst row the reducing sweeps keep per lane and merge across lanes, waves and workgroups (bounds.hip,
// validate.hip).  Device code.
#pragma once
#include <math.h>

#include "common.hpp"

// Running worst row of a sweep; rows are visited in increasing order.
// push only takes nv > v, so a slot with row >= 0 holds a non-NaN v > -inf and an empty one (row < 0) holds -inf:
// merge may test the row alone to tell them apart, and an empty slot never replaces anything.
struct Worst {
  double v;
  int64_t row;
  __device__ inline void init() { v = -INFINITY; row = -1; }
  __device__ inline void push(double nv, int64_t nrow, bool valid) {
    const bool take = valid && nv > v;                 // strict: the lowest row keeps a tie
    v = take ? nv : v;
    row = take ? nrow : row;
  }
  __device__ inline void merge(double ov, int64_t orow) {
    const bool take = orow >= 0 && (row < 0 || ov > v || (ov == v && orow < row));
    v = take ? ov : v;
    row = take ? orow : row;
  }
  __device__ inline void merge_lanes(int width) {      // butterfly over aligned groups of `width` lanes
    for (int o = width >> 1; o > 0; o >>= 1) {
      const double ov = __shfl_xor(v, o, 64);
      const long long orow = __shfl_xor((long long)row, o, 64);
      merge(ov, (int64_t)orow);
    }
  }
};
