// Device code shared by the one-workgroup-per-model training kernels (gp.hip, cokriging.hip): the fixed-order workgroup sums,
// the panel product, and steps 2-4 of an evaluation (factor, triangular inverse, K^-1).  Include after launch.hpp.
#pragma once
#include <float.h>
#include <math.h>

#include "launch.hpp"

namespace {

constexpr int GP_T = 256;
constexpr int GP_NB = 16;             // block rows / accumulators per thread
constexpr int GP_KC = 32;             // contraction rows per LDS chunk
constexpr int GP_LDP = GP_NB + 1;     // row stride of the diagonal block in LDS
constexpr int GP_PB = 8;              // test points per workgroup of the predict kernel
constexpr int GP_MAX_M = SPR_GP_MAX_M;

// Sums of N values over the workgroup: butterfly inside a wave, the four waves through LDS in a fixed order.  Every thread
// returns with the same bits, read from the same LDS words.
template <int N>
__device__ inline void gp_block_sum(double (&v)[N], double *red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = group_sum_t<64>(v[n]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) red[wave * N + n] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = ((red[n] + red[N + n]) + red[2 * N + n]) + red[3 * N + n];
}

// acc[j] += sum_{k0 <= k < k1} M1[k][col] M2[k][c0 + j],  j < GP_NB, both matrices m x m row-major.  k0, k1, c0 are the same
// for the whole workgroup (barriers inside); cv: this thread has a column.  M2's rows go through LDS in chunks of GP_KC,
// columns past m as zeros.
__device__ inline void gp_panel_acc(const double *M1, const double *M2, int m, int k0, int k1, int col, bool cv, int c0,
                                    double *S, double (&acc)[GP_NB]) {
  for (int kc = k0; kc < k1; kc += GP_KC) {
    __syncthreads();               // the previous chunk is consumed; what other threads wrote to M1 / M2 is visible
    for (int e = threadIdx.x; e < GP_KC * GP_NB; e += GP_T) {
      const int k = kc + e / GP_NB, c = c0 + e % GP_NB;
      S[e] = (k < k1 && c < m) ? M2[k * m + c] : 0.0;
    }
    __syncthreads();
    if (cv) {
      const int kn = k1 - kc < GP_KC ? k1 - kc : GP_KC;
      for (int kk = 0; kk < kn; ++kk) {
        const double v = M1[(kc + kk) * m + col];
#pragma unroll
        for (int j = 0; j < GP_NB; ++j) acc[j] = fma(v, S[kk * GP_NB + j], acc[j]);
      }
    }
  }
}

// the diagonal block of R at (c0, c0) into LDS, padded to GP_NB with the identity
__device__ inline void gp_load_diag(const double *A, int m, int c0, int nb, double *Ld) {
  for (int e = threadIdx.x; e < GP_NB * GP_NB; e += GP_T) {
    const int a = e / GP_NB, b = e % GP_NB;
    Ld[a * GP_LDP + b] = (a <= b && b < nb) ? A[(c0 + a) * m + c0 + b] : (a == b ? 1.0 : 0.0);
  }
}

// x <- U^-T x for the upper triangular block in LDS (forward substitution, in registers)
__device__ inline void gp_fwd(const double *Ld, double (&x)[GP_NB]) {
#pragma unroll
  for (int j = 0; j < GP_NB; ++j) {
    double s = x[j];
#pragma unroll
    for (int k = 0; k < j; ++k) s = fma(-Ld[k * GP_LDP + j], x[k], s);
    x[j] = s / Ld[j * GP_LDP + j];
  }
}

template <int NSUM>
struct GpSharedT {
  double S[GP_KC * GP_NB];
  double Ld[GP_NB * GP_LDP];
  double res[GP_MAX_M];
  double al[GP_MAX_M];
  double red[4 * NSUM];
  int stop;
};
using GpShared = GpSharedT<5>;

// Steps 2-4 of an evaluation, shared by both training kernels: K (upper triangle of A) -> R in A, X = L^-1, K^-1 = X^T X, and
// log det K.  -> 0, or the status of a failed pivot (the same in every thread).
template <class Sh>
__device__ inline int gp_factor_invert(int m, double *A, double *X, double *Kinv, Sh &sh, double &logdet) {
  const int tid = threadIdx.x;

  // 2. K = R^T R
  logdet = 0.0;
  for (int cb = 0; cb < m; cb += GP_NB) {
    const int nb = m - cb < GP_NB ? m - cb : GP_NB;
    const int ng = (m - cb + GP_T - 1) / GP_T;
    for (int g = 0; g < ng && cb > 0; ++g) {
      const int i = cb + g * GP_T + tid;
      const bool cv = i < m;
      double acc[GP_NB];
#pragma unroll
      for (int j = 0; j < GP_NB; ++j) acc[j] = 0.0;
      gp_panel_acc(A, A, m, 0, cb, i, cv, cb, sh.S, acc);
      if (cv) {
#pragma unroll
        for (int j = 0; j < GP_NB; ++j)
          if (j < nb && cb + j <= i) A[(cb + j) * m + i] -= acc[j];
      }
    }
    __syncthreads();
    gp_load_diag(A, m, cb, nb, sh.Ld);
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      const double p = sh.Ld[j * GP_LDP + j];            // the same LDS word in every thread
      if (!(p > 0.0)) return p != p ? 2 : 1;
      if (!(p <= DBL_MAX)) return 2;
      const double s = sqrt(p);
      logdet += log(p);
      if (tid > j && tid < nb) sh.Ld[j * GP_LDP + tid] /= s;
      __syncthreads();
      for (int e = tid; e < GP_NB * GP_NB; e += GP_T) {
        const int a = e / GP_NB, b = e % GP_NB;
        if (a > j && b >= a && b < nb) sh.Ld[a * GP_LDP + b] -= sh.Ld[j * GP_LDP + a] * sh.Ld[j * GP_LDP + b];
      }
      if (tid == 0) sh.Ld[j * GP_LDP + j] = s;
      __syncthreads();
    }
    for (int e = tid; e < GP_NB * GP_NB; e += GP_T) {
      const int a = e / GP_NB, b = e % GP_NB;
      if (a <= b && b < nb) A[(cb + a) * m + cb + b] = sh.Ld[a * GP_LDP + b];
    }
    for (int i = cb + nb + tid; i < m; i += GP_T) {       // the block row right of the diagonal block
      double x[GP_NB];
#pragma unroll
      for (int j = 0; j < GP_NB; ++j) x[j] = j < nb ? A[(cb + j) * m + i] : 0.0;
      gp_fwd(sh.Ld, x);
#pragma unroll
      for (int j = 0; j < GP_NB; ++j)
        if (j < nb) A[(cb + j) * m + i] = x[j];
    }
    __syncthreads();
  }

  // 3. X = L^-1 = R^-T, lower triangular, zeros above the diagonal
  const int ngm = (m + GP_T - 1) / GP_T;
  for (int rb = 0; rb < m; rb += GP_NB) {
    const int nb = m - rb < GP_NB ? m - rb : GP_NB;
    gp_load_diag(A, m, rb, nb, sh.Ld);
    __syncthreads();
    for (int g = 0; g < ngm; ++g) {
      const int c = g * GP_T + tid;
      const bool cv = c < rb + nb;
      double x[GP_NB];
#pragma unroll
      for (int j = 0; j < GP_NB; ++j) x[j] = 0.0;
      gp_panel_acc(X, A, m, g * GP_T, rb, c, cv, rb, sh.S, x);   // rows of X above the block; zeros where k < c
      if (c < m) {
        if (cv) {
#pragma unroll
          for (int j = 0; j < GP_NB; ++j) x[j] = (c == rb + j ? 1.0 : 0.0) - x[j];
          gp_fwd(sh.Ld, x);
        }
#pragma unroll
        for (int j = 0; j < GP_NB; ++j)
          if (j < nb) X[(rb + j) * m + c] = cv ? x[j] : 0.0;
      }
    }
    __syncthreads();
  }

  // 4. K^-1 = X^T X
  for (int ab = 0; ab < m; ab += GP_NB) {
    const int nb = m - ab < GP_NB ? m - ab : GP_NB;
    const int ng = (m - ab + GP_T - 1) / GP_T;
    for (int g = 0; g < ng; ++g) {
      const int b = ab + g * GP_T + tid;
      const bool cv = b < m;
      double acc[GP_NB];
#pragma unroll
      for (int j = 0; j < GP_NB; ++j) acc[j] = 0.0;
      gp_panel_acc(X, X, m, ab + g * GP_T, m, b, cv, ab, sh.S, acc);
      if (cv) {
#pragma unroll
        for (int j = 0; j < GP_NB; ++j)
          if (j < nb) {
            Kinv[(ab + j) * m + b] = acc[j];
            Kinv[b * m + ab + j] = acc[j];
          }
      }
    }
  }
  return 0;
}

}  // namespace
