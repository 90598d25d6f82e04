// Exact Gaussian processes on the POD coefficients: GPR.train / GPR.predict / GPR.update (openmeasure_amd/gpr.py).
//
// Model, per retained mode (r independent GPs over the same m scaled parameter points, reference gpr.py:485-509):
//   raw = (raw_l, raw_n, mu);  l = softplus(raw_l),  s2 = softplus(raw_n) + 1e-4,  K = k(D / l) + s2 I,
//   D the Euclidean distance matrix of P0 clamped below at 1e-15,  res = y - mu,  alpha = K^-1 res,
//   loss = [ res^T alpha / 2 + log det K / 2 + (m / 2) log 2 pi ] / m            (the exact marginal likelihood, negated, per datum)
//   W = K^-1 - alpha alpha^T:   d loss / d raw_l = sigmoid(raw_l) sum_ij W_ij dK_ij/dl / 2m,
//   d loss / d raw_n = sigmoid(raw_n) tr W / 2m,   d loss / d mu = -sum alpha / m.
// Adam (beta = 0.9, 0.999, eps = 1e-8, bias correction) with the reference's loop (:230-247): evaluate, e = |loss - loss_old|,
// step, stop when e <= tol or after max_iter evaluations (the step of the stopping evaluation is taken).
//
// gp_train_kernel: ONE WORKGROUP PER MODE, the whole loop in one launch; no atomics, no communication between workgroups.
// An evaluation, all in the mode's slice of the workspace (two m x m matrices, L2-resident) and the K^-1 output:
//   1. K (upper triangle) from D.
//   2. K = R^T R, R upper triangular and row-major (R[k][i] = L[i][k]): left-looking by block rows of GP_NB.  The correction
//      of a block row is a panel product with one thread per column -- GP_NB accumulators in registers, the finished rows it
//      multiplies with staged through LDS in chunks of GP_KC, every global read coalesced (gp_panel_acc); the diagonal block
//      is factored in LDS; the rest of the block row is a forward substitution per column in registers (gp_fwd).
//   3. X = L^-1 by block rows: the same panel product (finished rows of X against the block's columns of R), then gp_fwd.
//      The strict upper triangle of X is stored as zeros, so the products below need no triangular bounds per thread.
//   4. K^-1 = X^T X by block rows of the lower triangle, mirrored: the same panel product a third time.  Both halves of a
//      diagonal block add the same products in the same order: K^-1 is symmetric bit for bit.
//   5. alpha = K^-1 res (one thread per row, fixed order), the five sums (res.alpha, sum alpha, tr K^-1, alpha.alpha,
//      sum W o dK/dl over the upper triangle, doubled) per thread in a fixed assignment, closed with a butterfly and four LDS words in a fixed order.
// m^3 flops per evaluation (a third each for 2, 3, 4) on the vector pipe.
// Control flow: every loop bound is an argument or derived from m; every decision that changes it is taken on a value all
// threads read from the same LDS word behind a barrier -- a pivot (<= 0 or not finite: status 1 / 2, the mode stops), the sums
// that give the loss, and the stop flag thread 0 publishes -- so no barrier is ever reached by part of a workgroup.
// Two runs agree bit for bit.
//
// gp_predict_kernel: one workgroup per (mode, GP_PB test points): k* into LDS, K^-1 read once for the block of points
// (coalesced by symmetry), mean = mu + k*.alpha, var = max(k(0) - k*^T K^-1 k*, 0) + s2, k(0) = 1 for the four kernels.
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

__device__ inline double gp_softplus(double x) { return x > 0.0 ? x + log1p(exp(-x)) : log1p(exp(x)); }
__device__ inline double gp_sigmoid(double x) {
  if (x >= 0.0) return 1.0 / (1.0 + exp(-x));
  const double e = exp(x);
  return e / (1.0 + e);
}

// k(t) and l dK/dl at t = D / l
__device__ inline void gp_kern(int code, double t, double &k, double &dk) {
  if (code == SPR_GP_MATERN52) {
    const double s = sqrt(5.0) * t, e = exp(-s), t2 = t * t;
    k = (1.0 + s + (5.0 / 3.0) * t2) * e;
    dk = (5.0 / 3.0) * t2 * (1.0 + s) * e;
  } else if (code == SPR_GP_MATERN32) {
    const double s = sqrt(3.0) * t, e = exp(-s);
    k = (1.0 + s) * e;
    dk = s * s * e;
  } else if (code == SPR_GP_MATERN12) {
    const double e = exp(-t);
    k = e;
    dk = t * e;
  } else {
    const double t2 = t * t, e = exp(-0.5 * t2);
    k = e;
    dk = t2 * e;
  }
}

__device__ inline double gp_dist(const double *a, const double *b, int d) {
  double s = 0.0;
  for (int c = 0; c < d; ++c) {
    const double v = a[c] - b[c];
    s = fma(v, v, s);
  }
  s = sqrt(s);
  return s > 1e-15 ? s : 1e-15;     // (a NaN coordinate is refused on the host)
}

__global__ __launch_bounds__(GP_T) void gp_dist_kernel(const double *__restrict__ P, int m, int d, int64_t ldp,
                                                       double *__restrict__ D) {
  const int idx = blockIdx.x * GP_T + threadIdx.x;
  if (idx >= m * m) return;
  const int i = idx / m, j = idx - i * m;
  D[idx] = gp_dist(P + (int64_t)i * ldp, P + (int64_t)j * ldp, d);
}

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

struct GpShared {
  double S[GP_KC * GP_NB];
  double Ld[GP_NB * GP_LDP];
  double res[GP_MAX_M];
  double al[GP_MAX_M];
  double red[4 * 5];
  int stop;
};

// One evaluation at (raw_l, raw_n, mu): K^-1 and alpha to their outputs, loss and gradient returned.  -> 0, or the status
// of a failed pivot (the same in every thread).
__device__ int gp_evaluate(int code, int m, const double *__restrict__ D, const double *__restrict__ y, int64_t ldy,
                           double raw_l, double raw_n, double mu, double *A, double *X, double *Kinv, double *alpha,
                           GpShared &sh, double &loss, double (&grad)[3]) {
  const int tid = threadIdx.x;
  const double ell = gp_softplus(raw_l), sig2 = gp_softplus(raw_n) + 1e-4;

  // 1. K, upper triangle
  for (int idx = tid; idx < m * m; idx += GP_T) {
    const int k = idx / m, i = idx - k * m;
    if (i >= k) {
      double kv, dk;
      gp_kern(code, D[idx] / ell, kv, dk);
      A[idx] = i == k ? kv + sig2 : kv;
    }
  }
  __syncthreads();

  // 2. K = R^T R
  double logdet = 0.0;
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
  for (int i = tid; i < m; i += GP_T) sh.res[i] = y[(int64_t)i * ldy] - mu;
  __syncthreads();

  // 5. alpha and the sums
  double part[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < m; i += GP_T) {
    double a = 0.0;
    for (int j = 0; j < m; ++j) a = fma(Kinv[j * m + i], sh.res[j], a);
    sh.al[i] = a;
    alpha[i] = a;
    part[0] += sh.res[i] * a;
    part[1] += a;
    part[2] += Kinv[i * m + i];
    part[3] += a * a;
  }
  __syncthreads();
  for (int idx = tid; idx < m * m; idx += GP_T) {          // W o dK/dl is symmetric: the upper triangle, doubled
    const int k = idx / m, i = idx - k * m;
    if (i >= k) {
      double kv, dk;
      gp_kern(code, D[idx] / ell, kv, dk);
      const double w = (Kinv[idx] - sh.al[k] * sh.al[i]) * dk;
      part[4] += i == k ? w : 2.0 * w;
    }
  }
  gp_block_sum<5>(part, sh.red);
  const double dm = (double)m;
  loss = (0.5 * part[0] + 0.5 * logdet + 0.5 * dm * log(2.0 * M_PI)) / dm;
  grad[0] = gp_sigmoid(raw_l) * (part[4] / ell) / (2.0 * dm);
  grad[1] = gp_sigmoid(raw_n) * (part[2] - part[3]) / (2.0 * dm);
  grad[2] = -part[1] / dm;
  return 0;
}

__global__ __launch_bounds__(GP_T) void gp_train_kernel(const double *__restrict__ D, const double *__restrict__ Y,
                                                        int64_t ldy, int m, int code, double *raw, double lr, int max_iter,
                                                        double tol, double *Kinv_all, double *alpha_all, double *info,
                                                        double *trace, double *ws) {
  __shared__ GpShared sh;
  const int q = blockIdx.x, tid = threadIdx.x;
  const size_t mm = (size_t)m * m;
  double *A = ws + 2 * mm * q, *X = A + mm;
  double *Kinv = Kinv_all + mm * q, *alpha = alpha_all + (size_t)m * q;
  double p[3] = {raw[3 * q], raw[3 * q + 1], raw[3 * q + 2]};
  double m1[3] = {0.0, 0.0, 0.0}, m2[3] = {0.0, 0.0, 0.0}, b1t = 1.0, b2t = 1.0;
  double loss_old = 1e10, loss = 0.0, e = 1e10, grad[3] = {0.0, 0.0, 0.0};
  double rec[8] = {0.0, NAN, NAN, 0.0, NAN, NAN, NAN, 0.0};   // evaluations, loss, e, status, gradient
  int evals = 0, status = 0;
  bool last = max_iter == 0;
  for (int it = 0; it <= max_iter; ++it) {                   // max_iter evaluations with a step, one at the parameters kept
    status = gp_evaluate(code, m, D, Y + q, ldy, p[0], p[1], p[2], A, X, Kinv, alpha, sh, loss, grad);
    if (status != 0) break;
    if (last) {
      if (max_iter == 0) { rec[1] = loss; rec[4] = grad[0]; rec[5] = grad[1]; rec[6] = grad[2]; }
      break;
    }
    e = fabs(loss - loss_old);
    loss_old = loss;
    if (trace != nullptr && tid == 0) {
      double *tr = trace + ((size_t)q * max_iter + it) * 4;
      tr[0] = loss; tr[1] = p[0]; tr[2] = p[1]; tr[3] = p[2];
    }
    b1t *= 0.9;
    b2t *= 0.999;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      m1[c] = 0.9 * m1[c] + (1.0 - 0.9) * grad[c];
      m2[c] = 0.999 * m2[c] + (1.0 - 0.999) * grad[c] * grad[c];
      const double denom = sqrt(m2[c]) / sqrt(1.0 - b2t) + 1e-8;
      p[c] -= (lr / (1.0 - b1t)) * (m1[c] / denom);
    }
    ++evals;
    rec[0] = evals; rec[1] = loss; rec[2] = e; rec[4] = grad[0]; rec[5] = grad[1]; rec[6] = grad[2];
    if (tid == 0) sh.stop = (e <= tol || evals >= max_iter) ? 1 : 0;
    __syncthreads();
    last = sh.stop != 0;                                     // one LDS word decides for the whole workgroup
    __syncthreads();
  }
  rec[3] = status;
  if (tid == 0) {
    for (int c = 0; c < 8; ++c) info[8 * q + c] = rec[c];
    for (int c = 0; c < 3; ++c) raw[3 * q + c] = p[c];
  }
}

__global__ __launch_bounds__(GP_T) void gp_predict_kernel(const double *__restrict__ P0, int m, int d, int64_t ldp,
                                                          const double *__restrict__ Ps, int np, int64_t lds_, int code,
                                                          const double *__restrict__ raw, const double *__restrict__ Kinv_all,
                                                          const double *__restrict__ alpha_all, double *__restrict__ mean,
                                                          double *__restrict__ var, int r) {
  __shared__ double ks[GP_PB * GP_MAX_M];
  __shared__ double red[4 * 2 * GP_PB];
  const int q = blockIdx.x, p0 = blockIdx.y * GP_PB, tid = threadIdx.x;
  const int npb = np - p0 < GP_PB ? np - p0 : GP_PB;
  const double ell = gp_softplus(raw[3 * q]), sig2 = gp_softplus(raw[3 * q + 1]) + 1e-4, mu = raw[3 * q + 2];
  const double *Kinv = Kinv_all + (size_t)m * m * q, *alpha = alpha_all + (size_t)m * q;
  for (int e = tid; e < GP_PB * m; e += GP_T) {
    const int pp = e / m, i = e - pp * m;
    double kv = 0.0, dk;
    if (pp < npb) gp_kern(code, gp_dist(P0 + (int64_t)i * ldp, Ps + (int64_t)(p0 + pp) * lds_, d) / ell, kv, dk);
    ks[e] = kv;
  }
  __syncthreads();
  double part[2 * GP_PB];
#pragma unroll
  for (int c = 0; c < 2 * GP_PB; ++c) part[c] = 0.0;
  for (int i = tid; i < m; i += GP_T) {
    double acc[GP_PB];
#pragma unroll
    for (int pp = 0; pp < GP_PB; ++pp) acc[pp] = 0.0;
    for (int j = 0; j < m; ++j) {
      const double kij = Kinv[j * m + i];                  // = K^-1[i][j]: symmetric, read along the row for coalescing
#pragma unroll
      for (int pp = 0; pp < GP_PB; ++pp) acc[pp] = fma(kij, ks[pp * m + j], acc[pp]);
    }
    const double a = alpha[i];
#pragma unroll
    for (int pp = 0; pp < GP_PB; ++pp) {
      const double kv = ks[pp * m + i];
      part[pp] = fma(kv, a, part[pp]);
      part[GP_PB + pp] = fma(kv, acc[pp], part[GP_PB + pp]);
    }
  }
  gp_block_sum<2 * GP_PB>(part, red);
  if (tid == 0) {
#pragma unroll
    for (int pp = 0; pp < GP_PB; ++pp)
      if (pp < npb) {
        const double v = 1.0 - part[GP_PB + pp];
        mean[(int64_t)(p0 + pp) * r + q] = mu + part[pp];
        var[(int64_t)(p0 + pp) * r + q] = (v > 0.0 ? v : 0.0) + sig2;
      }
  }
}

// ------------------------------------------------------------------------------------------------ host side
size_t gp_workspace(int32_t m, int32_t r) {
  if (m < 1 || m > GP_MAX_M || r < 1) return 0;
  return sizeof(double) * (size_t)m * m * (1 + 2 * (size_t)r);
}

int gp_train(const char *name, const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r,
             int64_t ldy, int32_t kernel, double *d_raw, double lr, int32_t max_iter, double tol, double *d_Kinv,
             double *d_alpha, double *d_info, double *d_trace, void *d_workspace, size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_P0 && d_Y && d_raw && d_Kinv && d_alpha && d_info && d_workspace, SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(m > 0 && d > 0 && r > 0 && ldp >= d && ldy >= r && max_iter >= 0, SPR_E_INVALID,
              "%s: bad shape m=%d d=%d ldp=%lld r=%d ldy=%lld max_iter=%d", name, m, d, (long long)ldp, r, (long long)ldy,
              max_iter);
  SPR_REQUIRE(kernel >= SPR_GP_MATERN52 && kernel <= SPR_GP_RBF, SPR_E_INVALID, "%s: unknown kernel code %d", name, kernel);
  SPR_REQUIRE(lr > 0.0 && lr <= DBL_MAX && tol >= 0.0 && tol <= DBL_MAX, SPR_E_INVALID,
              "%s: lr = %g must be positive and tol = %g non-negative, both finite", name, lr, tol);
  SPR_REQUIRE(m <= GP_MAX_M, SPR_E_UNSUPPORTED, "%s: m = %d exceeds %d", name, m, GP_MAX_M);
  SPR_REQUIRE(workspace_bytes >= gp_workspace(m, r), SPR_E_INVALID, "%s: workspace of %zu bytes, %zu needed", name,
              workspace_bytes, gp_workspace(m, r));
  SPR_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, SPR_E_INVALID, "%s: workspace must be 8-byte aligned", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *D = static_cast<double *>(d_workspace);
  hipLaunchKernelGGL(gp_dist_kernel, dim3((m * m + GP_T - 1) / GP_T), dim3(GP_T), 0, st, d_P0, (int)m, (int)d, ldp, D);
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gp_train_kernel, dim3(r), dim3(GP_T), 0, st, D, d_Y, ldy, (int)m, (int)kernel, d_raw, lr, (int)max_iter,
                     tol, d_Kinv, d_alpha, d_info, d_trace, D + (size_t)m * m);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

int gp_predict(const char *name, const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Pstar, int32_t n_p,
               int64_t ldps, int32_t kernel, const double *d_raw, int32_t r, const double *d_Kinv, const double *d_alpha,
               double *d_mean, double *d_var, void *stream) {
  SPR_REQUIRE(d_P0 && d_Pstar && d_raw && d_Kinv && d_alpha && d_mean && d_var, SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(m > 0 && d > 0 && r > 0 && n_p > 0 && ldp >= d && ldps >= d, SPR_E_INVALID,
              "%s: bad shape m=%d d=%d ldp=%lld n_p=%d ldps=%lld r=%d", name, m, d, (long long)ldp, n_p, (long long)ldps, r);
  SPR_REQUIRE(kernel >= SPR_GP_MATERN52 && kernel <= SPR_GP_RBF, SPR_E_INVALID, "%s: unknown kernel code %d", name, kernel);
  SPR_REQUIRE(m <= GP_MAX_M, SPR_E_UNSUPPORTED, "%s: m = %d exceeds %d", name, m, GP_MAX_M);
  const int nblk = (n_p + GP_PB - 1) / GP_PB;
  SPR_REQUIRE(nblk <= 65535, SPR_E_UNSUPPORTED, "%s: n_p = %d exceeds %d test points per call", name, n_p, 65535 * GP_PB);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(gp_predict_kernel, dim3(r, nblk), dim3(GP_T), 0, st, d_P0, (int)m, (int)d, ldp, d_Pstar, (int)n_p, ldps,
                     (int)kernel, d_raw, d_Kinv, d_alpha, d_mean, d_var, (int)r);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

}  // namespace

extern "C" size_t spr_gp_workspace(int32_t m, int32_t r) { return gp_workspace(m, r); }

SPR_ENTRY(spr_gp_train_f64,
          (const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy, int32_t kernel,
           double *d_raw, double lr, int32_t max_iter, double tol, double *d_Kinv, double *d_alpha, double *d_info,
           double *d_trace, void *d_workspace, size_t workspace_bytes, void *stream),
          gp_train, d_P0, m, d, ldp, d_Y, r, ldy, kernel, d_raw, lr, max_iter, tol, d_Kinv, d_alpha, d_info, d_trace,
          d_workspace, workspace_bytes, stream)

SPR_ENTRY(spr_gp_predict_f64,
          (const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Pstar, int32_t n_p, int64_t ldps,
           int32_t kernel, const double *d_raw, int32_t r, const double *d_Kinv, const double *d_alpha, double *d_mean,
           double *d_var, void *stream),
          gp_predict, d_P0, m, d, ldp, d_Pstar, n_p, ldps, kernel, d_raw, r, d_Kinv, d_alpha, d_mean, d_var, stream)
