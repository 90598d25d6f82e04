// Universal kriging with a regression trend, the level model of CoKriging (openmeasure_amd/cokriging.py).
//
// Model, per latent dimension (r independent models over the same n points X, n x d, d <= SPR_GP_MAX_D):
//   v_c = log10 theta_c,  u_c = x_ic - x_jc,  s_ij = sum_c (theta_c u_c) u_c (fma in index order: the difference is taken BEFORE the
//   scaling, so s carries a relative error only, however far the points lie from the origin),
//   R = exp(-s) + nugget I,  trend F (n x P) = [rho,] 1 [, X]  (rho: a given column, the lower level's data; P <= SPR_CK_MAX_P),
//   G = F^T R^-1 F,  beta = G^-1 F^T R^-1 y,  gamma = R^-1 (y - F beta),  sigma2 = (y - F beta)^T gamma / (n - P),
//   loss = [ (n - P) log sigma2 + log det R ] / n            (the concentrated likelihood: beta and sigma2 profiled out)
//   W = R^-1 - gamma gamma^T / sigma2:   d loss / d v_c = ln10 sum_ij W_ij (-theta_c u_c^2 exp(-s_ij)) / n.
// Adam on v with the loop and the stopping rule of gp_train_kernel (gp.hip), v clipped to [v_lo, v_hi] after every step.
//
// ck_train_kernel: ONE WORKGROUP PER MODEL, the whole loop in one launch; no atomics, no communication between workgroups.
// Once per launch: Z = X coordinate-major (d x n), so that the pair loops read coordinates coalesced.
// An evaluation, in the model's slice of the workspace (A, X: n x n; Z) and its outputs:
//   1. theta = 10^v in every thread.           2. R (upper triangle of A) from Z and theta.
//   3. gp_factor_invert (gp_core.hpp): R = U^T U, L^-1, R^-1 = L^-T L^-1, log det R, the pivot status.
//   4. R^-1 F: one thread per row, P accumulators in registers, the rows of F staged through LDS in chunks of GP_KC
//      (R^-1 is symmetric bit for bit: read along its rows, coalesced).
//   5. G and F^T R^-1 y row by row of G: P + 1 fixed-order workgroup sums (gp_block_sum) per row.
//   6. thread 0, in LDS: G = L L^T, beta by two triangular solves, G^-1 = L^-T L^-1.
//   7. res = y - F beta, gamma = R^-1 res (one thread per row, fixed order), sigma2 by one workgroup sum.
//   8. the triangle pass: exp(-s) and u_c recomputed from Z, d sums over the upper triangle doubled, one workgroup sum.
//   9. thread 0: Adam's step, the clip, the record, the stop word.
// n^3 flops per evaluation in step 3, about (2P + 2d + 8) n^2 in the others.
// Control flow: every loop bound is an argument or derived from n; every decision that changes it is taken on a value all
// threads read from the same LDS word behind a barrier -- a pivot of R (status 1 / 2), a pivot of G (status 3), a sigma2 that is
// not positive and finite (status 4), the stop flag -- so no barrier is ever reached by part of a workgroup, and the model
// stops at the first status.  Two runs agree bit for bit.
//
// ck_predict_kernel: one workgroup per (model, GP_PB test points): r* into LDS, R^-1 read once for the block of points,
//   mean = f*^T beta + r*^T gamma,  u = F^T R^-1 r* - f*,  mse = max(sigma2 (1 - r*^T R^-1 r* + u^T G^-1 u), 0);
// f* = [rho*,] 1 [, x*], rho* a given column (the lower level's mean).  s* is formed as training forms s: a test point equal to a
// training point is at s = 0 exactly.
#include <float.h>
#include <math.h>

#include "launch.hpp"
#include "gp_core.hpp"

namespace {

constexpr int CK_MAX_D = SPR_GP_MAX_D;
constexpr int CK_MAX_P = SPR_CK_MAX_P;
constexpr int CK_NRED = CK_MAX_P + 1;          // the widest workgroup sum: a row of G and its entry of F^T R^-1 y
using CkShared = GpSharedT<CK_NRED>;
static_assert(GP_KC * CK_MAX_P <= GP_KC * GP_NB, "a chunk of F fits the staging buffer");

// v, its gradient and Adam's moments, and the P x P trend system: owned by thread 0; v, beta and status are read by every
// thread behind a barrier.
struct CkState {
  double v[CK_MAX_D], grad[CK_MAX_D], m1[CK_MAX_D], m2[CK_MAX_D];
  double G[CK_MAX_P * CK_MAX_P], Li[CK_MAX_P * CK_MAX_P], b[CK_MAX_P], beta[CK_MAX_P];
  int status;
};

// trend entry F[i][c]: columns [rho,] 1 [, x_0 .. x_{d-1}]; hr = 1 with a rho column
__device__ inline double ck_trend(const double *__restrict__ X, int64_t ldx, const double *__restrict__ rho, int64_t ldr,
                                  int hr, int i, int c) {
  if (c < hr) return rho[(int64_t)i * ldr];
  if (c == hr) return 1.0;
  return X[(int64_t)i * ldx + (c - hr - 1)];
}

// theta = 10^v in every thread (the same bits: the same LDS words through the same code)
__device__ inline void ck_theta(const double *v, int d, double (&th)[CK_MAX_D]) {
#pragma unroll
  for (int c = 0; c < CK_MAX_D; ++c) th[c] = c < d ? pow(10.0, v[c]) : 0.0;
}

// s = sum_c theta_c (x_kc - x_ic)^2; Z is the coordinate-major copy of X (d x n): summed coordinate by coordinate in index order
__device__ inline double ck_sqdist(const double *Z, const double (&th)[CK_MAX_D], int n, int d, int k, int i) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < CK_MAX_D; ++c)
    if (c < d) {
      const double u = Z[c * n + k] - Z[c * n + i];
      s = fma(th[c] * u, u, s);
    }
  return s;
}

// thread 0: G (upper triangle read) = L L^T in st.G's lower triangle, beta = G^-1 b by two substitutions, Li = L^-1, and
// Ginv = Li^T Li to its output.  -> 0, or 3 at a pivot that is not positive and finite.
__device__ inline int ck_trend_solve(int P, CkState &st, double *Ginv) {
  double *G = st.G, *Li = st.Li;
  for (int j = 0; j < P; ++j) {
    double p = G[j * CK_MAX_P + j];
    for (int k = 0; k < j; ++k) p = fma(-G[j * CK_MAX_P + k], G[j * CK_MAX_P + k], p);
    if (!(p > 0.0) || !(p <= DBL_MAX)) return 3;
    const double s = sqrt(p);
    G[j * CK_MAX_P + j] = s;
    for (int i = j + 1; i < P; ++i) {
      double a = G[j * CK_MAX_P + i];                        // the upper triangle holds G
      for (int k = 0; k < j; ++k) a = fma(-G[i * CK_MAX_P + k], G[j * CK_MAX_P + k], a);
      G[i * CK_MAX_P + j] = a / s;
    }
  }
  for (int i = 0; i < P; ++i) {                              // L w = b
    double a = st.b[i];
    for (int k = 0; k < i; ++k) a = fma(-G[i * CK_MAX_P + k], st.beta[k], a);
    st.beta[i] = a / G[i * CK_MAX_P + i];
  }
  for (int i = P - 1; i >= 0; --i) {                         // L^T beta = w
    double a = st.beta[i];
    for (int k = i + 1; k < P; ++k) a = fma(-G[k * CK_MAX_P + i], st.beta[k], a);
    st.beta[i] = a / G[i * CK_MAX_P + i];
  }
  for (int c = 0; c < P; ++c)                                // Li = L^-1, column by column
    for (int i = 0; i < P; ++i) {
      double a = i == c ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) a = fma(-G[i * CK_MAX_P + k], Li[k * CK_MAX_P + c], a);
      Li[i * CK_MAX_P + c] = i < c ? 0.0 : a / G[i * CK_MAX_P + i];
    }
  for (int a = 0; a < P; ++a)
    for (int c = 0; c < P; ++c) {
      double s = 0.0;
      for (int k = (a > c ? a : c); k < P; ++k) s = fma(Li[k * CK_MAX_P + a], Li[k * CK_MAX_P + c], s);
      Ginv[a * P + c] = s;
    }
  return 0;
}

// One evaluation at st.v: every output at that v, the loss returned in every thread, the gradient left in st.grad by thread 0
// (for thread 0 alone, until the caller's next barrier), and only with status 0.  The caller has a barrier between its last
// write of st.v and this call.  -> the status (the same in every thread).
__device__ int ck_evaluate(int n, int d, int P, int hr, const double *__restrict__ X, int64_t ldx,
                           const double *__restrict__ y, int64_t ldy, const double *__restrict__ rho, int64_t ldr,
                           double nugget, CkState &st, double *Z, double *A, double *Xi, double *Rinv, double *RinvF,
                           double *Ginv, double *beta, double *gamma, double *sigma2, CkShared &sh, double &loss) {
  const int tid = threadIdx.x;

  // 1-2. theta, then R (upper triangle) from the coordinate-major copy of X the kernel made at its start
  {
    double th[CK_MAX_D];
    ck_theta(st.v, d, th);
    for (int idx = tid; idx < n * n; idx += GP_T) {
      const int k = idx / n, i = idx - k * n;
      if (i >= k) {
        const double rv = exp(-ck_sqdist(Z, th, n, d, k, i));
        A[idx] = i == k ? rv + nugget : rv;
      }
    }
  }
  __syncthreads();

  // 3. factor, invert
  double logdet;
  int status = gp_factor_invert(n, A, Xi, Rinv, sh, logdet);
  if (status != 0) return status;

  // 4. R^-1 F
  const int ngn = (n + GP_T - 1) / GP_T;
  for (int g = 0; g < ngn; ++g) {
    const int i = g * GP_T + tid;
    const bool cv = i < n;
    double acc[CK_MAX_P];
#pragma unroll
    for (int c = 0; c < CK_MAX_P; ++c) acc[c] = 0.0;
    for (int jc = 0; jc < n; jc += GP_KC) {
      __syncthreads();             // the previous chunk is consumed; R^-1 as other threads wrote it is visible
      for (int e = tid; e < GP_KC * CK_MAX_P; e += GP_T) {
        const int j = jc + e / CK_MAX_P, c = e % CK_MAX_P;
        sh.S[e] = (j < n && c < P) ? ck_trend(X, ldx, rho, ldr, hr, j, c) : 0.0;
      }
      __syncthreads();
      if (cv) {
        const int kn = n - jc < GP_KC ? n - jc : GP_KC;
        for (int jj = 0; jj < kn; ++jj) {
          const double w = Rinv[(jc + jj) * n + i];
#pragma unroll
          for (int c = 0; c < CK_MAX_P; ++c) acc[c] = fma(w, sh.S[jj * CK_MAX_P + c], acc[c]);
        }
      }
    }
    if (cv) {
#pragma unroll
      for (int c = 0; c < CK_MAX_P; ++c)
        if (c < P) RinvF[i * P + c] = acc[c];
    }
  }

  // 5. G = F^T (R^-1 F) and b = (R^-1 F)^T y, a row of G at a time (every thread reads the rows of R^-1 F it wrote)
  for (int a = 0; a < P; ++a) {
    double part[CK_NRED];
#pragma unroll
    for (int c = 0; c < CK_NRED; ++c) part[c] = 0.0;
    for (int i = tid; i < n; i += GP_T) {
      const double fa = ck_trend(X, ldx, rho, ldr, hr, i, a);
#pragma unroll
      for (int c = 0; c < CK_MAX_P; ++c)
        if (c < P) part[c] = fma(fa, RinvF[i * P + c], part[c]);
      part[CK_MAX_P] = fma(RinvF[i * P + a], y[(int64_t)i * ldy], part[CK_MAX_P]);
    }
    gp_block_sum<CK_NRED>(part, sh.red);
    if (tid == 0) {
#pragma unroll
      for (int c = 0; c < CK_MAX_P; ++c) st.G[a * CK_MAX_P + c] = part[c];
      st.b[a] = part[CK_MAX_P];
    }
  }

  // 6. the trend system
  if (tid == 0) {
    st.status = ck_trend_solve(P, st, Ginv);
    for (int c = 0; c < P; ++c) beta[c] = st.beta[c];
  }
  __syncthreads();
  status = st.status;                                        // one LDS word decides for the whole workgroup
  if (status != 0) return status;

  // 7. res, gamma, sigma2
  for (int i = tid; i < n; i += GP_T) {
    double f = 0.0;
    for (int c = 0; c < P; ++c) f = fma(ck_trend(X, ldx, rho, ldr, hr, i, c), st.beta[c], f);
    sh.res[i] = y[(int64_t)i * ldy] - f;
  }
  __syncthreads();
  double ps[1] = {0.0};
  for (int i = tid; i < n; i += GP_T) {
    double a = 0.0;
    for (int j = 0; j < n; ++j) a = fma(Rinv[j * n + i], sh.res[j], a);
    sh.al[i] = a;
    gamma[i] = a;
    ps[0] = fma(sh.res[i], a, ps[0]);
  }
  gp_block_sum<1>(ps, sh.red);                                // (its barriers put sh.al behind them)
  const double s2 = ps[0] / (double)(n - P);
  if (!(s2 > 0.0) || !(s2 <= DBL_MAX)) return 4;             // the same bits in every thread

  // 8. the triangle pass: sum_ij W_ij (-theta_c u_c^2 exp(-s_ij)), the upper triangle doubled (the diagonal has u = 0 exactly)
  double pg[CK_MAX_D];
#pragma unroll
  for (int c = 0; c < CK_MAX_D; ++c) pg[c] = 0.0;
  {
    double th[CK_MAX_D];
    ck_theta(st.v, d, th);
    for (int idx = tid; idx < n * n; idx += GP_T) {
      const int k = idx / n, i = idx - k * n;
      if (i > k) {
        const double rv = exp(-ck_sqdist(Z, th, n, d, k, i));
        const double w = -2.0 * (Rinv[idx] - sh.al[k] * sh.al[i] / s2) * rv;
#pragma unroll
        for (int c = 0; c < CK_MAX_D; ++c)
          if (c < d) {
            const double u = Z[c * n + k] - Z[c * n + i];
            pg[c] = fma(w * (th[c] * u), u, pg[c]);
          }
      }
    }
  }
  gp_block_sum<CK_MAX_D>(pg, sh.red);
  const double dn = (double)n;
  loss = ((double)(n - P) * log(s2) + logdet) / dn;
  if (tid == 0) {
    *sigma2 = s2;
#pragma unroll
    for (int c = 0; c < CK_MAX_D; ++c) st.grad[c] = c < d ? M_LN10 * pg[c] / dn : 0.0;
  }
  return 0;
}

// info row: evaluations, loss, e, status, gradient (d); thread 0 keeps it current in memory.  ws: per model A, X (n x n each)
// and Z (d x n).
__global__ __launch_bounds__(GP_T) void ck_train_kernel(const double *__restrict__ X, int64_t ldx,
                                                        const double *__restrict__ Y, int64_t ldy,
                                                        const double *__restrict__ Rho, int64_t ldr, int n, int d, int P,
                                                        double *v_all, double nugget, double v_lo, double v_hi, double lr,
                                                        int max_iter, double tol, double *Rinv_all, double *RinvF_all,
                                                        double *Ginv_all, double *beta_all, double *gamma_all,
                                                        double *sigma2_all, double *info, double *trace, double *ws) {
  __shared__ CkShared sh;
  __shared__ CkState st;
  const int q = blockIdx.x, tid = threadIdx.x;
  const int hr = Rho != nullptr ? 1 : 0;
  const size_t nn = (size_t)n * n;
  double *A = ws + (2 * nn + (size_t)n * d) * q, *Xi = A + nn, *Z = Xi + nn;
  double *Rinv = Rinv_all + nn * q, *RinvF = RinvF_all + (size_t)n * P * q, *Ginv = Ginv_all + (size_t)P * P * q;
  double *beta = beta_all + (size_t)P * q, *gamma = gamma_all + (size_t)n * q, *sigma2 = sigma2_all + q;
  const double *rho = hr ? Rho + q : nullptr;
  double *rec = info + (size_t)(4 + d) * q;
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < CK_MAX_D; ++c) {
      st.v[c] = c < d ? v_all[(size_t)d * q + c] : 0.0;
      st.m1[c] = 0.0; st.m2[c] = 0.0; st.grad[c] = NAN;
    }
    st.status = 0;
    rec[0] = 0.0; rec[1] = NAN; rec[2] = NAN; rec[3] = 0.0;
    for (int c = 0; c < d; ++c) rec[4 + c] = NAN;
  }
  for (int i = tid; i < n; i += GP_T)                        // Z: X coordinate-major, so that the pair loops read it coalesced
    for (int c = 0; c < d; ++c) Z[c * n + i] = X[(int64_t)i * ldx + c];
  __syncthreads();
  double b1t = 1.0, b2t = 1.0, loss_old = 1e10, loss = 0.0, e = 1e10;
  int evals = 0, status = 0;
  bool last = max_iter == 0;
  for (int it = 0; it <= max_iter; ++it) {                   // max_iter evaluations with a step, one at the parameters kept
    status = ck_evaluate(n, d, P, hr, X, ldx, Y + q, ldy, rho, ldr, nugget, st, Z, A, Xi, Rinv, RinvF, Ginv, beta, gamma,
                         sigma2, sh, loss);
    if (status != 0) break;
    if (last) {
      if (max_iter == 0 && tid == 0) {
        rec[1] = loss;
        for (int c = 0; c < d; ++c) rec[4 + c] = st.grad[c];
      }
      break;
    }
    e = fabs(loss - loss_old);
    loss_old = loss;
    b1t *= 0.9;
    b2t *= 0.999;
    ++evals;
    if (tid == 0) {
      if (trace != nullptr) {
        double *tr = trace + ((size_t)q * max_iter + it) * (1 + d);
        tr[0] = loss;
        for (int c = 0; c < d; ++c) tr[1 + c] = st.v[c];
      }
#pragma unroll
      for (int c = 0; c < CK_MAX_D; ++c)
        if (c < d) {
          const double g = st.grad[c];
          const double a1 = 0.9 * st.m1[c] + (1.0 - 0.9) * g;
          const double a2 = 0.999 * st.m2[c] + (1.0 - 0.999) * g * g;
          const double denom = sqrt(a2) / sqrt(1.0 - b2t) + 1e-8;
          st.m1[c] = a1;
          st.m2[c] = a2;
          const double w = st.v[c] - (lr / (1.0 - b1t)) * (a1 / denom);
          st.v[c] = w < v_lo ? v_lo : (w > v_hi ? v_hi : w);
          rec[4 + c] = g;
        }
      rec[0] = evals; rec[1] = loss; rec[2] = e;
      sh.stop = (e <= tol || evals >= max_iter) ? 1 : 0;
    }
    __syncthreads();
    last = sh.stop != 0;                                     // one LDS word decides for the whole workgroup
    __syncthreads();
  }
  if (tid == 0) {
    rec[3] = status;
    for (int c = 0; c < d; ++c) v_all[(size_t)d * q + c] = st.v[c];
  }
}

__global__ __launch_bounds__(GP_T) void ck_predict_kernel(const double *__restrict__ X, int n, int d, int64_t ldx,
                                                          const double *__restrict__ Xs, int np, int64_t ldxs,
                                                          const double *__restrict__ RhoS, int64_t ldrs, int P,
                                                          const double *__restrict__ v_all, const double *__restrict__ Rinv_all,
                                                          const double *__restrict__ RinvF_all,
                                                          const double *__restrict__ Ginv_all,
                                                          const double *__restrict__ beta_all,
                                                          const double *__restrict__ gamma_all,
                                                          const double *__restrict__ sigma2_all, double *__restrict__ mean,
                                                          double *__restrict__ mse, int r) {
  __shared__ double ks[GP_PB * GP_MAX_M];
  __shared__ double red[4 * 2 * GP_PB];
  __shared__ double us[GP_PB * CK_MAX_P];                     // F^T R^-1 r* per test point
  const int q = blockIdx.x, p0 = blockIdx.y * GP_PB, tid = threadIdx.x;
  const int npb = np - p0 < GP_PB ? np - p0 : GP_PB;
  const int hr = RhoS != nullptr ? 1 : 0;
  const double *Rinv = Rinv_all + (size_t)n * n * q, *RinvF = RinvF_all + (size_t)n * P * q;
  const double *Ginv = Ginv_all + (size_t)P * P * q, *beta = beta_all + (size_t)P * q, *gamma = gamma_all + (size_t)n * q;
  double th[CK_MAX_D];
  ck_theta(v_all + (size_t)d * q, d, th);
  for (int e = tid; e < GP_PB * n; e += GP_T) {
    const int pp = e / n, i = e - pp * n;
    double rv = 0.0;
    if (pp < npb) {
      const double *a = X + (int64_t)i * ldx, *b = Xs + (int64_t)(p0 + pp) * ldxs;
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < CK_MAX_D; ++c)
        if (c < d) {
          const double u = a[c] - b[c];
          s = fma(th[c] * u, u, s);
        }
      rv = exp(-s);
    }
    ks[e] = rv;
  }
  __syncthreads();
  double part[2 * GP_PB];                                    // r*.gamma and r*^T R^-1 r*
#pragma unroll
  for (int c = 0; c < 2 * GP_PB; ++c) part[c] = 0.0;
  for (int i = tid; i < n; i += GP_T) {
    double acc[GP_PB];
#pragma unroll
    for (int pp = 0; pp < GP_PB; ++pp) acc[pp] = 0.0;
    for (int j = 0; j < n; ++j) {
      const double w = Rinv[j * n + i];                      // = R^-1[i][j]: symmetric, read along the row for coalescing
#pragma unroll
      for (int pp = 0; pp < GP_PB; ++pp) acc[pp] = fma(w, ks[pp * n + j], acc[pp]);
    }
    const double g = gamma[i];
#pragma unroll
    for (int pp = 0; pp < GP_PB; ++pp) {
      const double rv = ks[pp * n + i];
      part[pp] = fma(rv, g, part[pp]);
      part[GP_PB + pp] = fma(rv, acc[pp], part[GP_PB + pp]);
    }
  }
  gp_block_sum<2 * GP_PB>(part, red);
  for (int c = 0; c < P; ++c) {                              // (R^-1 F)^T r*, a trend column at a time
    double pu[GP_PB];
#pragma unroll
    for (int pp = 0; pp < GP_PB; ++pp) pu[pp] = 0.0;
    for (int i = tid; i < n; i += GP_T) {
      const double w = RinvF[i * P + c];
#pragma unroll
      for (int pp = 0; pp < GP_PB; ++pp) pu[pp] = fma(w, ks[pp * n + i], pu[pp]);
    }
    gp_block_sum<GP_PB>(pu, red);
    if (tid == 0) {
#pragma unroll
      for (int pp = 0; pp < GP_PB; ++pp) us[pp * CK_MAX_P + c] = pu[pp];
    }
  }
  if (tid == 0) {
    const double s2 = sigma2_all[q];
#pragma unroll
    for (int pp = 0; pp < GP_PB; ++pp)
      if (pp < npb) {
        double fs[CK_MAX_P], u[CK_MAX_P], m = 0.0, quad = 0.0;
        for (int c = 0; c < P; ++c) {
          fs[c] = ck_trend(Xs, ldxs, hr ? RhoS + q : nullptr, ldrs, hr, p0 + pp, c);
          u[c] = us[pp * CK_MAX_P + c] - fs[c];
          m = fma(fs[c], beta[c], m);
        }
        for (int a = 0; a < P; ++a) {
          double t = 0.0;
          for (int c = 0; c < P; ++c) t = fma(Ginv[a * P + c], u[c], t);
          quad = fma(u[a], t, quad);
        }
        const double w = s2 * ((1.0 - part[GP_PB + pp]) + quad);
        mean[(int64_t)(p0 + pp) * r + q] = m + part[pp];
        mse[(int64_t)(p0 + pp) * r + q] = w > 0.0 ? w : 0.0;
      }
  }
}

// ------------------------------------------------------------------------------------------------ host side
inline int ck_trend_cols(int32_t d, int32_t regr, bool rho) { return (rho ? 1 : 0) + 1 + (regr == SPR_CK_LINEAR ? d : 0); }

size_t ck_workspace(int32_t n, int32_t d, int32_t r) {
  if (n < 1 || n > GP_MAX_M || d < 1 || d > CK_MAX_D || r < 1) return 0;
  return sizeof(double) * (size_t)r * (2 * (size_t)n * n + (size_t)n * d);
}

int ck_train(const char *name, const double *d_X, int32_t n, int32_t d, int64_t ldx, const double *d_Y, int32_t r, int64_t ldy,
             const double *d_Rho, int64_t ldr, int32_t regr, double *d_v, double nugget, double v_lo, double v_hi, double lr,
             int32_t max_iter, double tol, double *d_Rinv, double *d_RinvF, double *d_Ginv, double *d_beta, double *d_gamma,
             double *d_sigma2, double *d_info, double *d_trace, void *d_workspace, size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_X && d_Y && d_v && d_Rinv && d_RinvF && d_Ginv && d_beta && d_gamma && d_sigma2 && d_info && d_workspace,
              SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(n > 0 && d > 0 && r > 0 && ldx >= d && ldy >= r && (d_Rho == nullptr || ldr >= r) && max_iter >= 0, SPR_E_INVALID,
              "%s: bad shape n=%d d=%d ldx=%lld r=%d ldy=%lld ldr=%lld max_iter=%d", name, n, d, (long long)ldx, r,
              (long long)ldy, (long long)ldr, max_iter);
  SPR_REQUIRE(regr == SPR_CK_CONSTANT || regr == SPR_CK_LINEAR, SPR_E_INVALID, "%s: unknown regr code %d", name, regr);
  const int P = ck_trend_cols(d, regr, d_Rho != nullptr);
  SPR_REQUIRE(n > P, SPR_E_INVALID, "%s: bad shape: n = %d points do not exceed the %d trend columns", name, n, P);
  SPR_REQUIRE(nugget >= 0.0 && nugget <= DBL_MAX, SPR_E_INVALID, "%s: nugget = %g must be non-negative and finite", name, nugget);
  SPR_REQUIRE(lr > 0.0 && lr <= DBL_MAX && tol >= 0.0 && tol <= DBL_MAX, SPR_E_INVALID,
              "%s: lr = %g must be positive and tol = %g non-negative, both finite", name, lr, tol);
  SPR_REQUIRE(v_lo <= v_hi && v_lo >= -DBL_MAX && v_hi <= DBL_MAX, SPR_E_INVALID,
              "%s: bounds v_lo = %g <= v_hi = %g must be finite", name, v_lo, v_hi);
  SPR_REQUIRE(n <= GP_MAX_M, SPR_E_UNSUPPORTED, "%s: n = %d exceeds %d", name, n, GP_MAX_M);
  SPR_REQUIRE(d <= CK_MAX_D, SPR_E_UNSUPPORTED, "%s: d = %d coordinates exceed %d", name, d, CK_MAX_D);
  SPR_REQUIRE(workspace_bytes >= ck_workspace(n, d, r), SPR_E_INVALID, "%s: workspace of %zu bytes, %zu needed", name,
              workspace_bytes, ck_workspace(n, d, r));
  SPR_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, SPR_E_INVALID, "%s: workspace must be 8-byte aligned", name);
  hipLaunchKernelGGL(ck_train_kernel, dim3(r), dim3(GP_T), 0, static_cast<hipStream_t>(stream), d_X, ldx, d_Y, ldy, d_Rho, ldr,
                     (int)n, (int)d, P, d_v, nugget, v_lo, v_hi, lr, (int)max_iter, tol, d_Rinv, d_RinvF, d_Ginv, d_beta, d_gamma,
                     d_sigma2, d_info, d_trace, static_cast<double *>(d_workspace));
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

int ck_predict(const char *name, const double *d_X, int32_t n, int32_t d, int64_t ldx, const double *d_Xstar, int32_t n_p,
               int64_t ldxs, const double *d_RhoStar, int64_t ldrs, int32_t regr, const double *d_v, int32_t r,
               const double *d_Rinv, const double *d_RinvF, const double *d_Ginv, const double *d_beta, const double *d_gamma,
               const double *d_sigma2, double *d_mean, double *d_mse, void *stream) {
  SPR_REQUIRE(d_X && d_Xstar && d_v && d_Rinv && d_RinvF && d_Ginv && d_beta && d_gamma && d_sigma2 && d_mean && d_mse,
              SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(n > 0 && d > 0 && r > 0 && n_p > 0 && ldx >= d && ldxs >= d && (d_RhoStar == nullptr || ldrs >= r), SPR_E_INVALID,
              "%s: bad shape n=%d d=%d ldx=%lld n_p=%d ldxs=%lld ldrs=%lld r=%d", name, n, d, (long long)ldx, n_p,
              (long long)ldxs, (long long)ldrs, r);
  SPR_REQUIRE(regr == SPR_CK_CONSTANT || regr == SPR_CK_LINEAR, SPR_E_INVALID, "%s: unknown regr code %d", name, regr);
  const int P = ck_trend_cols(d, regr, d_RhoStar != nullptr);
  SPR_REQUIRE(n > P, SPR_E_INVALID, "%s: bad shape: n = %d points do not exceed the %d trend columns", name, n, P);
  SPR_REQUIRE(n <= GP_MAX_M, SPR_E_UNSUPPORTED, "%s: n = %d exceeds %d", name, n, GP_MAX_M);
  SPR_REQUIRE(d <= CK_MAX_D, SPR_E_UNSUPPORTED, "%s: d = %d coordinates exceed %d", name, d, CK_MAX_D);
  const int nblk = (n_p + GP_PB - 1) / GP_PB;
  SPR_REQUIRE(nblk <= 65535, SPR_E_UNSUPPORTED, "%s: n_p = %d exceeds %d test points per call", name, n_p, 65535 * GP_PB);
  hipLaunchKernelGGL(ck_predict_kernel, dim3(r, nblk), dim3(GP_T), 0, static_cast<hipStream_t>(stream), d_X, (int)n, (int)d, ldx,
                     d_Xstar, (int)n_p, ldxs, d_RhoStar, ldrs, P, d_v, d_Rinv, d_RinvF, d_Ginv, d_beta, d_gamma, d_sigma2, d_mean,
                     d_mse, (int)r);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

}  // namespace

extern "C" size_t spr_ck_workspace(int32_t n, int32_t d, int32_t r) { return ck_workspace(n, d, r); }

SPR_ENTRY(spr_ck_train_f64,
          (const double *d_X, int32_t n, int32_t d, int64_t ldx, const double *d_Y, int32_t r, int64_t ldy, const double *d_Rho,
           int64_t ldr, int32_t regr, double *d_v, double nugget, double v_lo, double v_hi, double lr, int32_t max_iter,
           double tol, double *d_Rinv, double *d_RinvF, double *d_Ginv, double *d_beta, double *d_gamma, double *d_sigma2,
           double *d_info, double *d_trace, void *d_workspace, size_t workspace_bytes, void *stream),
          ck_train, d_X, n, d, ldx, d_Y, r, ldy, d_Rho, ldr, regr, d_v, nugget, v_lo, v_hi, lr, max_iter, tol, d_Rinv, d_RinvF,
          d_Ginv, d_beta, d_gamma, d_sigma2, d_info, d_trace, d_workspace, workspace_bytes, stream)

SPR_ENTRY(spr_ck_predict_f64,
          (const double *d_X, int32_t n, int32_t d, int64_t ldx, const double *d_Xstar, int32_t n_p, int64_t ldxs,
           const double *d_RhoStar, int64_t ldrs, int32_t regr, const double *d_v, int32_t r, const double *d_Rinv,
           const double *d_RinvF, const double *d_Ginv, const double *d_beta, const double *d_gamma, const double *d_sigma2,
           double *d_mean, double *d_mse, void *stream),
          ck_predict, d_X, n, d, ldx, d_Xstar, n_p, ldxs, d_RhoStar, ldrs, regr, d_v, r, d_Rinv, d_RinvF, d_Ginv, d_beta, d_gamma,
          d_sigma2, d_mean, d_mse, stream)
