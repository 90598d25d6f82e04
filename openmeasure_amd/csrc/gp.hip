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
//
// ARD lengthscales and an output scale (GPR.train(kernel=GPKernel(...)); flags bit 0 / bit 1), L = d or 1, S = 1 or 0:
//   raw = (raw_l[0..L-1], [raw_o], raw_n, mu);  l_c = softplus(raw_l[c]),  o = softplus(raw_o) or 1,  z_i = P0[i, :] / l,
//   t_ij = max(|z_i - z_j|_2, 1e-15),  K = o k(t) + s2 I, the same loss;  d loss / d raw_l[c] = sigmoid(raw_l[c]) o sum_ij W_ij
//   dk(t_ij) u_c^2 / t_ij^2 / l_c / 2m with u_c = z_ic - z_jc (not ARD: sum W o dk / l / 2m),  d loss / d raw_o = sigmoid(raw_o)
//   sum W k / 2m;  predict: mean = mu + o k*.alpha, var = max(o - o^2 k*^T K^-1 k*, 0) + s2.
// gp_train_ard_kernel is gp_train_kernel with another step 1 and another triangle pass in step 5; steps 2-4 (gp_factor_invert)
// and alpha with its four sums (gp_alpha_sums) are the same functions.  Step 1 writes Z = P0 / l (coordinate-major, m x d, in
// the mode's workspace slice: no distance matrix, no pre-pass) and forms t from it with fma in index order; the triangle pass
// recomputes t, k, dk and accumulates 4 + S + L sums in a fixed array of 5 + SPR_GP_MAX_D (unrolled loops predicated on c < d).
// The parameters, their gradient and Adam's moments live in LDS, owned by thread 0 (the factorisation fills the register
// file); d, flags, n_par are arguments, uniform over the workgroup, and the stop decision is the same LDS word.
//
// Per-point noise (GPR.update(fixed_noise=True / retrain=True); spr_gp_train_noise_f64): n_i = w_i s2 + V[i, q] for mode q,
//   K = o k(t) + diag(n), the same loss;  d loss / d raw_n = sigmoid(raw_n) sum_i w_i (K^-1_ii - alpha_i^2) / 2m, every other
//   component unchanged in form.  w_i = 1: the point carries the learned noise; w_i = 0: its variance V[i, q] is given.
// It is gp_train_ard_kernel<true>: the diagonal of step 1 and two of the sums of step 5 (gp_alpha_sums<true>) read w and V, the
// factorisation, the loop, the control flow and the layouts are the same code, for flags 0..3.  With w = 1, V = 0 each of those
// operations multiplies by 1.0 or adds 0.0: the bits of gp_train_ard_kernel<false>.  predict reads K^-1 and alpha and adds s2
// at the test point: its variance stays latent + learned noise, V is not added.
//
// Accumulating data (GPR.update(append=True); spr_gp_state_f64, spr_gp_append_f64): the state is X = L^-1 and log det K beside K^-1.
// spr_gp_state_f64 is the launch of spr_gp_train_noise_f64 with max_iter = 0 (the same bits) and a second one that copies X out of
// the workspace and sums log det K from the factor's diagonal.  spr_gp_append_f64 adds k <= 64 rows to X in O(m^2 k) per mode --
// W = X B, S = C - W^T W factored in LDS, the new rows N = Ls^-1 [-W^T X, I], K'^-1 = K^-1 + N^T N -- in three launches of which none
// waits for another (see "state and append" below).  B and C are formed from the scaled coordinates z = P0 / l as
// gp_train_ard_kernel forms K; with flags = 0 that differs from the distance-matrix route of gp_train_kernel by rounding only.
#include <float.h>
#include <math.h>

#include "launch.hpp"
#include "gp_core.hpp"   // gp_block_sum, gp_panel_acc, gp_fwd, GpSharedT, gp_factor_invert: shared with cokriging.hip

namespace {

__device__ inline double gp_softplus(double x) { return x > 0.0 ? x + log1p(exp(-x)) : log1p(exp(x)); }
__device__ inline double gp_sigmoid(double x) {
  if (x >= 0.0) return 1.0 / (1.0 + exp(-x));
  const double e = exp(x);
  return e / (1.0 + e);
}

// a * b rounded to a double before anything is added to it (never one half of a fused multiply-add)
__device__ inline double gp_mul_rounded(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
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


// Step 5 up to the triangle pass, shared too: res = y - mu, alpha = K^-1 res (one thread per row, fixed order) and this thread's
// share of res.alpha, sum alpha, tr K^-1, alpha.alpha in part[0..3].  alpha is in sh.al behind the closing barrier.
// WT: the terms of part[2] and part[3] take the factor w[i] (the noise weights of gp_train_noise; a factor 1.0 changes no bit).
template <bool WT, class Sh, int N>
__device__ inline void gp_alpha_sums(int m, const double *__restrict__ y, int64_t ldy, double mu, const double *Kinv,
                                     double *alpha, Sh &sh, double (&part)[N], const double *__restrict__ w = nullptr) {
  const int tid = threadIdx.x;
  for (int i = tid; i < m; i += GP_T) sh.res[i] = y[(int64_t)i * ldy] - mu;
  __syncthreads();
  for (int i = tid; i < m; i += GP_T) {
    double a = 0.0;
    for (int j = 0; j < m; ++j) a = fma(Kinv[j * m + i], sh.res[j], a);
    sh.al[i] = a;
    alpha[i] = a;
    part[0] += sh.res[i] * a;
    part[1] += a;
    if (WT) {
      const double wi = w[i];
      part[2] += wi * Kinv[i * m + i];
      part[3] += (wi * a) * a;
    } else {
      part[2] += Kinv[i * m + i];
      part[3] += a * a;
    }
  }
  __syncthreads();
}

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

  // 2-4. factor, invert
  double logdet;
  const int status = gp_factor_invert(m, A, X, Kinv, sh, logdet);
  if (status != 0) return status;

  // 5. alpha and the sums
  double part[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  gp_alpha_sums<false>(m, y, ldy, mu, Kinv, alpha, sh, part);
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

// ------------------------------------------------------------------------------------------------ ARD / output scale
// flags: bit 0 ARD (one lengthscale per coordinate, d <= GP_MAX_D), bit 1 output scale.  L = d or 1, S = 1 or 0,
// n_par = L + S + 2; in memory raw = (raw_l[0..L-1], [raw_o], raw_n, mu), packed.  Inside the kernels the parameters, their
// gradient and Adam's moments sit in FIXED slots -- raw_l at 0 .. GP_MAX_D-1, raw_o at GP_O, raw_n at GP_N, mu at GP_MU -- so
// that every index is a compile-time constant; a slot the model does not have keeps 0 and a zero gradient (Adam leaves it
// where it is).  The training kernel keeps them in LDS (GpArdState), owned by thread 0: the factorisation already fills the
// register file, and 4 x 11 more doubles per thread went to scratch.
constexpr int GP_MAX_D = SPR_GP_MAX_D;
constexpr int GP_O = GP_MAX_D, GP_N = GP_MAX_D + 1, GP_MU = GP_MAX_D + 2, GP_NPAR = GP_MAX_D + 3;
constexpr int GP_NSUM = 5 + GP_MAX_D;
using GpSharedArd = GpSharedT<GP_NSUM>;

struct GpArdState {
  double par[GP_NPAR], grad[GP_NPAR], m1[GP_NPAR], m2[GP_NPAR];
};

__device__ inline void gp_unpack(const double *src, int L, int S, double *v) {
#pragma unroll
  for (int c = 0; c < GP_MAX_D; ++c) v[c] = c < L ? src[c] : 0.0;
  v[GP_O] = S ? src[L] : 0.0;
  v[GP_N] = src[L + S];
  v[GP_MU] = src[L + S + 1];
}

__device__ inline void gp_pack(const double *v, int L, int S, double *dst) {
#pragma unroll
  for (int c = 0; c < GP_MAX_D; ++c)
    if (c < L) dst[c] = v[c];
  if (S) dst[L] = v[GP_O];
  dst[L + S] = v[GP_N];
  dst[L + S + 1] = v[GP_MU];
}

// t between the scaled points k and i; Z is coordinate-major (d x m): summed coordinate by coordinate in index order
__device__ inline double gp_scaled_dist(const double *Z, int m, int d, int k, int i) {
  double s = 0.0;
  for (int c = 0; c < d; ++c) {
    const double v = Z[c * m + k] - Z[c * m + i];
    s = fma(v, v, s);
  }
  s = sqrt(s);
  return s > 1e-15 ? s : 1e-15;
}

// One evaluation of the ARD / scaled model at st.par: K^-1 and alpha to their outputs, the loss returned in every thread, the
// gradient left in st.grad by thread 0 (for thread 0 alone, until the caller's next barrier), and only when the factorisation
// succeeds (tw: thread 0's, when asked for, sum_i w_i (K^-1_ii - alpha_i^2) / 2m).  Z: this mode's m x d slice for the scaled coordinates.  The caller has a barrier between its last write of st.par
// and this call.  -> 0, or the status of a failed pivot (the same in every thread).
// NOISE (gp_train_noise): point i carries the noise n_i = w[i] s2 + v[i ldv] instead of s2 -- w the weights of the learned
// noise, v this mode's column of the fixed variances -- and the noise gradient weighs its terms with w.  With w = 1, v = 0
// every operation returns the bits of the homoscedastic model.
template <bool NOISE>
__device__ int gp_evaluate_ard(int code, int m, int d, int flags, const double *__restrict__ P0, int64_t ldp,
                               const double *__restrict__ y, int64_t ldy, const double *__restrict__ w,
                               const double *__restrict__ v, int64_t ldv, GpArdState &st, double *Z, double *A, double *X,
                               double *Kinv, double *alpha, GpSharedArd &sh, double &loss, double *tw = nullptr) {
  const int tid = threadIdx.x;
  const bool ard = (flags & 1) != 0, scl = (flags & 2) != 0;
  const double o = scl ? gp_softplus(st.par[GP_O]) : 1.0, sig2 = gp_softplus(st.par[GP_N]) + 1e-4, mu = st.par[GP_MU];

  // 1. Z = P0 / l, then K (upper triangle) from Z.  The barrier that closed the previous evaluation's sums is behind every
  //    read of the old Z.
  {
    double ell[GP_MAX_D];
    ell[0] = gp_softplus(st.par[0]);
#pragma unroll
    for (int c = 1; c < GP_MAX_D; ++c) ell[c] = (ard && c < d) ? gp_softplus(st.par[c]) : ell[0];
    for (int i = tid; i < m; i += GP_T) {
      if (ard) {
#pragma unroll
        for (int c = 0; c < GP_MAX_D; ++c)
          if (c < d) Z[c * m + i] = P0[(int64_t)i * ldp + c] / ell[c];
      } else {
        for (int c = 0; c < d; ++c) Z[c * m + i] = P0[(int64_t)i * ldp + c] / ell[0];
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < m * m; idx += GP_T) {
    const int k = idx / m, i = idx - k * m;
    if (i >= k) {
      double kv, dk;
      gp_kern(code, gp_scaled_dist(Z, m, d, k, i), kv, dk);
      if (NOISE) {
        A[idx] = i == k ? o * kv + (w[i] * sig2 + v[(int64_t)i * ldv]) : o * kv;
      } else {
        A[idx] = i == k ? o * kv + sig2 : o * kv;
      }
    }
  }
  __syncthreads();

  // 2-4. factor, invert
  double logdet;
  const int status = gp_factor_invert(m, A, X, Kinv, sh, logdet);
  if (status != 0) return status;

  // 5. alpha and the sums: part[4] = sum W k, part[5 + c] = sum W dk u_c^2 / t^2 (not ARD: part[5] = sum W dk), the upper
  //    triangle doubled; o multiplies them at the end.  A diagonal or duplicated point has u = 0 exactly: its lengthscale term
  //    is 0, whatever the clamp.
  double part[GP_NSUM];
#pragma unroll
  for (int c = 0; c < GP_NSUM; ++c) part[c] = 0.0;
  gp_alpha_sums<NOISE>(m, y, ldy, mu, Kinv, alpha, sh, part, w);
  for (int idx = tid; idx < m * m; idx += GP_T) {
    const int k = idx / m, i = idx - k * m;
    if (i >= k) {
      double kv, dk;
      const double t = gp_scaled_dist(Z, m, d, k, i);
      gp_kern(code, t, kv, dk);
      double w = Kinv[idx] - sh.al[k] * sh.al[i];
      w = i == k ? w : 2.0 * w;
      part[4] += w * kv;
      if (ard) {
        const double g = w * dk / (t * t);
#pragma unroll
        for (int c = 0; c < GP_MAX_D; ++c)
          if (c < d) {
            const double u = Z[c * m + k] - Z[c * m + i];
            part[5 + c] = fma(g * u, u, part[5 + c]);
          }
      } else {
        part[5] += w * dk;
      }
    }
  }
  gp_block_sum<GP_NSUM>(part, sh.red);
  const double dm = (double)m;
  // The constant term is a product rounded on its own in every kernel that calls this: the training loops hoist it out of the
  // loop (it never was fused there), and a caller without a loop (gp_mt_eval_kernel) must not fuse it into the sum either.
  loss = (0.5 * part[0] + 0.5 * logdet + gp_mul_rounded(0.5 * dm, log(2.0 * M_PI))) / dm;
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < GP_MAX_D; ++c)
      st.grad[c] = (c == 0 || (ard && c < d)) ? gp_sigmoid(st.par[c]) * (o * part[5 + c] / gp_softplus(st.par[c])) / (2.0 * dm) : 0.0;
    st.grad[GP_O] = scl ? gp_sigmoid(st.par[GP_O]) * part[4] / (2.0 * dm) : 0.0;
    st.grad[GP_N] = gp_sigmoid(st.par[GP_N]) * (part[2] - part[3]) / (2.0 * dm);
    st.grad[GP_MU] = -part[1] / dm;
    if (tw != nullptr) *tw = (part[2] - part[3]) / (2.0 * dm);   // the noise term without its sigmoid (gp_mt_eval_kernel)
  }
  return 0;
}

// The loop of gp_train_kernel over n_par parameters.  info row: evaluations, loss, e, status, gradient (packed); thread 0 keeps
// it current in memory instead of carrying it in registers.  ws: per mode A, X (m x m each) and Z (m x d).
// NOISE: the per-point noise of gp_evaluate_ard, w (m) shared by the modes and column q of V (m x r, row stride ldv) for mode q;
// without it the three arguments are not read.
template <bool NOISE>
__global__ __launch_bounds__(GP_T) void gp_train_ard_kernel(const double *__restrict__ P0, int64_t ldp,
                                                            const double *__restrict__ Y, int64_t ldy,
                                                            const double *__restrict__ w, const double *__restrict__ V,
                                                            int64_t ldv, int m, int d, int code,
                                                            int flags, int n_par, double *raw, double lr, int max_iter,
                                                            double tol, double *Kinv_all, double *alpha_all, double *info,
                                                            double *trace, double *ws) {
  __shared__ GpSharedArd sh;
  __shared__ GpArdState st;
  const int q = blockIdx.x, tid = threadIdx.x;
  const int L = (flags & 1) ? d : 1, S = (flags & 2) ? 1 : 0;
  const size_t mm = (size_t)m * m;
  double *A = ws + (2 * mm + (size_t)m * d) * q, *X = A + mm, *Z = X + mm;
  double *Kinv = Kinv_all + mm * q, *alpha = alpha_all + (size_t)m * q;
  double *rec = info + (size_t)(4 + n_par) * q;
  if (tid == 0) {
    gp_unpack(raw + (size_t)n_par * q, L, S, st.par);
#pragma unroll
    for (int c = 0; c < GP_NPAR; ++c) { st.m1[c] = 0.0; st.m2[c] = 0.0; st.grad[c] = NAN; }
    rec[0] = 0.0; rec[1] = NAN; rec[2] = NAN; rec[3] = 0.0;
    gp_pack(st.grad, L, S, rec + 4);
  }
  __syncthreads();
  double b1t = 1.0, b2t = 1.0, loss_old = 1e10, loss = 0.0, e = 1e10;
  int evals = 0, status = 0;
  bool last = max_iter == 0;
  for (int it = 0; it <= max_iter; ++it) {                   // max_iter evaluations with a step, one at the parameters kept
    status = gp_evaluate_ard<NOISE>(code, m, d, flags, P0, ldp, Y + q, ldy, w, NOISE ? V + q : nullptr, ldv, st, Z, A, X, Kinv,
                                    alpha, sh, loss);
    if (status != 0) break;
    if (last) {
      if (max_iter == 0 && tid == 0) { rec[1] = loss; gp_pack(st.grad, L, S, rec + 4); }
      break;
    }
    e = fabs(loss - loss_old);
    loss_old = loss;
    b1t *= 0.9;
    b2t *= 0.999;
    ++evals;
    if (tid == 0) {
      if (trace != nullptr) {
        double *tr = trace + ((size_t)q * max_iter + it) * (1 + n_par);
        tr[0] = loss;
        gp_pack(st.par, L, S, tr + 1);
      }
#pragma unroll
      for (int c = 0; c < GP_NPAR; ++c) {
        const double g = st.grad[c];
        const double a1 = 0.9 * st.m1[c] + (1.0 - 0.9) * g;
        const double a2 = 0.999 * st.m2[c] + (1.0 - 0.999) * g * g;
        const double denom = sqrt(a2) / sqrt(1.0 - b2t) + 1e-8;
        st.m1[c] = a1;
        st.m2[c] = a2;
        st.par[c] -= (lr / (1.0 - b1t)) * (a1 / denom);
      }
      rec[0] = evals; rec[1] = loss; rec[2] = e;
      gp_pack(st.grad, L, S, rec + 4);
      sh.stop = (e <= tol || evals >= max_iter) ? 1 : 0;
    }
    __syncthreads();
    last = sh.stop != 0;                                     // one LDS word decides for the whole workgroup
    __syncthreads();
  }
  if (tid == 0) {
    rec[3] = status;
    gp_pack(st.par, L, S, raw + (size_t)n_par * q);
  }
}

// this thread's share of k*.alpha (part[pp]) and k*^T K^-1 k* (part[GP_PB + pp]) for the GP_PB test points whose k* is in ks
__device__ inline void gp_predict_sums(int m, const double *__restrict__ Kinv, const double *__restrict__ alpha,
                                       const double *ks, double (&part)[2 * GP_PB]) {
  const int tid = threadIdx.x;
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
  gp_predict_sums(m, Kinv, alpha, ks, part);
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

// gp_predict_kernel for the ARD / scaled model: k* from the scaled coordinates (z = P0 / l and z* = P* / l divided separately, as
// training divides them: a test point equal to a training point is at t = 0 exactly), o on the mean and the variance.
__global__ __launch_bounds__(GP_T) void gp_predict_ard_kernel(const double *__restrict__ P0, int m, int d, int64_t ldp,
                                                              const double *__restrict__ Ps, int np, int64_t lds_, int code,
                                                              int flags, int n_par, const double *__restrict__ raw,
                                                              const double *__restrict__ Kinv_all,
                                                              const double *__restrict__ alpha_all, double *__restrict__ mean,
                                                              double *__restrict__ var, int r, const double *__restrict__ s2) {
  __shared__ double ks[GP_PB * GP_MAX_M];
  __shared__ double red[4 * 2 * GP_PB];
  const int q = blockIdx.x, p0 = blockIdx.y * GP_PB, tid = threadIdx.x;
  const int npb = np - p0 < GP_PB ? np - p0 : GP_PB;
  const bool ard = (flags & 1) != 0;
  const int L = ard ? d : 1, S = (flags & 2) ? 1 : 0;
  double p[GP_NPAR], ell[GP_MAX_D];
  gp_unpack(raw + (size_t)n_par * q, L, S, p);
  ell[0] = gp_softplus(p[0]);
#pragma unroll
  for (int c = 1; c < GP_MAX_D; ++c) ell[c] = (ard && c < d) ? gp_softplus(p[c]) : ell[0];
  const double o = S ? gp_softplus(p[GP_O]) : 1.0, mu = p[GP_MU];
  const double sig2 = s2 != nullptr ? s2[q] : gp_softplus(p[GP_N]) + 1e-4;     // s2: the multitask model's stored task + global noise
  const double *Kinv = Kinv_all + (size_t)m * m * q, *alpha = alpha_all + (size_t)m * q;
  for (int e = tid; e < GP_PB * m; e += GP_T) {
    const int pp = e / m, i = e - pp * m;
    double kv = 0.0, dk;
    if (pp < npb) {
      const double *a = P0 + (int64_t)i * ldp, *b = Ps + (int64_t)(p0 + pp) * lds_;
      double s = 0.0;
      if (ard) {
#pragma unroll
        for (int c = 0; c < GP_MAX_D; ++c)
          if (c < d) {
            const double v = a[c] / ell[c] - b[c] / ell[c];
            s = fma(v, v, s);
          }
      } else {
        for (int c = 0; c < d; ++c) {
          const double v = a[c] / ell[0] - b[c] / ell[0];
          s = fma(v, v, s);
        }
      }
      s = sqrt(s);
      gp_kern(code, s > 1e-15 ? s : 1e-15, kv, dk);
    }
    ks[e] = kv;
  }
  __syncthreads();
  double part[2 * GP_PB];
  gp_predict_sums(m, Kinv, alpha, ks, part);
  gp_block_sum<2 * GP_PB>(part, red);
  if (tid == 0) {
#pragma unroll
    for (int pp = 0; pp < GP_PB; ++pp)
      if (pp < npb) {
        const double v = o - o * o * part[GP_PB + pp];
        mean[(int64_t)(p0 + pp) * r + q] = mu + o * part[pp];
        var[(int64_t)(p0 + pp) * r + q] = (v > 0.0 ? v : 0.0) + sig2;
      }
  }
}

// ------------------------------------------------------------------------------------------------ multitask
// GPR(gpr_type='MultiTask'): the r GPs share one noise parameter raw_g and one loss (spr_gp_train_mt_f64).
//   s2_q = (softplus(raw_t_q) + 1e-4) + (softplus(raw_g) + 1e-4),  K_q = o_q k(t) + s2_q I,  loss_q as above,
//   LOSS = (1 / r) sum_q loss_q;  own parameters of mode q: the single-task gradient / r;
//   d LOSS / d raw_g = sigmoid(raw_g) (1 / r) sum_q tw_q,  tw_q = sum_i (K_q^-1_ii - alpha_qi^2) / 2m.
// ONE Adam loop over the r n_par + 1 values and one stopping test, so every step needs a sum over the modes.  No workgroup
// waits for another: the loop is a chain of plain launches on one stream, (gp_mt_eval_kernel, gp_mt_step_kernel) per evaluation,
// and a state record in the workspace tells each launch what to do.  Its phase word: 0 evaluate and step, 1 the evaluation at
// the parameters kept is pending, 2 done -- a launch that finds 2 returns at once and writes nothing, so the host may enqueue
// SPR_GP_MT_CHUNK pairs at a time and look at the word only between chunks.  Every thread of a launch reads the same word,
// written by an earlier kernel of the stream: the decision is uniform and no barrier is reached by part of a workgroup.
//   gp_mt_eval_kernel, grid r: one evaluation of mode q by gp_evaluate_ard<true> with w_i = 1 and the global noise as the additive
//     term v (row stride 0: one word of the record) -- the diagonal is 1 * sig2 + v as in spr_gp_train_noise_f64, the same
//     device function, the same bits.  It writes K_q^-1, alpha_q, s2[q] (the sum the diagonal got) and the mode's record
//     (loss_q, status, tw_q, the n_par own gradients).
//   gp_mt_step_kernel, one workgroup: thread 0 sums the r records in index order (LOSS, sum tw, any failed pivot), then
//     phase 0: e, the trace row, Adam on all r n_par + 1 values (a loop with the stride of the workgroup: r is not limited by
//     it), the new global noise, the count, phase 1 when e <= tol or the count reached max_iter;  phase 1: LOSS and the gradient
//     of the final evaluation to d_info, phase 2;  a failed pivot: the statuses to d_info, phase 2, the parameters stay.
// Workspace (doubles): r slices (A, X, Z) as for spr_gp_train_ard_f64, then the record: head (GP_MT_HEAD), Adam's two moments
// (r (d + 3) + 1 each: room for any flags), the per-mode records (r x (3 + n_par)), m ones (the weights w).
// d_info (4 + NP + r, NP = r n_par + 1): evaluations with a step, LOSS, e, the largest status, the gradient of LOSS in the order
// (d_raw, raw_g), the per-mode statuses.  d_trace: NULL or max_iter x (1 + NP): (LOSS, d_raw, raw_g) before each step.
struct GpMtHead {
  int phase, count, pad0, pad1;
  double loss_old, e, b1t, b2t, vg;       // vg = softplus(raw_g) + 1e-4: what the next evaluation adds to every diagonal
};
constexpr int GP_MT_HEAD = 8;             // doubles kept for the head
static_assert(sizeof(GpMtHead) <= GP_MT_HEAD * sizeof(double), "the head fits its slot");
constexpr int GP_MT_REC = 3;              // loss, status, tw before a mode's gradient

struct GpMtLayout {
  size_t slice, head, m1, m2, rec, ones, total;   // offsets in doubles
};
__host__ __device__ inline GpMtLayout gp_mt_layout(int m, int d, int r) {
  GpMtLayout l;
  const size_t np_cap = (size_t)r * (d + 3) + 1;
  l.slice = 2 * (size_t)m * m + (size_t)m * d;
  l.head = l.slice * r;
  l.m1 = l.head + GP_MT_HEAD;
  l.m2 = l.m1 + np_cap;
  l.rec = l.m2 + np_cap;
  l.ones = l.rec + (size_t)r * (GP_MT_REC + d + 3);
  l.total = l.ones + m;
  return l;
}

__global__ __launch_bounds__(GP_T) void gp_mt_init_kernel(int m, int d, int r, int n_par, int max_iter,
                                                          const double *__restrict__ raw_g, double *info, double *ws) {
  const GpMtLayout lay = gp_mt_layout(m, d, r);
  const int tid = threadIdx.x, NP = r * n_par + 1;
  for (int i = tid; i < NP; i += GP_T) {
    ws[lay.m1 + i] = 0.0;
    ws[lay.m2 + i] = 0.0;
    info[4 + i] = NAN;
  }
  for (int i = tid; i < r; i += GP_T) info[4 + NP + i] = 0.0;
  for (int i = tid; i < m; i += GP_T) ws[lay.ones + i] = 1.0;
  if (tid == 0) {
    GpMtHead *h = reinterpret_cast<GpMtHead *>(ws + lay.head);
    h->phase = max_iter == 0 ? 1 : 0;
    h->count = 0; h->pad0 = 0; h->pad1 = 0;
    h->loss_old = 1e10; h->e = NAN; h->b1t = 1.0; h->b2t = 1.0;
    h->vg = gp_softplus(raw_g[0]) + 1e-4;
    info[0] = 0.0; info[1] = NAN; info[2] = NAN; info[3] = 0.0;
  }
}

__global__ __launch_bounds__(GP_T) void gp_mt_eval_kernel(const double *__restrict__ P0, int64_t ldp,
                                                          const double *__restrict__ Y, int64_t ldy, int m, int d, int code,
                                                          int flags, int n_par, const double *raw, double *s2, double *Kinv_all,
                                                          double *alpha_all, double *ws) {
  __shared__ GpSharedArd sh;
  __shared__ GpArdState st;
  const int q = blockIdx.x, r = gridDim.x, tid = threadIdx.x;
  const GpMtLayout lay = gp_mt_layout(m, d, r);
  const GpMtHead *h = reinterpret_cast<const GpMtHead *>(ws + lay.head);
  if (h->phase == 2) return;                                 // the same word in every thread of every workgroup
  const int L = (flags & 1) ? d : 1, S = (flags & 2) ? 1 : 0;
  const size_t mm = (size_t)m * m;
  double *A = ws + lay.slice * q, *X = A + mm, *Z = X + mm;
  double *rec = ws + lay.rec + (size_t)(GP_MT_REC + n_par) * q;
  if (tid == 0) gp_unpack(raw + (size_t)n_par * q, L, S, st.par);
  __syncthreads();
  double loss = 0.0, tw = 0.0;
  const int status = gp_evaluate_ard<true>(code, m, d, flags, P0, ldp, Y + q, ldy, ws + lay.ones, &h->vg, 0, st, Z, A, X,
                                           Kinv_all + mm * q, alpha_all + (size_t)m * q, sh, loss, &tw);
  if (tid == 0) {
    rec[0] = status == 0 ? loss : NAN;
    rec[1] = status;
    rec[2] = status == 0 ? tw : NAN;
    if (status == 0) gp_pack(st.grad, L, S, rec + GP_MT_REC);
    s2[q] = 1.0 * (gp_softplus(st.par[GP_N]) + 1e-4) + h->vg;   // the diagonal's w_i sig2 + v, the same operations
  }
}

__global__ __launch_bounds__(GP_T) void gp_mt_step_kernel(int m, int d, int r, int n_par, double *raw, double *raw_g, double lr,
                                                          int max_iter, double tol, double *info, double *trace, double *ws) {
  __shared__ int s_phase, s_failed, s_it;
  __shared__ double s_gg, s_step, s_sq2;
  const GpMtLayout lay = gp_mt_layout(m, d, r);
  const int tid = threadIdx.x, NP = r * n_par + 1, stride = GP_MT_REC + n_par;
  GpMtHead *h = reinterpret_cast<GpMtHead *>(ws + lay.head);
  const double *recs = ws + lay.rec;
  if (tid == 0) {
    const int phase = h->phase;
    int failed = 0;
    if (phase != 2) {
      double LOSS = 0.0, tws = 0.0;
      for (int q = 0; q < r; ++q) {                          // index order
        const int sq = (int)recs[(size_t)stride * q + 1];
        failed = sq > failed ? sq : failed;
        LOSS += recs[(size_t)stride * q];
        tws += recs[(size_t)stride * q + 2];
      }
      LOSS /= (double)r;
      if (failed) {
        for (int q = 0; q < r; ++q) info[4 + NP + q] = recs[(size_t)stride * q + 1];
        info[3] = failed;
        h->phase = 2;
      } else if (phase == 1) {
        info[1] = LOSS;
        h->phase = 2;
      } else {
        const double e = fabs(LOSS - h->loss_old);
        const int it = h->count;
        h->loss_old = LOSS;
        h->e = e;
        h->b1t *= 0.9;
        h->b2t *= 0.999;
        h->count = it + 1;
        if (trace != nullptr) trace[(size_t)it * (1 + NP)] = LOSS;
        info[0] = it + 1; info[1] = LOSS; info[2] = e;
        s_it = it;
        s_step = lr / (1.0 - h->b1t);
        s_sq2 = sqrt(1.0 - h->b2t);
        h->phase = (e <= tol || it + 1 >= max_iter) ? 1 : 0;
      }
      s_gg = gp_sigmoid(raw_g[0]) * (tws / (double)r);
    }
    s_phase = phase;
    s_failed = failed;
  }
  __syncthreads();
  if (s_phase == 2 || s_failed != 0) return;                 // LDS words: the same in every thread
  const bool step = s_phase == 0;
  double *m1 = ws + lay.m1, *m2 = ws + lay.m2;
  for (int idx = tid; idx < NP; idx += GP_T) {
    const bool own = idx < NP - 1;
    const int q = idx / n_par, c = idx - q * n_par;
    const double g = own ? recs[(size_t)stride * q + GP_MT_REC + c] / (double)r : s_gg;
    double *p = own ? raw + idx : raw_g;
    info[4 + idx] = g;
    if (step) {
      const double pv = *p;
      if (trace != nullptr) trace[(size_t)s_it * (1 + NP) + 1 + idx] = pv;
      const double a1 = 0.9 * m1[idx] + (1.0 - 0.9) * g;
      const double a2 = 0.999 * m2[idx] + (1.0 - 0.999) * g * g;
      const double denom = sqrt(a2) / s_sq2 + 1e-8;
      m1[idx] = a1;
      m2[idx] = a2;
      const double pn = pv - s_step * (a1 / denom);
      *p = pn;
      if (!own) h->vg = gp_softplus(pn) + 1e-4;
    }
  }
}

// ------------------------------------------------------------------------------------------------ state and append
// spr_gp_state_f64 is gp_train_ard_kernel<true> with max_iter = 0 -- the launch of spr_gp_train_noise_f64, hence its bits in K^-1,
// alpha and the info row -- followed by gp_state_finish_kernel, one workgroup per mode: X = L^-1 copied out of the mode's workspace
// slice as the factorisation left it (step 3 stores every entry of a row, the strict upper triangle as zeros) and
// log det K = 2 sum_j log R_jj from the factor's diagonal, per thread in a fixed assignment, closed by gp_block_sum.
__global__ __launch_bounds__(GP_T) void gp_state_finish_kernel(const double *__restrict__ ws, int m, int d, int n_par,
                                                               const double *__restrict__ info, double *__restrict__ X_all,
                                                               double *__restrict__ logdet_all) {
  __shared__ double red[4];
  __shared__ int failed;
  const int q = blockIdx.x, tid = threadIdx.x;
  const size_t mm = (size_t)m * m;
  if (tid == 0) failed = info[(size_t)(4 + n_par) * q + 3] != 0.0;
  __syncthreads();
  if (failed) {                                            // one LDS word decides for the whole workgroup
    if (tid == 0) logdet_all[q] = NAN;
    return;
  }
  const double *A = ws + (2 * mm + (size_t)m * d) * q, *X = A + mm;
  double *Xo = X_all + mm * q;
  for (size_t e = tid; e < mm; e += GP_T) Xo[e] = X[e];
  double part[1] = {0.0};
  for (int j = tid; j < m; j += GP_T) part[0] += log(A[(size_t)j * m + j]);
  gp_block_sum<1>(part, red);
  if (tid == 0) logdet_all[q] = 2.0 * part[0];
}

// Append k points to a factored state (GPR.update(append=True); spr_gp_append_f64).  K' = [[K, B], [B^T, C]], m' = m + k:
//   W = X B,  S = C - W^T W = Rs^T Rs,  N = Rs^-T [-W^T X, I]  (k x m': the new rows of X'),  X' = [[X, 0], N],
//   K'^-1 = [[K^-1, 0], [0, 0]] + N^T N,  logdet' = logdet + sum log(pivots of S),  alpha' = K'^-1 (y' - mu),  the loss of training.
// The top-left block of N^T N holds the terms X'^T X' has beyond X^T X, so K'^-1 is as accurate as a fresh product; K^-1 is never
// updated through its own Schur complement (that drifts).  B and C are formed from the scaled coordinates z = P0 / l as
// gp_train_ard_kernel forms K: with flags = 0 they differ from the distance-matrix route of gp_train_kernel by rounding only.
// Three launches, no workgroup waits for another, no atomics; the old X, K^-1 and logdet are read only.
//   1. gp_append_factor_kernel, one workgroup per mode: z, B^T (k x m), W^T = (X B)^T by 64 x 32 tiles of X read along its rows
//      (coalesced) and turned in LDS, S accumulated by the same tile product, factored in LDS (k <= 64), then N by threads that
//      own a column: the panel product W^T X (rows of X read coalesced, W^T staged through LDS in chunks of GP_KC) and a
//      forward substitution per column in registers, by block rows of GP_NB.  N goes to rows m.. of X', logdet' and the status
//      (a pivot <= m' 2^-53 C_jj: 1, not finite: 2, decided on the same LDS words by every thread) to their outputs.
//   2. gp_append_apply_kernel, one workgroup per (mode, GP_NB rows of K'^-1): K'^-1[i][j] = K^-1[i][j] + sum_t N[t][i] N[t][j] with t
//      ascending -- (i, j) and (j, i) add the same products in the same order onto the same bits: symmetric bit for bit --, rows
//      < m of X' (the old block copied, zeros right of it), and alpha' for its rows (a workgroup sum in a fixed order).
//   3. gp_append_loss_kernel, one workgroup per mode: res . alpha' in a fixed order, the loss.
// info row (4 doubles): m', loss, logdet', status.  A mode with status != 0 leaves its rows of X', K'^-1 and alpha' undefined.
constexpr int AP_MAX_K = SPR_GP_MAX_APPEND;
constexpr int AP_TR = 64;             // rows of a tile (= AP_MAX_K: the tile product serves S too)
constexpr int AP_TC = 32;             // contraction columns per tile
constexpr int AP_LDT = AP_TC + 1;     // row stride of a tile in LDS
constexpr int AP_LDS = AP_MAX_K + 1;  // row stride of S / Rs in LDS
constexpr int AP_NJ = AP_MAX_K / 4;   // outputs per thread of the tile product
static_assert(AP_TR == AP_MAX_K && AP_TR * AP_LDS <= 2 * AP_TR * AP_LDT, "S takes the place of the two tiles");

struct GpAppendShared {
  double tiles[2 * AP_TR * AP_LDT];   // the two tiles of steps W and S; then S / Rs (AP_MAX_K x AP_LDS)
  double stage[GP_KC * GP_LDP];       // a chunk of W^T for the panel product
  double cdiag[AP_MAX_K];             // the diagonal of C: the scale a pivot of S is judged against
  double par[GP_NPAR];
};

// acc[jj] += sum_cc Xs[a][cc] Bs[tg + 4 jj][cc], jj < nj: thread (a, tg) of a 64 x 4 arrangement, tg the wave
__device__ inline void gp_tile_mac(const double *Xs, const double *Bs, int a, int tg, int nj, double (&acc)[AP_NJ]) {
  for (int cc = 0; cc < AP_TC; ++cc) {
    const double xv = Xs[a * AP_LDT + cc];
#pragma unroll
    for (int jj = 0; jj < AP_NJ; ++jj)
      if (jj < nj) acc[jj] = fma(xv, Bs[(tg + 4 * jj) * AP_LDT + cc], acc[jj]);
  }
}

// acc[j] += sum_{k0 <= i < k1} X[i][col] Wt[tb + j][i], j < GP_NB: gp_panel_acc with the second factor stored transposed (k x m)
__device__ inline void gp_panel_acc_t(const double *__restrict__ X, const double *Wt, int m, int k, int k0, int k1, int col, bool cv,
                                      int tb, double *S, double (&acc)[GP_NB]) {
  for (int kc = k0; kc < k1; kc += GP_KC) {
    __syncthreads();
    for (int e = threadIdx.x; e < GP_KC * GP_NB; e += GP_T) {
      const int j = e / GP_KC, kk = e % GP_KC;
      S[kk * GP_LDP + j] = (kc + kk < k1 && tb + j < k) ? Wt[(tb + j) * m + kc + kk] : 0.0;
    }
    __syncthreads();
    if (cv) {
      const int kn = k1 - kc < GP_KC ? k1 - kc : GP_KC;
      for (int kk = 0; kk < kn; ++kk) {
        const double v = X[(kc + kk) * m + col];
#pragma unroll
        for (int j = 0; j < GP_NB; ++j) acc[j] = fma(v, S[kk * GP_LDP + j], acc[j]);
      }
    }
  }
}

// Steps of launch 1 for one mode.  -> 0, or the status of a failed pivot of S (the same in every thread).  Zs: d x m' scaled
// coordinates, Bt, Wt: k x m each (this mode's workspace slice); Xn: rows m.. of X' (k x m').
__device__ int gp_append_factor(int code, int m, int k, int d, int flags, const double *__restrict__ P0, int64_t ldp,
                                const double *__restrict__ w, const double *__restrict__ v, int64_t ldv,
                                const double *__restrict__ X, double *Zs, double *Bt, double *Wt, double *Xn, GpAppendShared &sh,
                                double &logdet_s) {
  const int tid = threadIdx.x, mp = m + k;
  const int a = tid & 63, tg = tid >> 6;
  const int nj = k > tg ? (k - tg + 3) / 4 : 0;
  const bool ard = (flags & 1) != 0, scl = (flags & 2) != 0;
  const double o = scl ? gp_softplus(sh.par[GP_O]) : 1.0, sig2 = gp_softplus(sh.par[GP_N]) + 1e-4;
  double *Xs = sh.tiles, *Bs = sh.tiles + AP_TR * AP_LDT, *Sm = sh.tiles;

  // z = P0 / l for all m' points, then B^T
  {
    double ell[GP_MAX_D];
    ell[0] = gp_softplus(sh.par[0]);
#pragma unroll
    for (int c = 1; c < GP_MAX_D; ++c) ell[c] = (ard && c < d) ? gp_softplus(sh.par[c]) : ell[0];
    for (int i = tid; i < mp; i += GP_T) {
      if (ard) {
#pragma unroll
        for (int c = 0; c < GP_MAX_D; ++c)
          if (c < d) Zs[c * mp + i] = P0[(int64_t)i * ldp + c] / ell[c];
      } else {
        for (int c = 0; c < d; ++c) Zs[c * mp + i] = P0[(int64_t)i * ldp + c] / ell[0];
      }
    }
  }
  __syncthreads();
  for (int t = 0; t < k; ++t)
    for (int i = tid; i < m; i += GP_T) {
      double kv, dk;
      gp_kern(code, gp_scaled_dist(Zs, mp, d, i, m + t), kv, dk);
      Bt[t * m + i] = o * kv;
    }

  // W^T = (X B)^T: 64 rows of X at a time against all k columns of B; X is zero right of its diagonal
  for (int i0 = 0; i0 < m; i0 += AP_TR) {
    double acc[AP_NJ];
#pragma unroll
    for (int jj = 0; jj < AP_NJ; ++jj) acc[jj] = 0.0;
    const int cend = i0 + AP_TR < m ? i0 + AP_TR : m;
    for (int c0 = 0; c0 < cend; c0 += AP_TC) {
      __syncthreads();               // the previous tiles are consumed; B^T written by other threads is visible
      for (int e = tid; e < AP_TR * AP_TC; e += GP_T) {
        const int ra = e / AP_TC, cc = e % AP_TC, c = c0 + cc;
        Xs[ra * AP_LDT + cc] = (i0 + ra < m && c < m) ? X[(i0 + ra) * m + c] : 0.0;
        Bs[ra * AP_LDT + cc] = (ra < k && c < m) ? Bt[ra * m + c] : 0.0;
      }
      __syncthreads();
      gp_tile_mac(Xs, Bs, a, tg, nj, acc);
    }
    if (i0 + a < m) {
#pragma unroll
      for (int jj = 0; jj < AP_NJ; ++jj)
        if (jj < nj) Wt[(tg + 4 * jj) * m + i0 + a] = acc[jj];
    }
  }

  // S = C - W^T W: thread (a, tg) holds S[a][tg + 4 jj]
  {
    double acc[AP_NJ];
#pragma unroll
    for (int jj = 0; jj < AP_NJ; ++jj) acc[jj] = 0.0;
    for (int i0 = 0; i0 < m; i0 += AP_TC) {
      __syncthreads();               // W^T written by other threads is visible
      for (int e = tid; e < AP_TR * AP_TC; e += GP_T) {
        const int t = e / AP_TC, ii = e % AP_TC;
        Xs[t * AP_LDT + ii] = (t < k && i0 + ii < m) ? Wt[t * m + i0 + ii] : 0.0;
      }
      __syncthreads();
      gp_tile_mac(Xs, Xs, a, tg, nj, acc);
    }
    __syncthreads();                 // the tiles are consumed: S takes their place
    if (a < k) {
#pragma unroll
      for (int jj = 0; jj < AP_NJ; ++jj)
        if (jj < nj) {
          const int u = tg + 4 * jj, lo = a < u ? a : u, hi = a < u ? u : a;
          double kv, dk;
          gp_kern(code, gp_scaled_dist(Zs, mp, d, m + lo, m + hi), kv, dk);
          const double c = a == u ? o * kv + (w[m + a] * sig2 + v[(int64_t)(m + a) * ldv]) : o * kv;
          if (a == u) sh.cdiag[a] = c;
          Sm[a * AP_LDS + u] = c - acc[jj];
        }
    }
    __syncthreads();
  }

  // S = Rs^T Rs in LDS, Rs upper triangular.  A pivot is what is left of C_jj after a cancellation that loses about m' eps C_jj:
  // at or below that it holds no correct digit (an exact copy of an exact point gives +- a few eps C_jj, of either sign) and
  // counts as not positive.
  logdet_s = 0.0;
  const double tol = (double)mp * 0x1p-53;
  for (int j = 0; j < k; ++j) {
    const double p = Sm[j * AP_LDS + j];                   // the same LDS words in every thread
    if (!(p > tol * sh.cdiag[j])) return (p != p || sh.cdiag[j] != sh.cdiag[j]) ? 2 : 1;
    if (!(p <= DBL_MAX)) return 2;
    const double s = sqrt(p);
    logdet_s += log(p);
    if (tid > j && tid < k) Sm[j * AP_LDS + tid] /= s;
    __syncthreads();
    for (int e = tid; e < k * k; e += GP_T) {
      const int ra = e / k, rb = e % k;
      if (ra > j && rb >= ra) Sm[ra * AP_LDS + rb] -= Sm[j * AP_LDS + ra] * Sm[j * AP_LDS + rb];
    }
    if (tid == 0) Sm[j * AP_LDS + j] = s;
    __syncthreads();
  }

  // N = Rs^-T [-W^T X, I] by block rows of GP_NB; a thread owns column c of X' and reads back only what it wrote itself
  const int ng = (mp + GP_T - 1) / GP_T;
  for (int g = 0; g < ng; ++g) {
    const int c = g * GP_T + tid;
    const bool cv = c < mp;
    for (int tb = 0; tb < k; tb += GP_NB) {
      const int nb = k - tb < GP_NB ? k - tb : GP_NB;
      double x[GP_NB];
#pragma unroll
      for (int j = 0; j < GP_NB; ++j) x[j] = 0.0;
      gp_panel_acc_t(X, Wt, m, k, g * GP_T, m, c, c < m, tb, sh.stage, x);    // rows of X from the group's first column on
      if (cv) {
#pragma unroll
        for (int j = 0; j < GP_NB; ++j) x[j] = c < m ? -x[j] : (c - m == tb + j ? 1.0 : 0.0);
        for (int u = 0; u < tb; ++u) {
          const double nu = Xn[u * mp + c];
#pragma unroll
          for (int j = 0; j < GP_NB; ++j)
            if (j < nb) x[j] = fma(-Sm[u * AP_LDS + tb + j], nu, x[j]);
        }
#pragma unroll
        for (int j = 0; j < GP_NB; ++j)
          if (j < nb) {
            double s = x[j];
#pragma unroll
            for (int kk = 0; kk < j; ++kk) s = fma(-Sm[(tb + kk) * AP_LDS + tb + j], x[kk], s);
            x[j] = s / Sm[(tb + j) * AP_LDS + tb + j];
          }
#pragma unroll
        for (int j = 0; j < GP_NB; ++j)
          if (j < nb) Xn[(tb + j) * mp + c] = x[j];
      }
    }
  }
  return 0;
}

__global__ __launch_bounds__(GP_T) void gp_append_factor_kernel(const double *__restrict__ P0, int64_t ldp,
                                                                const double *__restrict__ w, const double *__restrict__ V,
                                                                int64_t ldv, int m, int k, int d, int code, int flags, int n_par,
                                                                const double *__restrict__ raw, const double *__restrict__ X_all,
                                                                const double *__restrict__ logdet_all, double *X2_all,
                                                                double *logdet2_all, double *info, double *ws) {
  __shared__ GpAppendShared sh;
  const int q = blockIdx.x, tid = threadIdx.x, mp = m + k;
  const int L = (flags & 1) ? d : 1, S = (flags & 2) ? 1 : 0;
  double *Zs = ws + ((size_t)d * mp + 2 * (size_t)k * m) * q, *Bt = Zs + (size_t)d * mp, *Wt = Bt + (size_t)k * m;
  if (tid == 0) gp_unpack(raw + (size_t)n_par * q, L, S, sh.par);
  __syncthreads();
  double logdet_s = 0.0;
  const int status = gp_append_factor(code, m, k, d, flags, P0, ldp, w, V + q, ldv, X_all + (size_t)m * m * q, Zs, Bt, Wt,
                                      X2_all + (size_t)mp * mp * q + (size_t)m * mp, sh, logdet_s);
  if (tid == 0) {
    const double ld = status == 0 ? logdet_all[q] + logdet_s : NAN;
    logdet2_all[q] = ld;
    info[4 * q] = mp; info[4 * q + 1] = NAN; info[4 * q + 2] = ld; info[4 * q + 3] = status;
  }
}

__global__ __launch_bounds__(GP_T) void gp_append_apply_kernel(const double *__restrict__ Y, int64_t ldy, int m, int k, int n_par,
                                                               const double *__restrict__ raw, const double *__restrict__ X_all,
                                                               const double *__restrict__ Kinv_all, const double *info,
                                                               double *X2_all, double *Kinv2_all, double *alpha2_all) {
  __shared__ double Ni[AP_MAX_K * GP_NB];
  __shared__ double red[4 * GP_NB];
  __shared__ int failed;
  const int q = blockIdx.x, i0 = blockIdx.y * GP_NB, tid = threadIdx.x, mp = m + k;
  if (tid == 0) failed = info[4 * q + 3] != 0.0;
  __syncthreads();
  if (failed) return;                                      // one LDS word decides for the whole workgroup
  const double *X = X_all + (size_t)m * m * q, *Kinv = Kinv_all + (size_t)m * m * q;
  double *X2 = X2_all + (size_t)mp * mp * q, *Kinv2 = Kinv2_all + (size_t)mp * mp * q;
  const double *N = X2 + (size_t)m * mp;                   // written by launch 1; this launch writes rows < m only
  for (int e = tid; e < k * GP_NB; e += GP_T) {
    const int i = i0 + e % GP_NB;
    Ni[e] = i < mp ? N[(e / GP_NB) * mp + i] : 0.0;
  }
  __syncthreads();
  const double mu = raw[(size_t)n_par * q + n_par - 1];
  double part[GP_NB];
#pragma unroll
  for (int j = 0; j < GP_NB; ++j) part[j] = 0.0;
  for (int c = tid; c < mp; c += GP_T) {
    double acc[GP_NB];
#pragma unroll
    for (int j = 0; j < GP_NB; ++j) acc[j] = (i0 + j < m && c < m) ? Kinv[(i0 + j) * m + c] : 0.0;
    for (int t = 0; t < k; ++t) {
      const double nc = N[t * mp + c];
#pragma unroll
      for (int j = 0; j < GP_NB; ++j) acc[j] = fma(Ni[t * GP_NB + j], nc, acc[j]);
    }
    const double res = Y[(int64_t)c * ldy + q] - mu;
#pragma unroll
    for (int j = 0; j < GP_NB; ++j)
      if (i0 + j < mp) {
        Kinv2[(i0 + j) * mp + c] = acc[j];
        part[j] = fma(acc[j], res, part[j]);
        if (i0 + j < m) X2[(i0 + j) * mp + c] = c < m ? X[(i0 + j) * m + c] : 0.0;
      }
  }
  gp_block_sum<GP_NB>(part, red);
#pragma unroll
  for (int j = 0; j < GP_NB; ++j)
    if (tid == j && i0 + j < mp) alpha2_all[(size_t)mp * q + i0 + j] = part[j];
}

__global__ __launch_bounds__(GP_T) void gp_append_loss_kernel(const double *__restrict__ Y, int64_t ldy, int mp, int n_par,
                                                              const double *__restrict__ raw,
                                                              const double *__restrict__ alpha2_all, double *info) {
  __shared__ double red[4];
  __shared__ int failed;
  const int q = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) failed = info[4 * q + 3] != 0.0;
  __syncthreads();
  if (failed) return;
  const double mu = raw[(size_t)n_par * q + n_par - 1];
  double part[1] = {0.0};
  for (int i = tid; i < mp; i += GP_T) part[0] += (Y[(int64_t)i * ldy + q] - mu) * alpha2_all[(size_t)mp * q + i];
  gp_block_sum<1>(part, red);
  const double dm = (double)mp;
  if (tid == 0) info[4 * q + 1] = (0.5 * part[0] + 0.5 * info[4 * q + 2] + 0.5 * dm * log(2.0 * M_PI)) / dm;
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


size_t gp_workspace_ard(int32_t m, int32_t d, int32_t r) {
  if (m < 1 || m > GP_MAX_M || d < 1 || r < 1) return 0;
  return sizeof(double) * (size_t)r * (2 * (size_t)m * m + (size_t)m * d);
}

// spr_gp_train_ard_f64 (noise false: d_w, d_V, ldv are not looked at) and spr_gp_train_noise_f64: the same checks in the same
// order, the same workspace, one kernel template.
int gp_train_ard_any(const char *name, bool noise, const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y,
                     int32_t r, int64_t ldy, const double *d_w, const double *d_V, int64_t ldv, int32_t kernel, int32_t flags,
                     double *d_raw, double lr, int32_t max_iter, double tol, double *d_Kinv, double *d_alpha, double *d_info,
                     double *d_trace, void *d_workspace, size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_P0 && d_Y && d_raw && d_Kinv && d_alpha && d_info && d_workspace && (!noise || (d_w && d_V)), SPR_E_INVALID,
              "%s: NULL pointer", name);
  SPR_REQUIRE(m > 0 && d > 0 && r > 0 && ldp >= d && ldy >= r && max_iter >= 0, SPR_E_INVALID,
              "%s: bad shape m=%d d=%d ldp=%lld r=%d ldy=%lld max_iter=%d", name, m, d, (long long)ldp, r, (long long)ldy,
              max_iter);
  SPR_REQUIRE(!noise || ldv >= r, SPR_E_INVALID, "%s: bad shape r=%d ldv=%lld", name, r, (long long)ldv);
  SPR_REQUIRE(kernel >= SPR_GP_MATERN52 && kernel <= SPR_GP_RBF, SPR_E_INVALID, "%s: unknown kernel code %d", name, kernel);
  SPR_REQUIRE(flags >= 0 && flags <= 3, SPR_E_INVALID, "%s: flags = %d outside 0..3 (bit 0 ARD, bit 1 output scale)", name, flags);
  SPR_REQUIRE(lr > 0.0 && lr <= DBL_MAX && tol >= 0.0 && tol <= DBL_MAX, SPR_E_INVALID,
              "%s: lr = %g must be positive and tol = %g non-negative, both finite", name, lr, tol);
  SPR_REQUIRE(m <= GP_MAX_M, SPR_E_UNSUPPORTED, "%s: m = %d exceeds %d", name, m, GP_MAX_M);
  SPR_REQUIRE(!(flags & 1) || d <= GP_MAX_D, SPR_E_UNSUPPORTED, "%s: ARD over d = %d coordinates exceeds %d", name, d, GP_MAX_D);
  SPR_REQUIRE(workspace_bytes >= gp_workspace_ard(m, d, r), SPR_E_INVALID, "%s: workspace of %zu bytes, %zu needed", name,
              workspace_bytes, gp_workspace_ard(m, d, r));
  SPR_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, SPR_E_INVALID, "%s: workspace must be 8-byte aligned", name);
  const int n_par = ((flags & 1) ? d : 1) + ((flags & 2) ? 1 : 0) + 2;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *ws = static_cast<double *>(d_workspace);
  if (noise) {
    hipLaunchKernelGGL(gp_train_ard_kernel<true>, dim3(r), dim3(GP_T), 0, st, d_P0, ldp, d_Y, ldy, d_w, d_V, ldv, (int)m, (int)d,
                       (int)kernel, (int)flags, n_par, d_raw, lr, (int)max_iter, tol, d_Kinv, d_alpha, d_info, d_trace, ws);
  } else {
    hipLaunchKernelGGL(gp_train_ard_kernel<false>, dim3(r), dim3(GP_T), 0, st, d_P0, ldp, d_Y, ldy,
                       static_cast<const double *>(nullptr), static_cast<const double *>(nullptr), (int64_t)0, (int)m, (int)d,
                       (int)kernel, (int)flags, n_par, d_raw, lr, (int)max_iter, tol, d_Kinv, d_alpha, d_info, d_trace, ws);
  }
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

int gp_train_ard(const char *name, const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r,
                 int64_t ldy, int32_t kernel, int32_t flags, double *d_raw, double lr, int32_t max_iter, double tol,
                 double *d_Kinv, double *d_alpha, double *d_info, double *d_trace, void *d_workspace, size_t workspace_bytes,
                 void *stream) {
  return gp_train_ard_any(name, false, d_P0, m, d, ldp, d_Y, r, ldy, nullptr, nullptr, 0, kernel, flags, d_raw, lr, max_iter, tol,
                          d_Kinv, d_alpha, d_info, d_trace, d_workspace, workspace_bytes, stream);
}

int gp_train_noise(const char *name, const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r,
                   int64_t ldy, const double *d_w, const double *d_V, int64_t ldv, int32_t kernel, int32_t flags, double *d_raw,
                   double lr, int32_t max_iter, double tol, double *d_Kinv, double *d_alpha, double *d_info, double *d_trace,
                   void *d_workspace, size_t workspace_bytes, void *stream) {
  return gp_train_ard_any(name, true, d_P0, m, d, ldp, d_Y, r, ldy, d_w, d_V, ldv, kernel, flags, d_raw, lr, max_iter, tol, d_Kinv,
                          d_alpha, d_info, d_trace, d_workspace, workspace_bytes, stream);
}

// spr_gp_state_f64: the checks of spr_gp_train_noise_f64 in their order (no lr, max_iter, tol), its launch, then the two further outputs
int gp_state(const char *name, const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy,
             const double *d_w, const double *d_V, int64_t ldv, int32_t kernel, int32_t flags, double *d_raw, double *d_Kinv,
             double *d_alpha, double *d_info, double *d_X, double *d_logdet, void *d_workspace, size_t workspace_bytes,
             void *stream) {
  SPR_REQUIRE(d_P0 && d_Y && d_raw && d_Kinv && d_alpha && d_info && d_workspace && d_w && d_V && d_X && d_logdet, SPR_E_INVALID,
              "%s: NULL pointer", name);
  SPR_REQUIRE(m > 0 && d > 0 && r > 0 && ldp >= d && ldy >= r, SPR_E_INVALID, "%s: bad shape m=%d d=%d ldp=%lld r=%d ldy=%lld",
              name, m, d, (long long)ldp, r, (long long)ldy);
  SPR_REQUIRE(ldv >= r, SPR_E_INVALID, "%s: bad shape r=%d ldv=%lld", name, r, (long long)ldv);
  SPR_REQUIRE(kernel >= SPR_GP_MATERN52 && kernel <= SPR_GP_RBF, SPR_E_INVALID, "%s: unknown kernel code %d", name, kernel);
  SPR_REQUIRE(flags >= 0 && flags <= 3, SPR_E_INVALID, "%s: flags = %d outside 0..3 (bit 0 ARD, bit 1 output scale)", name, flags);
  SPR_REQUIRE(m <= GP_MAX_M, SPR_E_UNSUPPORTED, "%s: m = %d exceeds %d", name, m, GP_MAX_M);
  SPR_REQUIRE(!(flags & 1) || d <= GP_MAX_D, SPR_E_UNSUPPORTED, "%s: ARD over d = %d coordinates exceeds %d", name, d, GP_MAX_D);
  SPR_REQUIRE(workspace_bytes >= gp_workspace_ard(m, d, r), SPR_E_INVALID, "%s: workspace of %zu bytes, %zu needed", name,
              workspace_bytes, gp_workspace_ard(m, d, r));
  SPR_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, SPR_E_INVALID, "%s: workspace must be 8-byte aligned", name);
  const int n_par = ((flags & 1) ? d : 1) + ((flags & 2) ? 1 : 0) + 2;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *ws = static_cast<double *>(d_workspace);
  hipLaunchKernelGGL(gp_train_ard_kernel<true>, dim3(r), dim3(GP_T), 0, st, d_P0, ldp, d_Y, ldy, d_w, d_V, ldv, (int)m, (int)d,
                     (int)kernel, (int)flags, n_par, d_raw, 0.1, 0, 0.0, d_Kinv, d_alpha, d_info, static_cast<double *>(nullptr), ws);
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gp_state_finish_kernel, dim3(r), dim3(GP_T), 0, st, static_cast<const double *>(ws), (int)m, (int)d, n_par,
                     static_cast<const double *>(d_info), d_X, d_logdet);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

// per mode: z (d x m'), B^T and W^T (k x m each, counted as k x m')
size_t gp_workspace_append(int32_t m_new, int32_t d, int32_t k, int32_t r) {
  if (k < 1 || k > AP_MAX_K || m_new <= k || m_new > GP_MAX_M || d < 1 || r < 1) return 0;
  return sizeof(double) * (size_t)r * ((size_t)d * m_new + 2 * (size_t)k * m_new);
}

// m: rows of P0 / Y / w / V (= m'), the last k of them new; the state is that of the first m - k
int gp_append(const char *name, const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy,
              const double *d_w, const double *d_V, int64_t ldv, int32_t k, int32_t kernel, int32_t flags, const double *d_raw,
              const double *d_X, const double *d_Kinv, const double *d_logdet, double *d_X2, double *d_Kinv2, double *d_alpha2,
              double *d_logdet2, double *d_info, void *d_workspace, size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_P0 && d_Y && d_w && d_V && d_raw && d_X && d_Kinv && d_logdet && d_X2 && d_Kinv2 && d_alpha2 && d_logdet2 &&
                  d_info && d_workspace, SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(m > 0 && d > 0 && r > 0 && ldp >= d && ldy >= r, SPR_E_INVALID, "%s: bad shape m=%d d=%d ldp=%lld r=%d ldy=%lld",
              name, m, d, (long long)ldp, r, (long long)ldy);
  SPR_REQUIRE(ldv >= r, SPR_E_INVALID, "%s: bad shape r=%d ldv=%lld", name, r, (long long)ldv);
  SPR_REQUIRE(k >= 1 && k < m, SPR_E_INVALID, "%s: k = %d new rows of m = %d (1 <= k < m)", name, k, m);
  SPR_REQUIRE(kernel >= SPR_GP_MATERN52 && kernel <= SPR_GP_RBF, SPR_E_INVALID, "%s: unknown kernel code %d", name, kernel);
  SPR_REQUIRE(flags >= 0 && flags <= 3, SPR_E_INVALID, "%s: flags = %d outside 0..3 (bit 0 ARD, bit 1 output scale)", name, flags);
  SPR_REQUIRE(k <= AP_MAX_K, SPR_E_UNSUPPORTED, "%s: k = %d new rows exceed %d per call", name, k, AP_MAX_K);
  SPR_REQUIRE(m <= GP_MAX_M, SPR_E_UNSUPPORTED, "%s: m = %d exceeds %d", name, m, GP_MAX_M);
  SPR_REQUIRE(!(flags & 1) || d <= GP_MAX_D, SPR_E_UNSUPPORTED, "%s: ARD over d = %d coordinates exceeds %d", name, d, GP_MAX_D);
  SPR_REQUIRE(workspace_bytes >= gp_workspace_append(m, d, k, r), SPR_E_INVALID, "%s: workspace of %zu bytes, %zu needed", name,
              workspace_bytes, gp_workspace_append(m, d, k, r));
  SPR_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, SPR_E_INVALID, "%s: workspace must be 8-byte aligned", name);
  const int n_par = ((flags & 1) ? d : 1) + ((flags & 2) ? 1 : 0) + 2;
  const int m_old = m - k, nblk = (m + GP_NB - 1) / GP_NB;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(gp_append_factor_kernel, dim3(r), dim3(GP_T), 0, st, d_P0, ldp, d_w, d_V, ldv, m_old, (int)k, (int)d,
                     (int)kernel, (int)flags, n_par, d_raw, d_X, d_logdet, d_X2, d_logdet2, d_info,
                     static_cast<double *>(d_workspace));
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gp_append_apply_kernel, dim3(r, nblk), dim3(GP_T), 0, st, d_Y, ldy, m_old, (int)k, n_par, d_raw, d_X, d_Kinv,
                     static_cast<const double *>(d_info), d_X2, d_Kinv2, d_alpha2);
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gp_append_loss_kernel, dim3(r), dim3(GP_T), 0, st, d_Y, ldy, (int)m, n_par, d_raw,
                     static_cast<const double *>(d_alpha2), d_info);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

int gp_predict_ard(const char *name, const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Pstar,
                   int32_t n_p, int64_t ldps, int32_t kernel, int32_t flags, const double *d_raw, int32_t r,
                   const double *d_Kinv, const double *d_alpha, double *d_mean, double *d_var, void *stream) {
  SPR_REQUIRE(d_P0 && d_Pstar && d_raw && d_Kinv && d_alpha && d_mean && d_var, SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(m > 0 && d > 0 && r > 0 && n_p > 0 && ldp >= d && ldps >= d, SPR_E_INVALID,
              "%s: bad shape m=%d d=%d ldp=%lld n_p=%d ldps=%lld r=%d", name, m, d, (long long)ldp, n_p, (long long)ldps, r);
  SPR_REQUIRE(kernel >= SPR_GP_MATERN52 && kernel <= SPR_GP_RBF, SPR_E_INVALID, "%s: unknown kernel code %d", name, kernel);
  SPR_REQUIRE(flags >= 0 && flags <= 3, SPR_E_INVALID, "%s: flags = %d outside 0..3 (bit 0 ARD, bit 1 output scale)", name, flags);
  SPR_REQUIRE(m <= GP_MAX_M, SPR_E_UNSUPPORTED, "%s: m = %d exceeds %d", name, m, GP_MAX_M);
  SPR_REQUIRE(!(flags & 1) || d <= GP_MAX_D, SPR_E_UNSUPPORTED, "%s: ARD over d = %d coordinates exceeds %d", name, d, GP_MAX_D);
  const int nblk = (n_p + GP_PB - 1) / GP_PB;
  SPR_REQUIRE(nblk <= 65535, SPR_E_UNSUPPORTED, "%s: n_p = %d exceeds %d test points per call", name, n_p, 65535 * GP_PB);
  const int n_par = ((flags & 1) ? d : 1) + ((flags & 2) ? 1 : 0) + 2;
  hipLaunchKernelGGL(gp_predict_ard_kernel, dim3(r, nblk), dim3(GP_T), 0, static_cast<hipStream_t>(stream), d_P0, (int)m, (int)d,
                     ldp, d_Pstar, (int)n_p, ldps, (int)kernel, (int)flags, n_par, d_raw, d_Kinv, d_alpha, d_mean, d_var, (int)r,
                     static_cast<const double *>(nullptr));
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

size_t gp_workspace_mt(int32_t m, int32_t d, int32_t r) {
  if (m < 1 || m > GP_MAX_M || d < 1 || r < 1) return 0;
  return sizeof(double) * gp_mt_layout(m, d, r).total;
}

// spr_gp_train_mt_f64: the checks of spr_gp_train_ard_f64 in their order, then the chain of launches.  The only entry point of
// the file that waits for the stream: it reads the phase word after every chunk.
int gp_train_mt(const char *name, const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r,
                int64_t ldy, int32_t kernel, int32_t flags, double *d_raw, double *d_raw_g, double lr, int32_t max_iter,
                double tol, double *d_s2, double *d_Kinv, double *d_alpha, double *d_info, double *d_trace, void *d_workspace,
                size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_P0 && d_Y && d_raw && d_raw_g && d_s2 && d_Kinv && d_alpha && d_info && d_workspace, SPR_E_INVALID,
              "%s: NULL pointer", name);
  SPR_REQUIRE(m > 0 && d > 0 && r > 0 && ldp >= d && ldy >= r && max_iter >= 0, SPR_E_INVALID,
              "%s: bad shape m=%d d=%d ldp=%lld r=%d ldy=%lld max_iter=%d", name, m, d, (long long)ldp, r, (long long)ldy,
              max_iter);
  SPR_REQUIRE(kernel >= SPR_GP_MATERN52 && kernel <= SPR_GP_RBF, SPR_E_INVALID, "%s: unknown kernel code %d", name, kernel);
  SPR_REQUIRE(flags >= 0 && flags <= 3, SPR_E_INVALID, "%s: flags = %d outside 0..3 (bit 0 ARD, bit 1 output scale)", name, flags);
  SPR_REQUIRE(lr > 0.0 && lr <= DBL_MAX && tol >= 0.0 && tol <= DBL_MAX, SPR_E_INVALID,
              "%s: lr = %g must be positive and tol = %g non-negative, both finite", name, lr, tol);
  SPR_REQUIRE(m <= GP_MAX_M, SPR_E_UNSUPPORTED, "%s: m = %d exceeds %d", name, m, GP_MAX_M);
  SPR_REQUIRE(!(flags & 1) || d <= GP_MAX_D, SPR_E_UNSUPPORTED, "%s: ARD over d = %d coordinates exceeds %d", name, d, GP_MAX_D);
  SPR_REQUIRE(workspace_bytes >= gp_workspace_mt(m, d, r), SPR_E_INVALID, "%s: workspace of %zu bytes, %zu needed", name,
              workspace_bytes, gp_workspace_mt(m, d, r));
  SPR_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, SPR_E_INVALID, "%s: workspace must be 8-byte aligned", name);
  const int n_par = ((flags & 1) ? d : 1) + ((flags & 2) ? 1 : 0) + 2;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *ws = static_cast<double *>(d_workspace);
  const GpMtLayout lay = gp_mt_layout(m, d, r);
  hipLaunchKernelGGL(gp_mt_init_kernel, dim3(1), dim3(GP_T), 0, st, (int)m, (int)d, (int)r, n_par, (int)max_iter,
                     static_cast<const double *>(d_raw_g), d_info, ws);
  SPR_LAUNCH_CHECK();
  int64_t left = (int64_t)max_iter + 1;      // max_iter evaluations with a step and the one at the parameters kept
  int phase = 0;
  while (left > 0 && phase != 2) {
    const int n = left < SPR_GP_MT_CHUNK ? (int)left : SPR_GP_MT_CHUNK;
    for (int k = 0; k < n; ++k) {
      hipLaunchKernelGGL(gp_mt_eval_kernel, dim3(r), dim3(GP_T), 0, st, d_P0, ldp, d_Y, ldy, (int)m, (int)d, (int)kernel, (int)flags,
                         n_par, static_cast<const double *>(d_raw), d_s2, d_Kinv, d_alpha, ws);
      SPR_LAUNCH_CHECK();
      hipLaunchKernelGGL(gp_mt_step_kernel, dim3(1), dim3(GP_T), 0, st, (int)m, (int)d, (int)r, n_par, d_raw, d_raw_g, lr,
                         (int)max_iter, tol, d_info, d_trace, ws);
      SPR_LAUNCH_CHECK();
    }
    left -= n;
    SPR_HIP_TRY(hipMemcpyAsync(&phase, ws + lay.head, sizeof(int), hipMemcpyDeviceToHost, st));
    SPR_HIP_TRY(hipStreamSynchronize(st));
  }
  SPR_REQUIRE(phase == 2, SPR_E_HIP, "%s: the launch chain ended in phase %d", name, phase);
  return SPR_OK;
}

int gp_predict_mt(const char *name, const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Pstar, int32_t n_p,
                  int64_t ldps, int32_t kernel, int32_t flags, const double *d_raw, const double *d_s2, int32_t r,
                  const double *d_Kinv, const double *d_alpha, double *d_mean, double *d_var, void *stream) {
  SPR_REQUIRE(d_P0 && d_Pstar && d_raw && d_s2 && d_Kinv && d_alpha && d_mean && d_var, SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(m > 0 && d > 0 && r > 0 && n_p > 0 && ldp >= d && ldps >= d, SPR_E_INVALID,
              "%s: bad shape m=%d d=%d ldp=%lld n_p=%d ldps=%lld r=%d", name, m, d, (long long)ldp, n_p, (long long)ldps, r);
  SPR_REQUIRE(kernel >= SPR_GP_MATERN52 && kernel <= SPR_GP_RBF, SPR_E_INVALID, "%s: unknown kernel code %d", name, kernel);
  SPR_REQUIRE(flags >= 0 && flags <= 3, SPR_E_INVALID, "%s: flags = %d outside 0..3 (bit 0 ARD, bit 1 output scale)", name, flags);
  SPR_REQUIRE(m <= GP_MAX_M, SPR_E_UNSUPPORTED, "%s: m = %d exceeds %d", name, m, GP_MAX_M);
  SPR_REQUIRE(!(flags & 1) || d <= GP_MAX_D, SPR_E_UNSUPPORTED, "%s: ARD over d = %d coordinates exceeds %d", name, d, GP_MAX_D);
  const int nblk = (n_p + GP_PB - 1) / GP_PB;
  SPR_REQUIRE(nblk <= 65535, SPR_E_UNSUPPORTED, "%s: n_p = %d exceeds %d test points per call", name, n_p, 65535 * GP_PB);
  const int n_par = ((flags & 1) ? d : 1) + ((flags & 2) ? 1 : 0) + 2;
  hipLaunchKernelGGL(gp_predict_ard_kernel, dim3(r, nblk), dim3(GP_T), 0, static_cast<hipStream_t>(stream), d_P0, (int)m, (int)d,
                     ldp, d_Pstar, (int)n_p, ldps, (int)kernel, (int)flags, n_par, d_raw, d_Kinv, d_alpha, d_mean, d_var, (int)r,
                     d_s2);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

}  // namespace

extern "C" size_t spr_gp_workspace_mt(int32_t m, int32_t d, int32_t r) { return gp_workspace_mt(m, d, r); }

SPR_ENTRY(spr_gp_train_mt_f64,
          (const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy, int32_t kernel,
           int32_t flags, double *d_raw, double *d_raw_g, double lr, int32_t max_iter, double tol, double *d_s2, double *d_Kinv,
           double *d_alpha, double *d_info, double *d_trace, void *d_workspace, size_t workspace_bytes, void *stream),
          gp_train_mt, d_P0, m, d, ldp, d_Y, r, ldy, kernel, flags, d_raw, d_raw_g, lr, max_iter, tol, d_s2, d_Kinv, d_alpha,
          d_info, d_trace, d_workspace, workspace_bytes, stream)

SPR_ENTRY(spr_gp_predict_mt_f64,
          (const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Pstar, int32_t n_p, int64_t ldps,
           int32_t kernel, int32_t flags, const double *d_raw, const double *d_s2, int32_t r, const double *d_Kinv,
           const double *d_alpha, double *d_mean, double *d_var, void *stream),
          gp_predict_mt, d_P0, m, d, ldp, d_Pstar, n_p, ldps, kernel, flags, d_raw, d_s2, r, d_Kinv, d_alpha, d_mean, d_var, stream)

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

extern "C" size_t spr_gp_workspace_ard(int32_t m, int32_t d, int32_t r) { return gp_workspace_ard(m, d, r); }

SPR_ENTRY(spr_gp_train_ard_f64,
          (const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy, int32_t kernel,
           int32_t flags, double *d_raw, double lr, int32_t max_iter, double tol, double *d_Kinv, double *d_alpha,
           double *d_info, double *d_trace, void *d_workspace, size_t workspace_bytes, void *stream),
          gp_train_ard, d_P0, m, d, ldp, d_Y, r, ldy, kernel, flags, d_raw, lr, max_iter, tol, d_Kinv, d_alpha, d_info, d_trace,
          d_workspace, workspace_bytes, stream)

SPR_ENTRY(spr_gp_train_noise_f64,
          (const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy, const double *d_w,
           const double *d_V, int64_t ldv, int32_t kernel, int32_t flags, double *d_raw, double lr, int32_t max_iter, double tol,
           double *d_Kinv, double *d_alpha, double *d_info, double *d_trace, void *d_workspace, size_t workspace_bytes,
           void *stream),
          gp_train_noise, d_P0, m, d, ldp, d_Y, r, ldy, d_w, d_V, ldv, kernel, flags, d_raw, lr, max_iter, tol, d_Kinv, d_alpha,
          d_info, d_trace, d_workspace, workspace_bytes, stream)

SPR_ENTRY(spr_gp_state_f64,
          (const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy, const double *d_w,
           const double *d_V, int64_t ldv, int32_t kernel, int32_t flags, double *d_raw, double *d_Kinv, double *d_alpha,
           double *d_info, double *d_X, double *d_logdet, void *d_workspace, size_t workspace_bytes, void *stream),
          gp_state, d_P0, m, d, ldp, d_Y, r, ldy, d_w, d_V, ldv, kernel, flags, d_raw, d_Kinv, d_alpha, d_info, d_X, d_logdet,
          d_workspace, workspace_bytes, stream)

extern "C" size_t spr_gp_workspace_append(int32_t m_new, int32_t d, int32_t k, int32_t r) {
  return gp_workspace_append(m_new, d, k, r);
}

SPR_ENTRY(spr_gp_append_f64,
          (const double *d_P0, int32_t m_new, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy,
           const double *d_w, const double *d_V, int64_t ldv, int32_t k, int32_t kernel, int32_t flags, const double *d_raw,
           const double *d_X, const double *d_Kinv, const double *d_logdet, double *d_X2, double *d_Kinv2, double *d_alpha2,
           double *d_logdet2, double *d_info, void *d_workspace, size_t workspace_bytes, void *stream),
          gp_append, d_P0, m_new, d, ldp, d_Y, r, ldy, d_w, d_V, ldv, k, kernel, flags, d_raw, d_X, d_Kinv, d_logdet, d_X2, d_Kinv2,
          d_alpha2, d_logdet2, d_info, d_workspace, workspace_bytes, stream)

SPR_ENTRY(spr_gp_predict_ard_f64,
          (const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Pstar, int32_t n_p, int64_t ldps,
           int32_t kernel, int32_t flags, const double *d_raw, int32_t r, const double *d_Kinv, const double *d_alpha,
           double *d_mean, double *d_var, void *stream),
          gp_predict_ard, d_P0, m, d, ldp, d_Pstar, n_p, ldps, kernel, flags, d_raw, r, d_Kinv, d_alpha, d_mean, d_var, stream)
