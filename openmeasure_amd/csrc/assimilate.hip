// SPR.assimilate: the Bayesian update of a Gaussian prior on the POD coefficients with a vector of sensor readings -- one
// 256-thread workgroup per measurement vector, as in solve_ols_kernel.
//
// Model (scaled units of predict): y0 = (y - cnt) / scl, sig0 = sigma / scl, W = diag(1 / sig0), prior a ~ N(a0, C C^T) with
// C = diag(prior sigma) (r x r) or a given factor (r x q).  With B = W Theta C and res = y0 - Theta a0 the kernel forms the
// augmented Gram matrix of [B | W res] (s x (q+1)) with v_mfma_f64_16x16x4_f64 (sensors = contraction index), adds the
// identity, factors H' = I + B^T B = L' L'^T in LDS, solves z = H'^-1 B^T W res, forms X = L'^-1 in the unused upper triangle
// of the factor, and writes
//   a = a0 + C z,   F = C X^T  (cov = F F^T),   std = sqrt(diag(F F^T)),
//   chi2 = |W res|^2 - |L'^-1 B^T W res|^2,   logdet = sum log sig0^2 + 2 sum log L'_jj,   cond = (max L'_jj / min L'_jj)^2.
// H' has every eigenvalue >= 1, so there is no rank decision, no equilibration and no pseudo-inverse route for s < r.
// The diagonal prior is a column scale applied when a panel is loaded; for the factor form a small kernel first forms
// [Theta C_p | Theta a0_p] per vector into the workspace and the main kernel reads that as its design matrix (per-vector
// stride; 0 for the shared Theta), C is applied again in the epilogue from global memory.
// No atomics, fixed summation orders: two runs agree bit for bit.  Every barrier is outside divergent control flow; trip
// counts depend on the shape only.
// The file is self-contained: SolveCfg / tri_coords of solve.hip are repeated here (with q + 1 augmented columns, not
// r + 2) so that solve.hip and the code generated for it stay exactly as they are.
#include "common.hpp"
#include "launch.hpp"

namespace {

constexpr int AS_THREADS = 256;
constexpr int AS_WAVES = AS_THREADS / 64;

template <int NT> struct AssimCfg {
  static constexpr int NAP = 16 * NT;                            // padded augmented width
  static constexpr int CP = NAP + ((NT % 2 == 0) ? 16 : 0);      // LDS row stride (== 16 mod 32)
  static constexpr int SC = (NT >= 9) ? 16 : 32;                 // sensors per panel
  static constexpr int QMAX = (NAP - 1 > SPR_MAX_R) ? SPR_MAX_R : NAP - 1;
  static constexpr int LDN = QMAX + 1;
  static constexpr int T = NT * (NT + 1) / 2;
  static constexpr int TPW = (T + AS_WAVES - 1) / AS_WAVES;
};

template <int NT>
__device__ inline void as_tri_coords(int idx, int &ti, int &tj) {
  ti = 0;
  while (ti < NT - 1 && idx >= NT - ti) { idx -= NT - ti; ++ti; }
  tj = ti + idx;
  if (tj > NT - 1) tj = NT - 1;
}

// design[p] = [Theta C_p | Theta a0_p]  (s x (q+1) row-major), plain FMA chains over the modes in index order
__global__ __launch_bounds__(AS_THREADS) void assim_design_kernel(const double *__restrict__ Theta, int s, int r, int q,
                                                                  const double *__restrict__ a0_all,
                                                                  const double *__restrict__ C_all, double *__restrict__ D_all) {
  const int p = blockIdx.x;
  const double *C = C_all + (int64_t)p * r * q;
  const double *a0 = a0_all + (int64_t)p * r;
  double *D = D_all + (int64_t)p * s * (q + 1);
  const int64_t total = (int64_t)s * (q + 1);
  for (int64_t e = (int64_t)blockIdx.y * AS_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.y * AS_THREADS) {
    const int k = (int)(e / (q + 1)), c = (int)(e - (int64_t)k * (q + 1));
    const double *th = Theta + (int64_t)k * r;
    double acc = 0.0;
    if (c < q) {
      for (int j = 0; j < r; ++j) acc = fma(th[j], C[(int64_t)j * q + c], acc);
    } else {
      for (int j = 0; j < r; ++j) acc = fma(th[j], a0[j], acc);
    }
    D[e] = acc;
  }
}

// design: s x ldd row-major at design + p * dstride.  sigma != NULL (diagonal prior): design = Theta (ldd = r = q, dstride 0),
// column c is scaled by sigma[p][c] and Theta a0 is formed here.  sigma == NULL (factor prior): design = the workspace of
// assim_design_kernel (ldd = q + 1), column q holds Theta a0; Cf = the factors (n_p x r x q).
template <int NT>
__global__ __launch_bounds__(AS_THREADS) void assimilate_kernel(
    const double *__restrict__ design, int64_t dstride, int ldd, int s, int r, int q, const double *__restrict__ cnt,
    const double *__restrict__ scale, int n_features, const double *__restrict__ y_all, const double *__restrict__ a0_all,
    const double *__restrict__ sigma_all, const double *__restrict__ Cf_all, double *__restrict__ Ar, double *__restrict__ Ar_std,
    double *__restrict__ F_all, double *__restrict__ z_all, double *__restrict__ info) {
  using C = AssimCfg<NT>;
  constexpr int CP = C::CP, SC = C::SC, LDN = C::LDN, T = C::T, TPW = C::TPW, NAP = C::NAP, QMAX = C::QMAX;
  __shared__ double panel[SC * CP];
  __shared__ double N[QMAX * LDN];      // lower triangle + diagonal: H' then L'; strict upper triangle: X^T, X = L'^-1
  __shared__ double rhs[QMAX];          // B^T W res, then z
  __shared__ double sol[QMAX];          // u = L'^-1 B^T W res
  __shared__ double a0s[QMAX], sgs[QMAX], dinv[QMAX];
  __shared__ double sw[SC], sv[SC], sm[SC], slog[SC];
  __shared__ double wr2[1];
  __shared__ int flags[2];  // [0] Cholesky breakdown, [1] a sensor uncertainty that is zero or not finite

  const int p = blockIdx.x;
  const double *y = y_all + (int64_t)p * s * 3;
  const double *D = design + (int64_t)p * dstride;
  const double *a0 = a0_all + (int64_t)p * r;
  const bool diag = sigma_all != nullptr;     // kernel argument: the same for every thread
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  if (tid < 2) flags[tid] = 0;
  if (tid == 0) wr2[0] = 0.0;
  if (tid < SC) slog[tid] = 0.0;
  for (int c = tid; c < QMAX; c += AS_THREADS) {
    a0s[c] = (diag && c < q) ? a0[c] : 0.0;
    sgs[c] = (diag && c < q) ? sigma_all[(int64_t)p * r + c] : 1.0;
  }

  int offA[TPW], offB[TPW];
  int nt = T - wave * TPW;
  if (nt > TPW) nt = TPW;
  if (nt < 0) nt = 0;
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    int ti, tj;
    as_tri_coords<NT>(wave * TPW + u, ti, tj);
    offA[u] = ti * 16;
    offB[u] = tj * 16;
  }
  f64x4 acc[TPW];
#pragma unroll
  for (int u = 0; u < TPW; ++u) acc[u] = (f64x4){0.0, 0.0, 0.0, 0.0};

  const int frag = (lane >> 4) * CP + (lane & 15);
  for (int c0 = 0; c0 < s; c0 += SC) {
    __syncthreads();  // previous panel fully consumed (first pass: the prologue's LDS writes are visible)
    if (tid < SC) {
      const int k = c0 + tid;
      double w = 0.0, v0 = 0.0;
      if (k < s) {
        int f = (int)y[3 * k + 2];
        if (f < 0) f = 0;
        if (f > n_features - 1) f = n_features - 1;
        const double scl = scale[f];
        v0 = (y[3 * k] - cnt[k]) / scl;
        const double s0 = y[3 * k + 1] / scl;
        w = 1.0 / s0;
        if (!isfinite(w) || !isfinite(s0)) flags[1] = 1;
        slog[tid] += 2.0 * log(fabs(s0));     // this thread's sensors in index order
      }
      sw[tid] = w; sv[tid] = v0;
    }
    // raw design rows (the column scales go on after Theta a0 has been formed from them)
    for (int e = tid; e < SC * NAP; e += AS_THREADS) {
      const int kk = e / NAP, c = e - kk * NAP;
      const int k = c0 + kk;
      panel[kk * CP + c] = (k < s && c < ldd && c <= q) ? D[(int64_t)k * ldd + c] : 0.0;
    }
    __syncthreads();
    // Theta a0 per sensor of the panel: the factor form finds it in column q; the diagonal form sums it here, wave w
    // taking sensors w, w + 4, ... (a0s is zero for the factor form: the sum is computed and not used)
    for (int kk = wave; kk < SC; kk += AS_WAVES) {
      double d0 = 0.0;
      for (int c = lane; c < q; c += 64) d0 += panel[kk * CP + c] * a0s[c];
      d0 = group_sum(d0, 64);
      if (lane == 0) sm[kk] = diag ? d0 : panel[kk * CP + q];
    }
    __syncthreads();
    for (int e = tid; e < SC * NAP; e += AS_THREADS) {
      const int kk = e / NAP, c = e - kk * NAP;
      const int k = c0 + kk;
      if (k < s) {
        if (c < q) panel[kk * CP + c] *= sw[kk] * sgs[c];
        else if (c == q) panel[kk * CP + c] = sw[kk] * (sv[kk] - sm[kk]);
      }
    }
    __syncthreads();
#pragma unroll 1
    for (int k0 = 0; k0 < SC; k0 += 4) {
#pragma unroll
      for (int u = 0; u < TPW; ++u) {
        if (u < nt) {
          const double a = panel[frag + k0 * CP + offA[u]];
          const double b = panel[frag + k0 * CP + offB[u]];
          acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[u], 0, 0, 0);
        }
      }
    }
  }
  __syncthreads();

  // accumulators -> H' - I (both triangles), the right-hand side and |W res|^2
#pragma unroll
  for (int u = 0; u < TPW; ++u) {
    if (u < nt) {
      const double vals[4] = {acc[u].x, acc[u].y, acc[u].z, acc[u].w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int gi = offA[u] + (lane >> 4) + 4 * i, gj = offB[u] + (lane & 15);
        if (gi < q) {
          if (gj < q) { N[gi * LDN + gj] = vals[i]; N[gj * LDN + gi] = vals[i]; }
          else if (gj == q) rhs[gi] = vals[i];
        } else if (gi == q && gj == q) {
          wr2[0] = vals[i];
        }
      }
    }
  }
  __syncthreads();
  for (int j = tid; j < q; j += AS_THREADS) N[j * LDN + j] += 1.0;
  __syncthreads();

  // Cholesky H' = L' L'^T (lower, in place)
  for (int j = 0; j < q; ++j) {
    if (tid == 0) {
      double d = N[j * LDN + j];
      if (!(d > 0.0) || !isfinite(d)) { flags[0] = 1; d = 1e-300; }
      N[j * LDN + j] = sqrt(d);
    }
    __syncthreads();
    const double djj = N[j * LDN + j];
    for (int i = j + 1 + tid; i < q; i += AS_THREADS) N[i * LDN + j] /= djj;
    __syncthreads();
    const int cntj = q - j - 1;
    for (int e = tid; e < cntj * cntj; e += AS_THREADS) {
      const int a = e / cntj, b = e - a * cntj;
      if (b <= a) {
        const int i = j + 1 + a, k = j + 1 + b;
        N[i * LDN + k] -= N[i * LDN + j] * N[k * LDN + j];
      }
    }
    __syncthreads();
  }
  // L' u = B^T W res (u stays in sol), then L'^T z = u (z ends up in rhs)
  for (int j = 0; j < q; ++j) {
    if (tid == 0) sol[j] = rhs[j] / N[j * LDN + j];
    __syncthreads();
    for (int i = j + 1 + tid; i < q; i += AS_THREADS) rhs[i] -= N[i * LDN + j] * sol[j];
    __syncthreads();
  }
  for (int j = tid; j < q; j += AS_THREADS) rhs[j] = sol[j];
  __syncthreads();
  for (int j = q - 1; j >= 0; --j) {
    if (tid == 0) rhs[j] = rhs[j] / N[j * LDN + j];
    __syncthreads();
    for (int i = tid; i < j; i += AS_THREADS) rhs[i] -= N[j * LDN + i] * rhs[j];
    __syncthreads();
  }
  // X = L'^-1, column j by one thread: X_jj = 1 / L_jj, X_ij = -(sum_{k=j}^{i-1} L_ik X_kj) / L_ii.  X_ij (i > j) is kept
  // at N[j][i]: each thread writes its own row of the strict upper triangle and reads the lower triangle, which stays.
  for (int j = tid; j < q; j += AS_THREADS) dinv[j] = 1.0 / N[j * LDN + j];
  __syncthreads();
  for (int j = tid; j < q; j += AS_THREADS) {
    for (int i = j + 1; i < q; ++i) {
      double a = N[i * LDN + j] * dinv[j];
      for (int k = j + 1; k < i; ++k) a = fma(N[i * LDN + k], N[j * LDN + k], a);
      N[j * LDN + i] = -a / N[i * LDN + i];
    }
  }
  __syncthreads();

  // F = C X^T: F[i][j] = sum_{k <= j} C[i][k] X[j][k]
  double *F = F_all + (int64_t)p * r * q;
  if (diag) {
    for (int e = tid; e < r * q; e += AS_THREADS) {
      const int i = e / q, j = e - i * q;
      const double x = (j > i) ? N[i * LDN + j] : (j == i ? dinv[i] : 0.0);
      F[e] = (j >= i) ? sgs[i] * x : 0.0;
    }
  } else {
    const double *Cf = Cf_all + (int64_t)p * r * q;
    for (int e = tid; e < r * q; e += AS_THREADS) {
      const int i = e / q, j = e - i * q;
      double a = 0.0;
      for (int k = 0; k < j; ++k) a = fma(Cf[(int64_t)i * q + k], N[k * LDN + j], a);
      F[e] = fma(Cf[(int64_t)i * q + j], dinv[j], a);
    }
  }
  __syncthreads();  // the workgroup's own writes of F are visible to it
  for (int i = tid; i < r; i += AS_THREADS) {
    double v = 0.0, m = 0.0;
    for (int j = 0; j < q; ++j) { const double f = F[(int64_t)i * q + j]; v = fma(f, f, v); }
    if (diag) {
      m = sgs[i] * rhs[i];
    } else {
      const double *Cf = Cf_all + (int64_t)p * r * q;
      for (int k = 0; k < q; ++k) m = fma(Cf[(int64_t)i * q + k], rhs[k], m);
    }
    Ar[(int64_t)p * r + i] = (m == 0.0) ? a0[i] : a0[i] + m;     // a coefficient the prior pins keeps its bits
    Ar_std[(int64_t)p * r + i] = sqrt(v);
  }
  if (z_all)
    for (int j = tid; j < q; j += AS_THREADS) z_all[(int64_t)p * q + j] = rhs[j];
  if (tid == 0) {
    double dmax = 0.0, dmin = 1e300, uu = 0.0, ld = 0.0, ls = 0.0;
    for (int j = 0; j < q; ++j) {
      const double d = N[j * LDN + j];
      if (d > dmax) dmax = d;
      if (d < dmin) dmin = d;
      uu = fma(sol[j], sol[j], uu);
      ld += log(d);
    }
    for (int k = 0; k < SC; ++k) ls += slog[k];
    info[4 * p] = flags[1] ? 2.0 : (double)flags[0];   // 2: a sensor uncertainty that is zero or not finite, 1: breakdown
    info[4 * p + 1] = (dmax / dmin) * (dmax / dmin);
    info[4 * p + 2] = wr2[0] - uu;
    info[4 * p + 3] = ls + 2.0 * ld;
  }
}

inline size_t assim_workspace(int32_t s, int32_t q, int32_t n_p) {
  return sizeof(double) * (size_t)n_p * (size_t)s * ((size_t)q + 1);
}

}  // namespace

// bytes of workspace the factor form needs (the diagonal form needs none); 0 for shapes the entry point refuses
extern "C" size_t spr_assimilate_workspace(int32_t s, int32_t r, int32_t q, int32_t n_p) {
  if (s <= 0 || r <= 0 || r > SPR_MAX_R || q <= 0 || q > r || n_p <= 0) return 0;
  return assim_workspace(s, q, n_p);
}

extern "C" int spr_assimilate_f64(const double *d_Theta, int32_t s, int32_t r, const double *d_cnt, const double *d_scale,
                                  int32_t n_features, const double *d_y, int32_t n_p, const double *d_a0,
                                  const double *d_sigma, const double *d_factor, int32_t q, double *d_Ar, double *d_Ar_std,
                                  double *d_F, double *d_z, double *d_info, void *d_workspace, size_t workspace_bytes,
                                  void *stream) {
  SPR_REQUIRE(d_Theta && d_cnt && d_scale && d_y && d_a0 && d_Ar && d_Ar_std && d_F && d_info, SPR_E_INVALID,
              "spr_assimilate_f64: NULL pointer");
  SPR_REQUIRE((d_sigma != nullptr) != (d_factor != nullptr), SPR_E_INVALID,
              "spr_assimilate_f64: exactly one of d_sigma and d_factor");
  SPR_REQUIRE(s > 0 && r > 0 && n_p > 0 && n_features > 0 && q > 0 && q <= r && (d_factor || q == r), SPR_E_INVALID,
              "spr_assimilate_f64: bad shape");
  SPR_REQUIRE(r <= SPR_MAX_R, SPR_E_UNSUPPORTED, "spr_assimilate_f64: r=%d > %d not built", r, SPR_MAX_R);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double *design = d_Theta;
  int64_t dstride = 0;
  int ldd = r;
  if (d_factor) {
    SPR_REQUIRE(d_workspace != nullptr, SPR_E_INVALID, "spr_assimilate_f64: NULL pointer (the factor form needs a workspace)");
    SPR_REQUIRE(workspace_bytes >= assim_workspace(s, q, n_p), SPR_E_WORKSPACE,
                "spr_assimilate_f64: workspace too small (%zu bytes, %zu needed)", workspace_bytes, assim_workspace(s, q, n_p));
    SPR_REQUIRE((reinterpret_cast<uintptr_t>(d_workspace) & 7) == 0, SPR_E_INVALID,
                "spr_assimilate_f64: workspace must be 8-byte aligned");
    double *ws = static_cast<double *>(d_workspace);
    const int64_t per = (int64_t)s * (q + 1);
    int gy = (int)((per + AS_THREADS - 1) / AS_THREADS);
    if (gy > 1024) gy = 1024;
    hipLaunchKernelGGL(assim_design_kernel, dim3(n_p, gy), dim3(AS_THREADS), 0, st, d_Theta, (int)s, (int)r, (int)q, d_a0,
                       d_factor, ws);
    SPR_LAUNCH_CHECK();
    design = ws;
    dstride = per;
    ldd = q + 1;
  }
  SPR_DISPATCH_NT(spr_round_nt(q + 1), "spr_assimilate_f64", r,
                  hipLaunchKernelGGL(assimilate_kernel<RUNG>, dim3(n_p), dim3(AS_THREADS), 0, st, design, dstride, ldd, (int)s,
                                     (int)r, (int)q, d_cnt, d_scale, (int)n_features, d_y, d_a0, d_sigma, d_factor, d_Ar,
                                     d_Ar_std, d_F, d_z, d_info));
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}
