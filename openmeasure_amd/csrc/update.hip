// Incremental POD on the device: the two streaming passes of ROM.partial_fit (openmeasure_amd/_update.py) that the
// library did not have.  With the basis U (n x r, orthonormal), a batch X_b (n x k, k <= 64) and
//   X0_b[i][j] = (X_b[i][j] - X_cnt[i]) / X_scl[f(i)]
// formed on the way to LDS (never stored), and C = X0_b^T U from spr_encode_*:
//
//  * residual pass (spr_subspace_residual_*): E = X0_b - U C^T is formed per 64-row panel ON CHIP and
//      H = E^T E (k x k),   C2 = E^T U (k x r),   ss = sum X0_b^2
//    come back; E never reaches HBM.  This is gappy_kernel (gappy.hip) without the mask and with one front stage: after
//    the panels of U and X0_b are staged, every wave forms 16 rows of E on the f64 MFMA, contracting over r (A operand:
//    the staged U panel read across its rows; B operand: C, at most 64 KB and the same for every panel -- staged once per
//    workgroup in LDS where it fits beside the two images, read from L2 where it does not), and puts them where X0_b was.  The two products then run as in gappy with the rows of the panel as the contraction index.
//    H is formed from E, not as X0^T X0 - C C^T, which cancels when the batch lies in the span of U.  H is accumulated as
//    its upper 16 x 16 tiles and the reduce kernel writes element (min, max) to both places: symmetric bit for bit.
//    Per-workgroup slots and a second kernel that adds them in increasing order: no atomics, two runs agree bit for bit.
//  * basis update (spr_basis_update_*): U_new = U A + X0_b B (n x r2), a tall-skinny product with the two row panels side
//    by side in ONE LDS image as an (r + k)-wide operand against the stacked [A; B] (staged once per workgroup in LDS where
//    it fits, read from L2 where it does not).  Here the ROWS of the
//    panel are the M index of v_mfma_f64_16x16x4_f64 and the columns the contraction index, so the image is read across
//    its rows; its row stride is 2 (mod 32) doubles, which spreads the 16 rows x 2 columns of a half-wave's ds_read_b64
//    over the 32 eight-byte banks.  The next panel waits in registers (as loaded: the centring happens on the way to LDS)
//    while the current one is multiplied.  One pass: 8 r + 8 k + 8 bytes read and 8 r2 written per row, 2 (r + k) r2 flops
//    -- at r = k = r2 = 64 the f64 MFMA time and the HBM time are about equal.
#include <stdlib.h>

#include "rowtile.hpp"
#include "launch.hpp"

namespace {

constexpr int UP_THREADS = 256;
constexpr int UP_R = 64;         // panel rows
constexpr int UP_MAX_K = 64;     // columns of a batch: one slice of encode / gappy
constexpr int UP_TAIL = 8;       // doubles behind a slot's H block (ss + padding)

// ---- residual pass -------------------------------------------------------------------------------------------------------
// LDS images whose ROWS are the contraction index of the two products: the bank layout of gappy.hip / validate.hip
constexpr int up_mp(int mt) { return 16 * mt + ((mt % 2 == 0) ? 16 : 0); }
constexpr int up_wj(int mtr, int jt) { return jt >= 4 ? (mtr >= 4 ? 2 : 4) : jt; }     // waves along the X tiles
constexpr size_t up_lds_bytes(int mtr, int jt) { return (size_t)UP_R * (up_mp(mtr) + up_mp(jt)) * sizeof(double); }
// C as the B operand of the E stage, [c][j] with the row stride of the X image: staged once per workgroup where it fits beside
// the two panel images (every shape but r > 64 with k > 32, which reads it from L2)
constexpr bool up_c_lds(int mtr, int jt) {
  return up_lds_bytes(mtr, jt) + (size_t)16 * mtr * up_mp(jt) * sizeof(double) <= 160 * 1024;
}
constexpr size_t up_lds_total(int mtr, int jt) {
  return up_lds_bytes(mtr, jt) + (up_c_lds(mtr, jt) ? (size_t)16 * mtr * up_mp(jt) * sizeof(double) : 0);
}
inline int up_per_cu(int mtr, int jt) {
  const int fit = (int)((160 * 1024) / up_lds_total(mtr, jt));
  return fit < 1 ? 1 : (fit > 4 ? 4 : fit);
}
inline int up_round_mtr(int r) { return r <= 16 ? 1 : r <= 32 ? 2 : r <= 64 ? 4 : 8; }
inline int up_round_jt(int k) { return k <= 16 ? 1 : k <= 32 ? 2 : 4; }
inline size_t up_slot_doubles(int mtr, int jt) {
  return (size_t)(16 * jt) * (16 * mtr) + (size_t)(16 * jt) * (16 * jt) + UP_TAIL;
}
inline int64_t up_max_slots(int mtr, int jt, int32_t n_features) {
  return (int64_t)up_per_cu(mtr, jt) * spr_cus_or_default() + n_features;
}

// registers -> LDS of one staged panel: rows past the segment and padded columns are written as zeros by selection.
// SCALED: (x - cnt) / scl per element as encode forms it; returns this thread's sum of squares of what it stored.
template <bool SCALED, typename RT, int MP>
__device__ inline double up_store(const RT &t, double *__restrict__ lds, int m, double sc, int64_t crow0, int64_t hi,
                                  int wave, int lane) {
  const int grp = lane / RT::LPR, lig = lane % RT::LPR;
  double ssq = 0.0;
#pragma unroll
  for (int it = 0; it < RT::IT; ++it) {
    const int rloc = it * RT::ROWS_PER_IT + wave * RT::RPW + grp;
    const bool rv = crow0 + rloc < hi;
    const double mean = SCALED ? t.pmean[it] : 0.0;
#pragma unroll
    for (int v = 0; v < RT::VPL; ++v) {
      const int col = 2 * (lig + v * RT::LPR);
      const f64x2 w = widen(t.pre[it][v]);
      f64x2 c;
      if (SCALED) {
        c.x = (rv && col < m) ? (w.x - mean) / sc : 0.0;
        c.y = (rv && col + 1 < m) ? (w.y - mean) / sc : 0.0;
        ssq += c.x * c.x;
        ssq += c.y * c.y;
      } else {
        c.x = (rv && col < m) ? w.x : 0.0;
        c.y = (rv && col + 1 < m) ? w.y : 0.0;
      }
      *reinterpret_cast<f64x2 *>(lds + rloc * MP + col) = c;
    }
  }
  return ssq;
}

// slot[blockIdx] = [ C2: 16 JT x 16 MTR | H: 16 JT x 16 JT, upper tiles only | ss ]
template <int MTR, int JT, int VEC, typename TX>
__global__ __launch_bounds__(UP_THREADS) void residual_kernel(const double *__restrict__ Ur, int r, int64_t ldu,
                                                              const TX *__restrict__ X, int kx, int64_t ldx, SegPlan plan,
                                                              const double *__restrict__ rowmean,
                                                              const double *__restrict__ scale,
                                                              const double *__restrict__ C, double *__restrict__ part,
                                                              int64_t slot) {
  constexpr int NW = UP_THREADS / 64, R = UP_R;
  constexpr int MPU = up_mp(MTR), MPX = up_mp(JT);
  constexpr int WJ = up_wj(MTR, JT), WC = NW / WJ;
  constexpr int NA = JT / WJ, NB = (MTR + WC - 1) / WC;
  constexpr int NTH = JT * (JT + 1) / 2;            // upper tiles of H, dealt round-robin to the waves
  constexpr int NH = (NTH + NW - 1) / NW;
  static_assert(JT % WJ == 0 && NW % WJ == 0, "the waves must tile the X tiles");
  static_assert(R == 16 * NW, "a wave forms 16 rows of E");
  using RU = RowTile<MTR, R, MPU, NW, 16, double>;
  using RX = RowTile<JT, R, MPX, NW, 16, TX>;
  constexpr bool CLDS = up_c_lds(MTR, JT);
  __shared__ double us[R * MPU];
  __shared__ double xs[R * MPX];
  __shared__ double cs[CLDS ? 16 * MTR * MPX : 1];
  int f, wl, wpf, base;
  int64_t lo, hi;
  if (!seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wj = wave % WJ, wc = wave / WJ;
  const double sc = scale[f];
  if (CLDS) {                    // cs[c][j] = C[j][c], zeros in the padding (the first panel's barriers order it before its use)
    for (int e = threadIdx.x; e < 16 * MTR * 16 * JT; e += UP_THREADS) {
      const int j = e / (16 * MTR), c = e - j * (16 * MTR);
      const bool ok = j < kx && c < r;
      const double v = C[ok ? j * r + c : 0];
      cs[c * MPX + j] = ok ? v : 0.0;
    }
  }

  f64x4 acc[NA][NB];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
  int xoff[NA], uoff[NB];        // operand element [k = lane >> 4][lane & 15] of the wave's tiles
#pragma unroll
  for (int a = 0; a < NA; ++a) xoff[a] = (lane >> 4) * MPX + (lane & 15) + 16 * (wj + WJ * a);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int ct = wc + WC * b;                       // tiles past the basis (narrow r): a duplicate of tile 0, never stored
    uoff[b] = (lane >> 4) * MPU + (lane & 15) + 16 * (ct < MTR ? ct : 0);
  }
  f64x4 hacc[NH];
  int hia[NH], hib[NH], hoa[NH], hob[NH];             // wave-uniform tile (hia <= hib) and the LDS offsets of its operands
  bool hok[NH];
#pragma unroll
  for (int q = 0; q < NH; ++q) {
    hacc[q] = (f64x4){0.0, 0.0, 0.0, 0.0};
    const int t = wave + NW * q;
    hok[q] = t < NTH;
    int a = 0, rem = hok[q] ? t : 0;
    while (rem >= JT - a) { rem -= JT - a; ++a; }
    hia[q] = a;
    hib[q] = a + rem;
    hoa[q] = (lane >> 4) * MPX + (lane & 15) + 16 * hia[q];
    hob[q] = (lane >> 4) * MPX + (lane & 15) + 16 * hib[q];
  }
  // E stage: the wave's 16 rows of the panel; A operand [i = row][c], B operand [c][j] = C[j][c], D [row = (lane >> 4) + 4 q][j]
  const int ea = (16 * wave + (lane & 15)) * MPU + (lane >> 4);
  const int ed = (16 * wave + (lane >> 4)) * MPX + (lane & 15);
  int coff[JT];                                       // C[j][c0] of the lane, clamped; cok: j is a column of the batch
  bool cok[JT];
#pragma unroll
  for (int jt = 0; jt < JT; ++jt) {
    const int j = 16 * jt + (lane & 15);
    cok[jt] = j < kx;
    coff[jt] = (cok[jt] ? j : 0) * r;
  }

  RU tu;
  RX tx;
  double ssq = 0.0;
  const int64_t npanels = (hi - lo + R - 1) / R;
  int64_t c = wl;                                     // wl < wpf <= npanels (seg_wgs)
  tu.template load<VEC>(Ur, ldu, r, lo + c * R, hi, wave, lane);
  tx.template load<VEC>(X, ldx, kx, lo + c * R, hi, wave, lane, rowmean);
  while (c < npanels) {
    const int64_t cn = c + wpf;
    const int64_t nrow0 = (cn < npanels) ? lo + cn * R : hi;   // no panel left: a harmless re-read of the last row
    __syncthreads();             // every wave is done with the previous panel's images
    up_store<false, RU, MPU>(tu, us, r, 1.0, lo + c * R, hi, wave, lane);
    ssq += up_store<true, RX, MPX>(tx, xs, kx, sc, lo + c * R, hi, wave, lane);
    tu.template load<VEC>(Ur, ldu, r, nrow0, hi, wave, lane);
    tx.template load<VEC>(X, ldx, kx, nrow0, hi, wave, lane, rowmean);
    __syncthreads();
    {                            // E = X0 - U C^T for rows 16 wave .. 16 wave + 15, written over X0 (rows only this wave reads)
      f64x4 e[JT];
#pragma unroll
      for (int jt = 0; jt < JT; ++jt) {
        const double *p = xs + ed + 16 * jt;
        e[jt] = (f64x4){p[0], p[4 * MPX], p[8 * MPX], p[12 * MPX]};
      }
#pragma unroll 4
      for (int ks = 0; ks < 4 * MTR; ++ks) {
        const double av = -us[ea + 4 * ks];
        const int cc = 4 * ks + (lane >> 4);
        const bool cv = cc < r;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
          double bv;
          if (CLDS) {
            bv = cs[cc * MPX + 16 * jt + (lane & 15)];
          } else {
            const double raw = C[coff[jt] + (cv ? cc : 0)];
            bv = (cv && cok[jt]) ? raw : 0.0;
          }
          e[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, e[jt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int jt = 0; jt < JT; ++jt) {
        double *p = xs + ed + 16 * jt;
        p[0] = e[jt].x;
        p[4 * MPX] = e[jt].y;
        p[8 * MPX] = e[jt].z;
        p[12 * MPX] = e[jt].w;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < R / 4; ++ks) {
      double av[NA], bv[NB];
#pragma unroll
      for (int a = 0; a < NA; ++a) av[a] = xs[4 * ks * MPX + xoff[a]];
#pragma unroll
      for (int b = 0; b < NB; ++b) bv[b] = us[4 * ks * MPU + uoff[b]];
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < NH; ++q) {
        const double ha = xs[4 * ks * MPX + hoa[q]];
        const double hb = xs[4 * ks * MPX + hob[q]];
        hacc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ha, hb, hacc[q], 0, 0, 0);
      }
    }
    c = cn;
  }
  // D[i = (lane >> 4) + 4 q][j = lane & 15]: C2: i = column of the batch, j = column of the basis; H: i, j = columns of the batch
  double *pb = part + (int64_t)blockIdx.x * slot;
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int ct = wc + WC * b;
      if (ct < MTR) {
        double *o = pb + (16 * (wj + WJ * a) + (lane >> 4)) * (16 * MTR) + 16 * ct + (lane & 15);
        o[0] = acc[a][b].x;
        o[4 * 16 * MTR] = acc[a][b].y;
        o[8 * 16 * MTR] = acc[a][b].z;
        o[12 * 16 * MTR] = acc[a][b].w;
      }
    }
  double *ph = pb + (16 * JT) * (16 * MTR);
#pragma unroll
  for (int q = 0; q < NH; ++q) {
    if (hok[q]) {
      double *o = ph + (16 * hia[q] + (lane >> 4)) * (16 * JT) + 16 * hib[q] + (lane & 15);
      o[0] = hacc[q].x;
      o[4 * 16 * JT] = hacc[q].y;
      o[8 * 16 * JT] = hacc[q].z;
      o[12 * 16 * JT] = hacc[q].w;
    }
  }
  // ss: the threads' sums added by one thread in thread order (xs holds at least 1024 doubles)
  __syncthreads();
  xs[threadIdx.x] = ssq;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < UP_THREADS; ++i) s += xs[i];
    ph[(16 * JT) * (16 * JT)] = s;
  }
}

// sums over the slots, in increasing order: C2[j][c] (k x r), H[a][b] = H[b][a] = the sum of the upper element (min, max), ss
__global__ __launch_bounds__(256) void residual_reduce_kernel(const double *__restrict__ part, int nslots, int64_t slot, int pj,
                                                              int pc, int k, int r, double *__restrict__ C2,
                                                              double *__restrict__ H, double *__restrict__ ss) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int nb = k * r, nh = k * k;
  if (idx >= nb + nh + 1) return;
  const double *p;
  double *out;
  if (idx < nb) {
    const int j = idx / r, c = idx - j * r;
    p = part + (int64_t)j * pc + c;
    out = C2 + idx;
  } else if (idx < nb + nh) {
    const int e = idx - nb, c = e / k, d = e - c * k;
    const int a = c < d ? c : d, b = c < d ? d : c;
    p = part + (int64_t)pj * pc + (int64_t)a * pj + b;
    out = H + e;
  } else {
    p = part + (int64_t)pj * pc + (int64_t)pj * pj;
    out = ss;
  }
  double s = 0.0;
#pragma unroll 8
  for (int b = 0; b < nslots; ++b) s += p[b * slot];
  *out = s;
}

size_t residual_workspace(int32_t r, int32_t k, int32_t n_features) {
  if (r <= 0 || r > SPR_MAX_R || k <= 0 || k > UP_MAX_K || n_features <= 0) return 0;
  const int mtr = up_round_mtr(r), jt = up_round_jt(k);
  return (size_t)up_max_slots(mtr, jt, n_features) * up_slot_doubles(mtr, jt) * sizeof(double);
}

template <int MTR, int JT, typename TX>
int launch_residual(const char *name, const double *Ur, int32_t r, int64_t ldu, const TX *X, int32_t k, int64_t ldx,
                    SegPlan plan, const double *rowmean, const double *scale, const double *C, double *part,
                    size_t workspace_bytes, double *H, double *C2, double *ss, hipStream_t st) {
  const int grid = spr_plan_grid(plan, up_per_cu(MTR, JT), UP_R);
  const int64_t slot = (int64_t)up_slot_doubles(MTR, JT);
  // also bounded by the bytes the caller passed: not SPR_REQUIRE_GRID
  SPR_REQUIRE(grid > 0 && grid <= up_max_slots(MTR, JT, plan.n_features) &&
                  (size_t)grid * (size_t)slot * sizeof(double) <= workspace_bytes,
              SPR_E_INVALID, "%s: grid of %d exceeds the workspace", name, grid);
  const bool vec = spr_pair_aligned(Ur, r, ldu) && spr_pair_aligned(X, k, ldx);
#define UPK(V) hipLaunchKernelGGL((residual_kernel<MTR, JT, V, TX>), dim3(grid), dim3(UP_THREADS), 0, st, Ur, (int)r, ldu, X, (int)k, ldx, plan, rowmean, scale, C, part, slot)
  if (vec) UPK(1);
  else UPK(0);
#undef UPK
  SPR_LAUNCH_CHECK();
  const int total = k * r + k * k + 1;
  hipLaunchKernelGGL(residual_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, st, part, grid, slot, 16 * JT, 16 * MTR,
                     (int)k, (int)r, C2, H, ss);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

template <int MTR, typename TX>
int launch_residual_jt(const char *name, int jt, const double *Ur, int32_t r, int64_t ldu, const TX *X, int32_t k,
                       int64_t ldx, SegPlan plan, const double *rowmean, const double *scale, const double *C, double *part,
                       size_t workspace_bytes, double *H, double *C2, double *ss, hipStream_t st) {
  switch (jt) {
    case 1: return launch_residual<MTR, 1, TX>(name, Ur, r, ldu, X, k, ldx, plan, rowmean, scale, C, part, workspace_bytes, H, C2, ss, st);
    case 2: return launch_residual<MTR, 2, TX>(name, Ur, r, ldu, X, k, ldx, plan, rowmean, scale, C, part, workspace_bytes, H, C2, ss, st);
    default: return launch_residual<MTR, 4, TX>(name, Ur, r, ldu, X, k, ldx, plan, rowmean, scale, C, part, workspace_bytes, H, C2, ss, st);
  }
}

// the checks every entry of this file shares, in this order: pointers, shape, layout, r, k
#define UP_REQUIRE_COMMON(name)                                                                                             \
  SPR_REQUIRE(n_rows > 0 && r > 0 && ldu >= r && k >= 0 && (k == 0 || ldx >= k), SPR_E_INVALID,                              \
              "%s: bad shape n_rows=%lld r=%d ldu=%lld k=%d ldx=%lld", name, (long long)n_rows, r, (long long)ldu, k,       \
              (long long)ldx);                                                                                              \
  SPR_REQUIRE_LAYOUT(name, row0, n_rows, n_points, n_features);                                                             \
  SPR_REQUIRE(r <= SPR_MAX_R, SPR_E_UNSUPPORTED, "%s: r = %d exceeds the %d modes the update kernels are built for", name,  \
              r, SPR_MAX_R);                                                                                                \
  SPR_REQUIRE(k <= UP_MAX_K, SPR_E_UNSUPPORTED, "%s: k = %d exceeds the %d columns of one batch", name, k, UP_MAX_K)

template <typename TX>
int subspace_residual(const char *name, const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const TX *d_X, int32_t k,
                      int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                      const double *d_scale, const double *d_C, double *d_H, double *d_C2, double *d_ss, void *d_workspace,
                      size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_Ur && d_X && d_rowmean && d_scale && d_C && d_H && d_C2 && d_ss && d_workspace, SPR_E_INVALID,
              "%s: NULL pointer", name);
  UP_REQUIRE_COMMON(name);
  SPR_REQUIRE(k > 0, SPR_E_INVALID, "%s: k = 0: there is no batch", name);
  SPR_REQUIRE(workspace_bytes >= residual_workspace(r, k, n_features), SPR_E_INVALID,
              "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, residual_workspace(r, k, n_features));
  hipStream_t st = static_cast<hipStream_t>(stream);
  SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, UP_R);
  int rc = SPR_OK;
  SPR_DISPATCH_POW2(up_round_mtr(r), name, r,
                    rc = launch_residual_jt<RUNG, TX>(name, up_round_jt(k), d_Ur, r, ldu, d_X, k, ldx, plan, d_rowmean, d_scale,
                                                      d_C, static_cast<double *>(d_workspace), workspace_bytes, d_H, d_C2, d_ss,
                                                      st))
  return rc;
}

// ---- basis update -----------------------------------------------------------------------------------------------------
// one LDS image of the panel, [ U (16 mtr) | X0 (16 jt) ] per row; the row stride is 2 (mod 32) doubles (see the top)
inline int bu_mp(int mtr, int jt) { return 16 * (mtr + jt) + 2; }
inline size_t bu_lds_bytes(int mtr, int jt) { return (size_t)UP_R * bu_mp(mtr, jt) * sizeof(double); }
inline int bu_round_nt(int r2) { return r2 <= 16 ? 1 : r2 <= 32 ? 2 : r2 <= 64 ? 4 : 8; }
// the stacked [A; B] as the B operand, [c][j] with a row stride of 16 (mod 32) doubles: staged once per workgroup where it
// fits beside the panel image (160 KB in all; e.g. r = 128, k = 64 with r2 > 16 does not fit and reads it from L2)
inline int bu_wp(int nt) { return 16 * nt + 16; }
inline size_t bu_w_bytes(int mtr, int jt, int nt) { return (size_t)16 * (mtr + jt) * bu_wp(nt) * sizeof(double); }
inline bool bu_w_lds(int mtr, int jt, int nt) { return bu_lds_bytes(mtr, jt) + bu_w_bytes(mtr, jt, nt) <= 160 * 1024; }
inline size_t bu_lds_total(int mtr, int jt, int nt) {
  return bu_lds_bytes(mtr, jt) + (bu_w_lds(mtr, jt, nt) ? bu_w_bytes(mtr, jt, nt) : 0);
}
inline int bu_per_cu(int mtr, int jt, int nt) {
  const int fit = (int)((160 * 1024) / bu_lds_total(mtr, jt, nt));
  return fit < 1 ? 1 : (fit > 4 ? 4 : fit);
}

// NT: 16-column tiles of the output (padded to a power of two).  Waves: WC along the output tiles, 4 / WC along the
// four 16-row tiles of the panel.  mtr, jt: 16-column tiles of U and of the batch (run time: they only count loop trips).
template <int NT, bool WLDS, typename TX>
__global__ __launch_bounds__(UP_THREADS) void basis_update_kernel(const double *__restrict__ Ur, int r, int64_t ldu,
                                                                  const TX *__restrict__ X, int k, int64_t ldx, SegPlan plan,
                                                                  const double *__restrict__ rowmean,
                                                                  const double *__restrict__ scale,
                                                                  const double *__restrict__ A, const double *__restrict__ B,
                                                                  int r2, double *__restrict__ out, int64_t ldo, int mtr,
                                                                  int jt) {
  constexpr int NW = UP_THREADS / 64, R = UP_R;
  constexpr int WC = NT < NW ? NT : NW, WR = NW / WC;
  constexpr int NR = (R / 16) / WR, NB = NT / WC;     // row tiles and output tiles of a wave
  constexpr int RPW = R / NW;                         // rows a wave stages
  extern __shared__ double img[];
  int f, wl, wpf, base;
  int64_t lo, hi;
  if (!seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wc = wave % WC, wr = wave / WC;
  const double sc = scale[f];
  const int MP = 16 * (mtr + jt) + 2;
  const int wu = 16 * mtr;                            // padded width of the U half
  const bool two = mtr > 4;                           // the U half is wider than one lane per column
  constexpr int WP = 16 * NT + 16;
  double *ws = img + R * MP;                          // (WLDS) ws[c][j] = [A; B][c][j], zeros in the padding
  if (WLDS) {                    // (the first panel's barriers order it before its use)
    for (int e = threadIdx.x; e < 16 * (mtr + jt) * 16 * NT; e += UP_THREADS) {
      const int c = e / (16 * NT), j = e - c * (16 * NT);
      const bool top = c < wu;
      const int cb = c - wu;
      const bool ok = j < r2 && (top ? c < r : cb < k);
      const double *src = top ? A + (int64_t)(ok ? c : 0) * r2 : B + (int64_t)(ok ? cb : 0) * r2;
      const double v = src[ok ? j : 0];
      ws[c * WP + j] = ok ? v : 0.0;
    }
  }

  // staging: a wave takes RPW rows, a lane one column of U (two at r > 64) and one of the batch.  What waits in registers
  // is what was loaded: the centring happens on the way to LDS, so nothing waits for the loads before the MFMAs start
  double pu0[RPW], pu1[RPW], pm[RPW];
  TX px[RPW];
  const int cu0 = lane < r ? lane : 0, cu1 = lane + 64 < r ? lane + 64 : 0, cx = lane < k ? lane : 0;
  auto load = [&](int64_t prow0) {
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
      int64_t g = prow0 + wave * RPW + rr;
      g = g < hi ? g : hi - 1;
      pu0[rr] = Ur[g * ldu + cu0];
      pu1[rr] = two ? Ur[g * ldu + cu1] : 0.0;
      px[rr] = jt > 0 ? X[g * ldx + cx] : (TX)0;
      pm[rr] = jt > 0 ? rowmean[g] : 0.0;
    }
  };
  auto store = [&](int64_t prow0) {
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
      const int rloc = wave * RPW + rr;
      const bool rv = prow0 + rloc < hi;
      double *row = img + rloc * MP;
      if (lane < wu) row[lane] = (rv && lane < r) ? pu0[rr] : 0.0;
      if (two && lane + 64 < wu) row[lane + 64] = (rv && lane + 64 < r) ? pu1[rr] : 0.0;
      if (lane < 16 * jt) row[wu + lane] = (rv && lane < k) ? ((double)px[rr] - pm[rr]) / sc : 0.0;
    }
  };

  int aoff[NR];                                       // A operand [i = row][c = lane >> 4] of the wave's row tiles
#pragma unroll
  for (int a = 0; a < NR; ++a) aoff[a] = (16 * (wr * NR + a) + (lane & 15)) * MP + (lane >> 4);
  int bcol[NB];                                       // B operand [c = lane >> 4][j = lane & 15] of the wave's output tiles
  bool bok[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int j = 16 * (wc + WC * b) + (lane & 15);
    bok[b] = j < r2;
    bcol[b] = bok[b] ? j : 0;
  }

  const int64_t npanels = (hi - lo + R - 1) / R;
  int64_t c = wl;                                     // wl < wpf <= npanels (seg_wgs)
  load(lo + c * R);
  while (c < npanels) {
    const int64_t cn = c + wpf;
    const int64_t prow0 = lo + c * R;
    __syncthreads();             // every wave is done with the previous panel's image
    store(prow0);
    load(cn < npanels ? lo + cn * R : hi);            // no panel left: a harmless re-read of the last row
    __syncthreads();
    f64x4 acc[NR][NB];
#pragma unroll
    for (int a = 0; a < NR; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
    // the stacked contraction index in 16-column tiles (four MFMA steps each), U's tiles first: the operands of tile t + 1
    // are requested before the MFMAs of tile t are issued
    auto ld = [&](int t, double (&av)[4][NR], double (&bv)[4][NB]) {
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const int cc = 16 * t + 4 * s4 + (lane >> 4);
#pragma unroll
        for (int a = 0; a < NR; ++a) av[s4][a] = img[aoff[a] + 16 * t + 4 * s4];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (WLDS) {
            bv[s4][b] = ws[cc * WP + 16 * (wc + WC * b) + (lane & 15)];
          } else {
            const bool top = t < mtr;
            const int ci = top ? cc : cc - wu;
            const bool ok = (top ? ci < r : ci < k) && bok[b];
            const double *src = top ? A : B;
            const double raw = src[(int64_t)(ok ? ci : 0) * r2 + bcol[b]];
            bv[s4][b] = ok ? raw : 0.0;
          }
        }
      }
    };
    auto mm = [&](const double (&av)[4][NR], const double (&bv)[4][NB]) {
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int a = 0; a < NR; ++a)
#pragma unroll
          for (int b = 0; b < NB; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s4][a], bv[s4][b], acc[a][b], 0, 0, 0);
    };
    const int T = mtr + jt;
    double a0[4][NR], b0[4][NB], a1[4][NR], b1[4][NB];
    ld(0, a0, b0);
    int t = 0;
    for (; t + 1 < T; t += 2) {
      ld(t + 1, a1, b1);
      mm(a0, b0);
      ld(t + 2 < T ? t + 2 : T - 1, a0, b0);        // (past the end: a tile that exists, never multiplied)
      mm(a1, b1);
    }
    if (t < T) mm(a0, b0);
    // D[row = (lane >> 4) + 4 q][j = lane & 15]: rows inside the segment and columns < r2 only
#pragma unroll
    for (int a = 0; a < NR; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        if (bok[b]) {
          const double v[4] = {acc[a][b].x, acc[a][b].y, acc[a][b].z, acc[a][b].w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int64_t g = prow0 + 16 * (wr * NR + a) + (lane >> 4) + 4 * q;
            if (g < hi) out[g * ldo + bcol[b]] = v[q];
          }
        }
      }
    c = cn;
  }
}

template <int NT, typename TX>
int launch_basis_update(const double *Ur, int32_t r, int64_t ldu, const TX *X, int32_t k, int64_t ldx, SegPlan plan,
                        const double *rowmean, const double *scale, const double *A, const double *B, int32_t r2, double *out,
                        int64_t ldo, hipStream_t st) {
  const int mtr = (r + 15) / 16, jt = (k + 15) / 16;
  const size_t lds = bu_lds_total(mtr, jt, NT);
  const int grid = spr_plan_grid(plan, bu_per_cu(mtr, jt, NT), UP_R);
#define BUK(W)                                                                                                                \
  {                                                                                                                           \
    SPR_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&basis_update_kernel<NT, W, TX>),                          \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                   \
    hipLaunchKernelGGL((basis_update_kernel<NT, W, TX>), dim3(grid), dim3(UP_THREADS), lds, st, Ur, (int)r, ldu, X, (int)k,   \
                       ldx, plan, rowmean, scale, A, B, (int)r2, out, ldo, mtr, jt);                                          \
  }
  if (bu_w_lds(mtr, jt, NT)) BUK(true)
  else BUK(false)
#undef BUK
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

template <typename TX>
int basis_update(const char *name, const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const TX *d_X, int32_t k,
                 int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                 const double *d_scale, const double *d_A, const double *d_B, int32_t r2, double *d_out, int64_t ldo,
                 void *stream) {
  SPR_REQUIRE(d_Ur && d_rowmean && d_scale && d_A && d_out && (k <= 0 || (d_X && d_B)), SPR_E_INVALID, "%s: NULL pointer",
              name);
  UP_REQUIRE_COMMON(name);
  SPR_REQUIRE(r2 > 0, SPR_E_INVALID, "%s: bad shape r2=%d", name, r2);
  SPR_REQUIRE(r2 <= SPR_MAX_R, SPR_E_UNSUPPORTED, "%s: r2 = %d exceeds the %d modes the update kernels are built for", name,
              r2, SPR_MAX_R);
  SPR_REQUIRE(ldo >= r2, SPR_E_INVALID, "%s: ldo = %lld is less than r2 = %d", name, (long long)ldo, r2);
  SPR_REQUIRE(static_cast<const void *>(d_out) != static_cast<const void *>(d_Ur), SPR_E_INVALID,
              "%s: the new basis cannot be written over the old one", name);
  hipStream_t st = static_cast<hipStream_t>(stream);
  SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, UP_R);
  int rc = SPR_OK;
  SPR_DISPATCH_POW2(bu_round_nt(r2), name, r2,
                    rc = launch_basis_update<RUNG, TX>(d_Ur, r, ldu, d_X, k, ldx, plan, d_rowmean, d_scale, d_A, d_B, r2, d_out,
                                                       ldo, st))
  return rc;
}

}  // namespace

extern "C" size_t spr_subspace_residual_workspace(int32_t r, int32_t k, int32_t n_features) {
  return residual_workspace(r, k, n_features);
}

#define SPR_RESIDUAL_ENTRY(NAME, TX)                                                                                          \
  SPR_ENTRY(NAME,                                                                                                             \
            (const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const TX *d_X, int32_t k, int64_t ldx, int64_t row0,  \
             int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_C,         \
             double *d_H, double *d_C2, double *d_ss, void *d_workspace, size_t workspace_bytes, void *stream),               \
            (subspace_residual<TX>), d_Ur, n_rows, r, ldu, d_X, k, ldx, row0, n_points, n_features, d_rowmean, d_scale, d_C,  \
            d_H, d_C2, d_ss, d_workspace, workspace_bytes, stream)
SPR_RESIDUAL_ENTRY(spr_subspace_residual_f64, double)
SPR_RESIDUAL_ENTRY(spr_subspace_residual_x32, float)          // X stored as f32
#undef SPR_RESIDUAL_ENTRY

#define SPR_BASIS_UPDATE_ENTRY(NAME, TX)                                                                                      \
  SPR_ENTRY(NAME,                                                                                                             \
            (const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const TX *d_X, int32_t k, int64_t ldx, int64_t row0,  \
             int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_A,         \
             const double *d_B, int32_t r2, double *d_out, int64_t ldo, void *stream),                                        \
            (basis_update<TX>), d_Ur, n_rows, r, ldu, d_X, k, ldx, row0, n_points, n_features, d_rowmean, d_scale, d_A, d_B,  \
            r2, d_out, ldo, stream)
SPR_BASIS_UPDATE_ENTRY(spr_basis_update_f64, double)
SPR_BASIS_UPDATE_ENTRY(spr_basis_update_x32, float)           // X stored as f32
#undef SPR_BASIS_UPDATE_ENTRY
