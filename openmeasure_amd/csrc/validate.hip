// Held-out snapshots on the device: ROM.transform (encode) and ROM.reconstruction_error (field error).
//
// Encode:  A = X0_new^T Ur  with  X0_new[i, j] = (X_new[i, j] - X_cnt[i]) / X_scl[f(i)]  -- what users of the reference write
// as  Ur.T @ ((x - X_cnt) / X_scl)  on the host (the A_new its GPR.update(P_new, A_new) expects, gpr.py:603).  A tall-skinny
// cross product of two different matrices: one streaming read of the basis block and of X_new per column slice, nothing
// n-sized is written.  Workgroups are dealt to feature segments (common.hpp), so the divisor is a workgroup constant; the
// centring and the division are applied to each element as the host does, (x - cnt) / scl, while the row goes from the
// prefetch registers to LDS.  64-row panels of both matrices are staged by the rowtile.hpp loader and the ROWS of a panel
// are the contraction index of v_mfma_f64_16x16x4_f64: A operand = the X0 panel (tile row = column of X_new), B operand =
// the basis panel, 16 MFMA steps per panel and tile.  The four waves split the (k-slice x r) tiles between them and keep
// their accumulators for the whole kernel.  One LDS image per matrix (two of each do not fit at r = 128): the next panel
// waits in registers while the current one is multiplied and is stored behind a barrier.
// No atomics: every workgroup writes its tile block to its own slot of the workspace with plain stores and a second small
// kernel adds the slots in increasing order, so two runs on one device agree bit for bit.
// k is cut into column slices of EN_SLICE columns (one read of the basis block per slice); r > SPR_MAX_R runs the same
// kernel per 128-column group of the basis (one more read of X_new per group).
//
// Field error: the reconstruct pass (reconstruct.hip) with a comparison in place of the store.  Per row
// x = X_scl (Ur[i] . a_j) + X_cnt[i] as spr_reconstruct_* forms it, d = x - X_true[i, j]; per (vector, feature) the sums of
// d^2 and X_true^2, max |d| and the lowest global row attaining it.  Structure of bounds.hip: the 16-vectors-per-pass MFMA
// panel form for r <= SPR_MAX_R, a wave per row beyond; per-workgroup slots and a merge kernel (one wave per (vector,
// feature)), no atomics.
#include <math.h>
#include <type_traits>

#include "rowtile.hpp"
#include "worst.hpp"
#include "launch.hpp"

namespace {

// ---------------------------------------------------------------------------------------------------- encode
constexpr int EN_THREADS = 256;
constexpr int EN_R = 64;         // panel rows = 16 MFMA steps
constexpr int EN_SLICE = 64;     // columns of X_new per read of the basis block (LAB_NOTEBOOK: 64 against 32 and 16)

// row stride of an LDS image whose ROWS are the contraction index: the 32 lanes of one ds_read_b64 group read 16
// consecutive doubles of two rows; the rows have to start 32 banks apart (stride = 16 mod 32 doubles)
constexpr int en_mp(int mt) { return 16 * mt + ((mt % 2 == 0) ? 16 : 0); }
// waves along the X_new tiles (the others along the basis tiles)
constexpr int en_wj(int mtr, int jt) { return jt >= 4 ? (mtr >= 4 ? 2 : 4) : jt; }
constexpr size_t en_lds_bytes(int mtr, int jt) { return (size_t)EN_R * (en_mp(mtr) + en_mp(jt)) * sizeof(double); }
inline int en_per_cu(int mtr, int jt) {
  const int fit = (int)((160 * 1024) / en_lds_bytes(mtr, jt));
  return fit < 1 ? 1 : (fit > 4 ? 4 : fit);
}
inline int en_round_mtr(int r) { return r <= 16 ? 1 : r <= 32 ? 2 : r <= 64 ? 4 : 8; }
inline int en_round_jt(int k) { return k <= 16 ? 1 : k <= 32 ? 2 : 4; }

// registers -> LDS of one staged X_new panel: (x - cnt) / scl per element, zeros for rows past the segment and padded columns
template <typename RX, int MP>
__device__ inline void scaled_store(const RX &t, double *__restrict__ lds, int m, double sc, int64_t crow0, int64_t seg_hi,
                                    int wave, int lane) {
  const int grp = lane / RX::LPR, lig = lane % RX::LPR;
#pragma unroll
  for (int it = 0; it < RX::IT; ++it) {
    const int rloc = it * RX::ROWS_PER_IT + wave * RX::RPW + grp;
    const bool rv = crow0 + rloc < seg_hi;
    const double mean = t.pmean[it];
#pragma unroll
    for (int v = 0; v < RX::VPL; ++v) {
      const int col = 2 * (lig + v * RX::LPR);
      const f64x2 w = widen(t.pre[it][v]);
      f64x2 c;
      c.x = (rv && col < m) ? (w.x - mean) / sc : 0.0;
      c.y = (rv && col + 1 < m) ? (w.y - mean) / sc : 0.0;
      *reinterpret_cast<f64x2 *>(lds + rloc * MP + col) = c;
    }
  }
}

// part[blockIdx][16 JT][16 MTR]: the workgroup's partial  X0_slice^T Ur_group  over its rows
template <int MTR, int JT, int VEC, typename TU, typename TX>
__global__ __launch_bounds__(EN_THREADS) void encode_kernel(const TU *__restrict__ Ur, int r, int64_t ldu,
                                                            const TX *__restrict__ X, int kx, int64_t ldx, SegPlan plan,
                                                            const double *__restrict__ rowmean,
                                                            const double *__restrict__ scale, double *__restrict__ part) {
  constexpr int NW = EN_THREADS / 64, R = EN_R;
  constexpr int MPU = en_mp(MTR), MPX = en_mp(JT);
  constexpr int WJ = en_wj(MTR, JT), WC = NW / WJ;
  constexpr int NA = JT / WJ, NB = (MTR + WC - 1) / WC;
  static_assert(JT % WJ == 0 && NW % WJ == 0, "the waves must tile the X_new tiles");
  using RU = RowTile<MTR, R, MPU, NW, 16, TU>;
  using RX = RowTile<JT, R, MPX, NW, 16, TX>;
  __shared__ double us[R * MPU];
  __shared__ double xs[R * MPX];
  int f, wl, wpf, base;
  int64_t lo, hi;
  if (!seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wj = wave % WJ, wc = wave / WJ;
  const double sc = scale[f];

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

  RU tu;
  RX tx;
  const int64_t npanels = (hi - lo + R - 1) / R;
  int64_t c = wl;                                     // wl < wpf <= npanels (seg_wgs)
  tu.template load<VEC>(Ur, ldu, r, lo + c * R, hi, wave, lane);
  tx.template load<VEC>(X, ldx, kx, lo + c * R, hi, wave, lane, rowmean);
  while (c < npanels) {
    const int64_t crow0 = lo + c * R;
    const int64_t cn = c + wpf;
    const int64_t nrow0 = (cn < npanels) ? lo + cn * R : hi;   // past-the-end panel: a harmless re-read of the last row
    __syncthreads();             // every wave is done with the previous panel's images
    tu.raw_store(us, r, crow0, hi, wave, lane);
    scaled_store<RX, MPX>(tx, xs, kx, sc, crow0, hi, wave, lane);
    tu.template load<VEC>(Ur, ldu, r, nrow0, hi, wave, lane);
    tx.template load<VEC>(X, ldx, kx, nrow0, hi, wave, lane, rowmean);
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
    }
    c = cn;
  }
  // D[i = (lane >> 4) + 4 q][j = lane & 15]: i = column of the X_new slice, j = column of the basis group
  double *pb = part + (int64_t)blockIdx.x * (16 * JT) * (16 * MTR);
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
}

// A[j0 + j][g0 + c] = sum over the slots, in increasing order
__global__ __launch_bounds__(256) void encode_reduce_kernel(const double *__restrict__ part, int nslots, int pj, int pc,
                                                            int ksl, int rg, double *__restrict__ A, int64_t lda, int j0,
                                                            int g0) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= ksl * rg) return;
  const int j = idx / rg, c = idx - j * rg;
  const double *p = part + (int64_t)j * pc + c;
  const int64_t step = (int64_t)pj * pc;
  double s = 0.0;
#pragma unroll 8
  for (int b = 0; b < nslots; ++b) s += p[b * step];
  A[(int64_t)(j0 + j) * lda + g0 + c] = s;
}

inline int64_t en_max_slots(int32_t n_features) {
  return 4 * (int64_t)spr_cus_or_default() + n_features;
}

template <int MTR, int JT, typename TU, typename TX>
int launch_encode(const TU *Ur, int32_t rg, int64_t ldu, const TX *X, int32_t ksl, int64_t ldx, SegPlan plan,
                  const double *rowmean, const double *scale, double *part, int64_t max_slots, double *A, int64_t lda,
                  int j0, int g0, hipStream_t st) {
  const int grid = spr_plan_grid(plan, en_per_cu(MTR, JT), EN_R);
  SPR_REQUIRE_GRID("spr_encode", grid, max_slots);
  const bool uvec = spr_pair_aligned(Ur, rg, ldu);
  const bool xvec = spr_pair_aligned(X, ksl, ldx);
#define EN(V) hipLaunchKernelGGL((encode_kernel<MTR, JT, V, TU, TX>), dim3(grid), dim3(EN_THREADS), 0, st, Ur, (int)rg, ldu, X, (int)ksl, ldx, plan, rowmean, scale, part)
  if (uvec && xvec) EN(1);
  else EN(0);
#undef EN
  SPR_LAUNCH_CHECK();
  const int total = ksl * rg;
  hipLaunchKernelGGL(encode_reduce_kernel, dim3((total + 255) / 256), dim3(256), 0, st, part, grid, 16 * JT, 16 * MTR,
                     (int)ksl, (int)rg, A, lda, j0, g0);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

template <int MTR, typename TU, typename TX>
int launch_encode_jt(int jt, const TU *Ur, int32_t rg, int64_t ldu, const TX *X, int32_t ksl, int64_t ldx, SegPlan plan,
                     const double *rowmean, const double *scale, double *part, int64_t max_slots, double *A, int64_t lda,
                     int j0, int g0, hipStream_t st) {
  switch (jt) {
    case 1: return launch_encode<MTR, 1, TU, TX>(Ur, rg, ldu, X, ksl, ldx, plan, rowmean, scale, part, max_slots, A, lda, j0, g0, st);
    case 2: return launch_encode<MTR, 2, TU, TX>(Ur, rg, ldu, X, ksl, ldx, plan, rowmean, scale, part, max_slots, A, lda, j0, g0, st);
    default: return launch_encode<MTR, 4, TU, TX>(Ur, rg, ldu, X, ksl, ldx, plan, rowmean, scale, part, max_slots, A, lda, j0, g0, st);
  }
}

size_t encode_workspace(int32_t r, int32_t k, int32_t n_features) {
  if (r <= 0 || k <= 0 || n_features <= 0) return 0;
  const int pc = 16 * en_round_mtr(r < SPR_MAX_R ? r : SPR_MAX_R), pj = 16 * en_round_jt(k < EN_SLICE ? k : EN_SLICE);
  return (size_t)en_max_slots(n_features) * pc * pj * sizeof(double);
}

template <typename TU, typename TX>
int encode(const char *name, const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const TX *d_X, int32_t k, int64_t ldx,
           int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale, double *d_A,
           void *d_workspace, size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_Ur && d_X && d_rowmean && d_scale && d_A && d_workspace, SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(n_rows > 0 && r > 0 && ldu >= r && k > 0 && ldx >= k, SPR_E_INVALID,
              "%s: bad shape n_rows=%lld r=%d ldu=%lld k=%d ldx=%lld", name, (long long)n_rows, r, (long long)ldu, k,
              (long long)ldx);
  SPR_REQUIRE_LAYOUT(name, row0, n_rows, n_points, n_features);
  SPR_REQUIRE(r <= SPR_MAX_R_WIDE, SPR_E_UNSUPPORTED, "%s: r = %d exceeds %d", name, r, SPR_MAX_R_WIDE);
  SPR_REQUIRE(workspace_bytes >= encode_workspace(r, k, n_features), SPR_E_INVALID, "%s: workspace of %zu bytes, %zu needed",
              name, workspace_bytes, encode_workspace(r, k, n_features));
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *part = static_cast<double *>(d_workspace);
  SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, EN_R);
  const int64_t max_slots = en_max_slots(n_features);
  for (int j0 = 0; j0 < k; j0 += EN_SLICE) {
    const int ksl = (k - j0 < EN_SLICE) ? k - j0 : EN_SLICE;
    const int jt = en_round_jt(ksl);
    for (int g0 = 0; g0 < r; g0 += SPR_MAX_R) {
      const int rg = (r - g0 < SPR_MAX_R) ? r - g0 : SPR_MAX_R;
      int rc = SPR_OK;
      SPR_DISPATCH_POW2(en_round_mtr(rg), name, rg,
                        rc = launch_encode_jt<RUNG, TU, TX>(jt, d_Ur + g0, rg, ldu, d_X + j0, ksl, ldx, plan, d_rowmean, d_scale,
                                                            part, max_slots, d_A, (int64_t)r, j0, g0, st))
      if (rc != SPR_OK) return rc;
    }
  }
  return SPR_OK;
}

// ---------------------------------------------------------------------------------------------------- field error
constexpr int FE_THREADS = 256;
constexpr int FE_PB = 16;        // coefficient vectors per pass of the MFMA form
constexpr int FE_WPB = 4;        // ... of the wide form
constexpr int FE_SLOT = 4;       // doubles per (vector, workgroup) slot: sum d^2, sum X_true^2, max |d|, its global row

template <int MTR, int VEC, typename TU, typename TX>
__global__ __launch_bounds__(FE_THREADS) void field_error_mfma_kernel(
    const TU *__restrict__ Ur, int r, int64_t ldu, SegPlan plan, const double *__restrict__ rowmean,
    const double *__restrict__ scale, const double *__restrict__ A, int k, int np0, int npb, const TX *__restrict__ Xt,
    int64_t ldx, double *__restrict__ slots, int nslots) {
  constexpr int NW = FE_THREADS / 64, R = 64;
  constexpr int MPAD = 16 * MTR, MP = MPAD + 2, KSTEPS = MPAD / 4;
  using RT = RowTile<MTR, R, MP, NW, 16, TU>;
  __shared__ double smem[2 * R * MP];                 // >= 2304 doubles; the end-of-kernel merge needs 256
  double *const lds0 = smem, *const lds1 = smem + R * MP;
  int f, wl, wpf, base;
  int64_t lo, hi;
  if (!seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const double sc = scale[f];

  double vfrag[KSTEPS];          // MFMA A operand: A[i = lane & 15][k = lane >> 4] = vector np0+i, entry 4 ks + k
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) {
    const int kk = 4 * ks + (lane >> 4), j = lane & 15;
    vfrag[ks] = (j < npb && kk < r) ? A[(int64_t)(np0 + j) * r + kk] : 0.0;
  }
  Worst wm[4];                   // vector pv = 4 q + (lane >> 4)
  double sse[4], sst[4];
  int xcol[4];                   // column of X_true the lane compares with (clamped: the value of a padded vector is discarded)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    wm[q].init(); sse[q] = 0.0; sst[q] = 0.0;
    const int pv = np0 + 4 * q + (lane >> 4);
    xcol[q] = pv < k ? pv : k - 1;
  }

  RT tile;
  const int64_t npanels = (hi - lo + R - 1) / R;
  int64_t c = wl;                                     // wl < wpf <= npanels (seg_wgs)
  tile.template load<VEC>(Ur, ldu, r, lo + c * R, hi, wave, lane);
  tile.raw_store(lds0, r, lo + c * R, hi, wave, lane);
  int64_t cn = c + wpf;
  int64_t nrow0 = (cn < npanels) ? lo + cn * R : hi;
  tile.template load<VEC>(Ur, ldu, r, nrow0, hi, wave, lane);
  int buf = 0;
  const int ufrag = (lane & 15) * MP + (lane >> 4);   // B[k = lane >> 4][j = lane & 15] = panel[16 w + j][k0 + k]
  while (c < npanels) {
    const double *cur = buf ? lds1 : lds0;
    double *nxt = buf ? lds0 : lds1;
    const int64_t c2 = cn + wpf;
    const int64_t n2row0 = (c2 < npanels) ? lo + c2 * R : hi;
    __syncthreads();
    const int64_t row = lo + c * R + wave * 16 + (lane & 15);   // the panel row this lane's results belong to
    const int64_t rc = row < hi ? row : hi - 1;
    const double mu = rowmean[rc];                               // requested before the MFMAs
    double xt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) xt[q] = (double)Xt[rc * ldx + xcol[q]];
    const double *p = cur + wave * 16 * MP + ufrag;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vfrag[ks], p[4 * ks], acc, 0, 0, 0);
      if (ks == 0) {
#pragma unroll
        for (int it = 0; it < RT::IT; ++it) {
          tile.raw_store_pass(it, nxt, r, nrow0, hi, wave, lane);
          tile.template load_pass<VEC>(it, Ur, ldu, r, n2row0, hi, wave, lane);
        }
      }
    }
    // D[i = (lane >> 4) + 4 q][j = lane & 15] = a_{np0+i} . u_row
    const double d[4] = {acc.x, acc.y, acc.z, acc.w};
    const int64_t grow = plan.row0 + row;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool ok = (4 * q + (lane >> 4)) < npb && row < hi;
      const double x = sc * d[q] + mu;                 // as reconstruct.hip forms the field value
      const double e = x - xt[q];
      sse[q] += ok ? e * e : 0.0;
      sst[q] += ok ? xt[q] * xt[q] : 0.0;
      wm[q].push(fabs(e), grow, ok);
    }
    buf ^= 1;
    c = cn;
    cn = c2;
    nrow0 = n2row0;
  }
  // the 16 lanes of a group hold 16 rows of the same four vectors; then the four waves through LDS
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    wm[q].merge_lanes(16);
    sse[q] = group_sum_t<16>(sse[q]);
    sst[q] = group_sum_t<16>(sst[q]);
  }
  __syncthreads();               // the panels are done with
  if ((lane & 15) == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double *s = smem + (wave * FE_PB + 4 * q + (lane >> 4)) * FE_SLOT;
      s[0] = sse[q]; s[1] = sst[q]; s[2] = wm[q].v; s[3] = (double)wm[q].row;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < npb) {
    Worst a;
    a.init();
    double e2 = 0.0, t2 = 0.0;
    for (int w = 0; w < NW; ++w) {
      const double *s = smem + (w * FE_PB + threadIdx.x) * FE_SLOT;
      e2 += s[0]; t2 += s[1];
      a.merge(s[2], (int64_t)s[3]);
    }
    double *o = slots + ((int64_t)(np0 + threadIdx.x) * nslots + blockIdx.x) * FE_SLOT;
    o[0] = e2; o[1] = t2; o[2] = a.v; o[3] = (double)a.row;
  }
}

// r > SPR_MAX_R: one wave per row, lanes stride the columns, FE_WPB vectors per pass kept in LDS.  After the butterfly every
// lane holds the same sums, so every lane keeps the same running state.
template <typename TU, typename TX>
__global__ __launch_bounds__(FE_THREADS) void field_error_wide_kernel(
    const TU *__restrict__ Ur, int r, int64_t ldu, SegPlan plan, const double *__restrict__ rowmean,
    const double *__restrict__ scale, const double *__restrict__ A, int k, int np0, int npb, const TX *__restrict__ Xt,
    int64_t ldx, double *__restrict__ slots, int nslots) {
  constexpr int NW = FE_THREADS / 64, R = 64;
  __shared__ double gl[FE_WPB * SPR_MAX_R_WIDE];
  __shared__ double red[NW * FE_WPB * FE_SLOT];
  int f, wl, wpf, base;
  int64_t lo, hi;
  if (!seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double sc = scale[f];
  for (int i = threadIdx.x; i < FE_WPB * r; i += FE_THREADS) {
    const int p = i / r, kk = i - p * r;
    gl[i] = p < npb ? A[(int64_t)(np0 + p) * r + kk] : 0.0;
  }
  __syncthreads();
  Worst wm[FE_WPB];
  double sse[FE_WPB], sst[FE_WPB];
#pragma unroll
  for (int p = 0; p < FE_WPB; ++p) { wm[p].init(); sse[p] = 0.0; sst[p] = 0.0; }
  const int64_t npanels = (hi - lo + R - 1) / R;
  const int64_t c0 = npanels * wl / wpf, c1 = npanels * (wl + 1) / wpf;   // a contiguous run of panels, never empty
  int64_t rend = lo + c1 * R;
  rend = rend < hi ? rend : hi;
  for (int64_t row = lo + c0 * R + wave; row < rend; row += NW) {
    const TU *rp = Ur + row * ldu;
    double s[FE_WPB];
#pragma unroll
    for (int p = 0; p < FE_WPB; ++p) s[p] = 0.0;
    for (int kk = lane; kk < r; kk += 64) {
      const double u = (double)rp[kk];
#pragma unroll
      for (int p = 0; p < FE_WPB; ++p) s[p] += u * gl[p * r + kk];
    }
    const double mu = rowmean[row];
#pragma unroll
    for (int p = 0; p < FE_WPB; ++p) {
      const bool ok = p < npb;
      const double xt = (double)Xt[row * ldx + (ok ? np0 + p : np0)];
      const double x = sc * group_sum_t<64>(s[p]) + mu;
      const double e = x - xt;
      sse[p] += ok ? e * e : 0.0;
      sst[p] += ok ? xt * xt : 0.0;
      wm[p].push(fabs(e), plan.row0 + row, ok);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int p = 0; p < FE_WPB; ++p) {
      double *s = red + (wave * FE_WPB + p) * FE_SLOT;
      s[0] = sse[p]; s[1] = sst[p]; s[2] = wm[p].v; s[3] = (double)wm[p].row;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < npb) {
    Worst a;
    a.init();
    double e2 = 0.0, t2 = 0.0;
    for (int w = 0; w < NW; ++w) {
      const double *s = red + (w * FE_WPB + threadIdx.x) * FE_SLOT;
      e2 += s[0]; t2 += s[1];
      a.merge(s[2], (int64_t)s[3]);
    }
    double *o = slots + ((int64_t)(np0 + threadIdx.x) * nslots + blockIdx.x) * FE_SLOT;
    o[0] = e2; o[1] = t2; o[2] = a.v; o[3] = (double)a.row;
  }
}

// One wave per (vector, feature): the slots of the feature's workgroups (consecutive blocks, common.hpp) are summed lane-
// strided and closed with the butterfly; the maxima are merged with ties to the lower row.
// out[p][f] = { sum d^2, sum X_true^2, max |d|, row }; a feature without rows in the block: (0, 0, 0, -1).
__global__ __launch_bounds__(64) void field_error_merge_kernel(const double *__restrict__ slots, int nslots, SegPlan plan,
                                                               double *__restrict__ out) {
  const int F = plan.n_features;
  const int p = blockIdx.x / F, f = blockIdx.x - p * F;
  const int lane = threadIdx.x;
  int base = 0, w = 0;
  if (f >= seg_first_feature(plan) && f <= seg_last_feature(plan)) {
    for (int ff = seg_first_feature(plan); ff <= f; ++ff) {
      int64_t lo, hi;
      seg_range(plan, ff, lo, hi);
      base += w;
      w = seg_wgs(plan, hi - lo);
    }
  }
  Worst a;
  a.init();
  double e2 = 0.0, t2 = 0.0;
  const double *sl = slots + ((int64_t)p * nslots + base) * FE_SLOT;
  for (int b = lane; b < w; b += 64) {
    const double *s = sl + (int64_t)b * FE_SLOT;
    e2 += s[0]; t2 += s[1];
    a.merge(s[2], (int64_t)s[3]);
  }
  e2 = group_sum_t<64>(e2);
  t2 = group_sum_t<64>(t2);
  a.merge_lanes(64);
  if (lane == 0) {
    double *o = out + ((int64_t)p * F + f) * FE_SLOT;
    o[0] = e2; o[1] = t2; o[2] = a.row >= 0 ? a.v : 0.0; o[3] = (double)a.row;
  }
}

inline int64_t fe_max_slots(int32_t n_features) {
  return 6 * (int64_t)spr_cus_or_default() + n_features;
}

size_t field_error_workspace(int32_t k, int32_t n_features) {
  if (k <= 0 || n_features <= 0) return 0;
  return (size_t)k * (size_t)fe_max_slots(n_features) * FE_SLOT * sizeof(double);
}

template <int MTR, typename TU, typename TX>
int launch_field_mfma(const TU *Ur, int32_t r, int64_t ldu, SegPlan &plan, const double *rowmean, const double *scale,
                      const double *A, int32_t k, const TX *Xt, int64_t ldx, double *slots, int &nslots, int64_t max_slots,
                      hipStream_t st) {
  const int grid = spr_plan_grid(plan, spr_panel_per_cu(MTR), 64);
  SPR_REQUIRE_GRID("spr_field_error", grid, max_slots);
  nslots = grid;
  const bool vec_ok = spr_pair_aligned(Ur, r, ldu);
  for (int p0 = 0; p0 < k; p0 += FE_PB) {
    const int npb = (k - p0 < FE_PB) ? k - p0 : FE_PB;
#define FE(V) hipLaunchKernelGGL((field_error_mfma_kernel<MTR, V, TU, TX>), dim3(grid), dim3(FE_THREADS), 0, st, Ur, (int)r, ldu, plan, rowmean, scale, A, (int)k, p0, npb, Xt, ldx, slots, grid)
    if (vec_ok) FE(1);
    else FE(0);
#undef FE
    SPR_LAUNCH_CHECK();
  }
  return SPR_OK;
}

template <typename TU, typename TX>
int field_error(const char *name, const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_A, int32_t k,
                const TX *d_Xtrue, int64_t ldx, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_Ur && d_rowmean && d_scale && d_A && d_Xtrue && d_out && d_workspace, SPR_E_INVALID, "%s: NULL pointer",
              name);
  SPR_REQUIRE(n_rows > 0 && r > 0 && ldu >= r && k > 0 && ldx >= k, SPR_E_INVALID,
              "%s: bad shape n_rows=%lld r=%d ldu=%lld k=%d ldx=%lld", name, (long long)n_rows, r, (long long)ldu, k,
              (long long)ldx);
  SPR_REQUIRE_LAYOUT(name, row0, n_rows, n_points, n_features);
  SPR_REQUIRE(r <= SPR_MAX_R_WIDE, SPR_E_UNSUPPORTED, "%s: r = %d exceeds %d", name, r, SPR_MAX_R_WIDE);
  SPR_REQUIRE((int64_t)k * n_features <= INT32_MAX, SPR_E_UNSUPPORTED, "%s: k * n_features = %lld exceeds the grid", name,
              (long long)k * n_features);
  SPR_REQUIRE(workspace_bytes >= field_error_workspace(k, n_features), SPR_E_INVALID,
              "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, field_error_workspace(k, n_features));
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *slots = static_cast<double *>(d_workspace);
  SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, 64);
  const int64_t max_slots = fe_max_slots(n_features);
  int nslots = 0, rc = SPR_OK;
  if (r > SPR_MAX_R) {
    const int grid = spr_plan_grid(plan, 4, 64);
    SPR_REQUIRE_GRID(name, grid, max_slots);
    nslots = grid;
    for (int p0 = 0; p0 < k; p0 += FE_WPB) {
      const int npb = (k - p0 < FE_WPB) ? k - p0 : FE_WPB;
      hipLaunchKernelGGL((field_error_wide_kernel<TU, TX>), dim3(grid), dim3(FE_THREADS), 0, st, d_Ur, (int)r, ldu, plan,
                         d_rowmean, d_scale, d_A, (int)k, p0, npb, d_Xtrue, ldx, slots, grid);
      SPR_LAUNCH_CHECK();
    }
  } else {
    // padded width in 16-column tiles; r <= SPR_MAX_R: one of 1, 2, 3, 4, 6, 8
    SPR_DISPATCH_MT(spr_round_mt(r), name, r,
                    rc = launch_field_mfma<RUNG, TU, TX>(d_Ur, r, ldu, plan, d_rowmean, d_scale, d_A, k, d_Xtrue, ldx, slots,
                                                         nslots, max_slots, st))
  }
  if (rc != SPR_OK) return rc;
  hipLaunchKernelGGL(field_error_merge_kernel, dim3(k * n_features), dim3(64), 0, st, slots, nslots, plan, d_out);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

}  // namespace

extern "C" size_t spr_encode_workspace(int32_t r, int32_t k, int32_t n_features) { return encode_workspace(r, k, n_features); }

#define SPR_ENCODE_ENTRY(NAME, TU, TX)                                                                                        \
  extern "C" int NAME(const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const TX *d_X, int32_t k, int64_t ldx,          \
                      int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale,     \
                      double *d_A, void *d_workspace, size_t workspace_bytes, void *stream) {                                 \
    return encode<TU, TX>(#NAME, d_Ur, n_rows, r, ldu, d_X, k, ldx, row0, n_points, n_features, d_rowmean, d_scale, d_A,      \
                          d_workspace, workspace_bytes, stream);                                                              \
  }
SPR_ENCODE_ENTRY(spr_encode_f64, double, double)
SPR_ENCODE_ENTRY(spr_encode_x32, double, float)          // X_new stored as f32
SPR_ENCODE_ENTRY(spr_encode_u32, float, double)          // basis stored as f32
SPR_ENCODE_ENTRY(spr_encode_x32_u32, float, float)
#undef SPR_ENCODE_ENTRY

extern "C" size_t spr_field_error_workspace(int32_t k, int32_t n_features) { return field_error_workspace(k, n_features); }

#define SPR_FIELD_ERROR_ENTRY(NAME, TU, TX)                                                                                   \
  extern "C" int NAME(const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,                 \
                      int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_A, int32_t k,       \
                      const TX *d_Xtrue, int64_t ldx, double *d_out, void *d_workspace, size_t workspace_bytes,               \
                      void *stream) {                                                                                         \
    return field_error<TU, TX>(#NAME, d_Ur, n_rows, r, ldu, row0, n_points, n_features, d_rowmean, d_scale, d_A, k, d_Xtrue,  \
                               ldx, d_out, d_workspace, workspace_bytes, stream);                                             \
  }
SPR_FIELD_ERROR_ENTRY(spr_field_error_f64, double, double)
SPR_FIELD_ERROR_ENTRY(spr_field_error_x32, double, float)   // X_true stored as f32
SPR_FIELD_ERROR_ENTRY(spr_field_error_u32, float, double)   // basis stored as f32
SPR_FIELD_ERROR_ENTRY(spr_field_error_x32_u32, float, float)
#undef SPR_FIELD_ERROR_ENTRY
