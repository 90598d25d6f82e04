// Gappy POD on the device: the normal equations of ROM.gappy_transform for snapshots with a row mask.
//
// With a 0/1 mask M over the rows the least-squares coefficients of a snapshot in the basis are
//   a = (Ur^T M Ur)^+ Ur^T M x0,   x0[i] = (x[i] - X_cnt[i]) / X_scl[f(i)].
// One streaming pass over the basis block and X forms, over the block's rows,
//   H[c][d] = sum_i m_i Ur[i][c] Ur[i][d]   (r x r),   B[j][c] = sum_i m_i x0[i][j] Ur[i][c]   (k x r),   nobs = sum_i m_i;
// the r x r solve is the caller's.  This is the encode pass of validate.hip with a row mask and a second, symmetric
// product: 64-row panels staged by the rowtile.hpp loader, the ROWS of a panel are the contraction index of
// v_mfma_f64_16x16x4_f64, workgroups dealt to feature segments (common.hpp) so the divisor is a workgroup constant, one
// LDS image per matrix with the next panel waiting in registers, per-workgroup slots and a second kernel that adds them
// in increasing order (no atomics: two runs agree bit for bit).
//  * The basis panel is staged ONCE with the masked rows written as zeros and is both operands of H (M^2 = M) and the B
//    operand of the cross product.  A masked-out element is selected away on its way to LDS, never multiplied by zero:
//    NaN or garbage in an unobserved row of X (or of the basis) reaches nothing.
//  * H is accumulated as its upper 16 x 16 tiles (diagonal included), 9 per wave at r > 64; the reduce kernel
//    forms the sum of element (min(c, d), max(c, d)) for both (c, d) and (d, c), so H comes out exactly symmetric.
//  * Panel skipping: every wave reads the 64 mask bytes of a candidate panel (one byte per lane, a ballot makes them a
//    wave-uniform 64-bit word) BEFORE anything else of the panel is requested; a panel without an observed row is passed
//    over.  GP_SCAN candidates are tested per round so a long run of empty panels costs one memory latency per GP_SCAN
//    panels, and the search for the panel after next runs behind the MFMAs of the current one.  Inside a panel that is
//    not fully observed a group of four rows without an observed one skips its MFMA step (a wave-uniform test of the word).
//  * k is cut into slices of 64 columns; H and nobs are formed in the first slice only.
#include <stdlib.h>

#include "rowtile.hpp"
#include "launch.hpp"

namespace {

constexpr int GP_THREADS = 256;
constexpr int GP_R = 64;         // panel rows = 16 MFMA steps
constexpr int GP_SLICE = 64;     // columns of X per read of the basis block (as encode)
constexpr int GP_SCAN = 8;       // candidate panels whose mask bytes are in flight together
constexpr int GP_SCAN_WIDE = 2;  // ... at r > 64 with H: the accumulators leave no registers for more (LAB_NOTEBOOK)
constexpr int GP_TAIL = 8;       // doubles behind a slot's H block (nobs + padding)

// LDS image whose ROWS are the contraction index: the bank layout of validate.hip (rows start 32 banks apart)
constexpr int gp_mp(int mt) { return 16 * mt + ((mt % 2 == 0) ? 16 : 0); }
constexpr int gp_wj(int mtr, int jt) { return jt >= 4 ? (mtr >= 4 ? 2 : 4) : jt; }     // waves along the X tiles
constexpr size_t gp_lds_bytes(int mtr, int jt) { return (size_t)GP_R * (gp_mp(mtr) + gp_mp(jt)) * sizeof(double); }
inline int gp_per_cu(int mtr, int jt) {
  const int fit = (int)((160 * 1024) / gp_lds_bytes(mtr, jt));
  return fit < 1 ? 1 : (fit > 4 ? 4 : fit);
}
inline int gp_round_mtr(int r) { return r <= 16 ? 1 : r <= 32 ? 2 : r <= 64 ? 4 : 8; }
inline int gp_round_jt(int k) { return k <= 16 ? 1 : k <= 32 ? 2 : 4; }
inline size_t gp_slot_doubles(int mtr, int jt, bool with_h) {
  return (size_t)(16 * jt) * (16 * mtr) + (with_h ? (size_t)(16 * mtr) * (16 * mtr) + GP_TAIL : 0);
}
inline int64_t gp_max_slots(int mtr, int jt, int32_t n_features) {
  return (int64_t)gp_per_cu(mtr, jt) * spr_cus_or_default() + n_features;
}

// The mask bytes of GP_SCAN candidate panels c0, c0 + wpf, ...: issue() requests them (one byte per lane and panel, clamped
// addresses, no branch), first() turns them into wave-uniform words and names the first panel with an observed row.
template <int SCAN>
struct MaskScan {
  uint8_t b[SCAN];
  __device__ inline void issue(const uint8_t *__restrict__ mask, int64_t ldm, int64_t lo, int64_t hi, int64_t c0, int wpf,
                               int64_t npanels, int lane) {
#pragma unroll
    for (int u = 0; u < SCAN; ++u) {
      const int64_t cand = c0 + (int64_t)u * wpf;
      const int64_t row = lo + cand * GP_R + lane;
      const bool ok = cand < npanels && row < hi;
      const uint8_t v = mask[(ok ? row : lo) * ldm];
      b[u] = ok ? v : (uint8_t)0;
    }
  }
  __device__ inline bool first(int64_t c0, int wpf, int64_t &c, uint64_t &bits) const {
    bool found = false;
#pragma unroll
    for (int u = 0; u < SCAN; ++u) {
      const uint64_t w = __ballot(b[u] != 0);
      if (!found && w != 0) {
        found = true;
        c = c0 + (int64_t)u * wpf;
        bits = w;
      }
    }
    return found;
  }
};

// first panel c0, c0 + wpf, ... with an observed row (npanels, bits 0: none).  Every wave reads the same bytes, so the
// answer is the same in all four.
template <int SCAN>
__device__ inline void gp_find(const uint8_t *__restrict__ mask, int64_t ldm, int64_t lo, int64_t hi, int64_t c0, int wpf,
                               int64_t npanels, int lane, int64_t &c, uint64_t &bits) {
  MaskScan<SCAN> s;
  while (c0 < npanels) {
    s.issue(mask, ldm, lo, hi, c0, wpf, npanels, lane);
    if (s.first(c0, wpf, c, bits)) return;
    c0 += (int64_t)SCAN * wpf;
  }
  c = npanels;
  bits = 0;
}

// registers -> LDS of one staged panel: rows whose bit is clear (unobserved, or past the segment) and padded columns are
// written as zeros by selection.  SCALED: (x - cnt) / scl per element as encode forms it.
template <bool SCALED, typename RT, int MP>
__device__ inline void masked_store(const RT &t, double *__restrict__ lds, int m, double sc, uint64_t bits, int wave,
                                    int lane) {
  const int grp = lane / RT::LPR, lig = lane % RT::LPR;
#pragma unroll
  for (int it = 0; it < RT::IT; ++it) {
    const int rloc = it * RT::ROWS_PER_IT + wave * RT::RPW + grp;
    const bool rv = (bits >> rloc) & 1;
    const double mean = SCALED ? t.pmean[it] : 0.0;
#pragma unroll
    for (int v = 0; v < RT::VPL; ++v) {
      const int col = 2 * (lig + v * RT::LPR);
      const f64x2 w = widen(t.pre[it][v]);
      f64x2 c;
      if (SCALED) {
        c.x = (rv && col < m) ? (w.x - mean) / sc : 0.0;
        c.y = (rv && col + 1 < m) ? (w.y - mean) / sc : 0.0;
      } else {
        c.x = (rv && col < m) ? w.x : 0.0;
        c.y = (rv && col + 1 < m) ? w.y : 0.0;
      }
      *reinterpret_cast<f64x2 *>(lds + rloc * MP + col) = c;
    }
  }
}

// slot[blockIdx] = [ B: 16 JT x 16 MTR | H: 16 MTR x 16 MTR, upper tiles only | nobs ]  (the last two with WITH_H)
template <int MTR, int JT, int VEC, bool WITH_H, typename TU, typename TX>
__global__ __launch_bounds__(GP_THREADS) void gappy_kernel(const TU *__restrict__ Ur, int r, int64_t ldu,
                                                           const TX *__restrict__ X, int kx, int64_t ldx, SegPlan plan,
                                                           const double *__restrict__ rowmean,
                                                           const double *__restrict__ scale,
                                                           const uint8_t *__restrict__ mask, int64_t ldm,
                                                           double *__restrict__ part, int64_t slot) {
  constexpr int NW = GP_THREADS / 64, R = GP_R;
  constexpr int MPU = gp_mp(MTR), MPX = gp_mp(JT);
  constexpr int WJ = gp_wj(MTR, JT), WC = NW / WJ;
  constexpr int NA = JT / WJ, NB = (MTR + WC - 1) / WC;
  // H as the unordered pairs {i, (i + d) mod MTR} of 16-column blocks, d = 0 .. MTR / 2: wave w takes i = w (and w + 4 at
  // MTR = 8), so its operand addresses are one register plus constants (no wrap for i = w at MTR = 8; three more registers
  // for i = w + 4) -- a table of offsets per tile does not fit beside 17 accumulator tiles
  constexpr int HD = MTR / 2 + 1;
  constexpr int NH = WITH_H ? (MTR == 8 ? 2 * HD - 1 : HD) : 0;   // tiles per wave
  constexpr int SCAN = (MTR == 8 && WITH_H) ? GP_SCAN_WIDE : GP_SCAN;
  static_assert(JT % WJ == 0 && NW % WJ == 0, "the waves must tile the X tiles");
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
  f64x4 hacc[NH > 0 ? NH : 1];
  int hia[NH > 0 ? NH : 1], hib[NH > 0 ? NH : 1];   // wave-uniform 16-column blocks of the A and the B operand
  int hoa[NH > 0 ? NH : 1], hob[NH > 0 ? NH : 1];   // LDS offsets of the two operands
  bool hok[NH > 0 ? NH : 1];                        // the pair exists and is this wave's (else: computed, never stored)
  const int hl = (lane >> 4) * MPU + (lane & 15);
  const int hw = hl + 16 * (wave < MTR ? wave : 0);
#pragma unroll
  for (int q = 0; q < NH; ++q) {
    hacc[q] = (f64x4){0.0, 0.0, 0.0, 0.0};
    const int ii = q / HD, d = q - ii * HD;
    if (MTR == 8) {
      hia[q] = wave + 4 * ii;
      hib[q] = ii == 0 ? wave + d : ((wave + 4 + d) & 7);
      hoa[q] = hw + 64 * ii;
      hob[q] = ii == 0 ? hw + 16 * d : hl + 16 * hib[q];
      hok[q] = true;                                  // i = w: d = 0 .. 4;  i = w + 4: d = 0 .. 3
    } else {
      hia[q] = wave < MTR ? wave : 0;
      hib[q] = (hia[q] + d) % MTR;
      hoa[q] = hw;
      hob[q] = hl + 16 * hib[q];
      hok[q] = wave < MTR && (d == 0 || 2 * d < MTR || (2 * d == MTR && wave < MTR / 2));
    }
  }

  RU tu;
  RX tx;
  const int64_t npanels = (hi - lo + R - 1) / R;
  int64_t c, cn;                                      // the panel in registers / the one after it, both with observed rows
  uint64_t bc, bn;                                    // their mask words: bit i = row i observed (0 past the segment)
  long long nobs = 0;
  gp_find<SCAN>(mask, ldm, lo, hi, wl, wpf, npanels, lane, c, bc);   // wl < wpf <= npanels (seg_wgs)
  cn = npanels; bn = 0;
  if (c < npanels) {
    tu.template load<VEC>(Ur, ldu, r, lo + c * R, hi, wave, lane);
    tx.template load<VEC>(X, ldx, kx, lo + c * R, hi, wave, lane, rowmean);
    gp_find<SCAN>(mask, ldm, lo, hi, c + wpf, wpf, npanels, lane, cn, bn);
  }
  while (c < npanels) {
    const int64_t nrow0 = (cn < npanels) ? lo + cn * R : hi;   // no panel left: a harmless re-read of the last row
    MaskScan<SCAN> scan;
    __syncthreads();             // every wave is done with the previous panel's images
    masked_store<false, RU, MPU>(tu, us, r, 1.0, bc, wave, lane);
    masked_store<true, RX, MPX>(tx, xs, kx, sc, bc, wave, lane);
    scan.issue(mask, ldm, lo, hi, cn + wpf, wpf, npanels, lane);   // the mask bytes first: the panel after next
    tu.template load<VEC>(Ur, ldu, r, nrow0, hi, wave, lane);
    tx.template load<VEC>(X, ldx, kx, nrow0, hi, wave, lane, rowmean);
    __syncthreads();
#define GP_STEP(ks)                                                                                                           \
  {                                                                                                                           \
    double av[NA], bv[NB];                                                                                                    \
    _Pragma("unroll") for (int a = 0; a < NA; ++a) av[a] = xs[4 * (ks) * MPX + xoff[a]];                                       \
    _Pragma("unroll") for (int b = 0; b < NB; ++b) bv[b] = us[4 * (ks) * MPU + uoff[b]];                                       \
    _Pragma("unroll") for (int a = 0; a < NA; ++a)                                                                             \
      _Pragma("unroll") for (int b = 0; b < NB; ++b)                                                                           \
        acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);                                    \
    _Pragma("unroll") for (int q = 0; q < NH; ++q) {                                                                           \
      const double ha = us[4 * (ks) * MPU + hoa[q]];                                                                            \
      const double hb = us[4 * (ks) * MPU + hob[q]];                                                                            \
      hacc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ha, hb, hacc[q], 0, 0, 0);                                                \
    }                                                                                                                         \
  }
    if (bc == ~0ull) {           // fully observed panel: one straight run of MFMA steps
#pragma unroll
      for (int ks = 0; ks < R / 4; ++ks) GP_STEP(ks)
    } else {                     // four rows without an observed one contribute zeros: skip their step
#pragma unroll
      for (int ks = 0; ks < R / 4; ++ks)
        if ((bc >> (4 * ks)) & 0xFull) GP_STEP(ks)
    }
#undef GP_STEP
    nobs += __popcll(bc);
    int64_t c2;
    uint64_t b2;
    if (!scan.first(cn + wpf, wpf, c2, b2))
      gp_find<SCAN>(mask, ldm, lo, hi, cn + (int64_t)(1 + SCAN) * wpf, wpf, npanels, lane, c2, b2);
    c = cn; bc = bn;
    cn = c2; bn = b2;
  }
  // D[i = (lane >> 4) + 4 q][j = lane & 15]: B: i = column of the X slice, j = column of the basis; H: i, j = columns of the basis
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
  if (WITH_H) {
    double *ph = pb + (16 * JT) * (16 * MTR);
#pragma unroll
    for (int q = 0; q < NH; ++q) {
      if (hok[q]) {                                   // a pair with i > j is the transpose of the upper tile (j, i)
        const bool up = hia[q] <= hib[q];
        const int row = 16 * hia[q] + (lane >> 4), col = 16 * hib[q] + (lane & 15);
        double *o = ph + (up ? row * (16 * MTR) + col : col * (16 * MTR) + row);
        const int st = up ? 16 * MTR : 1;
        o[0] = hacc[q].x;
        o[4 * st] = hacc[q].y;
        o[8 * st] = hacc[q].z;
        o[12 * st] = hacc[q].w;
      }
    }
    if (threadIdx.x == 0) ph[(16 * MTR) * (16 * MTR)] = (double)nobs;
  }
}

// sums over the slots, in increasing order: B[j0 + j][c] (ksl x r), and with WITH_H  H[c][d] = H[d][c] = the sum of the
// upper element (min, max)  and  nobs
template <bool WITH_H>
__global__ __launch_bounds__(256) void gappy_reduce_kernel(const double *__restrict__ part, int nslots, int64_t slot, int pj,
                                                           int pc, int ksl, int r, double *__restrict__ B, int j0,
                                                           double *__restrict__ H, double *__restrict__ nobs) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int nb = ksl * r, nh = WITH_H ? r * r : 0;
  if (idx >= nb + nh + (WITH_H ? 1 : 0)) return;
  const double *p;
  double *out;
  if (idx < nb) {
    const int j = idx / r, c = idx - j * r;
    p = part + (int64_t)j * pc + c;
    out = B + (int64_t)(j0 + j) * r + c;
  } else if (idx < nb + nh) {
    const int e = idx - nb, c = e / r, d = e - c * r;
    const int a = c < d ? c : d, b = c < d ? d : c;
    p = part + (int64_t)pj * pc + (int64_t)a * pc + b;
    out = H + e;
  } else {
    p = part + (int64_t)pj * pc + (int64_t)pc * pc;
    out = nobs;
  }
  double s = 0.0;
#pragma unroll 8
  for (int b = 0; b < nslots; ++b) s += p[b * slot];
  *out = s;
}

template <int MTR, int JT, bool WITH_H, typename TU, typename TX>
int launch_gappy(const TU *Ur, int32_t r, int64_t ldu, const TX *X, int32_t ksl, int64_t ldx, SegPlan plan,
                 const double *rowmean, const double *scale, const uint8_t *mask, int64_t ldm, double *part,
                 size_t workspace_bytes, double *H, double *B, double *nobs, int j0, hipStream_t st) {
  const int grid = spr_plan_grid(plan, gp_per_cu(MTR, JT), GP_R);
  const int64_t slot = (int64_t)gp_slot_doubles(MTR, JT, WITH_H);
  // also bounded by the bytes the caller passed: not SPR_REQUIRE_GRID
  SPR_REQUIRE(grid > 0 && grid <= gp_max_slots(MTR, JT, plan.n_features) &&
                  (size_t)grid * (size_t)slot * sizeof(double) <= workspace_bytes,
              SPR_E_INVALID, "spr_gappy_normal: grid of %d exceeds the workspace", grid);
  const bool uvec = spr_pair_aligned(Ur, r, ldu);
  const bool xvec = spr_pair_aligned(X, ksl, ldx);
#define GP(V) hipLaunchKernelGGL((gappy_kernel<MTR, JT, V, WITH_H, TU, TX>), dim3(grid), dim3(GP_THREADS), 0, st, Ur, (int)r, ldu, X, (int)ksl, ldx, plan, rowmean, scale, mask, ldm, part, slot)
  if (uvec && xvec) GP(1);
  else GP(0);
#undef GP
  SPR_LAUNCH_CHECK();
  const int total = ksl * r + (WITH_H ? r * r + 1 : 0);
  hipLaunchKernelGGL((gappy_reduce_kernel<WITH_H>), dim3((total + 255) / 256), dim3(256), 0, st, part, grid, slot, 16 * JT,
                     16 * MTR, (int)ksl, (int)r, B, j0, H, nobs);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

template <int MTR, bool WITH_H, typename TU, typename TX>
int launch_gappy_jt(int jt, const TU *Ur, int32_t r, int64_t ldu, const TX *X, int32_t ksl, int64_t ldx, SegPlan plan,
                    const double *rowmean, const double *scale, const uint8_t *mask, int64_t ldm, double *part,
                    size_t workspace_bytes, double *H, double *B, double *nobs, int j0, hipStream_t st) {
  switch (jt) {
    case 1: return launch_gappy<MTR, 1, WITH_H, TU, TX>(Ur, r, ldu, X, ksl, ldx, plan, rowmean, scale, mask, ldm, part, workspace_bytes, H, B, nobs, j0, st);
    case 2: return launch_gappy<MTR, 2, WITH_H, TU, TX>(Ur, r, ldu, X, ksl, ldx, plan, rowmean, scale, mask, ldm, part, workspace_bytes, H, B, nobs, j0, st);
    default: return launch_gappy<MTR, 4, WITH_H, TU, TX>(Ur, r, ldu, X, ksl, ldx, plan, rowmean, scale, mask, ldm, part, workspace_bytes, H, B, nobs, j0, st);
  }
}

// the largest (slots x doubles per slot) of the launches a call makes: the first slice with H, the later ones without
size_t gappy_workspace(int32_t r, int32_t k, int32_t n_features) {
  if (r <= 0 || r > SPR_MAX_R || k <= 0 || n_features <= 0) return 0;
  const int mtr = gp_round_mtr(r);
  const int k0 = k < GP_SLICE ? k : GP_SLICE;
  size_t need = (size_t)gp_max_slots(mtr, gp_round_jt(k0), n_features) * gp_slot_doubles(mtr, gp_round_jt(k0), true);
  for (int j0 = GP_SLICE; j0 < k; j0 += GP_SLICE) {
    const int jt = gp_round_jt(k - j0 < GP_SLICE ? k - j0 : GP_SLICE);
    const size_t n2 = (size_t)gp_max_slots(mtr, jt, n_features) * gp_slot_doubles(mtr, jt, false);
    need = n2 > need ? n2 : need;
  }
  return need * sizeof(double);
}

template <typename TU, typename TX>
int gappy_normal(const char *name, const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const TX *d_X, int32_t k,
                 int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                 const double *d_scale, const uint8_t *d_mask, int64_t ldm, double *d_H, double *d_B, double *d_nobs,
                 void *d_workspace, size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_Ur && d_X && d_rowmean && d_scale && d_mask && d_H && d_B && d_nobs && d_workspace, SPR_E_INVALID,
              "%s: NULL pointer", name);
  SPR_REQUIRE(n_rows > 0 && r > 0 && ldu >= r && k > 0 && ldx >= k && ldm > 0, SPR_E_INVALID,
              "%s: bad shape n_rows=%lld r=%d ldu=%lld k=%d ldx=%lld ldm=%lld", name, (long long)n_rows, r, (long long)ldu, k,
              (long long)ldx, (long long)ldm);
  SPR_REQUIRE_LAYOUT(name, row0, n_rows, n_points, n_features);
  SPR_REQUIRE(r <= SPR_MAX_R, SPR_E_INVALID, "%s: r = %d exceeds the %d modes the masked Gram matrix is built for", name, r,
              SPR_MAX_R);
  SPR_REQUIRE(workspace_bytes >= gappy_workspace(r, k, n_features), SPR_E_INVALID, "%s: workspace of %zu bytes, %zu needed",
              name, workspace_bytes, gappy_workspace(r, k, n_features));
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *part = static_cast<double *>(d_workspace);
  SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, GP_R);
  for (int j0 = 0; j0 < k; j0 += GP_SLICE) {
    const int ksl = (k - j0 < GP_SLICE) ? k - j0 : GP_SLICE;
    const int jt = gp_round_jt(ksl);
    int rc = SPR_OK;
    SPR_DISPATCH_POW2(gp_round_mtr(r), name, r,
                      rc = j0 == 0 ? launch_gappy_jt<RUNG, true, TU, TX>(jt, d_Ur, r, ldu, d_X + j0, ksl, ldx, plan, d_rowmean,
                                                                         d_scale, d_mask, ldm, part, workspace_bytes, d_H, d_B,
                                                                         d_nobs, j0, st)
                                   : launch_gappy_jt<RUNG, false, TU, TX>(jt, d_Ur, r, ldu, d_X + j0, ksl, ldx, plan, d_rowmean,
                                                                          d_scale, d_mask, ldm, part, workspace_bytes, d_H, d_B,
                                                                          d_nobs, j0, st))
    if (rc != SPR_OK) return rc;
  }
  return SPR_OK;
}

}  // namespace

extern "C" size_t spr_gappy_normal_workspace(int32_t r, int32_t k, int32_t n_features) {
  return gappy_workspace(r, k, n_features);
}

#define SPR_GAPPY_ENTRY(NAME, TU, TX)                                                                                         \
  extern "C" int NAME(const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const TX *d_X, int32_t k, int64_t ldx,          \
                      int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale,     \
                      const uint8_t *d_mask, int64_t ldm, double *d_H, double *d_B, double *d_nobs, void *d_workspace,        \
                      size_t workspace_bytes, void *stream) {                                                                 \
    return gappy_normal<TU, TX>(#NAME, d_Ur, n_rows, r, ldu, d_X, k, ldx, row0, n_points, n_features, d_rowmean, d_scale,     \
                                d_mask, ldm, d_H, d_B, d_nobs, d_workspace, workspace_bytes, stream);                         \
  }
SPR_GAPPY_ENTRY(spr_gappy_normal_f64, double, double)
SPR_GAPPY_ENTRY(spr_gappy_normal_x32, double, float)          // X stored as f32
SPR_GAPPY_ENTRY(spr_gappy_normal_u32, float, double)          // basis stored as f32
SPR_GAPPY_ENTRY(spr_gappy_normal_x32_u32, float, float)
#undef SPR_GAPPY_ENTRY
