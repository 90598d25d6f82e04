// K10 + K11: x = X_scl * (Ur a) + X_cnt  -- one streaming pass over the basis shard.
//
// HBM-bound (2 flops per 8 bytes).  The pass is the skinny product A . Ur^T with up to 16 coefficient vectors at
// once (v_mfma_f64_16x16x4_f64, the vectors as the A operand, in registers for the whole kernel); the un-scaling
// (sparse_sensing.py:235) is applied before the store.  Workgroups are dealt to feature segments (common.hpp) so
// the per-feature scale is a workgroup constant.  The result tile has the vector index down the rows and the
// basis row across the 16 lanes of a group, so each store instruction writes 16 consecutive field values per
// vector and no cross-lane reduction is needed at all.  r/4 MFMAs per 16 rows are far below the HBM time of the rows.
//
// Two forms, which differ in how the rows of Ur reach the B operand.  The LDS-panel form (any r <= 128, any
// alignment): 64-row panels of Ur are staged raw in LDS by the rowtile.hpp loader (double-buffered, the loads of
// the panel after next issued behind the stores) and wave w reads its 16-row block with strided ds_read_b64.  The
// register-direct form (whole 16-column groups, 16-byte aligned rows): HBM -> registers in the MFMA layout, no
// LDS and no barrier; reconstruct_groups says which shapes take it.
#include <type_traits>

#include "rowtile.hpp"
#include "launch.hpp"
#include "field_dot.hpp"

namespace {

constexpr int RM_THREADS = 256;
constexpr int RM_PB = 16;   // coefficient vectors per pass (one MFMA tile of rows)

template <int MTR, int VEC, typename TU>
__global__ __launch_bounds__(RM_THREADS) void reconstruct_mfma_kernel(
    const TU *__restrict__ Ur, int r, int64_t ldu, SegPlan plan, const double *__restrict__ rowmean,
    const double *__restrict__ scale, const double *__restrict__ rowscale, const double *__restrict__ A, int64_t lda,
    int np0, int npb, double *__restrict__ out, int64_t ldo, int accumulate) {
  constexpr int NW = RM_THREADS / 64, R = 64;
  constexpr int MPAD = 16 * MTR, MP = MPAD + 2, KSTEPS = MPAD / 4;
  using RT = RowTile<MTR, R, MP, NW, 16, TU>;
  __shared__ double smem[2 * R * MP];
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
    const int k = 4 * ks + (lane >> 4), j = lane & 15;
    vfrag[ks] = (j < npb && k < r) ? A[(int64_t)(np0 + j) * lda + k] : 0.0;
  }
  RT tile;
  const int64_t npanels = (hi - lo + R - 1) / R;
  int64_t c = wl;
  if (c >= npanels) return;                       // workgroup-uniform
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
    const double rs = rowscale ? rowscale[rc] : sc;              // sampled rows carry their own scale
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
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int pv = 4 * q + (lane >> 4);
      if (pv < npb && row < hi) {
        // accumulate: a further column group of a basis wider than one launch handles -- the centre is already in
        double *o = out + (int64_t)(np0 + pv) * ldo + row;
        *o = rs * d[q] + (accumulate ? *o : mu);
      }
    }
    buf ^= 1;
    c = cn;
    cn = c2;
    nrow0 = n2row0;
  }
}

template <int MTR, typename TU>
int launch_mfma(const TU *Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                int32_t n_features, const double *rowmean, const double *scale, const double *rowscale,
                const double *A, int64_t lda, int32_t n_p, double *out, int64_t ldo, int accumulate, hipStream_t st) {
  SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, 64);
  const int grid = spr_plan_grid(plan, spr_panel_per_cu(MTR));
  const int lm = spr_load_mode(spr_pair_aligned(Ur, r, ldu), r, MTR);
  for (int p0 = 0; p0 < n_p; p0 += RM_PB) {
    const int npb = (n_p - p0 < RM_PB) ? n_p - p0 : RM_PB;
#define RM(LM) hipLaunchKernelGGL((reconstruct_mfma_kernel<MTR, LM, TU>), dim3(grid), dim3(RM_THREADS), 0, st, Ur, (int)r, ldu, plan, rowmean, scale, rowscale, A, lda, p0, npb, out, ldo, accumulate)
    if (lm == 2) RM(2);
    else if (lm == 1) RM(1);
    else RM(0);
#undef RM
    SPR_LAUNCH_CHECK();
  }
  return SPR_OK;
}

// Register-direct form for an f32-stored basis (BASELINE config 5): its rows carry half the bytes for the same MFMAs and the
// same fixed cost per LDS panel, which held the panel form at 3.1 TB/s (133 KB of LDS per workgroup at r = 128: one
// workgroup, four waves, per CU).  Here -- as in qr_refresh_direct_kernel -- lane (j = l & 15, kk = l >> 4) of a wave owns row
// j of the wave's 16-row block and loads the 16-byte pieces [16 g + 4 kk, +4) of it straight into the MFMA B operand
// (contraction index permuted accordingly, the coefficient fragments are permuted the same way once per kernel): no LDS,
// no barrier, every wave independent, the next block requested before this one is multiplied.
template <int NG, typename TU>
__global__ __launch_bounds__(RM_THREADS) void reconstruct_direct_kernel(
    const TU *__restrict__ Ur, int r, int64_t ldu, SegPlan plan, const double *__restrict__ rowmean,
    const double *__restrict__ scale, const double *__restrict__ rowscale, const double *__restrict__ A, int64_t lda,
    int np0, int npb, double *__restrict__ out, int64_t ldo, int accumulate) {
  constexpr int R = 64;
  using P4 = typename std::conditional<std::is_same<TU, float>::value, float4, double4>::type;
  int f, wl, wpf, base;
  int64_t lo, hi;
  if (!seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, kk = lane >> 4;
  const double sc = scale[f];
  double vfrag[4 * NG];          // A[i = li][k]: vector np0 + li, entry 16 g + 4 kk + t at MFMA step 4 g + t
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int t = 0; t < 4; ++t) vfrag[4 * g + t] = (li < npb) ? A[(int64_t)(np0 + li) * lda + 16 * g + 4 * kk + t] : 0.0;
  const int64_t npanels = (hi - lo + R - 1) / R;
  auto load_block = [&](int64_t c, P4 (&dst)[NG]) {
    int64_t row = lo + c * R + wave * 16 + li;
    row = row < hi ? row : hi - 1;                             // past the segment: a harmless re-read, never stored
    const TU *rp = Ur + row * ldu + 4 * kk;
#pragma unroll
    for (int g = 0; g < NG; ++g) dst[g] = *reinterpret_cast<const P4 *>(rp + 16 * g);
  };
  int64_t c = wl;
  if (c >= npanels) return;
  P4 cur[NG], nxt[NG];
  load_block(c, cur);
  while (c < npanels) {
    const int64_t cn = c + wpf;
    load_block(cn < npanels ? cn : c, nxt);
    const int64_t row = lo + c * R + wave * 16 + li;           // the row this lane's results belong to
    const int64_t rc = row < hi ? row : hi - 1;
    const double mu = rowmean[rc];
    const double rs = rowscale ? rowscale[rc] : sc;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const double b4[4] = {(double)cur[g].x, (double)cur[g].y, (double)cur[g].z, (double)cur[g].w};
#pragma unroll
      for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vfrag[4 * g + t], b4[t], acc, 0, 0, 0);
    }
    const double d[4] = {acc.x, acc.y, acc.z, acc.w};          // D[i = kk + 4 q][j = li] = a_{np0+i} . u_row
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int pv = 4 * q + kk;
      if (pv < npb && row < hi) {
        double *o = out + (int64_t)(np0 + pv) * ldo + row;
        *o = rs * d[q] + (accumulate ? *o : mu);
      }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) cur[g] = nxt[g];
    c = cn;
  }
}

template <int NG, typename TU>
int launch_direct(const TU *Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                  int32_t n_features, const double *rowmean, const double *scale, const double *rowscale,
                  const double *A, int64_t lda, int32_t n_p, double *out, int64_t ldo, int accumulate, hipStream_t st) {
  // an f64 basis comes here with more than 96 columns only (reconstruct_groups): its narrower rungs are not built
  if constexpr (std::is_same<TU, float>::value || NG > 6) {
    SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, 64);
    const int grid = spr_plan_grid(plan, 4);                   // no LDS: registers decide (16 waves per CU)
    for (int p0 = 0; p0 < n_p; p0 += RM_PB) {
      const int npb = (n_p - p0 < RM_PB) ? n_p - p0 : RM_PB;
      hipLaunchKernelGGL((reconstruct_direct_kernel<NG, TU>), dim3(grid), dim3(RM_THREADS), 0, st, Ur, (int)r, ldu, plan,
                         rowmean, scale, rowscale, A, lda, p0, npb, out, ldo, accumulate);
      SPR_LAUNCH_CHECK();
    }
    return SPR_OK;
  }
  return SPR_E_UNSUPPORTED;
}

// Row-dot form for up to SPR_FIELD_NF coefficient vectors (whole 16-column groups, rows that keep the 16-byte alignment of
// their pairs): no MFMA at all.  Lane (li = l & 15, kk = l >> 4) of a wave loads the rows kk + 4 i, i = 0..3, of the wave's
// 16-row block at the columns 16 ct + li -- the accumulator layout in which the W-stationary projection holds the same
// rows -- and calls the very function that projection's field epilogue calls (field_dot.hpp), so a field is the same bit for
// bit whichever kernel wrote it.  16 lanes read 128 consecutive bytes of a row; every wave is independent, the next block
// is requested before this one is reduced.  At BASELINE config 3 (one vector, r = 64): 7.9 ms against 8.3 ms of the MFMA form
// (8.4 ms with 16 waves per CU, plain loads and the four 32-byte stores per block: each of the three gives a part).
template <int NG, typename TU>
__global__ __launch_bounds__(RM_THREADS) void reconstruct_rowdot_kernel(
    const TU *__restrict__ Ur, int r, int64_t ldu, SegPlan plan, const double *__restrict__ rowmean,
    const double *__restrict__ scale, const double *__restrict__ A, int64_t lda, int n_p, double *__restrict__ out,
    int64_t ldo) {
  constexpr int R = 64, NF = SPR_FIELD_NF;
  int f, wl, wpf, base;
  int64_t lo, hi;
  if (!seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, kk = lane >> 4;
  const double sc = scale[f];
  double av[NF][NG];
#pragma unroll
  for (int v = 0; v < NF; ++v)
#pragma unroll
    for (int ct = 0; ct < NG; ++ct) av[v][ct] = (v < n_p) ? A[(int64_t)v * lda + 16 * ct + li] : 0.0;
  const int64_t npanels = (hi - lo + R - 1) / R;
  auto load_block = [&](int64_t c, TU (&dst)[4][NG]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int64_t row = lo + c * R + wave * 16 + kk + 4 * i;
      row = row < hi ? row : hi - 1;                           // past the segment: a harmless re-read, never stored
      const TU *rp = Ur + row * ldu + li;
#pragma unroll
      for (int ct = 0; ct < NG; ++ct) dst[i][ct] = __builtin_nontemporal_load(rp + 16 * ct);   // read once
    }
  };
  int64_t c = wl;
  if (c >= npanels) return;
  TU cur[4][NG], nxt[4][NG];
  load_block(c, cur);
  while (c < npanels) {
    const int64_t cn = c + wpf;
    load_block(cn < npanels ? cn : c, nxt);
    const int64_t row0 = lo + c * R + wave * 16 + kk;          // this lane's rows: row0 + 4 i
    double mu[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) mu[i] = rowmean[row0 + 4 * i < hi ? row0 + 4 * i : hi - 1];
    double xs[NF][4];                                          // row row0 + 4 i, the same bits in all 16 lanes of group kk
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double u[NG];
#pragma unroll
      for (int ct = 0; ct < NG; ++ct) u[ct] = (double)cur[i][ct];
#pragma unroll
      for (int v = 0; v < NF; ++v) xs[v][i] = field_row_value<NG>(u, av[v], sc, mu[i]);
    }
    // lane L < 16 collects row L of the block (held by group L & 3 as its entry L >> 2): one 128-byte store per block and
    // vector instead of four 32-byte ones
    const int64_t rowL = lo + c * R + wave * 16 + lane;
#pragma unroll
    for (int v = 0; v < NF; ++v) {
      double g = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double t = __shfl(xs[v][i], 16 * (lane & 3), 64);
        if ((lane >> 2) == i) g = t;
      }
      if (lane < 16 && v < n_p && rowL < hi) out[(int64_t)v * ldo + rowL] = g;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int ct = 0; ct < NG; ++ct) cur[i][ct] = nxt[i][ct];
    c = cn;
  }
}

template <int NG, typename TU>
int launch_rowdot(const TU *Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points, int32_t n_features,
                  const double *rowmean, const double *scale, const double *A, int64_t lda, int32_t n_p, double *out,
                  int64_t ldo, hipStream_t st) {
  SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, 64);
  const int grid = spr_plan_grid(plan, 8);                     // no LDS: registers decide (50-96: 20-32 waves per CU resident)
  hipLaunchKernelGGL((reconstruct_rowdot_kernel<NG, TU>), dim3(grid), dim3(RM_THREADS), 0, st, Ur, (int)r, ldu, plan, rowmean,
                     scale, A, lda, (int)n_p, out, ldo);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

// r <= 128 per launch; a wider basis (r <= m in the reference, :336) goes in column groups of 128 that accumulate
template <typename TU>
int reconstruct_groups(const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                       int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_rowscale,
                       const double *d_A, int32_t n_p, double *d_Xrec, int64_t ldo, hipStream_t st) {
  // up to SPR_FIELD_NF vectors on a basis the W-stationary projection can have written (16/32/48/64 columns, aligned rows,
  // per-feature scale): the row-dot form, whose field equals the one that projection emits itself (spr_project_field_*)
  if (n_p <= SPR_FIELD_NF && !d_rowscale && r <= 64 && r % 16 == 0 && spr_rows_aligned16(d_Ur, ldu * sizeof(TU))) {
#define RD(NGV) case NGV: return launch_rowdot<NGV, TU>(d_Ur, n_rows, r, ldu, row0, n_points, n_features, d_rowmean, d_scale, d_A, r, n_p, d_Xrec, ldo, st)
    switch (r / 16) { RD(1); RD(2); RD(3); RD(4); }
#undef RD
  }
  for (int g0 = 0; g0 < r; g0 += SPR_MAX_R) {
    const int rg = (r - g0 < SPR_MAX_R) ? r - g0 : SPR_MAX_R;
    int rc = SPR_OK;
    // whole 16-column groups, 16-byte aligned rows: the register-direct form for an f32 basis and for f64 bases wider than
    // 96 columns (whose LDS panels leave room for one workgroup per CU only: 3.5 -> 2.8 ms at the c5s shape)
    if ((std::is_same<TU, float>::value || rg > 96) && rg % 16 == 0 && spr_rows_aligned16(d_Ur + g0, ldu * sizeof(TU))) {
      SPR_DISPATCH_1TO8(rg / 16, "spr_reconstruct", rg,
                        rc = launch_direct<RUNG, TU>(d_Ur + g0, n_rows, rg, ldu, row0, n_points, n_features, d_rowmean, d_scale,
                                                     d_rowscale, d_A + g0, r, n_p, d_Xrec, ldo, g0 > 0, st))
      if (rc != SPR_OK) return rc;
      continue;
    }
    SPR_DISPATCH_MT(spr_round_mt(rg), "spr_reconstruct", rg,      // padded width of the group in 16-column tiles
                    rc = launch_mfma<RUNG, TU>(d_Ur + g0, n_rows, rg, ldu, row0, n_points, n_features, d_rowmean, d_scale,
                                               d_rowscale, d_A + g0, r, n_p, d_Xrec, ldo, g0 > 0, st))
    if (rc != SPR_OK) return rc;
  }
  return SPR_OK;
}

}  // namespace

namespace {
template <typename TU>
int reconstruct(const char *name, const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_rowscale,
                const double *d_A, int32_t n_p, double *d_Xrec, int64_t ldo, void *stream) {
  SPR_REQUIRE(d_Ur && d_rowmean && d_scale && d_A && d_Xrec, SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(n_rows > 0 && r > 0 && ldu >= r && n_p > 0 && ldo >= n_rows, SPR_E_INVALID,
              "%s: bad shape n_rows=%lld r=%d ldu=%lld n_p=%d ldo=%lld", name, (long long)n_rows, r, (long long)ldu, n_p,
              (long long)ldo);
  SPR_REQUIRE_LAYOUT(name, row0, n_rows, n_points, n_features);
  return reconstruct_groups<TU>(d_Ur, n_rows, r, ldu, row0, n_points, n_features, d_rowmean, d_scale, d_rowscale, d_A, n_p,
                                d_Xrec, ldo, static_cast<hipStream_t>(stream));
}
}  // namespace

// TU = float: basis stored as f32 (the dtype of an f32 snapshot shard's U), arithmetic and output f64
#define SPR_RECONSTRUCT_ENTRY(NAME, TU)                                                                                       \
  SPR_ENTRY(NAME,                                                                                                             \
            (const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points, int32_t n_features,      \
             const double *d_rowmean, const double *d_scale, const double *d_rowscale, const double *d_A, int32_t n_p,        \
             double *d_Xrec, int64_t ldo, void *stream),                                                                      \
            (reconstruct<TU>), d_Ur, n_rows, r, ldu, row0, n_points, n_features, d_rowmean, d_scale, d_rowscale, d_A, n_p,    \
            d_Xrec, ldo, stream)
SPR_RECONSTRUCT_ENTRY(spr_reconstruct_f64, double)
SPR_RECONSTRUCT_ENTRY(spr_reconstruct_u32, float)
#undef SPR_RECONSTRUCT_ENTRY

// Sharded reconstruct() with several coefficient vectors: the ONE all-gather of the ranks' (n_p, n_loc) blocks leaves
// stage[q][v][i]; the reference's result has the vectors as columns of the whole field (:371-375), i.e. out[v][q n_loc + i].
namespace {
__global__ __launch_bounds__(256) void field_unstage_kernel(const double *__restrict__ stage, int world, int n_p,
                                                            int64_t n_loc, double *__restrict__ out, int64_t ldo) {
  // one (q, v) block per blockIdx.y; 16-byte pieces where both sides are aligned, scalar tail otherwise
  const int q = blockIdx.y / n_p, v = blockIdx.y - q * n_p;
  const double *src = stage + ((int64_t)q * n_p + v) * n_loc;
  double *dst = out + (int64_t)v * ldo + (int64_t)q * n_loc;
  const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  if (vec) {
    const int64_t n2 = n_loc / 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += stride)
      reinterpret_cast<f64x2 *>(dst)[i] = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(src) + i);
    if ((n_loc & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[n_loc - 1] = src[n_loc - 1];
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_loc; i += stride) dst[i] = src[i];
  }
}
}  // namespace

extern "C" int spr_field_unstage_f64(const double *d_stage, int32_t world, int32_t n_p, int64_t n_loc, double *d_out,
                                     int64_t ldo, void *stream) {
  SPR_REQUIRE(d_stage && d_out, SPR_E_INVALID, "spr_field_unstage_f64: NULL pointer");
  SPR_REQUIRE(world > 0 && n_p > 0 && n_loc > 0 && ldo >= (int64_t)world * n_loc && (int64_t)world * n_p <= 65535,
              SPR_E_INVALID, "spr_field_unstage_f64: bad shape world=%d n_p=%d n_loc=%lld ldo=%lld", world, n_p,
              (long long)n_loc, (long long)ldo);
  int64_t bx = (n_loc / 2 + 255) / 256;
  if (bx > 1024) bx = 1024;
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(field_unstage_kernel, dim3((unsigned)bx, (unsigned)(world * n_p)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), d_stage, (int)world, (int)n_p, n_loc, d_out, ldo);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

namespace {
__global__ __launch_bounds__(256) void field_unstage_blocks_kernel(const double *__restrict__ stage, int n_p, int64_t n_max,
                                                                   const int64_t *__restrict__ layout,
                                                                   double *__restrict__ out, int64_t ldo) {
  // one (q, v) block per blockIdx.y, rows_q of its n_max padded entries; same copy loop as field_unstage_kernel
  const int q = blockIdx.y / n_p, v = blockIdx.y - q * n_p;
  const int64_t off = layout[2 * q], rows = layout[2 * q + 1];
  const double *src = stage + ((int64_t)q * n_p + v) * n_max;
  double *dst = out + (int64_t)v * ldo + off;
  const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  if (vec) {
    const int64_t n2 = rows / 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += stride)
      reinterpret_cast<f64x2 *>(dst)[i] = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(src) + i);
    if ((rows & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[rows - 1] = src[rows - 1];
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows; i += stride) dst[i] = src[i];
  }
}
}  // namespace

extern "C" int spr_field_unstage_blocks_f64(const double *d_stage, int32_t world, int32_t n_p, int64_t n_max,
                                            const int64_t *d_layout, double *d_out, int64_t ldo, void *stream) {
  SPR_REQUIRE(d_stage && d_out && d_layout, SPR_E_INVALID, "spr_field_unstage_blocks_f64: NULL pointer");
  SPR_REQUIRE(world > 0 && n_p > 0 && n_max > 0 && ldo > 0 && (int64_t)world * n_p <= 65535, SPR_E_INVALID,
              "spr_field_unstage_blocks_f64: bad shape world=%d n_p=%d n_max=%lld ldo=%lld", world, n_p, (long long)n_max,
              (long long)ldo);
  int64_t bx = (n_max / 2 + 255) / 256;
  if (bx > 1024) bx = 1024;
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(field_unstage_blocks_kernel, dim3((unsigned)bx, (unsigned)(world * n_p)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), d_stage, (int)n_p, n_max, d_layout, d_out, ldo);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}
