// Field uncertainty on the device: ROM.reconstruct_std.  Per-cell standard deviation of the reconstructed field when the
// coefficients carry a Gaussian uncertainty -- linear propagation through  x = X_scl (Ur a) + X_cnt.
//
// Diagonal form:  out[j, i] = s_i sqrt( sum_c Ur[i, c]^2 S[j, c]^2 )  for independent per-coefficient deviations S (k, r),
// the orientation of Ar_sigma.  This is the reconstruct pass (reconstruct.hip) with squares: 64-row panels staged raw in
// LDS by the rowtile.hpp loader, double-buffered; the squared deviations of up to 16 vectors are the MFMA A operand (in
// registers for the whole kernel), the panel entry is squared between the LDS read and the MFMA, the square root and the
// scale are applied before the store.  HBM-bound: one read of the basis block per 16 vectors, k n doubles written, no
// centre read.  r > SPR_MAX_R runs per 128-column group: the groups before the last leave the partial variance in out,
// the last one adds its own and closes with the root.
//
// Factor form:  out[j, i] = s_i || L_j^T u_i ||_2  for covariance factors Sigma_j = L_j L_j^T, L (k, r, q).  A tall-skinny
// product per vector followed by a row-wise sum of squares; 2 n r q k flops, MFMA-bound.  Loop order: PANEL outermost.  A
// workgroup stages one 64-row panel of the basis in LDS, every wave takes the B-operand fragments of its 16 rows into
// registers once, and then all k factors stream past the panel in slices of FS_SLW columns (A operand = slice^T from LDS,
// two independent accumulator tiles per wave).  The basis is read from HBM exactly once; the factors (k r q doubles, 0.5
// MB at k = 16, r = q = 64) are re-read once per panel and come from L2.  The other order (factor resident, panels inner)
// would read the n r basis block k times from HBM.  The next slice and the next panel wait in registers while the current
// slice is multiplied.  The accumulator tiles are squared and added per lane in a fixed order, slices in increasing order,
// and the four lane groups that share a row are closed with a two-step butterfly.
//
// Both forms: workgroups are dealt to feature segments (common.hpp), so s_i is a workgroup constant unless a rowscale is
// given; no atomics, plain stores, every output element has one writer: two runs agree bit for bit.  A NaN in S_j or L_j
// stays in row j of the MFMA result tiles, i.e. in output column j.  sqrt(0) = 0 exactly.
#include <math.h>

#include "rowtile.hpp"
#include "launch.hpp"

namespace {

constexpr int FS_THREADS = 256;
constexpr int FS_PB = 16;        // vectors per pass of the diagonal form (one MFMA tile of rows)
constexpr int FS_SLW = 32;       // factor columns per LDS slice: two MFMA tiles
// row stride of the slice image, whose ROWS are the contraction index: the 32 lanes of one ds_read_b64 group read 16
// consecutive doubles of two rows, which have to start 32 banks apart (stride = 16 mod 32 doubles)
constexpr int FS_SLP = FS_SLW + 16;

// ------------------------------------------------------------------------------------------------ diagonal form
template <int MTR, int VEC, typename TU>
__global__ __launch_bounds__(FS_THREADS) void field_std_diag_kernel(
    const TU *__restrict__ Ur, int r, int64_t ldu, SegPlan plan, const double *__restrict__ scale,
    const double *__restrict__ rowscale, const double *__restrict__ S, int64_t lds, int np0, int npb,
    double *__restrict__ out, int64_t ldo, int first, int last) {
  constexpr int NW = FS_THREADS / 64, R = 64;
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

  double vfrag[KSTEPS];          // MFMA A operand: A[i = lane & 15][k = lane >> 4] = S[np0 + i][4 ks + k]^2
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) {
    const int k = 4 * ks + (lane >> 4), j = lane & 15;
    const double s = (j < npb && k < r) ? S[(int64_t)(np0 + j) * lds + k] : 0.0;
    vfrag[ks] = s * s;
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
  const int ufrag = (lane & 15) * MP + (lane >> 4);   // B[k = lane >> 4][j = lane & 15] = panel[16 w + j][k0 + k]^2
  while (c < npanels) {
    const double *cur = buf ? lds1 : lds0;
    double *nxt = buf ? lds0 : lds1;
    const int64_t c2 = cn + wpf;
    const int64_t n2row0 = (c2 < npanels) ? lo + c2 * R : hi;
    __syncthreads();
    const int64_t row = lo + c * R + wave * 16 + (lane & 15);   // the panel row this lane's results belong to
    const int64_t rc = row < hi ? row : hi - 1;
    const double rs = rowscale ? rowscale[rc] : sc;              // sampled rows carry their own scale
    const double *p = cur + wave * 16 * MP + ufrag;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const double u = p[4 * ks];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vfrag[ks], u * u, acc, 0, 0, 0);
      if (ks == 0) {
#pragma unroll
        for (int it = 0; it < RT::IT; ++it) {
          tile.raw_store_pass(it, nxt, r, nrow0, hi, wave, lane);
          tile.template load_pass<VEC>(it, Ur, ldu, r, n2row0, hi, wave, lane);
        }
      }
    }
    // D[i = (lane >> 4) + 4 q][j = lane & 15] = variance of vector np0 + i at the row, in scaled units
    const double d[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int pv = 4 * q + (lane >> 4);
      if (pv < npb && row < hi) {
        double *o = out + (int64_t)(np0 + pv) * ldo + row;
        const double v = first ? d[q] : *o + d[q];     // column groups of a wide basis accumulate the variance in out
        *o = last ? rs * sqrt(v) : v;
      }
    }
    buf ^= 1;
    c = cn;
    cn = c2;
    nrow0 = n2row0;
  }
}

template <int MTR, typename TU>
int launch_diag(const TU *Ur, int32_t rg, int64_t ldu, SegPlan plan, const double *scale, const double *rowscale,
                const double *S, int64_t lds, int32_t k, double *out, int64_t ldo, int first, int last, hipStream_t st) {
  const int grid = spr_plan_grid(plan, spr_panel_per_cu(MTR), 64);
  const bool vec_ok = spr_pair_aligned(Ur, rg, ldu);
  for (int p0 = 0; p0 < k; p0 += FS_PB) {
    const int npb = (k - p0 < FS_PB) ? k - p0 : FS_PB;
#define FD(V) hipLaunchKernelGGL((field_std_diag_kernel<MTR, V, TU>), dim3(grid), dim3(FS_THREADS), 0, st, Ur, (int)rg, ldu, plan, scale, rowscale, S, lds, p0, npb, out, ldo, first, last)
    if (vec_ok) FD(1);
    else FD(0);
#undef FD
    SPR_LAUNCH_CHECK();
  }
  return SPR_OK;
}

// ------------------------------------------------------------------------------------------------ factor form
constexpr size_t factor_lds_bytes(int mtr) { return ((size_t)64 * (16 * mtr + 2) + (size_t)16 * mtr * FS_SLP) * sizeof(double); }

template <int MTR, int VEC, typename TU>
__global__ __launch_bounds__(FS_THREADS) void field_std_factor_kernel(
    const TU *__restrict__ Ur, int r, int64_t ldu, SegPlan plan, const double *__restrict__ scale,
    const double *__restrict__ rowscale, const double *__restrict__ L, int k, int q, double *__restrict__ out,
    int64_t ldo) {
  constexpr int NW = FS_THREADS / 64, R = 64;
  constexpr int MPAD = 16 * MTR, MP = MPAD + 2, KSTEPS = MPAD / 4;
  constexpr int LPT = MPAD * FS_SLW / FS_THREADS;     // slice elements per thread
  static_assert(FS_SLW == 32 && (MPAD * FS_SLW) % FS_THREADS == 0, "slice staging assumes 32 columns, 8 rows per sweep");
  using RT = RowTile<MTR, R, MP, NW, 16, TU>;
  __shared__ double us[R * MP];                       // the panel; at r = q = 128: 65 KB + 48 KB of the 160 KB
  __shared__ double ls[MPAD * FS_SLP];                // one slice of one factor, rows = contraction index
  int f, wl, wpf, base;
  int64_t lo, hi;
  if (!seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const double sc = scale[f];
  const int64_t rq = (int64_t)r * q;

  // slice staging: thread (c0 = tid >> 5, t = tid & 31) moves rows c0 + 8 i of column t0 + t.  Branch-free: entries past
  // the factor are read from its first element and stored as zeros.
  const int sc0 = threadIdx.x >> 5, st = threadIdx.x & 31;
  double lpre[LPT];
  auto load_slice = [&](int j, int t0) {
    const double *Lj = L + (int64_t)j * rq;
    const bool tv = t0 + st < q;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int cc = sc0 + 8 * i;
      lpre[i] = Lj[(tv && cc < r) ? (int64_t)cc * q + t0 + st : 0];
    }
  };
  auto store_slice = [&](int t0) {
    const bool tv = t0 + st < q;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int cc = sc0 + 8 * i;
      ls[cc * FS_SLP + st] = (tv && cc < r) ? lpre[i] : 0.0;
    }
  };

  RT tile;
  const int64_t npanels = (hi - lo + R - 1) / R;
  int64_t c = wl;
  if (c >= npanels) return;                           // workgroup-uniform
  tile.template load<VEC>(Ur, ldu, r, lo + c * R, hi, wave, lane);
  load_slice(0, 0);
  const int ufrag = (lane & 15) * MP + (lane >> 4);   // B[k = lane >> 4][j = lane & 15] = panel[16 w + j][4 ks + k]
  const int lfrag = (lane >> 4) * FS_SLP + (lane & 15);   // A[i = lane & 15][k = lane >> 4] = slice[4 ks + k][16 tile + i]
  double ub[KSTEPS];
  while (c < npanels) {
    const int64_t crow0 = lo + c * R;
    const int64_t cn = c + wpf;
    const int64_t nrow0 = (cn < npanels) ? lo + cn * R : hi;   // past-the-end panel: a harmless re-read of the last row
    __syncthreads();             // every wave is done with the previous panel and its last slice
    tile.raw_store(us, r, crow0, hi, wave, lane);
    tile.template load<VEC>(Ur, ldu, r, nrow0, hi, wave, lane);
    const int64_t row = crow0 + wave * 16 + (lane & 15);        // the panel row this lane's results belong to
    const int64_t rc = row < hi ? row : hi - 1;
    const double rs = rowscale ? rowscale[rc] : sc;
    double ss = 0.0;
    int j = 0, t0 = 0;
    for (int s = 0; s < k; ) {   // s counts the finished factors; (j, t0) is the slice being multiplied
      if (j > 0 || t0 > 0) __syncthreads();           // the previous slice has been consumed
      store_slice(t0);
      const bool endj = t0 + FS_SLW >= q;
      const int jn = endj ? (j + 1 < k ? j + 1 : 0) : j, tn = endj ? 0 : t0 + FS_SLW;
      load_slice(jn, tn);                             // the slice after this one (the next panel starts at (0, 0) again)
      __syncthreads();
      if (j == 0 && t0 == 0) {
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) ub[ks] = us[wave * 16 * MP + ufrag + 4 * ks];
      }
      const double *lp = ls + lfrag;
      f64x4 a0 = {0.0, 0.0, 0.0, 0.0}, a1 = {0.0, 0.0, 0.0, 0.0};
      if (t0 + 16 < q) {                              // both tiles hold columns of the factor
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
          a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lp[4 * ks * FS_SLP], ub[ks], a0, 0, 0, 0);
          a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(lp[4 * ks * FS_SLP + 16], ub[ks], a1, 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lp[4 * ks * FS_SLP], ub[ks], a0, 0, 0, 0);
      }
      // D[i = (lane >> 4) + 4 e][j = lane & 15] = (L_j^T u_row)[t0 + 16 tile + i]; fixed order of the additions
      ss += a0.x * a0.x;
      ss += a0.y * a0.y;
      ss += a0.z * a0.z;
      ss += a0.w * a0.w;
      ss += a1.x * a1.x;
      ss += a1.y * a1.y;
      ss += a1.z * a1.z;
      ss += a1.w * a1.w;
      if (endj) {
        double v = ss + __shfl_xor(ss, 16, 64);       // the four lane groups hold four columns each of the same row
        v += __shfl_xor(v, 32, 64);
        if (lane < 16 && row < hi) out[(int64_t)j * ldo + row] = rs * sqrt(v);
        ss = 0.0;
        ++s;
      }
      j = endj ? j + 1 : j;
      t0 = tn;
    }
    c = cn;
  }
}

template <int MTR, typename TU>
int launch_factor(const TU *Ur, int32_t r, int64_t ldu, SegPlan plan, const double *scale, const double *rowscale,
                  const double *L, int32_t k, int32_t q, double *out, int64_t ldo, hipStream_t st) {
  int per_cu = (int)((160 * 1024) / factor_lds_bytes(MTR));
  per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
  const int grid = spr_plan_grid(plan, per_cu, 64);
  const bool vec_ok = spr_pair_aligned(Ur, r, ldu);
#define FF(V) hipLaunchKernelGGL((field_std_factor_kernel<MTR, V, TU>), dim3(grid), dim3(FS_THREADS), 0, st, Ur, (int)r, ldu, plan, scale, rowscale, L, (int)k, (int)q, out, ldo)
  if (vec_ok) FF(1);
  else FF(0);
#undef FF
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

// ------------------------------------------------------------------------------------------------ host side
int check_common(const char *name, const void *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                 int32_t n_features, const double *d_scale, const double *d_in, int32_t k, const double *d_out, int64_t ldo) {
  SPR_REQUIRE(d_Ur && d_scale && d_in && d_out, SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(n_rows > 0 && r > 0 && ldu >= r && k > 0 && ldo >= n_rows, SPR_E_INVALID,
              "%s: bad shape n_rows=%lld r=%d ldu=%lld k=%d ldo=%lld", name, (long long)n_rows, r, (long long)ldu, k,
              (long long)ldo);
  SPR_REQUIRE_LAYOUT(name, row0, n_rows, n_points, n_features);
  return SPR_OK;
}

template <typename TU>
int field_std_diag(const char *name, const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                   int32_t n_features, const double *d_scale, const double *d_rowscale, const double *d_S, int32_t k,
                   double *d_out, int64_t ldo, void *stream) {
  int rc = check_common(name, d_Ur, n_rows, r, ldu, row0, n_points, n_features, d_scale, d_S, k, d_out, ldo);
  if (rc != SPR_OK) return rc;
  SPR_REQUIRE(r <= SPR_MAX_R_WIDE, SPR_E_UNSUPPORTED, "%s: r = %d exceeds %d", name, r, SPR_MAX_R_WIDE);
  hipStream_t st = static_cast<hipStream_t>(stream);
  SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, 64);
  for (int g0 = 0; g0 < r; g0 += SPR_MAX_R) {
    const int rg = (r - g0 < SPR_MAX_R) ? r - g0 : SPR_MAX_R;
    const int first = g0 == 0, last = g0 + rg == r;
    SPR_DISPATCH_MT(spr_round_mt(rg), name, rg,   // padded width of the group in 16-column tiles
                    rc = launch_diag<RUNG, TU>(d_Ur + g0, rg, ldu, plan, d_scale, d_rowscale, d_S + g0, (int64_t)r, k, d_out,
                                               ldo, first, last, st))
    if (rc != SPR_OK) return rc;
  }
  return SPR_OK;
}

template <typename TU>
int field_std_factor(const char *name, const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0,
                     int64_t n_points, int32_t n_features, const double *d_scale, const double *d_rowscale,
                     const double *d_L, int32_t k, int32_t q, double *d_out, int64_t ldo, void *stream) {
  int rc = check_common(name, d_Ur, n_rows, r, ldu, row0, n_points, n_features, d_scale, d_L, k, d_out, ldo);
  if (rc != SPR_OK) return rc;
  SPR_REQUIRE(r <= SPR_MAX_R, SPR_E_INVALID, "%s: r = %d exceeds %d (the factor form keeps a whole basis row per panel)",
              name, r, SPR_MAX_R);
  SPR_REQUIRE(q >= 1 && q <= r, SPR_E_INVALID, "%s: q = %d outside [1, r = %d]", name, q, r);
  hipStream_t st = static_cast<hipStream_t>(stream);
  SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, 64);
  SPR_DISPATCH_MT(spr_round_mt(r), name, r,
                  rc = launch_factor<RUNG, TU>(d_Ur, r, ldu, plan, d_scale, d_rowscale, d_L, k, q, d_out, ldo, st))
  return rc;
}

}  // namespace

// TU = float: basis stored as f32, widened exactly; arithmetic and output f64
#define SPR_FIELD_STD_DIAG_ENTRY(NAME, TU)                                                                                    \
  SPR_ENTRY(NAME,                                                                                                             \
            (const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points, int32_t n_features,      \
             const double *d_scale, const double *d_rowscale, const double *d_S, int32_t k, double *d_out, int64_t ldo,       \
             void *stream),                                                                                                   \
            (field_std_diag<TU>), d_Ur, n_rows, r, ldu, row0, n_points, n_features, d_scale, d_rowscale, d_S, k, d_out, ldo,  \
            stream)
SPR_FIELD_STD_DIAG_ENTRY(spr_field_std_diag_f64, double)
SPR_FIELD_STD_DIAG_ENTRY(spr_field_std_diag_u32, float)
#undef SPR_FIELD_STD_DIAG_ENTRY

#define SPR_FIELD_STD_FACTOR_ENTRY(NAME, TU)                                                                                  \
  SPR_ENTRY(NAME,                                                                                                             \
            (const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points, int32_t n_features,      \
             const double *d_scale, const double *d_rowscale, const double *d_L, int32_t k, int32_t q, double *d_out,         \
             int64_t ldo, void *stream),                                                                                      \
            (field_std_factor<TU>), d_Ur, n_rows, r, ldu, row0, n_points, n_features, d_scale, d_rowscale, d_L, k, q, d_out,  \
            ldo, stream)
SPR_FIELD_STD_FACTOR_ENTRY(spr_field_std_factor_f64, double)
SPR_FIELD_STD_FACTOR_ENTRY(spr_field_std_factor_u32, float)
#undef SPR_FIELD_STD_FACTOR_ENTRY
