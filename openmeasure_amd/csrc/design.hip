// Design sweep for SPR.augment_placement / placement_gain: the score of every row of the basis as the NEXT sensor of a
// sequential optimal design.  With M the information matrix of the sensors placed so far and B = M^-1 (symmetric, r x r,
// formed on the host), a candidate row u with weight w is scored from  z = B u,  d = u^T z,  q = z^T z:
//   criterion 0 (D):  w d                 det(M + w u u^T) = det M (1 + w d)
//   criterion 1 (A):  w q / (1 + w d)     the Sherman-Morrison drop of trace M^-1
// One streaming read of the basis block per sweep, 2 n r^2 flops on the f64 MFMA against 8 n r bytes.
//
// The factor form of field_std.hip with k = 1, q = r: a workgroup stages one 64-row panel in LDS (rowtile.hpp), every
// wave takes the B-operand fragments of its 16 rows into registers once, and B streams past the panel in slices of
// DS_SLW columns (A operand = slice^T from LDS, two independent accumulator tiles per wave; B is re-read once per panel
// and comes from L2).  The kernel multiplies by B^T: the caller passes a symmetric matrix.  The result tile holds z
// entries of ONE row per lane -- z[t0 + 16 tile + (lane >> 4) + 4 e] of panel row lane & 15 --; z^2 and z u are
// accumulated per lane in a fixed order (slices, tiles, e increasing), u read from the LDS panel (8 reads per slice next
// to the 64 of the A operand: the entries also sit in the lane's operand fragment, but indexing that needs the slice
// loop unrolled, which costs 222 AGPRs of copies and 138 spilled SGPRs at r = 128), and the four lane groups that share
// a row are closed with a two-step butterfly.
//
// Every lane of the first group keeps a running best and runner-up (worst.hpp's rules with two entries: strict
// comparison, so the lowest row keeps a tie; NaN never wins); lanes, waves and workgroups are merged by (value, lowest
// row); every workgroup writes its slot with plain stores and a one-workgroup kernel merges the slots and copies the
// winner's row of the basis into the record.  No atomics: two runs agree bit for bit.  The weight is a workgroup
// constant (workgroups are dealt to feature segments, common.hpp).
#include <math.h>

#include "rowtile.hpp"
#include "launch.hpp"

namespace {

constexpr int DS_THREADS = 256;
constexpr int DS_SLW = 32;       // columns of B per LDS slice: two MFMA tiles
constexpr int DS_SLP = DS_SLW + 16;   // row stride of the slice image (field_std.hip, FS_SLP)
constexpr int DS_SLOT = 3;       // doubles per workgroup slot: best score, its global row, runner-up score
constexpr int DS_PER_CU_MAX = 4;

// Running best and runner-up VALUE of a sweep; rows are visited in increasing order.  push only takes nv > v, so an empty
// entry (row < 0) holds -inf and a NaN is never stored.  v2 is the second-largest score over all rows but the best one
// (equal to v for a tie).
struct Best2 {
  double v, v2;
  int64_t row;
  __device__ inline void init() { v = -INFINITY; v2 = -INFINITY; row = -1; }
  __device__ inline void push(double nv, int64_t nrow, bool valid) {
    const bool take = valid && nv > v;                 // strict: the lowest row keeps a tie
    const bool second = valid && !take && nv > v2;
    v2 = take ? v : (second ? nv : v2);
    v = take ? nv : v;
    row = take ? nrow : row;
  }
  __device__ inline void merge(double ov, int64_t orow, double ov2) {
    const bool take = orow >= 0 && (row < 0 || ov > v || (ov == v && orow < row));
    const double lose = take ? v : ov;                 // the best of the side that lost (-inf when that side is empty)
    v2 = fmax(fmax(v2, ov2), lose);
    v = take ? ov : v;
    row = take ? orow : row;
  }
  __device__ inline void merge_lanes(int width) {      // butterfly over aligned groups of `width` lanes
    for (int o = width >> 1; o > 0; o >>= 1) {
      const double ov = __shfl_xor(v, o, 64), ov2 = __shfl_xor(v2, o, 64);
      const long long orow = __shfl_xor((long long)row, o, 64);
      merge(ov, (int64_t)orow, ov2);
    }
  }
};

constexpr size_t design_lds_bytes(int mtr) {
  return ((size_t)64 * (16 * mtr + 2) + (size_t)16 * mtr * DS_SLP + 4 * DS_SLOT) * sizeof(double);
}

template <int MTR, int VEC, typename TU>
__global__ __launch_bounds__(DS_THREADS) void design_sweep_kernel(
    const TU *__restrict__ Ur, int r, int64_t ldu, SegPlan plan, const double *__restrict__ B,
    const double *__restrict__ wfeat, const double *__restrict__ alive, int criterion, double *__restrict__ scores,
    double *__restrict__ slots) {
  constexpr int NW = DS_THREADS / 64, R = 64;
  constexpr int MPAD = 16 * MTR, MP = MPAD + 2, KSTEPS = MPAD / 4;
  constexpr int LPT = MPAD * DS_SLW / DS_THREADS;     // slice elements per thread
  static_assert(DS_SLW == 32 && (MPAD * DS_SLW) % DS_THREADS == 0, "slice staging assumes 32 columns, 8 rows per sweep");
  using RT = RowTile<MTR, R, MP, NW, 16, TU>;
  __shared__ double us[R * MP];                       // the panel
  __shared__ double ls[MPAD * DS_SLP];                // one slice of B, rows = contraction index
  __shared__ double red[NW * DS_SLOT];
  double *const slot = slots + (int64_t)blockIdx.x * DS_SLOT;
  int f, wl, wpf, base;
  int64_t lo, hi;
  const bool located = seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi);
  const int64_t npanels = located ? (hi - lo + R - 1) / R : 0;
  int64_t c = located ? wl : 0;
  if (c >= npanels) {                                 // workgroup-uniform; the grid has no such workgroup (seg_wgs)
    if (threadIdx.x == 0) { slot[0] = -INFINITY; slot[1] = -1.0; slot[2] = -INFINITY; }
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const double w = wfeat ? wfeat[f] : 1.0;

  // slice staging: thread (c0 = tid >> 5, t = tid & 31) moves rows c0 + 8 i of column t0 + t.  Branch-free: entries past
  // the matrix are read from its first element and stored as zeros.
  const int sc0 = threadIdx.x >> 5, st = threadIdx.x & 31;
  double lpre[LPT];
  auto load_slice = [&](int t0) {
    const bool tv = t0 + st < r;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int cc = sc0 + 8 * i;
      lpre[i] = B[(tv && cc < r) ? cc * r + t0 + st : 0];
    }
  };
  auto store_slice = [&](int t0) {
    const bool tv = t0 + st < r;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int cc = sc0 + 8 * i;
      ls[cc * DS_SLP + st] = (tv && cc < r) ? lpre[i] : 0.0;
    }
  };

  RT tile;
  Best2 best;
  best.init();
  tile.template load<VEC>(Ur, ldu, r, lo + c * R, hi, wave, lane);
  load_slice(0);
  const int ufrag = (lane & 15) * MP + (lane >> 4);   // B[k = lane >> 4][j = lane & 15] = panel[16 w + j][4 ks + k]
  const int lfrag = (lane >> 4) * DS_SLP + (lane & 15);   // A[i = lane & 15][k = lane >> 4] = slice[4 ks + k][16 tile + i]
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
    const double al = alive ? alive[rc] : 0.0;                  // requested before the MFMAs
    double dd = 0.0, qq = 0.0;
#pragma nounroll
    for (int t0 = 0; t0 < MPAD; t0 += DS_SLW) {       // rolled, as in the factor form: one copy of the MFMA loop
      if (t0 > 0) __syncthreads();                    // the previous slice has been consumed
      store_slice(t0);
      load_slice(t0 + DS_SLW < MPAD ? t0 + DS_SLW : 0);   // the slice after this one (the next panel starts at 0 again)
      __syncthreads();
      if (t0 == 0) {
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) ub[ks] = us[wave * 16 * MP + ufrag + 4 * ks];
      }
      const double *lp = ls + lfrag;
      const double *up = us + wave * 16 * MP + ufrag + t0;   // u_row[t0 + 16 tile + (lane >> 4) + 4 e] = up[16 tile + 4 e]
      // D[i = (lane >> 4) + 4 e][j = lane & 15] = (B^T u_row)[t0 + 16 tile + i]; fixed order of the additions
      f64x4 a0 = {0.0, 0.0, 0.0, 0.0}, a1 = {0.0, 0.0, 0.0, 0.0};
      const bool two = t0 + 16 < r;                   // both tiles hold columns of B (wave-uniform)
      if (two) {
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
          a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lp[4 * ks * DS_SLP], ub[ks], a0, 0, 0, 0);
          a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(lp[4 * ks * DS_SLP + 16], ub[ks], a1, 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(lp[4 * ks * DS_SLP], ub[ks], a0, 0, 0, 0);
      }
      qq += a0.x * a0.x; dd += a0.x * up[0];
      qq += a0.y * a0.y; dd += a0.y * up[4];
      qq += a0.z * a0.z; dd += a0.z * up[8];
      qq += a0.w * a0.w; dd += a0.w * up[12];
      if (two) {
        qq += a1.x * a1.x; dd += a1.x * up[16];
        qq += a1.y * a1.y; dd += a1.y * up[20];
        qq += a1.z * a1.z; dd += a1.z * up[24];
        qq += a1.w * a1.w; dd += a1.w * up[28];
      }
    }
    dd += __shfl_xor(dd, 16, 64);                     // the four lane groups hold four columns each of the same row
    dd += __shfl_xor(dd, 32, 64);
    qq += __shfl_xor(qq, 16, 64);
    qq += __shfl_xor(qq, 32, 64);
    const double wd = w * dd;
    const double sc = criterion ? w * qq / (1.0 + wd) : wd;
    const bool own = lane < 16 && row < hi, ok = own && !(al < 0.0);
    if (scores && own) scores[row] = ok ? sc : -INFINITY;
    best.push(sc, plan.row0 + row, ok);
    c = cn;
  }
  best.merge_lanes(16);          // lanes 0 .. 15 hold the 16 rows of the wave; then the four waves through LDS
  if (lane == 0) { red[wave * DS_SLOT] = best.v; red[wave * DS_SLOT + 1] = (double)best.row; red[wave * DS_SLOT + 2] = best.v2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    Best2 a;
    a.init();
    for (int wv = 0; wv < NW; ++wv) a.merge(red[wv * DS_SLOT], (int64_t)red[wv * DS_SLOT + 1], red[wv * DS_SLOT + 2]);
    slot[0] = a.v; slot[1] = (double)a.row; slot[2] = a.v2;
  }
}

// One workgroup: merge of the slots (a total order -- larger value, then the lower row -- so the result does not depend on
// the grid) and the record: best score, its global row, the runner-up's score, the winner's row of the basis.
template <typename TU>
__global__ __launch_bounds__(DS_THREADS) void design_merge_kernel(const double *__restrict__ slots, int nslots,
                                                                  const TU *__restrict__ Ur, int r, int64_t ldu, int64_t row0,
                                                                  int64_t n_rows, double *__restrict__ rec) {
  constexpr int NW = DS_THREADS / 64;
  __shared__ double red[NW * DS_SLOT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Best2 b;
  b.init();
  for (int s = threadIdx.x; s < nslots; s += DS_THREADS)
    b.merge(slots[(int64_t)s * DS_SLOT], (int64_t)slots[(int64_t)s * DS_SLOT + 1], slots[(int64_t)s * DS_SLOT + 2]);
  b.merge_lanes(64);
  if (lane == 0) { red[wave * DS_SLOT] = b.v; red[wave * DS_SLOT + 1] = (double)b.row; red[wave * DS_SLOT + 2] = b.v2; }
  __syncthreads();
  Best2 a;
  a.init();
  for (int wv = 0; wv < NW; ++wv) a.merge(red[wv * DS_SLOT], (int64_t)red[wv * DS_SLOT + 1], red[wv * DS_SLOT + 2]);
  if (threadIdx.x == 0) { rec[0] = a.v; rec[1] = (double)a.row; rec[2] = a.v2; }
  const int64_t loc = a.row - row0;
  const bool have = a.row >= 0 && loc >= 0 && loc < n_rows;
  for (int cidx = threadIdx.x; cidx < r; cidx += DS_THREADS) rec[3 + cidx] = have ? (double)Ur[loc * ldu + cidx] : 0.0;
}

// workgroups the sweep may launch for a block with n_features features (seg_wgs: at least one per feature present)
inline int64_t ds_max_slots(int32_t n_features) { return (int64_t)DS_PER_CU_MAX * spr_cus_or_default() + n_features; }

template <int MTR, typename TU>
int launch_design(const char *name, const TU *Ur, int32_t r, int64_t ldu, SegPlan plan, const double *B, const double *wfeat,
                  const double *alive, int criterion, double *scores, double *slots, int &nslots, int64_t max_slots,
                  hipStream_t st) {
  int per_cu = (int)((160 * 1024) / design_lds_bytes(MTR));
  per_cu = per_cu < 1 ? 1 : (per_cu > DS_PER_CU_MAX ? DS_PER_CU_MAX : per_cu);
  const int grid = spr_plan_grid(plan, per_cu, 64);
  SPR_REQUIRE_GRID(name, grid, max_slots);
  nslots = grid;
  const bool vec_ok = spr_pair_aligned(Ur, r, ldu);
#define DSW(V) hipLaunchKernelGGL((design_sweep_kernel<MTR, V, TU>), dim3(grid), dim3(DS_THREADS), 0, st, Ur, (int)r, ldu, plan, B, wfeat, alive, criterion, scores, slots)
  if (vec_ok) DSW(1);
  else DSW(0);
#undef DSW
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

template <typename TU>
int design_sweep(const char *name, const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                 int32_t n_features, const double *d_B, const double *d_wfeat, const double *d_alive, int32_t criterion,
                 double *d_scores, double *d_rec, void *d_workspace, size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_Ur && d_B && d_rec && d_workspace, SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(n_rows > 0 && r > 0 && ldu >= r, SPR_E_INVALID, "%s: bad shape n_rows=%lld r=%d ldu=%lld", name,
              (long long)n_rows, r, (long long)ldu);
  SPR_REQUIRE_LAYOUT(name, row0, n_rows, n_points, n_features);
  SPR_REQUIRE(criterion == 0 || criterion == 1, SPR_E_INVALID, "%s: criterion = %d is neither 0 (D) nor 1 (A)", name,
              criterion);
  SPR_REQUIRE(r <= SPR_MAX_R, SPR_E_UNSUPPORTED, "%s: r = %d exceeds %d (the sweep keeps a whole basis row per panel)", name,
              r, SPR_MAX_R);
  SPR_REQUIRE(workspace_bytes >= spr_design_sweep_workspace(r, n_features), SPR_E_INVALID,
              "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, spr_design_sweep_workspace(r, n_features));
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *slots = static_cast<double *>(d_workspace);
  SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, 64);
  const int64_t max_slots = ds_max_slots(n_features);
  int nslots = 0, rc = SPR_OK;
  SPR_DISPATCH_MT(spr_round_mt(r), name, r,
                  rc = launch_design<RUNG, TU>(name, d_Ur, r, ldu, plan, d_B, d_wfeat, d_alive, (int)criterion, d_scores,
                                               slots, nslots, max_slots, st))
  if (rc != SPR_OK) return rc;
  hipLaunchKernelGGL((design_merge_kernel<TU>), dim3(1), dim3(DS_THREADS), 0, st, slots, nslots, d_Ur, (int)r, ldu, row0,
                     n_rows, d_rec);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

}  // namespace

extern "C" size_t spr_design_sweep_workspace(int32_t r, int32_t n_features) {
  if (r <= 0 || r > SPR_MAX_R || n_features <= 0) return 0;
  return (size_t)ds_max_slots(n_features) * DS_SLOT * sizeof(double);
}

// TU = float: basis stored as f32, widened exactly; arithmetic and record f64
#define SPR_DESIGN_SWEEP_ENTRY(NAME, TU)                                                                                      \
  SPR_ENTRY(NAME,                                                                                                             \
            (const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points, int32_t n_features,      \
             const double *d_B, const double *d_wfeat, const double *d_alive, int32_t criterion, double *d_scores,            \
             double *d_rec, void *d_workspace, size_t workspace_bytes, void *stream),                                         \
            (design_sweep<TU>), d_Ur, n_rows, r, ldu, row0, n_points, n_features, d_B, d_wfeat, d_alive, criterion, d_scores,  \
            d_rec, d_workspace, workspace_bytes, stream)
SPR_DESIGN_SWEEP_ENTRY(spr_design_sweep_f64, double)
SPR_DESIGN_SWEEP_ENTRY(spr_design_sweep_u32, float)
#undef SPR_DESIGN_SWEEP_ENTRY
