// Bound sweep for train(method='COLS'):  which rows of  lo0 <= Ur g <= hi0  does a coefficient vector g violate?
//
// The reconstruct pass (reconstruct.hip) without its store.  The reference builds two n-sized limit vectors
// (sparse_sensing.py:883, scale_limits :173-210) and hands all 2 n rows to a conic solver (:886-889); the
// constraint-generation driver (openmeasure_amd/_cols.py) only needs, per vector, the worst violation, the number of
// violated rows and a short list of badly violated rows to add to its working set.  One streaming read of Ur and
// rowmean (8 r + 8 bytes per row for an f64 basis), nothing n-sized is written.
//
// The scaled limits are formed on the fly from the per-feature limits: lo0_i = (lo_f - X_cnt_i) / X_scl_f with the
// same operations, in the same order, as ROM.scale_limits does on the host (so both agree bit for bit), unless the
// clamp entry of the feature is not NaN: then the whole feature block takes that constant (:201-204, +-1000).
//
// Layout: workgroups are dealt to feature segments (common.hpp) so limits, clamps and scale are workgroup constants.
// Within a feature every workgroup takes ONE CONTIGUOUS run of 64-row panels: neighbouring cells violate together,
// so a contiguous run per workgroup spreads the per-workgroup candidates over the domain (a strided deal would make
// every workgroup report a row of the same blob).  r <= 128: the MFMA panel form of reconstruct.hip (vectors as the
// A operand, rowtile.hpp panels double-buffered in LDS); the result tile has the panel row across the 16 lanes of a
// group, so a lane compares 4 values of ONE row per panel and keeps a running (max, row) per side and a count per
// vector; one cross-lane reduction when the workgroup's rows are done.  r > 128 (up to SPR_MAX_R_WIDE): a wave per
// row, lanes across the columns, the vectors in LDS.  Every workgroup writes its slot with plain stores; a second
// small kernel (one workgroup per vector) merges the slots.  No atomics: results are deterministic for a fixed grid.
#include <math.h>

#include <type_traits>

#include "rowtile.hpp"
#include "worst.hpp"
#include "launch.hpp"

namespace {

constexpr int BS_THREADS = 256;
constexpr int BS_PB = 16;        // coefficient vectors per pass of the MFMA form
constexpr int BS_WPB = 4;        // ... of the wide form
constexpr int BS_SLOT = 5;       // doubles per (vector, workgroup) slot: v_lo, row_lo, v_hi, row_hi, count
constexpr int BS_MAX_K = 256;

struct FeatLimits {              // workgroup constants of one feature
  double lo, hi, clo, chi, sc;
  __device__ inline void load(const double *limits, const double *clamp, const double *scale, int f, int F) {
    lo = limits[f]; hi = limits[F + f]; clo = clamp[f]; chi = clamp[F + f]; sc = scale[f];
  }
  __device__ inline double lo0(double mu) const { return isnan(clo) ? (lo - mu) / sc : clo; }
  __device__ inline double hi0(double mu) const { return isnan(chi) ? (hi - mu) / sc : chi; }
};

// contiguous run of panels of workgroup wl out of wpf (wpf <= npanels by seg_wgs): never empty
__device__ inline void panel_run(int64_t npanels, int wl, int wpf, int64_t &c0, int64_t &c1) {
  c0 = npanels * wl / wpf;
  c1 = npanels * (wl + 1) / wpf;
}

template <int MTR, int VEC, typename TU>
__global__ __launch_bounds__(BS_THREADS) void bound_sweep_mfma_kernel(
    const TU *__restrict__ Ur, int r, int64_t ldu, SegPlan plan, const double *__restrict__ rowmean,
    const double *__restrict__ scale, const double *__restrict__ limits, const double *__restrict__ clamp,
    const double *__restrict__ G, int np0, int npb, double tol, double *__restrict__ slots, int nslots) {
  constexpr int NW = BS_THREADS / 64, R = 64;
  constexpr int MPAD = 16 * MTR, MP = MPAD + 2, KSTEPS = MPAD / 4;
  using RT = RowTile<MTR, R, MP, NW, 16, TU>;
  __shared__ double smem[2 * R * MP];                 // >= 2304 doubles; the end-of-kernel merge needs 320
  double *const lds0 = smem, *const lds1 = smem + R * MP;
  int f, wl, wpf, base;
  int64_t lo, hi;
  if (!seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  FeatLimits fl;
  fl.load(limits, clamp, scale, f, plan.n_features);

  double vfrag[KSTEPS];          // MFMA A operand: A[i = lane & 15][k = lane >> 4] = vector np0+i, entry 4 ks + k
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) {
    const int k = 4 * ks + (lane >> 4), j = lane & 15;
    vfrag[ks] = (j < npb && k < r) ? G[(int64_t)(np0 + j) * r + k] : 0.0;
  }
  Worst wlo[4], whi[4];          // vector pv = 4 q + (lane >> 4)
  int cnt[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { wlo[q].init(); whi[q].init(); cnt[q] = 0; }

  RT tile;
  const int64_t npanels = (hi - lo + R - 1) / R;
  int64_t c, cend;
  panel_run(npanels, wl, wpf, c, cend);
  tile.template load<VEC>(Ur, ldu, r, lo + c * R, hi, wave, lane);
  tile.raw_store(lds0, r, lo + c * R, hi, wave, lane);
  int64_t nrow0 = (c + 1 < cend) ? lo + (c + 1) * R : hi;
  tile.template load<VEC>(Ur, ldu, r, nrow0, hi, wave, lane);
  int buf = 0;
  const int ufrag = (lane & 15) * MP + (lane >> 4);   // B[k = lane >> 4][j = lane & 15] = panel[16 w + j][k0 + k]
  while (c < cend) {
    const double *cur = buf ? lds1 : lds0;
    double *nxt = buf ? lds0 : lds1;
    const int64_t n2row0 = (c + 2 < cend) ? lo + (c + 2) * R : hi;
    __syncthreads();
    const int64_t row = lo + c * R + wave * 16 + (lane & 15);   // the panel row this lane's results belong to
    const int64_t rc = row < hi ? row : hi - 1;
    const double mu = rowmean[rc];                               // requested before the MFMAs
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
    // D[i = (lane >> 4) + 4 q][j = lane & 15] = g_{np0+i} . u_row
    const double l0 = fl.lo0(mu), h0 = fl.hi0(mu);
    const double d[4] = {acc.x, acc.y, acc.z, acc.w};
    const int64_t grow = plan.row0 + row;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool ok = (4 * q + (lane >> 4)) < npb && row < hi;
      const double vl = l0 - d[q], vh = d[q] - h0;
      wlo[q].push(vl, grow, ok);
      whi[q].push(vh, grow, ok);
      cnt[q] += (ok && (vl > tol || vh > tol)) ? 1 : 0;
    }
    buf ^= 1;
    ++c;
    nrow0 = n2row0;
  }
  // the 16 lanes of a group hold 16 rows of the same four vectors; then the four waves through LDS
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    wlo[q].merge_lanes(16);
    whi[q].merge_lanes(16);
    for (int o = 8; o > 0; o >>= 1) cnt[q] += __shfl_xor(cnt[q], o, 64);
  }
  __syncthreads();               // the panels are done with
  if ((lane & 15) == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double *s = smem + (wave * BS_PB + 4 * q + (lane >> 4)) * BS_SLOT;
      s[0] = wlo[q].v; s[1] = (double)wlo[q].row; s[2] = whi[q].v; s[3] = (double)whi[q].row; s[4] = (double)cnt[q];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < npb) {
    Worst a, b;
    a.init(); b.init();
    double n = 0.0;
    for (int w = 0; w < NW; ++w) {
      const double *s = smem + (w * BS_PB + threadIdx.x) * BS_SLOT;
      a.merge(s[0], (int64_t)s[1]);
      b.merge(s[2], (int64_t)s[3]);
      n += s[4];
    }
    double *o = slots + ((int64_t)(np0 + threadIdx.x) * nslots + blockIdx.x) * BS_SLOT;
    o[0] = a.v; o[1] = (double)a.row; o[2] = b.v; o[3] = (double)b.row; o[4] = n;
  }
}

// r > SPR_MAX_R: one wave per row, lanes stride the columns (8 r contiguous bytes per row), BS_WPB vectors per pass kept
// in LDS.  After the butterfly every lane holds the same sums, so every lane keeps the same running state.
template <typename TU>
__global__ __launch_bounds__(BS_THREADS) void bound_sweep_wide_kernel(
    const TU *__restrict__ Ur, int r, int64_t ldu, SegPlan plan, const double *__restrict__ rowmean,
    const double *__restrict__ scale, const double *__restrict__ limits, const double *__restrict__ clamp,
    const double *__restrict__ G, int np0, int npb, double tol, double *__restrict__ slots, int nslots) {
  constexpr int NW = BS_THREADS / 64, R = 64;
  __shared__ double gl[BS_WPB * SPR_MAX_R_WIDE];
  __shared__ double red[NW * BS_WPB * BS_SLOT];
  int f, wl, wpf, base;
  int64_t lo, hi;
  if (!seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  FeatLimits fl;
  fl.load(limits, clamp, scale, f, plan.n_features);
  for (int i = threadIdx.x; i < BS_WPB * r; i += BS_THREADS) {
    const int p = i / r, k = i - p * r;
    gl[i] = p < npb ? G[(int64_t)(np0 + p) * r + k] : 0.0;
  }
  __syncthreads();
  Worst wlo[BS_WPB], whi[BS_WPB];
  int cnt[BS_WPB];
#pragma unroll
  for (int p = 0; p < BS_WPB; ++p) { wlo[p].init(); whi[p].init(); cnt[p] = 0; }
  const int64_t npanels = (hi - lo + R - 1) / R;
  int64_t c0, c1;
  panel_run(npanels, wl, wpf, c0, c1);
  int64_t rend = lo + c1 * R;
  rend = rend < hi ? rend : hi;
  for (int64_t row = lo + c0 * R + wave; row < rend; row += NW) {
    const TU *rp = Ur + row * ldu;
    double s[BS_WPB];
#pragma unroll
    for (int p = 0; p < BS_WPB; ++p) s[p] = 0.0;
    for (int k = lane; k < r; k += 64) {
      const double u = (double)rp[k];
#pragma unroll
      for (int p = 0; p < BS_WPB; ++p) s[p] += u * gl[p * r + k];
    }
    const double mu = rowmean[row];
    const double l0 = fl.lo0(mu), h0 = fl.hi0(mu);
#pragma unroll
    for (int p = 0; p < BS_WPB; ++p) {
      const double x = group_sum_t<64>(s[p]);
      const double vl = l0 - x, vh = x - h0;
      const bool ok = p < npb;
      wlo[p].push(vl, plan.row0 + row, ok);
      whi[p].push(vh, plan.row0 + row, ok);
      cnt[p] += (ok && (vl > tol || vh > tol)) ? 1 : 0;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int p = 0; p < BS_WPB; ++p) {
      double *s = red + (wave * BS_WPB + p) * BS_SLOT;
      s[0] = wlo[p].v; s[1] = (double)wlo[p].row; s[2] = whi[p].v; s[3] = (double)whi[p].row; s[4] = (double)cnt[p];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < npb) {
    Worst a, b;
    a.init(); b.init();
    double n = 0.0;
    for (int w = 0; w < NW; ++w) {
      const double *s = red + (w * BS_WPB + threadIdx.x) * BS_SLOT;
      a.merge(s[0], (int64_t)s[1]);
      b.merge(s[2], (int64_t)s[3]);
      n += s[4];
    }
    double *o = slots + ((int64_t)(np0 + threadIdx.x) * nslots + blockIdx.x) * BS_SLOT;
    o[0] = a.v; o[1] = (double)a.row; o[2] = b.v; o[3] = (double)b.row; o[4] = n;
  }
}

// ---- batched sweep for ROM.CPOD (openmeasure_amd/_cpod.py): all m snapshots are swept every round ----------------------
// The kernel above keeps BS_PB = 16 vectors per read of the basis; a batch of hundreds of vectors would re-read it once
// per 16.  This one keeps BB_PB = 64 per read.  Roles of the operands as above, but the PANEL fragment is what waits in
// registers (a wave's 16 rows x r columns: 2 r / 4 VGPRs) and the vectors come from an LDS slab, 16 at a time: the
// registers a 64-vector A operand would need (8 r) do not exist.  Because the panel fragment is taken out of LDS at
// once, one panel image suffices: the next panel's registers are stored as soon as every wave holds its fragment.
// Eight waves: wave w works on panel rows 16 (w & 3) ... and on the 16-vector groups g with (g & 1) == (w >> 2), so two
// waves per SIMD are resident although the LDS of r = 128 (panel + slab: 133 KB) admits one workgroup per CU.  Running
// state per lane: (max, row) per side and a count for 2 groups x 4 vectors, the row as a 32-bit offset into the
// workgroup's run of rows (56 VGPRs instead of 72).  Same slot layout and select kernel as above.
constexpr int BB_THREADS = 512;
constexpr int BB_PB = 64;        // coefficient vectors per pass
constexpr int BB_GPW = BB_PB / 16 / 2;   // 16-vector groups per wave

struct WorstL {                  // Worst with the row as an offset into the workgroup's run (visited in increasing order)
  double v;
  int off;
  __device__ inline void init() { v = -INFINITY; off = -1; }
  __device__ inline void push(double nv, int noff, bool valid) {
    const bool take = valid && nv > v;                 // strict: the lowest row keeps a tie
    v = take ? nv : v;
    off = take ? noff : off;
  }
  __device__ inline void merge_lanes16() {
    for (int o = 8; o > 0; o >>= 1) {
      const double ov = __shfl_xor(v, o, 64);
      const int oo = __shfl_xor(off, o, 64);
      const bool take = ov > v || (ov == v && oo >= 0 && (off < 0 || oo < off));
      v = take ? ov : v;
      off = take ? oo : off;
    }
  }
};

template <int MTR, int VEC, typename TU>
__global__ __launch_bounds__(BB_THREADS) void bound_sweep_batch_kernel(
    const TU *__restrict__ Ur, int r, int64_t ldu, SegPlan plan, const double *__restrict__ rowmean,
    const double *__restrict__ scale, const double *__restrict__ limits, const double *__restrict__ clamp,
    const double *__restrict__ G, int np0, int npb, double tol, double *__restrict__ slots, int nslots) {
  constexpr int NW = BB_THREADS / 64, R = 64;
  constexpr int MPAD = 16 * MTR, MP = MPAD + 2, KSTEPS = MPAD / 4;
  using RT = RowTile<MTR, R, MP, NW, 16, TU>;
  __shared__ double panel[R * MP];
  __shared__ double slab[BB_PB * MP];
  __shared__ double red[4 * BB_PB * BS_SLOT];
  int f, wl, wpf, base;
  int64_t lo, hi;
  if (!seg_locate(plan, blockIdx.x, f, wl, wpf, base, lo, hi)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wrow = wave & 3, half = wave >> 2;
  FeatLimits fl;
  fl.load(limits, clamp, scale, f, plan.n_features);

  for (int i = threadIdx.x; i < BB_PB * MPAD; i += BB_THREADS) {
    const int p = i / MPAD, k = i - p * MPAD;
    slab[p * MP + k] = (p < npb && k < r) ? G[(int64_t)(np0 + p) * r + k] : 0.0;
  }
  WorstL wlo[BB_GPW][4], whi[BB_GPW][4];     // vector 16 (2 s + half) + 4 q + (lane >> 4)
  int cnt[BB_GPW][4];
#pragma unroll
  for (int s = 0; s < BB_GPW; ++s)
#pragma unroll
    for (int q = 0; q < 4; ++q) { wlo[s][q].init(); whi[s][q].init(); cnt[s][q] = 0; }

  RT tile;
  const int64_t npanels = (hi - lo + R - 1) / R;
  int64_t c, cend;
  panel_run(npanels, wl, wpf, c, cend);
  const int64_t run0 = lo + c * R;                    // offsets are relative to this row (host: n_rows < 2^31)
  tile.template load<VEC>(Ur, ldu, r, run0, hi, wave, lane);
  const int frag = (lane & 15) * MP + (lane >> 4);    // operand element [k = lane >> 4][j = lane & 15] of a 16-row image
  while (c < cend) {
    const int64_t crow0 = lo + c * R;
    const int64_t nrow0 = (c + 1 < cend) ? lo + (c + 1) * R : hi;
    __syncthreads();             // every wave holds its fragment of the previous panel (first time: nothing to wait for)
    tile.raw_store(panel, r, crow0, hi, wave, lane);
    tile.template load<VEC>(Ur, ldu, r, nrow0, hi, wave, lane);
    __syncthreads();             // the panel (first time: and the slab) is complete
    const int64_t row = crow0 + wrow * 16 + (lane & 15);         // the panel row this lane's results belong to
    const int64_t rc = row < hi ? row : hi - 1;
    const double mu = rowmean[rc];
    double bfrag[KSTEPS];        // B[k][j] = panel[16 wrow + j][4 ks + k]
    {
      const double *p = panel + wrow * 16 * MP + frag;
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) bfrag[ks] = p[4 * ks];
    }
    const double l0 = fl.lo0(mu), h0 = fl.hi0(mu);
    const int off = (int)(row - run0);
    const bool rowok = row < hi;
#pragma unroll
    for (int s = 0; s < BB_GPW; ++s) {
      const int g = 2 * s + half;
      if (16 * g < npb) {        // wave-uniform
        const double *a = slab + g * 16 * MP + frag;             // A[i = lane & 15][k = lane >> 4] = vector 16 g + i
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[4 * ks], bfrag[ks], acc, 0, 0, 0);
        // D[i = (lane >> 4) + 4 q][j = lane & 15] = g_{np0 + 16 g + i} . u_row
        const double d[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool ok = rowok && (16 * g + 4 * q + (lane >> 4)) < npb;
          const double vl = l0 - d[q], vh = d[q] - h0;
          wlo[s][q].push(vl, off, ok);
          whi[s][q].push(vh, off, ok);
          cnt[s][q] += (ok && (vl > tol || vh > tol)) ? 1 : 0;
        }
      }
    }
    ++c;
  }
  // the 16 lanes of a group hold 16 rows of the same vectors; then the four row-waves of each half through LDS
#pragma unroll
  for (int s = 0; s < BB_GPW; ++s)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      wlo[s][q].merge_lanes16();
      whi[s][q].merge_lanes16();
      for (int o = 8; o > 0; o >>= 1) cnt[s][q] += __shfl_xor(cnt[s][q], o, 64);
    }
  if ((lane & 15) == 0) {
#pragma unroll
    for (int s = 0; s < BB_GPW; ++s)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int pv = 16 * (2 * s + half) + 4 * q + (lane >> 4);
        double *o = red + (wrow * BB_PB + pv) * BS_SLOT;
        o[0] = wlo[s][q].v; o[1] = (double)wlo[s][q].off; o[2] = whi[s][q].v; o[3] = (double)whi[s][q].off;
        o[4] = (double)cnt[s][q];
      }
  }
  __syncthreads();
  if ((int)threadIdx.x < npb) {
    Worst a, b;
    a.init(); b.init();
    double n = 0.0;
    const int64_t g0 = plan.row0 + run0;
    for (int w = 0; w < 4; ++w) {
      const double *s = red + (w * BB_PB + threadIdx.x) * BS_SLOT;
      a.merge(s[0], s[1] < 0.0 ? (int64_t)-1 : g0 + (int64_t)s[1]);
      b.merge(s[2], s[3] < 0.0 ? (int64_t)-1 : g0 + (int64_t)s[3]);
      n += s[4];
    }
    double *o = slots + ((int64_t)(np0 + threadIdx.x) * nslots + blockIdx.x) * BS_SLOT;
    o[0] = a.v; o[1] = (double)a.row; o[2] = b.v; o[3] = (double)b.row; o[4] = n;
  }
}

// Merge of the slots of one vector (one workgroup per vector): the entries (v, row, side) are totally ordered --
// larger v first, then the lower row, then the lower side -- and the k first with v > tol are written in that order, each
// found as the largest entry below the previous one (read-only on the slots: no marking, no sorting network).
// out[p] = { max violation, its row, count, k x (row, side, v) }; missing entries are (-1, 0, -inf).
struct Key {
  double v;
  int64_t row;
  int side;
  __device__ inline bool before(const Key &o) const {   // this comes earlier in the order than o
    if (row < 0 || o.row < 0) return o.row < 0 && row >= 0;
    return v > o.v || (v == o.v && (row < o.row || (row == o.row && side < o.side)));
  }
};

__global__ __launch_bounds__(BS_THREADS) void bound_select_kernel(const double *__restrict__ slots, int nslots, double tol,
                                                                  int k, double *__restrict__ out) {
  constexpr int NW = BS_THREADS / 64;
  __shared__ double sv[NW];
  __shared__ long long srow[NW];
  __shared__ int sside[NW];
  __shared__ double scnt[NW];
  const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double *sl = slots + (int64_t)p * nslots * BS_SLOT;
  double *o = out + (int64_t)p * (3 + 3 * k);
  double n = 0.0;
  for (int b = threadIdx.x; b < nslots; b += BS_THREADS) n += sl[(int64_t)b * BS_SLOT + 4];
  n = group_sum_t<64>(n);
  if (lane == 0) scnt[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < NW; ++w) t += scnt[w];      // integers below 2^53: exact in any order
    o[2] = t;
  }
  Key prev;
  prev.v = INFINITY; prev.row = -2; prev.side = -1;  // row -2: "no previous entry", see below
  bool open = true;
  for (int it = 0; it < k || it == 0; ++it) {
    Key best;
    best.v = -INFINITY; best.row = -1; best.side = 0;
    if (open) {
      for (int e = threadIdx.x; e < 2 * nslots; e += BS_THREADS) {
        Key c;
        c.side = e & 1;
        c.v = sl[(int64_t)(e >> 1) * BS_SLOT + 2 * c.side];
        c.row = (int64_t)sl[(int64_t)(e >> 1) * BS_SLOT + 2 * c.side + 1];
        const bool below = prev.row == -2 || prev.before(c);
        if (c.row >= 0 && below && c.before(best)) best = c;
      }
    }
    for (int of = 32; of > 0; of >>= 1) {
      Key c;
      c.v = __shfl_xor(best.v, of, 64);
      c.row = (int64_t)__shfl_xor((long long)best.row, of, 64);
      c.side = __shfl_xor(best.side, of, 64);
      if (c.before(best)) best = c;
    }
    __syncthreads();                                 // the previous round's reads of sv / srow / sside are over
    if (lane == 0) { sv[wave] = best.v; srow[wave] = best.row; sside[wave] = best.side; }
    __syncthreads();
    for (int w = 0; w < NW; ++w) {
      Key c;
      c.v = sv[w]; c.row = srow[w]; c.side = sside[w];
      if (c.before(best)) best = c;
    }
    if (it == 0 && threadIdx.x == 0) { o[0] = best.v; o[1] = (double)best.row; }
    if (best.row < 0 || !(best.v > tol)) open = false;          // uniform over the workgroup
    if (it < k && threadIdx.x == 0) {
      o[3 + 3 * it] = open ? (double)best.row : -1.0;
      o[3 + 3 * it + 1] = open ? (double)best.side : 0.0;
      o[3 + 3 * it + 2] = open ? best.v : -INFINITY;
    }
    prev = best;
  }
}

// workgroups the sweep may launch for a block with n_features features (seg_wgs: at least one per feature present)
inline int64_t bs_max_slots(int32_t n_features) {
  return 6 * (int64_t)spr_cus_or_default() + n_features;
}

template <int MTR, typename TU>
int launch_sweep_mfma(const TU *Ur, int32_t r, int64_t ldu, SegPlan plan, const double *rowmean, const double *scale,
                      const double *limits, const double *clamp, const double *G, int32_t n_p, double tol, double *slots,
                      int &nslots, int64_t max_slots, hipStream_t st) {
  const int grid = spr_plan_grid(plan, spr_panel_per_cu(MTR), 64);
  SPR_REQUIRE_GRID("spr_bound_sweep", grid, max_slots);
  nslots = grid;
  const int lm = spr_load_mode(spr_pair_aligned(Ur, r, ldu), r, MTR);
  for (int p0 = 0; p0 < n_p; p0 += BS_PB) {
    const int npb = (n_p - p0 < BS_PB) ? n_p - p0 : BS_PB;
#define BS(LM) hipLaunchKernelGGL((bound_sweep_mfma_kernel<MTR, LM, TU>), dim3(grid), dim3(BS_THREADS), 0, st, Ur, (int)r, ldu, plan, rowmean, scale, limits, clamp, G, p0, npb, tol, slots, grid)
    if (lm == 2) BS(2);
    else if (lm == 1) BS(1);
    else BS(0);
#undef BS
    SPR_LAUNCH_CHECK();
  }
  return SPR_OK;
}

template <typename TU>
int launch_sweep_wide(const TU *Ur, int32_t r, int64_t ldu, SegPlan plan, const double *rowmean, const double *scale,
                      const double *limits, const double *clamp, const double *G, int32_t n_p, double tol, double *slots,
                      int &nslots, int64_t max_slots, hipStream_t st) {
  const int grid = spr_plan_grid(plan, 4, 64);
  SPR_REQUIRE_GRID("spr_bound_sweep", grid, max_slots);
  nslots = grid;
  for (int p0 = 0; p0 < n_p; p0 += BS_WPB) {
    const int npb = (n_p - p0 < BS_WPB) ? n_p - p0 : BS_WPB;
    hipLaunchKernelGGL((bound_sweep_wide_kernel<TU>), dim3(grid), dim3(BS_THREADS), 0, st, Ur, (int)r, ldu, plan, rowmean,
                       scale, limits, clamp, G, p0, npb, tol, slots, grid);
    SPR_LAUNCH_CHECK();
  }
  return SPR_OK;
}

// 8-wave workgroups: two per CU need 4 waves per SIMD, i.e. <= 128 VGPRs: r <= 32 (118 / 126 VGPRs); from r = 33 on (MTR >= 3,
// 130 ... 202 VGPRs, 3 or 2 waves per SIMD) one workgroup per CU
inline int bb_per_cu(int mt) { return mt <= 2 ? 2 : 1; }

template <int MTR, typename TU>
int launch_sweep_batch(const TU *Ur, int32_t r, int64_t ldu, SegPlan plan, const double *rowmean, const double *scale,
                       const double *limits, const double *clamp, const double *G, int32_t n_p, double tol, double *slots,
                       int &nslots, int64_t max_slots, hipStream_t st) {
  const int grid = spr_plan_grid(plan, bb_per_cu(MTR), 64);
  SPR_REQUIRE_GRID("spr_bound_sweep_batch", grid, max_slots);
  nslots = grid;
  const int lm = spr_load_mode(spr_pair_aligned(Ur, r, ldu), r, MTR);
  for (int p0 = 0; p0 < n_p; p0 += BB_PB) {
    const int npb = (n_p - p0 < BB_PB) ? n_p - p0 : BB_PB;
#define BB(LM) hipLaunchKernelGGL((bound_sweep_batch_kernel<MTR, LM, TU>), dim3(grid), dim3(BB_THREADS), 0, st, Ur, (int)r, ldu, plan, rowmean, scale, limits, clamp, G, p0, npb, tol, slots, grid)
    if (lm == 2) BB(2);
    else if (lm == 1) BB(1);
    else BB(0);
#undef BB
    SPR_LAUNCH_CHECK();
  }
  return SPR_OK;
}

template <typename TU>
int bound_sweep(const char *name, const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_limits,
                const double *d_clamp, const double *d_G, int32_t n_p, double tol, int32_t k, double *d_out,
                void *d_workspace, size_t workspace_bytes, void *stream, bool batch = false) {
  SPR_REQUIRE(d_Ur && d_rowmean && d_scale && d_limits && d_clamp && d_G && d_out && d_workspace, SPR_E_INVALID,
              "%s: NULL pointer", name);
  SPR_REQUIRE(n_rows > 0 && r > 0 && ldu >= r && n_p > 0 && k > 0 && k <= BS_MAX_K, SPR_E_INVALID,
              "%s: bad shape n_rows=%lld r=%d ldu=%lld n_p=%d k=%d (k <= %d)", name, (long long)n_rows, r, (long long)ldu,
              n_p, k, BS_MAX_K);
  SPR_REQUIRE_LAYOUT(name, row0, n_rows, n_points, n_features);
  SPR_REQUIRE(tol >= 0.0, SPR_E_INVALID, "%s: tol = %g must not be negative", name, tol);
  SPR_REQUIRE(r <= SPR_MAX_R_WIDE, SPR_E_UNSUPPORTED, "%s: r = %d exceeds %d", name, r, SPR_MAX_R_WIDE);
  SPR_REQUIRE(workspace_bytes >= spr_bound_sweep_workspace(n_p, n_features), SPR_E_INVALID,
              "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes, spr_bound_sweep_workspace(n_p, n_features));
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *slots = static_cast<double *>(d_workspace);
  SegPlan plan = spr_make_plan(row0, n_rows, n_points, n_features, 64);
  const int64_t max_slots = bs_max_slots(n_features);
  int nslots = 0, rc = SPR_OK;
  if (r > SPR_MAX_R) {
    rc = launch_sweep_wide<TU>(d_Ur, r, ldu, plan, d_rowmean, d_scale, d_limits, d_clamp, d_G, n_p, tol, slots, nslots, max_slots, st);
  } else {
    // padded width in 16-column tiles; r <= SPR_MAX_R: one of 1, 2, 3, 4, 6, 8
#define SWEEP_MT(LAUNCH)                                                                                                       \
  SPR_DISPATCH_MT(spr_round_mt(r), name, r,                                                                                    \
                  rc = LAUNCH<RUNG, TU>(d_Ur, r, ldu, plan, d_rowmean, d_scale, d_limits, d_clamp, d_G, n_p, tol, slots,       \
                                        nslots, max_slots, st))
    // batch: BB_PB vectors per read of the basis; its row offsets are 32-bit, larger blocks take the 16-vector kernel
    if (batch && n_rows < INT32_MAX) {
      SWEEP_MT(launch_sweep_batch)
    } else {
      SWEEP_MT(launch_sweep_mfma)
    }
#undef SWEEP_MT
  }
  if (rc != SPR_OK) return rc;
  hipLaunchKernelGGL(bound_select_kernel, dim3(n_p), dim3(BS_THREADS), 0, st, slots, nslots, tol, (int)k, d_out);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

}  // namespace

extern "C" size_t spr_bound_sweep_workspace(int32_t n_p, int32_t n_features) {
  if (n_p <= 0 || n_features <= 0) return 0;
  return (size_t)n_p * (size_t)bs_max_slots(n_features) * BS_SLOT * sizeof(double);
}

// TU = float: basis stored as f32, arithmetic f64
#define SPR_BOUND_SWEEP_ENTRY(NAME, TU, BATCH)                                                                                \
  SPR_ENTRY(NAME,                                                                                                             \
            (const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points, int32_t n_features,      \
             const double *d_rowmean, const double *d_scale, const double *d_limits, const double *d_clamp,                   \
             const double *d_G, int32_t n_p, double tol, int32_t k, double *d_out, void *d_workspace,                         \
             size_t workspace_bytes, void *stream),                                                                           \
            (bound_sweep<TU>), d_Ur, n_rows, r, ldu, row0, n_points, n_features, d_rowmean, d_scale, d_limits, d_clamp, d_G,  \
            n_p, tol, k, d_out, d_workspace, workspace_bytes, stream, BATCH)
SPR_BOUND_SWEEP_ENTRY(spr_bound_sweep_f64, double, false)
SPR_BOUND_SWEEP_ENTRY(spr_bound_sweep_u32, float, false)

// ---- batched form (ROM.CPOD): same arguments, same records; 64 vectors per read of the basis where r <= SPR_MAX_R
extern "C" size_t spr_bound_sweep_batch_workspace(int32_t n_p, int32_t n_features) {
  return spr_bound_sweep_workspace(n_p, n_features);
}

SPR_BOUND_SWEEP_ENTRY(spr_bound_sweep_batch_f64, double, true)
SPR_BOUND_SWEEP_ENTRY(spr_bound_sweep_batch_u32, float, true)
#undef SPR_BOUND_SWEEP_ENTRY
