// POD from incomplete snapshots (ROM.fit_gappy): the two passes that write into the holes of the snapshot block in place.
//
// mask (n x m, one byte per entry, non-zero = observed) marks the entries of X that were measured; the others are holes.
//  * spr_gappy_rowfill_*: every hole gets the mean of the observed entries of its row (the start of the iteration), and the
//    block is validated: rows without an observed entry, observed entries that are not finite.
//  * spr_gappy_fill_*:    every hole gets the rank-r reconstruction  scale[f(i)] (Ur[i] . A[j]) + rowmean[i]  and the pass
//    returns  S_d = sum over holes (new - old)^2,  S_n = sum over holes new^2  (the caller's stopping test).
// An observed entry is never written and never enters a sum.  No atomics: per-workgroup slots in the workspace and a
// second kernel that combines them in increasing order; the deal of the rows to the waves is static, so two runs on one
// device agree bit for bit.
//
// The fill kernel.  Holes are sparse (a few per cent), so the dot products run PER HOLE on the vector pipe: forming the
// whole 64 x m tile of a panel on the f64 MFMA and selecting the holes afterwards would issue 1 / (hole fraction) times the
// flops (2 n m r = 2.9 TFLOP at 90M rows, m = 256, r = 64: 70 ms at the 40 TFLOP/s the other passes reach), while the holes
// alone are 0.15 TFLOP at 5 %.
//  * A (m x r, f64) is staged in LDS in slices of  min(256, 8192 / r)  columns (64 KB: 64 columns at r = 128, 128 at r = 64,
//    all 256 at r <= 32), slices outermost: a slice is staged once per workgroup, then the workgroup's panels stream past
//    it.  Every mask byte is read exactly once (the slices partition the columns); the basis row of a row with a hole is
//    read once per slice in which it has one.
//  * The eight waves of a workgroup work independently (no barrier inside a slice); wave w of workgroup b takes the 64-row
//    panels 8 b + w, + 8 gridDim, ...  Of a panel it first reads the mask bytes of the slice's columns, one byte per lane
//    and row, a ballot makes them a 64-bit word per row (kept by lane = row).  A panel without a hole is left BEFORE any
//    of its basis or X rows is requested.
//  * Rows with holes are visited in order, the next one's basis row (16 lanes x E values, the same in all four 16-lane
//    groups), centre, scale and OLD values (a masked load: only the holes' addresses are requested) are in flight while
//    the current one is worked on.  Four holes per step, one per 16-lane group: r products against the LDS row of A,
//    a DPP butterfly over the 16 lanes, one store.
// Measured: 109 ms at 90M rows x 256, r = 64, 5 % holes -- bound by the latency of the per-row loads (1.6 steps
// per row and slice, one row of prefetch), 5 x the time of its traffic model.
#include <stdlib.h>

#include "common.hpp"
#include "launch.hpp"

namespace {

constexpr int GF_THREADS = 512;
constexpr int GF_WAVES = GF_THREADS / 64;
constexpr int GF_R = 64;              // rows of a panel: one per lane
constexpr int GF_LDS_DOUBLES = 8192;  // the slice of A: 64 KB, two workgroups (16 waves) per CU
constexpr int GF_MAXQ = 4;            // 64-column words of a slice: at most 256 columns
constexpr int GF_PANELS_PER_WG = 32;  // panels a workgroup should have before another one is started (amortises the staging)
constexpr int GF_BATCH = 16;          // mask bytes in flight per lane
constexpr int RF_THREADS = 256;
constexpr int RF_SLOT = 8;            // doubles per slot of the row fill (5 used)

inline int gf_slice(int r) {
  const int s = GF_LDS_DOUBLES / r;
  return s > 64 * GF_MAXQ ? 64 * GF_MAXQ : s;
}
inline int gf_max_grid() { return 2 * spr_cus_or_default(); }
inline int rf_max_grid() { return 8 * spr_cus_or_default(); }
inline size_t gf_workspace() {
  const size_t a = (size_t)gf_max_grid() * 2, b = (size_t)rf_max_grid() * RF_SLOT;
  return (a > b ? a : b) * sizeof(double);
}

__device__ inline uint64_t readlane64(uint64_t v, int l) {   // l wave-uniform
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, l), hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

template <int E>
struct RowRegs {
  double u[E];            // basis row: element t + 16 e of lane t of every 16-lane group
  double old[GF_MAXQ];    // X[row][j0 + 64 q + lane] where that entry is a hole
  uint64_t h[GF_MAXQ];    // hole words of the row (wave-uniform)
  double mu, sc;
};

template <int E, typename TU, typename TX>
__global__ __launch_bounds__(GF_THREADS) void gappy_fill_kernel(const TU *__restrict__ Ur, int r, int64_t ldu,
                                                                TX *__restrict__ X, int m, int64_t ldx, int64_t n_rows,
                                                                int64_t row0, int64_t n_points, int n_features,
                                                                const double *__restrict__ rowmean,
                                                                const double *__restrict__ scale,
                                                                const double *__restrict__ A,
                                                                const uint8_t *__restrict__ mask, int64_t ldm, int sl,
                                                                double *__restrict__ part) {
  __shared__ double As[GF_LDS_DOUBLES];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, t = lane & 15;
  const int64_t npanels = (n_rows + GF_R - 1) / GF_R;
  const int64_t tw = (int64_t)gridDim.x * GF_WAVES, gw = (int64_t)blockIdx.x * GF_WAVES + wave;
  double sd = 0.0, sn = 0.0;

  for (int j0 = 0; j0 < m; j0 += sl) {
    const int w = (m - j0 < sl) ? m - j0 : sl;
    const int nq = (w + 63) / 64;
    __syncthreads();               // every wave is done with the previous slice
    for (int idx = threadIdx.x; idx < w * r; idx += GF_THREADS) As[idx] = A[(int64_t)j0 * r + idx];
    __syncthreads();
    for (int64_t p = gw; p < npanels; p += tw) {
      const int64_t base = p * GF_R;
      const int rows = (n_rows - base < GF_R) ? (int)(n_rows - base) : GF_R;
      // ---- the mask bytes of the panel: lane = column inside a 64-column word; the word of row i ends up in lane i
      uint64_t hw[GF_MAXQ] = {0, 0, 0, 0};
#pragma unroll
      for (int q = 0; q < GF_MAXQ; ++q) {
        if (q < nq) {
          const int cl = 64 * q + lane;
          const bool cok = cl < w;
          const uint8_t *mp = mask + j0 + (cok ? cl : 0);
          for (int i0 = 0; i0 < GF_R; i0 += GF_BATCH) {
            uint8_t b[GF_BATCH];
#pragma unroll
            for (int u = 0; u < GF_BATCH; ++u) {
              const int i = i0 + u;
              const bool ok = cok && i < rows;
              const uint8_t v = mp[(base + (i < rows ? i : 0)) * ldm];
              b[u] = ok ? v : (uint8_t)1;       // past the slice or the block: not a hole
            }
#pragma unroll
            for (int u = 0; u < GF_BATCH; ++u) {
              const uint64_t hole = __ballot(b[u] == 0);
              if (lane == i0 + u) hw[q] = hole;
            }
          }
        }
      }
      uint64_t todo = __ballot((hw[0] | hw[1] | hw[2] | hw[3]) != 0);
      if (todo == 0) continue;     // no hole in this panel and slice: nothing of its basis or X rows is requested

      auto load = [&](RowRegs<E> &rr, int i) {
        const int64_t row = base + i;
#pragma unroll
        for (int q = 0; q < GF_MAXQ; ++q) rr.h[q] = readlane64(hw[q], i);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int c = t + 16 * e;
          rr.u[e] = c < r ? (double)Ur[row * ldu + c] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < GF_MAXQ; ++q)
          rr.old[q] = ((rr.h[q] >> lane) & 1) ? (double)X[row * ldx + j0 + 64 * q + lane] : 0.0;
        int64_t f = (row0 + row) / n_points;
        if (f > n_features - 1) f = n_features - 1;
        rr.mu = rowmean[row];
        rr.sc = scale[f];
      };

      int i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
      todo &= todo - 1;
      RowRegs<E> nx;
      load(nx, i);
      while (true) {
        const RowRegs<E> cur = nx;
        const int64_t row = base + i;
        const bool more = todo != 0;
        if (more) {
          i = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
          todo &= todo - 1;
          load(nx, i);
        }
#pragma unroll
        for (int q = 0; q < GF_MAXQ; ++q) {
          uint64_t hq = cur.h[q];
          while (hq != 0) {          // wave-uniform: four holes per step, one per 16-lane group
            int jb = 0;
            bool valid = false;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const bool v = hq != 0;
              const int bit = v ? __builtin_ctzll(hq) : 0;
              if (v) hq &= hq - 1;
              if (g == s) {
                jb = bit;
                valid = v;
              }
            }
            const int jl = 64 * q + jb;
            const double *a = As + jl * r + t;
            double dot = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const double av = (t + 16 * e < r) ? a[16 * e] : 0.0;
              dot = fma(cur.u[e], av, dot);
            }
            dot = group_sum_t<16>(dot);
            const double o = __shfl(cur.old[q], jb, 64);
            if (valid && t == 0) {
              const TX stored = (TX)(cur.sc * dot + cur.mu);   // rounded once for an f32 block
              X[row * ldx + j0 + jl] = stored;
              const double vs = (double)stored, d = vs - o;
              sd += d * d;
              sn += vs * vs;
            }
          }
        }
        if (!more) break;
      }
    }
  }
  sd = group_sum_t<64>(sd);
  sn = group_sum_t<64>(sn);
  __syncthreads();                 // the last slice of A is no longer needed: its first doubles carry the waves' sums
  double *const wsum = As;
  if (lane == 0) {
    wsum[2 * wave] = sd;
    wsum[2 * wave + 1] = sn;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = 0.0;
    for (int k = 0; k < GF_WAVES; ++k) s += wsum[2 * k + threadIdx.x];
    part[2 * (int64_t)blockIdx.x + threadIdx.x] = s;
  }
}

__global__ void gappy_fill_reduce_kernel(const double *__restrict__ part, int nslots, double *__restrict__ out) {
  if (threadIdx.x < 2) {
    double s = 0.0;
    for (int b = 0; b < nslots; ++b) s += part[2 * (int64_t)b + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// ---- row fill: lpr (a power of two <= 64) lanes per row, 64 / lpr rows per wave and step.  FILL = false: count and validate
// only (slots: holes, rows without an observed entry, the lowest such global row, non-finite observed entries, the lowest
// global row holding one); FILL = true: write the row means -- unless the verdict of the first sweep names a bad row.
__device__ inline int group_sum_int(int v, int width) {
  for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double wave_min(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}

template <bool FILL, typename TX>
__global__ __launch_bounds__(RF_THREADS) void gappy_rowfill_kernel(TX *__restrict__ X, int64_t n_rows, int m, int64_t ldx,
                                                                   int64_t row0, const uint8_t *__restrict__ mask,
                                                                   int64_t ldm, int lpr, const double *__restrict__ verdict,
                                                                   double *__restrict__ part) {
  constexpr int NW = RF_THREADS / 64;
  __shared__ double wrec[NW * 5];
  if (FILL && (verdict[1] != 0.0 || verdict[3] != 0.0)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rpw = 64 / lpr, g = lane / lpr, t = lane % lpr;
  const int64_t step = (int64_t)gridDim.x * NW * rpw;
  double holes = 0.0, nempty = 0.0, nbad = 0.0, rempty = INFINITY, rbad = INFINITY;
  for (int64_t rb = ((int64_t)blockIdx.x * NW + wave) * rpw; rb < n_rows; rb += step) {
    const int64_t row = rb + g;
    const bool ok = row < n_rows;
    const int64_t rr = ok ? row : n_rows - 1;
    double s = 0.0;
    int cnt = 0, bad = 0;
    for (int col = t; col < m; col += lpr) {
      if (mask[rr * ldm + col]) {
        const double x = (double)X[rr * ldx + col];
        ++cnt;
        if (!isfinite(x)) ++bad;
        s += x;
      }
    }
    s = group_sum(s, lpr);
    cnt = group_sum_int(cnt, lpr);
    bad = group_sum_int(bad, lpr);
    if (!FILL) {
      if (ok && t == 0) {
        holes += (double)(m - cnt);
        if (cnt == 0) {
          nempty += 1.0;
          rempty = fmin(rempty, (double)(row0 + row));
        }
        if (bad != 0) {
          nbad += (double)bad;
          rbad = fmin(rbad, (double)(row0 + row));
        }
      }
    } else if (ok && cnt > 0 && cnt < m && bad == 0) {
      const TX mean = (TX)(s / (double)cnt);
      for (int col = t; col < m; col += lpr)
        if (!mask[rr * ldm + col]) X[rr * ldx + col] = mean;
    }
  }
  if (FILL) return;
  holes = group_sum(holes, 64);
  nempty = group_sum(nempty, 64);
  nbad = group_sum(nbad, 64);
  rempty = wave_min(rempty);
  rbad = wave_min(rbad);
  if (lane == 0) {
    double *o = wrec + 5 * wave;
    o[0] = holes; o[1] = nempty; o[2] = rempty; o[3] = nbad; o[4] = rbad;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const bool is_min = threadIdx.x == 2 || threadIdx.x == 4;
    double v = wrec[threadIdx.x];
    for (int k = 1; k < NW; ++k) v = is_min ? fmin(v, wrec[5 * k + threadIdx.x]) : v + wrec[5 * k + threadIdx.x];
    part[(int64_t)blockIdx.x * RF_SLOT + threadIdx.x] = v;
  }
}

__global__ void gappy_rowfill_reduce_kernel(const double *__restrict__ part, int nslots, double *__restrict__ out) {
  if (threadIdx.x < 8) {
    const int k = threadIdx.x;
    double v = 0.0;
    if (k < 5) {
      const bool is_min = k == 2 || k == 4;
      v = part[k];
      for (int b = 1; b < nslots; ++b) v = is_min ? fmin(v, part[(int64_t)b * RF_SLOT + k]) : v + part[(int64_t)b * RF_SLOT + k];
      if (is_min && !(v < INFINITY)) v = -1.0;
    }
    out[k] = v;
  }
}

template <typename TX>
int gappy_rowfill(const char *name, TX *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0, const uint8_t *d_mask,
                  int64_t ldm, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_X && d_mask && d_out && d_workspace, SPR_E_INVALID, "%s: NULL pointer", name);
  SPR_REQUIRE(n_rows > 0 && m > 0 && ldx >= m && ldm >= m && row0 >= 0, SPR_E_INVALID,
              "%s: bad shape n_rows=%lld m=%d ldx=%lld ldm=%lld row0=%lld", name, (long long)n_rows, m, (long long)ldx,
              (long long)ldm, (long long)row0);
  SPR_REQUIRE(workspace_bytes >= gf_workspace(), SPR_E_INVALID, "%s: workspace of %zu bytes, %zu needed", name,
              workspace_bytes, gf_workspace());
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *part = static_cast<double *>(d_workspace);
  int lpr = 1;
  while (lpr < 64 && lpr < m) lpr *= 2;
  const int64_t per_wg = (int64_t)(RF_THREADS / 64) * (64 / lpr);
  int64_t want = (n_rows + per_wg - 1) / per_wg;
  const int grid = (int)(want < rf_max_grid() ? want : rf_max_grid());
  hipLaunchKernelGGL((gappy_rowfill_kernel<false, TX>), dim3(grid), dim3(RF_THREADS), 0, st, d_X, n_rows, (int)m, ldx, row0,
                     d_mask, ldm, lpr, (const double *)d_out, part);
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gappy_rowfill_reduce_kernel, dim3(1), dim3(64), 0, st, (const double *)part, grid, d_out);
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL((gappy_rowfill_kernel<true, TX>), dim3(grid), dim3(RF_THREADS), 0, st, d_X, n_rows, (int)m, ldx, row0,
                     d_mask, ldm, lpr, (const double *)d_out, part);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

template <typename TU, typename TX>
int gappy_fill(const char *name, const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, TX *d_X, int32_t m, int64_t ldx,
               int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale,
               const double *d_A, const uint8_t *d_mask, int64_t ldm, double *d_out, void *d_workspace,
               size_t workspace_bytes, void *stream) {
  SPR_REQUIRE(d_Ur && d_X && d_rowmean && d_scale && d_A && d_mask && d_out && d_workspace, SPR_E_INVALID,
              "%s: NULL pointer", name);
  SPR_REQUIRE(n_rows > 0 && r > 0 && ldu >= r && m > 0 && ldx >= m && ldm >= m, SPR_E_INVALID,
              "%s: bad shape n_rows=%lld r=%d ldu=%lld m=%d ldx=%lld ldm=%lld", name, (long long)n_rows, r, (long long)ldu, m,
              (long long)ldx, (long long)ldm);
  SPR_REQUIRE_LAYOUT(name, row0, n_rows, n_points, n_features);
  SPR_REQUIRE(r <= SPR_MAX_R, SPR_E_UNSUPPORTED, "%s: r = %d exceeds the %d modes the fill pass is built for", name, r,
              SPR_MAX_R);
  SPR_REQUIRE(workspace_bytes >= gf_workspace(), SPR_E_INVALID, "%s: workspace of %zu bytes, %zu needed", name,
              workspace_bytes, gf_workspace());
  hipStream_t st = static_cast<hipStream_t>(stream);
  double *part = static_cast<double *>(d_workspace);
  const int64_t npanels = (n_rows + GF_R - 1) / GF_R;
  const int64_t want = (npanels + GF_PANELS_PER_WG - 1) / GF_PANELS_PER_WG;
  const int grid = (int)(want < gf_max_grid() ? want : gf_max_grid());
  const int sl = gf_slice(r);
#define GF(EV)                                                                                                                \
  hipLaunchKernelGGL((gappy_fill_kernel<EV, TU, TX>), dim3(grid), dim3(GF_THREADS), 0, st, d_Ur, (int)r, ldu, d_X, (int)m, ldx, \
                     n_rows, row0, n_points, (int)n_features, d_rowmean, d_scale, d_A, d_mask, ldm, sl, part)
  if (r <= 16) GF(1);
  else if (r <= 32) GF(2);
  else if (r <= 64) GF(4);
  else GF(8);
#undef GF
  SPR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gappy_fill_reduce_kernel, dim3(1), dim3(64), 0, st, (const double *)part, grid, d_out);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

}  // namespace

extern "C" size_t spr_gappy_fill_workspace(void) { return gf_workspace(); }

#define SPR_ROWFILL_ENTRY(NAME, TX)                                                                                           \
  extern "C" int NAME(TX *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0, const uint8_t *d_mask, int64_t ldm,      \
                      double *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {                               \
    return gappy_rowfill<TX>(#NAME, d_X, n_rows, m, ldx, row0, d_mask, ldm, d_out, d_workspace, workspace_bytes, stream);     \
  }
SPR_ROWFILL_ENTRY(spr_gappy_rowfill_f64, double)
SPR_ROWFILL_ENTRY(spr_gappy_rowfill_x32, float)
#undef SPR_ROWFILL_ENTRY

#define SPR_FILL_ENTRY(NAME, TU, TX)                                                                                          \
  extern "C" int NAME(const TU *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, TX *d_X, int32_t m, int64_t ldx, int64_t row0,  \
                      int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale,                   \
                      const double *d_A, const uint8_t *d_mask, int64_t ldm, double *d_out, void *d_workspace,                \
                      size_t workspace_bytes, void *stream) {                                                                 \
    return gappy_fill<TU, TX>(#NAME, d_Ur, n_rows, r, ldu, d_X, m, ldx, row0, n_points, n_features, d_rowmean, d_scale, d_A,  \
                              d_mask, ldm, d_out, d_workspace, workspace_bytes, stream);                                      \
  }
SPR_FILL_ENTRY(spr_gappy_fill_f64, double, double)
SPR_FILL_ENTRY(spr_gappy_fill_x32, double, float)          // X stored as f32
SPR_FILL_ENTRY(spr_gappy_fill_u32, float, double)          // basis stored as f32
SPR_FILL_ENTRY(spr_gappy_fill_x32_u32, float, float)
#undef SPR_FILL_ENTRY
