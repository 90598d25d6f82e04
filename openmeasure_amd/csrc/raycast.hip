// Camera projection matrix C (p = C f, docs/ctc_doc.ipynb) built on the device: line segments in, CSR out.
//
// Replaces the reference's Python loop with one pyvista line query per pixel and per random ray (utils.py:318-469) by a
// ray caster through a voxel grid.  The grid is nx x ny x nz axis-aligned cells, cell id = i + nx (j + ny k): uniform, with
// origin (ox, oy, oz) and spacing (hx, hy, hz), or rectilinear, with nx + 1 / ny + 1 / nz + 1 ascending edge coordinates
// per axis on the device (the *_rect entry points; the same traversal over another plane and start-cell accessor).
// A segment is p(t) = a + t (b - a), t in [0, 1], six doubles; pixel p owns the n_ray consecutive segments from p n_ray.
// A cell belongs to a segment iff the part of the segment inside the cell has positive length IN THIS ARITHMETIC (a touch
// at a point, an edge or a face is no hit); the chord length (t_exit - t_enter) |b - a| is kept with every hit.
//
// Four kernels; the two prefix sums between them are the caller's (torch.cumsum):
//   count    one thread per segment: slab clip to the grid, 3-D DDA (Amanatides-Woo), number of cells
//   fill     the same traversal, writing (cell, chord) from the segment's offset
//   merge    one workgroup per pixel: sort the pixel's entries by cell, add the chords of equal cells, unique entries
//            to the front of the pixel's range of the OUTPUT pair of buffers, their number to d_uniq
//   compact  fronts -> final indices (+ col0) and vals (1, or the summed chord / n_ray)
// No atomics, no communication between workgroups, no spin waits: two runs agree bit for bit.  The traversal is a for
// loop of at most nx + ny + nz + 2 steps whatever the data (NaN included), every cell index is clamped into the grid
// before it is used, and fill never writes past the segment's counted range.  Every barrier of the merge kernel sits
// in a loop whose bounds are the same for the whole workgroup.
#include <math.h>

#include "common.hpp"
#include "launch.hpp"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_LDS_ENTRIES = 2048;   // entries of one pixel sorted in LDS: 2048 x (4 + 8) bytes = 24 KB

// plane k of an axis; ONE expression for the slab clip and for the traversal, so the last plane of the traversal is the
// face the clip used
__device__ inline double rc_plane(double o, double h, int k) { return fma((double)k, h, o); }

__device__ inline int rc_start(double p, double o, double h, int n) {
  double f = floor((p - o) / h);
  f = fmin(fmax(f, 0.0), (double)(n - 1));   // a NaN ends as 0
  return (int)f;
}

// One axis of a grid, as the traversal sees it: n cells, plane(k) for k in 0 .. n, lo() / hi() the two faces the slab
// clip uses, start(p) = the cell that holds p, clamped into 0 .. n - 1.  Uniform: the closed forms above.
struct RcAxisUniform {
  double o, h;
  int n;
  __device__ inline double plane(int k) const { return rc_plane(o, h, k); }
  __device__ inline double lo() const { return o; }
  __device__ inline double hi() const { return plane(n); }
  __device__ inline int start(double p) const { return rc_start(p, o, h, n); }
};

// Rectilinear: plane k is the LOADED e[k] (n + 1 doubles), for the clip and for the traversal alike, so the last plane
// of the traversal is bit for bit the face the clip used.  Nothing is assumed about the contents of e: every index is
// clamped before it addresses the array, and the bisection runs a trip count that depends on n alone.
struct RcAxisEdges {
  const double *__restrict__ e;
  int n;
  __device__ inline double plane(int k) const { return e[min(max(k, 0), n)]; }
  __device__ inline double lo() const { return plane(0); }
  __device__ inline double hi() const { return plane(n); }
  // the i with e[i] <= p < e[i + 1]: lo <= i < hi, halved ceil(log2 n) <= 31 times.  mid lies in 1 .. n - 1; p below e[0]
  // or a NaN (every comparison false) ends at 0, p at or above e[n] at n - 1
  __device__ inline int start(double p) const {
    int lo = 0, hi = n;
    const int trips = n > 1 ? 32 - __clz(n - 1) : 0;
    for (int t = 0; t < trips; ++t) {
      if (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (p >= e[mid]) lo = mid; else hi = mid;
      }
    }
    return min(max(lo, 0), n - 1);
  }
};

struct RcGrid {
  int nx, ny, nz;
  double ox, oy, oz, hx, hy, hz;
  __device__ inline RcAxisUniform x() const { return {ox, hx, nx}; }
  __device__ inline RcAxisUniform y() const { return {oy, hy, ny}; }
  __device__ inline RcAxisUniform z() const { return {oz, hz, nz}; }
};

struct RcGridEdges {
  int nx, ny, nz;
  const double *xe, *ye, *ze;
  __device__ inline RcAxisEdges x() const { return {xe, nx}; }
  __device__ inline RcAxisEdges y() const { return {ye, ny}; }
  __device__ inline RcAxisEdges z() const { return {ze, nz}; }
};

// clip [t0, t1] to lo < a + t d < hi.  d == 0 exactly: inside or outside for all t, no division and no 0 * inf
__device__ inline bool rc_slab(double a, double d, double lo, double hi, double &t0, double &t1) {
  if (d == 0.0) return a > lo && a < hi;
  const double ta = (lo - a) / d, tb = (hi - a) / d;
  t0 = fmax(t0, fmin(ta, tb));
  t1 = fmin(t1, fmax(ta, tb));
  return true;
}

// parameter at which the segment leaves cell index i of an axis: +inf for d == 0; a tiny non-zero d gives a huge finite
// value or +-inf, which never is the minimum below t1 (never steps)
template <typename AXIS>
__device__ inline double rc_tnext(double a, double d, const AXIS &ax, int i) {
  return d == 0.0 ? INFINITY : (ax.plane(i + (d > 0.0 ? 1 : 0)) - a) / d;
}

// -> number of cells; FILL: the first `cap` of them to cell[0..], chord[0..].  GRID: RcGrid or RcGridEdges
template <bool FILL, typename GRID>
__device__ inline int rc_traverse(const double *__restrict__ seg, const GRID &g, int64_t *__restrict__ cell,
                                  double *__restrict__ chord, int64_t cap) {
  const auto gx = g.x(), gy = g.y(), gz = g.z();
  const double ax = seg[0], ay = seg[1], az = seg[2];
  const double dx = seg[3] - ax, dy = seg[4] - ay, dz = seg[5] - az;
  const double len = sqrt(dx * dx + dy * dy + dz * dz);
  if (!(len > 0.0)) return 0;
  double t0 = 0.0, t1 = 1.0;
  if (!rc_slab(ax, dx, gx.lo(), gx.hi(), t0, t1)) return 0;
  if (!rc_slab(ay, dy, gy.lo(), gy.hi(), t0, t1)) return 0;
  if (!rc_slab(az, dz, gz.lo(), gz.hi(), t0, t1)) return 0;
  if (!(t0 < t1)) return 0;
  int ix = gx.start(ax + t0 * dx);
  int iy = gy.start(ay + t0 * dy);
  int iz = gz.start(az + t0 * dz);
  const int sx = dx > 0.0 ? 1 : -1, sy = dy > 0.0 ? 1 : -1, sz = dz > 0.0 ? 1 : -1;
  double tx = rc_tnext(ax, dx, gx, ix);
  double ty = rc_tnext(ay, dy, gy, iy);
  double tz = rc_tnext(az, dz, gz, iz);
  double tc = t0;
  int cnt = 0;
  const int max_steps = g.nx + g.ny + g.nz + 2;
  for (int it = 0; it < max_steps; ++it) {
    const double tn = fmin(fmin(tx, ty), fmin(tz, t1));
    if (tn > tc) {                                   // positive length inside this cell
      if (FILL && cnt < cap) {
        cell[cnt] = (int64_t)ix + (int64_t)g.nx * ((int64_t)iy + (int64_t)g.ny * iz);
        chord[cnt] = (tn - tc) * len;
      }
      ++cnt;
      tc = tn;
    }
    if (tn >= t1) break;
    if (tx <= ty && tx <= tz) {
      ix += sx;
      if (ix < 0 || ix >= g.nx) break;
      tx = rc_tnext(ax, dx, gx, ix);
    } else if (ty <= tz) {
      iy += sy;
      if (iy < 0 || iy >= g.ny) break;
      ty = rc_tnext(ay, dy, gy, iy);
    } else {
      iz += sz;
      if (iz < 0 || iz >= g.nz) break;
      tz = rc_tnext(az, dz, gz, iz);
    }
  }
  return cnt;
}

__global__ __launch_bounds__(RC_THREADS) void raycast_count_kernel(const double *__restrict__ seg, int64_t n_seg, RcGrid g,
                                                                   int64_t *__restrict__ count) {
  const int64_t s = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (s >= n_seg) return;
  count[s] = rc_traverse<false>(seg + 6 * s, g, nullptr, nullptr, 0);
}

__global__ __launch_bounds__(RC_THREADS) void raycast_fill_kernel(const double *__restrict__ seg, int64_t n_seg, RcGrid g,
                                                                  const int64_t *__restrict__ offset,
                                                                  int64_t *__restrict__ cell, double *__restrict__ chord) {
  const int64_t s = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (s >= n_seg) return;
  const int64_t e0 = offset[s], cap = offset[s + 1] - e0;
  if (e0 < 0 || cap <= 0) return;
  rc_traverse<true>(seg + 6 * s, g, cell + e0, chord + e0, cap);
}

// the same two kernels over a rectilinear grid: the edge arrays are a few KB that every thread reads, plain loads
// through the cache
__global__ __launch_bounds__(RC_THREADS) void raycast_count_rect_kernel(const double *__restrict__ seg, int64_t n_seg,
                                                                        RcGridEdges g, int64_t *__restrict__ count) {
  const int64_t s = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (s >= n_seg) return;
  count[s] = rc_traverse<false>(seg + 6 * s, g, nullptr, nullptr, 0);
}

__global__ __launch_bounds__(RC_THREADS) void raycast_fill_rect_kernel(const double *__restrict__ seg, int64_t n_seg,
                                                                       RcGridEdges g, const int64_t *__restrict__ offset,
                                                                       int64_t *__restrict__ cell,
                                                                       double *__restrict__ chord) {
  const int64_t s = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x;
  if (s >= n_seg) return;
  const int64_t e0 = offset[s], cap = offset[s + 1] - e0;
  if (e0 < 0 || cap <= 0) return;
  rc_traverse<true>(seg + 6 * s, g, cell + e0, chord + e0, cap);
}

// Ascending bitonic network over key[0, len) with val carried along.  Every compare-exchange moves the smaller key to
// the lower index (first substage of a block mirrored, the rest straight), so the list behaves as if padded with
// +inf up to the next power of two, and pairs that reach past len are skipped.  Equal keys keep no particular order,
// but the same order in every run.  All loop bounds are uniform over the workgroup.
template <typename K>
__device__ inline void rc_sort(K *key, double *val, int len) {
  int P = 1;
  while (P < len) P <<= 1;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += RC_THREADS) {
        const int i = 2 * t - (t & (j - 1));
        const int l = (j == (k >> 1)) ? (i ^ (k - 1)) : (i ^ j);
        if (l < len) {
          const K a = key[i], b = key[l];
          if (a > b) {
            const double va = val[i], vb = val[l];
            key[i] = b; key[l] = a;
            val[i] = vb; val[l] = va;
          }
        }
      }
      __syncthreads();
    }
  }
}

// sorted (key, val) -> unique keys with summed vals at out[0..], their number to *uniq.  Each thread owns a contiguous
// chunk; a run is summed front to back by the thread that owns its head.
template <typename K>
__device__ inline void rc_emit(const K *key, const double *val, int len, int *s_cnt, int64_t *__restrict__ cell_out,
                               double *__restrict__ chord_out, int64_t *__restrict__ uniq) {
  const int t = threadIdx.x;
  const int c = (len + RC_THREADS - 1) / RC_THREADS;
  const int lo = min(t * c, len), hi = min(lo + c, len);
  int heads = 0;
  for (int i = lo; i < hi; ++i) heads += (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
  s_cnt[t] = heads;
  __syncthreads();
  for (int o = 1; o < RC_THREADS; o <<= 1) {       // inclusive scan
    const int v = t >= o ? s_cnt[t - o] : 0;
    __syncthreads();
    s_cnt[t] += v;
    __syncthreads();
  }
  int q = s_cnt[t] - heads;
  for (int i = lo; i < hi; ++i) {
    if (i == 0 || key[i] != key[i - 1]) {
      const K kk = key[i];
      double sum = 0.0;
      for (int j = i; j < len && key[j] == kk; ++j) sum += val[j];
      cell_out[q] = (int64_t)kk;
      chord_out[q] = sum;
      ++q;
    }
  }
  if (t == RC_THREADS - 1) *uniq = s_cnt[t];
}

__global__ __launch_bounds__(RC_THREADS) void raycast_merge_kernel(const int64_t *__restrict__ offset, int n_ray,
                                                                   int64_t *cell, double *chord,
                                                                   int64_t *__restrict__ cell_out,
                                                                   double *__restrict__ chord_out,
                                                                   int64_t *__restrict__ uniq) {
  __shared__ int s_key[RC_LDS_ENTRIES];
  __shared__ double s_val[RC_LDS_ENTRIES];
  __shared__ int s_cnt[RC_THREADS];
  const int64_t pix = blockIdx.x;
  const int64_t e0 = offset[pix * n_ray], e1 = offset[(pix + 1) * n_ray];
  const int64_t n = e1 - e0;
  const int len = n < 0 ? 0 : n > (1 << 30) ? (1 << 30) : (int)n;   // the host refuses what could exceed 2^30
  if (len <= RC_LDS_ENTRIES) {                      // uniform over the workgroup
    for (int i = threadIdx.x; i < len; i += RC_THREADS) {
      s_key[i] = (int)cell[e0 + i];
      s_val[i] = chord[e0 + i];
    }
    __syncthreads();
    rc_sort(s_key, s_val, len);
    rc_emit(s_key, s_val, len, s_cnt, cell_out + e0, chord_out + e0, uniq + pix);
  } else {                                          // the same network on the global buffer, by this workgroup alone
    rc_sort(cell + e0, chord + e0, len);
    rc_emit(cell + e0, chord + e0, len, s_cnt, cell_out + e0, chord_out + e0, uniq + pix);
  }
}

constexpr int RC_WAVES = RC_THREADS / 64;

// one wave per pixel
__global__ __launch_bounds__(RC_THREADS) void raycast_compact_kernel(const int64_t *__restrict__ offset, int64_t n_pix,
                                                                     int n_ray, const int64_t *__restrict__ cell,
                                                                     const double *__restrict__ chord,
                                                                     const int64_t *__restrict__ indptr, int weights,
                                                                     int64_t col0, int64_t *__restrict__ indices,
                                                                     double *__restrict__ vals) {
  const int64_t pix = (int64_t)blockIdx.x * RC_WAVES + (threadIdx.x >> 6);
  if (pix >= n_pix) return;
  const int lane = threadIdx.x & 63;
  const int64_t src = offset[pix * n_ray], dst = indptr[pix], n = indptr[pix + 1] - dst;
  const int64_t room = offset[(pix + 1) * n_ray] - src;      // a front is never longer than the pixel's range
  for (int64_t k = lane; k < n && k < room; k += 64) {
    indices[dst + k] = cell[src + k] + col0;
    vals[dst + k] = weights == SPR_RAYCAST_HIT ? 1.0 : chord[src + k] / (double)n_ray;
  }
}

// pointers first, then shapes, then the cell-count cap
int rc_check_grid(const char *who, int32_t nx, int32_t ny, int32_t nz, double ox, double oy, double oz, double hx,
                  double hy, double hz, RcGrid &g) {
  SPR_REQUIRE(nx > 0 && ny > 0 && nz > 0, SPR_E_INVALID, "%s: bad grid %d x %d x %d", who, nx, ny, nz);
  SPR_REQUIRE(isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(hx) && isfinite(hy) && isfinite(hz) && hx > 0.0 &&
                  hy > 0.0 && hz > 0.0,
              SPR_E_INVALID, "%s: origin and spacing must be finite, spacing positive", who);
  SPR_REQUIRE((int64_t)nx * ny < ((int64_t)1 << 31) && (int64_t)nx * ny * nz < ((int64_t)1 << 31), SPR_E_UNSUPPORTED,
              "%s: %d x %d x %d cells reach 2^31", who, nx, ny, nz);
  g.nx = nx; g.ny = ny; g.nz = nz;
  g.ox = ox; g.oy = oy; g.oz = oz;
  g.hx = hx; g.hy = hy; g.hz = hz;
  return SPR_OK;
}

// the rectilinear grid: the edge arrays live on the device, so only the counts can be checked here; the kernels hold
// for any contents
int rc_check_edges(const char *who, int32_t nx, int32_t ny, int32_t nz, const double *d_xe, const double *d_ye,
                   const double *d_ze, RcGridEdges &g) {
  SPR_REQUIRE(nx > 0 && ny > 0 && nz > 0, SPR_E_INVALID, "%s: bad grid %d x %d x %d", who, nx, ny, nz);
  SPR_REQUIRE((int64_t)nx * ny < ((int64_t)1 << 31) && (int64_t)nx * ny * nz < ((int64_t)1 << 31), SPR_E_UNSUPPORTED,
              "%s: %d x %d x %d cells reach 2^31", who, nx, ny, nz);
  g.nx = nx; g.ny = ny; g.nz = nz;
  g.xe = d_xe; g.ye = d_ye; g.ze = d_ze;
  return SPR_OK;
}

inline bool rc_seg_count_ok(int64_t n_seg) { return n_seg > 0 && n_seg <= (int64_t)INT32_MAX * RC_THREADS; }

// n_pix pixels of n_ray segments: a grid dimension, and a segment index, that fit
inline bool rc_pixels_ok(int64_t n_pix, int32_t n_ray) {
  return n_pix > 0 && n_ray > 0 && n_pix <= INT32_MAX && n_pix <= INT64_MAX / 2 / n_ray;
}

}  // namespace

extern "C" int32_t spr_raycast_merge_lds_entries(void) { return RC_LDS_ENTRIES; }

extern "C" int spr_raycast_count_f64(const double *d_seg, int64_t n_seg, int32_t nx, int32_t ny, int32_t nz, double ox,
                                     double oy, double oz, double hx, double hy, double hz, int64_t *d_count,
                                     void *stream) {
  const char *who = "spr_raycast_count_f64";
  SPR_REQUIRE(d_seg && d_count, SPR_E_INVALID, "%s: NULL pointer", who);
  SPR_REQUIRE(rc_seg_count_ok(n_seg), SPR_E_INVALID, "%s: bad segment count %lld", who, (long long)n_seg);
  RcGrid g;
  if (int rc = rc_check_grid(who, nx, ny, nz, ox, oy, oz, hx, hy, hz, g)) return rc;
  const unsigned grid = (unsigned)((n_seg + RC_THREADS - 1) / RC_THREADS);
  hipLaunchKernelGGL(raycast_count_kernel, dim3(grid), dim3(RC_THREADS), 0, static_cast<hipStream_t>(stream), d_seg, n_seg,
                     g, d_count);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

extern "C" int spr_raycast_fill_f64(const double *d_seg, int64_t n_seg, int32_t nx, int32_t ny, int32_t nz, double ox,
                                    double oy, double oz, double hx, double hy, double hz, const int64_t *d_offset,
                                    int64_t *d_cell, double *d_chord, void *stream) {
  const char *who = "spr_raycast_fill_f64";
  SPR_REQUIRE(d_seg && d_offset && d_cell && d_chord, SPR_E_INVALID, "%s: NULL pointer", who);
  SPR_REQUIRE(rc_seg_count_ok(n_seg), SPR_E_INVALID, "%s: bad segment count %lld", who, (long long)n_seg);
  RcGrid g;
  if (int rc = rc_check_grid(who, nx, ny, nz, ox, oy, oz, hx, hy, hz, g)) return rc;
  const unsigned grid = (unsigned)((n_seg + RC_THREADS - 1) / RC_THREADS);
  hipLaunchKernelGGL(raycast_fill_kernel, dim3(grid), dim3(RC_THREADS), 0, static_cast<hipStream_t>(stream), d_seg, n_seg,
                     g, d_offset, d_cell, d_chord);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

extern "C" int spr_raycast_count_rect_f64(const double *d_seg, int64_t n_seg, int32_t nx, int32_t ny, int32_t nz,
                                          const double *d_xe, const double *d_ye, const double *d_ze, int64_t *d_count,
                                          void *stream) {
  const char *who = "spr_raycast_count_rect_f64";
  SPR_REQUIRE(d_seg && d_xe && d_ye && d_ze && d_count, SPR_E_INVALID, "%s: NULL pointer", who);
  SPR_REQUIRE(rc_seg_count_ok(n_seg), SPR_E_INVALID, "%s: bad segment count %lld", who, (long long)n_seg);
  RcGridEdges g;
  if (int rc = rc_check_edges(who, nx, ny, nz, d_xe, d_ye, d_ze, g)) return rc;
  const unsigned grid = (unsigned)((n_seg + RC_THREADS - 1) / RC_THREADS);
  hipLaunchKernelGGL(raycast_count_rect_kernel, dim3(grid), dim3(RC_THREADS), 0, static_cast<hipStream_t>(stream), d_seg,
                     n_seg, g, d_count);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

extern "C" int spr_raycast_fill_rect_f64(const double *d_seg, int64_t n_seg, int32_t nx, int32_t ny, int32_t nz,
                                         const double *d_xe, const double *d_ye, const double *d_ze,
                                         const int64_t *d_offset, int64_t *d_cell, double *d_chord, void *stream) {
  const char *who = "spr_raycast_fill_rect_f64";
  SPR_REQUIRE(d_seg && d_xe && d_ye && d_ze && d_offset && d_cell && d_chord, SPR_E_INVALID, "%s: NULL pointer", who);
  SPR_REQUIRE(rc_seg_count_ok(n_seg), SPR_E_INVALID, "%s: bad segment count %lld", who, (long long)n_seg);
  RcGridEdges g;
  if (int rc = rc_check_edges(who, nx, ny, nz, d_xe, d_ye, d_ze, g)) return rc;
  const unsigned grid = (unsigned)((n_seg + RC_THREADS - 1) / RC_THREADS);
  hipLaunchKernelGGL(raycast_fill_rect_kernel, dim3(grid), dim3(RC_THREADS), 0, static_cast<hipStream_t>(stream), d_seg,
                     n_seg, g, d_offset, d_cell, d_chord);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

extern "C" int spr_raycast_merge(const int64_t *d_offset, int64_t n_pix, int32_t n_ray, int32_t max_cells_per_ray,
                                 int64_t *d_cell, double *d_chord, int64_t *d_cell_out, double *d_chord_out,
                                 int64_t *d_uniq, void *stream) {
  const char *who = "spr_raycast_merge";
  SPR_REQUIRE(d_offset && d_cell && d_chord && d_cell_out && d_chord_out && d_uniq, SPR_E_INVALID, "%s: NULL pointer", who);
  SPR_REQUIRE(d_cell != d_cell_out && d_chord != d_chord_out, SPR_E_INVALID, "%s: output buffers alias the input", who);
  SPR_REQUIRE(rc_pixels_ok(n_pix, n_ray) && max_cells_per_ray > 0, SPR_E_INVALID, "%s: bad shape n_pix=%lld n_ray=%d",
              who, (long long)n_pix, n_ray);
  SPR_REQUIRE((int64_t)n_ray * max_cells_per_ray <= ((int64_t)1 << 30), SPR_E_UNSUPPORTED,
              "%s: %d rays of up to %d cells exceed 2^30 entries per pixel", who, n_ray, max_cells_per_ray);
  hipLaunchKernelGGL(raycast_merge_kernel, dim3((unsigned)n_pix), dim3(RC_THREADS), 0, static_cast<hipStream_t>(stream),
                     d_offset, (int)n_ray, d_cell, d_chord, d_cell_out, d_chord_out, d_uniq);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

extern "C" int spr_raycast_compact(const int64_t *d_offset, int64_t n_pix, int32_t n_ray, const int64_t *d_cell,
                                   const double *d_chord, const int64_t *d_indptr, int32_t weights, int64_t col0,
                                   int64_t *d_indices, double *d_vals, void *stream) {
  const char *who = "spr_raycast_compact";
  SPR_REQUIRE(d_offset && d_cell && d_chord && d_indptr && d_indices && d_vals, SPR_E_INVALID, "%s: NULL pointer", who);
  SPR_REQUIRE(rc_pixels_ok(n_pix, n_ray) && col0 >= 0, SPR_E_INVALID, "%s: bad shape n_pix=%lld n_ray=%d col0=%lld", who,
              (long long)n_pix, n_ray, (long long)col0);
  SPR_REQUIRE(weights == SPR_RAYCAST_HIT || weights == SPR_RAYCAST_LENGTH, SPR_E_INVALID, "%s: weights %d is neither hit nor length",
              who, weights);
  const unsigned grid = (unsigned)((n_pix + RC_WAVES - 1) / RC_WAVES);
  hipLaunchKernelGGL(raycast_compact_kernel, dim3(grid), dim3(RC_THREADS), 0, static_cast<hipStream_t>(stream), d_offset,
                     n_pix, (int)n_ray, d_cell, d_chord, d_indptr, (int)weights, col0, d_indices, d_vals);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}
