// Resampling of point-cloud snapshots: values at one cloud of cell centres -> another cloud or the centres of a voxel grid.
//
// Stands where the reference has resample_to_grid (utils.py:17-99, VTK's probe filter) and the GPR notebook its
// griddata(..., method='nearest') loop.  The operator is sparse, at most k <= 8 entries per target:
//   neighbours  the k sources smallest under (d2, source index), lexicographic; d2 = float64 squared distance, formed as
//               ((dx dx) + (dy dy)) + (dz dz) with every product and sum rounded once (no contraction);
//   weights     'nearest': 1.  'idw' (Shepard, power 2): w_j = (1 / d2_j) / sum_i (1 / d2_i); d2_0 == 0: 1, 0, 0, ...
//   apply       out[f n_dst + c, :] = sum_j w[c, j] X[f n_src + idx[c, j], :], j ascending, in float64; 'nearest' copies bits.
//
// Three kernels; the sort of the bin keys and the prefix sum over the bin counts are the caller's (torch.sort, cumsum):
//   bin     one thread per source: the key of its bin in a uniform grid over the sources' bounding box
//   knn     one thread per target: shells of bins of growing Chebyshev radius around the target's clamped bin, best-K list
//           in registers; stops when the K-th best d2 is STRICTLY below the squared distance to the unsearched bins
//   apply   one wave per destination row: wave-uniform indices and weights, lanes across the m columns, up to 8 source rows
//           in flight per wave ('nearest': 4 destination rows at once, two pieces of each), grid-stride over (feature, target)
// rs_bin() is the ONE map from a coordinate to a bin index, used for placing sources and for placing queries.
// No atomics, no LDS, no barriers: two runs agree bit for bit.  Every loop of the search is bounded by the bin counts
// (radius <= the largest of them) and by the caller's start array clamped to [0, n_src]; an index that is negative or not
// below n_src is never dereferenced by apply.
#include <math.h>

#include "common.hpp"
#include "launch.hpp"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_WAVES_PER_CU = 16;     // the measured recipe of the register gather
constexpr int RS_NEAREST_ROWS = 4;      // destination rows a wave of the 'nearest' copy has in flight
constexpr int RS_MAX_K = 8;
constexpr int32_t RS_EMPTY = INT32_MAX;
constexpr double RS_EPS = 2.220446049250313e-16;

struct RsBins {
  int nb[3];
  double lo[3], inv[3], w[3], slack[3];   // inv = bins per unit length (0: an axis without extent), w = bin width
};

struct RsGrid {
  int nx, ny, nz;
  double ox, oy, oz, hx, hy, hz;
};

// the bin of coordinate p along one axis, clamped into the grid; monotone in p; a NaN ends as 0
__device__ inline int rs_bin(double p, double lo, double inv, int nb) {
#pragma clang fp contract(off)
  double f = floor((p - lo) * inv);
  f = fmin(fmax(f, 0.0), (double)(nb - 1));
  return (int)f;
}

__device__ inline double rs_d2(double qx, double qy, double qz, double sx, double sy, double sz) {
#pragma clang fp contract(off)
  const double dx = qx - sx, dy = qy - sy, dz = qz - sz;
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  return (xx + yy) + zz;
}

// a centre of VoxelGrid.cell_centers, in its arithmetic: the product rounded, then the sum
__device__ inline double rs_centre(double o, double h, int i) {
#pragma clang fp contract(off)
  const double t = ((double)i + 0.5) * h;
  return o + t;
}

__global__ __launch_bounds__(RS_THREADS) void resample_bin_kernel(const double *__restrict__ xyz, int64_t n_src, RsBins b,
                                                                  int64_t *__restrict__ key) {
  const int64_t s = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (s >= n_src) return;
  const int bx = rs_bin(xyz[3 * s], b.lo[0], b.inv[0], b.nb[0]);
  const int by = rs_bin(xyz[3 * s + 1], b.lo[1], b.inv[1], b.nb[1]);
  const int bz = rs_bin(xyz[3 * s + 2], b.lo[2], b.inv[2], b.nb[2]);
  key[s] = (int64_t)bx + (int64_t)b.nb[0] * ((int64_t)by + (int64_t)b.nb[1] * bz);
}

// Distance from q to the bins of one axis outside [i0, i1], made SMALLER than the true one by the rounding of rs_bin and of
// the faces (slack) so that no source in an unsearched bin is nearer; +inf where the block ends at the grid's outer face.
__device__ inline double rs_axis_gap(double q, double lo, double w, double slack, int i0, int i1, int nb) {
  double g = INFINITY;
  if (i0 > 0) g = fmin(g, q - fma((double)i0, w, lo));
  if (i1 < nb - 1) g = fmin(g, fma((double)(i1 + 1), w, lo) - q);
  return g == INFINITY ? g : g * (1.0 - 8.0 * RS_EPS) - slack;
}

// The best k <= K candidates under (d2, index), ascending, in the LAST k of K register slots; the first K - k slots hold
// -inf, which no candidate displaces, so the k-th best is always d[K - 1]: every index into the arrays is a constant
// (a run-time index would send them to scratch).
template <int K>
struct RsBest {
  double d[K];
  int32_t i[K];
  __device__ __forceinline__ void init(int k) {
#pragma unroll
    for (int j = 0; j < K; ++j) { d[j] = j < K - k ? -INFINITY : INFINITY; i[j] = RS_EMPTY; }
  }
  // insertion, fully unrolled: the candidate sinks to its place, the displaced entries move down, the last one drops out
  __device__ __forceinline__ void insert(double cd, int32_t ci) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const bool less = cd < d[j] || (cd == d[j] && ci < i[j]);
      const double td = d[j];
      const int32_t ti = i[j];
      d[j] = less ? cd : td;
      i[j] = less ? ci : ti;
      cd = less ? td : cd;
      ci = less ? ti : ci;
    }
  }
};

template <int K>
__global__ __launch_bounds__(RS_THREADS) void resample_knn_kernel(const double *__restrict__ src, const int64_t *__restrict__ perm,
                                                                  const int64_t *__restrict__ start, int64_t n_src, RsBins b,
                                                                  const double *__restrict__ dst, int64_t n_dst, RsGrid g,
                                                                  int k, int idw, double dmax, int64_t *__restrict__ idx,
                                                                  double *__restrict__ d2, double *__restrict__ weight,
                                                                  int32_t *__restrict__ inspected) {
  const int64_t c = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (c >= n_dst) return;
  double qx, qy, qz;
  if (dst) {
    qx = dst[3 * c]; qy = dst[3 * c + 1]; qz = dst[3 * c + 2];
  } else {                                          // the arithmetic of VoxelGrid.cell_centers: origin + (i + 0.5) spacing
    const int64_t plane = (int64_t)g.nx * g.ny;
    const int kz = (int)(c / plane);
    const int64_t rem = c - (int64_t)kz * plane;
    const int jy = (int)(rem / g.nx), ix = (int)(rem - (int64_t)jy * g.nx);
    qx = rs_centre(g.ox, g.hx, ix);
    qy = rs_centre(g.oy, g.hy, jy);
    qz = rs_centre(g.oz, g.hz, kz);
  }
  const int bx = rs_bin(qx, b.lo[0], b.inv[0], b.nb[0]);
  const int by = rs_bin(qy, b.lo[1], b.inv[1], b.nb[1]);
  const int bz = rs_bin(qz, b.lo[2], b.inv[2], b.nb[2]);
  const bool limited = dmax >= 0.0;
  const double dmax2 = dmax * dmax;
  RsBest<K> best;
  best.init(k);
  int seen = 0;
  const int max_r = max(b.nb[0], max(b.nb[1], b.nb[2]));
  for (int R = 0; R <= max_r; ++R) {                   // R == 0: the query's own bin, through the face branch
    const int x0 = max(bx - R, 0), x1 = min(bx + R, b.nb[0] - 1);
    const int y0 = max(by - R, 0), y1 = min(by + R, b.nb[1] - 1);
    const int z0 = max(bz - R, 0), z1 = min(bz + R, b.nb[2] - 1);
    for (int iz = z0; iz <= z1; ++iz) {
      for (int iy = y0; iy <= y1; ++iy) {
        const bool face = (iz - bz == R) || (bz - iz == R) || (iy - by == R) || (by - iy == R);
        const int64_t row = (int64_t)b.nb[0] * ((int64_t)iy + (int64_t)b.nb[1] * iz);
        // a row of the shell's faces: all its bins, which are consecutive keys; else the two bins at distance R in x
        for (int part = 0; part < (face ? 1 : 2); ++part) {
          int a0, a1;
          if (face) { a0 = x0; a1 = x1; }
          else if (part == 0) { a0 = a1 = bx - R; }
          else { a0 = a1 = bx + R; }
          if (a0 < 0 || a1 >= b.nb[0]) continue;
          int64_t p0 = start[row + a0], p1 = start[row + a1 + 1];
          p0 = p0 < 0 ? 0 : p0;
          p1 = p1 > n_src ? n_src : p1;
          for (int64_t p = p0; p < p1; ++p) {
            const double cd = rs_d2(qx, qy, qz, src[3 * p], src[3 * p + 1], src[3 * p + 2]);
            ++seen;
            if (limited && cd > dmax2) continue;
            const int64_t s = perm[p];
            if (s < 0 || s >= n_src) continue;
            best.insert(cd, (int32_t)s);
          }
        }
      }
    }
    if (x0 == 0 && y0 == 0 && z0 == 0 && x1 == b.nb[0] - 1 && y1 == b.nb[1] - 1 && z1 == b.nb[2] - 1) break;
    const double gap = fmin(fmin(rs_axis_gap(qx, b.lo[0], b.w[0], b.slack[0], x0, x1, b.nb[0]),
                                 rs_axis_gap(qy, b.lo[1], b.w[1], b.slack[1], y0, y1, b.nb[1])),
                            rs_axis_gap(qz, b.lo[2], b.w[2], b.slack[2], z0, z1, b.nb[2]));
    if (gap > 0.0) {
      if (best.d[K - 1] < gap * gap) break;            // strictly: a source at exactly the gap may carry a lower index
      if (limited && gap > dmax) break;
    }
  }
  const int pad = K - k;                              // slot pad + j holds neighbour j
  double inv[K], sum = 0.0;
  bool hit0 = false;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    const bool used = s >= pad && best.i[s] != RS_EMPTY;
    inv[s] = used ? 1.0 / best.d[s] : 0.0;
    if (used) sum += inv[s];
    hit0 = hit0 || (s == pad && used && best.d[s] == 0.0);
  }
#pragma unroll
  for (int s = 0; s < K; ++s) {
    const int j = s - pad;
    if (j >= 0) {
      const bool used = best.i[s] != RS_EMPTY;
      double w = 0.0;
      if (used) w = (!idw || hit0) ? (j == 0 ? 1.0 : 0.0) : inv[s] / sum;
      idx[c * k + j] = used ? (int64_t)best.i[s] : (int64_t)-1;
      d2[c * k + j] = used ? best.d[s] : INFINITY;
      weight[c * k + j] = w;
    }
  }
  inspected[c] = seen;
}

// ---- apply ----------------------------------------------------------------------------------------------------------------
template <typename T, int V> struct RsVec;
template <> struct RsVec<double, 1> { using type = double; };
template <> struct RsVec<double, 2> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct RsVec<float, 1> { using type = float; };
template <> struct RsVec<float, 2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct RsVec<float, 4> { typedef float type __attribute__((ext_vector_type(4))); };

template <typename T, int V>
__device__ inline void rs_fill(typename RsVec<T, V>::type &v, T x) {
  T *e = reinterpret_cast<T *>(&v);
#pragma unroll
  for (int t = 0; t < V; ++t) e[t] = x;
}

// 'nearest': RS_NEAREST_ROWS consecutive destination rows per wave and step, two pieces of every source row loaded before the
// first is stored (whole rows of up to 2 KB: 8 loads in flight per lane); the bits are copied, no arithmetic touches them.
// Every row is read once and written once, so both go past the caches (nontemporal): measured 5 % faster than plain.
template <typename T, int V>
__global__ __launch_bounds__(RS_THREADS) void resample_copy_kernel(const T *__restrict__ X, int64_t ldx, int64_t n_src,
                                                                   int n_features, int m, const int64_t *__restrict__ idx,
                                                                   int64_t n_dst, int k, T fill, T *__restrict__ out,
                                                                   int64_t ldo) {
  using Vec = typename RsVec<T, V>::type;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t gpf = (n_dst + RS_NEAREST_ROWS - 1) / RS_NEAREST_ROWS;   // groups per feature: a group stays inside one
  const int64_t stride = (int64_t)gridDim.x * RS_WAVES;
  const int ncg = m / V;
  Vec fillv;
  rs_fill<T, V>(fillv, fill);
  // (feature, group) advance by additions: a 64-bit division per row costs the wave more instructions than the copy itself
  const int64_t first = (int64_t)blockIdx.x * RS_WAVES + wave;
  int64_t f = first / gpf, g = first - f * gpf;
  while (f < n_features) {
    int64_t srow[RS_NEAREST_ROWS], drow[RS_NEAREST_ROWS];   // wave-uniform: the source and destination rows, or -1
#pragma unroll
    for (int q = 0; q < RS_NEAREST_ROWS; ++q) {
      const int64_t c = g * RS_NEAREST_ROWS + q;
      srow[q] = -1;
      drow[q] = c < n_dst ? f * n_dst + c : -1;
      if (c < n_dst) {
        const int64_t s = idx[c * k];
        if (s >= 0 && s < n_src) srow[q] = f * n_src + s;
      }
    }
    for (int cg = lane; cg < ncg; cg += 2 * 64) {       // two pieces of every row: 8 loads in flight per lane
      const int cg2 = cg + 64;
      const bool two = cg2 < ncg;
      Vec v[RS_NEAREST_ROWS][2];
#pragma unroll
      for (int q = 0; q < RS_NEAREST_ROWS; ++q) {
        v[q][0] = fillv;
        v[q][1] = fillv;
        if (srow[q] >= 0) {
          const T *x = X + srow[q] * ldx;
          v[q][0] = __builtin_nontemporal_load(reinterpret_cast<const Vec *>(x + (int64_t)cg * V));
          if (two) v[q][1] = __builtin_nontemporal_load(reinterpret_cast<const Vec *>(x + (int64_t)cg2 * V));
        }
      }
#pragma unroll
      for (int q = 0; q < RS_NEAREST_ROWS; ++q) {
        if (drow[q] >= 0) {
          T *o = out + drow[q] * ldo;
          __builtin_nontemporal_store(v[q][0], reinterpret_cast<Vec *>(o + (int64_t)cg * V));
          if (two) __builtin_nontemporal_store(v[q][1], reinterpret_cast<Vec *>(o + (int64_t)cg2 * V));
        }
      }
    }
    g += stride;
    while (g >= gpf && f < n_features) { g -= gpf; ++f; }
  }
}

// 'idw': one destination row per wave and step, its K source rows' pieces loaded before the first is used
template <typename T, int V, int K>
__global__ __launch_bounds__(RS_THREADS) void resample_idw_kernel(const T *__restrict__ X, int64_t ldx, int64_t n_src,
                                                                  int n_features, int m, const int64_t *__restrict__ idx,
                                                                  const double *__restrict__ weight, int64_t n_dst, int k,
                                                                  T fill, T *__restrict__ out, int64_t ldo) {
  using Vec = typename RsVec<T, V>::type;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * RS_WAVES;
  const int ncg = m / V;
  Vec fillv;
  rs_fill<T, V>(fillv, fill);
  const int64_t first = (int64_t)blockIdx.x * RS_WAVES + wave;
  int64_t f = first / n_dst, c = first - f * n_dst;     // advanced by additions, see resample_copy_kernel
  for (; f < n_features; c += stride) {
    while (c >= n_dst && f < n_features) { c -= n_dst; ++f; }
    if (f >= n_features) break;
    const int64_t row = f * n_dst + c;
    int64_t srow[K];
    double w[K];
    bool any = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      srow[j] = -1;
      w[j] = 0.0;
      if (j < k) {
        const int64_t s = idx[c * k + j];
        if (s >= 0 && s < n_src) {
          srow[j] = f * n_src + s;
          w[j] = weight[c * k + j];
          any = true;
        }
      }
    }
    T *o = out + row * ldo;
    if (!any) {                                       // an invalid target: the fill value in every column
      for (int cg = lane; cg < ncg; cg += 64) *reinterpret_cast<Vec *>(o + (int64_t)cg * V) = fillv;
      continue;
    }
    for (int cg = lane; cg < ncg; cg += 64) {
      Vec v[K];
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (srow[j] >= 0) v[j] = *reinterpret_cast<const Vec *>(X + srow[j] * ldx + (int64_t)cg * V);
      double acc[V];
#pragma unroll
      for (int t = 0; t < V; ++t) acc[t] = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (srow[j] >= 0) {
          const T *e = reinterpret_cast<const T *>(&v[j]);
#pragma unroll
          for (int t = 0; t < V; ++t) acc[t] += w[j] * (double)e[t];
        }
      }
      Vec r;
      T *e = reinterpret_cast<T *>(&r);
#pragma unroll
      for (int t = 0; t < V; ++t) e[t] = (T)acc[t];
      *reinterpret_cast<Vec *>(o + (int64_t)cg * V) = r;
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// the bin grid both entry points build from the same arguments: one spelling of inv, w and slack
int rs_make_bins(const char *who, int32_t nbx, int32_t nby, int32_t nbz, double lox, double loy, double loz, double hix,
                 double hiy, double hiz, int64_t n_src, RsBins &b) {
  SPR_REQUIRE(nbx > 0 && nby > 0 && nbz > 0, SPR_E_INVALID, "%s: bad bin counts %d x %d x %d", who, nbx, nby, nbz);
  const double lo[3] = {lox, loy, loz}, hi[3] = {hix, hiy, hiz};
  const int nb[3] = {nbx, nby, nbz};
  for (int a = 0; a < 3; ++a) {
    SPR_REQUIRE(isfinite(lo[a]) && isfinite(hi[a]) && hi[a] >= lo[a] && isfinite(hi[a] - lo[a]), SPR_E_INVALID,
                "%s: the bounding box must be finite with hi >= lo", who);
    SPR_REQUIRE(hi[a] > lo[a] || nb[a] == 1, SPR_E_INVALID, "%s: an axis without extent has one bin, not %d", who, nb[a]);
    const double ext = hi[a] - lo[a];
    b.nb[a] = nb[a];
    b.lo[a] = lo[a];
    b.inv[a] = ext > 0.0 ? (double)nb[a] / ext : 0.0;
    b.w[a] = ext / (double)nb[a];
    b.slack[a] = 16.0 * RS_EPS * (fabs(lo[a]) + fabs(hi[a]));
    SPR_REQUIRE(isfinite(b.inv[a]), SPR_E_INVALID, "%s: the extent of axis %d is too small for %d bins", who, a, nb[a]);
  }
  const int64_t total = (int64_t)nbx * nby * nbz;
  SPR_REQUIRE((int64_t)nbx * nby < ((int64_t)1 << 31) && total < ((int64_t)1 << 31) && total <= 8 * n_src + 8, SPR_E_UNSUPPORTED,
              "%s: %d x %d x %d bins exceed 8 per source point or 2^31", who, nbx, nby, nbz);
  return SPR_OK;
}

inline bool rs_count_ok(int64_t n) { return n > 0 && n < ((int64_t)1 << 31); }

inline int rs_round_k(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8; }

template <typename T>
int rs_apply(const char *who, const T *d_X, int64_t ldx, int64_t n_src, int32_t n_features, int32_t m, const int64_t *d_idx,
             const double *d_weight, int64_t n_dst, int32_t k, int32_t method, double fill_value, T *d_out, int64_t ldo,
             void *stream) {
  SPR_REQUIRE(d_X && d_idx && d_weight && d_out, SPR_E_INVALID, "%s: NULL pointer", who);
  SPR_REQUIRE((const void *)d_X != (const void *)d_out, SPR_E_INVALID, "%s: the output aliases the input", who);
  SPR_REQUIRE(n_src > 0 && n_dst > 0 && n_features > 0 && m > 0 && ldx >= m && ldo >= m, SPR_E_INVALID,
              "%s: bad shape n_src=%lld n_dst=%lld n_features=%d m=%d ldx=%lld ldo=%lld", who, (long long)n_src,
              (long long)n_dst, n_features, m, (long long)ldx, (long long)ldo);
  SPR_REQUIRE(k >= 1 && k <= RS_MAX_K, SPR_E_INVALID, "%s: k = %d is outside 1 .. %d", who, k, RS_MAX_K);
  SPR_REQUIRE(method == SPR_RESAMPLE_NEAREST || method == SPR_RESAMPLE_IDW, SPR_E_INVALID, "%s: method %d is neither nearest nor idw",
              who, method);
  SPR_REQUIRE(rs_count_ok(n_src) && rs_count_ok(n_dst), SPR_E_UNSUPPORTED, "%s: 2^31 or more points", who);
  const int64_t units = (int64_t)n_features * (method == SPR_RESAMPLE_NEAREST ? (n_dst + RS_NEAREST_ROWS - 1) / RS_NEAREST_ROWS : n_dst);
  const int64_t want = (units + RS_WAVES - 1) / RS_WAVES;
  const int64_t cap = (int64_t)spr_cus_or_default() * (RS_WAVES_PER_CU / RS_WAVES);
  const dim3 grid((unsigned)(want < cap ? want : cap)), block(RS_THREADS);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const T fill = (T)fill_value;
  // elements per lane and load: 16 bytes where every row of both matrices starts on a 16-byte boundary and m fills whole
  // pieces, pairs of float where only 8 bytes are granted, single elements otherwise
  constexpr int W16 = 16 / (int)sizeof(T);
  int vec = 1;
  if (m % W16 == 0 && spr_rows_aligned16(d_X, (size_t)ldx * sizeof(T)) && spr_rows_aligned16(d_out, (size_t)ldo * sizeof(T)))
    vec = W16;
  else if (sizeof(T) == 4 && spr_pair_aligned(d_X, (int64_t)m, ldx) && spr_pair_aligned(d_out, (int64_t)m, ldo))
    vec = 2;
#define RS_LAUNCH_(V)                                                                                                      \
  do {                                                                                                                     \
    if (method == SPR_RESAMPLE_NEAREST) {                                                                                  \
      hipLaunchKernelGGL((resample_copy_kernel<T, V>), grid, block, 0, st, d_X, ldx, n_src, (int)n_features, (int)m, d_idx, \
                         n_dst, (int)k, fill, d_out, ldo);                                                                 \
    } else {                                                                                                               \
      SPR_DISPATCH_POW2(rs_round_k(k), who, k,                                                                             \
                        hipLaunchKernelGGL((resample_idw_kernel<T, V, RUNG>), grid, block, 0, st, d_X, ldx, n_src,         \
                                           (int)n_features, (int)m, d_idx, d_weight, n_dst, (int)k, fill, d_out, ldo));    \
    }                                                                                                                      \
  } while (0)
  if (vec == W16) RS_LAUNCH_(W16);
  else if (vec == 2) RS_LAUNCH_((sizeof(T) == 4 ? 2 : W16));
  else RS_LAUNCH_(1);
#undef RS_LAUNCH_
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

}  // namespace

extern "C" int spr_resample_bin_f64(const double *d_xyz, int64_t n_src, int32_t nbx, int32_t nby, int32_t nbz, double lox,
                                    double loy, double loz, double hix, double hiy, double hiz, int64_t *d_key,
                                    void *stream) {
  const char *who = "spr_resample_bin_f64";
  SPR_REQUIRE(d_xyz && d_key, SPR_E_INVALID, "%s: NULL pointer", who);
  SPR_REQUIRE(n_src > 0, SPR_E_INVALID, "%s: bad source count %lld", who, (long long)n_src);
  SPR_REQUIRE(rs_count_ok(n_src), SPR_E_UNSUPPORTED, "%s: 2^31 or more source points", who);
  RsBins b;
  if (int rc = rs_make_bins(who, nbx, nby, nbz, lox, loy, loz, hix, hiy, hiz, n_src, b)) return rc;
  const unsigned grid = (unsigned)((n_src + RS_THREADS - 1) / RS_THREADS);
  hipLaunchKernelGGL(resample_bin_kernel, dim3(grid), dim3(RS_THREADS), 0, static_cast<hipStream_t>(stream), d_xyz, n_src, b,
                     d_key);
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

extern "C" int spr_resample_knn_f64(const double *d_src_sorted, const int64_t *d_perm, const int64_t *d_start, int64_t n_src,
                                    int32_t nbx, int32_t nby, int32_t nbz, double lox, double loy, double loz, double hix,
                                    double hiy, double hiz, const double *d_dst, int64_t n_dst, int32_t gx, int32_t gy,
                                    int32_t gz, double ox, double oy, double oz, double hx, double hy, double hz, int32_t k,
                                    int32_t method, double max_distance, int64_t *d_idx, double *d_d2, double *d_weight,
                                    int32_t *d_inspected, void *stream) {
  const char *who = "spr_resample_knn_f64";
  SPR_REQUIRE(d_src_sorted && d_perm && d_start && d_idx && d_d2 && d_weight && d_inspected, SPR_E_INVALID, "%s: NULL pointer",
              who);
  SPR_REQUIRE(n_src > 0 && n_dst > 0, SPR_E_INVALID, "%s: bad point counts n_src=%lld n_dst=%lld", who, (long long)n_src,
              (long long)n_dst);
  SPR_REQUIRE(k >= 1 && k <= RS_MAX_K, SPR_E_INVALID, "%s: k = %d is outside 1 .. %d", who, k, RS_MAX_K);
  SPR_REQUIRE(method == SPR_RESAMPLE_NEAREST || method == SPR_RESAMPLE_IDW, SPR_E_INVALID, "%s: method %d is neither nearest nor idw",
              who, method);
  SPR_REQUIRE(method == SPR_RESAMPLE_IDW || k == 1, SPR_E_INVALID, "%s: nearest means k = 1, not %d", who, k);
  SPR_REQUIRE(!isnan(max_distance), SPR_E_INVALID, "%s: max_distance is NaN (negative: no limit)", who);
  SPR_REQUIRE(rs_count_ok(n_src) && rs_count_ok(n_dst), SPR_E_UNSUPPORTED, "%s: 2^31 or more points", who);
  RsBins b;
  if (int rc = rs_make_bins(who, nbx, nby, nbz, lox, loy, loz, hix, hiy, hiz, n_src, b)) return rc;
  RsGrid g = {1, 1, 1, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0};
  if (!d_dst) {                                       // targets are the centres of a voxel grid, formed by the kernel
    SPR_REQUIRE(gx > 0 && gy > 0 && gz > 0 && (int64_t)gx * gy < ((int64_t)1 << 31) && (int64_t)gx * gy * gz == n_dst,
                SPR_E_INVALID, "%s: a grid of %d x %d x %d cells does not have %lld centres", who, gx, gy, gz, (long long)n_dst);
    SPR_REQUIRE(isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(hx) && isfinite(hy) && isfinite(hz) && hx > 0.0 &&
                    hy > 0.0 && hz > 0.0,
                SPR_E_INVALID, "%s: origin and spacing must be finite, spacing positive", who);
    g.nx = gx; g.ny = gy; g.nz = gz;
    g.ox = ox; g.oy = oy; g.oz = oz;
    g.hx = hx; g.hy = hy; g.hz = hz;
  }
  const unsigned grid = (unsigned)((n_dst + RS_THREADS - 1) / RS_THREADS);
  const dim3 gd(grid), bd(RS_THREADS);
  hipStream_t st = static_cast<hipStream_t>(stream);
  SPR_DISPATCH_POW2(rs_round_k(k), who, k,
                    hipLaunchKernelGGL((resample_knn_kernel<RUNG>), gd, bd, 0, st, d_src_sorted, d_perm, d_start, n_src, b, d_dst,
                                       n_dst, g, (int)k, (int)(method == SPR_RESAMPLE_IDW), max_distance, d_idx, d_d2, d_weight,
                                       d_inspected));
  SPR_LAUNCH_CHECK();
  return SPR_OK;
}

extern "C" int spr_resample_apply_f64(const double *d_X, int64_t ldx, int64_t n_src, int32_t n_features, int32_t m,
                                      const int64_t *d_idx, const double *d_weight, int64_t n_dst, int32_t k, int32_t method,
                                      double fill_value, double *d_out, int64_t ldo, void *stream) {
  return rs_apply<double>("spr_resample_apply_f64", d_X, ldx, n_src, n_features, m, d_idx, d_weight, n_dst, k, method,
                          fill_value, d_out, ldo, stream);
}

extern "C" int spr_resample_apply_x32(const float *d_X, int64_t ldx, int64_t n_src, int32_t n_features, int32_t m,
                                      const int64_t *d_idx, const double *d_weight, int64_t n_dst, int32_t k, int32_t method,
                                      double fill_value, float *d_out, int64_t ldo, void *stream) {
  return rs_apply<float>("spr_resample_apply_x32", d_X, ldx, n_src, n_features, m, d_idx, d_weight, n_dst, k, method,
                         fill_value, d_out, ldo, stream);
}
