/*
 * spr_hip.h -- C ABI of libspr_hip.so: the MI355X (gfx950) kernels under
 * openmeasure_amd.sparse_sensing.SPR.
 *
 * The reference (burn-research/OpenMEASURE, src/openmeasure/sparse_sensing.py) has no
 * FFI; its "operator interface" for this path is the set of NumPy/SciPy calls listed in
 * SURVEY.md section 2 (K1..K11).  Each entry point below replaces one of those call
 * sites and says which (file:line of sparse_sensing.py).  The Python class in
 * openmeasure_amd/rom.py (imported as openmeasure_amd.sparse_sensing) binds them with ctypes; INTEGRATION.md shows the
 * same binding as a maintainer of the reference would add it.
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer (HBM) owned by the caller; the
 *     library allocates nothing (one exception: spr_p2p_alloc, whose interprocess handle needs
 *     the base pointer of an allocation) and keeps no state between calls;
 *   - matrices are row-major float64; "ld*" is the row stride in elements;
 *   - rows of the snapshot matrix are feature-major (global row = f*n_points + cell,
 *     sparse_sensing.py:110); a rank holds the contiguous global rows
 *     [row0, row0+n_rows) and passes the GLOBAL n_points so kernels can tell the
 *     feature of every local row;
 *   - stream is a hipStream_t passed as void* (NULL = default stream); all work is
 *     enqueued asynchronously on it, nothing synchronises the host;
 *   - return value: 0 = ok, <0 = error (SPR_E_*); spr_last_error() gives the text for
 *     the calling thread.  No C++ exception crosses this boundary.
 *
 * Which kernel an entry point launches depends on its arguments alone.  Environment variables read by the library (operational
 * settings and diagnostics of the multi-GPU paths; each is read once per process, at the first call that consults it):
 *   SPR_RESERVE_CUS=k         every persistent grid is sized for k compute units fewer (multi-GPU diagnostic: leaves CUs to
 *                             RCCL's kernel, which cannot share one with the Gram / projection workgroups)
 *   SPR_P2P_BLIT=1            spr_p2p_copy / spr_field_gather_p2p: blit kernels instead of the SDMA engines
 *   SPR_P2P_PROBE=1           spr_field_gather_p2p prints the host time of each of its runtime calls (tools/p2p_push_probe.py)
 *   SPR_RCCL_LIBRARY=<path>   spr_comm_*: the RCCL library to load (default: the one already in the process, else librccl.so.1)
 * and by the Python layer (openmeasure_amd/):
 * SPR_GAP_FILLER=1|0 (ROM.gap_filler, opt-in: a filler launch in fit()'s host gap), SPR_GATHER=auto|p2p|rccl (field exchange of
 * sharded objects), SPR_GATHER_TRIAL=0 (no first-exchange trial of the two exchanges: 'auto' = p2p whenever available),
 * SPR_DEFER_RECONSTRUCT=0|1 (ROM.defer_reconstruct), SPR_NATIVE_COMM=1 (fit()'s all-reduce through spr_fit_gram_pass / this library's
 * own communicator), SPR_P2P_STREAMS / SPR_P2P_BUFFERS / SPR_P2P_MEMORY / SPR_P2P_JOIN_TIMEOUT_S / SPR_P2P_RELEASE_TIMEOUT_S
 * (openmeasure_amd/p2p.py), SPR_PINNED_RESULT_GB=<g> (budget of page-locked
 * memory for host results still alive, default 8; 0 = pageable copies only), SPR_TRACE=1 (per-phase wall clock of fit(),
 * synchronising), SPR_HIP_LIBRARY=<path> (another build of this library: how two builds are compared in one process,
 * tools/kernel_ab.py).  None of them is needed in production.
 */
#ifndef SPR_HIP_H
#define SPR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPR_OK 0
#define SPR_E_INVALID (-1)   /* bad argument (shape, alignment, NULL)            */
#define SPR_E_UNSUPPORTED (-2) /* shape outside what the kernels are built for   */
#define SPR_E_HIP (-3)       /* a HIP runtime call failed                        */
#define SPR_E_WORKSPACE (-4) /* workspace too small                              */

#define SPR_MAX_M 256        /* snapshots (columns of X) one symmetric-Gram / register-resident projection launch handles */
#define SPR_MAX_M_WIDE 512   /* ... and the two-slice Gram path that forms the row means itself (spr_gram_cross, centre 1);
                                wider matrices go as slice pairs (spr_gram_cross_pair), any m                       */
#define SPR_MAX_R 128        /* retained modes / sensors ONE launch handles; callers go in column groups beyond      */
#define SPR_MAX_R_STREAM 256 /* ... columns ONE spr_project_stream_f64 / _x32_f64out launch takes (float64 output, 16-byte-aligned rows,
                                m % 4 == 0, no row norms): all m columns of fit()'s refinement pass at m <= 256 with X read once */
#define SPR_MAX_R_WIDE 1024  /* ... the widest basis the placement / solve kernels accept (r <= m in the reference, :336) */

/* Bumped whenever an entry point changes its argument list or meaning (round 3 -> 4: spr_qr_steps_f64 gained
 * first_exact, new entry points arrived; round 5, still 4: the CU-free field exchange spr_p2p_* / spr_field_gather_p2p*,
 * spr_field_unstage_blocks_f64; 4 -> 5 (round 6): spr_field_gather_p2p gained d_status and the poison bit, the communicator
 * entry points spr_comm_* arrived).  A binding written for another value must refuse to
 * call into this library: openmeasure_amd/_lib.py compares spr_abi_version() with the value its prototypes were
 * written for. */
#define SPR_ABI_VERSION 5
int spr_abi_version(void);
const char *spr_last_error(void);
/* number of compute units of the current device (used to size persistent grids) */
int spr_device_cus(int *out_cus);
/* Small host -> device upload executed as a kernel on `stream` (no copy-engine dependency in front of the next
 * kernel): h_pinned_src is page-locked, device-visible host memory (hipHostMalloc / torch pin_memory), n_bytes a
 * multiple of 8.  Carries the small operands the reference keeps as host ndarrays next to X -- W = V_r S_r^-1
 * (sparse_sensing.py:272-279), X_scl per feature (:115), the coefficient vectors of reconstruct (:371) -- to
 * the device.  The source may be rewritten once work queued after this call on the stream has completed. */
int spr_upload_bytes(void *d_dst, const void *h_pinned_src, int64_t n_bytes, void *stream);
/* ... and back: n_bytes (multiple of 8, <= 4 MiB) from the device into page-locked, device-visible host memory, by a kernel on
 * `stream`, which then stores ticket_value at h_pinned_ticket (a 64-bit word of such memory as well) with system-scope release:
 * the host polls the ticket instead of blocking on an event.  Carries the scaled m x m Gram matrix and the feature statistics
 * to the host eigen-solve that replaces the V factor of np.linalg.svd (sparse_sensing.py:272) -- 32 KB at BASELINE config 2. */
int spr_download_bytes(void *h_pinned_dst, const void *d_src, int64_t n_bytes, void *h_pinned_ticket, uint64_t ticket_value,
                       void *stream);
/* HOST-side helper (host pointers, no device work): unit eigenvectors of the symmetric tridiagonal matrix (h_d[m], h_e[m-1]) for
 * the r eigenvalues h_lam, all at once -- the inverse iterations of LAPACK's dstein (dlagtf / dlagts) with the eigenvalue index
 * as the vectorised dimension, without dstein's re-orthogonalisation inside clusters (check the result; fit() falls back to
 * dstein).  h_Z: m x r row-major, column j belongs to h_lam[j].  Part of the host eigen-solve of the m x m Gram matrix between
 * the two passes of fit() -- the reference's np.linalg.svd call site (sparse_sensing.py:272), of which :336 keeps r vectors. */
int spr_host_tridiag_vectors(const double *h_d, const double *h_e, int32_t m, const double *h_lam, int32_t r, double *h_Z,
                             int32_t iterations);
/* ... and the whole route in one host call: h_G (m x m, symmetric) -> h_lam[m] (all eigenvalues, DESCENDING) and h_V (m x r
 * row-major: the unit eigenvectors of the r largest, column j belonging to h_lam[j]).  fn_dsytrd / fn_dsterf / fn_dormtr: the
 * addresses of the caller's LAPACK routines with the Fortran calling convention without hidden string lengths, as SciPy exports
 * them (scipy.linalg.cython_lapack.__pyx_capi__) -- this library links no LAPACK.  Returns 0; 1 when LAPACK reports a failure;
 * 2 when the vectors miss their orthonormality checks (close eigenvalues): the caller then takes dstein / dsyevd.  < 0: SPR_E_*. */
int spr_host_eig_top(const double *h_G, int32_t m, int32_t r, double *h_lam, double *h_V, void *fn_dsytrd, void *fn_dsterf,
                     void *fn_dormtr);
/* The same idea for the SVD that ends fit()'s conditioning refinement pass (np.linalg.svd of an m x m factor, openmeasure_amd/rom.py
 * _refine_spectrum; reference: the accuracy of np.linalg.svd(X0), :272): ALL singular values (h_S, descending) and the r leading
 * RIGHT singular vectors (h_V, m x r row-major) of the row-major m x m matrix h_M -- dgebrd, dbdsdc (values only), the batched
 * inverse iteration on the Golub-Kahan form of the bidiagonal matrix, dormbr; LAPACK again through the caller's function
 * pointers.  0 ok, 1 LAPACK failed, 2 the vectors failed their orthonormality checks (take dgesdd). */
int spr_host_svd_top(const double *h_M, int32_t m, int32_t r, double *h_S, double *h_V, void *fn_dgebrd, void *fn_dbdsdc,
                     void *fn_dormbr);

/* ---- K1 + K3a : fused row mean, per-feature statistics, per-feature Gram -----------
 * Replaces np.average(x, axis=1) (:112), np.std(x) (:115), the materialised
 * X0 = (X - X_cnt)/X_scl (:169) and the X0^T X0 half of np.linalg.svd (:272).
 * Two calls on the same stream and workspace:
 *   spr_stats_gram_f64           the one read of X: d_rowmean[i] = mean_j X[i,j] for every
 *                                local row, per-workgroup Gram / Welford partials -> workspace;
 *   spr_stats_gram_finalize_f64  fixed-order reduction of the partials (bitwise reproducible,
 *                                no float atomics).  For every feature f over its LOCAL rows:
 *     d_fstats[3f..3f+2] = (count, mean, M2) of the row means (Welford/Chan form),
 *     d_gram[f*m*m ..]   = sum_i (x_i - mean_i)(x_i - mean_i)^T          (m x m, full).
 * The caller combines: var_f = (trace(G_f) + m*M2_f) / (count_f*m) -> X_scl; G = sum_f G_f/var_f.
 * Across ranks d_gram is summed (all-reduce) and d_fstats Chan-merged.
 * center = 1: as above.  center = 0: rows are taken as they are (d_rowmean is written as
 * zeros) -- the plain X^T X needed by ROM.decomposition(X0) on a caller-supplied X0 (:272).
 * Workspace: spr_stats_gram_workspace() bytes, 16-byte aligned.  m <= SPR_MAX_M. */
size_t spr_stats_gram_workspace(int32_t m, int32_t n_features);
int spr_stats_gram_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx,
                       int64_t row0, int64_t n_points, int32_t n_features, int32_t center,
                       double *d_rowmean, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_stats_gram_finalize_f64(int64_t n_rows, int32_t m, int64_t row0, int64_t n_points,
                                int32_t n_features, const void *d_workspace, size_t workspace_bytes,
                                double *d_fstats, double *d_gram, int32_t ldg, int32_t origin,
                                void *stream);
/* ldg / origin: the m x m block is written at (origin, origin) of per-feature ldg x ldg matrices
 * (ldg = m, origin = 0 for a stand-alone Gram).
 *
 * 256 < m <= 512 (column-split path, csrc/gram_wide.hip): columns A = [0,256), B = [256,m).
 *   spr_gram_cross_f64    A^T B and its transpose into ldg = m matrices.  center = 1: the means of the FULL rows are
 *                         formed in this pass (the panels hold whole rows) and WRITTEN to d_rowmean; run it first,
 *                         then spr_rowmean_stats_f64 for the per-feature statistics (count, mean, M2 of the row
 *                         means: reads the n means, not X).  center = 2: means READ from d_rowmean; 0: none;
 *   spr_rowstats_f64      (alternative to center = 1 above) row means of the full rows + per-feature statistics in a
 *                         separate read of X;
 *   spr_stats_gram_f64    on the slices (d_X, 256) and (d_X + 256, m - 256), ldx = full stride,
 *                         center = 2: the row means are READ from d_rowmean (no statistics; give
 *                         the finalize call a scratch d_fstats), finalize with ldg = m and
 *                         origin = 0 / 256. */
size_t spr_rowstats_workspace(int32_t n_features);
int spr_rowstats_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                     int64_t n_points, int32_t n_features, double *d_rowmean, double *d_fstats,
                     void *d_workspace, size_t workspace_bytes, void *stream);
size_t spr_gram_cross_workspace(int32_t m, int32_t n_features);
int spr_gram_cross_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                       int64_t n_points, int32_t n_features, int32_t center, double *d_rowmean,
                       double *d_gram, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_rowmean_stats_f64(const double *d_rowmean, int64_t n_rows, int64_t row0, int64_t n_points,
                          int32_t n_features, double *d_fstats, void *d_workspace, size_t workspace_bytes,
                          void *stream);   /* workspace: spr_rowstats_workspace(n_features) */
/* m > 512 (any snapshot count, :272 accepts any X0): the columns are cut into slices of 256 (the last one 1..256 wide);
 *   spr_rowstats_f64 first (row means of the full rows + feature statistics: one read of X), then, all with the row
 *   means READ from d_rowmean (centre mode 2; 0 for rows taken as they are),
 *   spr_stats_gram_f64 + finalize (ldg = m, origin = 256 i) on every slice i -> diagonal blocks,
 *   spr_gram_cross_pair_f64 on every pair i < j: A = the 256 columns at col_a = 256 i, B = the w_b columns at
 *   col_b = 256 j; block (col_a.., col_b..) and its mirror are written into the per-feature ldg x ldg matrices.
 *   Workspace of a pair: spr_gram_cross_workspace(256 + w_b, n_features). */
int spr_gram_cross_pair_f64(const double *d_X, int64_t n_rows, int32_t col_a, int32_t col_b, int32_t w_b,
                            int32_t ldg, int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features,
                            int32_t center, double *d_rowmean, double *d_gram, void *d_workspace,
                            size_t workspace_bytes, void *stream);

/* ---- K3b : device-side spectrum for m <= spr_spectrum_max_m() (= 64) ------------------------
 * Replaces, for small snapshot counts, the host eigen-solve behind np.linalg.svd (:272), the block
 * statistics merge (np.std :115 and the other scale_type formulas :117-161 that derive from block
 * mean / variance), A = (diag(S) Vt)^T (:273) and the explained variance (:274-275), so that fit()
 * needs no host synchronisation.  d_gram [F][m][m] and d_fstats_all [n_ranks][F][3] are the
 * (all-reduced / all-gathered) outputs of spr_stats_gram_finalize_f64.  scale_code: 0 'std',
 * 1 'none', 2 'pareto', 3 'vast', 4 'level', 5 'variance', 6 'poisson', 7 'l2-norm'.
 * Outputs: d_feat [F][5] = (count, block mean, block variance, scale, variance of the row-centred values =
 * trace(G_f) / (count m)); d_scale, d_inv_scale
 * [F]; d_lam, d_S, d_expvar [m] (descending); d_V [m][m] (columns = eigenvectors, largest-magnitude
 * entry positive); d_W = V_r S_r^-1 and d_Ar = V_r S_r [m][r]; d_info = (Jacobi sweeps, off^2, diag^2). */
int32_t spr_spectrum_max_m(void);
int spr_spectrum_f64(const double *d_gram, const double *d_fstats_all, int32_t n_ranks,
                     int32_t n_features, int32_t m, int32_t scale_code, int32_t r, double *d_feat,
                     double *d_scale, double *d_inv_scale, double *d_lam, double *d_S, double *d_expvar,
                     double *d_V, double *d_W, double *d_Ar, double *d_info, void *stream);

/* ---- K3a' : per-feature Gram blocks -> the scaled m x m Gram matrix --------------------
 * G = sum_f G_f / X_scl_f^2 is the Gram matrix of the reference's X0 = (X - X_cnt)/X_scl (:169) whose SVD :272 takes.
 * Inputs as for spr_spectrum_f64 (all-reduced d_gram [F][m][m], all-gathered d_fstats_all [n_ranks][F][3], scale_code
 * 0..7); outputs d_G [m][m], d_feat [F][5] = (count, block mean, block variance (:115), scale, variance of the
 * row-centred values), and the scales
 * d_scale / d_inv_scale [F] that the projection and reconstruction kernels read.  Replaces the host merge of fit():
 * one download of m^2 + 5 F doubles instead of F m^2, no upload. */
int spr_gram_combine_f64(const double *d_gram, const double *d_fstats_all, int32_t n_ranks,
                         int32_t n_features, int32_t m, int32_t scale_code, double *d_G, double *d_feat,
                         double *d_scale, double *d_inv_scale, void *stream);

/* ---- K1 + K3a for 256 < m <= 512 without a pass for the full-row means (np.average :112 + Gram half of :272) ----
 * The Gram matrix of row-centred data is P G_s P, P = I - 1 1^T / m, for the Gram matrix G_s of rows shifted by any
 * per-row constant.  The three launches of the wide path therefore all shift by the mean of the FIRST 256 columns, which
 * the first symmetric launch (spr_stats_gram_f64 on that slice, center = 1) forms anyway:
 *   spr_stats_gram_shifted_*   the symmetric pass on another column slice with the given shifts (centre mode 2) that also
 *                              writes the RAW row sums of its slice (d_rowsum[n_rows]);
 *   spr_gram_cross_*           center = 2 with the same shifts (no row sums);
 *   spr_gram_shift_finish_f64  d_rowmean <- (w_a d_rowmean + d_rowsum_b) / m (the means of the full rows) and
 *                              G_f <- P G_f P for the F matrices. */
int spr_stats_gram_shifted_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                               int64_t n_points, int32_t n_features, const double *d_shift, double *d_rowsum,
                               void *d_workspace, size_t workspace_bytes, void *stream);
int spr_gram_shift_finish_f64(double *d_rowmean, const double *d_rowsum_b, int64_t n_rows, int32_t w_a, int32_t m,
                              double *d_gram, int32_t n_features, void *stream);

/* ---- K4 : basis projection  Ur = X0 . W,  W = V_r Sigma_r^-1 (m x r) ----------------
 * Replaces the U factor of np.linalg.svd (:272) and the truncation U[:, :r] (:336).
 * Second read of X.  center = 1: d_rowmean (the row means written by spr_stats_gram_f64)
 * is removed in the epilogue as x.W - mean*(1^T W); the per-feature 1/X_scl
 * (d_inv_scale[n_features]) is applied there too, so X0 never exists.  center = 0:
 * rows are used as they are (d_rowmean may be NULL).  accumulate = 1 adds to d_Ur instead of
 * overwriting it: a wider X (m <= 512) is projected as two column slices, (d_X, d_W) and
 * (d_X + 256, d_W + 256 r), the second one accumulating. */
int spr_project_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx,
                    int64_t row0, int64_t n_points, int32_t n_features, int32_t center,
                    const double *d_inv_scale, const double *d_rowmean, const double *d_W, int32_t r,
                    double *d_Ur, int64_t ldu, int32_t accumulate, void *stream);

/* ---- K4s : the same projection for ANY snapshot count m (csrc/project_stream.hip) -----------------------------
 * Replaces the U factor of np.linalg.svd (:272) / U[:, :r] (:336) when W = V_r Sigma_r^-1 no longer fits a workgroup's
 * registers or LDS (m > 256; BASELINE config 5 has m = 512, r = 128).  ONE launch over the full contraction length:
 * W streams through LDS in k-chunks from a permuted image the call builds in the workspace, the accumulators live
 * across all chunks and d_Ur is written once (rounded once when it is float).  m is a run-time loop count -- no upper
 * bound; r <= SPR_MAX_R per call (the caller projects wider bases in column groups: d_W = the group's columns packed
 * m x r, d_Ur + column offset, same ldu).  center: 0 rows as they are, 1 row means removed in the epilogue
 * (x.W - mean (1^T W)), 2 row means subtracted from the operand before the multiplication (data whose mean dwarfs its
 * fluctuation).  Workspace: spr_project_stream_workspace(m, r, x_is_f32) bytes, 16-byte aligned. */
size_t spr_project_stream_workspace(int32_t m, int32_t r, int32_t x_is_f32);
int spr_project_stream_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                           int64_t n_points, int32_t n_features, int32_t center, const double *d_inv_scale,
                           const double *d_rowmean, const double *d_W, int32_t r, double *d_Ur, int64_t ldu,
                           void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- K4 + the first sweep of K6 : projection that also leaves the squared row norms of the basis ---------------
 * optimal_placement (:739) starts from |Ur[i, :]|^2 of every row; the plain route reads all of Ur once more for them
 * (spr_qr_init_*).  These variants write d_rownorm2[n_rows] -- the norms of the values AS STORED, i.e. rounded to the
 * basis type first -- from the accumulators of the projection that stores d_Ur, and spr_qr_init_norms_* starts the
 * pivoting from that vector (8 bytes per row instead of r values).  Same arguments and results otherwise.
 * spr_project_norms_*        only the W-stationary form produces norms (m = 64 / 128 / 192 / 256 packed rows, 16-byte aligned,
 *                            r <= 64, n_rows >= 4096): spr_project_norms_supported() says whether a shape qualifies;
 *                            SPR_E_UNSUPPORTED and nothing launched otherwise.
 * spr_project_stream_norms_* every shape spr_project_stream_* takes (any m, r <= SPR_MAX_R per call). */
int32_t spr_project_norms_supported(int32_t m, int32_t r, int64_t n_rows, int64_t ldx, const void *d_X,
                                    int32_t x_is_f32);
int spr_project_norms_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                          int64_t n_points, int32_t n_features, int32_t center, const double *d_inv_scale,
                          const double *d_rowmean, const double *d_W, int32_t r, double *d_Ur, int64_t ldu,
                          double *d_rownorm2, void *stream);
int spr_project_stream_norms_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                                 int64_t n_points, int32_t n_features, int32_t center, const double *d_inv_scale,
                                 const double *d_rowmean, const double *d_W, int32_t r, double *d_Ur, int64_t ldu,
                                 double *d_rownorm2, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- K4 + K10/K11 : projection that also emits the field of the next reconstruct() ---------------------------------
 * A step fit() -> reconstruct(a) reads all of Ur back from HBM only to form one dot product per row; the W-stationary
 * projection has each such row in its accumulators.  These variants also write
 *     d_Xrec[v * ldo + i] = d_scale[feature of i] * (Ur[i, :] . d_A[v, :]) + d_rowmean[i],   v < n_p <= spr_project_field_max(),
 * from the values of Ur AS STORED (rounded to the basis type first), with d_A n_p x r packed.  d_Ur -- and d_rownorm2,
 * when not NULL -- come out bit for bit as from spr_project_* / spr_project_norms_* on a shape those give to the same
 * kernel (spr_project_norms_supported()), and the field bit for bit as from spr_reconstruct_* on that d_Ur with the same
 * d_A: per row and lane one fused multiply-add per 16-column tile in ascending order, a butterfly sum over the 16 lanes,
 * one fused multiply-add for scale and centre (csrc/field_dot.hpp; spr_reconstruct_* runs the same function for
 * n_p <= spr_project_field_max() on bases of 16/32/48/64 columns with 16-byte-aligned rows and no d_rowscale).
 * The rows are always centred (center = 1 of spr_project_*).  Only the W-stationary form does this: SPR_E_UNSUPPORTED and
 * nothing launched for m other than 64/128/192/256 packed 16-byte-aligned rows, r other than 16/32/48/64 and
 * n_p > spr_project_field_max() -- the caller then makes the two calls.  Any n_rows.
 * Python layer: ROM.defer_project (default on; SPR_DEFER_PROJECT=0 switches it off) -- fit() RECORDS the projection of such
 * a shape, and the next call on the object launches it: reconstruct() with n_p <= spr_project_field_max() through these
 * entry points, anything else that needs the basis through spr_project_*.  Between fit() returning and that next call the
 * projection has NOT started.  The ABI version is unchanged: entry points were added, none changed. */
int32_t spr_project_field_max(void);
int spr_project_field_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                          int64_t n_points, int32_t n_features, const double *d_inv_scale, const double *d_rowmean,
                          const double *d_W, int32_t r, double *d_Ur, int64_t ldu, double *d_rownorm2,
                          const double *d_scale, const double *d_A, int32_t n_p, double *d_Xrec, int64_t ldo,
                          void *stream);

/* ---- K2 / K11 as stand-alone calls (ROM.scale_data's return value, ROM.unscale_data) --
 * spr_scale_rows:  X0 = (X - rowmean) * inv_scale[feature]   (:169), n_rows x m.
 * spr_unscale:     x  = scale[feature] * x0 + rowmean        (:235), n_rows; with d_rowscale != NULL
 *                  the per-row factor is used instead (the sampled form, :233). */
int spr_scale_rows_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                       int64_t n_points, int32_t n_features, const double *d_rowmean,
                       const double *d_inv_scale, double *d_X0, int64_t ldo, void *stream);
int spr_unscale_f64(const double *d_x0, int64_t n_rows, int64_t row0, int64_t n_points,
                    int32_t n_features, const double *d_rowmean, const double *d_scale,
                    const double *d_rowscale, double *d_x, void *stream);

/* ---- per-feature min / max of the raw block: np.max(x), np.min(x) of scale_type 'range' (:128)
 * and 'max' (:135).  d_minmax[2f] = min, [2f+1] = max over the LOCAL rows of feature f (+inf/-inf
 * when a feature has no local rows; ranks combine with min / max).  One extra read of X. */
size_t spr_feature_minmax_workspace(int32_t n_features);
int spr_feature_minmax_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                           int64_t n_points, int32_t n_features, double *d_minmax,
                           void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- per-feature order statistics of the raw block: np.median(x) of scale_type 'median' (:140-141).
 * Radix selection on order-preserving keys (key(x) = bits(x) ^ sign for x >= 0, ~bits(x) for x < 0): one call
 * counts, for every feature f with local rows and for two targets t (lower / upper middle element), the keys
 * whose bits above position shift+bits equal those of d_prefix[2f+t], by the `bits`-wide digit at position
 * `shift` (1 <= bits <= 13; shift + bits == 64 counts every key).  Counts are ADDED to
 * d_hist[f][t][1 << bits] (caller zeroes it; ranks sum them).  two_targets = 0 when both prefixes are equal
 * (one histogram is built and written to both halves).  Five calls (13+13+13+13+12 bits) pin down both keys;
 * the caller walks the cumulative counts between calls.  One read of X per call. */
int spr_feature_digit_hist_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                               int64_t n_points, int32_t n_features, const uint64_t *d_prefix, int32_t shift,
                               int32_t bits, int32_t two_targets, uint64_t *d_hist, void *stream);

/* ---- axis_cnt=None (np.average(x, axis=None), :112): scalar centre per feature ----------------
 * spr_colsums_f64: d_out[f][0][m] = sum_i (x_i - mean_i), d_out[f][1][m] = sum_i mean_i (x_i - mean_i)
 * over the LOCAL rows of feature f -- the two vectors that turn the row-centred Gram blocks into the
 * Gram blocks of (X - mu_f) (csrc/scale.hip).  One extra read of X, only for this option.
 * spr_fill_feature_f64: d_out[i] = d_values[feature of row i] (the new X_cnt column). */
size_t spr_colsums_workspace(int32_t m, int32_t n_features);
int spr_colsums_f64(const double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                    int64_t n_points, int32_t n_features, const double *d_rowmean, double *d_out,
                    void *d_workspace, size_t workspace_bytes, void *stream);
int spr_fill_feature_f64(double *d_out, int64_t n_rows, int64_t row0, int64_t n_points, int32_t n_features,
                         const double *d_values, void *stream);

/* ---- K10 + K11 : reconstruction  x = X_scl * (Ur a) + X_cnt -------------------------
 * Replaces Ur @ Ar.T (:371) and unscale_data (:235, :372-373) in one streaming pass.
 * d_A is n_p x r row-major (the Ar argument); output d_Xrec is COLUMN-major
 * (n_p columns of ldo >= n_rows doubles each). d_scale[n_features] = X_scl per feature;
 * d_rowscale (optional) = one factor per row instead, for reconstruct(sampling=S) (:365-368)
 * where the rows are S.Ur, the centre S.X_cnt and the factor S.X_scl. */
int spr_reconstruct_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu,
                        int64_t row0, int64_t n_points, int32_t n_features,
                        const double *d_rowmean, const double *d_scale, const double *d_rowscale,
                        const double *d_A, int32_t n_p, double *d_Xrec, int64_t ldo,
                        void *stream);
/* ---- bound sweep for train(method='COLS'): the rows of  lo0 <= Ur g <= hi0  a vector violates -------------
 * Replaces the n-sized scaled limits (:883, scale_limits :173-210) and the 2 n constraint rows handed to the conic
 * solver (:886, :889) by ONE streaming read of the basis block per round of the constraint-generation loop
 * (openmeasure_amd/_cols.py); nothing n-sized is written.
 * d_G is n_p x r row-major.  d_limits[2][n_features] = lower / upper limit per feature in physical units;
 * d_clamp[2][n_features] = NaN, or the constant (+-1000) the reference substitutes for the scaled limit of the whole
 * feature block (:201-204).  Scaled limit of row i of feature f:  (limit_f - d_rowmean[i]) / d_scale[f]  unless clamped.
 * Violation of a row:  v = max(x - hi0, lo0 - x),  x = Ur[i] . g,  in scaled units.
 * d_out[p][3 + 3 k] doubles per vector:  [0] max violation over the block (may be negative), [1] the lowest GLOBAL row
 * attaining it, [2] number of rows with v > tol, then k candidates (global row, side 0 = lower / 1 = upper, v) with
 * v > tol, worst first, ties to the lower row; unused entries are (-1, 0, -inf).  Candidates are the worst row per side
 * of every workgroup's contiguous run of rows, so they are spread over the block; the first one is the global worst.
 * Deterministic for a fixed device (no atomics).  r <= SPR_MAX_R_WIDE, 0 < k <= 256, tol >= 0. */
size_t spr_bound_sweep_workspace(int32_t n_p, int32_t n_features);
int spr_bound_sweep_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                        int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_limits,
                        const double *d_clamp, const double *d_G, int32_t n_p, double tol, int32_t k, double *d_out,
                        void *d_workspace, size_t workspace_bytes, void *stream);
int spr_bound_sweep_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                        int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_limits,
                        const double *d_clamp, const double *d_G, int32_t n_p, double tol, int32_t k, double *d_out,
                        void *d_workspace, size_t workspace_bytes, void *stream);
/* Batched form for ROM.CPOD (openmeasure_amd/_cpod.py), which sweeps all m snapshots every round: same arguments, same
 * records, but 64 vectors stay resident per read of the basis block (r <= SPR_MAX_R and n_rows < 2^31; anything else runs
 * the kernels of spr_bound_sweep_*).  The candidates are those of ITS grid: a different, equally valid spread. */
size_t spr_bound_sweep_batch_workspace(int32_t n_p, int32_t n_features);
int spr_bound_sweep_batch_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                              int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_limits,
                              const double *d_clamp, const double *d_G, int32_t n_p, double tol, int32_t k, double *d_out,
                              void *d_workspace, size_t workspace_bytes, void *stream);
int spr_bound_sweep_batch_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                              int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_limits,
                              const double *d_clamp, const double *d_G, int32_t n_p, double tol, int32_t k, double *d_out,
                              void *d_workspace, size_t workspace_bytes, void *stream);
/* ---- held-out snapshots: ROM.transform / ROM.reconstruction_error (csrc/validate.hip) -----------------------
 * spr_encode_*: d_A[j][c] = sum_i X0_new[i][j] * Ur[i][c],  X0_new[i][j] = (X_new[i][j] - d_rowmean[i]) / d_scale[f(i)],
 * over the block's rows.  Replaces the user-side  Ur.T @ ((x - X_cnt) / X_scl)  of the reference's notebooks
 * (docs/sparse_sensing_doc.ipynb; the A_new its GPR.update(P_new, A_new) takes, gpr.py:603), for which the whole basis
 * had to be downloaded.  d_X is n_rows x k row-major with row stride ldx (the layout of X); d_A is k x r row-major, f64
 * (the orientation of Ar and of what spr_reconstruct_* takes).  The centring and the division are applied per element,
 * in the host's order; the products are summed on the f64 MFMA with the rows of a 64-row panel as the contraction index.
 * Every workgroup leaves its partial block in the workspace and a second kernel adds them in a fixed order: no atomics,
 * two runs on one device agree bit for bit.  k is cut into slices of 64 columns (one read of the basis block each);
 * r > SPR_MAX_R runs per 128-column group of the basis (one read of X_new each), r <= SPR_MAX_R_WIDE.
 * A sharded caller sums the ranks' d_A.
 * Suffixes: _x32 = X_new stored as f32, _u32 = basis stored as f32, _x32_u32 = both; arithmetic is f64 throughout. */
size_t spr_encode_workspace(int32_t r, int32_t k, int32_t n_features);
int spr_encode_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const double *d_X, int32_t k, int64_t ldx,
                   int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale,
                   double *d_A, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_encode_x32(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const float *d_X, int32_t k, int64_t ldx,
                   int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale,
                   double *d_A, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_encode_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const double *d_X, int32_t k, int64_t ldx,
                   int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale,
                   double *d_A, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_encode_x32_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const float *d_X, int32_t k, int64_t ldx,
                       int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale,
                       double *d_A, void *d_workspace, size_t workspace_bytes, void *stream);
/* spr_field_error_*: the pass of spr_reconstruct_* with a comparison in place of the store.  Replaces reconstruct
 * (Ur @ Ar.T and unscale_data, :371-375), the copy of the n x k field to the host and the NumPy norms taken there.
 * d_A is k x r row-major, d_Xtrue n_rows x k row-major with row stride ldx, in physical units.  Per row
 * x = d_scale[f] * (Ur[i] . a_j) + d_rowmean[i] as spr_reconstruct_* forms it and d = x - X_true[i][j];
 * d_out[j][f][4] doubles per (vector, feature) over the block's rows:  sum d^2, sum X_true^2, max |d|, the lowest GLOBAL
 * row attaining that maximum (-1, with zeros in front, when the block holds no row of the feature).
 * Per-workgroup slots in the workspace and a merge kernel: no atomics, deterministic.  r <= SPR_MAX_R_WIDE.
 * A sharded caller adds the sums and merges the maxima (lowest row on a tie).  Suffixes as for spr_encode_*. */
size_t spr_field_error_workspace(int32_t k, int32_t n_features);
int spr_field_error_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                        int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_A, int32_t k,
                        const double *d_Xtrue, int64_t ldx, double *d_out, void *d_workspace, size_t workspace_bytes,
                        void *stream);
int spr_field_error_x32(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                        int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_A, int32_t k,
                        const float *d_Xtrue, int64_t ldx, double *d_out, void *d_workspace, size_t workspace_bytes,
                        void *stream);
int spr_field_error_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                        int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_A, int32_t k,
                        const double *d_Xtrue, int64_t ldx, double *d_out, void *d_workspace, size_t workspace_bytes,
                        void *stream);
int spr_field_error_x32_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                            int32_t n_features, const double *d_rowmean, const double *d_scale, const double *d_A, int32_t k,
                            const float *d_Xtrue, int64_t ldx, double *d_out, void *d_workspace, size_t workspace_bytes,
                            void *stream);
/* ---- gappy POD: ROM.gappy_transform (csrc/gappy.hip) -----------------------------------------------------------
 * The normal equations of the least-squares fit of masked snapshots in the basis,  a = (Ur^T M Ur)^+ Ur^T M x0,  over the
 * block's rows, in one streaming pass over the basis block and d_X:
 *   d_H[c][d] = sum_i m_i Ur[i][c] Ur[i][d]     r x r row-major, exactly symmetric
 *   d_B[j][c] = sum_i m_i X0[i][j] Ur[i][c]     k x r row-major (the orientation of Ar),  X0 as spr_encode_* forms it
 *   d_nobs[0] = sum_i m_i                       one double, exact
 * m_i = (d_mask[i * ldm] != 0): ONE mask column for all k columns of the call (a column of an n x k row-major mask is
 * passed with ldm = k).  Replaces the user-side  np.linalg.lstsq(Ur[m], x0[m])  for which the basis had to be downloaded,
 * and the train(C) + predict(y) route whose Theta = C Ur has one row per observed cell.
 * A masked-out element is selected away, never multiplied by zero: NaN / Inf / garbage in an unobserved row of d_X reaches
 * no output; a NaN in an observed row makes row j of d_B NaN and nothing else.  A 64-row panel without an observed row is
 * skipped before its basis and X rows are requested (the mask bytes are read first).  Per-workgroup slots in the
 * workspace and a second kernel that adds them in a fixed order: no atomics, two runs on one device agree bit for bit.
 * k is cut into slices of 64 columns (one read of the basis block each; H and nobs come from the first).
 * r <= SPR_MAX_R: a larger r returns SPR_E_INVALID and launches nothing.  A sharded caller sums the ranks' outputs.
 * Suffixes as for spr_encode_*. */
size_t spr_gappy_normal_workspace(int32_t r, int32_t k, int32_t n_features);
int spr_gappy_normal_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const double *d_X, int32_t k,
                         int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                         const double *d_scale, const uint8_t *d_mask, int64_t ldm, double *d_H, double *d_B,
                         double *d_nobs, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_gappy_normal_x32(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const float *d_X, int32_t k,
                         int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                         const double *d_scale, const uint8_t *d_mask, int64_t ldm, double *d_H, double *d_B,
                         double *d_nobs, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_gappy_normal_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const double *d_X, int32_t k,
                         int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                         const double *d_scale, const uint8_t *d_mask, int64_t ldm, double *d_H, double *d_B,
                         double *d_nobs, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_gappy_normal_x32_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const float *d_X, int32_t k,
                             int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                             const double *d_scale, const uint8_t *d_mask, int64_t ldm, double *d_H, double *d_B,
                             double *d_nobs, void *d_workspace, size_t workspace_bytes, void *stream);
/* ---- incremental POD: ROM.partial_fit (csrc/update.hip) -----------------------------------------------------------
 * The two passes of the block incremental SVD (Brand 2002 / 2006; the rank-k update behind scikit-learn's
 * IncrementalPCA) over the basis block d_Ur (n_rows x r, f64, orthonormal) and a batch d_X (n_rows x k row-major with row
 * stride ldx, k <= 64), X0 = (X - d_rowmean) / d_scale[f] as spr_encode_* forms it, never stored.  The small algebra
 * between them is the caller's (openmeasure_amd/_update.py).
 *
 * spr_subspace_residual_*: with d_C (k x r row-major, what spr_encode_* wrote for this batch) and E = X0 - Ur C^T
 *   d_H[a][b]  = sum_i E[i][a] E[i][b]       k x k row-major, symmetric bit for bit
 *   d_C2[j][c] = sum_i E[i][j] Ur[i][c]      k x r row-major: what the held basis has lost of its orthonormality
 *   d_ss[0]    = sum_ij X0[i][j]^2           non-finite when the batch holds a NaN / Inf
 * Replaces the host-side  E = X0 - U (U^T X0); np.linalg.qr(E)  of the update, for which the basis and the batch would be
 * downloaded.  E is formed per 64-row panel in LDS on the f64 MFMA and never written to HBM; H comes from E itself, not
 * from X0^T X0 - C C^T.  Per-workgroup slots in the workspace and a second kernel that adds them in a fixed order: no
 * atomics, two runs on one device agree bit for bit.  A sharded caller would sum the ranks' outputs.
 *
 * spr_basis_update_*: d_out[i][0 .. r2) = sum_c Ur[i][c] d_A[c][.] + sum_j X0[i][j] d_B[j][.]  with d_A r x r2 and d_B
 *   k x r2 row-major, packed.  Replaces  U_new = np.hstack([U, Q]) @ P  on the host.  One pass; d_out (row stride
 *   ldo >= r2) is another buffer than d_Ur; its columns beyond r2 are not written.  k = 0 is a pure rotation (d_X, d_B
 *   unused, may be NULL).
 *
 * Refusals, in this order, nothing launched after one: a NULL pointer, a shape that is not positive (k < 0 here) or a
 * leading dimension below its width, the feature layout (all SPR_E_INVALID); r > SPR_MAX_R, k > 64 (SPR_E_UNSUPPORTED);
 * then for the residual k = 0 and the workspace (SPR_E_INVALID), for the update r2 < 1 (SPR_E_INVALID), r2 > SPR_MAX_R
 * (SPR_E_UNSUPPORTED), ldo < r2, d_out == d_Ur (SPR_E_INVALID).  An f32-stored basis has no entry: its columns are
 * orthonormal to f32 rounding only.  Suffix _x32 = d_X stored as f32; arithmetic is f64 throughout. */
size_t spr_subspace_residual_workspace(int32_t r, int32_t k, int32_t n_features);
int spr_subspace_residual_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const double *d_X, int32_t k,
                              int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                              const double *d_scale, const double *d_C, double *d_H, double *d_C2, double *d_ss,
                              void *d_workspace, size_t workspace_bytes, void *stream);
int spr_subspace_residual_x32(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const float *d_X, int32_t k,
                              int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                              const double *d_scale, const double *d_C, double *d_H, double *d_C2, double *d_ss,
                              void *d_workspace, size_t workspace_bytes, void *stream);
int spr_basis_update_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const double *d_X, int32_t k,
                         int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                         const double *d_scale, const double *d_A, const double *d_B, int32_t r2, double *d_out,
                         int64_t ldo, void *stream);
int spr_basis_update_x32(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, const float *d_X, int32_t k,
                         int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                         const double *d_scale, const double *d_A, const double *d_B, int32_t r2, double *d_out,
                         int64_t ldo, void *stream);
/* ---- POD from incomplete snapshots: ROM.fit_gappy (csrc/gappy_fill.hip) -----------------------------------------
 * The two passes that write into the holes of the snapshot block d_X (n_rows x m, row stride ldx) IN PLACE.  d_mask is
 * n_rows x m bytes with row stride ldm >= m, non-zero = observed; the other entries are holes.  An observed entry of d_X is
 * never written and never enters a sum of the fill pass: its bytes stay identical.  Per-workgroup slots in the workspace
 * (spr_gappy_fill_workspace() bytes, for both calls) and a second kernel that combines them in a fixed order: no atomics,
 * two runs on one device agree bit for bit.  Replaces the host loop "reconstruct, download, overwrite the holes, upload".
 *
 * spr_gappy_rowfill_*: every hole gets the mean of the observed entries of its row (formed in f64, rounded once for an
 * f32 block).  d_out (8 doubles, exact integers):
 *   [0] holes of the block   [1] rows without an observed entry   [2] the lowest such GLOBAL row (row0 + i; -1: none)
 *   [3] observed entries that are not finite   [4] the lowest global row holding one (-1: none)   [5..7] 0
 * Two sweeps: the first only reads (mask and observed entries) and forms d_out; the second writes the means and leaves
 * at once when d_out[1] or d_out[3] is non-zero -- a block with a bad row is not modified at all.
 *
 * spr_gappy_fill_*: every hole (i, j) gets  d_scale[f(i)] * (Ur[i] . A[j]) + d_rowmean[i]  -- what spr_reconstruct_* puts
 * there for the rows of d_A (m x r row-major, f64) -- all arithmetic in f64, a value stored to an f32 block rounded once.
 *   d_out[0] = S_d = sum over holes (new - old)^2     d_out[1] = S_n = sum over holes new^2      (new as stored)
 * The old value of a hole enters S_d: a NaN there makes S_d NaN (the hole itself is overwritten with the finite value).
 * The mask bytes of a 64-row panel are read first; a panel without a hole is left before any of its basis or X rows is
 * requested.  d_A is staged in LDS in slices of min(256, 8192 / r) columns, slices outermost: every mask byte is read
 * once, the basis row of a row with holes once per slice in which it has one, every hole is read once and written once.
 * The dot products run per hole on the vector pipe (four holes per wave step).  Any m >= 1.  r <= SPR_MAX_R: a larger r
 * returns SPR_E_UNSUPPORTED and launches nothing.  Suffixes as for spr_encode_*. */
size_t spr_gappy_fill_workspace(void);
int spr_gappy_rowfill_f64(double *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0, const uint8_t *d_mask,
                          int64_t ldm, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_gappy_rowfill_x32(float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0, const uint8_t *d_mask,
                          int64_t ldm, double *d_out, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_gappy_fill_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, double *d_X, int32_t m, int64_t ldx,
                       int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale,
                       const double *d_A, const uint8_t *d_mask, int64_t ldm, double *d_out, void *d_workspace,
                       size_t workspace_bytes, void *stream);
int spr_gappy_fill_x32(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, float *d_X, int32_t m, int64_t ldx,
                       int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale,
                       const double *d_A, const uint8_t *d_mask, int64_t ldm, double *d_out, void *d_workspace,
                       size_t workspace_bytes, void *stream);
int spr_gappy_fill_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, double *d_X, int32_t m, int64_t ldx,
                       int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean, const double *d_scale,
                       const double *d_A, const uint8_t *d_mask, int64_t ldm, double *d_out, void *d_workspace,
                       size_t workspace_bytes, void *stream);
int spr_gappy_fill_x32_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, float *d_X, int32_t m, int64_t ldx,
                           int64_t row0, int64_t n_points, int32_t n_features, const double *d_rowmean,
                           const double *d_scale, const double *d_A, const uint8_t *d_mask, int64_t ldm, double *d_out,
                           void *d_workspace, size_t workspace_bytes, void *stream);
/* ---- field uncertainty: ROM.reconstruct_std (csrc/field_std.hip) -------------------------------------------------
 * Per-cell standard deviation of the reconstructed field for Gaussian coefficient uncertainty, propagated linearly
 * through  x = X_scl (Ur a) + X_cnt.  Replaces the download of the basis and the host-side
 * X_scl * sqrt((Ur**2) @ sigma**2)  or  sqrt(diag(Ur Sigma Ur^T))  users had to write after predict().
 * Output as spr_reconstruct_*: COLUMN-major, k columns of ldo >= n_rows doubles, d_out[j * ldo + i] for local row i;
 * s_i = d_scale[feature of row i], or d_rowscale[i] when that pointer is non-NULL.
 * spr_field_std_diag_*:   d_out[j][i] = s_i sqrt( sum_c Ur[i][c]^2 d_S[j][c]^2 ).  d_S is k x r row-major: independent
 *   per-coefficient standard deviations, the orientation of Ar_sigma (signs do not matter, the kernel squares).
 *   One read of the basis block per 16 vectors; r <= SPR_MAX_R_WIDE (r > SPR_MAX_R per 128-column group, the partial
 *   variance waiting in d_out between the groups).
 * spr_field_std_factor_*: d_out[j][i] = s_i || L_j^T u_i ||_2,  u_i = row i of the basis.  d_L is k x r x q contiguous:
 *   factors of the coefficient covariances, Sigma_j = L_j L_j^T, 1 <= q <= r.  One read of the basis block for all k
 *   vectors; 2 n r q k flops on the f64 MFMA.  r <= SPR_MAX_R: a larger r returns SPR_E_INVALID and launches nothing.
 * No workspace, no atomics: two runs on one device agree bit for bit.  A NaN row of d_S / factor of d_L gives a NaN
 * column j and nothing else; a zero variance gives exactly 0.  Suffix _u32 = basis stored as f32 (widened exactly). */
int spr_field_std_diag_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                           int32_t n_features, const double *d_scale, const double *d_rowscale, const double *d_S,
                           int32_t k, double *d_out, int64_t ldo, void *stream);
int spr_field_std_diag_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                           int32_t n_features, const double *d_scale, const double *d_rowscale, const double *d_S,
                           int32_t k, double *d_out, int64_t ldo, void *stream);
int spr_field_std_factor_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                             int32_t n_features, const double *d_scale, const double *d_rowscale, const double *d_L,
                             int32_t k, int32_t q, double *d_out, int64_t ldo, void *stream);
int spr_field_std_factor_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                             int32_t n_features, const double *d_scale, const double *d_rowscale, const double *d_L,
                             int32_t k, int32_t q, double *d_out, int64_t ldo, void *stream);
/* ---- sequential optimal design: SPR.augment_placement / placement_gain (csrc/design.hip) ---------------------------
 * The score of every local row of the basis as the NEXT sensor, given d_B = M^-1 (r x r row-major, SYMMETRIC: the kernel
 * multiplies by its transpose), M the information matrix of the sensors placed so far.  For row u with weight w:
 * z = B u, d = u^T z, q = z^T z;  criterion 0 (D): w d  (the gain of log det M is log(1 + w d));  criterion 1 (A):
 * w q / (1 + w d), the drop of trace M^-1.  One streaming read of the basis block, 2 n r^2 flops on the f64 MFMA.
 * d_wfeat: n_features weights (the feature of a row from row0 / n_points), NULL = all ones.  d_alive: one double per
 * local row, NULL = all rows; a row whose entry is negative is out of the race (the convention of the pivoting state's
 * norms, so spr_qr_exclude_f64 maintains it).  d_scores: NULL, or n_rows doubles that receive every row's score (-inf
 * for rows that are out).  d_rec: r + 3 doubles -- best score, its GLOBAL row (lowest row on a tie), the runner-up's
 * score (second-largest score over all other rows), the r entries of the winning row of the basis: the layout of the
 * pivoting record.  No row alive: score -inf, row -1, zeros.  A NaN score never wins.  r <= SPR_MAX_R (larger:
 * SPR_E_UNSUPPORTED).  Workspace: spr_design_sweep_workspace bytes (0 for arguments the sweep refuses).  No atomics: two
 * runs on one device agree bit for bit.  Suffix _u32 = basis stored as f32 (widened exactly). */
size_t spr_design_sweep_workspace(int32_t r, int32_t n_features);
int spr_design_sweep_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                         int32_t n_features, const double *d_B, const double *d_wfeat, const double *d_alive,
                         int32_t criterion, double *d_scores, double *d_rec, void *d_workspace, size_t workspace_bytes,
                         void *stream);
int spr_design_sweep_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0, int64_t n_points,
                         int32_t n_features, const double *d_B, const double *d_wfeat, const double *d_alive,
                         int32_t criterion, double *d_scores, double *d_rec, void *d_workspace, size_t workspace_bytes,
                         void *stream);
/* ---- exact Gaussian processes on the POD coefficients: GPR.train / predict / update (csrc/gp.hip) -----------------------
 * r independent GPs over the same m points d_P0 (m x d row-major, row stride ldp >= d), targets the columns of d_Y
 * (m x r, row stride ldy >= r).  Per mode q, d_raw[3q .. 3q+2] = (raw_l, raw_n, mu):  l = softplus(raw_l),
 * s2 = softplus(raw_n) + 1e-4,  K = k(D / l) + s2 I with D the Euclidean distances of d_P0 clamped below at 1e-15,
 * loss = [ (y - mu)^T K^-1 (y - mu) / 2 + log det K / 2 + (m / 2) log 2 pi ] / m.  kernel: SPR_GP_* below, one shared
 * lengthscale, no output scale.
 * spr_gp_train_f64: Adam (beta 0.9 / 0.999, eps 1e-8, bias correction, step lr) on the three values, at most max_iter
 *   evaluations; after each one e = |loss - previous loss| (1e10 before the first), the step is taken, and the mode stops
 *   when e <= tol.  d_raw is updated in place; d_Kinv (r x m x m) and d_alpha (r x m) receive K^-1 and K^-1 (y - mu) AT THE
 *   PARAMETERS LEFT IN d_raw (one more factorisation after the last step).  max_iter = 0: factor at the given d_raw, no
 *   step.  d_info (r x 8): [0] evaluations that were followed by a step, [1] loss and [4..6] gradient (raw_l, raw_n, mu) of
 *   the last of them (max_iter = 0: of the factorisation), [2] its e, [3] status: 0 ok, 1 a pivot <= 0, 2 a pivot that is
 *   not finite (the mode stops there; its d_Kinv / d_alpha rows are undefined), [7] 0.  d_trace: NULL, or r x max_iter x 4
 *   doubles: (loss, raw_l, raw_n, mu) of every evaluation that was followed by a step.  One workgroup per mode, the whole
 *   loop in one launch, no atomics: two runs agree bit for bit.  m <= SPR_GP_MAX_M (SPR_E_UNSUPPORTED beyond);
 *   workspace: spr_gp_workspace(m, r) bytes (0 for shapes that are refused), 8-byte aligned.
 * spr_gp_predict_f64: d_Pstar (n_p x d, row stride ldps >= d) -> d_mean, d_var (n_p x r row-major):
 *   mean = mu + k*^T alpha,  var = max(1 - k*^T K^-1 k*, 0) + s2  (k(0) = 1 for every kernel here). */
#define SPR_GP_MAX_M 800
#define SPR_GP_MATERN52 0
#define SPR_GP_MATERN32 1
#define SPR_GP_MATERN12 2
#define SPR_GP_RBF 3
size_t spr_gp_workspace(int32_t m, int32_t r);
int spr_gp_train_f64(const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy,
                     int32_t kernel, double *d_raw, double lr, int32_t max_iter, double tol, double *d_Kinv, double *d_alpha,
                     double *d_info, double *d_trace, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_gp_predict_f64(const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Pstar, int32_t n_p,
                       int64_t ldps, int32_t kernel, const double *d_raw, int32_t r, const double *d_Kinv,
                       const double *d_alpha, double *d_mean, double *d_var, void *stream);
/* The same GPs with one lengthscale per coordinate (ARD, flags bit 0) and / or an output scale (flags bit 1).  L = d with ARD,
 * else 1; S = 1 with the scale, else 0; n_par = L + S + 2.  Per mode q, d_raw[n_par q ..] = (raw_l[0..L-1], [raw_o], raw_n, mu):
 * l_c = softplus(raw_l[c]) (l_0 for every c without ARD), o = softplus(raw_o) or 1, s2 = softplus(raw_n) + 1e-4,
 * z_i = P0[i, :] / l coordinate by coordinate, t_ij = max(|z_i - z_j|_2, 1e-15), K = o k(t) + s2 I, the loss as above.
 * spr_gp_train_ard_f64: the loop of spr_gp_train_f64 over the n_par values.  d_raw is r x n_par; d_info is r x (4 + n_par):
 *   evaluations, loss, e, status, then the gradient in the order of d_raw; d_trace is NULL or r x max_iter x (1 + n_par):
 *   (loss, raw).  flags = 0 is the model of spr_gp_train_f64 (same numbers to rounding, not bit for bit: the distances are
 *   formed from scaled coordinates).  m <= SPR_GP_MAX_M, and d <= SPR_GP_MAX_D with ARD (SPR_E_UNSUPPORTED beyond);
 *   workspace: spr_gp_workspace_ard(m, d, r) = 8 r (2 m^2 + m d) bytes (0 for shapes that are refused), 8-byte aligned.
 * spr_gp_predict_ard_f64: mean = mu + o k*^T alpha,  var = max(o - o^2 k*^T K^-1 k*, 0) + s2. */
#define SPR_GP_MAX_D 8
#define SPR_GP_FLAG_ARD 1
#define SPR_GP_FLAG_SCALE 2
size_t spr_gp_workspace_ard(int32_t m, int32_t d, int32_t r);
int spr_gp_train_ard_f64(const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy,
                         int32_t kernel, int32_t flags, double *d_raw, double lr, int32_t max_iter, double tol,
                         double *d_Kinv, double *d_alpha, double *d_info, double *d_trace, void *d_workspace,
                         size_t workspace_bytes, void *stream);
int spr_gp_predict_ard_f64(const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Pstar, int32_t n_p,
                           int64_t ldps, int32_t kernel, int32_t flags, const double *d_raw, int32_t r, const double *d_Kinv,
                           const double *d_alpha, double *d_mean, double *d_var, void *stream);
/* The same GPs with a noise per point (GPR.update(fixed_noise=True / retrain=True)): for mode q, n_i = w_i s2 + V[i, q] and
 * K = o k(t) + diag(n); the loss as above; d loss / d raw_n = sigmoid(raw_n) sum_i w_i (K^-1_ii - alpha_i^2) / 2m, the other
 * gradient components unchanged in form.  d_w: m doubles, 1 for a point that carries the learned noise s2, 0 for a point whose
 * variance is given; d_V: m x r, row stride ldv >= r, >= 0, the given variances in the units of d_Y^2 (column q for mode q).
 * spr_gp_train_noise_f64 is spr_gp_train_ard_f64 with these two arrays, for flags 0..3 (flags = 0: raw = (raw_l, raw_n, mu),
 *   n_par = 3): the same d_raw / d_info / d_trace layouts, Adam loop, stopping rule, status codes, caps and workspace
 *   (spr_gp_workspace_ard), no atomics, two runs agree bit for bit.  With w = 1 and V = 0 it returns the bits of
 *   spr_gp_train_ard_f64.  The predict entry points take its d_Kinv / d_alpha as they are; they add s2, not V, at the test point. */
int spr_gp_train_noise_f64(const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy,
                           const double *d_w, const double *d_V, int64_t ldv, int32_t kernel, int32_t flags, double *d_raw,
                           double lr, int32_t max_iter, double tol, double *d_Kinv, double *d_alpha, double *d_info,
                           double *d_trace, void *d_workspace, size_t workspace_bytes, void *stream);
/* Accumulating data without factoring again (GPR.update(append=True)): beside K^-1 the state keeps X = L^-1 (K = L L^T, row-major,
 * strict upper triangle zero) and log det K, and k new rows are appended to X in O(m^2 k) per mode.
 * spr_gp_state_f64: the arguments and the numbers of spr_gp_train_noise_f64 with max_iter = 0 (no lr / max_iter / tol / trace): it is
 *   that launch, d_Kinv, d_alpha and d_info (r x (4 + n_par)) receive the same bits and d_raw is rewritten with the values it holds.
 *   A second launch copies X out of the workspace to d_X (r x m x m) and sums d_logdet (r) = 2 sum_j log L_jj in a fixed order (NaN
 *   and an undefined d_X for a mode whose status is not 0).  Workspace: spr_gp_workspace_ard.
 * spr_gp_append_f64: d_P0 / d_Y / d_w / d_V hold m_new = m + k rows, the last k of them new (1 <= k <= SPR_GP_MAX_APPEND, m >= 1,
 *   m_new <= SPR_GP_MAX_M; SPR_E_UNSUPPORTED beyond either cap); d_X, d_Kinv (r x m x m) and d_logdet (r) are the state of the first m
 *   rows at d_raw and are never written.  With K' = [[K, B], [B^T, C]], C including the new points' noise w_i s2 + V[i, q]:
 *   W = X B,  S = C - W^T W = Ls Ls^T,  Z = Ls^-1 W^T X,  X' = [[X, 0], [-Z, Ls^-1]],  K'^-1 = [[K^-1, 0], [0, 0]] + N^T N with
 *   N = [-Z, Ls^-1] -- the terms X'^T X' adds to X^T X; K^-1 is not updated through its own Schur complement --, logdet' = logdet +
 *   sum log(pivots of S), alpha' = K'^-1 (y' - mu), the loss as above.  B and C come from the scaled coordinates z = P0 / l, as in
 *   spr_gp_train_ard_f64 (flags = 0: the numbers of the distance-matrix route of spr_gp_train_f64 to rounding).  Outputs, out of
 *   place: d_X2, d_Kinv2 (r x m_new x m_new; the old block of d_X2 is a copy, K'^-1 is symmetric bit for bit), d_alpha2
 *   (r x m_new), d_logdet2 (r), d_info (r x 4): m_new, loss, logdet', status -- 0 ok, 1 a pivot of S that is <= m_new 2^-53 C_jj (not
 *   positive to working precision: it is what a cancellation of that size leaves of C_jj), 2 a pivot that is not finite; such a mode's rows of the other outputs are undefined, the other modes are not affected.  Three launches in stream
 *   order, no atomics, no workgroup waits for another; two runs agree bit for bit.  Workspace: spr_gp_workspace_append(m_new, d, k, r)
 *   = 8 r m_new (d + 2 k) bytes (0 for shapes that are refused), 8-byte aligned. */
#define SPR_GP_MAX_APPEND 64
int spr_gp_state_f64(const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy,
                     const double *d_w, const double *d_V, int64_t ldv, int32_t kernel, int32_t flags, double *d_raw,
                     double *d_Kinv, double *d_alpha, double *d_info, double *d_X, double *d_logdet, void *d_workspace,
                     size_t workspace_bytes, void *stream);
size_t spr_gp_workspace_append(int32_t m_new, int32_t d, int32_t k, int32_t r);
int spr_gp_append_f64(const double *d_P0, int32_t m_new, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy,
                      const double *d_w, const double *d_V, int64_t ldv, int32_t k, int32_t kernel, int32_t flags,
                      const double *d_raw, const double *d_X, const double *d_Kinv, const double *d_logdet, double *d_X2,
                      double *d_Kinv2, double *d_alpha2, double *d_logdet2, double *d_info, void *d_workspace,
                      size_t workspace_bytes, void *stream);
/* Jointly trained GPs with a shared noise (GPR(gpr_type='MultiTask')): the model of spr_gp_train_ard_f64 per mode q, for flags
 * 0..3 and the same d_raw layout (r x n_par, its noise entry raw_t the TASK noise), plus ONE shared value d_raw_g[0]:
 *   s2_q = (softplus(raw_t_q) + 1e-4) + (softplus(raw_g) + 1e-4),  K_q = o_q k(t) + s2_q I,  loss_q as above,
 *   LOSS = (1 / r) sum_q loss_q;  d LOSS / d (own parameter of q) = the single-task expression / r,
 *   d LOSS / d raw_g = sigmoid(raw_g) (1 / r) sum_q sum_i (K_q^-1_ii - alpha_qi^2) / 2m.
 * spr_gp_train_mt_f64: ONE Adam loop (beta 0.9 / 0.999, eps 1e-8, bias correction, step lr) over the NP = r n_par + 1 values with
 *   the loop of spr_gp_train_f64 on LOSS: evaluate, e = |LOSS - previous LOSS| (1e10 before the first), step, stop when e <= tol
 *   or after max_iter evaluations, then one more evaluation at the parameters kept; max_iter = 0: that evaluation alone.  d_raw and
 *   d_raw_g are updated in place; d_s2 (r) receives the s2_q that evaluation used, d_Kinv (r x m x m) and d_alpha (r x m) its K^-1
 *   and alpha.  d_info (4 + NP + r): [0] evaluations that were followed by a step, [1] LOSS of the final evaluation, [2] e of the
 *   last step (NaN with max_iter = 0), [3] the largest per-mode status, [4 .. 4 + NP) the gradient of LOSS at the final evaluation
 *   in the order (d_raw, raw_g), then the r per-mode statuses (0 ok, 1 a pivot <= 0, 2 a pivot that is not finite).  A failed
 *   pivot in any mode ends the loop there: the parameters stay those of that evaluation, [1] and the gradient are those of the
 *   last step before it, and d_Kinv / d_alpha of that mode are undefined.  d_trace: NULL, or max_iter x (1 + NP) doubles:
 *   (LOSS, d_raw, raw_g) of every evaluation that was followed by a step.  The loop is a chain of launches on `stream`, one
 *   workgroup per mode to evaluate and one workgroup to sum and step, driven by a phase word on the device; SPR_GP_MT_CHUNK
 *   pairs are enqueued at a time and the call WAITS for the stream after each chunk to read that word (launches behind the stop
 *   change nothing).  No atomics, no workgroup waits for another; two runs agree bit for bit, whatever the chunking.  With
 *   max_iter = 0, d_Kinv, d_alpha and loss_q are the bits of spr_gp_train_noise_f64 with w = 1, V = softplus(raw_g) + 1e-4.
 *   m <= SPR_GP_MAX_M, d <= SPR_GP_MAX_D with ARD (SPR_E_UNSUPPORTED beyond); workspace: spr_gp_workspace_mt(m, d, r) bytes
 *   (spr_gp_workspace_ard plus the loop's state; 0 for shapes that are refused), 8-byte aligned.
 * spr_gp_predict_mt_f64: spr_gp_predict_ard_f64 with s2 read from d_s2 (r) as stored, not recomputed from d_raw. */
#define SPR_GP_MT_CHUNK 16
size_t spr_gp_workspace_mt(int32_t m, int32_t d, int32_t r);
int spr_gp_train_mt_f64(const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Y, int32_t r, int64_t ldy,
                        int32_t kernel, int32_t flags, double *d_raw, double *d_raw_g, double lr, int32_t max_iter, double tol,
                        double *d_s2, double *d_Kinv, double *d_alpha, double *d_info, double *d_trace, void *d_workspace,
                        size_t workspace_bytes, void *stream);
int spr_gp_predict_mt_f64(const double *d_P0, int32_t m, int32_t d, int64_t ldp, const double *d_Pstar, int32_t n_p,
                          int64_t ldps, int32_t kernel, int32_t flags, const double *d_raw, const double *d_s2, int32_t r,
                          const double *d_Kinv, const double *d_alpha, double *d_mean, double *d_var, void *stream);
/* Universal kriging with a regression trend, the level model of CoKriging (csrc/cokriging.hip).  r independent models over
 * the same n points d_X (n x d row-major, row stride ldx >= d, d <= SPR_GP_MAX_D), targets the columns of d_Y (n x r, row
 * stride ldy >= r).  Per model q, d_v[d q ..] = v, theta_c = 10^v_c,
 * R_ij = exp(-sum_c theta_c (x_ic - x_jc)^2) + nugget delta_ij.  Trend F (n x P): [rho,] 1 [, X] -- the column rho = d_Rho[:, q] (n x r, row
 * stride ldr >= r) only when d_Rho is not NULL, the d columns of X only with regr = SPR_CK_LINEAR; n > P.
 * G = F^T R^-1 F, beta = G^-1 F^T R^-1 y, gamma = R^-1 (y - F beta), sigma2 = (y - F beta)^T gamma / (n - P),
 * loss = [ (n - P) log sigma2 + log det R ] / n  (beta and sigma2 profiled out; d loss / d v is the exact derivative).
 * spr_ck_train_f64: Adam (beta 0.9 / 0.999, eps 1e-8, bias correction, step lr) on v with the loop and the stopping rule of
 *   spr_gp_train_f64 (e = |loss - previous loss|, stop when e <= tol or after max_iter evaluations), v clipped to
 *   [v_lo, v_hi] after every step.  d_v is updated in place; d_Rinv (r x n x n), d_RinvF (r x n x P), d_Ginv (r x P x P),
 *   d_beta (r x P), d_gamma (r x n), d_sigma2 (r) are AT THE PARAMETERS LEFT IN d_v (one more factorisation after the last
 *   step).  max_iter = 0: factor at the given d_v, no step.  d_info (r x (4 + d)): evaluations, loss, e, status, then the
 *   gradient, of the last evaluation with a step (max_iter = 0: of the factorisation).  status: 0 ok; 1 a pivot of R <= 0;
 *   2 a pivot of R that is not finite; 3 a pivot of G that is not positive and finite; 4 sigma2 not positive and finite (the
 *   model stops there; its other outputs are undefined).  d_trace: NULL, or r x max_iter x (1 + d): (loss, v) of every
 *   evaluation that was followed by a step.  One workgroup per model, the whole loop in one launch, no atomics: two runs
 *   agree bit for bit.  n <= SPR_GP_MAX_M, d <= SPR_GP_MAX_D (SPR_E_UNSUPPORTED beyond); workspace: spr_ck_workspace(n, d, r)
 *   = 8 r (2 n^2 + n d) bytes (0 for shapes that are refused), 8-byte aligned.
 * spr_ck_predict_f64: d_Xstar (n_p x d, row stride ldxs >= d), d_RhoStar (n_p x r, row stride ldrs >= r; NULL exactly when
 *   d_Rho was) -> d_mean, d_mse (n_p x r row-major):  f* = [rho*,] 1 [, x*],  r*_i = exp(-sum_c theta_c (x*_c - x_ic)^2),
 *   mean = f*^T beta + r*^T gamma,  u = F^T R^-1 r* - f*,  mse = max(sigma2 (1 - r*^T R^-1 r* + u^T G^-1 u), 0). */
#define SPR_CK_MAX_P (SPR_GP_MAX_D + 2)
#define SPR_CK_CONSTANT 0
#define SPR_CK_LINEAR 1
size_t spr_ck_workspace(int32_t n, int32_t d, int32_t r);
int spr_ck_train_f64(const double *d_X, int32_t n, int32_t d, int64_t ldx, const double *d_Y, int32_t r, int64_t ldy,
                     const double *d_Rho, int64_t ldr, int32_t regr, double *d_v, double nugget, double v_lo, double v_hi,
                     double lr, int32_t max_iter, double tol, double *d_Rinv, double *d_RinvF, double *d_Ginv, double *d_beta,
                     double *d_gamma, double *d_sigma2, double *d_info, double *d_trace, void *d_workspace,
                     size_t workspace_bytes, void *stream);
int spr_ck_predict_f64(const double *d_X, int32_t n, int32_t d, int64_t ldx, const double *d_Xstar, int32_t n_p, int64_t ldxs,
                       const double *d_RhoStar, int64_t ldrs, int32_t regr, const double *d_v, int32_t r, const double *d_Rinv,
                       const double *d_RinvF, const double *d_Ginv, const double *d_beta, const double *d_gamma,
                       const double *d_sigma2, double *d_mean, double *d_mse, void *stream);
/* Sharded reconstruct() with n_p > 1 coefficient vectors: the one all-gather of the ranks' (n_p, n_loc) result blocks
 * leaves d_stage[world][n_p][n_loc]; this copies it into the layout the reference returns (:371-375: the vectors as columns
 * of the WHOLE field), d_out[v * ldo + q * n_loc + i] = d_stage[q][v][i].  (One vector needs nothing: the staged blocks are
 * the field.) */
int spr_field_unstage_f64(const double *d_stage, int32_t world, int32_t n_p, int64_t n_loc, double *d_out, int64_t ldo,
                          void *stream);
/* ... and for row blocks of DIFFERENT sizes (the gather then carries blocks padded to n_max rows):
 * d_out[v * ldo + off_q + i] = d_stage[q][v][i] for i < rows_q, with (off_q, rows_q) = d_layout[2q], d_layout[2q+1]
 * (int64, on the device; off_q = first global row of rank q's block minus that of rank 0's). */
int spr_field_unstage_blocks_f64(const double *d_stage, int32_t world, int32_t n_p, int64_t n_max, const int64_t *d_layout,
                                 double *d_out, int64_t ldo, void *stream);

/* ---- the same exchange WITHOUT compute units (csrc/p2p.hip, round 5) -------------------------------------------------
 * RCCL's all-gather runs a device kernel that cannot share a compute unit with the Gram / projection workgroups, so a field
 * gather left in flight under the next fit() only progresses where a CU is free.  On one node the ranks can instead map each
 * other's copy of the field (interprocess handles) and WRITE their block into it with the SDMA engines.
 *   spr_p2p_alloc / spr_p2p_free   a device buffer of n_bytes (multiple of 4096) and its interprocess handle
 *                                  (spr_p2p_handle_bytes() bytes at h_handle).  kind 0: hipMalloc (coarse-grained: coherent
 *                                  between GPUs at kernel boundaries); 1: fine-grained (coherent at system scope while
 *                                  kernels run: the counters); 2: uncached.  The ONE allocation this library makes: a
 *                                  handle can only be taken of the base pointer of an allocation.
 *   spr_p2p_open / spr_p2p_close   map / unmap a buffer exported by ANOTHER process of this node (peer access is enabled
 *                                  lazily); the handle bytes travel through any channel the caller has (torch.distributed).
 *   spr_p2p_device_id / _peer_access   the PCI bus id of the current device (>= 16 bytes at h_buf), and whether the current
 *                                  device IS the one with a given bus id or may access its memory (*h_can = 1 / 0; 0 also
 *                                  for a device this process cannot see).  Exchanged next to the handles: a write into
 *                                  mapped memory of a GPU without peer access is a memory fault, not an error code.
 *   spr_p2p_signal / spr_p2p_wait  hipStreamWriteValue64 / hipStreamWaitValue64(>=) on a 64-bit counter inside such a
 *                                  buffer (own or mapped); used on the copy streams.
 *   spr_p2p_flags_set / _wait      ONE single-wave kernel that raises / awaits n <= 128 counters (host table of device
 *                                  pointers, passed to the kernel by value): what the compute stream uses.  The wait gives
 *                                  up after timeout_s seconds of the device's wall clock -- or at once on a counter that
 *                                  carries the poison bit, spr_p2p_poison_bit() = 1 << 62: "this exchange is broken" -- and
 *                                  leaves (index + 1, value seen) in the two words at d_status (NULL: nowhere) -- every
 *                                  wave reaches its exit.
 *   spr_p2p_copy                   one device-to-device copy through the SDMA engines (hipMemcpyDeviceToDeviceNoCU).
 *   spr_field_gather_p2p           this rank's block of the field -- columns [first, first + n_loc) of the n_p rows of its
 *                                  own (n_p, ldo) copy d_field -- into the same place of every peer's copy: per peer p, on
 *                                  streams[p] (streams may repeat; the peers of one stream are served together: one wait
 *                                  kernel, their copies, one kernel for their counters): wait until *d_release_flag[p] >=
 *                                  release_value (a counter in THIS rank's memory that peer p raises when it no longer reads
 *                                  what its copy held; 0 = no wait; a single-wave kernel that gives up after
 *                                  release_timeout_s), n_p copies of n_loc doubles, *d_peer_arrive_flag[p] = arrive_value (a
 *                                  counter in peer p's memory), and, if given, *d_pushed_flag[p] = arrive_value (this rank's
 *                                  own: "the push to p has left").  A release wait that gives up leaves (p + 1, value seen) in
 *                                  the two words at d_status (page-locked host or device memory the kernels can reach; NULL:
 *                                  nowhere) and -- an SDMA copy cannot be taken back -- every arrival counter raised while
 *                                  *d_status != 0 carries the poison bit: the peer's join of this gather and this rank's own
 *                                  both fail, nobody is handed a field that was overwritten while it may still have been read.
 *                                  The caller orders streams[p] behind the kernel that wrote the block -- with events, or
 *                                  (d_ready_flag != NULL) with a counter of its own that it raises to ready_value on its
 *                                  compute stream behind that kernel (spr_p2p_flags_set: system-scope release): the copy
 *                                  streams' wait kernels then await it too (index n_peers in the status words if it never
 *                                  comes) and no event of the compute stream is needed.
 *   spr_field_gather_p2p_join      `stream` waits (one kernel) until every one of the n counters -- the peers' arrivals and
 *                                  this rank's own pushed counters -- has reached arrive_value.
 *   spr_field_gather_p2p_release   *d_peer_release_flag[p] = value for every peer (one kernel), behind everything enqueued
 *                                  on `stream` so far (the consumers of the previous field).
 * All pointer tables are HOST arrays of device pointers.  Replaces the remote half of Ur @ Ar.T being whole on every caller
 * (sparse_sensing.py:371-375) next to torch.distributed's all_gather; SPR_P2P_BLIT=1 swaps the SDMA copies for blit kernels
 * (a diagnostic). */
size_t spr_p2p_handle_bytes(void);
int spr_p2p_alloc(size_t n_bytes, int32_t kind, void **d_ptr, void *h_handle);
int spr_p2p_free(void *d_ptr);
int spr_p2p_open(const void *h_handle, void **d_mapped);
int spr_p2p_close(void *d_mapped);
int spr_p2p_device_id(char *h_buf, int32_t n_buf);
int spr_p2p_peer_access(const char *h_bus_id, int32_t *h_can);
int spr_p2p_signal(void *d_flag, uint64_t value, void *stream);
int spr_p2p_wait(void *d_flag, uint64_t value, void *stream);
int spr_p2p_flags_set(void *const *d_flags, int32_t n, uint64_t value, void *stream);
int spr_p2p_flags_wait(void *const *d_flags, int32_t n, uint64_t value, double timeout_s, void *d_status, void *stream);
int spr_p2p_copy(void *d_dst, const void *d_src, int64_t n_bytes, void *stream);
uint64_t spr_p2p_poison_bit(void);
int spr_field_gather_p2p(const double *d_field, int64_t ldo, int32_t n_p, int64_t first, int64_t n_loc, int32_t n_peers,
                         void *const *d_peer_field, void *const *d_release_flag, uint64_t release_value,
                         double release_timeout_s, void *const *d_peer_arrive_flag, uint64_t arrive_value,
                         void *const *d_pushed_flag, void *const *streams, void *d_status, void *d_ready_flag,
                         uint64_t ready_value);
int spr_field_gather_p2p_join(void *const *d_flags, int32_t n_flags, uint64_t arrive_value, double timeout_s, void *d_status,
                              void *stream);
int spr_field_gather_p2p_release(void *const *d_peer_release_flag, int32_t n_peers, uint64_t value, void *stream);

/* ---- the collectives of the sharded path behind this ABI (csrc/comm.hip, round 6) -------------------------------------------
 * north_star: "a single RCCL all-reduce over xGMI for the Gram matrix and a final all-gather for the reconstructed field"; the
 * reference has neither (one process, NumPy).  RCCL is reached through dlopen -- the copy that is already in the process
 * (PyTorch's), else librccl.so.1 of the ROCm installation, else SPR_RCCL_LIBRARY=<path> -- so this library links nothing but the
 * HIP runtime; where no RCCL can be loaded these calls return SPR_E_UNSUPPORTED with the loader's text.
 *   spr_comm_unique_id   (one rank) fills spr_comm_unique_id_bytes() bytes; the caller carries them to the other ranks through
 *                        any channel it has (a file, MPI, torch.distributed);
 *   spr_comm_init        COLLECTIVE over the `world` callers: a communicator on the CURRENT device; spr_comm_destroy frees it;
 *   spr_allreduce_f64    in-place sum of `count` doubles over the ranks, enqueued on `stream` (_i64: 64-bit integers -- the
 *                        digit histograms of the median scaling, :140-141);
 *   spr_allgather        rank q's bytes_per_rank bytes land at d_recv + q * bytes_per_rank on every rank (the field of
 *                        reconstruct(), sparse_sensing.py:371-375: whole on every caller);
 *   spr_fit_gram_pass    the first pass of fit() WITH its collective as one enqueue (SURVEY 8(b) "spr_fit_stats_gram (includes
 *                        collectives)"): spr_stats_gram + finalize into the rank's slots of d_buf = [F m m Gram | world x F x 3
 *                        statistics | world first rows] (spr_fit_gram_pass_buffer() bytes; zeroed here), the all-reduce of d_buf
 *                        over `comm` (NULL: one rank, no collective), spr_gram_combine_f64 -> d_G [m][m], d_feat [F][5],
 *                        d_scale / d_inv_scale [F].  Replaces np.average / np.std / X0 = (X - cnt)/scl / the X0^T X0 half of
 *                        np.linalg.svd (:112, :115, :169, :272) for a row block of a sharded X.  m <= SPR_MAX_M_WIDE (beyond 256 the
 *                        column-split path with its three launches, BASELINE config 5's m = 512); workspace:
 *                        spr_fit_gram_pass_workspace(m, n_features, n_rows) bytes, 256-byte aligned; scale_code as
 *                        for spr_gram_combine_f64; x_is_f32: d_X is float (storage only).  Afterwards d_buf still holds what
 *                        every rank contributed: rows per (rank, feature) = d_buf[F m m + (q F + f) 3], first rows at the end. */
size_t spr_comm_unique_id_bytes(void);
int spr_comm_unique_id(void *h_id);
int spr_comm_init(const void *h_id, int32_t rank, int32_t world, void **comm);
int spr_comm_destroy(void *comm);
int spr_comm_info(void *comm, int32_t *rank, int32_t *world);
const char *spr_comm_library(void);
int spr_allreduce_f64(void *comm, double *d_buf, int64_t count, void *stream);
int spr_allreduce_i64(void *comm, int64_t *d_buf, int64_t count, void *stream);
int spr_allgather(void *comm, const void *d_send, void *d_recv, int64_t bytes_per_rank, void *stream);
size_t spr_fit_gram_pass_buffer(int32_t m, int32_t n_features, int32_t world);
size_t spr_fit_gram_pass_workspace(int32_t m, int32_t n_features, int64_t n_rows);
int spr_fit_gram_pass(void *comm, const void *d_X, int32_t x_is_f32, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                      int64_t n_points, int32_t n_features, int32_t scale_code, double *d_rowmean, double *d_buf,
                      size_t buf_bytes, double *d_G, double *d_feat, double *d_scale, double *d_inv_scale, void *d_workspace,
                      size_t workspace_bytes, void *stream);

/* ---- K6 : QR column pivoting of Ur^T (sensor selection) -----------------------------
 * Replaces scipy.linalg.qr(Ur.T, pivoting=True) (:739) -- only the first s pivots are
 * used by the reference (:740-743).  Greedy max-residual-norm selection with norm
 * down-dating, identical in exact arithmetic to dgeqp3's choice; ties go to the lowest
 * global row index (LAPACK idamax).  Candidate-set form (csrc/qr_pivot.hip): a full sweep
 * over Ur leaves exact residual norms, a candidate set (the largest rows of every sweep
 * block) and tau = the largest norm a non-candidate can have; steps run on the candidates
 * and are certified while the winner's residual is strictly above tau.
 *
 * spr_mask_rows     Ur[~mask,:] = 0 in place (:737-738); d_mask is n_rows bytes.
 * spr_qr_init       d_nrm[i] = |Ur[i,:]|^2, candidate set, this rank's best record
 *                   d_rec[0..r+2] = (value, global row as double, runner-up, row of Ur) and
 *                   d_tau[0].
 * spr_qr_step       given the ranks' records d_recs[n_rec][r+3] and taus d_taus[n_tau]: picks
 *                   the winner, writes d_piv[step], the direction d_Q[step][r], d_gap[step]
 *                   (relative gap to the best rival candidate) and d_ok[step] (1 = certified:
 *                   first step after a sweep, or winner > tau), down-dates the candidate
 *                   residuals and leaves this rank's next record in d_rec.
 * spr_qr_refresh    applies the nq <= spr_qr_batch() accepted directions Q[j0..j0+nq) to all
 *                   rows in one sweep (pivots marked), then new candidates / d_rec / d_tau.
 * Driver loop (host): up to spr_qr_batch() steps, read d_ok once, keep the certified prefix
 * (always >= 1 step), refresh, repeat.  Single GPU: d_recs == d_rec, d_taus == d_tau.
 * Workspace: spr_qr_workspace(n_rows) bytes, the same buffer for all calls of one run.
 *
 * calc_type='gem' (SPR.gem, :586-698) runs on the same machinery: the conditional variance of a row given the
 * rows already picked is the squared residual of the row, centred over its r entries, after projecting out the
 * centred picks -- i.e. the pivoting above with the direction 1/sqrt(r) applied first (host puts it in Q[0],
 * piv[0] = -1, one refresh) and the steps numbered from 1.  Two extras:
 * spr_qr_exclude     d_nrm[i] = -1 (out of the pool for good) for rows with d_mask[i] == 0 (search mask, :617)
 *                    and for rows whose position d_xyz[(row0+i) % n_points][xyz_dim] lies closer than d_min to
 *                    the position of one of the picks d_piv[0..nq) (:649-652); call it before the refresh that
 *                    applies those picks.  d_mask / d_xyz may be NULL.
 * spr_qr_step        with d_xyz != NULL also drops the candidates closer than d_min to the step's pick.
 * "Closer" is the reference's np.linalg.norm(p_sensor - xyz, axis=1) < d_min bit for bit: every square rounded, the
 * squares added in coordinate order (no fused multiply-add), a correctly rounded square root -- so that cells lying ON
 * the d_min sphere of a structured mesh fall on the reference's side (tests/test_exclude_gpu.py). */
#define SPR_QR_REC_LEN(r) ((r) + 3)
size_t spr_qr_workspace(int64_t n_rows);                 /* r <= SPR_MAX_R */
size_t spr_qr_workspace_r(int64_t n_rows, int32_t r);    /* any r <= SPR_MAX_R_WIDE (0 beyond) */
int32_t spr_qr_batch(void);
int spr_mask_rows_f64(double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu,
                      const uint8_t *d_mask, void *stream);
int spr_qr_init_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu,
                    int64_t row0, double *d_nrm, double *d_rec, double *d_tau,
                    void *d_workspace, size_t workspace_bytes, void *stream);
/* spr_qr_init with the squared row norms given (d_nrm0, written by spr_project_norms_* / spr_project_stream_norms_* for this
 * very d_Ur; not modified): no pass over the basis.  d_nrm is the working vector the steps down-date. */
int spr_qr_init_norms_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0,
                          const double *d_nrm0, double *d_nrm, double *d_rec, double *d_tau,
                          void *d_workspace, size_t workspace_bytes, void *stream);
int spr_qr_step_f64(int64_t n_rows, int32_t r, int32_t step, const double *d_recs, int32_t n_rec,
                    const double *d_taus, int32_t n_tau, int32_t first, double *d_Q,
                    int64_t *d_piv, double *d_gap, double *d_ok, double *d_rec,
                    const double *d_xyz, int32_t xyz_dim, int64_t n_points, double d_min,
                    void *d_workspace, size_t workspace_bytes, void *stream);
/* single GPU: n_steps consecutive steps in one call (d_recs = d_rec, n_rec = 1, first = first_exact for the call's
 * first step: 1 after spr_qr_init_* / spr_qr_refresh_* / a full epoch sweep, 0 after a pool sweep) */
int spr_qr_steps_f64(int64_t n_rows, int32_t r, int32_t step0, int32_t n_steps, int32_t first_exact,
                     const double *d_tau, double *d_Q, int64_t *d_piv, double *d_gap, double *d_ok, double *d_rec,
                     const double *d_xyz, int32_t xyz_dim, int64_t n_points, double d_min,
                     void *d_workspace, size_t workspace_bytes, void *stream);
/* ---- K6, epoch sweeps: refreshes that only visit the rows that can still be picked (csrc/qr_pivot.hip) -----------
 * Same pivots as the refresh-per-batch scheme above (:739), fewer passes over Ur.  d_nrm_e holds norms that are exact
 * for the directions [0, j_e) (a copy of the initial norms, later rewritten by full sweeps); the rows with d_nrm_e >
 * theta form the POOL (spr_qr_pool_build: sorted local row list).  A pool sweep recomputes d_nrm = d_nrm_e - sum over the
 * epoch's directions [j_e, j) of (u . q)^2 for the pool's rows only and certifies the following steps against
 * max(tau of the pool, tau_floor = theta); a full sweep (d_pool = NULL) does it for every row, rewrites d_nrm_e and
 * starts the next epoch at j.  j_mark: the picks d_piv[j_mark, j) have not been taken out of the race yet.
 * Range: r a multiple of 16 up to SPR_MAX_R, 16-byte aligned rows, fewer than 2^31 local rows
 * (spr_qr_epoch_supported); at most spr_qr_epoch_max_directions(r) directions per sweep. */
int32_t spr_qr_epoch_supported(int32_t r, int64_t ldu, const void *d_Ur, int32_t u_is_f32, int64_t n_rows);
int32_t spr_qr_epoch_max_directions(int32_t r);
size_t spr_qr_pool_workspace(void);
int spr_qr_pool_build(const double *d_nrm_e, int64_t n_rows, double theta, int32_t *d_pool, int64_t cap,
                      int32_t *d_pool_n, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_qr_epoch_sweep_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0,
                           const double *d_Q, const int64_t *d_piv, int32_t j_e, int32_t j, int32_t j_mark,
                           double *d_nrm_e, double *d_nrm, const int32_t *d_pool, const int32_t *d_pool_n,
                           int64_t pool_n_host, double tau_floor, double *d_rec, double *d_tau,
                           void *d_workspace, size_t workspace_bytes, void *stream);
int spr_qr_exclude_f64(double *d_nrm, int64_t n_rows, int64_t row0, int64_t n_points,
                       const uint8_t *d_mask, const double *d_xyz, int32_t xyz_dim,
                       const int64_t *d_piv, int32_t nq, double d_min, void *stream);
int spr_qr_refresh_f64(const double *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0,
                       const double *d_Q, const int64_t *d_piv, int32_t j0, int32_t nq,
                       double *d_nrm, double *d_rec, double *d_tau,
                       void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- K7 + K8 : Theta = C . Ur and cnt = C . X_cnt for a CSR measurement matrix ------
 * Replaces C.dot(self.Ur) (:797) and self.C.dot(self.X_cnt[:,0]) (:573).  The one-hot C
 * of optimal_placement is the 1-nnz-per-row case (a row gather).  Column indices are
 * GLOBAL rows; entries outside [row0,row0+n_rows) are skipped, so per-rank results are
 * partial sums to be all-reduced.  d_Theta is s x r row-major, d_cnt has s entries.
 * d_scl (optional, s entries) = C . X_scl[:,0] (sampling @ X_scl, :233) from the per-feature
 * d_scale[n_features] and the global n_points.  r = 0: d_Ur and d_Theta may be NULL, only d_cnt / d_scl are written. */
int spr_measure_csr_f64(const int64_t *d_indptr, const int64_t *d_indices,
                        const double *d_vals, int32_t s, const double *d_Ur,
                        int64_t n_rows, int32_t r, int64_t ldu, int64_t row0,
                        const double *d_rowmean, const double *d_scale, int64_t n_points,
                        int32_t n_features, double *d_Theta, double *d_cnt, double *d_scl,
                        void *stream);

/* ---- K8 + K9 : scale_vector + (weighted) least squares ------------------------------
 * Replaces scale_vector (:571-582) and the OLS branch of predict (:868-878) for n_p
 * measurement vectors at once.  d_y is n_p x s x 3 (value, std-dev, feature id).
 * Per vector: y0 = ((y-cnt)/scl, sigma/scl); W = I if every sigma is 0 else diag(1/y0_sigma);
 * normal equations (W Theta)^T (W Theta) a = (W Theta)^T W y0 by f64 MFMA + Cholesky.
 * Outputs: d_Ar, d_Ar_sigma (n_p x r), d_y0 (n_p x s x 2, may be NULL),
 * d_info (n_p x 2: [0] = 0 ok / 1 Cholesky breakdown / 2 a weight 1/sigma that is not finite -- an uncertainty that is zero or
 * NaN for SOME sensors makes W = diag(1/0) at :872 and np.linalg.pinv raises LinAlgError --, [1] = (max L_jj / min L_jj)^2). */
int spr_solve_ols_f64(const double *d_Theta, int32_t s, int32_t r, const double *d_cnt,
                      const double *d_scale, int32_t n_features, const double *d_y,
                      int32_t n_p, double *d_Ar, double *d_Ar_sigma, double *d_y0,
                      double *d_info, void *stream);

/* r > SPR_MAX_R (up to SPR_MAX_R_WIDE): the same normal-equations solve with its matrices in a workspace of
 * spr_solve_ols_workspace(s, r, n_p) bytes (L2-resident; one 1024-thread workgroup per vector), same outputs. */
size_t spr_solve_ols_workspace(int32_t s, int32_t r, int32_t n_p);
int spr_solve_ols_wide_f64(const double *d_Theta, int32_t s, int32_t r, const double *d_cnt,
                           const double *d_scale, int32_t n_features, const double *d_y, int32_t n_p,
                           double *d_Ar, double *d_Ar_sigma, double *d_y0, double *d_info, void *d_workspace,
                           size_t workspace_bytes, void *stream);

/* ---- K9b : the same solve with the reference's pseudo-inverse semantics ---------------
 * np.linalg.pinv(W @ Theta) (:873, :877; SVD, rcond = 1e-15) returns the MINIMUM-NORM least-squares solution when
 * W Theta is rank deficient or has fewer rows than columns (s < r: every GEM placement, :660-668).  Same inputs and
 * scaling as spr_solve_ols_f64; per vector the rows of [W Theta | W y0 | y0_sigma] are reduced to an r x (r+2)
 * triangular factor (streaming Householder QR, only when s > r) and a one-sided Jacobi SVD of that factor gives
 * a = sum_{sigma_i > rcond sigma_max} v_i (u_i^T b) / sigma_i.  predict() takes this path when s < r, on Cholesky
 * breakdown, or when the fast path reports cond^2 > 1e13.  s_cnt = entries of d_cnt (must equal s).
 * d_info (n_p x 4): [0] Jacobi sweeps (negative = not converged, or a non-finite weight 1/sigma as in spr_solve_ols_f64:
 * the reference's pinv raises LinAlgError for both), [1] rank kept, [2] sigma_max, [3] smallest
 * singular value kept. */
int spr_solve_pinv_f64(const double *d_Theta, int32_t s, int32_t r, const double *d_cnt, int32_t s_cnt,
                       const double *d_scale, int32_t n_features, const double *d_y, int32_t n_p,
                       double rcond, double *d_Ar, double *d_Ar_sigma, double *d_y0, double *d_info,
                       void *stream);

/* r > SPR_MAX_R (the reference keeps any r <= m modes, :336): the same algorithm with its factor in a workspace of
 * spr_solve_pinv_workspace(r, n_p) bytes (L2-resident; one 1024-thread workgroup per vector), r <= SPR_MAX_R_WIDE. */
size_t spr_solve_pinv_workspace(int32_t r, int32_t n_p);
int spr_solve_pinv_wide_f64(const double *d_Theta, int32_t s, int32_t r, const double *d_cnt, int32_t s_cnt,
                            const double *d_scale, int32_t n_features, const double *d_y, int32_t n_p,
                            double rcond, double *d_Ar, double *d_Ar_sigma, double *d_y0, double *d_info,
                            void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- sensors fused with a Gaussian prior: SPR.assimilate (csrc/assimilate.hip) ---------------------------------------
 * The Bayesian update of a prior  a ~ N(a0, C C^T)  on the coefficients with n_p measurement vectors, in the scaled units
 * of spr_solve_ols_f64: d_y is n_p x s x 3 (value, std-dev, feature id), y0 = (y - cnt) / scl, sig0 = sigma / scl,
 * W = diag(1 / sig0) ALWAYS (an uncertainty that is zero or not finite is status 2, there is no W = I case).
 * Exactly one of d_sigma (n_p x r: C = diag(sigma), q must equal r) and d_factor (n_p x r x q contiguous, 1 <= q <= r).
 * d_a0 is n_p x r.  Per vector, with  B = W Theta C  (s x q)  and  res = y0 - Theta a0:
 *   H' = I + B^T B = L' L'^T  (f64 MFMA Gram with the sensors as the contraction index, Cholesky in LDS; positive definite
 *   for ANY s >= 1, so s < r needs no pseudo-inverse),  z = H'^-1 B^T W res,
 *   d_Ar (n_p x r) = a0 + C z,  d_F (n_p x r x q) = C L'^-T  (posterior covariance F F^T),  d_Ar_std (n_p x r) =
 *   sqrt(diag(F F^T)),  d_z (n_p x q, may be NULL) = z,
 *   d_info (n_p x 4): [0] 0 ok / 1 a Cholesky pivot that is <= 0 or not finite / 2 a sensor uncertainty that is zero or not
 *   finite, [1] (max L'_jj / min L'_jj)^2, [2] chi2 = |W res|^2 - |L'^-1 B^T W res|^2 = res^T (Theta C C^T Theta^T + R)^-1 res
 *   with R = diag(sig0^2), [3] log det(Theta C C^T Theta^T + R) = sum log sig0^2 + 2 sum log L'_jj.
 * A coefficient whose row of C is zero returns d_a0 bit for bit, with std 0 and a zero row of F.
 * One 256-thread workgroup per vector; the factor form first forms [Theta C_p | Theta a0_p] per vector into the workspace
 * (spr_assimilate_workspace(s, r, q, n_p) = 8 n_p s (q + 1) bytes, 8-byte aligned; 0 for shapes that are refused; the
 * diagonal form takes d_workspace = NULL).  No atomics, fixed summation orders: two runs agree bit for bit.
 * Refusals, in this order: a NULL pointer or both / neither prior (SPR_E_INVALID), a shape that is not positive or
 * q outside [1, r] or q != r with d_sigma (SPR_E_INVALID), r > SPR_MAX_R (SPR_E_UNSUPPORTED), the workspace
 * (SPR_E_INVALID when NULL or misaligned, SPR_E_WORKSPACE when too small).  Nothing is launched after a refusal. */
size_t spr_assimilate_workspace(int32_t s, int32_t r, int32_t q, int32_t n_p);
int spr_assimilate_f64(const double *d_Theta, int32_t s, int32_t r, const double *d_cnt, const double *d_scale,
                       int32_t n_features, const double *d_y, int32_t n_p, const double *d_a0, const double *d_sigma,
                       const double *d_factor, int32_t q, double *d_Ar, double *d_Ar_std, double *d_F, double *d_z,
                       double *d_info, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- synthetic snapshot matrices (benchmark input) -------------------
 * X[i,j] = (f+1) * ( sum_k L[i,k] R[k,j] + eps * N[i,j] ) + 10 f, with L, N standard
 * normal from a counter-based generator keyed by (seed, GLOBAL row, column), so any row
 * range is reproducible on any rank count.  d_R is k x ldr (ldr >= col0+ncols).
 * Columns [col0, col0+ncols) of the virtual matrix are written to d_X (n_rows x ldx). */
int spr_synth_f64(double *d_X, int64_t n_rows, int32_t ncols, int64_t ldx, int64_t row0,
                  int64_t n_points, int32_t col0, const double *d_R, int32_t k, int32_t ldr,
                  double eps, uint64_t seed, void *stream);
/* the same generator evaluated at arbitrary global rows for one column (held-out state) */
int spr_synth_gather_f64(const int64_t *d_rows, int32_t n, int64_t n_points, int32_t col,
                         const double *d_R, int32_t k, int32_t ldr, double eps,
                         uint64_t seed, double *d_out, void *stream);

/* ---- camera projection matrix: segments in, CSR out (csrc/raycast.hip) ---------------------------------------------------
 * Replaces the reference's per-pixel pyvista line queries (openmeasure.utils.camera.project, utils.py:318-469).  The grid is
 * nx x ny x nz axis-aligned cells with origin (ox, oy, oz) and spacing (hx, hy, hz), or with stored edge coordinates (the
 * _rect entry points below), cell id = i + nx (j + ny k), nx ny nz < 2^31.
 * d_seg holds n_seg segments of 6 doubles (a, b), p(t) = a + t (b - a), t in [0, 1]; pixel p owns the
 * n_ray consecutive segments from p n_ray.  A cell belongs to a segment iff the part of the segment inside it has positive
 * length in the kernel's arithmetic (a touch at a point, an edge or a face is no hit); agreement with another locator on
 * grazing rays is not promised.
 *   spr_raycast_count_f64  d_count[n_seg] = cells of each segment (slab clip, then a 3-D DDA of at most nx + ny + nz + 2 steps);
 *   spr_raycast_fill_f64   the same traversal; d_offset[n_seg + 1] is the exclusive prefix sum of d_count (the caller's scan),
 *                          (cell, chord length) of segment s go to d_cell / d_chord [d_offset[s], d_offset[s + 1]);
 *   spr_raycast_count_rect_f64 / spr_raycast_fill_rect_f64  the same two over a RECTILINEAR grid: d_xe / d_ye / d_ze hold
 *                          nx + 1 / ny + 1 / nz + 1 device doubles, the ascending coordinates of the cell faces; cell (i, j, k) is
 *                          the box d_xe[i] .. d_xe[i + 1] x d_ye[j] .. d_ye[j + 1] x d_ze[k] .. d_ze[k + 1].  Plane k of an axis is
 *                          the loaded edge, in the slab clip (edges 0 and n) and in the traversal alike; the start cell is found
 *                          by a bisection of ceil(log2 n) <= 31 steps and clamped into the grid; t_next = (e[i + (d > 0)] - a) / d,
 *                          +inf for d == 0.  The library cannot see the edge values: whatever they hold, the traversal takes at
 *                          most nx + ny + nz + 2 steps, every index is clamped before it addresses an edge array or forms a cell
 *                          id, and fill stays inside the segment's counted range; edges that do not ascend give cells without
 *                          meaning, not a fault.  merge and compact below serve both kinds of grid;
 *   spr_raycast_merge      one workgroup per pixel: sorts the pixel's entries by cell and adds the chords of equal cells;
 *                          the unique entries, ascending, go to the front of the pixel's range of d_cell_out / d_chord_out and
 *                          their number to d_uniq[n_pix].  Lists of up to spr_raycast_merge_lds_entries() entries are sorted
 *                          in LDS, longer ones by the same network in d_cell / d_chord (which it therefore reorders).
 *                          max_cells_per_ray: the caller's bound on d_count (nx + ny + nz + 2); n_ray max_cells_per_ray <= 2^30;
 *   spr_raycast_compact    d_indptr[n_pix + 1] is the exclusive prefix sum of d_uniq; d_indices = cell + col0 and d_vals = 1
 *                          (SPR_RAYCAST_HIT: the reference's C, the union over the pixel's rays) or the summed chord / n_ray
 *                          (SPR_RAYCAST_LENGTH: the line integral).
 * No atomics, no communication between workgroups: two runs agree bit for bit.  Refusals, in this order: a NULL pointer
 * (SPR_E_INVALID), a shape (SPR_E_INVALID), the cell-count cap (SPR_E_UNSUPPORTED).  Nothing is launched after a refusal. */
#define SPR_RAYCAST_HIT 0
#define SPR_RAYCAST_LENGTH 1
int32_t spr_raycast_merge_lds_entries(void);
int spr_raycast_count_f64(const double *d_seg, int64_t n_seg, int32_t nx, int32_t ny, int32_t nz, double ox, double oy,
                          double oz, double hx, double hy, double hz, int64_t *d_count, void *stream);
int spr_raycast_fill_f64(const double *d_seg, int64_t n_seg, int32_t nx, int32_t ny, int32_t nz, double ox, double oy,
                         double oz, double hx, double hy, double hz, const int64_t *d_offset, int64_t *d_cell,
                         double *d_chord, void *stream);
int spr_raycast_count_rect_f64(const double *d_seg, int64_t n_seg, int32_t nx, int32_t ny, int32_t nz, const double *d_xe,
                               const double *d_ye, const double *d_ze, int64_t *d_count, void *stream);
int spr_raycast_fill_rect_f64(const double *d_seg, int64_t n_seg, int32_t nx, int32_t ny, int32_t nz, const double *d_xe,
                              const double *d_ye, const double *d_ze, const int64_t *d_offset, int64_t *d_cell,
                              double *d_chord, void *stream);
int spr_raycast_merge(const int64_t *d_offset, int64_t n_pix, int32_t n_ray, int32_t max_cells_per_ray, int64_t *d_cell,
                      double *d_chord, int64_t *d_cell_out, double *d_chord_out, int64_t *d_uniq, void *stream);
int spr_raycast_compact(const int64_t *d_offset, int64_t n_pix, int32_t n_ray, const int64_t *d_cell, const double *d_chord,
                        const int64_t *d_indptr, int32_t weights, int64_t col0, int64_t *d_indices, double *d_vals,
                        void *stream);

/* ---- resampling of point-cloud snapshots onto another cloud or a voxel grid (csrc/resample.hip) -------------------------
 * Stands where the reference has resample_to_grid (utils.py:17-99) and the GPR notebook its griddata(method='nearest') loop.
 * A mesh is its (n, 3) float64 cell centres.  For every target the neighbours are the k <= 8 sources smallest under
 * (d2, source index), lexicographic; d2 = ((dx dx) + (dy dy)) + (dz dz) in float64, every operation rounded once.
 * SPR_RESAMPLE_NEAREST: k = 1, weight 1.  SPR_RESAMPLE_IDW: Shepard's weights of power 2, w_j = (1 / d2_j) / sum_i (1 / d2_i);
 * d2_0 == 0 gives 1, 0, 0, ...  A source with d2 > max_distance^2 is no neighbour (max_distance < 0: no limit); unused slots
 * hold index -1, weight 0 and d2 = +inf; a target without a neighbour is invalid.  Agreement with VTK's probe filter
 * (containing-cell interpolation on the mesh's connectivity, which this library never sees) is not promised.
 *   spr_resample_bin_f64    d_key[n_src] = bx + nbx (by + nby bz), the source's bin in a grid of nbx x nby x nbz bins over the
 *                           box [lo, hi] (an axis with hi == lo has one bin; at most 8 n_src + 8 bins, below 2^31).  The
 *                           caller sorts the keys (stably, so that a bin's points ascend in source index) and forms
 *                           d_start[n_bins + 1], the exclusive prefix sum of the bin counts;
 *   spr_resample_knn_f64    one thread per target.  d_src_sorted (n_src, 3) are the sources in sorted order, d_perm[n_src] their
 *                           source indices; bins and box as given to spr_resample_bin_f64.  Targets: d_dst (n_dst, 3), or
 *                           d_dst == NULL and the centres o + (i + 0.5) h of a gx x gy x gz voxel grid in cell-id order
 *                           (gx gy gz == n_dst), formed in the kernel.  Shells of bins of growing Chebyshev radius around the
 *                           target's clamped bin are searched until the k-th best d2 is strictly below the squared distance to
 *                           the bins not yet searched (or that distance exceeds max_distance, or every bin was searched):
 *                           at most max(nbx, nby, nbz) + 1 shells whatever the data.  Writes d_idx (n_dst, k) int64, d_d2 and
 *                           d_weight (n_dst, k), d_inspected[n_dst] = candidate points looked at;
 *   spr_resample_apply_*    d_out[(f n_dst + c) ldo + :m] = sum_j d_weight[c k + j] d_X[(f n_src + d_idx[c k + j]) ldx + :m] for
 *                           the n_features blocks, summed for j = 0, 1, ... in float64, rounded once on store (_x32: float
 *                           storage, widened on load).  SPR_RESAMPLE_NEAREST copies row d_idx[c k] bit for bit.  An index
 *                           that is negative or >= n_src is never dereferenced; a target with no usable index gets fill_value
 *                           in every column.  One wave per destination row, 16-byte loads where every row of both matrices
 *                           starts on a 16-byte boundary and m fills whole pieces.  Every row offset is 64-bit.
 * No atomics: two runs agree bit for bit.  Refusals: a NULL pointer or a shape (SPR_E_INVALID), 2^31 or more points or too
 * many bins (SPR_E_UNSUPPORTED).  Nothing is launched after a refusal. */
#define SPR_RESAMPLE_NEAREST 0
#define SPR_RESAMPLE_IDW 1
int spr_resample_bin_f64(const double *d_xyz, int64_t n_src, int32_t nbx, int32_t nby, int32_t nbz, double lox, double loy,
                         double loz, double hix, double hiy, double hiz, int64_t *d_key, void *stream);
int spr_resample_knn_f64(const double *d_src_sorted, const int64_t *d_perm, const int64_t *d_start, int64_t n_src,
                         int32_t nbx, int32_t nby, int32_t nbz, double lox, double loy, double loz, double hix, double hiy,
                         double hiz, const double *d_dst, int64_t n_dst, int32_t gx, int32_t gy, int32_t gz, double ox,
                         double oy, double oz, double hx, double hy, double hz, int32_t k, int32_t method,
                         double max_distance, int64_t *d_idx, double *d_d2, double *d_weight, int32_t *d_inspected,
                         void *stream);
int spr_resample_apply_f64(const double *d_X, int64_t ldx, int64_t n_src, int32_t n_features, int32_t m,
                           const int64_t *d_idx, const double *d_weight, int64_t n_dst, int32_t k, int32_t method,
                           double fill_value, double *d_out, int64_t ldo, void *stream);
int spr_resample_apply_x32(const float *d_X, int64_t ldx, int64_t n_src, int32_t n_features, int32_t m,
                           const int64_t *d_idx, const double *d_weight, int64_t n_dst, int32_t k, int32_t method,
                           double fill_value, float *d_out, int64_t ldo, void *stream);

/* ---- f32 STORAGE (BASELINE config 5: 50M cells x 16 features x 512 snapshots does not fit 8 x 288 GB in f64) ----
 * The reference keeps X in whatever float dtype the caller passes (sparse_sensing.py:74); its X_cnt / X_scl are float64
 * (np.zeros, :106-107), so X0 = (X - X_cnt)/X_scl (:169) and the U of its SVD (:272) are float64 whatever that dtype is.
 * These entry points take the snapshot shard as float (suffix _x32), widen every element on load and do ALL arithmetic
 * in f64 exactly like their _f64 twins -- same arguments, same outputs (row means, statistics, Gram blocks, norms, Theta,
 * fields stay double).  The basis is float64 by default (spr_project_x32_f64out, spr_project_stream_x32_f64out); storing
 * it as float as well is a STORAGE OPTION the reference does not have (spr_project_x32 / spr_project_stream_x32 write the
 * f64 result rounded once; the _u32 twins read such a basis), for shards whose f64 basis would not fit.  Two-element
 * pieces: rows 8-byte aligned and an even m / ld take the vector path.  With a float basis, parity of the sensors is
 * checked against both the reference's choice (pivots of the f64 basis) and dgeqp3 on the stored basis widened to f64. */
int spr_stats_gram_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                       int64_t n_points, int32_t n_features, int32_t center, double *d_rowmean,
                       void *d_workspace, size_t workspace_bytes, void *stream);
int spr_rowstats_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                     int64_t n_points, int32_t n_features, double *d_rowmean, double *d_fstats,
                     void *d_workspace, size_t workspace_bytes, void *stream);
int spr_gram_cross_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                       int64_t n_points, int32_t n_features, int32_t center, double *d_rowmean,
                       double *d_gram, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_gram_cross_pair_x32(const float *d_X, int64_t n_rows, int32_t col_a, int32_t col_b, int32_t w_b,
                            int32_t ldg, int64_t ldx, int64_t row0, int64_t n_points, int32_t n_features,
                            int32_t center, double *d_rowmean, double *d_gram, void *d_workspace,
                            size_t workspace_bytes, void *stream);
int spr_project_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                    int64_t n_points, int32_t n_features, int32_t center, const double *d_inv_scale,
                    const double *d_rowmean, const double *d_W, int32_t r, float *d_Ur, int64_t ldu,
                    int32_t accumulate, void *stream);
/* f32 shard, f64 result: for the column slices of a wide X (m > 256), whose partial sums cancel by up to
 * sigma_1/sigma_r between the slices -- accumulate them in an f64 block of rows, round to f32 once afterwards */
int spr_project_x32_f64out(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                           int64_t n_points, int32_t n_features, int32_t center, const double *d_inv_scale,
                           const double *d_rowmean, const double *d_W, int32_t r, double *d_Ur, int64_t ldu,
                           int32_t accumulate, void *stream);
/* ... and its last slice: adds the f64 partial sums d_acc_in (row stride lda) and stores the f32 total in d_Ur */
int spr_project_x32_acc(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                        int64_t n_points, int32_t n_features, int32_t center, const double *d_inv_scale,
                        const double *d_rowmean, const double *d_W, int32_t r, const double *d_acc_in,
                        int64_t lda, float *d_Ur, int64_t ldu, void *stream);
/* streamed-W projection (any m) of an f32 shard: float basis, or double basis (the reference's dtype for a float32 X:
 * X_cnt / X_scl are float64, :106-107, so X0 = (X - X_cnt)/X_scl and U are float64 whatever the dtype of X) */
int spr_project_stream_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                           int64_t n_points, int32_t n_features, int32_t center, const double *d_inv_scale,
                           const double *d_rowmean, const double *d_W, int32_t r, float *d_Ur, int64_t ldu,
                           void *d_workspace, size_t workspace_bytes, void *stream);
int spr_project_stream_x32_f64out(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                                  int64_t n_points, int32_t n_features, int32_t center, const double *d_inv_scale,
                                  const double *d_rowmean, const double *d_W, int32_t r, double *d_Ur, int64_t ldu,
                                  void *d_workspace, size_t workspace_bytes, void *stream);
int spr_project_norms_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                          int64_t n_points, int32_t n_features, int32_t center, const double *d_inv_scale,
                          const double *d_rowmean, const double *d_W, int32_t r, float *d_Ur, int64_t ldu,
                          double *d_rownorm2, void *stream);
int spr_project_norms_x32_f64out(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                                 int64_t n_points, int32_t n_features, int32_t center, const double *d_inv_scale,
                                 const double *d_rowmean, const double *d_W, int32_t r, double *d_Ur, int64_t ldu,
                                 double *d_rownorm2, void *stream);
int spr_project_field_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                          int64_t n_points, int32_t n_features, const double *d_inv_scale, const double *d_rowmean,
                          const double *d_W, int32_t r, float *d_Ur, int64_t ldu, double *d_rownorm2,
                          const double *d_scale, const double *d_A, int32_t n_p, double *d_Xrec, int64_t ldo,
                          void *stream);
int spr_project_field_x32_f64out(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                                 int64_t n_points, int32_t n_features, const double *d_inv_scale,
                                 const double *d_rowmean, const double *d_W, int32_t r, double *d_Ur, int64_t ldu,
                                 double *d_rownorm2, const double *d_scale, const double *d_A, int32_t n_p,
                                 double *d_Xrec, int64_t ldo, void *stream);
int spr_project_stream_norms_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                                 int64_t n_points, int32_t n_features, int32_t center, const double *d_inv_scale,
                                 const double *d_rowmean, const double *d_W, int32_t r, float *d_Ur, int64_t ldu,
                                 double *d_rownorm2, void *d_workspace, size_t workspace_bytes, void *stream);
int spr_project_stream_norms_x32_f64out(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                                        int64_t n_points, int32_t n_features, int32_t center,
                                        const double *d_inv_scale, const double *d_rowmean, const double *d_W,
                                        int32_t r, double *d_Ur, int64_t ldu, double *d_rownorm2, void *d_workspace,
                                        size_t workspace_bytes, void *stream);
int spr_stats_gram_shifted_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                               int64_t n_points, int32_t n_features, const double *d_shift, double *d_rowsum,
                               void *d_workspace, size_t workspace_bytes, void *stream);
int spr_scale_rows_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                       int64_t n_points, int32_t n_features, const double *d_rowmean,
                       const double *d_inv_scale, double *d_X0, int64_t ldo, void *stream);
int spr_feature_minmax_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                           int64_t n_points, int32_t n_features, double *d_minmax,
                           void *d_workspace, size_t workspace_bytes, void *stream);
int spr_colsums_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                    int64_t n_points, int32_t n_features, const double *d_rowmean, double *d_out,
                    void *d_workspace, size_t workspace_bytes, void *stream);
int spr_feature_digit_hist_x32(const float *d_X, int64_t n_rows, int32_t m, int64_t ldx, int64_t row0,
                               int64_t n_points, int32_t n_features, const uint64_t *d_prefix, int32_t shift,
                               int32_t bits, int32_t two_targets, uint64_t *d_hist, void *stream);
int spr_synth_f32(float *d_X, int64_t n_rows, int32_t ncols, int64_t ldx, int64_t row0,
                  int64_t n_points, int32_t col0, const double *d_R, int32_t k, int32_t ldr,
                  double eps, uint64_t seed, void *stream);
int spr_reconstruct_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0,
                        int64_t n_points, int32_t n_features, const double *d_rowmean,
                        const double *d_scale, const double *d_rowscale, const double *d_A, int32_t n_p,
                        double *d_Xrec, int64_t ldo, void *stream);
int spr_mask_rows_u32(float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu,
                      const uint8_t *d_mask, void *stream);
int spr_qr_init_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu,
                    int64_t row0, double *d_nrm, double *d_rec, double *d_tau,
                    void *d_workspace, size_t workspace_bytes, void *stream);
int spr_qr_init_norms_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0,
                          const double *d_nrm0, double *d_nrm, double *d_rec, double *d_tau,
                          void *d_workspace, size_t workspace_bytes, void *stream);
int spr_qr_epoch_sweep_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0,
                           const double *d_Q, const int64_t *d_piv, int32_t j_e, int32_t j, int32_t j_mark,
                           double *d_nrm_e, double *d_nrm, const int32_t *d_pool, const int32_t *d_pool_n,
                           int64_t pool_n_host, double tau_floor, double *d_rec, double *d_tau,
                           void *d_workspace, size_t workspace_bytes, void *stream);
int spr_qr_refresh_u32(const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu, int64_t row0,
                       const double *d_Q, const int64_t *d_piv, int32_t j0, int32_t nq,
                       double *d_nrm, double *d_rec, double *d_tau,
                       void *d_workspace, size_t workspace_bytes, void *stream);
int spr_measure_csr_u32(const int64_t *d_indptr, const int64_t *d_indices, const double *d_vals,
                        int32_t s, const float *d_Ur, int64_t n_rows, int32_t r, int64_t ldu,
                        int64_t row0, const double *d_rowmean, const double *d_scale, int64_t n_points,
                        int32_t n_features, double *d_Theta, double *d_cnt, double *d_scl, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPR_HIP_H */
