/*
 * matinv.h -- native C ABI of the MI355X batched small-matrix inversion engine
 * (libmatinv_hip.so). Plain pointers and sizes only; no C++/torch types.
 *
 * This is the device-resident, stream-aware core that the reference-named
 * entry points of inverse_gpu.h are thin wrappers over. A matrix is n x n,
 * column-major (element (r,c) at c*n + r), and matrix k of a batch starts at
 * base + k*stride elements (stride >= n*n; the reference uses a pitched
 * allocation, /root/reference/src/helper.cu:103-118, so a stride is needed to
 * accept its device tables without a copy).
 *
 * All functions return MATINV_OK (0) or a negative matinv_status and never
 * call exit(); matinv_last_error() describes the last failure of the calling
 * thread. The reference-named wrappers keep the reference's fatal behaviour
 * (include/helper_gpu.h:9-18 there) on top of this.
 */
#ifndef MATINV_H_INCLUDED
#define MATINV_H_INCLUDED

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MATINV_OK = 0,
    MATINV_ERR_ARG = -1,         /* bad n / batch / pointer / stride                   */
    MATINV_ERR_UNSUPPORTED = -2, /* n > 1024, or the forced kernel family cannot serve it */
    MATINV_ERR_HIP = -3,         /* a HIP runtime call failed (message in last_error)  */
    MATINV_ERR_NO_DEVICE = -4    /* no gfx950 device visible                           */
} matinv_status;

typedef enum {
    MATINV_F64 = 0,
    MATINV_F32 = 1
} matinv_dtype;

typedef enum {
    MATINV_ALGO_GAUSS_JORDAN = 0, /* general matrices, partial pivoting. Replaces pivotRow/normalizeRow/
                                     transform_matrix, src/gauss/batched_invert.cu:17-95, and the cuBLAS LU
                                     path src/gauss/inverse_gpu.cu:16-58                                   */
    MATINV_ALGO_CHOLESKY = 1      /* SPD matrices (only the lower triangle is read), full symmetric result.
                                     Replaces the four Cholesky families of src/inverse_cholesky_gpu.cu. LDS family:
                                     literal L L^T, L^-1, L^-T L^-1; tile family: the square-root-free symmetric
                                     blocked sweep (same Schur complements, pivots = squares of diag(L))       */
} matinv_algo;

/* Kernel families; MATINV_KERNEL_AUTO picks by (algo, dtype, n). The others force one family and
 * fail with MATINV_ERR_UNSUPPORTED when it cannot handle the request (used by tests and bench). */
typedef enum {
    MATINV_KERNEL_AUTO = 0,
    MATINV_KERNEL_LDS = 1,     /* one workgroup per matrix, matrix resident in LDS, any n up to the LDS limit */
    MATINV_KERNEL_ROWLANE = 2, /* n <= 16: 64/npad matrices per wavefront, one row per lane, DPP broadcasts     */
    MATINV_KERNEL_TILE = 3     /* 16x16 MFMA accumulator tiles, f64 and f32: blocked Gauss-Jordan with one wavefront per matrix
                                  (n <= 64) or four (64 < n <= 128); for MATINV_ALGO_CHOLESKY the symmetric blocked sweep on
                                  lower-triangular tiles (n <= 64) / the four-wave sweep with positivity-checked pivots */,
    MATINV_KERNEL_ROW = 4,     /* n <= 64: one matrix per wavefront, row per lane, classical partial pivoting with the pivot
                                  row broadcast through v_readlane; the pivoting path behind the tile family */
    MATINV_KERNEL_GLOBAL = 5,  /* any n <= 1024 (the reference's limit): one 1024-thread workgroup per matrix, working copy
                                  in global memory; the functional path for matrices that do not fit on chip */
    MATINV_KERNEL_TILEP = 7,   /* the MFMA tile Gauss-Jordan with TRUE partial pivoting inside the kernel (pivot search on the
                                  LDS-staged panel, one row per lane; rows never move, the permutation is folded into the store
                                  addresses): general matrices at MFMA speed. One wavefront per matrix (n <= 64), four
                                  (n <= 128), one per tile column (n <= 192 in f64, 256 in f32; automatic there) */
    MATINV_KERNEL_BLOCKED = 6  /* any n <= 1024, global-memory working copies, two launches per panel over the whole batch.
                                  MATINV_ALGO_CHOLESKY: blocked right-looking Cholesky, A^-1 = L^-T L^-1 as one symmetric product
                                  (automatic beyond n = 128). MATINV_ALGO_GAUSS_JORDAN: blocked Gauss-Jordan with partial
                                  pivoting, panel of 32 columns eliminated with one thread per row (automatic beyond the LDS limit) */
} matinv_kernel;

/* Gauss-Jordan, 16 < n <= 192 (f64) / 256 (f32): which MFMA tile kernel a launch uses (process-wide, atomic; default
 * MATINV_GJ_NATURAL_FIRST, or the environment's MATINV_GJ_POLICY=natural|pivot|adaptive read at the first launch).
 *   NATURAL_FIRST  the natural-order kernel (pivots verified, not searched: the fast path of dominant / SPD batches); a
 *                  matrix it rejects is redone by the pivoting kernel in the same stream. The result of a matrix depends
 *                  on that matrix alone: repeatable bit for bit, identical for a sharded and an unsharded batch.
 *   PIVOT          straight to the kernel with partial pivoting inside the MFMA sweep (general matrices at full speed; also
 *                  per-matrix deterministic). The reference's LU names (inverse_lu_cuda_batched_*) always take it.
 *   ADAPTIVE       chooses per launch from the reject count of the last completed natural-order launch of that size on
 *                  that device: fastest on streams of like batches, but a matrix that both kernels accept may get either
 *                  kernel's bits depending on what ran before. */
typedef enum {
    MATINV_GJ_NATURAL_FIRST = 0,
    MATINV_GJ_PIVOT = 1,
    MATINV_GJ_ADAPTIVE = 2
} matinv_gj_policy;
int matinv_set_gj_policy(int policy); /* returns the previous policy, or MATINV_ERR_ARG */

/* THREAD SAFETY. Every entry point may be called concurrently from several host threads, on the same or on different devices
 * (the device is the calling thread's current HIP device; matinv_last_error() is per thread). The library keeps no state
 * between calls except: the GJ policy above (atomic), the ADAPTIVE policy's per-device counters (atomic), and the staging
 * memory cached per (device, stream) inside the library (mutex-protected; matinv_release_cache). A matinv_queue is NOT internally locked: one
 * thread at a time per queue. Launches on one stream execute in issue order, as HIP defines. */

/* Invert `batch` matrices that are already resident in device memory.
 *   dA      in : batch matrices, matrix k at dA + k*strideA (elements). Never written.
 *   dAinv   out: matrix k at dAinv + k*strideInv. May be exactly dA with strideInv == strideA (in place:
 *                every kernel reads a whole matrix before writing it); partial overlap is undefined.
 *   dInfo   out: optional int[batch] (device). 0 = ok; k+1 = no usable pivot at elimination step k
 *                (Gauss-Jordan: singular) or leading minor k+1 not positive (Cholesky: not SPD).
 *                Gauss-Jordan: for a matrix with several deficient columns the code names one of them, not necessarily the first.
 *                Cholesky, MATINV_F32, 160 < n <= 256 under MATINV_KERNEL_AUTO or MATINV_KERNEL_TILE (and the solve composed from
 *                that inversion): the kernel eliminates the 16 columns of a tile in a permuted order, and the code names a column of
 *                the same 16-column tile [16 t, 16 t + 16) as the first non-positive leading minor, never one beyond n. It is that
 *                column itself when a single non-positive diagonal entry is all that keeps the matrix from being positive
 *                definite. Every other path, in both dtypes, names the column itself.
 *                For info != 0 the output matrix is filled with NaN (never left half-written).
 *   stream     : hipStream_t as void* (NULL = default stream). Asynchronous.
 */
int matinv_inverse_batched(int algo, int dtype, int n, const void *dA, size_t strideA, void *dAinv,
                           size_t strideInv, size_t batch, int *dInfo, void *stream);

/* Same, forcing a kernel family (matinv_kernel). */
int matinv_inverse_batched_ex(int algo, int dtype, int n, const void *dA, size_t strideA, void *dAinv,
                              size_t strideInv, size_t batch, int *dInfo, void *stream, int kernel);

/* Which family MATINV_KERNEL_AUTO resolves to (a matinv_kernel), or a negative status. */
int matinv_select_kernel(int algo, int dtype, int n);

/* Name of the __global__ function a (algo, dtype, n, kernel) request launches -- the name rocprofv3 reports ("" for a request that
 * matinv_inverse_batched_ex would refuse: a forced family without a kernel for this n, n beyond 1024). Pure host logic. */
const char *matinv_kernel_name(int algo, int dtype, int n, int kernel);

/* Batched linear solve X_k = A_k^-1 B_k without forming the inverse in memory (for 16 < n <= 64 and nrhs <= 16).
 *   dA      in : n x n, column-major, matrix k at dA + k*strideA (strideA >= n*n). Never written. MATINV_ALGO_CHOLESKY reads
 *                only the lower triangle (SPD input), MATINV_ALGO_GAUSS_JORDAN serves general matrices.
 *   dB      in : n x nrhs, column-major (column r at r*n), matrix k at dB + k*strideB (strideB >= n*nrhs). Never written.
 *   dX      out: n x nrhs like B, stride strideX. May be exactly dB with strideX == strideB (in place); partial overlap is undefined.
 *   dInfo   out: optional int[batch] (device), the codes of matinv_inverse_batched: for a structurally singular (Gauss-Jordan) or
 *                clearly indefinite (Cholesky) A_k the same value as the inverse reports. For info != 0, X_k is all NaN.
 *   stream     : hipStream_t as void*. Asynchronous; no host synchronisation (except under MATINV_DEBUG_REJECTS).
 * Paths: 16 < n <= 64 and nrhs <= 16: one fused MFMA tile kernel per batch (A^T with B^T as a border tile row); Gauss-Jordan
 * matrices its natural pivot order rejects are solved again with partial pivoting in the same stream (under MATINV_GJ_PIVOT
 * that row solve takes the whole batch). Elsewhere (n <= 1024): the inverse of matinv_inverse_batched_ex into a scratch block,
 * in k-range chunks of at most the blocked-path workspace cap, then a batched product. X_k depends on matrix k alone.
 * batch == 0 is a no-op; bad arguments return MATINV_ERR_ARG without touching a device; n > 1024: MATINV_ERR_UNSUPPORTED. */
int matinv_solve_batched(int algo, int dtype, int n, int nrhs, const void *dA, size_t strideA, const void *dB, size_t strideB,
                         void *dX, size_t strideX, size_t batch, int *dInfo, void *stream);
/* Same, forcing a path: MATINV_KERNEL_AUTO = as above; MATINV_KERNEL_TILE = the fused kernel (plus its row-solve fallback) only,
 * MATINV_ERR_UNSUPPORTED outside its range; any other family = the composed path with that family doing the inversion. */
int matinv_solve_batched_ex(int algo, int dtype, int n, int nrhs, const void *dA, size_t strideA, const void *dB, size_t strideB,
                            void *dX, size_t strideX, size_t batch, int *dInfo, void *stream, int kernel);
/* Name of the first __global__ function a solve request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_solve_kernel_name(int algo, int dtype, int n, int nrhs, int kernel);
/* Host-pointer form (packed: stride n*n for A, n*nrhs for B and X; `info` optional host int[batch]). Synchronous. */
int matinv_solve_batched_host(int algo, int dtype, int n, int nrhs, const void *hA, const void *hB, void *hX, size_t batch,
                              int *info);

/* Fused Gaussian-process pipeline, device-resident (replaces calcluateMean / calcluateVariance,
 * src/gauss_bench.cu:127-265,275-409: addDiagonal + batched inverse + two gemmBatched):
 *   means[k] = a_k^T (B_k + diag(c_k))^-1 d_k
 *   vars[k]  = e_k - a_k^T (B_k + diag(c_k))^-1 a_k
 * a,c,d: batch*n; B: batch*n*n (SPD, column-major, stride n*n); e, out: batch scalars. No input is modified
 * and the inverse is never written to memory.
 */
int matinv_mean_batched(int dtype, int n, const void *dAs, const void *dBs, const void *dCs, const void *dDs,
                        void *dMeans, size_t batch, int *dInfo, void *stream);
int matinv_variance_batched(int dtype, int n, const void *dAs, const void *dBs, const void *dCs, const void *dEs,
                            void *dVars, size_t batch, int *dInfo, void *stream);
/* Name of the first __global__ function a mean (variance == 0) or variance request launches ("" for a request that would be refused).
 * Both forms run the same instantiation. Pure host logic. */
const char *matinv_gp_kernel_name(int dtype, int n, int variance);

/* Batched log-determinant: sign_k * exp(logabsdet_k) = det A_k, without ever forming the determinant (it may overflow or underflow
 * the number format; log|det| does not).
 *   dA          in : n x n, column-major, matrix k at dA + k*strideA (strideA >= n*n). Never written. MATINV_ALGO_CHOLESKY reads only
 *                    the lower triangle (SPD input; sign is +1), MATINV_ALGO_GAUSS_JORDAN serves general matrices with partial
 *                    pivoting (the sign includes the parity of the row exchanges).
 *   dLogAbsDet  out: batch scalars of A's dtype.
 *   dSign       out: optional (NULL allowed) batch scalars of A's dtype: +1 or -1.
 *   dInfo       out: optional int[batch] (device), the codes of matinv_inverse_batched (k+1: no usable pivot at step k / leading minor
 *                    k+1 not positive). For info != 0 both outputs of that matrix are NaN.
 *   stream         : hipStream_t as void*. Asynchronous; no host synchronisation.
 * Paths: Cholesky, n <= 96: one MFMA tile kernel (the factorisation half of the symmetric blocked sweep, pivots folded into a
 * mantissa / exponent pair). Gauss-Jordan, n <= 64: one matrix per wavefront, row per lane, partial pivoting. Everything else up to
 * n = 1024: one workgroup per matrix on a working copy in library scratch (k-range chunks under the blocked-path workspace cap).
 * The result for matrix k depends on matrix k alone. batch == 0 is a no-op; bad arguments return MATINV_ERR_ARG without touching a
 * device; n > 1024: MATINV_ERR_UNSUPPORTED. */
int matinv_logdet_batched(int algo, int dtype, int n, const void *dA, size_t strideA, void *dLogAbsDet, void *dSign, size_t batch,
                          int *dInfo, void *stream);
/* Same, forcing a kernel: MATINV_KERNEL_AUTO = as above; MATINV_KERNEL_TILE (Cholesky, n <= 96), MATINV_KERNEL_ROW (Gauss-Jordan,
 * n <= 64), MATINV_KERNEL_GLOBAL (both, n <= 1024) force that kernel and return MATINV_ERR_UNSUPPORTED outside its range; any other
 * family: MATINV_ERR_UNSUPPORTED; an unknown value: MATINV_ERR_ARG. */
int matinv_logdet_batched_ex(int algo, int dtype, int n, const void *dA, size_t strideA, void *dLogAbsDet, void *dSign, size_t batch,
                             int *dInfo, void *stream, int kernel);
/* Name of the __global__ function a logdet request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_logdet_kernel_name(int algo, int dtype, int n, int kernel);
/* Host-pointer form (packed: stride n*n; hSign and `info` optional). Synchronous. */
int matinv_logdet_batched_host(int algo, int dtype, int n, const void *hA, void *hLogAbsDet, void *hSign, size_t batch, int *info);

/* Gaussian-process log marginal likelihood, device-resident:
 *   logml[k] = -1/2 d_k^T M_k^-1 d_k - 1/2 log det M_k - n/2 log(2 pi),     M_k = B_k + diag(c_k)
 * B: batch*n*n (SPD, column-major, stride n*n; only the lower triangle is read); c, d: batch*n; dCs may be NULL (M = B); logml: batch
 * scalars. No input is modified; neither the inverse nor M is written to memory. dInfo as above (logml[k] is NaN for info != 0).
 * n <= 96: one bordered MFMA tile kernel (d rides as a border row, the corner ends as -d^T M^-1 d). Beyond, to n = 1024: composed
 * from matinv_variance_batched (a = d, e = 0), the global-memory logdet kernel on B + diag c and a combining kernel. Asynchronous. */
int matinv_logml_batched(int dtype, int n, const void *dBs, const void *dCs, const void *dDs, void *dLogml, size_t batch, int *dInfo,
                         void *stream);
/* Name of the first __global__ function a logml request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_logml_kernel_name(int dtype, int n);
/* Host-pointer form (packed; hCs and `info` optional). Synchronous. */
int matinv_logml_batched_host(int dtype, int n, const void *hBs, const void *hCs, const void *hDs, void *hLogml, size_t batch, int *info);

/* Leave-one-out cross-validation of a Gaussian process (Rasmussen & Williams 5.4.2), device-resident. With M_k = B_k + diag(c_k),
 * kappa_i = [M^-1]_ii and alpha = M^-1 d:
 *   mean[k*n + i] = d_i - alpha_i / kappa_i      the prediction at training point i from the other n - 1
 *   var[k*n + i]  = 1 / kappa_i                  its predictive variance (of the observation: the noise c_i included)
 *   logpl[k]      = sum_i (1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i) - n/2 log(2 pi)      the log pseudo-likelihood
 * B: batch*n*n (SPD, column-major, stride n*n; only the lower triangle is read); c, d: batch*n; dCs may be NULL (M = B).
 * dMean, dVar: batch*n, dLogPL: batch scalars; each may be NULL (all three NULL: MATINV_ERR_ARG), and which of them are requested
 * does not change a bit of the others. No input is modified (outputs must not overlap inputs); neither M nor its inverse is written
 * to caller memory; the result of matrix k depends on matrix k alone. dInfo (optional): 0, or the 1-based column of the first
 * non-positive (or NaN) pivot -- every output of that matrix is then NaN. n <= 96: the LOO form of the one-wavefront SPD tile sweep
 * (n^2/2 + 2n elements read, 2n + 1 written). Beyond, to n = 1024: the LOO form of the global-memory Cholesky kernel on a working
 * copy in library scratch. Asynchronous, no host synchronisation. */
int matinv_loo_batched(int dtype, int n, const void *dBs, const void *dCs, const void *dDs, void *dMean, void *dVar, void *dLogPL,
                       size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function a leave-one-out request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_loo_kernel_name(int dtype, int n);
/* Host-pointer form (packed; hCs, `info` and each output optional). Synchronous. */
int matinv_loo_batched_host(int dtype, int n, const void *hBs, const void *hCs, const void *hDs, void *hMean, void *hVar, void *hLogPL,
                            size_t batch, int *info);

/* Gradients of the GP log marginal likelihood (the one matinv_logml_batched returns), device-resident. With M_k = B_k + diag(c_k),
 * K = M^-1, alpha = K d and nparam symmetric derivative matrices dM_p = dM / d theta_p per matrix:
 *   grad[k*nparam + p] = 1/2 sum_ij (alpha_i alpha_j - K_ij) dM_p[i][j]      d logml / d theta_p = 1/2 tr((alpha alpha^T - K) dM_p)
 *   gradc[k*n + i]     = 1/2 (alpha_i^2 - K_ii)                              d logml / d c_i
 *   alpha[k*n + i]     = alpha_i                                             what the predictive mean needs
 * B, c, d as in matinv_loo_batched (SPD, column-major, only the lower triangle read; dCs may be NULL). dDMs: batch*nparam*n*n elements,
 * matrix (k, p) at offset (k*nparam + p)*n*n, column-major; only its lower triangle is read, the upper one is implied by symmetry.
 * dGrad: batch*nparam, dGradC, dAlpha: batch*n; each may be NULL (all three NULL: MATINV_ERR_ARG), and which of them are requested
 * does not change a bit of the others. dGrad needs nparam >= 1 and dDMs; without dGrad, nparam = 0 and dDMs = NULL are fine (dDMs is
 * not read). No input is modified (outputs must not overlap inputs); neither M nor its inverse is written to caller memory; the result
 * of matrix k depends on matrix k alone. dInfo (optional): 0, or the 1-based column of the first non-positive (or NaN) pivot -- every
 * output of that matrix is then NaN. n <= 96: the gradient form of the one-wavefront SPD tile sweep ((nparam + 1) n^2/2 + 2n elements
 * read, nparam + 2n written). Beyond, to n = 1024: the gradient form of the global-memory Cholesky kernel on a working copy in library
 * scratch. The log marginal likelihood itself is not an output here. Asynchronous, no host synchronisation. */
int matinv_logml_grad_batched(int dtype, int n, int nparam, const void *dBs, const void *dCs, const void *dDs, const void *dDMs, void *dGrad,
                              void *dGradC, void *dAlpha, size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function a gradient request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_logml_grad_kernel_name(int dtype, int n);
/* Host-pointer form (packed; hCs, `info` and each output optional; hDMs is read only with hGrad). Synchronous. */
int matinv_logml_grad_batched_host(int dtype, int n, int nparam, const void *hBs, const void *hCs, const void *hDs, const void *hDMs,
                                   void *hGrad, void *hGradC, void *hAlpha, size_t batch, int *info);

/* Gaussian-process prediction at nquery query points per covariance matrix, device-resident. With M_k = B_k + diag(c_k), K = M^-1,
 * alpha = K d, a_kj the cross-covariance vector of query j of matrix k (n elements) and e_kj its prior variance:
 *   mean[k*nquery + j] = a_kj^T alpha_k                 the predictive mean
 *   var[k*nquery + j]  = e_kj - a_kj^T K_k a_kj         the predictive variance of the latent function
 * For nquery = 1 this is what matinv_mean_batched / matinv_variance_batched compute, without a second factorisation for the second
 * output and without one per query beyond. B, c, d as in matinv_loo_batched (SPD, column-major, only the lower triangle read; dCs may be
 * NULL). dAs: batch*nquery*n elements, vector (k, j) at offset (k*nquery + j)*n, i.e. the n x nquery cross-covariance matrix of item k
 * in column-major order. dEs: batch*nquery elements, or NULL (e = 0: var is then minus the variance reduction). dMean, dVar:
 * batch*nquery elements; each may be NULL (both NULL: MATINV_ERR_ARG), and which of them is requested does not change a bit of the
 * other. dDs is read only with dMean, dEs only with dVar. nquery >= 1. var is not clamped: a tiny negative value from cancellation
 * is the caller's to see. No input is modified (outputs must not overlap inputs); neither M nor its inverse is written to caller
 * memory; the result for (k, j) depends on matrix k and query j alone, bit for bit -- not on batch, nquery or the position of j among
 * the queries. dInfo (optional): 0, or the 1-based column of the first non-positive (or NaN) pivot -- every output of that matrix is
 * then NaN. n <= 96: the prediction form of the one-wavefront SPD tile sweep, the queries in groups of 16 on the MFMA unit
 * (n^2/2 + 2n + nquery (n + 1) elements read, 2 nquery written). Beyond, to n = 1024: the prediction form of the global-memory
 * Cholesky kernel on a working copy in library scratch. Asynchronous, no host synchronisation. */
int matinv_predict_batched(int dtype, int n, int nquery, const void *dBs, const void *dCs, const void *dDs, const void *dAs, const void *dEs,
                           void *dMean, void *dVar, size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function a prediction request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_predict_kernel_name(int dtype, int n);
/* Host-pointer form (packed; hCs, hEs, `info` and each output optional; hDs is read only with hMean). Synchronous. */
int matinv_predict_batched_host(int dtype, int n, int nquery, const void *hBs, const void *hCs, const void *hDs, const void *hAs,
                                const void *hEs, void *hMean, void *hVar, size_t batch, int *info);

/* The joint predictive covariance between the nquery query points of a covariance matrix, device-resident. With M, K, alpha and a_ki as in
 * matinv_predict_batched and E_k the nquery x nquery prior covariance between the queries of matrix k:
 *   mean[k*nquery + i]                      = a_ki^T alpha_k                   the predictive mean
 *   cov[k*nquery^2 + j*nquery + i]          = E_k[i][j] - a_ki^T K_k a_kj      nquery x nquery per matrix, column-major
 * dBs, dCs, dDs, dAs as in matinv_predict_batched (only the lower triangle of B read; dCs may be NULL). dEs: batch*nquery^2 elements,
 * column-major per matrix, of which only the lower triangle is read (element (i, j), i >= j, at j*nquery + i), or NULL (E = 0). dCov:
 * batch*nquery^2 elements, BOTH triangles written: the lower element (i >= j) is computed and the upper one is a copy of its bits, so the
 * result is exactly symmetric. dMean: batch*nquery elements. Either output may be NULL (both NULL: MATINV_ERR_ARG), and which of them is
 * requested does not change a bit of the other. dDs is read only with dMean, dEs only with dCov. 1 <= nquery <= 1024 (beyond:
 * MATINV_ERR_UNSUPPORTED). cov is not clamped or regularised. mean carries the same bits as matinv_predict_batched returns for the
 * same inputs; the diagonal of cov equals its var only to rounding, because it is summed on the MFMA unit. No input is modified
 * (outputs must not overlap inputs); neither M nor its inverse is written to caller memory. Bit for bit, mean[k, i] depends on matrix
 * k and query i alone, and cov[k, i, j] with i >= j on matrix k, a_ki, a_kj and E_k[i][j] alone -- not on batch, nquery or the positions
 * of i and j among the queries, as long as i stays the later of the two (swapping two queries may change the last bits). dInfo
 * (optional): 0, or the 1-based column of the first non-positive (or NaN) pivot -- all nquery^2 + nquery outputs of that matrix are
 * then NaN. n <= 96: the covariance form of the one-wavefront SPD tile sweep, a 16 x 16 block of cov per pair of query groups on the
 * MFMA unit (n^2/2 + 2n + 16 n G (G + 1) / 2 + nquery^2 / 2 elements read with G = ceil(nquery / 16), nquery^2 + nquery written).
 * Beyond, to n = 1024: the covariance form of the global-memory Cholesky kernel on a working copy of n (n + nquery) elements per matrix
 * in library scratch. Asynchronous, no host synchronisation. */
int matinv_predict_cov_batched(int dtype, int n, int nquery, const void *dBs, const void *dCs, const void *dDs, const void *dAs,
                               const void *dEs, void *dMean, void *dCov, size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function a predictive-covariance request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_predict_cov_kernel_name(int dtype, int n);
/* Host-pointer form (packed; hCs, hEs, `info` and each output optional; hDs is read only with hMean, hEs only with hCov). Synchronous. */
int matinv_predict_cov_batched_host(int dtype, int n, int nquery, const void *hBs, const void *hCs, const void *hDs, const void *hAs,
                                    const void *hEs, void *hMean, void *hCov, size_t batch, int *info);

/* The lower Cholesky factor of batched SPD matrices and samples coloured by it, device-resident:
 *   C_k = L_k L_k^T,   Y_k[:, s] = m_k + L_k z_ks      for the nsample vectors z_ks of matrix k
 * dC: matrix k is q x q, column-major, at element k*strideC (strideC >= q*q); only its lower triangle is read. dM: batch*q elements, or
 * NULL (m = 0). dZ: batch*q*nsample elements, sample s of matrix k the run of q elements at (k*nsample + s)*q. dY: the same layout.
 * dL: batch*q*q elements, column-major per matrix: the lower triangle with a positive diagonal, the strict upper triangle written as
 * exact zeros. dY and dL are each optional (both NULL: MATINV_ERR_ARG), and which of them is requested does not change a bit of the
 * other; dZ and nsample >= 1 are needed with dY only. 1 <= q <= 1024 and nsample <= 1024 (beyond: MATINV_ERR_UNSUPPORTED). No input is
 * modified (outputs must not overlap inputs). Bit for bit, L_k depends on C_k alone and Y_k[:, s] on C_k, m_k and z_ks alone -- not on
 * batch, nsample or the position of the sample; Z = 0 returns the bits of m (one exception: an element m_i = -0.0 comes back as +0.0,
 * because the zero products are added to it). The library draws no random numbers: Z is the caller's,
 * which keeps every result reproducible. dInfo (optional): 0, or the 1-based column of the first non-positive (or NaN) pivot -- every
 * requested output of that matrix is then NaN; there is no jitter and no pivoting (a semi-definite C is the caller's to regularise).
 * q <= 96: the colour form of the one-wavefront SPD tile sweep, the samples in groups of 16 on the MFMA unit (q^2/2 + q + q nsample
 * elements read, q^2 + q nsample written). Beyond, to q = 1024: the colour form of the global-memory Cholesky kernel on a working copy
 * in library scratch. Asynchronous, no host synchronisation. */
int matinv_colour_batched(int dtype, int q, int nsample, const void *dC, size_t strideC, const void *dM, const void *dZ, void *dY, void *dL,
                          size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function a colour request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_colour_kernel_name(int dtype, int q);
/* Host-pointer form (hM, `info` and each output optional; hZ is read only with hY). Synchronous. */
int matinv_colour_batched_host(int dtype, int q, int nsample, const void *hC, size_t strideC, const void *hM, const void *hZ, void *hY,
                               void *hL, size_t batch, int *info);

/* Whitened points, squared Mahalanobis distances, the log-determinant and the Gaussian log-density of batched SPD matrices,
 * device-resident -- the inverse map of matinv_colour_batched. With C_k = L_k L_k^T and the npoint points x_ks of matrix k:
 *   W_k[:, s]    = L_k^-1 (x_ks - m_k)
 *   maha_k[s]    = ||W_k[:, s]||^2                 = (x - m)^T C^-1 (x - m)
 *   logdet_k     = log det C_k = 2 sum_i log L_ii
 *   logpdf_k[s]  = -1/2 (maha_k[s] + logdet_k + q log 2 pi)        the log-density of N(m_k, C_k) at x_ks
 * dC, strideC, dM: as in matinv_colour_batched (lower triangle read; dM NULL: m = 0). dX: batch*q*npoint elements, point s of matrix k
 * the run of q elements at (k*npoint + s)*q. dW: the same layout. dMaha, dLogpdf: batch*npoint elements, at k*npoint + s. dLogdet: batch
 * elements. Every output is optional and at least one is required (all NULL: MATINV_ERR_ARG); which of them are requested does not
 * change a bit of the others. dX and npoint >= 1 are needed with dW, dMaha or dLogpdf only: with dLogdet alone dX is not read and may be
 * NULL. 1 <= q <= 1024 and npoint <= 1024 (beyond: MATINV_ERR_UNSUPPORTED); the argument checks are those of matinv_colour_batched, in
 * its order. No input is modified (outputs must not overlap inputs). Bit for bit, logdet_k depends on C_k alone and W, maha and logpdf of
 * a point on C_k, m_k and that point alone -- not on batch, npoint or the position of the point. x = m returns W = +0.0 in every element
 * (also where x and m are -0.0) and maha = +0.0. logdet is taken from the running product of the pivots as mantissa and exponent, one
 * logarithm per matrix: it neither overflows nor underflows where det C would. dInfo (optional): 0, or the 1-based column of the first
 * non-positive (or NaN) pivot -- every requested output of that matrix is then NaN; there is no jitter, no pivoting and no fallback launch.
 * q <= 96: the whiten form of the one-wavefront SPD tile sweep; the factor stays in registers in the lane layout of the MFMA's A
 * operand and the points are solved in groups of 16, two dependent MFMAs per block of four columns (q^2/2 + q + q npoint elements read,
 * q npoint + 2 npoint + 1 written). Beyond, to q = 1024: the whiten form of the global-memory Cholesky kernel on a working copy in
 * library scratch (k-range chunks under MATINV_BLOCKED_WS_MB), one thread per point. Asynchronous, no host synchronisation. */
int matinv_whiten_batched(int dtype, int q, int npoint, const void *dC, size_t strideC, const void *dM, const void *dX, void *dW, void *dMaha,
                          void *dLogdet, void *dLogpdf, size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function a whiten request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_whiten_kernel_name(int dtype, int q);
/* Host-pointer form (hM, `info` and each output optional; hX is read only with hW, hMaha or hLogpdf). Synchronous. */
int matinv_whiten_batched_host(int dtype, int q, int npoint, const void *hC, size_t strideC, const void *hM, const void *hX, void *hW,
                               void *hMaha, void *hLogdet, void *hLogpdf, size_t batch, int *info);

/* Multi-output GP solves, device-resident: ntarget target vectors y_kt and nquery query points per covariance matrix. With
 * M_k = B_k + diag(c_k) and a_kj as in matinv_predict_batched:
 *   alpha[(k*ntarget + t)*n + i]           = (M_k^-1 y_kt)_i                          the layout of dYs
 *   quad[k*ntarget + t]                    = y_kt^T M_k^-1 y_kt
 *   logdet[k]                              = log det M_k
 *   logml[k*ntarget + t]                   = -1/2 (quad + logdet + n log 2 pi)        the log marginal likelihood of target t
 *   mean[(k*ntarget + t)*nquery + j]       = a_kj^T alpha_kt                          for ntarget = 1 the layout of matinv_predict_batched
 * dBs, dCs, dAs as in matinv_predict_batched (only the lower triangle of B read; dCs may be NULL). dYs: batch*ntarget*n elements, target t
 * of matrix k the run of n elements at (k*ntarget + t)*n. Every output is optional and at least one is required (all NULL:
 * MATINV_ERR_ARG); which of them are requested does not change a bit of the others. dYs and ntarget >= 1 are needed for every output but
 * dLogdet: with dLogdet alone ntarget may be 0 and dYs NULL. dAs and nquery >= 1 are needed with dMean only: without it nquery may be 0,
 * dAs NULL, and dAs is not read. 1 <= n <= 1024, ntarget <= 1024, nquery <= 1024 (beyond: MATINV_ERR_UNSUPPORTED, after the pointer
 * checks); batch < 2^31; batch == 0 is a no-op after the dtype and n checks. No input is modified (outputs must not overlap inputs);
 * neither M, its inverse nor its factor is written to caller memory. Bit for bit, logdet_k depends on matrix k alone, alpha, quad and
 * logml of (k, t) on matrix k and target t alone, and mean of (k, t, j) additionally on query j alone -- not on batch, ntarget, nquery
 * or the position of t or j. dInfo (optional): 0, or the 1-based column of the first non-positive (or NaN) pivot -- every requested
 * output of that matrix is then NaN; there is no fallback launch. n <= 96: the multi-target form of the one-wavefront SPD tile sweep;
 * the targets in groups of 16 on the MFMA unit, T = M^-1 Y kept in registers and multiplied with every group of 16 queries
 * (n^2/2 + n + ntarget n + ceil(ntarget / 16) nquery n elements read, ntarget n + 2 ntarget + 1 + ntarget nquery written). Beyond, to
 * n = 1024: the multi-target form of the global-memory Cholesky kernel on a working copy of n (n + ntarget) elements per matrix in
 * library scratch (k-range chunks under MATINV_BLOCKED_WS_MB), one thread per target. Asynchronous, no host synchronisation. */
int matinv_multi_target_batched(int dtype, int n, int ntarget, int nquery, const void *dBs, const void *dCs, const void *dYs, const void *dAs,
                                void *dAlpha, void *dQuad, void *dLogdet, void *dLogml, void *dMean, size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function a multi-target request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_multi_target_kernel_name(int dtype, int n);
/* Host-pointer form (packed; hCs, `info` and each output optional; hYs is read with every output but hLogdet, hAs only with hMean).
 * Synchronous. */
int matinv_multi_target_batched_host(int dtype, int n, int ntarget, int nquery, const void *hBs, const void *hCs, const void *hYs,
                                     const void *hAs, void *hAlpha, void *hQuad, void *hLogdet, void *hLogml, void *hMean, size_t batch,
                                     int *info);

/* Gradients of the multi-output GP log marginal likelihood, device-resident: the gradient of sum_t logml_kt of
 * matinv_multi_target_batched, from one factorisation. With M_k = B_k + diag(c_k), K = M_k^-1, D = ntarget targets y_kt,
 * alpha_t = K y_kt, P = nparam symmetric derivative matrices dM_p per matrix and G = sum_t alpha_t alpha_t^T - D K:
 *   grad[k*nparam + p]            = 1/2 sum_ij G_ij dM_p[i][j]                   d(sum_t logml_t) / d theta_p
 *   gradc[k*n + i]                = 1/2 G_ii                                     d(sum_t logml_t) / d c_i
 *   logml[k*ntarget + t]          = -1/2 (y_t^T K y_t + log det M + n log 2 pi)  as matinv_multi_target_batched
 *   alpha[(k*ntarget + t)*n + i]  = (alpha_t)_i                                  the layout of dYs
 * dBs, dCs, dYs as in matinv_multi_target_batched (only the lower triangle of B read; dCs may be NULL); dDMs as in
 * matinv_logml_grad_batched (matrix (k, p) at (k*nparam + p)*n*n, only its lower triangle read). Every output is optional and at least
 * one is required (all NULL: MATINV_ERR_ARG); which of them are requested does not change a bit of the others. dGrad needs nparam >= 1
 * and dDMs; without it nparam may be 0, dDMs NULL, and dDMs is not read. ntarget >= 1 and dYs are always needed. 1 <= n <= 1024,
 * ntarget <= 1024, nparam <= 1024 (beyond: MATINV_ERR_UNSUPPORTED, after the pointer checks); batch < 2^31; batch == 0 is a no-op after
 * the dtype and n checks. No input is modified (outputs must not overlap inputs); neither M, its inverse nor its factor is written to
 * caller memory. logml and alpha carry the bits matinv_multi_target_batched gives for the same inputs. dInfo (optional): 0, or the
 * 1-based column of the first non-positive (or NaN) pivot -- every requested output of that matrix is then NaN; there is no fallback
 * launch. n <= 96: the gradient form of the multi-target tile sweep: the targets in groups of 16 on the MFMA unit, then
 * G accumulated over -D K in the registers by rank-16 MFMA updates and contracted with each dM_p streamed once
 * (n^2/2 + n + ntarget n + nparam n^2/2 elements read, nparam + n + ntarget + ntarget n written; with ntarget > 16 alpha is read back
 * once, from dAlpha or from ntarget n elements of library scratch per workgroup). Beyond, to n = 1024: the multi-target gradient form of
 * the global-memory Cholesky kernel on a working copy of n (n + ntarget) elements per matrix in library scratch (k-range chunks under
 * MATINV_BLOCKED_WS_MB). Asynchronous, no host synchronisation. */
int matinv_multi_target_grad_batched(int dtype, int n, int ntarget, int nparam, const void *dBs, const void *dCs, const void *dYs,
                                     const void *dDMs, void *dGrad, void *dGradC, void *dLogml, void *dAlpha, size_t batch, int *dInfo,
                                     void *stream);
/* Name of the __global__ function a multi-target gradient request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_multi_target_grad_kernel_name(int dtype, int n);
/* Host-pointer form (packed; hCs, `info` and each output optional; hDMs is read only with hGrad). Synchronous. */
int matinv_multi_target_grad_batched_host(int dtype, int n, int ntarget, int nparam, const void *hBs, const void *hCs, const void *hYs,
                                          const void *hDMs, void *hGrad, void *hGradC, void *hLogml, void *hAlpha, size_t batch, int *info);

/* GP regression with a linear trend (universal kriging; Rasmussen & Williams 2.7, explicit basis functions with a vague prior on the
 * coefficients), device-resident. Per matrix k: M = B_k + diag(c_k), Kinv = M^-1, K = nbasis basis vectors h_b (H = [h_1 .. h_K], n x K),
 * D = ntarget targets y_t, Q = nquery queries with cross-covariance a_j, basis values g_j (K) and prior variance e_j. With
 * A = H^T Kinv H (K x K, positive definite iff H has full column rank):
 *   beta[(k*D + t)*K + b]      = (A^-1 H^T Kinv y_t)_b                               the generalised-least-squares coefficients
 *   covbeta[k*K*K + b*K + b']  = (A^-1)_bb'                                          their covariance; bitwise symmetric
 *   alpha[(k*D + t)*n + i]     = (Kinv (y_t - H beta_t))_i                           the layout of dYs; H^T alpha_t = 0
 *   quad[k*D + t]              = (y_t - H beta_t)^T Kinv (y_t - H beta_t) = y_t^T alpha_t
 *   logml[k*D + t]             = -1/2 (quad_t + log det M + log det A + (n - K) log 2 pi)    the restricted likelihood, R&W eq. 2.45
 *   mean[(k*D + t)*Q + j]      = a_j^T alpha_t + g_j^T beta_t
 *   var[k*Q + j]               = e_j - a_j^T Kinv a_j + r_j^T A^-1 r_j,  r_j = g_j - H^T Kinv a_j    R&W eq. 2.42; the same for every target
 * dBs, dCs, dYs, dAs as in matinv_multi_target_batched (only the lower triangle of B read; dCs may be NULL). dHs: batch*K*n elements, basis
 * vector b of matrix k the run of n elements at (k*K + b)*n (the layout of dYs). dGs: batch*Q*K elements, g_j of matrix k at (k*Q + j)*K.
 * dEs: batch*Q elements. Every output is optional and at least one is required (all NULL: MATINV_ERR_ARG); which of them are requested
 * does not change a bit of the others. dBs and dHs are always needed. dYs and ntarget >= 1 are needed with dBeta, dAlpha, dQuad, dLogml or
 * dMean; dAs, dGs and nquery >= 1 with dMean or dVar; dEs with dVar. What is not needed is not read and may be NULL (its count 0): dCovBeta
 * alone needs only B, c and H. 1 <= n <= 1024; 1 <= nbasis <= 16 and nbasis <= n (otherwise MATINV_ERR_ARG, checked with n and dtype);
 * ntarget <= 1024, nquery <= 1024 (beyond: MATINV_ERR_UNSUPPORTED, after the pointer checks); batch < 2^31; batch == 0 is a no-op after
 * the dtype, n and nbasis checks. No input is modified (outputs must not overlap inputs); neither M, its inverse nor its factor is written
 * to caller memory. Bit for bit, covbeta_k depends on matrix k and its basis alone, var of (k, j) additionally on query j alone, beta,
 * alpha, quad and logml of (k, t) on matrix k, its basis and target t alone, mean of (k, t, j) additionally on query j alone -- not on
 * batch, ntarget, nquery or the position of t or j. dInfo (optional): 0; or the 1-based column of the first non-positive (or NaN) pivot
 * of M; or n + b for the first non-positive (or NaN) pivot b (1-based) of A, i.e. a basis that is rank deficient to working precision
 * (the convention matinv_sample_batched uses for cov). On a non-zero info every requested output of that matrix is NaN; there is no
 * fallback launch. n <= 96: the trend form of the one-wavefront SPD tile sweep: H, the targets and the queries in groups of 16 on the
 * MFMA unit, Kinv H parked in LDS, A factored inside the wave (n^2/2 + n + K n + D n read; with mean or var (ceil(D / 16) + 1) Q (n + K) + Q
 * more; K^2 + D K + D n + 2 D + D Q + Q written). Beyond, to n = 1024: the trend form of the global-memory Cholesky kernel on a working
 * copy per matrix in library scratch (k-range chunks under MATINV_BLOCKED_WS_MB), one thread per column of [H | Y] and per query.
 * Asynchronous, no host synchronisation. */
int matinv_trend_batched(int dtype, int n, int nbasis, int ntarget, int nquery, const void *dBs, const void *dCs, const void *dHs,
                         const void *dYs, const void *dAs, const void *dGs, const void *dEs, void *dBeta, void *dCovBeta, void *dAlpha,
                         void *dQuad, void *dLogml, void *dMean, void *dVar, size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function a trend request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_trend_kernel_name(int dtype, int n);
/* Host-pointer form (packed; hCs, `info` and each output optional; the inputs are read as the device form reads them). Synchronous. */
int matinv_trend_batched_host(int dtype, int n, int nbasis, int ntarget, int nquery, const void *hBs, const void *hCs, const void *hHs,
                              const void *hYs, const void *hAs, const void *hGs, const void *hEs, void *hBeta, void *hCovBeta, void *hAlpha,
                              void *hQuad, void *hLogml, void *hMean, void *hVar, size_t batch, int *info);

/* Gradients of the restricted (REML) log marginal likelihood of the trend model, device-resident: the gradient of sum_t logml_kt of
 * matinv_trend_batched, from one factorisation. With M_k = B_k + diag(c_k), Kinv = M_k^-1, H the K = nbasis basis vectors,
 * A = H^T Kinv H, P = Kinv - Kinv H A^-1 H^T Kinv, D = ntarget targets y_kt, alpha_t = P y_kt, nparam symmetric derivative matrices dM_p
 * per matrix and G = sum_t alpha_t alpha_t^T - D P (H does not depend on the parameters):
 *   grad[k*nparam + p]            = 1/2 sum_ij G_ij dM_p[i][j]                   d(sum_t logml_t) / d theta_p
 *   gradc[k*n + i]                = 1/2 G_ii                                     d(sum_t logml_t) / d c_i
 *   logml[k*ntarget + t], alpha[(k*ntarget + t)*n + i], beta[(k*ntarget + t)*K + b]    as matinv_trend_batched
 * dBs, dCs, dHs, dYs as in matinv_trend_batched (only the lower triangle of B read; dCs may be NULL); dDMs as in
 * matinv_logml_grad_batched (matrix (k, p) at (k*nparam + p)*n*n, only its lower triangle read). Every output is optional and at least
 * one is required (all NULL: MATINV_ERR_ARG); which of them are requested does not change a bit of the others. dGrad needs nparam >= 1
 * and dDMs; without it nparam may be 0, dDMs NULL, and dDMs is not read. ntarget >= 1, dYs and dHs are always needed. 1 <= n <= 1024;
 * 1 <= nbasis <= 16 and nbasis <= n (otherwise MATINV_ERR_ARG, checked with n and dtype); ntarget <= 1024, nparam <= 1024 (beyond:
 * MATINV_ERR_UNSUPPORTED, after the pointer checks); batch < 2^31; batch == 0 is a no-op after the dtype, n and nbasis checks. No input
 * is modified (outputs must not overlap inputs); neither M, its inverse nor its factor is written to caller memory. logml, alpha and
 * beta carry the bits matinv_trend_batched gives for the same inputs. dInfo (optional): as matinv_trend_batched: 0, the 1-based column
 * of the first non-positive (or NaN) pivot of M, or n + b for the first non-positive (or NaN) pivot b of A; on a non-zero info every
 * requested output of that matrix is NaN; there is no fallback launch. n <= 96: the gradient form of the trend tile sweep: the trend
 * epilogue without queries, then U = Kinv H L_A^-T on the MFMA unit, -P = -Kinv + U U^T and G over it in the registers by rank-16 MFMA
 * updates, contracted with each dM_p streamed once (n^2/2 + n + K n + D n + nparam n^2/2 elements read, nparam + n + D + D n + D K
 * written; with D > 16 alpha is read back once, from dAlpha or from D n elements of library scratch per workgroup). Beyond, to n = 1024:
 * the trend gradient form of the global-memory Cholesky kernel on a working copy per matrix in library scratch (k-range chunks under
 * MATINV_BLOCKED_WS_MB). Asynchronous, no host synchronisation. */
int matinv_trend_grad_batched(int dtype, int n, int nbasis, int ntarget, int nparam, const void *dBs, const void *dCs, const void *dHs,
                              const void *dYs, const void *dDMs, void *dGrad, void *dGradC, void *dLogml, void *dAlpha, void *dBeta,
                              size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function a trend gradient request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_trend_grad_kernel_name(int dtype, int n);
/* Host-pointer form (packed; hCs, `info` and each output optional; hDMs is read only with hGrad). Synchronous. */
int matinv_trend_grad_batched_host(int dtype, int n, int nbasis, int ntarget, int nparam, const void *hBs, const void *hCs, const void *hHs,
                                   const void *hYs, const void *hDMs, void *hGrad, void *hGradC, void *hLogml, void *hAlpha, void *hBeta,
                                   size_t batch, int *info);

/* Leave-one-out cross-validation of the trend model (universal kriging), device-resident: all n held-out predictions of every target from
 * one factorisation (Dubrule's identities; Rasmussen & Williams 5.4.2 with the trend's projection). With M_k = B_k + diag(c_k),
 * Kinv = M_k^-1, H the K = nbasis basis vectors, A = H^T Kinv H, P = Kinv - Kinv H A^-1 H^T Kinv, D = ntarget targets y_kt and
 * alpha_t = P y_kt:
 *   var[k*n + i]                = 1 / P_ii                          predictive variance of observation i from the other n - 1 (its noise
 *                                                                    c_i and the uncertainty of the trend coefficients included)
 *   mean[(k*ntarget + t)*n + i] = y_ti - alpha_ti / P_ii            predictive mean of target t at point i from the other n - 1
 *   logpl[k*ntarget + t]        = sum_i (1/2 log P_ii - 1/2 alpha_ti^2 / P_ii) - n/2 log 2 pi     = sum_i log N(y_ti; mean_ti, var_i)
 * dBs, dCs, dHs, dYs as in matinv_trend_batched (only the lower triangle of B read; dCs may be NULL; basis vector (k, b) at
 * (k*nbasis + b)*n, target (k, t) at (k*ntarget + t)*n). Every output is optional and at least one is required (all NULL: MATINV_ERR_ARG).
 * var depends on M and H only: a call with ntarget = 0 and dYs = dMean = dLogPL = NULL is valid and reads no Y; dMean and dLogPL need
 * ntarget >= 1 and dYs (otherwise MATINV_ERR_ARG). 1 <= nbasis <= 16 and nbasis < n <= 1024: with n <= nbasis no held-out fit exists
 * (MATINV_ERR_ARG, checked with n and dtype); n > 1024 and ntarget > 1024: MATINV_ERR_UNSUPPORTED, after the pointer checks;
 * batch < 2^31; batch == 0 is a no-op after the dtype, n and nbasis checks. No input is modified (outputs must not overlap inputs).
 * No bit of a result depends on the batch, on the grid or on which outputs are requested; for mean and logpl no bit depends on ntarget or
 * on the other targets; var does not depend on Y at all.
 * dInfo (optional): 0; or the 1-based column of the first non-positive (or NaN) pivot of M; or n + b for the first non-positive (or NaN)
 * pivot b of A -- both exactly the values matinv_trend_batched reports for the same B, c, H; or n + nbasis + i for the first point i
 * (1-based) whose computed P_ii is not > 0 (<= 0 or NaN): holding i out leaves the basis rank deficient (in exact arithmetic e_i lies in
 * the span of H). On a non-zero info every requested output of that matrix is NaN; there is no fallback launch. A tiny positive P_ii is
 * returned as it is and gives a huge variance: the caller judges it.
 * n <= 96: the leave-one-out form of the trend tile sweep: the trend epilogue up to the factor of A, then U = Kinv H L_A^-T on the MFMA
 * unit and only the diagonal of P, P_ii = Kinv_ii - sum_b U_ib^2 (n^2/2 + n + K n + D n elements read, n + D n + D written). Beyond, to
 * n = 1024: the trend leave-one-out form of the global-memory Cholesky kernel on a working copy per matrix in library scratch (k-range
 * chunks under MATINV_BLOCKED_WS_MB); correct first, not fast. Asynchronous, no host synchronisation. */
int matinv_trend_loo_batched(int dtype, int n, int nbasis, int ntarget, const void *dBs, const void *dCs, const void *dHs, const void *dYs,
                             void *dMean, void *dVar, void *dLogPL, size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function a trend leave-one-out request launches ("" for a request that would be refused: n < 2, n > 1024, an
 * unknown dtype). Pure host logic. */
const char *matinv_trend_loo_kernel_name(int dtype, int n);
/* Host-pointer form (packed; hCs, `info` and each output optional; hYs is read only with hMean or hLogPL). Synchronous. */
int matinv_trend_loo_batched_host(int dtype, int n, int nbasis, int ntarget, const void *hBs, const void *hCs, const void *hHs,
                                  const void *hYs, void *hMean, void *hVar, void *hLogPL, size_t batch, int *info);

/* GP log marginal likelihood and its gradient FROM COORDINATES, device-resident: the covariance matrix of every batch member is generated
 * inside the kernel from its n points in ndim dimensions and its ndim + 2 hyperparameters; neither it, nor its inverse, nor a derivative
 * matrix reaches memory. Per matrix k: points x_i (element (i, d) at dXs[k*xstride + i*ndim + d]), targets y (dYs[k*ystride + i]) and
 * theta = (log sf2, log l_1 .. log l_ndim, log sn2) at dThetas[k*(ndim + 2)]. With z_id = x_id / l_d and s_ij = sum_d (z_id - z_jd)^2,
 * summed in the order d = 0 .. ndim - 1:
 *   M_ij = sf2 phi(s_ij) + sn2 delta_ij        K = M^-1,  alpha = K y,  G = alpha alpha^T - K
 *   MATINV_COV_SE:        phi(s) = exp(-s/2)                                      psi(s) = phi(s)
 *   MATINV_COV_MATERN52:  phi(s) = (1 + sqrt5 r + 5 s / 3) exp(-sqrt5 r), r = sqrt s   psi(s) = 5/3 (1 + sqrt5 r) exp(-sqrt5 r)
 *   logml[k]                  = -1/2 y^T alpha - 1/2 log det M - n/2 log 2 pi
 *   grad[k*(ndim+2)]          = 1/2 sum_ij G_ij sf2 phi(s_ij)                           d logml / d log sf2
 *   grad[k*(ndim+2) + 1 + d]  = 1/2 sum_ij G_ij sf2 psi(s_ij) (z_id - z_jd)^2           d logml / d log l_d       (psi = -2 phi')
 *   grad[k*(ndim+2) + ndim+1] = 1/2 sn2 sum_i G_ii                                      d logml / d log sn2
 *   alpha[k*n + i]            = alpha_i
 * xstride is n*ndim, or 0 for one point set shared by the whole batch; ystride is n, or 0 likewise; any other stride: MATINV_ERR_ARG.
 * dThetas is always per matrix. dLogML: batch, dGrad: batch*(ndim + 2), dAlpha: batch*n elements; each may be NULL (all three NULL:
 * MATINV_ERR_ARG), and which of them are requested does not change a bit of the others. The result for matrix k depends on matrix k's
 * inputs alone: no bit depends on the batch, the grid or the strides. 1 <= n <= 1024; 1 <= ndim <= 16 (0 or less: MATINV_ERR_ARG, beyond 16:
 * MATINV_ERR_UNSUPPORTED); batch < 2^31; batch == 0 is a no-op after the dtype, n, kind and ndim checks. No input is modified.
 * dInfo (optional): 0, or the 1-based column of the first non-positive (or NaN) leading pivot of M in natural order; every requested
 * output of that matrix is then NaN. There is no fallback launch.
 * n <= 96: the ARD form of the one-wavefront SPD tile sweep: every lane generates the accumulator elements it owns from z in LDS, the
 * epilogue regenerates them once more for the contraction (n ndim + n + ndim + 2 elements read, ndim + 3 + n written). Beyond, to
 * n = 1024: the ARD form of the global-memory Cholesky kernel, which generates into its working copy in library scratch (k-range chunks
 * under MATINV_BLOCKED_WS_MB); correct first, not fast. Asynchronous, no host synchronisation. */
enum {
    MATINV_COV_SE = 0,       /* squared exponential with one length scale per dimension */
    MATINV_COV_MATERN52 = 1  /* Matern 5/2, likewise */
};
int matinv_ard_logml_batched(int dtype, int kind, int n, int ndim, const void *dXs, size_t xstride, const void *dYs, size_t ystride,
                             const void *dThetas, void *dLogML, void *dGrad, void *dAlpha, size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function such a request launches ("" for a request that would be refused: n < 1, n > 1024, an unknown dtype or
 * kind). Pure host logic. */
const char *matinv_ard_logml_kernel_name(int dtype, int kind, int n);
/* Host-pointer form (`info` and each output optional; a shared point set or target vector, stride 0, is staged once). Synchronous. */
int matinv_ard_logml_batched_host(int dtype, int kind, int n, int ndim, const void *hXs, size_t xstride, const void *hYs, size_t ystride,
                                  const void *hThetas, void *hLogML, void *hGrad, void *hAlpha, size_t batch, int *info);

/* GP prediction FROM COORDINATES, device-resident: the counterpart of matinv_ard_logml_batched once theta is fitted. The covariance
 * matrix of every batch member AND the cross-covariance vectors of its nquery query points are generated inside the kernel; neither they
 * nor the inverse reach memory. Per matrix k: X, y, theta, z = x / l, s, phi and M = sf2 phi(s) + sn2 I exactly as
 * matinv_ard_logml_batched defines them, K = M^-1, alpha = K y; query j's coordinate d at dXqs[k*xqstride + j*ndim + d], zq_jd =
 * xq_jd / l_d:
 *   a_j[i]               = sf2 phi(sum_d (z_id - zq_jd)^2)        summed in the order d = 0 .. ndim - 1
 *   mean[k*nquery + j]   = a_j^T alpha
 *   var[k*nquery + j]    = sf2 - a_j^T K a_j
 * var is the variance of the LATENT function; the variance of a noisy observation is var + exp(theta[ndim + 1]), which the caller adds.
 * var is not clamped: where rounding outweighs a tiny variance it can come out slightly negative. A query that coincides with a
 * training point has s = 0 and a_j[i] = sf2 phi(0) exactly (no noise term: sn2 belongs to M's diagonal alone).
 * xstride and ystride as in matinv_ard_logml_batched; xqstride is nquery*ndim, or 0 for one query set shared by the whole batch; any
 * other stride: MATINV_ERR_ARG. dThetas is always per matrix. dMean, dVar: batch*nquery elements; each may be NULL (both NULL:
 * MATINV_ERR_ARG), and which of them are requested does not change a bit of the other. dYs is read with dMean only and may be NULL
 * without it (dMean without dYs: MATINV_ERR_ARG). The result for matrix k depends on matrix k's inputs alone: no bit depends on the
 * batch, the grid or the strides; query j's result does not depend on nquery, on the other queries or on its position among them.
 * nquery >= 1 (MATINV_ERR_ARG otherwise; no upper limit); 1 <= n <= 1024; 1 <= ndim <= 16 (0 or less: MATINV_ERR_ARG, beyond 16:
 * MATINV_ERR_UNSUPPORTED); batch < 2^31; batch == 0 is a no-op after the dtype, n, kind and ndim checks. No input is modified.
 * dInfo (optional): 0, or the 1-based column of the first non-positive (or NaN) leading pivot of M in natural order -- the value
 * matinv_ard_logml_batched reports for the same X, theta; every requested output of that matrix is then NaN. There is no fallback
 * launch. A NaN in a QUERY's coordinates makes that query's outputs NaN and changes neither info nor a bit of any other query.
 * n <= 96: the ARD prediction form of the one-wavefront tile sweep: generation and sweep of the ARD form, then the queries in groups of
 * 16 whose cross-covariance block is generated in LDS and multiplied on the MFMA unit (n ndim + n + ndim + 2 + nquery ndim elements
 * read, 2 nquery written). Beyond, to n = 1024: a global-memory Cholesky kernel that generates into its working copy in library scratch
 * (k-range chunks under MATINV_BLOCKED_WS_MB) and takes one query at a time; correct first, not fast. Asynchronous, no host
 * synchronisation. */
int matinv_ard_predict_batched(int dtype, int kind, int n, int ndim, int nquery, const void *dXs, size_t xstride, const void *dYs,
                               size_t ystride, const void *dThetas, const void *dXqs, size_t xqstride, void *dMean, void *dVar, size_t batch,
                               int *dInfo, void *stream);
/* Name of the __global__ function such a request launches ("" for a request that would be refused: n < 1, n > 1024, an unknown dtype or
 * kind). Pure host logic. */
const char *matinv_ard_predict_kernel_name(int dtype, int kind, int n);
/* Host-pointer form (`info` and each output optional; a shared point set, target vector or query set, stride 0, is staged once; hYs is
 * read only with hMean). Synchronous. */
int matinv_ard_predict_batched_host(int dtype, int kind, int n, int ndim, int nquery, const void *hXs, size_t xstride, const void *hYs,
                                    size_t ystride, const void *hThetas, const void *hXqs, size_t xqstride, void *hMean, void *hVar,
                                    size_t batch, int *info);

/* Joint posterior samples of a GP at its query points, device-resident: with mean_k and cov_k as matinv_predict_cov_batched returns them
 * for the same dBs, dCs, dDs, dAs, dEs,
 *   Y_k[:, s] = mean_k + chol(cov_k) z_ks      dZs, dY: batch*nquery*nsample elements, laid out as in matinv_colour_batched
 * It is two launches: the predictive-covariance route for this n, then the colour route for nquery (their kernels are named by
 * matinv_predict_cov_kernel_name(dtype, n) and matinv_colour_kernel_name(dtype, nquery)). dMean (batch*nquery) and dCov
 * (batch*nquery^2) are optional extra outputs and carry the bits of matinv_predict_cov_batched; Y carries the bits of
 * matinv_colour_batched on that cov and mean, whether or not they are requested (what is not requested lives in library scratch, in
 * k-range chunks under MATINV_BLOCKED_WS_MB). dDs == NULL means the zero-mean posterior: Y = chol(cov) z, and dMean must then be NULL
 * too. n, nquery, nsample <= 1024 (beyond: MATINV_ERR_UNSUPPORTED). dInfo (optional): 0; the 1-based column (1 .. n) of the first
 * non-positive pivot of M -- every output of that matrix is then NaN; or n + j when column j of cov has the first non-positive pivot --
 * Y is then NaN while mean and cov stay valid. There is no jitter parameter: E is the caller's, and jitter goes on its diagonal.
 * Asynchronous, no host synchronisation. */
int matinv_sample_batched(int dtype, int n, int nquery, int nsample, const void *dBs, const void *dCs, const void *dDs, const void *dAs,
                          const void *dEs, const void *dZs, void *dY, void *dMean, void *dCov, size_t batch, int *dInfo, void *stream);
/* Host-pointer form (packed; hCs, hDs, hEs, hMean, hCov and `info` optional). Synchronous. */
int matinv_sample_batched_host(int dtype, int n, int nquery, int nsample, const void *hBs, const void *hCs, const void *hDs, const void *hAs,
                               const void *hEs, const void *hZs, void *hY, void *hMean, void *hCov, size_t batch, int *info);

/* Gradients of the GP leave-one-out log pseudo-likelihood (the logpl matinv_loo_batched returns; Rasmussen & Williams 5.4.2),
 * device-resident. With M_k = B_k + diag(c_k), K = M^-1, alpha = K d, kappa_i = K_ii and nparam symmetric derivative matrices
 * dM_p = dM / d theta_p per matrix:
 *   b_i = alpha_i / kappa_i,  beta = K b,  s_i = (1 + alpha_i^2 / kappa_i) / kappa_i,  H = K diag(s) K,
 *   G = 1/2 (alpha beta^T + beta alpha^T) - 1/2 H
 *   grad[k*nparam + p] = sum_ij G_ij dM_p[i][j]                                                  d logpl / d theta_p
 *   gradc[k*n + i]     = G_ii = alpha_i beta_i - 1/2 sum_t s_t K_it^2                            d logpl / d c_i
 *   logpl[k]           = sum_i (1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i) - n/2 log(2 pi)       the value itself
 * B, c, d and dDMs as in matinv_logml_grad_batched (SPD, column-major, only the lower triangles of B and of every dM_p read; dCs may be
 * NULL; matrix (k, p) of dDMs at offset (k*nparam + p)*n*n). dGrad: batch*nparam, dGradC: batch*n, dLogPL: batch; each may be NULL (all
 * three NULL: MATINV_ERR_ARG), and which of them are requested does not change a bit of the others. dGrad needs nparam >= 1 and dDMs;
 * without dGrad, nparam = 0 and dDMs = NULL are fine (dDMs is not read). No input is modified (outputs must not overlap inputs);
 * neither M, its inverse nor H is written to caller memory; the result of matrix k depends on matrix k alone, and grad[k, p] on dM_p
 * alone, bit for bit. dInfo (optional): 0, or the 1-based column of the first non-positive (or NaN) pivot -- every output of that
 * matrix is then NaN. n <= 96: the LOO-gradient form of the one-wavefront SPD tile sweep, H built one tile column at a time on the MFMA
 * unit ((nparam + 1) n^2/2 + 2n elements read, nparam + n + 1 written). Beyond, to n = 1024: the LOO-gradient form of the
 * global-memory Cholesky kernel on a working copy of 2 n^2 elements per matrix in library scratch. Asynchronous, no host
 * synchronisation. */
int matinv_loo_grad_batched(int dtype, int n, int nparam, const void *dBs, const void *dCs, const void *dDs, const void *dDMs, void *dGrad,
                            void *dGradC, void *dLogPL, size_t batch, int *dInfo, void *stream);
/* Name of the __global__ function a LOO-gradient request launches ("" for a request that would be refused). Pure host logic. */
const char *matinv_loo_grad_kernel_name(int dtype, int n);
/* Host-pointer form (packed; hCs, `info` and each output optional; hDMs is read only with hGrad). Synchronous. */
int matinv_loo_grad_batched_host(int dtype, int n, int nparam, const void *hBs, const void *hCs, const void *hDs, const void *hDMs,
                                 void *hGrad, void *hGradC, void *hLogPL, size_t batch, int *info);

/* Host-pointer convenience used by the reference-named *_gpu wrappers: allocate, H2D, invert, D2H, free.
 * `info` is an optional host int[batch]. Synchronous. */
int matinv_inverse_batched_host(int algo, int dtype, int n, const void *hA, void *hAinv, size_t batch, int *info);

/* The same over SEVERAL devices of this process (one node): the batch is cut into `nshards` contiguous blocks of
 * ceil(batch / nshards) matrices (rounded up to the per-wavefront packing of the small-n kernels: 8 for n <= 8, 4 for n <= 16),
 * shard g runs on device g mod (number of gfx950 devices) on its own host thread with its own streams and its own host link
 * -- no collective: the result goes back to host memory. nshards <= 0: one shard per visible device. More shards than
 * devices is allowed ("virtual shards": several per device). The bits of every matrix are those of the single-device call.
 * The reference-named *_batched_gpu entry points take this path with nshards = MATINV_DEVICES when that variable is > 1. */
int matinv_inverse_batched_host_multi(int algo, int dtype, int n, const void *hA, void *hAinv, size_t batch, int *info,
                                      int nshards);
int matinv_device_count(void); /* visible gfx950 devices, or a negative status */
/* The block of shard g of nshards: [*lo, *hi) (pure host arithmetic, no device needed; the same partition as shard.py). */
int matinv_shard_range(size_t batch, int nshards, int n, int g, size_t *lo, size_t *hi);

/* Reassembly of device-resident shards over RCCL (librccl is opened at the first call: no link-time dependency). Every rank
 * contributes `count` elements (pad the short tail shard) and receives nranks * count.
 *   one process per GPU: matinv_comm_unique_id on rank 0 -> ship the 128 bytes to the others by any means ->
 *                        matinv_comm_init_rank everywhere -> matinv_allgather_shards(comm, ...) on each rank's stream;
 *   one process, several GPUs: matinv_allgather_local(ndev, devices, ...) (communicators created once and cached). It runs on
 *                        the library's own streams and returns when the gather has completed. Input readiness:
 *                        matinv_allgather_local synchronises every listed device on entry (whatever was enqueued there before the
 *                        call has finished when the gather reads dSend[g]); matinv_allgather_local_after takes, per device, the
 *                        stream whose work so far produces dSend[g] (0 = that device's null stream) and makes the gather wait
 *                        for an event recorded on it instead -- no host-side synchronisation of the producers. */
int matinv_comm_unique_id(void *id128);
int matinv_comm_init_rank(void **comm, int nranks, const void *id128, int rank);
int matinv_comm_destroy(void *comm);
int matinv_allgather_shards(void *comm, int dtype, const void *dSend, void *dRecv, size_t count, void *stream);
int matinv_allgather_local(int ndev, const int *devices, int dtype, const void *const *dSend, void *const *dRecv, size_t count);
int matinv_allgather_local_after(int ndev, const int *devices, int dtype, const void *const *dSend, void *const *dRecv, size_t count,
                                 void *const *producer_streams);

/* Host-pointer form of the fused pipeline (what gauss_bench times): H2D, one kernel, D2H of `batch` scalars.
 * Inputs are NOT modified (the reference CPU path destroys Bs and Cs, include/gauss_cpu.h:42 there). Synchronous. */
int matinv_mean_batched_host(int dtype, int n, const void *hAs, const void *hBs, const void *hCs, const void *hDs,
                             void *hMeans, size_t batch, int *info);
int matinv_variance_batched_host(int dtype, int n, const void *hAs, const void *hBs, const void *hCs, const void *hEs,
                                 void *hVars, size_t batch, int *info);

/* The reference's batch allocator (batchedCudaMalloc, src/helper.cu:103-118; declared include/helper_gpu.h:4): ONE pitched
 * device allocation of batchSize rows of arraySize BYTES; devArrayPtr (host array of batchSize pointers, caller-owned)
 * receives the row addresses, *pitch the row pitch in bytes (a multiple of 256, so of sizeof(double)). The tables are what
 * the *_batched_device entry points of inverse_gpu.h take. matinv_batched_free releases the block behind devArrayPtr[0]. */
int matinv_batched_malloc(void **devArrayPtr, size_t *pitch, size_t arraySize, int batchSize);
int matinv_batched_free(void **devArrayPtr);
/* cudaMemcpy2D as the reference uses it on those blocks (src/gauss_bench.cu:165-170,244): width bytes x height rows,
 * blocking. toDevice != 0: host -> device, else device -> host. Lets a plain-C caller stage data without HIP headers. */
int matinv_memcpy_2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, int toDevice);
int matinv_device_synchronize(void);
/* Counters of the tile family's Gauss-Jordan dispatch since load: launches that started with the natural-order kernel /
 * went straight to the pivoting kernel, and -- MATINV_GJ_ADAPTIVE only -- the reject count / batch of the last natural-order
 * launch whose count has come back (call matinv_device_synchronize first for an exact figure). Any pointer may be NULL. */
int matinv_tile_stats(unsigned long long *natural_launches, unsigned long long *pivot_launches, unsigned long long *last_rejected,
                      unsigned long long *last_batch);
/* Unscreened 64 x 64 fp64 Gauss-Jordan launches since load: those that ran the symmetric-only kernel in front of the two-arm kernel /
 * the two-arm kernel alone, and how many matrices the last front launch whose count has come back found not symmetric, of how many
 * (call matinv_device_synchronize first for an exact figure). The route never changes a result. Any pointer may be NULL. */
int matinv_sym_front_stats(unsigned long long *front_launches, unsigned long long *direct_launches, unsigned long long *last_not_symmetric,
                           unsigned long long *last_batch);

/* Size-binned multi-queue for mixed-size pipeline items (the reference sketches it, README.md:41-44: "use multiple queues
 * for different sizes: 32, 128, 512, 1024"; BASELINE configs[4]). Items of any n <= the largest bin are submitted as
 * chunks of `count` equally sized items lying back to back in device memory (As, Cs, Ds: count*n; Bs: count*n*n
 * column-major; Es: count scalars or NULL); submit only records the chunk and hands out consecutive tickets. flush runs
 * the largest pending bin on one HIP stream and the other bins on a second (forked from and joined back into `stream`; or
 * everything in the queue's own stream: matinv_queue_stream), one launch of the fused mean (and variance) kernel per distinct n of a bin -- the kernels pad a matrix to their tile size in registers, nothing is padded in memory --
 * gathering a group's chunks with one segmented-copy kernel unless they already form one contiguous run, and writes
 * means[ticket] (and variances[ticket] when dVariances != NULL, which needs every item to carry e). Asynchronous; the
 * item memory must stay valid until the work in `stream` has completed. bins == NULL / nbins == 0: {32, 128, 512, 1024}. */
typedef struct matinv_queue matinv_queue;
int matinv_queue_create(matinv_queue **q, int dtype, const int *bins, int nbins);
int matinv_queue_submit(matinv_queue *q, int n, const void *dAs, const void *dBs, const void *dCs, const void *dDs,
                        const void *dEs, size_t count, size_t *first_ticket);
/* the same for `chunks` chunks in one call (arrays of `chunks` entries; dEs NULL = no item carries e) */
int matinv_queue_submit_chunks(matinv_queue *q, size_t chunks, const int *n, const void *const *dAs, const void *const *dBs,
                               const void *const *dCs, const void *const *dDs, const void *const *dEs, const size_t *count,
                               size_t *first_tickets);
int matinv_queue_pending(const matinv_queue *q, size_t *items, size_t *per_bin);
int matinv_queue_bins(const matinv_queue *q, int *bins, int cap);
int matinv_queue_flush(matinv_queue *q, void *dMeans, void *dVariances, void *stream);
/* The queue's own stream (a hipStream_t; non-blocking), created with the queue. A flush issued ON it (pass it as `stream`) runs in it from
 * end to end, largest bin first: no fork, no join -- nothing in such a flush waits for another stream. HIP multiplexes the streams of a
 * process onto four hardware queues (a new stream goes to the least used one): four queues created at start-up, before the process
 * creates other streams, and used alternately overlap their flushes completely (bench.py, mixed workload: 0.93 / 0.59 / 0.47 / 0.41 ms
 * per step with 1 / 2 / 3 / 4 flushes in flight). A flush issued on any OTHER stream (the null stream included) forks the launch chain
 * of its largest bin into a second stream of the queue beside the other bins and joins both back: the shorter latency for one flush by
 * itself (0.75 ms), and at the mercy of the process's other streams when several are in flight. The caller orders its own work after
 * a flush on the own stream with an event recorded on it. */
void *matinv_queue_stream(matinv_queue *q);
int matinv_queue_destroy(matinv_queue *q);
const char *matinv_queue_last_error(const matinv_queue *q);

const char *matinv_last_error(void);
int matinv_abi_version(void);

/* The host-pointer entry points (and the work lists / workspaces of the kernels) take their device scratch memory from a cache
 * inside the library, keyed by (device, stream) -- a block is reused on the stream it was first handed out on only, so
 * stream order makes the reuse safe -- and leave it there between calls: the reference's "allocate and free inside every
 * call" (src/gauss/batched_invert.cu:120-176) without its cost. The device's default memory pool is not touched. An
 * allocation that fails for lack of memory empties the cache and is tried once more. This call synchronises the current
 * device and hands everything that is not in use back to the driver.
 * Returns MATINV_OK, or MATINV_ERR_HIP / MATINV_ERR_NO_DEVICE. Never needed for correctness. */
int matinv_release_cache(void);
/* A caller that is about to destroy one of ITS streams on which it has called this library: synchronises the stream and hands the
 * scratch blocks cached for it (work lists, blocked-path workspaces: they are kept per (device, stream) and reused on that stream
 * only) to the other streams of its device. Without it they stay cached until matinv_release_cache() or memory runs out. */
int matinv_stream_retire(void *stream);

/* Test hook. With MATINV_DEBUG_REJECTS=1 in the environment when the library is loaded, every launcher whose first-pass kernel
 * hands rejected matrices (needs row exchanges / not positive definite / singular) to a second kernel through a work list reads
 * that list's length back after the launch (one stream synchronisation per launch: a test mode) and adds it to a running total.
 * Returns the total; reset != 0 also zeroes it. Without the environment variable: always 0. The results never show whether
 * the fast kernel or its fallback produced them -- the tests use this to pin "a well-conditioned batch is never rejected". */
long long matinv_debug_rejects(int reset);

#ifdef __cplusplus
}
#endif
#endif
