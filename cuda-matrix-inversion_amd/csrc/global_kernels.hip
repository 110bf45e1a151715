// global_kernels.hip -- kernel family "GLOBAL": any n up to 1024 (the reference's own limit: one thread per row,
// /root/reference/src/gauss/batched_invert.cu:87-93), for sizes whose matrix no longer fits on chip (n > 137 in f64,
// n > 200 in f32). One 1024-thread workgroup per matrix; the n x n working copy lives in the OUTPUT buffer (global memory,
// L2 / Infinity-Cache resident for the sizes in question) and only the pivot row and multiplier column of the current
// step are staged in LDS. Same arithmetic as the LDS family:
//   matinv_gj_global    in-place Gauss-Jordan with partial pivoting,
//   matinv_chol_global  Cholesky factor, in-place triangular inverse, L^-T L^-1 (SPD input, lower triangle read).
// It is a functional path (2 n^3 * sizeof(T) bytes of cache traffic per matrix), not a tuned one: the blocked, MFMA-based
// large-n path is listed as next in DESIGN.md.
#include "ard_element.hpp"
#include "common.hpp"
#include "pivot_product.hpp"

namespace matinv {

constexpr int GL_THREADS = 1024;

template <class T>
__device__ __forceinline__ T gl_abs(T v) { return v < 0 ? -v : v; }
template <class T>
__device__ __forceinline__ T gl_sqrt(T v);
template <>
__device__ __forceinline__ double gl_sqrt<double>(double v) { return sqrt(v); }
template <>
__device__ __forceinline__ float gl_sqrt<float>(float v) { return sqrtf(v); }

template <class T>
__device__ __forceinline__ void gl_fill_nan(T *X, int n)
{
    for (size_t e = threadIdx.x; e < (size_t)n * n; e += GL_THREADS) X[e] = nan_of<T>();
}

// block-wide arg-max of (val, idx); lowest index wins ties. Result broadcast to every thread.
template <class T>
__device__ __forceinline__ void gl_argmax(T &best, int &bi, T *s_val, int *s_idx)
{
    for (int off = 32; off >= 1; off >>= 1) {
        T ob = __shfl_down(best, off);
        int oi = __shfl_down(bi, off);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_val[w] = best; s_idx[w] = bi; }
    __syncthreads();
    best = s_val[0];
    bi = s_idx[0];
    for (int k = 1; k < GL_THREADS / 64; ++k) {
        T ob = s_val[k];
        int oi = s_idx[k];
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    __syncthreads();
}

template <class T>
__global__ __launch_bounds__(GL_THREADS) void matinv_gj_global(BatchRef<const T> Ain, BatchRef<T> Xout, int *info, int n)
{
    __shared__ T prow[1024], mcol[1024];
    __shared__ T s_val[GL_THREADS / 64];
    __shared__ int s_idx[GL_THREADS / 64];
    __shared__ int piv[1024];
    const size_t k_mat = blockIdx.x;
    const T *A = Ain.at_uniform(k_mat);
    T *X = Xout.at_uniform(k_mat);
    const int t = threadIdx.x;
    const size_t nn = (size_t)n * n;

    if (A != X)
        for (size_t e = t; e < nn; e += GL_THREADS) X[e] = A[e];
    __syncthreads();

    for (int k = 0; k < n; ++k) {
        T best = (T)-1;
        int bi = k;
        for (int i = k + t; i < n; i += GL_THREADS) {
            const T v = gl_abs(X[(size_t)k * n + i]);
            if (v > best) { best = v; bi = i; }
        }
        gl_argmax(best, bi, s_val, s_idx);
        const int p = bi;
        if (!(best > 0)) {
            if (info && t == 0) info[k_mat] = k + 1;
            __syncthreads();
            gl_fill_nan(X, n);
            return;
        }
        for (int c = t; c < n; c += GL_THREADS) {  // swap rows k <-> p, lift the pivot row
            const T vp = X[(size_t)c * n + p], vk = X[(size_t)c * n + k];
            X[(size_t)c * n + p] = vk;
            prow[c] = vp;
        }
        if (t == 0) piv[k] = p;
        __syncthreads();
        const T inv = (T)1 / prow[k];
        for (int i = t; i < n; i += GL_THREADS) mcol[i] = (i == k) ? (T)0 : X[(size_t)k * n + i];
        __syncthreads();
        for (size_t e = t; e < nn; e += GL_THREADS) {
            const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
            const T pr = (c == k) ? inv : prow[c] * inv;
            T v;
            if (r == k) v = pr;
            else if (c == k) v = -mcol[r] * inv;
            else v = X[e] - mcol[r] * pr;
            X[e] = v;
        }
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {  // undo the row swaps as column swaps, last first
        const int p = piv[k];
        if (p != k)
            for (int i = t; i < n; i += GL_THREADS) {
                const T a = X[(size_t)k * n + i];
                X[(size_t)k * n + i] = X[(size_t)p * n + i];
                X[(size_t)p * n + i] = a;
            }
        __syncthreads();
    }
    if (info && t == 0) info[k_mat] = 0;
}

// Cholesky pieces on a global-memory matrix W (lower triangle significant)
template <class T>
__device__ __forceinline__ int gl_chol_factor(T *W, int n, T *col)
{
    const int t = threadIdx.x;
    for (int k = 0; k < n; ++k) {
        const T d = W[(size_t)k * n + k];
        if (!(d > 0)) return k + 1;  // block-uniform (read after the barrier below / the initial one)
        const T sd = gl_sqrt<T>(d), rs = (T)1 / sd;
        __syncthreads();
        for (int i = k + t; i < n; i += GL_THREADS) {
            const T v = (i == k) ? sd : W[(size_t)k * n + i] * rs;
            W[(size_t)k * n + i] = v;
            col[i] = v;
        }
        __syncthreads();
        const size_t m = (size_t)(n - k - 1);
        for (size_t e = t; e < m * m; e += GL_THREADS) {  // trailing lower triangle: (i, j), j >= k+1, i >= j
            const int j = k + 1 + (int)(e / m), i = k + 1 + (int)(e % m);
            if (i >= j) W[(size_t)j * n + i] -= col[i] * col[j];
        }
        __syncthreads();
    }
    return 0;
}

template <class T>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(BatchRef<const T> Ain, BatchRef<T> Xout, int *info, int n,
                                                                 T *workspace)
{
    __shared__ T col[1024];
    const size_t k_mat = blockIdx.x;
    const T *A = Ain.at_uniform(k_mat);
    T *X = Xout.at_uniform(k_mat);
    T *W = workspace + k_mat * (size_t)n * n;  // factor / triangular inverse (X receives the product)
    const int t = threadIdx.x;
    const size_t nn = (size_t)n * n;
    for (size_t e = t; e < nn; e += GL_THREADS) W[e] = A[e];
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {
        if (info && t == 0) info[k_mat] = bad;
        gl_fill_nan(X, n);
        return;
    }
    for (int j = n - 1; j >= 0; --j) {  // L <- L^-1 in place, last column first
        const T ajj = (T)1 / W[(size_t)j * n + j];
        for (int i = j + 1 + t; i < n; i += GL_THREADS) col[i] = W[(size_t)j * n + i];
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += GL_THREADS) {
            T s = 0;
            for (int k = j + 1; k <= i; ++k) s += W[(size_t)k * n + i] * col[k];
            W[(size_t)j * n + i] = -s * ajj;
        }
        if (t == 0) W[(size_t)j * n + j] = ajj;
        __syncthreads();
    }
    for (size_t e = t; e < nn; e += GL_THREADS) {  // X = L^-T L^-1
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        T s = 0;
        for (int k = (r > c ? r : c); k < n; ++k) s += W[(size_t)r * n + k] * W[(size_t)c * n + k];
        X[e] = s;
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
bool global_family_supports(int n) { return n >= 1 && n <= 1024; }
template bool global_family_supports<double>(int);
template bool global_family_supports<float>(int);

template <class T>
hipError_t launch_gj_global(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    hipLaunchKernelGGL(matinv_gj_global<T>, dim3((unsigned)batch), dim3(GL_THREADS), 0, stream, A, X, info, n);
    return hipGetLastError();
}

template <class T>
hipError_t launch_chol_global(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), batch * (size_t)n * n * sizeof(T), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(matinv_chol_global<T>, dim3((unsigned)batch), dim3(GL_THREADS), 0, stream, A, X, info, n, ws);
    e = hipGetLastError();
    hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

#define INST(T)                                                                                                        \
    template hipError_t launch_gj_global<T>(int, BatchRef<const T>, BatchRef<T>, size_t, int *, hipStream_t);         \
    template hipError_t launch_chol_global<T>(int, BatchRef<const T>, BatchRef<T>, size_t, int *, hipStream_t);
INST(double)
INST(float)
#undef INST

const char *name_gj_global(bool f64) { return f64 ? "matinv_gj_global<double>" : "matinv_gj_global<float>"; }
const char *name_chol_global(bool f64) { return f64 ? "matinv_chol_global<double>" : "matinv_chol_global<float>"; }

// ---- leave-one-out cross-validation of a GP, 96 < n <= 1024 (matinv_loo_batched behind loo_tile_impl.hpp) -------------------------
// The LOO form of matinv_chol_global: an overload with one more template argument ("Leave-one-out cross-validation", says
// why it carries that name). M = B + diag c (lower triangle read, c optional) is factored in a working copy in library scratch and
// the factor inverted in place, as above; then instead of the product L^-T L^-1
//     kappa_i = sum_{k >= i} (L^-1)_ki^2,      alpha = L^-T (L^-1 d)       (two triangular products through LDS vectors)
//     mean_i = d_i - alpha_i / kappa_i,   var_i = 1 / kappa_i,   logpl = sum_i (1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i) - n/2 log(2 pi)
// so neither M nor its inverse reaches caller memory. Not SPD: info = the failing column + 1 and every output NaN. Correct first, as
// logdet_global_kernels.hip: speed is not a goal here. Workgroup blockIdx.x serves matrix first + blockIdx.x.
template <class T>
__device__ __forceinline__ T gl_log(T v);
template <>
__device__ __forceinline__ double gl_log<double>(double v) { return log(v); }
template <>
__device__ __forceinline__ float gl_log<float>(float v) { return logf(v); }

template <class T, bool LOO>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Bs, const T *Cs, const T *Ds, T *mean, T *var, T *logpl, int *info,
                                                                 int n, T *workspace, size_t first)
{
    static_assert(LOO, "the two-argument form is the leave-one-out kernel");
    __shared__ T col[1024], vd[1024], vy[1024];
    const size_t k_mat = first + blockIdx.x;
    const T *A = Bs + k_mat * (size_t)n * n;
    T *W = workspace + (size_t)blockIdx.x * n * n;
    const int t = threadIdx.x;
    const size_t nn = (size_t)n * n;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        T v = A[e];
        if (Cs && r == c) v += Cs[k_mat * n + r];
        W[e] = v;
    }
    for (int i = t; i < n; i += GL_THREADS) vd[i] = Ds[k_mat * n + i];
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {  // block-uniform
        for (int i = t; i < n; i += GL_THREADS) {
            if (mean) mean[k_mat * n + i] = nan_of<T>();
            if (var) var[k_mat * n + i] = nan_of<T>();
        }
        if (t == 0) {
            if (logpl) logpl[k_mat] = nan_of<T>();
            if (info) info[k_mat] = bad;
        }
        return;
    }
    for (int j = n - 1; j >= 0; --j) {  // L <- L^-1 in place, last column first (the loop of the inverse kernel)
        const T ajj = (T)1 / W[(size_t)j * n + j];
        for (int i = j + 1 + t; i < n; i += GL_THREADS) col[i] = W[(size_t)j * n + i];
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += GL_THREADS) {
            T s = 0;
            for (int k = j + 1; k <= i; ++k) s += W[(size_t)k * n + i] * col[k];
            W[(size_t)j * n + i] = -s * ajj;
        }
        if (t == 0) W[(size_t)j * n + j] = ajj;
        __syncthreads();
    }
    // y = L^-1 d: (L^-1)_kj sits at W[j*n + k]
    for (int k = t; k < n; k += GL_THREADS) {
        T s = 0;
        for (int j = 0; j <= k; ++j) s += W[(size_t)j * n + k] * vd[j];
        vy[k] = s;
    }
    __syncthreads();
    // column i of L^-1 gives kappa_i and alpha_i
    T term = 0;
    for (int i = t; i < n; i += GL_THREADS) {
        T kappa = 0, alpha = 0;
        for (int k = i; k < n; ++k) {
            const T w = W[(size_t)i * n + k];
            kappa += w * w;
            alpha += w * vy[k];
        }
        const T rk = (T)1 / kappa;
        const T q = alpha * rk;
        if (mean) mean[k_mat * n + i] = vd[i] - q;
        if (var) var[k_mat * n + i] = rk;
        term += (T)0.5 * gl_log<T>(kappa) - (T)0.5 * alpha * q;
    }
    // block sum of the terms on a fixed tree
    col[t] = term;
    __syncthreads();
    for (int off = GL_THREADS / 2; off >= 1; off >>= 1) {
        if (t < off) col[t] += col[t + off];
        __syncthreads();
    }
    if (t == 0) {
        if (logpl) logpl[k_mat] = col[0] - (T)n * (T)0.91893853320467274178;
        if (info) info[k_mat] = 0;
    }
}

template <class T>
hipError_t launch_loo_global(int n, const T *Bs, const T *Cs, const T *Ds, T *mean, T *var, T *logpl, size_t batch, int *info,
                             hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk fit the blocked-path workspace cap (launch_logdet_global)
    const size_t mat = (size_t)n * n;
    size_t chunk = blocked_workspace_cap() / (mat * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * mat * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true>), dim3((unsigned)cnt), dim3(GL_THREADS), 0, stream, Bs, Cs, Ds, mean, var, logpl, info,
                           n, ws, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_loo_global<double>(int, const double *, const double *, const double *, double *, double *, double *, size_t, int *,
                                              hipStream_t);
template hipError_t launch_loo_global<float>(int, const float *, const float *, const float *, float *, float *, float *, size_t, int *,
                                             hipStream_t);

const char *name_loo_global(bool f64) { return f64 ? "matinv_chol_global<double, true>" : "matinv_chol_global<float, true>"; }

// ---- gradients of the GP log marginal likelihood, 96 < n <= 1024 (matinv_logml_grad_batched behind logml_grad_tile_impl.hpp) ----------
// The gradient form of matinv_chol_global: one more template argument again ("Gradients of the log marginal likelihood").
// M = B + diag c is factored in a working copy in library scratch and the factor inverted in place, as above; then
//     alpha = L^-T (L^-1 d)                                     (the two triangular products of the LOO form, while L^-1 is still there)
//     K_rc  = sum_{k >= r} (L^-1)_kr (L^-1)_kc,  r >= c         (the lower triangle of M^-1 over L^-1, one column at a time through LDS)
//     gradc_i = 1/2 (alpha_i^2 - K_ii),   grad_p = sum_{r >= c} w_rc (alpha_r alpha_c - K_rc) dM_p[r][c],  w = 1/2 on the diagonal, 1 below
// with dM_p read from caller memory (lower triangle only) and grad_p summed per thread in element order, then on a fixed LDS tree.
// Not SPD: info = the failing column + 1 and every output NaN. Correct first; speed is not a goal here. Workgroup blockIdx.x serves
// matrix first + blockIdx.x.
template <class T, bool LOO, bool GRAD>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Bs, const T *Cs, const T *Ds, const T *dMs, int nparam, T *grad,
                                                                 T *gradc, T *alpha, int *info, int n, T *workspace, size_t first)
{
    static_assert(LOO && GRAD, "the three-argument form is the log-marginal-likelihood gradient kernel");
    __shared__ T col[1024], va[1024], vy[1024];
    const size_t k_mat = first + blockIdx.x;
    const T *A = Bs + k_mat * (size_t)n * n;
    T *W = workspace + (size_t)blockIdx.x * n * n;
    const int t = threadIdx.x;
    const size_t nn = (size_t)n * n;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        T v = A[e];
        if (Cs && r == c) v += Cs[k_mat * n + r];
        W[e] = v;
    }
    for (int i = t; i < n; i += GL_THREADS) va[i] = Ds[k_mat * n + i];
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {  // block-uniform
        for (int i = t; i < n; i += GL_THREADS) {
            if (alpha) alpha[k_mat * n + i] = nan_of<T>();
            if (gradc) gradc[k_mat * n + i] = nan_of<T>();
        }
        if (grad)
            for (int p = t; p < nparam; p += GL_THREADS) grad[k_mat * nparam + p] = nan_of<T>();
        if (info && t == 0) info[k_mat] = bad;
        return;
    }
    for (int j = n - 1; j >= 0; --j) {  // L <- L^-1 in place, last column first (the loop of the inverse kernel)
        const T ajj = (T)1 / W[(size_t)j * n + j];
        for (int i = j + 1 + t; i < n; i += GL_THREADS) col[i] = W[(size_t)j * n + i];
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += GL_THREADS) {
            T s = 0;
            for (int k = j + 1; k <= i; ++k) s += W[(size_t)k * n + i] * col[k];
            W[(size_t)j * n + i] = -s * ajj;
        }
        if (t == 0) W[(size_t)j * n + j] = ajj;
        __syncthreads();
    }
    // y = L^-1 d: (L^-1)_kj sits at W[j*n + k]
    for (int k = t; k < n; k += GL_THREADS) {
        T s = 0;
        for (int j = 0; j <= k; ++j) s += W[(size_t)j * n + k] * va[j];
        vy[k] = s;
    }
    __syncthreads();
    // alpha_i = column i of L^-1 against y; it takes the place of d
    for (int i = t; i < n; i += GL_THREADS) {
        T a = 0;
        for (int k = i; k < n; ++k) a += W[(size_t)i * n + k] * vy[k];
        va[i] = a;
        if (alpha) alpha[k_mat * n + i] = a;
    }
    __syncthreads();
    // column c of K over column c of L^-1; the columns beyond c are still those of L^-1
    for (int c = 0; c < n; ++c) {
        for (int k = c + t; k < n; k += GL_THREADS) col[k] = W[(size_t)c * n + k];
        __syncthreads();
        for (int r = c + t; r < n; r += GL_THREADS) {
            T s = 0;
            if (r == c) {
                for (int k = r; k < n; ++k) s += col[k] * col[k];
            } else {
                for (int k = r; k < n; ++k) s += W[(size_t)r * n + k] * col[k];
            }
            W[(size_t)c * n + r] = s;
        }
        __syncthreads();
    }
    if (gradc)
        for (int i = t; i < n; i += GL_THREADS) gradc[k_mat * n + i] = (T)0.5 * (va[i] * va[i] - W[(size_t)i * n + i]);
    if (grad) {
        for (int p = 0; p < nparam; ++p) {
            const T *D = dMs + (k_mat * nparam + p) * nn;
            T s = 0;
            for (size_t e = t; e < nn; e += GL_THREADS) {
                const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
                if (r < c) continue;
                const T g = va[r] * va[c] - W[e];
                s += (r == c ? (T)0.5 : (T)1) * g * D[e];
            }
            // block sum on a fixed tree
            col[t] = s;
            __syncthreads();
            for (int off = GL_THREADS / 2; off >= 1; off >>= 1) {
                if (t < off) col[t] += col[t + off];
                __syncthreads();
            }
            if (t == 0) grad[k_mat * nparam + p] = col[0];
            __syncthreads();
        }
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_logml_grad_global(int n, int nparam, const T *Bs, const T *Cs, const T *Ds, const T *dMs, T *grad, T *gradc, T *alpha,
                                    size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk fit the blocked-path workspace cap (launch_loo_global)
    const size_t mat = (size_t)n * n;
    size_t chunk = blocked_workspace_cap() / (mat * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * mat * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true>), dim3((unsigned)cnt), dim3(GL_THREADS), 0, stream, Bs, Cs, Ds, dMs, nparam, grad,
                           gradc, alpha, info, n, ws, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_logml_grad_global<double>(int, int, const double *, const double *, const double *, const double *, double *, double *,
                                                     double *, size_t, int *, hipStream_t);
template hipError_t launch_logml_grad_global<float>(int, int, const float *, const float *, const float *, const float *, float *, float *,
                                                    float *, size_t, int *, hipStream_t);

const char *name_logml_grad_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true>" : "matinv_chol_global<float, true, true>";
}

// ---- GP prediction at many query points, 96 < n <= 1024 (matinv_predict_batched behind predict_tile_impl.hpp) --------------------------
// The prediction form of matinv_chol_global: one more template argument again ("Prediction at many query points").
// M = B + diag c is factored in a working copy in library scratch and the factor inverted in place, as above; then
//     alpha = L^-T (L^-1 d)                            (the two triangular products of the LOO form; only when mean is asked for)
//     per query j:  v = L^-1 a_j                       (a triangular product, a_j in an LDS vector, one thread per row)
//                   var_j = e_j - sum_k v_k^2,   mean_j = sum_k a_jk alpha_k      (both on the fixed LDS tree)
// one query after the other in an order that knows nothing of Q. Not SPD: info = the failing column + 1 and every output NaN. Correct
// first; speed is not a goal here. Workgroup blockIdx.x serves matrix first + blockIdx.x.
template <class T, bool LOO, bool GRAD, bool PREDICT>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Bs, const T *Cs, const T *Ds, const T *As, int nquery, const T *Es,
                                                                 T *mean, T *var, int *info, int n, T *workspace, size_t first)
{
    static_assert(LOO && GRAD && PREDICT, "the four-argument form is the prediction kernel");
    __shared__ T col[1024], va[1024], vy[1024], vq[1024];
    const size_t k_mat = first + blockIdx.x;
    const T *A = Bs + k_mat * (size_t)n * n;
    T *W = workspace + (size_t)blockIdx.x * n * n;
    const int t = threadIdx.x;
    const size_t nn = (size_t)n * n;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        T v = A[e];
        if (Cs && r == c) v += Cs[k_mat * n + r];
        W[e] = v;
    }
    if (mean)
        for (int i = t; i < n; i += GL_THREADS) va[i] = Ds[k_mat * n + i];
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {  // block-uniform
        for (int j = t; j < nquery; j += GL_THREADS) {
            if (mean) mean[k_mat * nquery + j] = nan_of<T>();
            if (var) var[k_mat * nquery + j] = nan_of<T>();
        }
        if (info && t == 0) info[k_mat] = bad;
        return;
    }
    for (int j = n - 1; j >= 0; --j) {  // L <- L^-1 in place, last column first (the loop of the inverse kernel)
        const T ajj = (T)1 / W[(size_t)j * n + j];
        for (int i = j + 1 + t; i < n; i += GL_THREADS) col[i] = W[(size_t)j * n + i];
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += GL_THREADS) {
            T s = 0;
            for (int k = j + 1; k <= i; ++k) s += W[(size_t)k * n + i] * col[k];
            W[(size_t)j * n + i] = -s * ajj;
        }
        if (t == 0) W[(size_t)j * n + j] = ajj;
        __syncthreads();
    }
    if (mean) {  // block-uniform
        // y = L^-1 d: (L^-1)_kj sits at W[j*n + k]
        for (int k = t; k < n; k += GL_THREADS) {
            T s = 0;
            for (int j = 0; j <= k; ++j) s += W[(size_t)j * n + k] * va[j];
            vy[k] = s;
        }
        __syncthreads();
        // alpha_i = column i of L^-1 against y; it takes the place of d
        for (int i = t; i < n; i += GL_THREADS) {
            T a = 0;
            for (int k = i; k < n; ++k) a += W[(size_t)i * n + k] * vy[k];
            va[i] = a;
        }
        __syncthreads();
    }
    for (int j = 0; j < nquery; ++j) {
        const size_t out = k_mat * nquery + j;
        const T *a = As + out * n;
        for (int i = t; i < n; i += GL_THREADS) vq[i] = a[i];
        __syncthreads();
        T sq = 0, sm = 0;
        for (int k = t; k < n; k += GL_THREADS) {
            if (var) {  // v_k = row k of L^-1 against a
                T s = 0;
                for (int i = 0; i <= k; ++i) s += W[(size_t)i * n + k] * vq[i];
                sq += s * s;
            }
            if (mean) sm += vq[k] * va[k];
        }
        // block sums on a fixed tree
        col[t] = sq;
        vy[t] = sm;
        __syncthreads();
        for (int off = GL_THREADS / 2; off >= 1; off >>= 1) {
            if (t < off) {
                col[t] += col[t + off];
                vy[t] += vy[t + off];
            }
            __syncthreads();
        }
        if (t == 0) {
            if (var) var[out] = (Es ? Es[out] : (T)0) - col[0];
            if (mean) mean[out] = vy[0];
        }
        __syncthreads();  // the next query overwrites vq, col and vy
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_predict_global(int n, int nquery, const T *Bs, const T *Cs, const T *Ds, const T *As, const T *Es, T *mean, T *var,
                                 size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk fit the blocked-path workspace cap (launch_loo_global)
    const size_t mat = (size_t)n * n;
    size_t chunk = blocked_workspace_cap() / (mat * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * mat * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true, true>), dim3((unsigned)cnt), dim3(GL_THREADS), 0, stream, Bs, Cs, Ds, As, nquery,
                           Es, mean, var, info, n, ws, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_predict_global<double>(int, int, const double *, const double *, const double *, const double *, const double *,
                                                  double *, double *, size_t, int *, hipStream_t);
template hipError_t launch_predict_global<float>(int, int, const float *, const float *, const float *, const float *, const float *, float *,
                                                 float *, size_t, int *, hipStream_t);

const char *name_predict_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true, true>" : "matinv_chol_global<float, true, true, true>";
}

// ---- joint predictive covariance between the query points, 96 < n <= 1024 (matinv_predict_cov_batched behind predict_cov_tile_impl.hpp) ---
// The covariance form of matinv_chol_global: one more template argument again ("Joint predictive covariance"). M = B + diag c
// is factored in the matrix's slice of library scratch and the factor inverted in place, as above; the slice is n (n + Q) elements, the
// last n Q of them V = L^-1 A (column-major, n x Q). Then
//     alpha, mean_j                                   (the code of the prediction form, for the same bits)
//     per query j:  V[:, j] = L^-1 a_j                (the triangular product of the prediction form, kept instead of squared and summed)
//     per pair i >= j, one thread each:  cov[i][j] = E[i][j] - sum_k V[k][i] V[k][j], k ascending; cov[j][i] = the same bits
// so the order of operations of a pair knows nothing of Q or of the pair's position. Not SPD: info = the failing column + 1 and every
// output NaN. Correct first; speed is not a goal here. Workgroup blockIdx.x serves matrix first + blockIdx.x.
template <class T, bool LOO, bool GRAD, bool PREDICT, bool COV>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Bs, const T *Cs, const T *Ds, const T *As, int nquery, const T *Es,
                                                                 T *mean, T *cov, int *info, int n, T *workspace, size_t first)
{
    static_assert(LOO && GRAD && PREDICT && COV, "the five-argument form is the predictive-covariance kernel");
    __shared__ T col[1024], va[1024], vy[1024], vq[1024];
    const size_t k_mat = first + blockIdx.x;
    const T *A = Bs + k_mat * (size_t)n * n;
    const size_t nn = (size_t)n * n, qq = (size_t)nquery * nquery;
    T *W = workspace + (size_t)blockIdx.x * (nn + (size_t)n * nquery);
    T *V = W + nn;
    const int t = threadIdx.x;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        T v = A[e];
        if (Cs && r == c) v += Cs[k_mat * n + r];
        W[e] = v;
    }
    if (mean)
        for (int i = t; i < n; i += GL_THREADS) va[i] = Ds[k_mat * n + i];
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {  // block-uniform
        if (mean)
            for (int j = t; j < nquery; j += GL_THREADS) mean[k_mat * nquery + j] = nan_of<T>();
        if (cov)
            for (size_t e = t; e < qq; e += GL_THREADS) cov[k_mat * qq + e] = nan_of<T>();
        if (info && t == 0) info[k_mat] = bad;
        return;
    }
    for (int j = n - 1; j >= 0; --j) {  // L <- L^-1 in place, last column first (the loop of the inverse kernel)
        const T ajj = (T)1 / W[(size_t)j * n + j];
        for (int i = j + 1 + t; i < n; i += GL_THREADS) col[i] = W[(size_t)j * n + i];
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += GL_THREADS) {
            T s = 0;
            for (int k = j + 1; k <= i; ++k) s += W[(size_t)k * n + i] * col[k];
            W[(size_t)j * n + i] = -s * ajj;
        }
        if (t == 0) W[(size_t)j * n + j] = ajj;
        __syncthreads();
    }
    if (mean) {  // block-uniform
        // y = L^-1 d: (L^-1)_kj sits at W[j*n + k]
        for (int k = t; k < n; k += GL_THREADS) {
            T s = 0;
            for (int j = 0; j <= k; ++j) s += W[(size_t)j * n + k] * va[j];
            vy[k] = s;
        }
        __syncthreads();
        // alpha_i = column i of L^-1 against y; it takes the place of d
        for (int i = t; i < n; i += GL_THREADS) {
            T a = 0;
            for (int k = i; k < n; ++k) a += W[(size_t)i * n + k] * vy[k];
            va[i] = a;
        }
        __syncthreads();
    }
    for (int j = 0; j < nquery; ++j) {
        const size_t out = k_mat * nquery + j;
        const T *a = As + out * n;
        for (int i = t; i < n; i += GL_THREADS) vq[i] = a[i];
        __syncthreads();
        T sm = 0;
        for (int k = t; k < n; k += GL_THREADS) {
            if (cov) {  // V[k][j] = row k of L^-1 against a
                T s = 0;
                for (int i = 0; i <= k; ++i) s += W[(size_t)i * n + k] * vq[i];
                V[(size_t)j * n + k] = s;
            }
            if (mean) sm += vq[k] * va[k];
        }
        if (mean) {  // block-uniform: the block sum on the fixed tree of the prediction form
            vy[t] = sm;
            __syncthreads();
            for (int off = GL_THREADS / 2; off >= 1; off >>= 1) {
                if (t < off) vy[t] += vy[t + off];
                __syncthreads();
            }
            if (t == 0) mean[out] = vy[0];
        }
        __syncthreads();  // the next query overwrites vq and vy; after the last one, V is complete for every thread
    }
    if (cov) {  // block-uniform
        const T *E = Es ? Es + k_mat * qq : nullptr;
        T *C = cov + k_mat * qq;
        for (size_t e = t; e < qq; e += GL_THREADS) {
            const int j = (int)(e / nquery), i = (int)(e - (size_t)j * nquery);
            if (i < j) continue;
            const T *vi = V + (size_t)i * n, *vj = V + (size_t)j * n;
            T s = 0;
            for (int k = 0; k < n; ++k) s += vi[k] * vj[k];
            const T v = (E ? E[e] : (T)0) - s;
            C[e] = v;
            C[(size_t)i * nquery + j] = v;
        }
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_predict_cov_global(int n, int nquery, const T *Bs, const T *Cs, const T *Ds, const T *As, const T *Es, T *mean, T *cov,
                                     size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk, each with its n x Q block V, fit the blocked-path workspace cap (launch_predict_global)
    const size_t per = (size_t)n * ((size_t)n + (size_t)nquery);
    size_t chunk = blocked_workspace_cap() / (per * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * per * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true, true, true>), dim3((unsigned)cnt), dim3(GL_THREADS), 0, stream, Bs, Cs, Ds, As,
                           nquery, Es, mean, cov, info, n, ws, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_predict_cov_global<double>(int, int, const double *, const double *, const double *, const double *,
                                                      const double *, double *, double *, size_t, int *, hipStream_t);
template hipError_t launch_predict_cov_global<float>(int, int, const float *, const float *, const float *, const float *, const float *,
                                                     float *, float *, size_t, int *, hipStream_t);

const char *name_predict_cov_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true, true, true>" : "matinv_chol_global<float, true, true, true, true>";
}

// ---- gradients of the GP leave-one-out log pseudo-likelihood, 96 < n <= 1024 (matinv_loo_grad_batched behind loo_grad_tile_impl.hpp) -----
// The LOO-gradient form of matinv_chol_global: one more template argument again ("Gradients of the leave-one-out
// pseudo-likelihood"). The matrix's slice of library scratch is 2 n^2 elements: W, then H. The pipeline of the gradient form -- working
// copy, factor, triangular inverse, alpha, the lower triangle of K = M^-1 in place -- continued:
//     K mirrored into the upper triangle of W        (every later access runs down a column: consecutive threads, consecutive addresses)
//     kappa_i = K_ii,  b_i = alpha_i / kappa_i,  s_i = (1 + alpha_i^2 / kappa_i) / kappa_i,  logpl on the fixed LDS tree
//     beta = K b
//     H_rc = sum_t s_t K_rt K_tc, r >= c, t ascending, one thread per element
//     gradc_i = alpha_i beta_i - 1/2 H_ii
//     grad_p = sum_{r >= c} w_rc (1/2 (alpha_r beta_c + beta_r alpha_c) - 1/2 H_rc) dM_p[r][c],  w = 1 on the diagonal, 2 below
// with dM_p read from caller memory (lower triangle only) and grad_p summed per thread in element order, then on the fixed LDS tree.
// Not SPD: info = the failing column + 1 and every output NaN. Correct first; speed is not a goal here. Workgroup blockIdx.x serves
// matrix first + blockIdx.x.
template <class T, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Bs, const T *Cs, const T *Ds, const T *dMs, int nparam, T *grad,
                                                                 T *gradc, T *logpl, int *info, int n, T *workspace, size_t first)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD, "the six-argument form is the leave-one-out gradient kernel");
    __shared__ T col[1024], va[1024], vy[1024], vs[1024], vb[1024];
    const size_t k_mat = first + blockIdx.x;
    const T *A = Bs + k_mat * (size_t)n * n;
    const size_t nn = (size_t)n * n;
    T *W = workspace + (size_t)blockIdx.x * 2 * nn;
    T *H = W + nn;
    const int t = threadIdx.x;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        T v = A[e];
        if (Cs && r == c) v += Cs[k_mat * n + r];
        W[e] = v;
    }
    for (int i = t; i < n; i += GL_THREADS) va[i] = Ds[k_mat * n + i];
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {  // block-uniform
        if (gradc)
            for (int i = t; i < n; i += GL_THREADS) gradc[k_mat * n + i] = nan_of<T>();
        if (grad)
            for (int p = t; p < nparam; p += GL_THREADS) grad[k_mat * nparam + p] = nan_of<T>();
        if (t == 0) {
            if (logpl) logpl[k_mat] = nan_of<T>();
            if (info) info[k_mat] = bad;
        }
        return;
    }
    for (int j = n - 1; j >= 0; --j) {  // L <- L^-1 in place, last column first (the loop of the inverse kernel)
        const T ajj = (T)1 / W[(size_t)j * n + j];
        for (int i = j + 1 + t; i < n; i += GL_THREADS) col[i] = W[(size_t)j * n + i];
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += GL_THREADS) {
            T s = 0;
            for (int k = j + 1; k <= i; ++k) s += W[(size_t)k * n + i] * col[k];
            W[(size_t)j * n + i] = -s * ajj;
        }
        if (t == 0) W[(size_t)j * n + j] = ajj;
        __syncthreads();
    }
    // y = L^-1 d: (L^-1)_kj sits at W[j*n + k]
    for (int k = t; k < n; k += GL_THREADS) {
        T s = 0;
        for (int j = 0; j <= k; ++j) s += W[(size_t)j * n + k] * va[j];
        vy[k] = s;
    }
    __syncthreads();
    // alpha_i = column i of L^-1 against y; it takes the place of d
    for (int i = t; i < n; i += GL_THREADS) {
        T a = 0;
        for (int k = i; k < n; ++k) a += W[(size_t)i * n + k] * vy[k];
        va[i] = a;
    }
    __syncthreads();
    // column c of K over column c of L^-1; the columns beyond c are still those of L^-1
    for (int c = 0; c < n; ++c) {
        for (int k = c + t; k < n; k += GL_THREADS) col[k] = W[(size_t)c * n + k];
        __syncthreads();
        for (int r = c + t; r < n; r += GL_THREADS) {
            T s = 0;
            if (r == c) {
                for (int k = r; k < n; ++k) s += col[k] * col[k];
            } else {
                for (int k = r; k < n; ++k) s += W[(size_t)r * n + k] * col[k];
            }
            W[(size_t)c * n + r] = s;
        }
        __syncthreads();
    }
    // the mirror: K_rc, r < c, from K_cr
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) W[e] = W[(size_t)r * n + c];
    }
    // kappa, b, s and the terms of logpl; b takes the place of y
    T term = 0;
    for (int i = t; i < n; i += GL_THREADS) {
        const T kappa = W[(size_t)i * n + i], a = va[i];
        const T rk = (T)1 / kappa;
        const T b = a * rk;
        vy[i] = b;
        vs[i] = (a * b + (T)1) * rk;
        term += (T)0.5 * gl_log<T>(kappa) - (T)0.5 * a * b;
    }
    col[t] = term;
    __syncthreads();  // the mirror, b and s are complete as well
    for (int off = GL_THREADS / 2; off >= 1; off >>= 1) {
        if (t < off) col[t] += col[t + off];
        __syncthreads();
    }
    if (t == 0 && logpl) logpl[k_mat] = col[0] - (T)n * (T)0.91893853320467274178;
    if (grad || gradc) {  // block-uniform
        // beta_i = row i of K against b, read as column i
        for (int i = t; i < n; i += GL_THREADS) {
            T s = 0;
            for (int j = 0; j < n; ++j) s += W[(size_t)j * n + i] * vy[j];
            vb[i] = s;
        }
        // H_rc, r >= c: K_rt runs down column t with the thread, K_tc is one address per column c
        for (size_t e = t; e < nn; e += GL_THREADS) {
            const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
            if (r < c) continue;
            const T *kc = W + (size_t)c * n;
            T s = 0;
            for (int k = 0; k < n; ++k) s += vs[k] * W[(size_t)k * n + r] * kc[k];
            H[e] = s;
        }
        __syncthreads();
        if (gradc)
            for (int i = t; i < n; i += GL_THREADS) gradc[k_mat * n + i] = va[i] * vb[i] - (T)0.5 * H[(size_t)i * n + i];
        if (grad) {
            for (int p = 0; p < nparam; ++p) {
                const T *D = dMs + (k_mat * nparam + p) * nn;
                T s = 0;
                for (size_t e = t; e < nn; e += GL_THREADS) {
                    const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
                    if (r < c) continue;
                    const T g = (T)0.5 * (va[r] * vb[c] + vb[r] * va[c]) - (T)0.5 * H[e];
                    s += (r == c ? (T)1 : (T)2) * g * D[e];
                }
                // block sum on a fixed tree
                col[t] = s;
                __syncthreads();
                for (int off = GL_THREADS / 2; off >= 1; off >>= 1) {
                    if (t < off) col[t] += col[t + off];
                    __syncthreads();
                }
                if (t == 0) grad[k_mat * nparam + p] = col[0];
                __syncthreads();
            }
        }
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_loo_grad_global(int n, int nparam, const T *Bs, const T *Cs, const T *Ds, const T *dMs, T *grad, T *gradc, T *logpl,
                                  size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk, each with its n x n block H, fit the blocked-path workspace cap (launch_loo_global)
    const size_t per = 2 * (size_t)n * n;
    size_t chunk = blocked_workspace_cap() / (per * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * per * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true, true, true, true>), dim3((unsigned)cnt), dim3(GL_THREADS), 0, stream, Bs, Cs, Ds,
                           dMs, nparam, grad, gradc, logpl, info, n, ws, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_loo_grad_global<double>(int, int, const double *, const double *, const double *, const double *, double *, double *,
                                                   double *, size_t, int *, hipStream_t);
template hipError_t launch_loo_grad_global<float>(int, int, const float *, const float *, const float *, const float *, float *, float *,
                                                  float *, size_t, int *, hipStream_t);

const char *name_loo_grad_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true, true, true, true>" : "matinv_chol_global<float, true, true, true, true, true>";
}

// ---- Cholesky factor and coloured samples, 96 < n <= 1024 (matinv_colour_batched behind colour_tile_impl.hpp) ---------------------------
// The colour form of matinv_chol_global: one more template argument again ("Posterior samples"). The lower triangle of C is
// factored in the matrix's slice of library scratch, as above. Then
//     L out, the strict upper triangle as zeros;   per (row i, sample s), one thread each:  Y[i][s] = m_i + sum_k L[i][k] z_s[k], k ascending
// so the order of operations of an element knows nothing of S or of the sample's position. Not SPD: info = the failing column + 1 and
// every requested output NaN. Correct first; speed is not a goal here. Workgroup blockIdx.x serves matrix first + blockIdx.x.
template <class T, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Cs, size_t stride, const T *Ms, const T *Zs, int nsample, T *Ys,
                                                                 T *Ls, int *info, int info_base, int n, T *workspace, size_t first)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR, "the seven-argument form is the colour kernel");
    __shared__ T col[1024];
    const size_t k_mat = first + blockIdx.x;
    const T *A = Cs + k_mat * stride;
    const size_t nn = (size_t)n * n, ns = (size_t)n * nsample;
    T *W = workspace + (size_t)blockIdx.x * nn;
    T *Lm = Ls ? Ls + k_mat * nn : nullptr, *Ym = Ys ? Ys + k_mat * ns : nullptr;
    const int t = threadIdx.x;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r >= c) W[e] = A[e];
    }
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {  // block-uniform
        if (Lm)
            for (size_t e = t; e < nn; e += GL_THREADS) Lm[e] = nan_of<T>();
        if (Ym)
            for (size_t e = t; e < ns; e += GL_THREADS) Ym[e] = nan_of<T>();
        if (info && t == 0) {  // the code of an earlier stage stands (colour_tile_body)
            const int prior = info_base ? info[k_mat] : 0;
            info[k_mat] = prior ? prior : info_base + bad;
        }
        return;
    }
    if (Lm)
        for (size_t e = t; e < nn; e += GL_THREADS) {
            const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
            Lm[e] = r >= c ? W[e] : (T)0;
        }
    if (Ym) {
        const T *Z = Zs + k_mat * ns;
        for (size_t e = t; e < ns; e += GL_THREADS) {
            const int s = (int)(e / n), i = (int)(e - (size_t)s * n);
            const T *z = Z + (size_t)s * n;
            T a = 0;
            for (int k = 0; k <= i; ++k) a += W[(size_t)k * n + i] * z[k];
            Ym[e] = (Ms ? Ms[k_mat * n + i] : (T)0) + a;
        }
    }
    if (info && t == 0 && !info_base) info[k_mat] = 0;  // after an earlier stage a factored matrix has its 0 already
}

template <class T>
hipError_t launch_colour_global(int n, int nsample, const T *Cs, size_t stride, const T *Ms, const T *Zs, T *Ys, T *Ls, size_t batch,
                                int *info, int info_base, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk fit the blocked-path workspace cap (launch_loo_global)
    const size_t per = (size_t)n * n;
    size_t chunk = blocked_workspace_cap() / (per * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * per * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true, true, true, true, true>), dim3((unsigned)cnt), dim3(GL_THREADS), 0, stream, Cs,
                           stride, Ms, Zs, nsample, Ys, Ls, info, info_base, n, ws, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_colour_global<double>(int, int, const double *, size_t, const double *, const double *, double *, double *, size_t,
                                                 int *, int, hipStream_t);
template hipError_t launch_colour_global<float>(int, int, const float *, size_t, const float *, const float *, float *, float *, size_t,
                                                int *, int, hipStream_t);

const char *name_colour_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true, true, true, true, true>"
               : "matinv_chol_global<float, true, true, true, true, true, true>";
}

// ---- whitening, Mahalanobis distances and Gaussian log-density, 96 < n <= 1024 (matinv_whiten_batched behind whiten_tile_impl.hpp) ------
// The whiten form of matinv_chol_global: one more template argument again ("Whitening"). The lower triangle of C is factored in
// the matrix's slice of library scratch, as above. Thread 0 folds the diagonal of L into a PivotProduct: logdet = 2 log prod L_ii. Then one
// thread per point, on the point's own n elements of scratch behind the factor: v = x - m; columns k ascending: w_k = v_k / L_kk,
// maha += w_k^2, v_i -= L_ik w_k for i > k. The order of operations of a point knows nothing of S or of the point's position. Not SPD:
// info = the failing column + 1 and every requested output NaN. Correct first; speed is not a goal here. Workgroup blockIdx.x serves
// matrix first + blockIdx.x; `per` elements of workspace each (n^2, and n npoint more when the points are read).
template <class T, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Cs, size_t stride, const T *Ms, const T *Xs, int npoint, T *Ws,
                                                                 T *Mh, T *Ld, T *Lp, int *info, int n, T *workspace, size_t per,
                                                                 size_t first)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN, "the eight-argument form is the whiten kernel");
    __shared__ T col[1024];
    __shared__ T s_ld;
    const size_t k_mat = first + blockIdx.x;
    const T *A = Cs + k_mat * stride;
    const bool points = Ws || Mh || Lp;  // block-uniform
    const size_t nn = (size_t)n * n, np = points ? (size_t)npoint : 0, ns = (size_t)n * np;
    T *W = workspace + (size_t)blockIdx.x * per;
    T *V = W + nn;
    T *Wm = Ws ? Ws + k_mat * ns : nullptr;
    const int t = threadIdx.x;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r >= c) W[e] = A[e];
    }
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {  // block-uniform
        if (Wm)
            for (size_t e = t; e < ns; e += GL_THREADS) Wm[e] = nan_of<T>();
        for (size_t s = t; s < np; s += GL_THREADS) {
            if (Mh) Mh[k_mat * np + s] = nan_of<T>();
            if (Lp) Lp[k_mat * np + s] = nan_of<T>();
        }
        if (Ld && t == 0) Ld[k_mat] = nan_of<T>();
        if (info && t == 0) info[k_mat] = bad;
        return;
    }
    if (t == 0) {
        PivotProduct<T> prod;
        for (int i = 0; i < n; ++i) prod.fold(W[(size_t)i * n + i]);
        const T ld = (T)2 * prod.log_value();
        s_ld = ld;
        if (Ld) Ld[k_mat] = ld;
    }
    __syncthreads();
    const T ld = s_ld;
    for (size_t s = t; s < np; s += GL_THREADS) {
        const T *x = Xs + k_mat * ns + s * n;
        T *v = V + s * n;
        for (int i = 0; i < n; ++i) v[i] = x[i] - (Ms ? Ms[k_mat * n + i] : (T)0);
        T mh = 0;
        for (int k = 0; k < n; ++k) {
            const T *lk = W + (size_t)k * n;
            const T w = v[k] / lk[k];
            v[k] = w;
            mh += w * w;
            for (int i = k + 1; i < n; ++i) v[i] -= lk[i] * w;
        }
        if (Wm)
            for (int i = 0; i < n; ++i) Wm[s * n + i] = v[i];
        if (Mh) Mh[k_mat * np + s] = mh;
        // log 2 pi
        if (Lp) Lp[k_mat * np + s] = (T)-0.5 * ((mh + ld) + (T)n * (T)1.83787706640934548356);
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_whiten_global(int n, int npoint, const T *Cs, size_t stride, const T *Ms, const T *Xs, T *Ws, T *Mh, T *Ld, T *Lp,
                                size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk fit the blocked-path workspace cap (launch_loo_global)
    const size_t per = (size_t)n * n + ((Ws || Mh || Lp) ? (size_t)n * npoint : 0);
    size_t chunk = blocked_workspace_cap() / (per * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * per * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true, true, true, true, true, true>), dim3((unsigned)cnt), dim3(GL_THREADS), 0, stream,
                           Cs, stride, Ms, Xs, npoint, Ws, Mh, Ld, Lp, info, n, ws, per, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_whiten_global<double>(int, int, const double *, size_t, const double *, const double *, double *, double *,
                                                 double *, double *, size_t, int *, hipStream_t);
template hipError_t launch_whiten_global<float>(int, int, const float *, size_t, const float *, const float *, float *, float *, float *,
                                                float *, size_t, int *, hipStream_t);

const char *name_whiten_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true, true, true, true, true, true>"
               : "matinv_chol_global<float, true, true, true, true, true, true, true>";
}

// ---- multi-output GP solves, 96 < n <= 1024 (matinv_multi_target_batched behind multi_target_tile_impl.hpp) -----------------------------
// The multi-target form of matinv_chol_global: one more template argument again ("Multi-output solves"). M = B + diag c is
// factored in the matrix's slice of library scratch, as above. Thread 0 folds the diagonal of L into a PivotProduct: logdet = 2 log prod
// L_ii. Then one thread per target, on the target's own n elements of scratch behind the factor: v = y; columns k ascending:
// w_k = v_k / L_kk, quad += w_k^2, v_i -= L_ik w_k for i > k; then rows k descending: alpha_k = (w_k - sum_{i > k} L_ik alpha_i) / L_kk,
// i ascending. Then one thread per (target, query) pair: mean = sum_i a_j[i] alpha_t[i], i ascending. The order of operations of a
// target knows nothing of D or of its position, that of a pair nothing of Q either. Not SPD: info = the failing column + 1 and every
// requested output NaN. Correct first; speed is not a goal here. Workgroup blockIdx.x serves matrix first + blockIdx.x; `per` elements
// of workspace each (n^2, and n ntarget more when the targets are read).
template <class T, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Bs, const T *Cs, const T *Ys, const T *As, int ntarget, int nquery,
                                                                 T *Al, T *Qd, T *Ld, T *Lm, T *Mn, int *info, int n, T *workspace,
                                                                 size_t per, size_t first)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN && MULTI, "the nine-argument form is the multi-target kernel");
    __shared__ T col[1024];
    __shared__ T s_ld;
    const size_t k_mat = first + blockIdx.x;
    const T *A = Bs + k_mat * (size_t)n * n;
    const bool targets = Al || Qd || Lm || Mn;  // block-uniform
    const size_t nn = (size_t)n * n, nd = targets ? (size_t)ntarget : 0, nq = Mn ? (size_t)nquery : 0;
    T *W = workspace + (size_t)blockIdx.x * per;
    T *V = W + nn;
    const int t = threadIdx.x;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        T v = A[e];
        if (Cs && r == c) v += Cs[k_mat * n + r];
        W[e] = v;
    }
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {  // block-uniform
        if (Al)
            for (size_t e = t; e < nd * n; e += GL_THREADS) Al[k_mat * nd * n + e] = nan_of<T>();
        for (size_t s = t; s < nd; s += GL_THREADS) {
            if (Qd) Qd[k_mat * nd + s] = nan_of<T>();
            if (Lm) Lm[k_mat * nd + s] = nan_of<T>();
        }
        if (Mn)
            for (size_t e = t; e < nd * nq; e += GL_THREADS) Mn[k_mat * nd * nq + e] = nan_of<T>();
        if (Ld && t == 0) Ld[k_mat] = nan_of<T>();
        if (info && t == 0) info[k_mat] = bad;
        return;
    }
    if (t == 0) {
        PivotProduct<T> prod;
        for (int i = 0; i < n; ++i) prod.fold(W[(size_t)i * n + i]);
        const T ld = (T)2 * prod.log_value();
        s_ld = ld;
        if (Ld) Ld[k_mat] = ld;
    }
    __syncthreads();
    const T ld = s_ld;
    for (size_t s = t; s < nd; s += GL_THREADS) {
        const T *y = Ys + (k_mat * nd + s) * n;
        T *v = V + s * n;
        for (int i = 0; i < n; ++i) v[i] = y[i];
        T qd = 0;
        for (int k = 0; k < n; ++k) {
            const T *lk = W + (size_t)k * n;
            const T w = v[k] / lk[k];
            v[k] = w;
            qd += w * w;
            for (int i = k + 1; i < n; ++i) v[i] -= lk[i] * w;
        }
        for (int k = n - 1; k >= 0; --k) {
            const T *lk = W + (size_t)k * n;
            T a = v[k];
            for (int i = k + 1; i < n; ++i) a -= lk[i] * v[i];
            v[k] = a / lk[k];
        }
        if (Al)
            for (int i = 0; i < n; ++i) Al[(k_mat * nd + s) * n + i] = v[i];
        if (Qd) Qd[k_mat * nd + s] = qd;
        // log 2 pi
        if (Lm) Lm[k_mat * nd + s] = (T)-0.5 * ((qd + ld) + (T)n * (T)1.83787706640934548356);
    }
    if (Mn) {  // block-uniform
        __syncthreads();  // every target's alpha is in V
        for (size_t e = t; e < nd * nq; e += GL_THREADS) {
            const size_t s = e / nq, j = e - s * nq;
            const T *a = As + (k_mat * nq + j) * n, *v = V + s * n;
            T m = 0;
            for (int i = 0; i < n; ++i) m += a[i] * v[i];
            Mn[k_mat * nd * nq + e] = m;
        }
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_multi_target_global(int n, int ntarget, int nquery, const T *Bs, const T *Cs, const T *Ys, const T *As, T *Al, T *Qd,
                                      T *Ld, T *Lm, T *Mn, size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk, each with its n x D block of targets, fit the blocked-path workspace cap (launch_loo_global)
    const size_t per = (size_t)n * n + ((Al || Qd || Lm || Mn) ? (size_t)n * ntarget : 0);
    size_t chunk = blocked_workspace_cap() / (per * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * per * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true, true, true, true, true, true, true>), dim3((unsigned)cnt), dim3(GL_THREADS), 0,
                           stream, Bs, Cs, Ys, As, ntarget, nquery, Al, Qd, Ld, Lm, Mn, info, n, ws, per, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_multi_target_global<double>(int, int, int, const double *, const double *, const double *, const double *,
                                                       double *, double *, double *, double *, double *, size_t, int *, hipStream_t);
template hipError_t launch_multi_target_global<float>(int, int, int, const float *, const float *, const float *, const float *, float *,
                                                      float *, float *, float *, float *, size_t, int *, hipStream_t);

const char *name_multi_target_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true, true, true, true, true, true, true>"
               : "matinv_chol_global<float, true, true, true, true, true, true, true, true>";
}

// ---- gradients of the multi-output log marginal likelihood, 96 < n <= 1024 (matinv_multi_target_grad_batched behind
// multi_target_grad_tile_impl.hpp) ------------------------------------------------------------------------------------------------------
// The multi-target gradient form of matinv_chol_global: one more template argument again ("Gradients of the multi-output log
// marginal likelihood"). The factorisation, the diagonal fold and the one-thread-per-target substitutions are those of the multi-target
// form above, so logml and alpha are its values; alpha_t stays in the target's n elements of scratch behind the factor. Then, when grad
// or gradc is asked for, L <- L^-1 and K over it in place as in the gradient form, and with G_rc = sum_t alpha_tr alpha_tc - D K_rc
// formed on the fly (t ascending):
//     gradc_i = 1/2 G_ii,   grad_p = sum_{r >= c} w_rc G_rc dM_p[r][c],  w = 1/2 on the diagonal, 1 below
// grad_p summed per thread in element order, then on the fixed LDS tree. Not SPD: info = the failing column + 1 and every requested
// output NaN. Correct first; speed is not a goal here. Workgroup blockIdx.x serves matrix first + blockIdx.x; `per` = n (n + ntarget)
// elements of workspace each.
template <class T, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Bs, const T *Cs, const T *Ys, const T *dMs, int ntarget, int nparam,
                                                                 T *grad, T *gradc, T *Lm, T *Al, int *info, int n, T *workspace, size_t per,
                                                                 size_t first)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN && MULTI && MTGRAD,
                  "the ten-argument form is the multi-target gradient kernel");
    __shared__ T col[1024];
    __shared__ T s_ld;
    const size_t k_mat = first + blockIdx.x;
    const T *A = Bs + k_mat * (size_t)n * n;
    const size_t nn = (size_t)n * n, nd = (size_t)ntarget;
    T *W = workspace + (size_t)blockIdx.x * per;
    T *V = W + nn;
    const int t = threadIdx.x;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        T v = A[e];
        if (Cs && r == c) v += Cs[k_mat * n + r];
        W[e] = v;
    }
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {  // block-uniform
        if (Al)
            for (size_t e = t; e < nd * n; e += GL_THREADS) Al[k_mat * nd * n + e] = nan_of<T>();
        if (Lm)
            for (size_t s = t; s < nd; s += GL_THREADS) Lm[k_mat * nd + s] = nan_of<T>();
        if (gradc)
            for (int i = t; i < n; i += GL_THREADS) gradc[k_mat * n + i] = nan_of<T>();
        if (grad)
            for (int p = t; p < nparam; p += GL_THREADS) grad[k_mat * nparam + p] = nan_of<T>();
        if (info && t == 0) info[k_mat] = bad;
        return;
    }
    if (t == 0) {
        PivotProduct<T> prod;
        for (int i = 0; i < n; ++i) prod.fold(W[(size_t)i * n + i]);
        s_ld = (T)2 * prod.log_value();
    }
    __syncthreads();
    const T ld = s_ld;
    for (size_t s = t; s < nd; s += GL_THREADS) {
        const T *y = Ys + (k_mat * nd + s) * n;
        T *v = V + s * n;
        for (int i = 0; i < n; ++i) v[i] = y[i];
        T qd = 0;
        for (int k = 0; k < n; ++k) {
            const T *lk = W + (size_t)k * n;
            const T w = v[k] / lk[k];
            v[k] = w;
            qd += w * w;
            for (int i = k + 1; i < n; ++i) v[i] -= lk[i] * w;
        }
        for (int k = n - 1; k >= 0; --k) {
            const T *lk = W + (size_t)k * n;
            T a = v[k];
            for (int i = k + 1; i < n; ++i) a -= lk[i] * v[i];
            v[k] = a / lk[k];
        }
        if (Al)
            for (int i = 0; i < n; ++i) Al[(k_mat * nd + s) * n + i] = v[i];
        // log 2 pi
        if (Lm) Lm[k_mat * nd + s] = (T)-0.5 * ((qd + ld) + (T)n * (T)1.83787706640934548356);
    }
    if (grad || gradc) {  // block-uniform
        __syncthreads();  // every target's alpha is in V, and the factor is no longer needed
        for (int j = n - 1; j >= 0; --j) {  // L <- L^-1 in place, last column first (the loop of the inverse kernel)
            const T ajj = (T)1 / W[(size_t)j * n + j];
            for (int i = j + 1 + t; i < n; i += GL_THREADS) col[i] = W[(size_t)j * n + i];
            __syncthreads();
            for (int i = j + 1 + t; i < n; i += GL_THREADS) {
                T s = 0;
                for (int k = j + 1; k <= i; ++k) s += W[(size_t)k * n + i] * col[k];
                W[(size_t)j * n + i] = -s * ajj;
            }
            if (t == 0) W[(size_t)j * n + j] = ajj;
            __syncthreads();
        }
        // column c of K over column c of L^-1; the columns beyond c are still those of L^-1
        for (int c = 0; c < n; ++c) {
            for (int k = c + t; k < n; k += GL_THREADS) col[k] = W[(size_t)c * n + k];
            __syncthreads();
            for (int r = c + t; r < n; r += GL_THREADS) {
                T s = 0;
                if (r == c) {
                    for (int k = r; k < n; ++k) s += col[k] * col[k];
                } else {
                    for (int k = r; k < n; ++k) s += W[(size_t)r * n + k] * col[k];
                }
                W[(size_t)c * n + r] = s;
            }
            __syncthreads();
        }
        const T dscale = (T)ntarget;
        if (gradc)
            for (int i = t; i < n; i += GL_THREADS) {
                T aa = 0;
                for (size_t s = 0; s < nd; ++s) aa += V[s * n + i] * V[s * n + i];
                gradc[k_mat * n + i] = (T)0.5 * (aa - dscale * W[(size_t)i * n + i]);
            }
        if (grad) {
            for (int p = 0; p < nparam; ++p) {
                const T *D = dMs + (k_mat * nparam + p) * nn;
                T s = 0;
                for (size_t e = t; e < nn; e += GL_THREADS) {
                    const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
                    if (r < c) continue;
                    T aa = 0;
                    for (size_t u = 0; u < nd; ++u) aa += V[u * n + r] * V[u * n + c];
                    const T g = aa - dscale * W[e];
                    s += (r == c ? (T)0.5 : (T)1) * g * D[e];
                }
                // block sum on a fixed tree
                col[t] = s;
                __syncthreads();
                for (int off = GL_THREADS / 2; off >= 1; off >>= 1) {
                    if (t < off) col[t] += col[t + off];
                    __syncthreads();
                }
                if (t == 0) grad[k_mat * nparam + p] = col[0];
                __syncthreads();
            }
        }
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_multi_target_grad_global(int n, int ntarget, int nparam, const T *Bs, const T *Cs, const T *Ys, const T *dMs, T *grad,
                                           T *gradc, T *Lm, T *Al, size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk, each with its n x D block of targets, fit the blocked-path workspace cap (launch_loo_global)
    const size_t per = (size_t)n * n + (size_t)n * ntarget;
    size_t chunk = blocked_workspace_cap() / (per * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * per * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true, true, true, true, true, true, true, true>), dim3((unsigned)cnt),
                           dim3(GL_THREADS), 0, stream, Bs, Cs, Ys, dMs, ntarget, nparam, grad, gradc, Lm, Al, info, n, ws, per, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_multi_target_grad_global<double>(int, int, int, const double *, const double *, const double *, const double *,
                                                            double *, double *, double *, double *, size_t, int *, hipStream_t);
template hipError_t launch_multi_target_grad_global<float>(int, int, int, const float *, const float *, const float *, const float *, float *,
                                                           float *, float *, float *, size_t, int *, hipStream_t);

const char *name_multi_target_grad_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true, true, true, true, true, true, true, true>"
               : "matinv_chol_global<float, true, true, true, true, true, true, true, true, true>";
}

// ---- GP regression with a linear trend, 96 < n <= 1024 (matinv_trend_batched behind trend_tile_impl.hpp) -------------------------------
// The trend form of matinv_chol_global: one more template argument again ("Regression with a linear trend"). M = B + diag c
// is factored in the matrix's slice of library scratch and the diagonal of L folded as in the multi-target form. Then
//   * one thread per column of [H | Y], on the column's own n elements of scratch behind the factor: forward and backward substitution
//     as in the multi-target form, which leaves Kinv h_b and Kinv y_t;
//   * A[b][b'] = h_b^T (Kinv h_b'), b >= b', i ascending, one thread per element, into LDS; thread 0 factors A = L_A L_A^T (K <= 16) and
//     folds its pivots L_A,bb^2 into a PivotProduct: log det A. A non-positive or NaN pivot b: info = n + b, every requested output NaN.
//     Thread b solves column b of L_A^-1; covbeta[b][b'] = sum_i L_A^-1[i][b] L_A^-1[i][b'], i ascending from b, stored to both positions;
//   * one thread per target: (H^T Kinv y)_b = (Kinv h_b)^T y, beta by the two triangular solves, alpha = Kinv y - sum_b (Kinv h_b) beta_b
//     (b ascending) in place, quad = y^T alpha, logml;
//   * one thread per (target, query) pair: mean = sum_i a_j[i] alpha_t[i] + sum_b g_j[b] beta_t[b];
//   * one thread per query: w = L^-1 a_j on n elements of scratch, a^T Kinv a = sum w_k^2; r_b = g_b - (Kinv h_b)^T a_j; z = L_A^-1 r;
//     var = (e - a^T Kinv a) + sum z_b^2.
// The order of operations of an output knows nothing of D, Q, or the position of its target or query; the loops over the basis run over
// the K real vectors only, in ascending order. Correct first; speed is not a goal here. Workgroup blockIdx.x serves matrix
// first + blockIdx.x; `per` elements of workspace each: n^2 + n (K + D') + K D' + (n + K) Q', D' = D when the targets are read, Q' = Q
// with var.
template <class T, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD, bool TREND>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Bs, const T *Cs, const T *Hs, const T *Ys, const T *As, const T *Gs,
                                                                 const T *Es, int nbasis, int ntarget, int nquery, T *Be, T *Cb, T *Al, T *Qd,
                                                                 T *Lm, T *Mn, T *Vr, int *info, int n, T *workspace, size_t per, size_t first)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN && MULTI && MTGRAD && TREND,
                  "the eleven-argument form is the trend kernel");
    __shared__ T col[1024];
    __shared__ T sA[16 * 17], sLi[16 * 17];
    __shared__ T s_ld, s_ldA;
    __shared__ int s_abad;
    const size_t k_mat = first + blockIdx.x;
    const T *A = Bs + k_mat * (size_t)n * n;
    const bool targets = Be || Al || Qd || Lm || Mn;  // block-uniform
    const size_t nn = (size_t)n * n, K = (size_t)nbasis, nd = targets ? (size_t)ntarget : 0;
    const size_t nq = (Mn || Vr) ? (size_t)nquery : 0, nqv = Vr ? (size_t)nquery : 0;
    T *W = workspace + (size_t)blockIdx.x * per;
    T *V = W + nn;                 // Kinv h_b, b < K, then Kinv y_t -> alpha_t
    T *Bt = V + (K + nd) * n;      // beta_t
    T *U = Bt + nd * K;            // L^-1 a_j
    T *R = U + nqv * n;            // r_j -> z_j
    const int t = threadIdx.x;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        T v = A[e];
        if (Cs && r == c) v += Cs[k_mat * n + r];
        W[e] = v;
    }
    __syncthreads();
    int bad = gl_chol_factor(W, n, col);
    if (!bad) {  // block-uniform
        if (t == 0) {
            PivotProduct<T> prod;
            for (int i = 0; i < n; ++i) prod.fold(W[(size_t)i * n + i]);
            s_ld = (T)2 * prod.log_value();
        }
        for (size_t s = t; s < K + nd; s += GL_THREADS) {
            const T *x = s < K ? Hs + (k_mat * K + s) * n : Ys + (k_mat * nd + (s - K)) * n;
            T *v = V + s * n;
            for (int i = 0; i < n; ++i) v[i] = x[i];
            for (int k = 0; k < n; ++k) {
                const T *lk = W + (size_t)k * n;
                const T w = v[k] / lk[k];
                v[k] = w;
                for (int i = k + 1; i < n; ++i) v[i] -= lk[i] * w;
            }
            for (int k = n - 1; k >= 0; --k) {
                const T *lk = W + (size_t)k * n;
                T a = v[k];
                for (int i = k + 1; i < n; ++i) a -= lk[i] * v[i];
                v[k] = a / lk[k];
            }
        }
        __syncthreads();  // Kinv [H | Y] is in V
        for (size_t e = t; e < K * K; e += GL_THREADS) {
            const size_t b = e / K, b2 = e - b * K;
            if (b < b2) continue;
            const T *h = Hs + (k_mat * K + b) * n, *v = V + b2 * n;
            T a = 0;
            for (int i = 0; i < n; ++i) a += h[i] * v[i];
            sA[b * 17 + b2] = a;
        }
        __syncthreads();
        if (t == 0) {  // A = L_A L_A^T in place, 1 / L_bb on the diagonal
            int abad = 0;
            PivotProduct<T> prod;
            for (int j = 0; j < nbasis; ++j) {
                const T d = sA[j * 17 + j];
                if (!(d > (T)0) && abad == 0) abad = j + 1;
                prod.fold(d);
                const T rs = (T)1 / sqrt(d);
                // the update with the unscaled column and the quotient A[jj][j] / d: a basis vector that repeats an earlier one bit for
                // bit gets a pivot of exactly 0 (trend_tile_impl.hpp)
                for (int jj = j + 1; jj < nbasis; ++jj) {
                    const T m = sA[jj * 17 + j] / d;
                    for (int i = jj; i < nbasis; ++i) sA[i * 17 + jj] -= sA[i * 17 + j] * m;
                }
                sA[j * 17 + j] = rs;
                for (int i = j + 1; i < nbasis; ++i) sA[i * 17 + j] *= rs;
            }
            s_abad = abad;
            s_ldA = prod.log_value();
        }
        __syncthreads();
        if (s_abad) bad = n + s_abad;
    }
    if (bad) {  // block-uniform
        if (Be)
            for (size_t e = t; e < nd * K; e += GL_THREADS) Be[k_mat * nd * K + e] = nan_of<T>();
        if (Cb)
            for (size_t e = t; e < K * K; e += GL_THREADS) Cb[k_mat * K * K + e] = nan_of<T>();
        if (Al)
            for (size_t e = t; e < nd * n; e += GL_THREADS) Al[k_mat * nd * n + e] = nan_of<T>();
        for (size_t s = t; s < nd; s += GL_THREADS) {
            if (Qd) Qd[k_mat * nd + s] = nan_of<T>();
            if (Lm) Lm[k_mat * nd + s] = nan_of<T>();
        }
        if (Mn)
            for (size_t e = t; e < nd * nq; e += GL_THREADS) Mn[k_mat * nd * nq + e] = nan_of<T>();
        if (Vr)
            for (size_t e = t; e < nq; e += GL_THREADS) Vr[k_mat * nq + e] = nan_of<T>();
        if (info && t == 0) info[k_mat] = bad;
        return;
    }
    const T ld = s_ld, ldA = s_ldA;
    if (Cb) {  // block-uniform
        if (t < nbasis) {  // column t of L_A^-1
            for (int i = 0; i < nbasis; ++i) {
                T s = i == t ? (T)1 : (T)0;
                for (int k = 0; k < i; ++k) s -= sA[i * 17 + k] * sLi[k * 17 + t];
                sLi[i * 17 + t] = s * sA[i * 17 + i];
            }
        }
        __syncthreads();
        for (size_t e = t; e < K * K; e += GL_THREADS) {
            const size_t b = e / K, b2 = e - b * K;
            if (b < b2) continue;
            T a = 0;
            for (size_t i = b; i < K; ++i) a += sLi[i * 17 + b] * sLi[i * 17 + b2];
            Cb[k_mat * K * K + b * K + b2] = a;
            Cb[k_mat * K * K + b2 * K + b] = a;
        }
    }
    for (size_t s = t; s < nd; s += GL_THREADS) {
        const T *y = Ys + (k_mat * nd + s) * n;
        T *v = V + (K + s) * n, *be = Bt + s * K;
        for (size_t b = 0; b < K; ++b) {
            const T *kh = V + b * n;
            T a = 0;
            for (int i = 0; i < n; ++i) a += kh[i] * y[i];
            be[b] = a;
        }
        for (int i = 0; i < nbasis; ++i) {
            T a = be[i];
            for (int k = 0; k < i; ++k) a -= sA[i * 17 + k] * be[k];
            be[i] = a * sA[i * 17 + i];
        }
        for (int i = nbasis - 1; i >= 0; --i) {
            T a = be[i];
            for (int k = nbasis - 1; k > i; --k) a -= sA[k * 17 + i] * be[k];
            be[i] = a * sA[i * 17 + i];
        }
        for (size_t b = 0; b < K; ++b) {
            const T *kh = V + b * n;
            const T bb = be[b];
            for (int i = 0; i < n; ++i) v[i] -= kh[i] * bb;
        }
        T qd = 0;
        for (int i = 0; i < n; ++i) qd += y[i] * v[i];
        if (Be)
            for (size_t b = 0; b < K; ++b) Be[(k_mat * nd + s) * K + b] = be[b];
        if (Al)
            for (int i = 0; i < n; ++i) Al[(k_mat * nd + s) * n + i] = v[i];
        if (Qd) Qd[k_mat * nd + s] = qd;
        // log 2 pi
        if (Lm) Lm[k_mat * nd + s] = (T)-0.5 * ((qd + (ld + ldA)) + (T)(n - nbasis) * (T)1.83787706640934548356);
    }
    if (Mn) {  // block-uniform
        __syncthreads();  // every target's alpha is in V, its beta in Bt
        for (size_t e = t; e < nd * nq; e += GL_THREADS) {
            const size_t s = e / nq, j = e - s * nq;
            const T *a = As + (k_mat * nq + j) * n, *v = V + (K + s) * n, *g = Gs + (k_mat * nq + j) * K, *be = Bt + s * K;
            T m = 0, mb = 0;
            for (int i = 0; i < n; ++i) m += a[i] * v[i];
            for (size_t b = 0; b < K; ++b) mb += g[b] * be[b];
            Mn[k_mat * nd * nq + e] = m + mb;
        }
    }
    for (size_t j = t; j < nqv; j += GL_THREADS) {
        const T *a = As + (k_mat * nq + j) * n, *g = Gs + (k_mat * nq + j) * K;
        T *w = U + j * n, *r = R + j * K;
        for (size_t b = 0; b < K; ++b) {
            const T *kh = V + b * n;
            T s = 0;
            for (int i = 0; i < n; ++i) s += kh[i] * a[i];
            r[b] = g[b] - s;
        }
        for (int i = 0; i < n; ++i) w[i] = a[i];
        T aka = 0;
        for (int k = 0; k < n; ++k) {
            const T *lk = W + (size_t)k * n;
            const T x = w[k] / lk[k];
            aka += x * x;
            for (int i = k + 1; i < n; ++i) w[i] -= lk[i] * x;
        }
        T rar = 0;
        for (int i = 0; i < nbasis; ++i) {
            T s = r[i];
            for (int k = 0; k < i; ++k) s -= sA[i * 17 + k] * r[k];
            s *= sA[i * 17 + i];
            r[i] = s;
            rar += s * s;
        }
        Vr[k_mat * nq + j] = (Es[k_mat * nq + j] - aka) + rar;
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_trend_global(int n, int nbasis, int ntarget, int nquery, const T *Bs, const T *Cs, const T *Hs, const T *Ys, const T *As,
                               const T *Gs, const T *Es, T *Be, T *Cb, T *Al, T *Qd, T *Lm, T *Mn, T *Vr, size_t batch, int *info,
                               hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk fit the blocked-path workspace cap (launch_multi_target_global)
    const size_t nd = (Be || Al || Qd || Lm || Mn) ? (size_t)ntarget : 0, nqv = Vr ? (size_t)nquery : 0, K = (size_t)nbasis;
    const size_t per = (size_t)n * n + (size_t)n * (K + nd) + K * nd + ((size_t)n + K) * nqv;
    size_t chunk = blocked_workspace_cap() / (per * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * per * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true, true, true, true, true, true, true, true, true>), dim3((unsigned)cnt),
                           dim3(GL_THREADS), 0, stream, Bs, Cs, Hs, Ys, As, Gs, Es, nbasis, ntarget, nquery, Be, Cb, Al, Qd, Lm, Mn, Vr, info,
                           n, ws, per, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_trend_global<double>(int, int, int, int, const double *, const double *, const double *, const double *,
                                                const double *, const double *, const double *, double *, double *, double *, double *,
                                                double *, double *, double *, size_t, int *, hipStream_t);
template hipError_t launch_trend_global<float>(int, int, int, int, const float *, const float *, const float *, const float *, const float *,
                                               const float *, const float *, float *, float *, float *, float *, float *, float *, float *,
                                               size_t, int *, hipStream_t);

const char *name_trend_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true, true, true, true, true, true, true, true, true>"
               : "matinv_chol_global<float, true, true, true, true, true, true, true, true, true, true>";
}

// ---- gradients of the restricted log marginal likelihood of the trend model, 96 < n <= 1024 (matinv_trend_grad_batched behind
// trend_grad_tile_impl.hpp) ---------------------------------------------------------------------------------------------------------------
// The trend gradient form of matinv_chol_global: one more template argument again ("Gradients of the restricted log marginal
// likelihood"). The factorisation, the diagonal fold, the substitutions on [H | Y], A = H^T Kinv H, its factor, beta and alpha are those of
// the trend form above, so logml, alpha and beta are its values; Kinv h_b and alpha_t stay in scratch behind the factor. Then, when grad
// or gradc is asked for, L <- L^-1 and Kinv over it in place as in the multi-target gradient form, L_A^-1 column by column, and
// V = Kinv H L_A^-T over Kinv H, one thread per row, b descending (V_ib needs the columns b' <= b only). With
//     G_rc = sum_t alpha_tr alpha_tc - D (Kinv_rc - sum_b V_rb V_cb)          (t and b ascending)
// formed on the fly: gradc_i = 1/2 G_ii, grad_p = sum_{r >= c} w_rc G_rc dM_p[r][c], w = 1/2 on the diagonal, 1 below, summed per thread
// in element order, then on the fixed LDS tree. info and the NaN outputs as in the trend form. Correct first; speed is not a goal here.
// Workgroup blockIdx.x serves matrix first + blockIdx.x; `per` = n^2 + n (K + D) + K D elements of workspace each.
template <class T, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD, bool TREND,
          bool TRENDGRAD>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Bs, const T *Cs, const T *Hs, const T *Ys, const T *dMs, int nbasis,
                                                                 int ntarget, int nparam, T *grad, T *gradc, T *Lm, T *Al, T *Be, int *info,
                                                                 int n, T *workspace, size_t per, size_t first)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN && MULTI && MTGRAD && TREND && TRENDGRAD,
                  "the twelve-argument form is the trend gradient kernel");
    __shared__ T col[1024];
    __shared__ T sA[16 * 17], sLi[16 * 17];
    __shared__ T s_ld, s_ldA;
    __shared__ int s_abad;
    const size_t k_mat = first + blockIdx.x;
    const T *A = Bs + k_mat * (size_t)n * n;
    const size_t nn = (size_t)n * n, K = (size_t)nbasis, nd = (size_t)ntarget;
    T *W = workspace + (size_t)blockIdx.x * per;
    T *V = W + nn;             // Kinv h_b, b < K, then Kinv y_t -> alpha_t
    T *Bt = V + (K + nd) * n;  // beta_t
    const int t = threadIdx.x;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        T v = A[e];
        if (Cs && r == c) v += Cs[k_mat * n + r];
        W[e] = v;
    }
    __syncthreads();
    int bad = gl_chol_factor(W, n, col);
    if (!bad) {  // block-uniform
        if (t == 0) {
            PivotProduct<T> prod;
            for (int i = 0; i < n; ++i) prod.fold(W[(size_t)i * n + i]);
            s_ld = (T)2 * prod.log_value();
        }
        for (size_t s = t; s < K + nd; s += GL_THREADS) {
            const T *x = s < K ? Hs + (k_mat * K + s) * n : Ys + (k_mat * nd + (s - K)) * n;
            T *v = V + s * n;
            for (int i = 0; i < n; ++i) v[i] = x[i];
            for (int k = 0; k < n; ++k) {
                const T *lk = W + (size_t)k * n;
                const T w = v[k] / lk[k];
                v[k] = w;
                for (int i = k + 1; i < n; ++i) v[i] -= lk[i] * w;
            }
            for (int k = n - 1; k >= 0; --k) {
                const T *lk = W + (size_t)k * n;
                T a = v[k];
                for (int i = k + 1; i < n; ++i) a -= lk[i] * v[i];
                v[k] = a / lk[k];
            }
        }
        __syncthreads();  // Kinv [H | Y] is in V
        for (size_t e = t; e < K * K; e += GL_THREADS) {
            const size_t b = e / K, b2 = e - b * K;
            if (b < b2) continue;
            const T *h = Hs + (k_mat * K + b) * n, *v = V + b2 * n;
            T a = 0;
            for (int i = 0; i < n; ++i) a += h[i] * v[i];
            sA[b * 17 + b2] = a;
        }
        __syncthreads();
        if (t == 0) {  // A = L_A L_A^T in place, 1 / L_bb on the diagonal (the trend form)
            int abad = 0;
            PivotProduct<T> prod;
            for (int j = 0; j < nbasis; ++j) {
                const T d = sA[j * 17 + j];
                if (!(d > (T)0) && abad == 0) abad = j + 1;
                prod.fold(d);
                const T rs = (T)1 / sqrt(d);
                for (int jj = j + 1; jj < nbasis; ++jj) {
                    const T m = sA[jj * 17 + j] / d;
                    for (int i = jj; i < nbasis; ++i) sA[i * 17 + jj] -= sA[i * 17 + j] * m;
                }
                sA[j * 17 + j] = rs;
                for (int i = j + 1; i < nbasis; ++i) sA[i * 17 + j] *= rs;
            }
            s_abad = abad;
            s_ldA = prod.log_value();
        }
        __syncthreads();
        if (s_abad) bad = n + s_abad;
    }
    if (bad) {  // block-uniform
        if (Be)
            for (size_t e = t; e < nd * K; e += GL_THREADS) Be[k_mat * nd * K + e] = nan_of<T>();
        if (Al)
            for (size_t e = t; e < nd * n; e += GL_THREADS) Al[k_mat * nd * n + e] = nan_of<T>();
        if (Lm)
            for (size_t s = t; s < nd; s += GL_THREADS) Lm[k_mat * nd + s] = nan_of<T>();
        if (gradc)
            for (int i = t; i < n; i += GL_THREADS) gradc[k_mat * n + i] = nan_of<T>();
        if (grad)
            for (int p = t; p < nparam; p += GL_THREADS) grad[k_mat * nparam + p] = nan_of<T>();
        if (info && t == 0) info[k_mat] = bad;
        return;
    }
    const T ld = s_ld, ldA = s_ldA;
    for (size_t s = t; s < nd; s += GL_THREADS) {
        const T *y = Ys + (k_mat * nd + s) * n;
        T *v = V + (K + s) * n, *be = Bt + s * K;
        for (size_t b = 0; b < K; ++b) {
            const T *kh = V + b * n;
            T a = 0;
            for (int i = 0; i < n; ++i) a += kh[i] * y[i];
            be[b] = a;
        }
        for (int i = 0; i < nbasis; ++i) {
            T a = be[i];
            for (int k = 0; k < i; ++k) a -= sA[i * 17 + k] * be[k];
            be[i] = a * sA[i * 17 + i];
        }
        for (int i = nbasis - 1; i >= 0; --i) {
            T a = be[i];
            for (int k = nbasis - 1; k > i; --k) a -= sA[k * 17 + i] * be[k];
            be[i] = a * sA[i * 17 + i];
        }
        for (size_t b = 0; b < K; ++b) {
            const T *kh = V + b * n;
            const T bb = be[b];
            for (int i = 0; i < n; ++i) v[i] -= kh[i] * bb;
        }
        T qd = 0;
        for (int i = 0; i < n; ++i) qd += y[i] * v[i];
        if (Be)
            for (size_t b = 0; b < K; ++b) Be[(k_mat * nd + s) * K + b] = be[b];
        if (Al)
            for (int i = 0; i < n; ++i) Al[(k_mat * nd + s) * n + i] = v[i];
        // log 2 pi
        if (Lm) Lm[k_mat * nd + s] = (T)-0.5 * ((qd + (ld + ldA)) + (T)(n - nbasis) * (T)1.83787706640934548356);
    }
    if (grad || gradc) {  // block-uniform
        __syncthreads();  // every target's alpha is in V behind Kinv H, and the factor is no longer needed
        for (int j = n - 1; j >= 0; --j) {  // L <- L^-1 in place, last column first (the loop of the inverse kernel)
            const T ajj = (T)1 / W[(size_t)j * n + j];
            for (int i = j + 1 + t; i < n; i += GL_THREADS) col[i] = W[(size_t)j * n + i];
            __syncthreads();
            for (int i = j + 1 + t; i < n; i += GL_THREADS) {
                T s = 0;
                for (int k = j + 1; k <= i; ++k) s += W[(size_t)k * n + i] * col[k];
                W[(size_t)j * n + i] = -s * ajj;
            }
            if (t == 0) W[(size_t)j * n + j] = ajj;
            __syncthreads();
        }
        // column c of Kinv over column c of L^-1; the columns beyond c are still those of L^-1
        for (int c = 0; c < n; ++c) {
            for (int k = c + t; k < n; k += GL_THREADS) col[k] = W[(size_t)c * n + k];
            __syncthreads();
            for (int r = c + t; r < n; r += GL_THREADS) {
                T s = 0;
                if (r == c) {
                    for (int k = r; k < n; ++k) s += col[k] * col[k];
                } else {
                    for (int k = r; k < n; ++k) s += W[(size_t)r * n + k] * col[k];
                }
                W[(size_t)c * n + r] = s;
            }
            __syncthreads();
        }
        if (t < nbasis) {  // column t of L_A^-1 (the trend form's, for covbeta)
            for (int i = 0; i < nbasis; ++i) {
                T s = i == t ? (T)1 : (T)0;
                for (int k = 0; k < i; ++k) s -= sA[i * 17 + k] * sLi[k * 17 + t];
                sLi[i * 17 + t] = s * sA[i * 17 + i];
            }
        }
        __syncthreads();
        // V = Kinv H L_A^-T over Kinv H: V_ib = sum_{b' <= b} (Kinv H)_ib' L_A^-1[b][b'], b descending, b' ascending
        for (int i = t; i < n; i += GL_THREADS)
            for (int b = nbasis - 1; b >= 0; --b) {
                T s = 0;
                for (int b2 = 0; b2 <= b; ++b2) s += V[(size_t)b2 * n + i] * sLi[b * 17 + b2];
                V[(size_t)b * n + i] = s;
            }
        __syncthreads();
        const T dscale = (T)ntarget;
        const T *Va = V + K * n;  // alpha_t
        if (gradc)
            for (int i = t; i < n; i += GL_THREADS) {
                T aa = 0, uu = 0;
                for (size_t s = 0; s < nd; ++s) aa += Va[s * n + i] * Va[s * n + i];
                for (size_t b = 0; b < K; ++b) uu += V[b * n + i] * V[b * n + i];
                gradc[k_mat * n + i] = (T)0.5 * (aa - dscale * (W[(size_t)i * n + i] - uu));
            }
        if (grad) {
            for (int p = 0; p < nparam; ++p) {
                const T *D = dMs + (k_mat * nparam + p) * nn;
                T s = 0;
                for (size_t e = t; e < nn; e += GL_THREADS) {
                    const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
                    if (r < c) continue;
                    T aa = 0, uu = 0;
                    for (size_t u = 0; u < nd; ++u) aa += Va[u * n + r] * Va[u * n + c];
                    for (size_t b = 0; b < K; ++b) uu += V[b * n + r] * V[b * n + c];
                    const T g = aa - dscale * (W[e] - uu);
                    s += (r == c ? (T)0.5 : (T)1) * g * D[e];
                }
                // block sum on a fixed tree
                col[t] = s;
                __syncthreads();
                for (int off = GL_THREADS / 2; off >= 1; off >>= 1) {
                    if (t < off) col[t] += col[t + off];
                    __syncthreads();
                }
                if (t == 0) grad[k_mat * nparam + p] = col[0];
                __syncthreads();
            }
        }
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_trend_grad_global(int n, int nbasis, int ntarget, int nparam, const T *Bs, const T *Cs, const T *Hs, const T *Ys,
                                    const T *dMs, T *grad, T *gradc, T *Lm, T *Al, T *Be, size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk fit the blocked-path workspace cap (launch_trend_global)
    const size_t nd = (size_t)ntarget, K = (size_t)nbasis;
    const size_t per = (size_t)n * n + (size_t)n * (K + nd) + K * nd;
    size_t chunk = blocked_workspace_cap() / (per * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * per * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true, true, true, true, true, true, true, true, true, true>), dim3((unsigned)cnt),
                           dim3(GL_THREADS), 0, stream, Bs, Cs, Hs, Ys, dMs, nbasis, ntarget, nparam, grad, gradc, Lm, Al, Be, info, n, ws,
                           per, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_trend_grad_global<double>(int, int, int, int, const double *, const double *, const double *, const double *,
                                                     const double *, double *, double *, double *, double *, double *, size_t, int *,
                                                     hipStream_t);
template hipError_t launch_trend_grad_global<float>(int, int, int, int, const float *, const float *, const float *, const float *,
                                                    const float *, float *, float *, float *, float *, float *, size_t, int *, hipStream_t);

const char *name_trend_grad_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true, true, true, true, true, true, true, true, true, true>"
               : "matinv_chol_global<float, true, true, true, true, true, true, true, true, true, true, true>";
}

// ---- leave-one-out cross-validation of the trend model, 96 < n <= 1024 (matinv_trend_loo_batched behind trend_loo_tile_impl.hpp) ---------
// The trend leave-one-out form of matinv_chol_global: one more template argument again ("Leave-one-out cross-validation of the
// trend model"). The factorisation, the substitutions on [H | Y], A = H^T Kinv H, its factor, beta and alpha are those of the trend form
// above; Kinv h_b and alpha_t stay in scratch behind the factor. Then L <- L^-1 in place as in the trend gradient form, L_A^-1 column by
// column, and one thread per point:
//     P_ii = sum_{k >= i} (L^-1)_ki^2 - sum_b U_ib^2,   U_ib = sum_{b' <= b} (Kinv H)_ib' L_A^-1[b][b']     (k, b, b' ascending)
// into LDS; the first i with P_ii not > 0 by an atomic minimum. rp = 1 / P_ii is formed the same way wherever it is used:
//     var_i = rp      mean_ti = y_ti - alpha_ti rp      logpl_t = sum_i (1/2 log P_ii - 1/2 alpha_ti (alpha_ti rp)) - n/2 log 2 pi
// one thread per point, per (target, point) pair and per target (i ascending). The order of operations of an output knows nothing of D, of
// the position of its target, or of which outputs are stored. info: gl_chol_factor's column, n + b for pivot b of A (both as the trend
// form), n + K + i for the first such point i (1-based); every requested output of that matrix is then NaN. Correct first; speed is not a
// goal here. Workgroup blockIdx.x serves matrix first + blockIdx.x; `per` = n^2 + n (K + D') + K D' elements of workspace each, D' = D
// when the targets are read.
template <class T, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD, bool TREND,
          bool TRENDGRAD, bool TRENDLOO>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Bs, const T *Cs, const T *Hs, const T *Ys, int nbasis, int ntarget,
                                                                 T *Mn, T *Vr, T *Lp, int *info, int n, T *workspace, size_t per, size_t first)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN && MULTI && MTGRAD && TREND && TRENDGRAD && TRENDLOO,
                  "the thirteen-argument form is the trend leave-one-out kernel");
    __shared__ T col[1024];
    __shared__ T sA[16 * 17], sLi[16 * 17];
    __shared__ int s_abad, s_pbad;
    const size_t k_mat = first + blockIdx.x;
    const T *A = Bs + k_mat * (size_t)n * n;
    const bool targets = Mn || Lp;  // block-uniform
    const size_t nn = (size_t)n * n, K = (size_t)nbasis, nd = targets ? (size_t)ntarget : 0;
    T *W = workspace + (size_t)blockIdx.x * per;
    T *V = W + nn;             // Kinv h_b, b < K, then Kinv y_t -> alpha_t
    T *Bt = V + (K + nd) * n;  // beta_t
    const int t = threadIdx.x;
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        T v = A[e];
        if (Cs && r == c) v += Cs[k_mat * n + r];
        W[e] = v;
    }
    if (t == 0) s_pbad = 0x7fffffff;
    __syncthreads();
    int bad = gl_chol_factor(W, n, col);
    if (!bad) {  // block-uniform
        for (size_t s = t; s < K + nd; s += GL_THREADS) {
            const T *x = s < K ? Hs + (k_mat * K + s) * n : Ys + (k_mat * nd + (s - K)) * n;
            T *v = V + s * n;
            for (int i = 0; i < n; ++i) v[i] = x[i];
            for (int k = 0; k < n; ++k) {
                const T *lk = W + (size_t)k * n;
                const T w = v[k] / lk[k];
                v[k] = w;
                for (int i = k + 1; i < n; ++i) v[i] -= lk[i] * w;
            }
            for (int k = n - 1; k >= 0; --k) {
                const T *lk = W + (size_t)k * n;
                T a = v[k];
                for (int i = k + 1; i < n; ++i) a -= lk[i] * v[i];
                v[k] = a / lk[k];
            }
        }
        __syncthreads();  // Kinv [H | Y] is in V
        for (size_t e = t; e < K * K; e += GL_THREADS) {
            const size_t b = e / K, b2 = e - b * K;
            if (b < b2) continue;
            const T *h = Hs + (k_mat * K + b) * n, *v = V + b2 * n;
            T a = 0;
            for (int i = 0; i < n; ++i) a += h[i] * v[i];
            sA[b * 17 + b2] = a;
        }
        __syncthreads();
        if (t == 0) {  // A = L_A L_A^T in place, 1 / L_bb on the diagonal (the trend form)
            int abad = 0;
            for (int j = 0; j < nbasis; ++j) {
                const T d = sA[j * 17 + j];
                if (!(d > (T)0) && abad == 0) abad = j + 1;
                const T rs = (T)1 / sqrt(d);
                for (int jj = j + 1; jj < nbasis; ++jj) {
                    const T m = sA[jj * 17 + j] / d;
                    for (int i = jj; i < nbasis; ++i) sA[i * 17 + jj] -= sA[i * 17 + j] * m;
                }
                sA[j * 17 + j] = rs;
                for (int i = j + 1; i < nbasis; ++i) sA[i * 17 + j] *= rs;
            }
            s_abad = abad;
        }
        __syncthreads();
        if (s_abad) bad = n + s_abad;
    }
    if (!bad) {  // block-uniform
        if (t < nbasis) {  // column t of L_A^-1 (the trend form's, for covbeta)
            for (int i = 0; i < nbasis; ++i) {
                T s = i == t ? (T)1 : (T)0;
                for (int k = 0; k < i; ++k) s -= sA[i * 17 + k] * sLi[k * 17 + t];
                sLi[i * 17 + t] = s * sA[i * 17 + i];
            }
        }
        for (size_t s = t; s < nd; s += GL_THREADS) {  // beta and alpha as in the trend form
            const T *y = Ys + (k_mat * nd + s) * n;
            T *v = V + (K + s) * n, *be = Bt + s * K;
            for (size_t b = 0; b < K; ++b) {
                const T *kh = V + b * n;
                T a = 0;
                for (int i = 0; i < n; ++i) a += kh[i] * y[i];
                be[b] = a;
            }
            for (int i = 0; i < nbasis; ++i) {
                T a = be[i];
                for (int k = 0; k < i; ++k) a -= sA[i * 17 + k] * be[k];
                be[i] = a * sA[i * 17 + i];
            }
            for (int i = nbasis - 1; i >= 0; --i) {
                T a = be[i];
                for (int k = nbasis - 1; k > i; --k) a -= sA[k * 17 + i] * be[k];
                be[i] = a * sA[i * 17 + i];
            }
            for (size_t b = 0; b < K; ++b) {
                const T *kh = V + b * n;
                const T bb = be[b];
                for (int i = 0; i < n; ++i) v[i] -= kh[i] * bb;
            }
        }
        __syncthreads();  // the factor is no longer needed; L_A^-1 is in sLi
        for (int j = n - 1; j >= 0; --j) {  // L <- L^-1 in place, last column first (the loop of the inverse kernel)
            const T ajj = (T)1 / W[(size_t)j * n + j];
            for (int i = j + 1 + t; i < n; i += GL_THREADS) col[i] = W[(size_t)j * n + i];
            __syncthreads();
            for (int i = j + 1 + t; i < n; i += GL_THREADS) {
                T s = 0;
                for (int k = j + 1; k <= i; ++k) s += W[(size_t)k * n + i] * col[k];
                W[(size_t)j * n + i] = -s * ajj;
            }
            if (t == 0) W[(size_t)j * n + j] = ajj;
            __syncthreads();
        }
        for (int i = t; i < n; i += GL_THREADS) {
            T kii = 0, uu = 0;
            for (int k = i; k < n; ++k) kii += W[(size_t)i * n + k] * W[(size_t)i * n + k];
            for (int b = 0; b < nbasis; ++b) {
                T s = 0;
                for (int b2 = 0; b2 <= b; ++b2) s += V[(size_t)b2 * n + i] * sLi[b * 17 + b2];
                uu += s * s;
            }
            const T p = kii - uu;
            col[i] = p;
            if (!(p > (T)0)) atomicMin(&s_pbad, i + 1);
        }
        __syncthreads();
        if (s_pbad != 0x7fffffff) bad = n + nbasis + s_pbad;
    }
    if (bad) {  // block-uniform
        if (Mn)
            for (size_t e = t; e < nd * n; e += GL_THREADS) Mn[k_mat * nd * n + e] = nan_of<T>();
        if (Vr)
            for (int i = t; i < n; i += GL_THREADS) Vr[k_mat * n + i] = nan_of<T>();
        if (Lp)
            for (size_t s = t; s < nd; s += GL_THREADS) Lp[k_mat * nd + s] = nan_of<T>();
        if (info && t == 0) info[k_mat] = bad;
        return;
    }
    if (Vr)
        for (int i = t; i < n; i += GL_THREADS) Vr[k_mat * n + i] = (T)1 / col[i];
    if (Mn)
        for (size_t e = t; e < nd * n; e += GL_THREADS) {
            const size_t i = e % n;
            Mn[k_mat * nd * n + e] = Ys[k_mat * nd * n + e] - V[K * n + e] * ((T)1 / col[i]);
        }
    if (Lp)
        for (size_t s = t; s < nd; s += GL_THREADS) {
            const T *v = V + (K + s) * n;
            T a = 0;
            for (int i = 0; i < n; ++i) {
                const T p = col[i], al = v[i];
                a += (T)0.5 * log(p) - (T)0.5 * al * (al * ((T)1 / p));
            }
            // 1/2 log 2 pi
            Lp[k_mat * nd + s] = a - (T)n * (T)0.91893853320467274178;
        }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_trend_loo_global(int n, int nbasis, int ntarget, const T *Bs, const T *Cs, const T *Hs, const T *Ys, T *Mn, T *Vr, T *Lp,
                                   size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk fit the blocked-path workspace cap (launch_trend_global)
    const size_t nd = (Mn || Lp) ? (size_t)ntarget : 0, K = (size_t)nbasis;
    const size_t per = (size_t)n * n + (size_t)n * (K + nd) + K * nd;
    size_t chunk = blocked_workspace_cap() / (per * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * per * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true, true, true, true, true, true, true, true, true, true, true>),
                           dim3((unsigned)cnt), dim3(GL_THREADS), 0, stream, Bs, Cs, Hs, Ys, nbasis, ntarget, Mn, Vr, Lp, info, n, ws, per,
                           off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_trend_loo_global<double>(int, int, int, const double *, const double *, const double *, const double *, double *,
                                                    double *, double *, size_t, int *, hipStream_t);
template hipError_t launch_trend_loo_global<float>(int, int, int, const float *, const float *, const float *, const float *, float *,
                                                   float *, float *, size_t, int *, hipStream_t);

const char *name_trend_loo_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true, true, true, true, true, true, true, true, true, true, true>"
               : "matinv_chol_global<float, true, true, true, true, true, true, true, true, true, true, true, true>";
}

// ---- GP log marginal likelihood and its gradient from coordinates, 96 < n <= 1024 (matinv_ard_logml_batched behind ard_tile_impl.hpp) ---
// The ARD form of matinv_chol_global: one more template argument again ("Hyperparameter fits from coordinates"). The matrix is
// never read: z = x / l goes to the n ndim elements of scratch behind the working copy (dimension k at Z + k n), and the lower triangle of
// M = sf2 phi(s) + sn2 I is GENERATED into the working copy with the element function of the tile kernels (ard_element.hpp). It is factored
// and the factor inverted in place as in the log-marginal-likelihood gradient form; thread 0 folds the diagonal of L into a PivotProduct
// (logdet = 2 log prod L_ii) before the inversion. Then alpha = L^-T (L^-1 y), y^T alpha on a fixed LDS tree, K over L^-1 one column at
// a time, and with w = 1/2 on the diagonal and 1 below:
//     one pass over the lower triangle regenerates s_rc, sums w G_rc sf2 phi into grad[0] and G_rr into grad[ndim + 1] and leaves
//     w G_rc sf2 psi(s_rc) in place of K_rc; one pass per dimension k sums W_rc (z_rk - z_ck)^2.
// Every sum is per thread in element order, then on a fixed LDS tree. Not SPD: info = the failing column + 1 and every requested output
// NaN. Correct first; speed is not a goal here. Workgroup blockIdx.x serves matrix first + blockIdx.x; per = n^2 + n ndim elements of
// workspace each.
template <class T, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD, bool TREND,
          bool TRENDGRAD, bool TRENDLOO, bool ARD>
__global__ __launch_bounds__(GL_THREADS) void matinv_chol_global(const T *Xs, size_t xstride, const T *Ys, size_t ystride, const T *Th,
                                                                 int ndim, int kind, T *Lm, T *Gr, T *Al, int *info, int n, T *workspace,
                                                                 size_t per, size_t first)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN && MULTI && MTGRAD && TREND && TRENDGRAD && TRENDLOO && ARD,
                  "the fourteen-argument form is the ARD log-marginal-likelihood kernel");
    __shared__ T col[1024], va[1024], vy[1024];
    __shared__ T s_ld;
    const size_t k_mat = first + blockIdx.x;
    const int t = threadIdx.x;
    const size_t nn = (size_t)n * n;
    T *W = workspace + (size_t)blockIdx.x * per;
    T *Z = W + nn;
    const T *th = Th + k_mat * (size_t)(ndim + 2);
    const T sf2 = ard_exp(th[0]), sn2 = ard_exp(th[ndim + 1]);
    T *const gm = Gr ? Gr + k_mat * (size_t)(ndim + 2) : nullptr;
    if (t < ndim) col[t] = ard_exp(th[1 + t]);
    __syncthreads();
    {
        const T *X = Xs + k_mat * xstride, *Y = Ys + k_mat * ystride;
        for (int e = t; e < n * ndim; e += GL_THREADS) {
            const int i = e / ndim, k = e - i * ndim;
            Z[(size_t)k * n + i] = X[e] / col[k];
        }
        for (int i = t; i < n; i += GL_THREADS) va[i] = Y[i];
    }
    __syncthreads();
    // s_rc in the order k = 0 .. ndim - 1
    auto sqdist = [&](int r, int c) {
        T s = 0;
        for (int k = 0; k < ndim; ++k) {
            const T d = Z[(size_t)k * n + r] - Z[(size_t)k * n + c];
            s = ard_fma(d, d, s);
        }
        return s;
    };
    // block sum on a fixed tree; every thread returns with the sum
    auto block_sum = [&](T v) {
        __syncthreads();
        col[t] = v;
        __syncthreads();
        for (int off = GL_THREADS / 2; off >= 1; off >>= 1) {
            if (t < off) col[t] += col[t + off];
            __syncthreads();
        }
        return col[0];
    };
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        W[e] = ard_m(sqdist(r, c), kind, sf2, sn2, r == c);
    }
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {  // block-uniform
        if (Al)
            for (int i = t; i < n; i += GL_THREADS) Al[k_mat * n + i] = nan_of<T>();
        if (gm)
            for (int p = t; p < ndim + 2; p += GL_THREADS) gm[p] = nan_of<T>();
        if (t == 0) {
            if (Lm) Lm[k_mat] = nan_of<T>();
            if (info) info[k_mat] = bad;
        }
        return;
    }
    if (t == 0) {
        PivotProduct<T> prod;
        for (int i = 0; i < n; ++i) prod.fold(W[(size_t)i * n + i]);
        s_ld = (T)2 * prod.log_value();
    }
    for (int j = n - 1; j >= 0; --j) {  // L <- L^-1 in place, last column first (the loop of the inverse kernel)
        const T ajj = (T)1 / W[(size_t)j * n + j];
        for (int i = j + 1 + t; i < n; i += GL_THREADS) col[i] = W[(size_t)j * n + i];
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += GL_THREADS) {
            T s = 0;
            for (int k = j + 1; k <= i; ++k) s += W[(size_t)k * n + i] * col[k];
            W[(size_t)j * n + i] = -s * ajj;
        }
        if (t == 0) W[(size_t)j * n + j] = ajj;
        __syncthreads();
    }
    // y = L^-1 d: (L^-1)_kj sits at W[j*n + k]
    for (int k = t; k < n; k += GL_THREADS) {
        T s = 0;
        for (int j = 0; j <= k; ++j) s += W[(size_t)j * n + k] * va[j];
        vy[k] = s;
    }
    __syncthreads();
    // alpha_i = column i of L^-1 against y; it takes the place of y once y_i alpha_i is taken
    T qpart = 0;
    for (int i = t; i < n; i += GL_THREADS) {
        T a = 0;
        for (int k = i; k < n; ++k) a += W[(size_t)i * n + k] * vy[k];
        qpart += va[i] * a;
        va[i] = a;
        if (Al) Al[k_mat * n + i] = a;
    }
    const T quad = block_sum(qpart);
    // log 2 pi
    if (Lm && t == 0) Lm[k_mat] = (T)-0.5 * ((quad + s_ld) + (T)n * (T)1.83787706640934548356);
    if (gm) {  // block-uniform
        __syncthreads();
        // column c of K over column c of L^-1; the columns beyond c are still those of L^-1
        for (int c = 0; c < n; ++c) {
            for (int k = c + t; k < n; k += GL_THREADS) col[k] = W[(size_t)c * n + k];
            __syncthreads();
            for (int r = c + t; r < n; r += GL_THREADS) {
                T s = 0;
                if (r == c) {
                    for (int k = r; k < n; ++k) s += col[k] * col[k];
                } else {
                    for (int k = r; k < n; ++k) s += W[(size_t)r * n + k] * col[k];
                }
                W[(size_t)c * n + r] = s;
            }
            __syncthreads();
        }
        T p0 = 0, pn = 0;
        for (size_t e = t; e < nn; e += GL_THREADS) {
            const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
            if (r < c) continue;
            T phi, psi;
            ard_element(sqdist(r, c), kind, phi, psi);
            const T g = va[r] * va[c] - W[e];
            const T wg = (r == c ? (T)0.5 : (T)1) * g;
            if (r == c) pn += g;
            p0 += wg * (sf2 * phi);
            W[e] = wg * (sf2 * psi);
        }
        const T s0 = block_sum(p0);
        const T sn = block_sum(pn);
        if (t == 0) {
            gm[0] = s0;
            gm[ndim + 1] = ((T)0.5 * sn2) * sn;
        }
        for (int k = 0; k < ndim; ++k) {
            const T *zk = Z + (size_t)k * n;
            T s = 0;
            for (size_t e = t; e < nn; e += GL_THREADS) {
                const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
                if (r < c) continue;
                const T d = zk[r] - zk[c];
                s += W[e] * (d * d);
            }
            const T sk = block_sum(s);
            if (t == 0) gm[1 + k] = sk;
        }
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_ard_global(int kind, int n, int ndim, const T *Xs, size_t xstride, const T *Ys, size_t ystride, const T *Th, T *Lm, T *Gr,
                             T *Al, size_t batch, int *info, hipStream_t stream)
{
    if (!global_family_supports<T>(n) || ndim < 1 || ndim > ARD_MAX_DIM) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk fit the blocked-path workspace cap (launch_logml_grad_global)
    const size_t per = (size_t)n * n + (size_t)n * ndim;
    size_t chunk = blocked_workspace_cap() / (per * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * per * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_chol_global<T, true, true, true, true, true, true, true, true, true, true, true, true, true>),
                           dim3((unsigned)cnt), dim3(GL_THREADS), 0, stream, Xs, xstride, Ys, ystride, Th, ndim, kind, Lm, Gr, Al, info, n, ws,
                           per, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_ard_global<double>(int, int, int, const double *, size_t, const double *, size_t, const double *, double *, double *,
                                              double *, size_t, int *, hipStream_t);
template hipError_t launch_ard_global<float>(int, int, int, const float *, size_t, const float *, size_t, const float *, float *, float *,
                                             float *, size_t, int *, hipStream_t);

const char *name_ard_global(bool f64)
{
    return f64 ? "matinv_chol_global<double, true, true, true, true, true, true, true, true, true, true, true, true, true>"
               : "matinv_chol_global<float, true, true, true, true, true, true, true, true, true, true, true, true, true>";
}

// ---- GP prediction from coordinates, 96 < n <= 1024 (matinv_ard_predict_batched behind ard_predict_tile_impl.hpp) ------------------------
// Two forms above joined: the generation of the ARD form into the working copy (z behind it in scratch, dimension k at Z + k n), then the
// back end of the prediction form -- factor, L <- L^-1 in place, alpha (with mean only), and one query after the other:
//     a_j[i] = sf2 phi(sum_k (z_ik - zq_jk)^2) with the element function of the tile kernels, zq_j = xq_j / l in LDS,
//     v = L^-1 a_j,   var_j = sf2 - sum_k v_k^2,   mean_j = sum_k a_jk alpha_k      (both on the fixed LDS tree)
// in an order that knows nothing of Q. Not SPD: info = the failing column + 1 and every requested output NaN. Correct first; speed is not
// a goal here. Workgroup blockIdx.x serves matrix first + blockIdx.x; per = n^2 + n ndim elements of workspace each.
// The name is matinv_logdet_global's with a third template argument, not one more argument of matinv_chol_global ("Prediction
// from coordinates", says why).
template <class T, bool SPD, bool ARDPREDICT>
__global__ __launch_bounds__(GL_THREADS) void matinv_logdet_global(const T *Xs, size_t xstride, const T *Ys, size_t ystride, const T *Th,
                                                                   const T *Xqs, size_t xqstride, int nquery, int ndim, int kind, T *mean,
                                                                   T *var, int *info, int n, T *workspace, size_t per, size_t first)
{
    static_assert(SPD && ARDPREDICT, "the three-argument form is the prediction-from-coordinates kernel");
    __shared__ T col[1024], va[1024], vy[1024], vq[1024];
    __shared__ T ell[ARD_MAX_DIM], zq[ARD_MAX_DIM];
    const size_t k_mat = first + blockIdx.x;
    const int t = threadIdx.x;
    const size_t nn = (size_t)n * n;
    T *W = workspace + (size_t)blockIdx.x * per;
    T *Z = W + nn;
    const T *th = Th + k_mat * (size_t)(ndim + 2);
    const T sf2 = ard_exp(th[0]), sn2 = ard_exp(th[ndim + 1]);
    if (t < ndim) ell[t] = ard_exp(th[1 + t]);
    __syncthreads();
    {
        const T *X = Xs + k_mat * xstride;
        for (int e = t; e < n * ndim; e += GL_THREADS) {
            const int i = e / ndim, k = e - i * ndim;
            Z[(size_t)k * n + i] = X[e] / ell[k];
        }
        if (mean) {  // block-uniform: y is read for alpha only
            const T *Y = Ys + k_mat * ystride;
            for (int i = t; i < n; i += GL_THREADS) va[i] = Y[i];
        }
    }
    __syncthreads();
    // s_rc in the order k = 0 .. ndim - 1
    auto sqdist = [&](int r, int c) {
        T s = 0;
        for (int k = 0; k < ndim; ++k) {
            const T d = Z[(size_t)k * n + r] - Z[(size_t)k * n + c];
            s = ard_fma(d, d, s);
        }
        return s;
    };
    // column-major: element (r, c) at c*n + r; the lower triangle only (r >= c)
    for (size_t e = t; e < nn; e += GL_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (r < c) continue;
        W[e] = ard_m(sqdist(r, c), kind, sf2, sn2, r == c);
    }
    __syncthreads();
    const int bad = gl_chol_factor(W, n, col);
    if (bad) {  // block-uniform
        for (int j = t; j < nquery; j += GL_THREADS) {
            if (mean) mean[k_mat * nquery + j] = nan_of<T>();
            if (var) var[k_mat * nquery + j] = nan_of<T>();
        }
        if (info && t == 0) info[k_mat] = bad;
        return;
    }
    for (int j = n - 1; j >= 0; --j) {  // L <- L^-1 in place, last column first (the loop of the inverse kernel)
        const T ajj = (T)1 / W[(size_t)j * n + j];
        for (int i = j + 1 + t; i < n; i += GL_THREADS) col[i] = W[(size_t)j * n + i];
        __syncthreads();
        for (int i = j + 1 + t; i < n; i += GL_THREADS) {
            T s = 0;
            for (int k = j + 1; k <= i; ++k) s += W[(size_t)k * n + i] * col[k];
            W[(size_t)j * n + i] = -s * ajj;
        }
        if (t == 0) W[(size_t)j * n + j] = ajj;
        __syncthreads();
    }
    if (mean) {  // block-uniform
        // y = L^-1 d: (L^-1)_kj sits at W[j*n + k]
        for (int k = t; k < n; k += GL_THREADS) {
            T s = 0;
            for (int j = 0; j <= k; ++j) s += W[(size_t)j * n + k] * va[j];
            vy[k] = s;
        }
        __syncthreads();
        // alpha_i = column i of L^-1 against y; it takes the place of y
        for (int i = t; i < n; i += GL_THREADS) {
            T a = 0;
            for (int k = i; k < n; ++k) a += W[(size_t)i * n + k] * vy[k];
            va[i] = a;
        }
        __syncthreads();
    }
    const T *Xq = Xqs + k_mat * xqstride;
    for (int j = 0; j < nquery; ++j) {
        const size_t out = k_mat * nquery + j;
        if (t < ndim) zq[t] = Xq[(size_t)j * ndim + t] / ell[t];
        __syncthreads();
        for (int i = t; i < n; i += GL_THREADS) {
            T s = 0;
            for (int k = 0; k < ndim; ++k) {
                const T d = Z[(size_t)k * n + i] - zq[k];
                s = ard_fma(d, d, s);
            }
            vq[i] = ard_m(s, kind, sf2, sn2, false);
        }
        __syncthreads();
        T sq = 0, sm = 0;
        for (int k = t; k < n; k += GL_THREADS) {
            if (var) {  // v_k = row k of L^-1 against a
                T s = 0;
                for (int i = 0; i <= k; ++i) s += W[(size_t)i * n + k] * vq[i];
                sq += s * s;
            }
            if (mean) sm += vq[k] * va[k];
        }
        // block sums on a fixed tree
        col[t] = sq;
        vy[t] = sm;
        __syncthreads();
        for (int off = GL_THREADS / 2; off >= 1; off >>= 1) {
            if (t < off) {
                col[t] += col[t + off];
                vy[t] += vy[t + off];
            }
            __syncthreads();
        }
        if (t == 0) {
            if (var) var[out] = sf2 - col[0];
            if (mean) mean[out] = vy[0];
        }
        __syncthreads();  // the next query overwrites zq, vq, col and vy
    }
    if (info && t == 0) info[k_mat] = 0;
}

template <class T>
hipError_t launch_ard_predict_global(int kind, int n, int ndim, int nquery, const T *Xs, size_t xstride, const T *Ys, size_t ystride,
                                     const T *Th, const T *Xqs, size_t xqstride, T *mean, T *var, size_t batch, int *info,
                                     hipStream_t stream)
{
    if (!global_family_supports<T>(n) || ndim < 1 || ndim > ARD_MAX_DIM || nquery < 1) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // the working copies of a k-range chunk fit the blocked-path workspace cap (launch_ard_global)
    const size_t per = (size_t)n * n + (size_t)n * ndim;
    size_t chunk = blocked_workspace_cap() / (per * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * per * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        hipLaunchKernelGGL((matinv_logdet_global<T, true, true>), dim3((unsigned)cnt), dim3(GL_THREADS), 0, stream, Xs, xstride, Ys, ystride,
                           Th, Xqs, xqstride, nquery, ndim, kind, mean, var, info, n, ws, per, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template hipError_t launch_ard_predict_global<double>(int, int, int, int, const double *, size_t, const double *, size_t, const double *,
                                                      const double *, size_t, double *, double *, size_t, int *, hipStream_t);
template hipError_t launch_ard_predict_global<float>(int, int, int, int, const float *, size_t, const float *, size_t, const float *,
                                                     const float *, size_t, float *, float *, size_t, int *, hipStream_t);

const char *name_ard_predict_global(bool f64) { return f64 ? "matinv_logdet_global<double, true, true>" : "matinv_logdet_global<float, true, true>"; }

}  // namespace matinv
