// logdet_global_kernels.hip -- sign and log|det| for any n <= 1024: the functional path behind the tile and row kernels
// (logdet_tile_impl.hpp, logdet_row_kernels.hip), in the manner of the GLOBAL family (global_kernels.hip). One 1024-thread
// workgroup per matrix, the n x n working copy in library scratch (the input is never written), the launcher walks the batch in
// k-range chunks whose copies fit the blocked-path workspace cap.
//   SPD = false: unblocked LU with partial pivoting (rows exchanged in the copy); sign = exchange parity x pivot signs.
//   SPD = true : square-root-free Cholesky (L D L^T) on the lower triangle, every pivot must be positive; an optional `diag` is
//                added to the diagonal while copying, so the log marginal likelihood can use B + diag c without forming it.
// The pivots' magnitudes go into a mantissa / exponent pair, never into a product that could overflow; one logarithm at the end.
// info = k + 1 at the first step without a usable pivot, and both outputs NaN. Correct first: 2/3 n^3 sizeof(T) bytes of cache
// traffic per matrix, speed is not a goal here.
#include "pivot_product.hpp"

namespace matinv {

namespace {
constexpr int LG_THREADS = 1024;

// block-wide arg-max of (val, idx); lowest index wins ties. Result broadcast to every thread (gl_argmax of global_kernels.hip).
template <class T>
__device__ __forceinline__ void lg_argmax(T &best, int &bi, T *s_val, int *s_idx)
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
    for (int k = 1; k < LG_THREADS / 64; ++k) {
        T ob = s_val[k];
        int oi = s_idx[k];
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    __syncthreads();
}
}  // namespace

template <class T, bool SPD>
__global__ __launch_bounds__(LG_THREADS) void matinv_logdet_global(const T *As, size_t stride, const T *diag, T *workspace, T *logabs,
                                                                   T *sign, int *info, int n, size_t first)
{
    __shared__ T prow[1024], mcol[1024];
    __shared__ T s_val[LG_THREADS / 64];
    __shared__ int s_idx[LG_THREADS / 64];
    const size_t k_mat = first + blockIdx.x;
    const T *A = As + k_mat * stride;
    T *W = workspace + (size_t)blockIdx.x * n * n;
    const int t = threadIdx.x;
    const size_t nn = (size_t)n * n;
    // column-major: element (r, c) at c*n + r. SPD reads the lower triangle only (r >= c).
    for (size_t e = t; e < nn; e += LG_THREADS) {
        const int c = (int)(e / n), r = (int)(e - (size_t)c * n);
        if (SPD && r < c) continue;
        T v = A[e];
        if (diag && r == c) v += diag[k_mat * n + r];
        W[e] = v;
    }
    __syncthreads();

    PivotProduct<T> prod;  // the same in every thread
    unsigned negs = 0;
    int bad = 0;
    for (int k = 0; k < n; ++k) {
        T piv;
        if (SPD) {
            piv = W[(size_t)k * n + k];
            if (!(piv > 0)) { bad = k + 1; break; }  // block-uniform
            for (int i = k + 1 + t; i < n; i += LG_THREADS) mcol[i] = W[(size_t)k * n + i];
            __syncthreads();
            const T rd = (T)1 / piv;
            const size_t m = (size_t)(n - k - 1);
            for (size_t e = t; e < m * m; e += LG_THREADS) {  // trailing lower triangle: (i, j), j >= k+1, i >= j
                const int j = k + 1 + (int)(e / m), i = k + 1 + (int)(e % m);
                if (i >= j) W[(size_t)j * n + i] -= (mcol[i] * rd) * mcol[j];
            }
            __syncthreads();
        } else {
            T best = (T)-1;
            int bi = k;
            for (int i = k + t; i < n; i += LG_THREADS) {
                const T v = W[(size_t)k * n + i];
                const T av = v < 0 ? -v : v;
                if (av > best) { best = av; bi = i; }
            }
            lg_argmax(best, bi, s_val, s_idx);
            const int p = bi;
            if (!(best > 0) || !(best <= max_finite<T>())) { bad = k + 1; break; }  // block-uniform
            for (int c = k + t; c < n; c += LG_THREADS) {  // exchange rows k <-> p on the columns still live, lift the pivot row
                const T vp = W[(size_t)c * n + p], vk = W[(size_t)c * n + k];
                W[(size_t)c * n + p] = vk;
                W[(size_t)c * n + k] = vp;
                prow[c] = vp;
            }
            __syncthreads();
            piv = prow[k];
            const T inv = (T)1 / piv;
            for (int i = k + 1 + t; i < n; i += LG_THREADS) mcol[i] = W[(size_t)k * n + i] * inv;
            __syncthreads();
            const size_t m = (size_t)(n - k - 1);
            for (size_t e = t; e < m * m; e += LG_THREADS) {
                const int c = k + 1 + (int)(e / m), r = k + 1 + (int)(e % m);
                W[(size_t)c * n + r] -= mcol[r] * prow[c];
            }
            __syncthreads();
            negs ^= ((piv < 0) ? 1u : 0u) ^ ((p != k) ? 1u : 0u);
        }
        prod.fold(piv);
    }
    if (t == 0) {
        logabs[k_mat] = bad ? nan_of<T>() : prod.log_value();
        if (sign) sign[k_mat] = bad ? nan_of<T>() : ((negs & 1u) ? (T)-1 : (T)1);
        if (info) info[k_mat] = bad;
    }
}

// logml_k = 1/2 var_k - 1/2 logdet_k - n/2 log(2 pi), var_k = -d^T M^-1 d from the variance pipeline with a = d, e = 0
template <class T>
__global__ __launch_bounds__(256) void matinv_logml_combine(const T *var, const T *logdet, T *logml, int n, size_t batch)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < batch) logml[k] = (T)0.5 * var[k] - (T)0.5 * logdet[k] - (T)n * (T)0.91893853320467274178;
}

bool logdet_global_supports(int n) { return n >= 1 && n <= 1024; }

template <class T>
hipError_t launch_logdet_global(int n, bool spd, const T *As, size_t stride, const T *diag, T *logabs, T *sign, size_t batch, int *info,
                                hipStream_t stream)
{
    if (!logdet_global_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const size_t mat = (size_t)n * n;
    size_t chunk = blocked_workspace_cap() / (mat * sizeof(T));
    if (chunk < 1) chunk = 1;
    if (chunk > batch) chunk = batch;
    T *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), chunk * mat * sizeof(T), stream);
    if (e != hipSuccess) return e;
    for (size_t off = 0; off < batch && e == hipSuccess; off += chunk) {
        const size_t cnt = batch - off < chunk ? batch - off : chunk;
        if (spd)
            hipLaunchKernelGGL((matinv_logdet_global<T, true>), dim3((unsigned)cnt), dim3(LG_THREADS), 0, stream, As, stride, diag, ws, logabs,
                               sign, info, n, off);
        else
            hipLaunchKernelGGL((matinv_logdet_global<T, false>), dim3((unsigned)cnt), dim3(LG_THREADS), 0, stream, As, stride, diag, ws, logabs,
                               sign, info, n, off);
        e = hipGetLastError();
    }
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

template <class T>
hipError_t launch_logml_combine(int n, const T *var, const T *logdet, T *logml, size_t batch, hipStream_t stream)
{
    if (batch == 0) return hipSuccess;
    hipLaunchKernelGGL(matinv_logml_combine<T>, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, stream, var, logdet, logml, n, batch);
    return hipGetLastError();
}

#define INST(T)                                                                                                                  \
    template hipError_t launch_logdet_global<T>(int, bool, const T *, size_t, const T *, T *, T *, size_t, int *, hipStream_t); \
    template hipError_t launch_logml_combine<T>(int, const T *, const T *, T *, size_t, hipStream_t);
INST(double)
INST(float)
#undef INST

const char *name_logdet_global(bool f64, bool spd)
{
    if (f64) return spd ? "matinv_logdet_global<double, true>" : "matinv_logdet_global<double, false>";
    return spd ? "matinv_logdet_global<float, true>" : "matinv_logdet_global<float, false>";
}

}  // namespace matinv
