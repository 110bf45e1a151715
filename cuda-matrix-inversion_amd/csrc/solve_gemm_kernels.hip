// solve_gemm_kernels.hip -- the product step of the composed solve (n < 17, 64 < n <= 1024, nrhs > 16, forced families):
// X_k = Ainv_k B_k for a chunk of inverses that matinv_inverse_batched_ex has just written to a scratch block.
//
// A workgroup takes a group of matrices (256 / n of them for n <= 256, else one) and one block of SOLVE_GEMM_JW columns of B:
// it stages those columns of B in LDS, then each thread forms whole rows of the X block (consecutive threads read consecutive
// rows of a column of Ainv: coalesced). Every column block of X is read and written by ONE workgroup, and all of its reads come
// before the barrier that precedes its writes, so X may be exactly B. Plain FMAs over every term: a NaN anywhere in Ainv_k
// reaches every element of X_k.
#include "solve_tile_impl.hpp"

namespace matinv {

constexpr int SOLVE_GEMM_JW = 4;
constexpr int SOLVE_GEMM_THREADS = 256;

template <class T>
__global__ __launch_bounds__(SOLVE_GEMM_THREADS) void matinv_solve_gemm(const T *__restrict__ Ainv, BatchRef<const T> B, BatchRef<T> X, int n,
                                                                        int nrhs, unsigned count, unsigned mpb, unsigned ncb)
{
    constexpr int JW = SOLVE_GEMM_JW;
    __shared__ T bs[1024 * JW];  // mpb * n * JW <= max(256, n) * JW elements
    const unsigned groups = (count + mpb - 1) / mpb;
    const unsigned tid = threadIdx.x;
    const unsigned per = (unsigned)n * JW;
    for (size_t blk = blockIdx.x; blk < (size_t)groups * ncb; blk += gridDim.x) {
        const unsigned g = (unsigned)(blk / ncb), cb = (unsigned)(blk % ncb);
        const int j0 = (int)cb * JW;
        const int jw = nrhs - j0 < JW ? nrhs - j0 : JW;
        __syncthreads();  // the previous block's readers of bs are done
        for (unsigned e = tid; e < mpb * per; e += SOLVE_GEMM_THREADS) {
            const unsigned lm = e / per, rem = e % per, j = rem / (unsigned)n, m = rem % (unsigned)n;
            const size_t k = (size_t)g * mpb + lm;
            bs[e] = (k < count && (int)j < jw) ? B.at(k)[(size_t)(j0 + (int)j) * n + m] : (T)0;
        }
        __syncthreads();
        for (unsigned e = tid; e < mpb * (unsigned)n; e += SOLVE_GEMM_THREADS) {
            const unsigned lm = e / (unsigned)n, row = e % (unsigned)n;
            const size_t k = (size_t)g * mpb + lm;
            if (k >= count) continue;
            const T *Ai = Ainv + k * (size_t)n * n + row;
            const T *bl = bs + lm * per;
            T acc[JW];
#pragma unroll
            for (int j = 0; j < JW; ++j) acc[j] = (T)0;
            for (int m = 0; m < n; ++m) {
                const T a = Ai[(size_t)m * n];
#pragma unroll
                for (int j = 0; j < JW; ++j) acc[j] = fma_t(a, bl[j * n + m], acc[j]);
            }
            T *Xk = X.at(k);
#pragma unroll
            for (int j = 0; j < JW; ++j)
                if (j < jw) Xk[(size_t)(j0 + j) * n + row] = acc[j];
        }
    }
}

template <class T>
hipError_t launch_solve_gemm(int n, int nrhs, const T *Ainv, BatchRef<const T> B, BatchRef<T> X, size_t count, hipStream_t stream)
{
    if (n < 1 || n > 1024 || nrhs < 1 || count == 0 || count > 0xffffffffu) return hipErrorInvalidValue;
    const unsigned mpb = n <= SOLVE_GEMM_THREADS ? (unsigned)(SOLVE_GEMM_THREADS / n) : 1u;
    const unsigned ncb = (unsigned)((nrhs + SOLVE_GEMM_JW - 1) / SOLVE_GEMM_JW);
    const size_t blocks = (count + mpb - 1) / mpb * ncb;
    const size_t cap = 256u * 32u;  // resident blocks over the 256 CUs, several rounds; the kernel strides beyond
    const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
    hipLaunchKernelGGL((matinv_solve_gemm<T>), dim3(grid), dim3(SOLVE_GEMM_THREADS), 0, stream, Ainv, B, X, n, nrhs, (unsigned)count, mpb,
                       ncb);
    return hipGetLastError();
}
template hipError_t launch_solve_gemm<double>(int, int, const double *, BatchRef<const double>, BatchRef<double>, size_t, hipStream_t);
template hipError_t launch_solve_gemm<float>(int, int, const float *, BatchRef<const float>, BatchRef<float>, size_t, hipStream_t);

const char *name_solve_gemm(bool f64) { return f64 ? "matinv_solve_gemm<double>" : "matinv_solve_gemm<float>"; }

}  // namespace matinv
