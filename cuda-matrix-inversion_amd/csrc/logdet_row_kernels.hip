// logdet_row_kernels.hip -- sign and log|det| of general matrices with partial pivoting, n <= 64: the ROW design of the pivoting
// row solve (solve_row_kernels.hip) with no right-hand side.
//
// Lane i owns row i of A (register c = column c). Step k: true partial pivoting over the rows not used yet, implicit (no data
// moves; the pivot row's entries reach the other lanes as scalar operands through v_readlane), elimination of column k from the
// rows that have not pivoted yet; only the columns beyond k are updated. det A = sign(permutation) * prod(pivots): the pivots'
// magnitudes are folded into a running mantissa / exponent pair (the determinant itself is never formed), their signs into a
// parity bit, and the permutation k -> (row that pivoted at step k) adds the parity of its inversion count at the end.
// A step without a non-zero finite candidate makes info = k + 1 and both outputs NaN, as in the ROW inverse.
#include "pivot_product.hpp"
#include "wave_util.hpp"

namespace matinv {

template <class T, int NP>
__device__ __forceinline__ void logdet_row_one(const T *A, T *logabs_slot, T *sign_slot, int *info_slot, int n)
{
    int i = threadIdx.x & 63;
    asm volatile("" : "+v"(i));  // see gj_row_one: keeps the unrolled steps' lane masks out of the caller's loop
    const bool row_in = i < n;
    T a[NP];
#pragma unroll
    for (int c = 0; c < NP; ++c) a[c] = (row_in && c < n) ? A[c * n + i] : (T)0;

    bool used = !row_in;
    int pivstep = -1;  // step at which this lane's row was the pivot
    PivotProduct<T> prod;
    unsigned negs = 0;  // parity of the number of negative pivots
    int bad = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (k < n) {  // wave-uniform
            const unsigned key = used ? 0u : magkey(a[k]);
            const unsigned mx = wave_max_u32(key);
            if (key_bad(T(0), mx) && bad == 0) bad = k + 1;  // no non-zero finite candidate: singular
            const unsigned long long vote = __ballot(!used && key == mx);
            const int p = vote ? (int)__builtin_ctzll(vote) : 0;
            const T piv = lane_value(a[k], p);
            const T inv = rcp_full(piv);
            const bool me = (i == p);
            const T negm = (me || used) ? (T)0 : -(a[k] * inv);  // rows that have pivoted are final: U's rows, never read again
#pragma unroll
            for (int c = k + 1; c < NP; ++c) {
                a[c] = fmat(negm, lane_value(a[c], p), a[c]);
                if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // pin the readlanes in groups (SGPR pressure, see gj_row_one)
            }
            __builtin_amdgcn_sched_barrier(0);
            prod.fold(piv);
            negs ^= (piv < 0) ? 1u : 0u;
            pivstep = me ? k : pivstep;
            used = used || me;
        }
    }
    // parity of the permutation: inversions (j < i with pivstep_j > pivstep_i) counted per lane, summed over the wave
    unsigned inv_count = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int sj = __builtin_amdgcn_readlane(pivstep, j);
        inv_count += (j < n && row_in && j < i && sj > pivstep) ? 1u : 0u;
    }
    const unsigned long long odd = __ballot((inv_count & 1u) != 0u);
    const unsigned parity = ((unsigned)__builtin_popcountll(odd) ^ negs) & 1u;
    const bool fail = bad != 0;
    if (i == 0) {
        *logabs_slot = fail ? nan_of<T>() : prod.log_value();
        if (sign_slot) *sign_slot = fail ? nan_of<T>() : (parity ? (T)-1 : (T)1);
        if (info_slot) *info_slot = bad;
    }
}

// one wavefront per matrix, 4 wavefronts per workgroup, grid-stride over the batch
template <class T, int NP>
__global__ __launch_bounds__(256, 2) void matinv_logdet_row(const T *As, size_t stride, T *logabs, T *sign, int *info, int n, unsigned batch)
{
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), step = gridDim.x * 4;
    for (unsigned k = wave; k < batch; k += step)
        logdet_row_one<T, NP>(As + (size_t)k * stride, logabs + k, sign ? sign + k : nullptr, info ? info + k : nullptr, n);
}

bool logdet_row_supports(int n) { return n >= 1 && n <= 64; }

template <class T>
hipError_t launch_logdet_row(int n, const T *As, size_t stride, T *logabs, T *sign, size_t batch, int *info, hipStream_t stream)
{
    if (!logdet_row_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const size_t blocks = (batch + 3) / 4;
    const unsigned cap = 256u * 2u * tile_grid_rounds();
    const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
    if (n <= 32)
        hipLaunchKernelGGL((matinv_logdet_row<T, 32>), dim3(grid), dim3(256), 0, stream, As, stride, logabs, sign, info, n, (unsigned)batch);
    else
        hipLaunchKernelGGL((matinv_logdet_row<T, 64>), dim3(grid), dim3(256), 0, stream, As, stride, logabs, sign, info, n, (unsigned)batch);
    return hipGetLastError();
}
template hipError_t launch_logdet_row<double>(int, const double *, size_t, double *, double *, size_t, int *, hipStream_t);
template hipError_t launch_logdet_row<float>(int, const float *, size_t, float *, float *, size_t, int *, hipStream_t);

const char *name_logdet_row(bool f64, int n)
{
    if (!logdet_row_supports(n)) return "";
    static const char *const names[2][2] = {{"matinv_logdet_row<float, 32>", "matinv_logdet_row<float, 64>"},
                                            {"matinv_logdet_row<double, 32>", "matinv_logdet_row<double, 64>"}};
    return names[f64 ? 1 : 0][n <= 32 ? 0 : 1];
}

}  // namespace matinv
