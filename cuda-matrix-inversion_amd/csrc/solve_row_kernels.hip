// solve_row_kernels.hip -- pivoting row solve X = A^-1 B, n <= 64, nrhs <= 16: the fallback of the fused bordered tile solve
// (solve_tile_impl.hpp) for the matrices its natural order rejects, and the solve of the PIVOT policy in that range.
//
// The ROW design of row_kernels.hip: lane i owns row i of A (register c = column c) and, here, its nrhs values of B. Step k:
// true partial pivoting over the rows not used yet, implicit pivoting (no data moves; the pivot row's entries reach the other
// lanes as scalar operands through v_readlane), Gauss-Jordan elimination of column k from every other row. Only the columns
// beyond k and the B values are updated: the pivot row is zero left of k, and columns up to k are never read again. The lane
// that pivoted at step s ends holding row s of X times its pivot; the permutation is folded into the store addresses.
// A step without a non-zero finite candidate makes info = k + 1 and X all NaN, exactly as in the ROW inverse (an exactly zero
// column stays exactly zero under the elimination).
#include "solve_tile_impl.hpp"
#include "wave_util.hpp"

namespace matinv {

// NR = 4 or 16 registers of B per lane (nrhs <= NR): updated unconditionally -- a run-time bound per right-hand side inside the
// unrolled steps nearly doubles the scalar spills hipcc already has in this design
template <class T, int NP, int NR>
__device__ __forceinline__ void solve_row_one(const T *A, const T *B, T *X, int *info_slot, int n, int nrhs)
{
    int i = threadIdx.x & 63;
    asm volatile("" : "+v"(i));  // see gj_row_one: keeps the unrolled steps' lane masks out of the caller's loop
    const bool row_in = i < n;
    T a[NP], b[NR];
#pragma unroll
    for (int c = 0; c < NP; ++c) a[c] = (row_in && c < n) ? A[c * n + i] : (T)0;
#pragma unroll
    for (int r = 0; r < NR; ++r) b[r] = (row_in && r < nrhs) ? B[r * n + i] : (T)0;

    bool used = !row_in;
    int pivstep = 0;  // step at which this lane's row was the pivot = its row of X
    T rowscale = (T)1;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (k < n) {  // wave-uniform
            const unsigned key = used ? 0u : magkey(a[k]);
            const unsigned mx = wave_max_u32(key);
            if (key_bad(T(0), mx) && bad == 0) bad = k + 1;  // no non-zero finite candidate: singular
            const unsigned long long vote = __ballot(!used && key == mx);
            const int p = vote ? (int)__builtin_ctzll(vote) : 0;
            const T inv = rcp_full(lane_value(a[k], p));
            const bool me = (i == p);
            const T negm = me ? (T)0 : -(a[k] * inv);
#pragma unroll
            for (int c = k + 1; c < NP; ++c) {
                a[c] = fmat(negm, lane_value(a[c], p), a[c]);
                if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // pin the readlanes in groups (SGPR pressure, see gj_row_one)
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) b[r] = fmat(negm, lane_value(b[r], p), b[r]);  // zeros beyond nrhs stay zero
            __builtin_amdgcn_sched_barrier(0);
            rowscale = me ? inv : rowscale;
            pivstep = me ? k : pivstep;
            used = used || me;
        }
    }
    const bool fail = bad != 0;
#pragma unroll
    for (int r = 0; r < NR; ++r)
        if (r < nrhs && row_in) X[r * n + (fail ? i : pivstep)] = fail ? nan_of<T>() : b[r] * rowscale;
    if (info_slot && i == 0) *info_slot = bad;
}

// work-list form: one wavefront per listed matrix, 4 wavefronts per workgroup
template <class T, int NP, int NR>
__global__ __launch_bounds__(256, 2) void matinv_solve_row_worklist(BatchRef<const T> Ain, BatchRef<const T> Bin, BatchRef<T> Xout, int *info,
                                                                    int n, int nrhs, const int *work_count, const int *work_list)
{
    const int count = *work_count;
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), stride = gridDim.x * 4;
    for (unsigned w = wave; w < (unsigned)count; w += stride) {
        const size_t k = (size_t)work_list[w];
        solve_row_one<T, NP, NR>(Ain.at_uniform(k), Bin.at_uniform(k), Xout.at_uniform(k), info ? info + k : nullptr, n, nrhs);
    }
}

// whole-batch form (MATINV_GJ_PIVOT in the fused range)
template <class T, int NP, int NR>
__global__ __launch_bounds__(256, 2) void matinv_solve_row(BatchRef<const T> Ain, BatchRef<const T> Bin, BatchRef<T> Xout, int *info, int n,
                                                           int nrhs, unsigned batch)
{
    const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), stride = gridDim.x * 4;
    for (unsigned k = wave; k < batch; k += stride)
        solve_row_one<T, NP, NR>(Ain.at_uniform(k), Bin.at_uniform(k), Xout.at_uniform(k), info ? info + k : nullptr, n, nrhs);
}

bool solve_row_supports(int n, int nrhs) { return n >= 1 && n <= 64 && nrhs >= 1 && nrhs <= SOLVE_MAX_NRHS; }
bool solve_tile_supports(int n, int nrhs) { return n > 16 && n <= 64 && nrhs >= 1 && nrhs <= SOLVE_MAX_NRHS; }

const char *name_solve_tile(bool f64, bool spd, int n)
{
    if (n <= 16 || n > 64) return "";
    const TileShape s = tile_shape(n);
    static thread_local char buf[48];
    snprintf(buf, sizeof buf, "matinv_solve_tile_%s<%d, %s, %s>", f64 ? "f64" : "f32", s.nt, s.full ? "true" : "false", spd ? "true" : "false");
    return buf;
}

template <class T>
hipError_t launch_solve_row_worklist(int n, int nrhs, BatchRef<const T> A, BatchRef<const T> B, BatchRef<T> X, const int *work_count,
                                     const int *work_list, int *info, hipStream_t stream)
{
    if (!solve_row_supports(n, nrhs)) return hipErrorInvalidValue;
    // the list length is only known on the device: a few rounds of resident blocks; blocks beyond the list exit at once
    const unsigned wl_rounds = tile_grid_rounds() < 8u ? tile_grid_rounds() : 8u;
#define ROW_LAUNCH(NP_, NR_)                                                                                                   \
    hipLaunchKernelGGL((matinv_solve_row_worklist<T, NP_, NR_>), dim3(512 * wl_rounds), dim3(256), 0, stream, A, B, X, info, n, nrhs, \
                       work_count, work_list)
    if (n <= 32 && nrhs <= 4) ROW_LAUNCH(32, 4);
    else if (n <= 32) ROW_LAUNCH(32, 16);
    else if (nrhs <= 4) ROW_LAUNCH(64, 4);
    else ROW_LAUNCH(64, 16);
#undef ROW_LAUNCH
    return hipGetLastError();
}

template <class T>
hipError_t launch_solve_row(int n, int nrhs, BatchRef<const T> A, BatchRef<const T> B, BatchRef<T> X, size_t batch, int *info,
                            hipStream_t stream)
{
    if (!solve_row_supports(n, nrhs)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const size_t blocks = (batch + 3) / 4;
    const unsigned cap = 256u * 2u * tile_grid_rounds();
    const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
#define ROW_LAUNCH(NP_, NR_) \
    hipLaunchKernelGGL((matinv_solve_row<T, NP_, NR_>), dim3(grid), dim3(256), 0, stream, A, B, X, info, n, nrhs, (unsigned)batch)
    if (n <= 32 && nrhs <= 4) ROW_LAUNCH(32, 4);
    else if (n <= 32) ROW_LAUNCH(32, 16);
    else if (nrhs <= 4) ROW_LAUNCH(64, 4);
    else ROW_LAUNCH(64, 16);
#undef ROW_LAUNCH
    return hipGetLastError();
}

#define INST(T)                                                                                                                    \
    template hipError_t launch_solve_row_worklist<T>(int, int, BatchRef<const T>, BatchRef<const T>, BatchRef<T>, const int *,     \
                                                     const int *, int *, hipStream_t);                                            \
    template hipError_t launch_solve_row<T>(int, int, BatchRef<const T>, BatchRef<const T>, BatchRef<T>, size_t, int *, hipStream_t);
INST(double)
INST(float)
#undef INST

const char *name_solve_row(bool f64, int n, int nrhs)
{
    static const char *const names[2][2][2] = {
        {{"matinv_solve_row<float, 32, 4>", "matinv_solve_row<float, 32, 16>"}, {"matinv_solve_row<float, 64, 4>", "matinv_solve_row<float, 64, 16>"}},
        {{"matinv_solve_row<double, 32, 4>", "matinv_solve_row<double, 32, 16>"},
         {"matinv_solve_row<double, 64, 4>", "matinv_solve_row<double, 64, 16>"}}};
    return names[f64 ? 1 : 0][n <= 32 ? 0 : 1][nrhs <= 4 ? 0 : 1];
}

}  // namespace matinv
