// common.hpp -- shared declarations of the HIP translation units of libmatinv_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/matinv.h"

namespace matinv {

// (batch << 32) | rejected of a natural-order launch, stored by the work-list kernel behind it into pinned host memory
typedef unsigned long long hint_t;

// thread-local error message behind matinv_last_error(); returns `code` (abi.hip)
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int fail_hip(hipError_t e, const char *what);

// Device scratch of the launchers: blocks cached per (device, stream), reused on their own stream only (scratch.hip)
hipError_t scratch_alloc(void **p, size_t bytes, hipStream_t stream);
hipError_t scratch_free(void *p, hipStream_t stream);
void scratch_retire_stream(hipStream_t stream);  // after synchronising a stream that is about to be destroyed
void blocked_gp_release_graphs();                // the cached launch-chain graphs of blocked_gp_kernels.hip (they hold scratch pointers)
void scratch_release_device();                   // after hipDeviceSynchronize: hipFree everything not in use

// The work-list block of a launcher: `count` ints of scratch, the first `zeroed` of them cleared, body(ws) enqueued behind that
// and the block freed in stream order. Returns the first error; body runs only when the allocation and the clearing succeeded.
template <class Body>
hipError_t with_scratch_ints(size_t count, size_t zeroed, hipStream_t stream, Body &&body)
{
    int *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), count * sizeof(int), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(ws, 0, zeroed * sizeof(int), stream);
    if (e == hipSuccess) e = body(ws);
    const hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

// Compile-time tile count of a launch: f(std::integral_constant<int, NT>{}) for the run-time nt in [LO, HI]; any other nt takes HI
// (the `default:` of the switch this replaces).
template <int LO, int HI, class F>
decltype(auto) with_nt(int nt, F &&f)
{
    if constexpr (LO == HI) {
        return f(std::integral_constant<int, HI>{});
    } else {
        if (nt == LO) return f(std::integral_constant<int, LO>{});
        return with_nt<LO + 1, HI>(nt, f);
    }
}
// What a tile kernel is instantiated on: NT tiles of 16 per dimension, and FULL = n == 16 * NT (no partial tile: constant offsets,
// no bounds checks). The launchers and the kernel_name strings both derive it from these functions.
struct TileShape {
    int nt;
    bool full;
};
constexpr TileShape tile_shape(int n) { return {(n + 15) / 16, n % 16 == 0}; }
// f(NT, std::bool_constant<FULL>{}) as with_nt; FULL only for the nt the shape names
template <int LO, int HI, class F>
decltype(auto) with_tile(TileShape s, F &&f)
{
    return with_nt<LO, HI>(s.nt, [&](auto nt) -> decltype(auto) {
        if (s.full && s.nt == nt) return f(nt, std::true_type{});
        return f(nt, std::false_type{});
    });
}

// Where matrix k of a batch lives: either base + k*stride, or table[k] (the reference's
// "array of device pointers" form, /root/reference/src/helper.cu:103-118).
template <class T>
struct BatchRef {
    T *base;
    size_t stride;
    T *const *table;  // device-resident pointer table, or nullptr
    __device__ __forceinline__ T *at(size_t k) const { return table ? table[k] : base + k * stride; }
    // Same for a wave-uniform k: the table entry is moved to SGPRs at once, so that on the (usual) strided path the result
    // never lives in a VGPR that a pending vector load targets -- otherwise hipcc guards the merge with s_waitcnt vmcnt(0)
    // on BOTH paths, draining every outstanding load / store / LDS-DMA of the wave at each matrix boundary.
    __device__ __forceinline__ T *at_uniform(size_t k) const
    {
        if (table) {
            const unsigned long long p = reinterpret_cast<unsigned long long>(table[k]);
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)p), hi = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32));
            // rebuilt from integers: say explicitly that it is a global-memory pointer, or every access through it
            // (and, after the merge, through the strided path too) degrades to flat_load / flat_store
            typedef __attribute__((address_space(1))) T *global_ptr;
            return (T *)(global_ptr)(((unsigned long long)hi << 32) | lo);
        }
        return base + k * stride;
    }
};

template <class T>
__device__ __forceinline__ T max_finite();
template <>
__device__ __forceinline__ double max_finite<double>() { return 1.7976931348623157e308; }
template <>
__device__ __forceinline__ float max_finite<float>() { return 3.402823466e38f; }
template <class T>
__device__ __forceinline__ T nan_of();
template <>
__device__ __forceinline__ double nan_of<double>() { return __longlong_as_double(0x7ff8000000000000LL); }
template <>
__device__ __forceinline__ float nan_of<float>() { return __int_as_float(0x7fc00000); }

// Host-side launchers; each returns hipSuccess / an error, or hipErrorInvalidValue when the
// family cannot serve (n, dtype). All are asynchronous on `stream`.
template <class T>
hipError_t launch_gj_lds(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
// pivoted LDS kernel over a device-side work list (count + indices), used as the fallback of the fast families
template <class T>
hipError_t launch_gj_lds_worklist(int n, BatchRef<const T> A, BatchRef<T> X, const int *work_count, const int *work_list,
                                  int *info, hipStream_t stream);
template <class T>
hipError_t launch_chol_lds_worklist(int n, BatchRef<const T> A, BatchRef<T> X, const int *work_count,
                                    const int *work_list, int *info, hipStream_t stream);
// phases: bit 0 factor, bit 1 triangular inverse, bit 2 L^-T L^-1 (7 = full inverse)
template <class T>
hipError_t launch_chol_lds(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream,
                           int phases);
template <class T>
bool lds_family_supports(int n);

template <class T>
hipError_t launch_gj_rowlane(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
// the same kernel as the Cholesky entry point for n <= 16 (lower triangle only, natural positive pivots)
template <class T>
hipError_t launch_spd_rowlane(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
const char *name_spd_rowlane(bool f64, int n);
// fused GP scalars on the same kernel, n <= 16
template <class T>
hipError_t launch_gp_rowlane(int n, const T *As, const T *Bs, const T *Cs, const T *Ds, const T *Es, T *out, size_t batch,
                             int *info, hipStream_t stream);
const char *name_gp_rowlane(bool f64, int n);
template <class T>
bool rowlane_family_supports(int n);
// natural-order pass of the Gauss-Jordan entry point for 16 < n <= 25: the ROWLANE design with two rows per lane
// (rowlane2_kernels.hip); rejected matrices go to work_list like those of the natural-order tile kernels
bool rowlane2_supports(int n);  // 16 < n <= 25: where it replaces the MFMA tile kernels, natural-order pass and pipeline alike
template <class T>
hipError_t enqueue_gj_rowlane2(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream, int *work_count,
                               int *work_list);
const char *name_gj_rowlane2(bool f64, int n);
// r03: the same kernel as the fused mean / variance (positive pivots verified, a^T M^-1 d folded out of the registers)
template <class T>
hipError_t launch_gp_rowlane2(int n, const T *As, const T *Bs, const T *Cs, const T *Ds, const T *Es, T *out, size_t batch, int *info,
                              hipStream_t stream);
const char *name_gp_rowlane2(bool f64, int n);
template <class T>
hipError_t enqueue_gp_rowlane2(int n, const T *As, const T *Bs, const T *Cs, const T *Ds, const T *Es, T *out, size_t batch, int *info,
                               hipStream_t stream, int *work_count, int *work_list);

// blocked multi-launch Cholesky for the fused GP scalars at large n (blocked_gp_kernels.hip)
template <class T>
hipError_t launch_gp_blocked(int n, const T *As, const T *Bs, const T *Cs, const T *Ds, const T *Es, T *out, size_t batch,
                             int *info, hipStream_t stream);

// blocked SPD inverse for large n on the same panel / update kernels (identity border + symmetric rank-n product)
bool blocked_inverse_supports(int n);
template <class T>
hipError_t launch_chol_blocked(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);

// rounds of resident workgroups in the grids of the MFMA-tile kernels (each workgroup strides over the batch);
// MATINV_TILE_GRID_MULT overrides the default for A/B measurements (tile_kernels.hip)
unsigned tile_grid_rounds();
// grid of a tile-kernel launch: one workgroup per matrix, at most `rounds` rounds of per_cu resident workgroups on each of 256 CUs
inline unsigned tile_grid(size_t batch, unsigned per_cu, unsigned rounds = tile_grid_rounds())
{
    const unsigned cap = 256u * per_cu * rounds;
    return (unsigned)(batch < cap ? batch : cap);
}

// blocked Gauss-Jordan with partial pivoting for large general matrices (blocked_gj_kernels.hip)
bool blocked_gj_supports(int n);
int blocked_gj_two_level_min();
size_t blocked_workspace_cap();  // bytes; MATINV_BLOCKED_WS_MB overrides the 16 GiB default
template <class T>
hipError_t launch_gj_blocked(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);

// GLOBAL family (global_kernels.hip): any n <= 1024, working copy in global memory
template <class T>
bool global_family_supports(int n);
template <class T>
hipError_t launch_gj_global(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
template <class T>
hipError_t launch_chol_global(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
const char *name_gj_global(bool f64);
const char *name_chol_global(bool f64);

// ROW family (row_kernels.hip): true partial pivoting, one matrix per wavefront, n <= 64
template <class T>
bool row_family_supports(int n);
template <class T>
hipError_t launch_gj_row(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
template <class T>
hipError_t launch_gj_row_worklist(int n, BatchRef<const T> A, BatchRef<T> X, const int *work_count, const int *work_list,
                                  int *info, hipStream_t stream);
const char *name_gj_row(bool f64, int n);

template <class T>
hipError_t launch_gj_tile(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
template <class T>
bool tile_family_supports(int n);
// four-wave variant of the tile family, 64 < n <= 128, f64 and f32 (tile4_kernels.hip); the spd entry is the same
// kernel with lower-triangle loads and positivity-checked pivots (the Cholesky contract)
bool tile4_supports(int n);
bool tile4_wide_supports(bool f64, int n);  // SPD sweep and fused pipeline only: 128 < n <= 192 (f64) / 256 (f32)
template <class T>
hipError_t launch_gj_tile4(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
template <class T>
hipError_t launch_spd_tile4(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
const char *name_tile4(bool f64, bool spd, int n);
// SPD (symmetric blocked sweep) on the tile layout, f64, n <= 64
template <class T>
hipError_t launch_spd_tile(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
template <class T>
bool spd_tile_supports(int n);
const char *name_spd_tile(bool f64, int n);

// TILEP family (tilep_kernels.hip): the MFMA tile Gauss-Jordan with true partial pivoting inside the kernel, n <= 64
bool tilep_supports(int n);
template <class T>
hipError_t launch_gj_tilep(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
// work-list form: inverts in_list[0 .. *in_count) (device memory); singular ones go on to the ROW kernel through
// (bad_count, bad_list), zeroed by the caller; hint_out (pinned host memory, may be null) receives the list length
template <class T>
hipError_t launch_gj_tilep_worklist(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, const int *in_count, const int *in_list,
                                    int *bad_count, int *bad_list, int *info, hipStream_t stream, hint_t *hint_out, bool expect_many = false,
                                    const int *aux_count = nullptr, hint_t *aux_out = nullptr);
const char *name_gj_tilep(bool f64, int n);
// four wavefronts per matrix, 64 < n <= 128 (tilep4_kernels.hip)
template <class T>
hipError_t launch_gj_tilep4(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
template <class T>
hipError_t launch_gj_tilep4_worklist(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, const int *in_count, const int *in_list,
                                     int *bad_count, int *bad_list, int *info, hipStream_t stream, hint_t *hint_out, bool expect_many = false);
const char *name_gj_tilep4(bool f64, int n);
// r04: fixed pivot rows, searched pivot columns -- no run-time register index (tileq_kernels.hip): one wavefront per tile column,
// general 128 < n <= 192 (f64) / 256 (f32). in_count / in_list: work-list form (nullptr: the whole batch); bad_count / bad_list: unused
// at these sizes (the kernel finishes a singular matrix itself), kept for the n <= 128 instantiations of tools/tileq_stamps.hip
template <class T>
hipError_t launch_gj_tileq(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream, const int *in_count,
                           const int *in_list, hint_t *hint_out, int *bad_count, int *bad_list);
const char *name_gj_tileq(bool f64, int n);
// general 128 < n <= 192 (f64) / 256 (f32): TILEQ (tileq_kernels.hip)
bool tileq_supports(bool f64, int n);
// Adaptive choice between the natural-order (verified) tile kernel and the pivoting one (tile_kernels.hip): see gj_tile_policy
struct TileStats {
    unsigned long long natural_launches, pivot_launches, last_rejected, last_batch;
};
TileStats tile_stats();
bool tile_policy_use_pivot(bool f64, int nt);
// 64 x 64 fp64: launches that ran the symmetric-only kernel in front / the two-arm kernel alone, and what the last completed front
// launch found (tile_kernels.hip)
struct SymFrontStats {
    unsigned long long front_launches, direct_launches, last_not_symmetric, last_batch;
};
SymFrontStats sym_front_stats();
hint_t *tile_policy_record(bool f64, int nt, size_t batch);
int gj_policy();                // a matinv_gj_policy (include/matinv.h)
int set_gj_policy(int policy);  // returns the previous one

const char *name_gj_rowlane(bool f64, int n);
const char *name_gj_tile(bool f64, int n);
// the LDS pipeline kernel over a device-side work list: finishes the items a tile or rowlane2 pipeline kernel rejected.
// Ds == nullptr selects the variance form (needs Es); otherwise the mean form.
template <class T>
hipError_t launch_gp_lds_worklist(int n, const T *As, const T *Bs, const T *Cs, const T *Ds, const T *Es, T *out,
                                  const int *work_count, const int *work_list, int *info, hipStream_t stream);
// fused GP scalars on the MFMA tile layout, one wavefront per item: f64 16 < n <= 80, f32 16 < n <= 96 (gp_tile_kernels.hip)
bool gp_tile_supports(bool f64, int n);
template <class T>
hipError_t launch_gp_tile(int n, const T *As, const T *Bs, const T *Cs, const T *Ds, const T *Es, T *out, size_t batch,
                          int *info, hipStream_t stream);
const char *name_gp_tile(bool f64, int n);
// fused GP scalars on the SPD sweep of the Cholesky entry point (inverse in registers, folded, never stored): the sizes the
// bordered form above no longer holds in one wavefront -- f64 80 < n <= 96, f32 96 < n <= 112 (tile_impl.hpp)
// test hook (scratch.hip): MATINV_DEBUG_REJECTS=1 -> launchers with a work list add its final count to a running total
hipError_t debug_note_rejects(const int *work_count, hipStream_t stream);
long long debug_rejects(bool reset);
bool gp_spd_tile_supports(bool f64, int n);
const char *name_gp_spd_tile(bool f64, int n);
int spd_onewave_max(bool f64);  // largest n of the one-wavefront symmetric sweep (fp64 112, fp32 160)
// fp32 9 x 9 / 10 x 10 lower tiles on one wavefront (spd_wide_f32_kernels.hip, gp_spd_wide_f32_kernels.hip): the kernel launch only, ws = [count, list...]
hipError_t enqueue_spd_tile_wide_f32(int n, BatchRef<const float> A, BatchRef<float> X, unsigned grid, unsigned b, int *info, int *ws,
                                     hipStream_t stream);
// fp64 7 x 7 lower tiles on one wavefront (spd_wide_f64_kernels.hip, compiled with VGPR-form MFMAs)
hipError_t enqueue_spd_tile_wide_f64(int n, BatchRef<const double> A, BatchRef<double> X, unsigned grid, unsigned b, int *info, int *ws,
                                     hipStream_t stream);
hipError_t enqueue_gp_spd_tile_wide_f64(int n, const double *As, const double *Bs, const double *Cs, const double *Ds, const double *Es,
                                        double *out, unsigned grid, unsigned b, int *info, int *ws, hipStream_t stream);
hipError_t enqueue_gp_spd_tile_wide_f32(int n, const float *As, const float *Bs, const float *Cs, const float *Ds, const float *Es, float *out,
                                        unsigned grid, unsigned b, int *info, int *ws, hipStream_t stream);
// two (176 < n <= 192: three) wavefronts per matrix, lower tiles only, fp64 112 < n <= 192 (r04: beyond 128 too): Cholesky entry point and fused pipeline (spd_tile2_kernels.hip);
bool spd_tile2_supports(bool f64, int n);
hipError_t launch_spd_tile2(int n, BatchRef<const double> A, BatchRef<double> X, size_t batch, int *info, hipStream_t stream);
hipError_t launch_gp_spd_tile2(int n, const double *As, const double *Bs, const double *Cs, const double *Ds, const double *Es, double *out,
                               size_t batch, int *info, hipStream_t stream);
const char *name_spd_tile2(bool gp, int n);
template <class T>
hipError_t launch_gp_spd_tile(int n, const T *As, const T *Bs, const T *Cs, const T *Ds, const T *Es, T *out, size_t batch,
                              int *info, hipStream_t stream);
// Batched linear solve X = A^-1 B (matinv_solve_batched). B, X: n x nrhs column-major per matrix.
// (a) fused bordered MFMA tile kernel, 16 < n <= 64, nrhs <= 16, both algorithms (solve_tile_kernels.hip, solve_tile_f32_kernels.hip);
//     Gauss-Jordan rejects go to (b) through a device work list in the same stream
bool solve_tile_supports(int n, int nrhs);
template <class T>
hipError_t launch_solve_tile(int algo, int n, int nrhs, BatchRef<const T> A, BatchRef<const T> B, BatchRef<T> X, size_t batch, int *info,
                             hipStream_t stream);
const char *name_solve_tile(bool f64, bool spd, int n);
// (b) pivoting row solve, n <= 64, nrhs <= 16 (solve_row_kernels.hip): whole batch, or the matrices of a work list
bool solve_row_supports(int n, int nrhs);
template <class T>
hipError_t launch_solve_row(int n, int nrhs, BatchRef<const T> A, BatchRef<const T> B, BatchRef<T> X, size_t batch, int *info,
                            hipStream_t stream);
template <class T>
hipError_t launch_solve_row_worklist(int n, int nrhs, BatchRef<const T> A, BatchRef<const T> B, BatchRef<T> X, const int *work_count,
                                     const int *work_list, int *info, hipStream_t stream);
const char *name_solve_row(bool f64, int n, int nrhs);
// (c) product step of the composed path: X_k = Ainv_k B_k, Ainv packed (stride n^2), `count` matrices (solve_gemm_kernels.hip)
template <class T>
hipError_t launch_solve_gemm(int n, int nrhs, const T *Ainv, BatchRef<const T> B, BatchRef<T> X, size_t count, hipStream_t stream);
const char *name_solve_gemm(bool f64);

// Batched log-determinant and GP log marginal likelihood (matinv_logdet_batched, matinv_logml_batched).
// (a) symmetric MFMA tile sweep, one wavefront per matrix, n <= 96 (logdet_tile_kernels.hip, logdet_tile_f32_kernels.hip). border == false:
//     out0 = log det A (SPD, lower triangle), out1 = sign (optional); border == true: out0 = logml of B + diag Cs (Cs optional) and Ds
bool logdet_tile_supports(int n);
template <class T>
hipError_t launch_logdet_tile(int n, bool border, const T *As, size_t stride, const T *Cs, const T *Ds, T *out0, T *out1, size_t batch,
                              int *info, hipStream_t stream);
const char *name_logdet_tile(bool f64, bool border, int n);
// (b) pivoting row kernel for general matrices, n <= 64 (logdet_row_kernels.hip)
bool logdet_row_supports(int n);
template <class T>
hipError_t launch_logdet_row(int n, const T *As, size_t stride, T *logabs, T *sign, size_t batch, int *info, hipStream_t stream);
const char *name_logdet_row(bool f64, int n);
// (c) the functional path, n <= 1024 (logdet_global_kernels.hip): LU with partial pivoting, or (spd) L D L^T of A + diag(diag)
bool logdet_global_supports(int n);
template <class T>
hipError_t launch_logdet_global(int n, bool spd, const T *As, size_t stride, const T *diag, T *logabs, T *sign, size_t batch, int *info,
                                hipStream_t stream);
const char *name_logdet_global(bool f64, bool spd);
template <class T>
hipError_t launch_logml_combine(int n, const T *var, const T *logdet, T *logml, size_t batch, hipStream_t stream);

// Batched leave-one-out cross-validation of a GP (matinv_loo_batched): mean, var: batch * n, logpl: batch, each optional.
// (a) the LOO form of the one-wavefront SPD sweep, n <= 96 (loo_tile_kernels.hip, loo_tile_f32_kernels.hip)
bool loo_tile_supports(int n);
template <class T>
hipError_t launch_loo_tile(int n, const T *Bs, const T *Cs, const T *Ds, T *mean, T *var, T *logpl, size_t batch, int *info,
                           hipStream_t stream);
const char *name_loo_tile(bool f64, int n);
// (b) the LOO form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_loo_global(int n, const T *Bs, const T *Cs, const T *Ds, T *mean, T *var, T *logpl, size_t batch, int *info,
                             hipStream_t stream);
const char *name_loo_global(bool f64);

// Gradients of the batched GP log marginal likelihood (matinv_logml_grad_batched): grad: batch * nparam, gradc, alpha: batch * n, each
// optional; dMs: batch * nparam symmetric n x n matrices (lower triangle read), needed with grad only.
// (a) the gradient form of the one-wavefront SPD sweep, n <= 96 (logml_grad_tile_kernels.hip, logml_grad_tile_f32_kernels.hip)
bool logml_grad_tile_supports(int n);
template <class T>
hipError_t launch_logml_grad_tile(int n, int nparam, const T *Bs, const T *Cs, const T *Ds, const T *dMs, T *grad, T *gradc, T *alpha,
                                  size_t batch, int *info, hipStream_t stream);
const char *name_logml_grad_tile(bool f64, int n);
// (b) the gradient form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_logml_grad_global(int n, int nparam, const T *Bs, const T *Cs, const T *Ds, const T *dMs, T *grad, T *gradc, T *alpha,
                                    size_t batch, int *info, hipStream_t stream);
const char *name_logml_grad_global(bool f64);

// Batched GP prediction at nquery query points per matrix (matinv_predict_batched): As: batch * nquery vectors of n elements, Es (optional):
// batch * nquery prior variances; mean, var: batch * nquery, each optional. Ds is read with mean only.
// (a) the prediction form of the one-wavefront SPD sweep, n <= 96 (predict_tile_kernels.hip, predict_tile_f32_kernels.hip)
bool predict_tile_supports(int n);
template <class T>
hipError_t launch_predict_tile(int n, int nquery, const T *Bs, const T *Cs, const T *Ds, const T *As, const T *Es, T *mean, T *var,
                               size_t batch, int *info, hipStream_t stream);
const char *name_predict_tile(bool f64, int n);
// (b) the prediction form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_predict_global(int n, int nquery, const T *Bs, const T *Cs, const T *Ds, const T *As, const T *Es, T *mean, T *var,
                                 size_t batch, int *info, hipStream_t stream);
const char *name_predict_global(bool f64);

// Batched joint predictive covariance between nquery query points per matrix (matinv_predict_cov_batched): As as above; Es (optional):
// batch * nquery^2, column-major per matrix, lower triangle read; mean: batch * nquery, cov: batch * nquery^2 (both triangles written),
// each optional. Ds is read with mean only, Es with cov only.
// (a) the covariance form of the one-wavefront SPD sweep, n <= 96 (predict_cov_tile_kernels.hip, predict_cov_tile_f32_kernels.hip)
bool predict_cov_tile_supports(int n);
template <class T>
hipError_t launch_predict_cov_tile(int n, int nquery, const T *Bs, const T *Cs, const T *Ds, const T *As, const T *Es, T *mean, T *cov,
                                   size_t batch, int *info, hipStream_t stream);
const char *name_predict_cov_tile(bool f64, int n);
// (b) the covariance form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_predict_cov_global(int n, int nquery, const T *Bs, const T *Cs, const T *Ds, const T *As, const T *Es, T *mean, T *cov,
                                     size_t batch, int *info, hipStream_t stream);
const char *name_predict_cov_global(bool f64);

// Gradients of the batched GP leave-one-out log pseudo-likelihood (matinv_loo_grad_batched): grad: batch * nparam, gradc: batch * n,
// logpl: batch, each optional; dMs: batch * nparam symmetric n x n matrices (lower triangle read), needed with grad only.
// (a) the LOO-gradient form of the one-wavefront SPD sweep, n <= 96 (loo_grad_tile_kernels.hip, loo_grad_tile_f32_kernels.hip)
bool loo_grad_tile_supports(int n);
template <class T>
hipError_t launch_loo_grad_tile(int n, int nparam, const T *Bs, const T *Cs, const T *Ds, const T *dMs, T *grad, T *gradc, T *logpl,
                                size_t batch, int *info, hipStream_t stream);
const char *name_loo_grad_tile(bool f64, int n);
// (b) the LOO-gradient form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_loo_grad_global(int n, int nparam, const T *Bs, const T *Cs, const T *Ds, const T *dMs, T *grad, T *gradc, T *logpl,
                                  size_t batch, int *info, hipStream_t stream);
const char *name_loo_grad_global(bool f64);

// Batched Cholesky factor and coloured samples Y = m + chol(C) Z (matinv_colour_batched): Cs: matrix k at k * stride, n x n column-major,
// lower triangle read; Ms (optional): batch * n; Zs: batch * n * nsample, sample s of matrix k a run of n elements; Ys: as Zs; Ls:
// batch * n^2, column-major, strict upper triangle written as zeros. Ys and Ls are each optional; Zs is read with Ys only.
// info_base != 0 (matinv_sample_batched): info holds the codes of an earlier stage; a non-zero one stands, a failure here is info_base + column.
// (a) the colour form of the one-wavefront SPD sweep, n <= 96 (colour_tile_kernels.hip, colour_tile_f32_kernels.hip)
bool colour_tile_supports(int n);
template <class T>
hipError_t launch_colour_tile(int n, int nsample, const T *Cs, size_t stride, const T *Ms, const T *Zs, T *Ys, T *Ls, size_t batch, int *info,
                              int info_base, hipStream_t stream);
const char *name_colour_tile(bool f64, int n);
// (b) the colour form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_colour_global(int n, int nsample, const T *Cs, size_t stride, const T *Ms, const T *Zs, T *Ys, T *Ls, size_t batch,
                                int *info, int info_base, hipStream_t stream);
const char *name_colour_global(bool f64);

// Batched whitening, Mahalanobis distances and Gaussian log-density (matinv_whiten_batched): Cs, Ms as above; Xs: batch * n * npoint, point
// s of matrix k a run of n elements; Ws: as Xs, L^-1 (x - m); Mh: batch * npoint, ||w||^2; Ld: batch, log det C; Lp: batch * npoint,
// -1/2 (maha + logdet + n log 2 pi). Every output is optional; Xs is read only with Ws, Mh or Lp.
// (a) the whiten form of the one-wavefront SPD sweep, n <= 96 (whiten_tile_kernels.hip, whiten_tile_f32_kernels.hip)
bool whiten_tile_supports(int n);
template <class T>
hipError_t launch_whiten_tile(int n, int npoint, const T *Cs, size_t stride, const T *Ms, const T *Xs, T *Ws, T *Mh, T *Ld, T *Lp,
                              size_t batch, int *info, hipStream_t stream);
const char *name_whiten_tile(bool f64, int n);
// (b) the whiten form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_whiten_global(int n, int npoint, const T *Cs, size_t stride, const T *Ms, const T *Xs, T *Ws, T *Mh, T *Ld, T *Lp,
                                size_t batch, int *info, hipStream_t stream);
const char *name_whiten_global(bool f64);

// Multi-output GP solves (matinv_multi_target_batched): Bs, Cs as for the prediction; Ys: batch * ntarget * n, target t of matrix k a run
// of n elements at (k ntarget + t) n; As: batch * nquery * n as for the prediction; Al: as Ys, M^-1 y_t; Qd: batch * ntarget, y_t^T M^-1 y_t;
// Ld: batch, log det M; Lm: batch * ntarget, -1/2 (quad + logdet + n log 2 pi); Mn: batch * ntarget * nquery, element (k, t, j) at
// (k ntarget + t) nquery + j. Every output is optional; Ys is read with every output but Ld, As with Mn only.
// (a) the multi-target form of the one-wavefront SPD sweep, n <= 96 (multi_target_tile_kernels.hip, multi_target_tile_f32_kernels.hip)
bool multi_target_tile_supports(int n);
template <class T>
hipError_t launch_multi_target_tile(int n, int ntarget, int nquery, const T *Bs, const T *Cs, const T *Ys, const T *As, T *Al, T *Qd, T *Ld,
                                    T *Lm, T *Mn, size_t batch, int *info, hipStream_t stream);
const char *name_multi_target_tile(bool f64, int n);
// (b) the multi-target form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_multi_target_global(int n, int ntarget, int nquery, const T *Bs, const T *Cs, const T *Ys, const T *As, T *Al, T *Qd,
                                      T *Ld, T *Lm, T *Mn, size_t batch, int *info, hipStream_t stream);
const char *name_multi_target_global(bool f64);

// Gradients of the multi-output log marginal likelihood (matinv_multi_target_grad_batched): Bs, Cs, Ys as above, dMs as for
// matinv_logml_grad_batched; grad: batch * nparam, gradc: batch * n, Lm: batch * ntarget, Al: as Ys. Every output is optional; dMs is read
// with grad only.
// (a) the gradient form of the multi-target tile kernels, n <= 96 (multi_target_grad_tile_kernels.hip, multi_target_grad_tile_f32_kernels.hip)
bool multi_target_grad_tile_supports(int n);
template <class T>
hipError_t launch_multi_target_grad_tile(int n, int ntarget, int nparam, const T *Bs, const T *Cs, const T *Ys, const T *dMs, T *grad,
                                         T *gradc, T *Lm, T *Al, size_t batch, int *info, hipStream_t stream);
const char *name_multi_target_grad_tile(bool f64, int n);
// (b) the multi-target gradient form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_multi_target_grad_global(int n, int ntarget, int nparam, const T *Bs, const T *Cs, const T *Ys, const T *dMs, T *grad,
                                           T *gradc, T *Lm, T *Al, size_t batch, int *info, hipStream_t stream);
const char *name_multi_target_grad_global(bool f64);

// GP regression with a linear trend (matinv_trend_batched): Bs, Cs, Ys, As as for the multi-output solves; Hs: batch * nbasis * n, basis
// vector b of matrix k a run of n elements at (k nbasis + b) n; Gs: batch * nquery * nbasis, the basis values of query j at
// (k nquery + j) nbasis; Es: batch * nquery. Be: batch * ntarget * nbasis; Cb: batch * nbasis^2; Al: as Ys; Qd, Lm: batch * ntarget;
// Mn: batch * ntarget * nquery; Vr: batch * nquery. Every output is optional; Ys is read with Be, Al, Qd, Lm, Mn, As and Gs with Mn and Vr,
// Es with Vr.
// (a) the trend form of the one-wavefront SPD sweep, n <= 96 (trend_tile_kernels.hip, trend_tile_f32_kernels.hip)
bool trend_tile_supports(int n);
template <class T>
hipError_t launch_trend_tile(int n, int nbasis, int ntarget, int nquery, const T *Bs, const T *Cs, const T *Hs, const T *Ys, const T *As,
                             const T *Gs, const T *Es, T *Be, T *Cb, T *Al, T *Qd, T *Lm, T *Mn, T *Vr, size_t batch, int *info,
                             hipStream_t stream);
const char *name_trend_tile(bool f64, int n);
// (b) the trend form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_trend_global(int n, int nbasis, int ntarget, int nquery, const T *Bs, const T *Cs, const T *Hs, const T *Ys, const T *As,
                               const T *Gs, const T *Es, T *Be, T *Cb, T *Al, T *Qd, T *Lm, T *Mn, T *Vr, size_t batch, int *info,
                               hipStream_t stream);
const char *name_trend_global(bool f64);

// Gradients of the restricted log marginal likelihood of the trend model (matinv_trend_grad_batched): Bs, Cs, Hs, Ys as above, dMs as for
// matinv_logml_grad_batched; grad: batch * nparam, gradc: batch * n, Lm: batch * ntarget, Al: as Ys, Be: batch * ntarget * nbasis. Every
// output is optional; dMs is read with grad only.
// (a) the gradient form of the trend tile kernels, n <= 96 (trend_grad_tile_kernels.hip, trend_grad_tile_f32_kernels.hip)
bool trend_grad_tile_supports(int n);
template <class T>
hipError_t launch_trend_grad_tile(int n, int nbasis, int ntarget, int nparam, const T *Bs, const T *Cs, const T *Hs, const T *Ys,
                                  const T *dMs, T *grad, T *gradc, T *Lm, T *Al, T *Be, size_t batch, int *info, hipStream_t stream);
const char *name_trend_grad_tile(bool f64, int n);
// (b) the trend gradient form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_trend_grad_global(int n, int nbasis, int ntarget, int nparam, const T *Bs, const T *Cs, const T *Hs, const T *Ys,
                                    const T *dMs, T *grad, T *gradc, T *Lm, T *Al, T *Be, size_t batch, int *info, hipStream_t stream);
const char *name_trend_grad_global(bool f64);

// Leave-one-out cross-validation of the trend model (matinv_trend_loo_batched): Bs, Cs, Hs, Ys as above; Mn: as Ys, Vr: batch * n,
// Lp: batch * ntarget. Every output is optional; Ys is read with Mn and Lp only.
// (a) the leave-one-out form of the trend tile kernels, n <= 96 (trend_loo_tile_kernels.hip, trend_loo_tile_f32_kernels.hip)
bool trend_loo_tile_supports(int n);
template <class T>
hipError_t launch_trend_loo_tile(int n, int nbasis, int ntarget, const T *Bs, const T *Cs, const T *Hs, const T *Ys, T *Mn, T *Vr, T *Lp,
                                 size_t batch, int *info, hipStream_t stream);
const char *name_trend_loo_tile(bool f64, int n);
// (b) the trend leave-one-out form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_trend_loo_global(int n, int nbasis, int ntarget, const T *Bs, const T *Cs, const T *Hs, const T *Ys, T *Mn, T *Vr, T *Lp,
                                   size_t batch, int *info, hipStream_t stream);
const char *name_trend_loo_global(bool f64);

// GP log marginal likelihood and its gradient from coordinates (matinv_ard_logml_batched): Xs: point-major, element (i, k) of matrix b at
// b * xstride + i * ndim + k (xstride = n * ndim, or 0: one point set for the batch); Ys: b * ystride + i (ystride = n or 0);
// Th: batch * (ndim + 2) = (log sf2, log l_1 .. log l_ndim, log sn2); kind: MATINV_COV_*. Lm: batch, Gr: batch * (ndim + 2),
// Al: batch * n; every output is optional. 1 <= ndim <= ARD_MAX_DIM.
constexpr int ARD_MAX_DIM = 16;
// (a) the ARD form of the SPD tile kernels, n <= 96 (ard_tile_kernels.hip, ard_tile_f32_kernels.hip)
bool ard_tile_supports(int n);
template <class T>
hipError_t launch_ard_tile(int kind, int n, int ndim, const T *Xs, size_t xstride, const T *Ys, size_t ystride, const T *Th, T *Lm, T *Gr,
                           T *Al, size_t batch, int *info, hipStream_t stream);
const char *name_ard_tile(bool f64, int n);
// (b) the ARD form of the global-memory Cholesky kernel, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_ard_global(int kind, int n, int ndim, const T *Xs, size_t xstride, const T *Ys, size_t ystride, const T *Th, T *Lm, T *Gr,
                             T *Al, size_t batch, int *info, hipStream_t stream);
const char *name_ard_global(bool f64);

// GP prediction from coordinates (matinv_ard_predict_batched): Xs, Ys, Th, kind as above; Xqs: query j's coordinate k of matrix b at
// b * xqstride + j * ndim + k (xqstride = nquery * ndim, or 0: one query set for the batch). mean, var: batch * nquery, each optional;
// Ys is read with mean only.
// (a) the ARD prediction form of the bordered log-determinant tile kernels, n <= 96 (ard_predict_tile_kernels.hip, ..._f32_kernels.hip)
bool ard_predict_tile_supports(int n);
template <class T>
hipError_t launch_ard_predict_tile(int kind, int n, int ndim, int nquery, const T *Xs, size_t xstride, const T *Ys, size_t ystride,
                                   const T *Th, const T *Xqs, size_t xqstride, T *mean, T *var, size_t batch, int *info, hipStream_t stream);
const char *name_ard_predict_tile(bool f64, int n);
// (b) the ARD prediction form of the global-memory log-determinant kernel's name, n <= 1024 (global_kernels.hip)
template <class T>
hipError_t launch_ard_predict_global(int kind, int n, int ndim, int nquery, const T *Xs, size_t xstride, const T *Ys, size_t ystride,
                                     const T *Th, const T *Xqs, size_t xqstride, T *mean, T *var, size_t batch, int *info,
                                     hipStream_t stream);
const char *name_ard_predict_global(bool f64);

const char *name_gj_lds(bool f64);
const char *name_chol_lds(bool f64);

}  // namespace matinv
