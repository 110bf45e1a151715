// solve_tile_impl.hpp -- fused batched linear solve X = A^-1 B on the one-wavefront MFMA tile layout, 16 < n <= 64,
// 1 <= nrhs <= 16 (solve_tile_kernels.hip: fp64, solve_tile_f32_kernels.hip: fp32). The inverse is never formed.
//
// It is the natural-order Gauss-Jordan kernel of tile_impl.hpp (gj_tile_body) with one extra BORDER tile row: W = A^T
// sits in the NT x NT accumulator tiles exactly as there, and Z = B^T rides below it (row r of Z = column r of B, contiguous
// in memory, loaded like a row of W; rows nrhs .. 15 are zero). Every block step is the same blocked in-place step
//     Aop[i,:] = -W[i,K] D^-1,   W[i,J] += Aop[i,:] W[K,J],   W[:,K] <- Aop        (one 16x16x4 MFMA per tile)
// applied to the border and to the tile rows that still hold unpivoted rows: the solution needs nothing of a row that has been
// a pivot row, so the Cholesky form drops the tile rows above the pivot block's from the update. After the last block step the
// border holds -X^T (S = [A^T; B^T] swept on its first n rows: the border ends as -B^T A^-T), stored negated like a row of W,
// which gives column-major X. The Gauss-Jordan form carries the pivoted tile rows along all the same, through the tile columns
// still to be pivoted, because the verdict needs their multipliers (below). MFMAs per matrix: Cholesky 4 NT (NT (NT + 1) / 2 + NT),
// Gauss-Jordan 2 NT (NT^2 - 1) / 3 more -- 224 and 264 at n = 64 against 256 for the inverse -- and n^2 + 2 n nrhs elements of
// traffic against 2 n^2.
//
// Acceptance (rows of W only; B's entries never cause a rejection):
//   Gauss-Jordan: the natural-order kernel's threshold test (every multiplier |m| <= TILE_TAU, NaN fails), on EVERY row of W
//                 outside the pivot block, the rows already pivoted included: a matrix gets the verdict that inverse_batched
//                 gives it, whichever entry point it comes through (tests/test_gpu_accept.py counts both). A matrix that fails
//                 goes to a device work list and is solved again, in the same stream, by the partially pivoted row solve
//                 (solve_row_kernels.hip) -- which also reports a singular matrix's info exactly like the inverse's pivoting kernels.
//   Cholesky:     A is read from its lower triangle only (W is built symmetric) and every pivot must be positive. The kernel
//                 itself writes info = (first non-positive pivot's column) + 1 and fills X with NaN: no fallback.
#pragma once
#include "tile_screen.hpp"

namespace matinv {

constexpr int SOLVE_MAX_NRHS = 16;

// 1. the 4 pivot columns of block kb of the tile rows t0 .. NT - 1 and of the border -> LDS, [row][4]; the border is panel row 16 NT + z
template <int NT, class T>
__device__ __forceinline__ void solve_panel_to_lds(T *panel, const typename TileGeo<T>::vec4 (&acc)[NT][NT],
                                                   const typename TileGeo<T>::vec4 (&zacc)[NT], int kb, int t0, int q, int c)
{
    typedef TileGeo<T> G;
    const int tK = kb >> 2, rK = kb & 3;
    if (G::blk(c) == rK) {
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            if (ti < t0) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) panel[(16 * ti + G::trow(r, q)) * 4 + G::piv(c)] = acc[ti][tK][r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) panel[(16 * NT + G::trow(r, q)) * 4 + G::piv(c)] = zacc[tK][r];
    }
}

// 5.+6. B operand (pivot rows as they stand, I_4 on the pivot columns) and C operand (zero on the pivot columns) of the tile
// rows t0 .. NT - 1 and the border -- prep_operands of tile_impl.hpp restricted to those rows; asm for the reasons given there.
template <int NT, class T>
__device__ __forceinline__ void solve_prep_operands(typename TileGeo<T>::vec4 (&acc)[NT][NT], typename TileGeo<T>::vec4 (&zacc)[NT],
                                                    T (&bop)[NT], int kb, int t0, int q, int c)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    const int tK = kb >> 2, rK = kb & 3;
    const bool panel_lane = G::blk(c) == rK;
    const bool diag_lane = panel_lane && (G::piv(c) == q);
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) {
        if constexpr (sizeof(T) == 8)
            asm volatile("v_mov_b64_e32 %0, %1\n\tv_mov_b64_e32 %1, 0\n\ts_nop 1" : "=&v"(bop[tj]), "+v"(acc[tK][tj][rK]));
        else
            asm volatile("v_mov_b32_e32 %0, %1\n\tv_mov_b32_e32 %1, 0\n\ts_nop 1" : "=&v"(bop[tj]), "+v"(acc[tK][tj][rK]));
    }
    bop[tK] = panel_lane ? (diag_lane ? (T)1 : (T)0) : bop[tK];
    const unsigned long long zmask = __ballot(panel_lane);
    auto zero_cols = [&](vec4 &t) {
        unsigned long long save;
        if constexpr (sizeof(T) == 8)
            asm volatile("s_and_saveexec_b64 %[save], %[mask]\n\t"
                         "v_mov_b64_e32 %0, 0\n\t"
                         "v_mov_b64_e32 %1, 0\n\t"
                         "v_mov_b64_e32 %2, 0\n\t"
                         "v_mov_b64_e32 %3, 0\n\t"
                         "s_nop 1\n\t"
                         "s_mov_b64 exec, %[save]"
                         : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), [save] "=&s"(save)
                         : [mask] "s"(zmask)
                         : "scc");
        else
            asm volatile("s_and_saveexec_b64 %[save], %[mask]\n\t"
                         "v_mov_b32_e32 %0, 0\n\t"
                         "v_mov_b32_e32 %1, 0\n\t"
                         "v_mov_b32_e32 %2, 0\n\t"
                         "v_mov_b32_e32 %3, 0\n\t"
                         "s_nop 1\n\t"
                         "s_mov_b64 exec, %[save]"
                         : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), [save] "=&s"(save)
                         : [mask] "s"(zmask)
                         : "scc");
    };
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        if (ti < t0) continue;
        zero_cols(acc[ti][tK]);
    }
    zero_cols(zacc[tK]);
}

// One matrix per wavefront, grid-stride over the batch. FULL: n == 16 NT (compile-time addressing). SPD: the Cholesky contract.
template <class T, int NT, bool FULL, bool SPD>
__device__ __forceinline__ void solve_tile_body(BatchRef<const T> Ain, BatchRef<const T> Bin, BatchRef<T> Xout, int *info, int n_rt,
                                                int nrhs, unsigned batch, int *work_count, int *work_list, T *panel)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    typedef typename G::vec2 vec2;
    constexpr int N = 16 * NT;
    constexpr int NKB = 4 * NT;
    // 16-byte accesses through the symmetric relabelling of gj_tile_body (rows and columns of tile pairs interleaved by parity);
    // the border's columns take the same relabelling, its rows stay plain. The Cholesky form mirrors element by element instead.
    constexpr bool PAIRED = FULL && (NT % 2 == 0) && !SPD;
    const int l = threadIdx.x;
    for (unsigned mat = blockIdx.x; mat < batch; mat += gridDim.x) {
        const T *A = Ain.at_uniform(mat);
        const T *B = Bin.at_uniform(mat);
        T *X = Xout.at_uniform(mat);
        int n = FULL ? N : n_rt;
        if (!FULL) asm volatile("" : "+s"(n));
        int q = l >> 4, c = l & 15;
        const unsigned lane_off = (unsigned)(G::trow(0, l >> 4) * n + (l & 15));
        asm volatile("" : "+v"(q), "+v"(c));
        vec4 acc[NT][NT];
        vec4 zacc[NT];
        if (PAIRED) {
            const unsigned lane_off2 = (unsigned)(2 * G::trow(0, l >> 4) * N + 2 * (l & 15));
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int u = 0; u < NT / 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned uoff = (unsigned)((32 * (ti >> 1) + 2 * G::trow(r, 0) + (ti & 1)) * N + 32 * u);
                        const vec2 v = __builtin_nontemporal_load(reinterpret_cast<const vec2 *>(A + uoff + lane_off2));
                        acc[ti][2 * u][r] = v[0];
                        acc[ti][2 * u + 1][r] = v[1];
                    }
#pragma unroll
            for (int u = 0; u < NT / 2; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int z = G::trow(r, q);
                    vec2 v = {(T)0, (T)0};
                    if (z < nrhs) v = __builtin_nontemporal_load(reinterpret_cast<const vec2 *>(B + z * N + 32 * u + 2 * (l & 15)));
                    zacc[2 * u][r] = v[0];
                    zacc[2 * u + 1][r] = v[1];
                }
        } else {
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        // W[row][col] = A(col, row); identity padding beyond n as in gj_tile_body
                        const int row = 16 * ti + G::trow(r, q), col = 16 * tj + c;
                        const bool edge = !FULL && (ti == NT - 1 || tj == NT - 1);
                        T v;
                        if (SPD) {
                            // lower triangle of A only: A(col, row) with col >= row, else its mirror A(row, col)
                            const int lo = row < col ? row : col, hi = row < col ? col : row;
                            v = (!edge || (row < n && col < n)) ? A[(unsigned)(lo * n + hi)] : ((row == col) ? (T)1 : (T)0);
                        } else {
                            const unsigned uoff = (unsigned)((16 * ti + G::trow(r, 0)) * n + 16 * tj);
                            v = (!edge || (row < n && col < n)) ? A[uoff + lane_off] : ((row == col) ? (T)1 : (T)0);
                        }
                        acc[ti][tj][r] = v;
                    }
#pragma unroll
            for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int z = G::trow(r, q), col = 16 * tj + c;
                    zacc[tj][r] = (z < nrhs && (FULL || col < n)) ? B[(unsigned)(z * n + col)] : (T)0;  // zero padding
                }
        }
        unsigned long long bad = 0;  // wave-uniform: acceptance test failed somewhere
        int binfo = 0;               // SPD: column of the first non-positive pivot + 1
        T aop[NT], bop[NT], zop;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            if (!FULL && kb > 4 * (NT - 1) && kb - 4 * (NT - 1) >= G::real_blocks(n - 16 * (NT - 1))) continue;  // all padding
            const int tK = kb >> 2;
            // Gauss-Jordan: the tile rows above the pivot block's come along for their multipliers alone (see the head of the file)
            const int t0 = SPD ? tK : 0;
            solve_panel_to_lds<NT, T>(panel, acc, zacc, kb, t0, q, c);
            wave_lds_sync();
            {
                PanelSolve<NT, SPD, T> ps;
                if (SPD) ps.binfo = &binfo;
#pragma unroll
                for (int s = 0; s < 6; ++s) ps.stage(s, panel, kb, q, c, aop, bad);
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
                    if (ti >= t0) ps.stage(6 + ti, panel, kb, q, c, aop, bad);
                // border: Zop[z,:] = -Z[z,K] D^-1 (lane c = border row c, column q), exempt from the test
                const T *w = &panel[(16 * NT + c) * 4];
                zop = -fma_t(w[3], ps.x3, fma_t(w[2], ps.x2, fma_t(w[1], ps.x1, w[0] * ps.x0)));
            }
            wave_lds_sync();  // the panel is rewritten by the next block step
            solve_prep_operands<NT, T>(acc, zacc, bop, kb, t0, q, c);
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                if (ti < t0) continue;
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) {
                    if (ti < tK && tj < tK) continue;  // a pivoted row's pivoted columns: no later multiplier reads them
                    acc[ti][tj] = G::mfma(aop[ti], bop[tj], acc[ti][tj]);
                }
            }
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) zacc[tj] = G::mfma(zop, bop[tj], zacc[tj]);
        }
        const bool store = SPD || bad == 0;
        if (store) {
            // X = -Z^T; a matrix that is not SPD gets NaN everywhere
            const T sgn = (SPD && bad != 0) ? nan_of<T>() : (T)-1;
            if (PAIRED) {
#pragma unroll
                for (int u = 0; u < NT / 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int z = G::trow(r, q);
                        vec2 v;
                        v[0] = sgn * zacc[2 * u][r];
                        v[1] = sgn * zacc[2 * u + 1][r];
                        if (z < nrhs) __builtin_nontemporal_store(v, reinterpret_cast<vec2 *>(X + z * N + 32 * u + 2 * (l & 15)));
                    }
            } else {
#pragma unroll
                for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int z = G::trow(r, q), col = 16 * tj + c;
                        if (z < nrhs && (FULL || col < n)) X[(unsigned)(z * n + col)] = sgn * zacc[tj][r];
                    }
            }
            int code = SPD ? binfo : 0;
            if constexpr (SPD && sizeof(T) == 4) {
                if (bad != 0) {  // wave-uniform; rejected matrices only: the fp32 tile order does not say which column fails FIRST (tile_common.hpp)
                    const int nat = spd_natural_first_failure<NT, T>(A, (const T *)nullptr, n, panel, l);
                    if (nat) code = nat;
                }
            }
            if (info && l == 0) info[mat] = code;
        } else if (l == 0) {
            const int slot = atomicAdd(work_count, 1);
            work_list[slot] = (int)mat;
        }
    }
}

template <int NT, bool FULL, bool SPD>
__global__ __launch_bounds__(64, 2) void matinv_solve_tile_f64(BatchRef<const double> A, BatchRef<const double> B, BatchRef<double> X,
                                                               int *info, int n, int nrhs, unsigned batch, int *work_count,
                                                               int *work_list)
{
    __shared__ __attribute__((aligned(16))) double panel[16 * (NT + 1) * 4];  // [row][4 pivot columns], border rows last
    solve_tile_body<double, NT, FULL, SPD>(A, B, X, info, n, nrhs, batch, work_count, work_list, panel);
}

// fp32: three waves per SIMD -- with four (128 registers) the 4 x 4-tile instantiation spills the border
template <int NT, bool FULL, bool SPD>
__global__ __launch_bounds__(64, 3) void matinv_solve_tile_f32(BatchRef<const float> A, BatchRef<const float> B, BatchRef<float> X,
                                                               int *info, int n, int nrhs, unsigned batch, int *work_count,
                                                               int *work_list)
{
    __shared__ __attribute__((aligned(16))) float panel[16 * (NT + 1) * 4];  // [row][4 pivot columns], border rows last
    solve_tile_body<float, NT, FULL, SPD>(A, B, X, info, n, nrhs, batch, work_count, work_list, panel);
}

// GJ: the fused kernel, then the row solve over the matrices it rejected (same stream, device-side work list; the list length feeds
// the MATINV_DEBUG_REJECTS counter). Cholesky: the fused kernel alone.
template <class T>
hipError_t launch_solve_tile(int algo, int n, int nrhs, BatchRef<const T> A, BatchRef<const T> B, BatchRef<T> X, size_t batch, int *info,
                             hipStream_t stream)
{
    if (!solve_tile_supports(n, nrhs)) return hipErrorInvalidValue;
    const bool spd = algo == MATINV_ALGO_CHOLESKY;
    auto launch = [&](int *work_count, int *work_list) {
        // grid-stride over the batch, as the natural-order inverse (launch_gj_tile_natural)
        const unsigned grid = tile_grid(batch, sizeof(T) == 8 ? 8u : 16u), b = (unsigned)batch;
        with_tile<2, 4>(tile_shape(n), [&](auto NT, auto FULL) {
            auto go = [&](auto SPD) {
                if constexpr (sizeof(T) == 8)
                    hipLaunchKernelGGL((matinv_solve_tile_f64<NT, FULL, SPD>), dim3(grid), dim3(64), 0, stream, A, B, X, info, n, nrhs, b,
                                       work_count, work_list);
                else
                    hipLaunchKernelGGL((matinv_solve_tile_f32<NT, FULL, SPD>), dim3(grid), dim3(64), 0, stream, A, B, X, info, n, nrhs, b,
                                       work_count, work_list);
            };
            if (spd) go(std::true_type{});
            else go(std::false_type{});
        });
        return hipGetLastError();
    };
    if (spd) return launch(nullptr, nullptr);
    // [0] count, [4 ..) list
    return with_scratch_ints(batch + 4, 1, stream, [&](int *ws) {
        hipError_t e = launch(ws, ws + 4);
        if (e == hipSuccess) e = launch_solve_row_worklist<T>(n, nrhs, A, B, X, ws, ws + 4, info, stream);
        if (e == hipSuccess) e = debug_note_rejects(ws, stream);
        return e;
    });
}

}  // namespace matinv
