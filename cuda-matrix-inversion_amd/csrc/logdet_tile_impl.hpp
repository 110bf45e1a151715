// logdet_tile_impl.hpp (instantiated by logdet_tile_kernels.hip for f64 and logdet_tile_f32_kernels.hip for f32) -- batched
// log-determinant of SPD matrices and the Gaussian-process log marginal likelihood on the MFMA tile layout, n <= 96:
//     BORDER = false:  logabsdet = log det A                      (sign = +1)
//     BORDER = true :  logml = -1/2 d^T M^-1 d - 1/2 log det M - n/2 log(2 pi),   M = B + diag c   (c optional)
// It is the symmetric blocked sweep of gp_tile_body (gp_tile_impl.hpp): one wavefront per matrix, lower-triangular 16 x 16
// accumulator tiles, tile columns left of the pivot block dead and skipped, the next block's panel solved between the MFMAs
// of the current one. Nothing but the factorisation is computed: the four pivots every block step divides by (PanelSolve's
// d[0][0], u11, u22, u33: the squares of the Cholesky diagonal, the same value in every lane) are folded into a running
// mantissa / exponent pair, so the determinant itself is never formed and neither overflows nor underflows; one logarithm
// is taken at the end. Identity padding beyond n has pivots of exactly 1 and contributes exactly nothing. With a border, the
// single border row holds d and the corner tile ends as -d^T M^-1 d. HBM traffic per matrix: the lower tiles of A (plus c and
// d) in, one or two scalars out.
// A non-positive (or NaN) pivot makes info = its column + 1 (PanelSolve::binfo, as in solve_tile_body) and every output NaN:
// no fallback launch.
#pragma once
#include <cstdio>

#include "pivot_product.hpp"
#include "tile_common.hpp"

namespace matinv {

// logdet: out0 = logabsdet, out1 = sign (optional). logml (BORDER): out0 = logml, Cs optional, Ds the border.
template <class T, int NT, bool FULL, bool BORDER>
__device__ __forceinline__ void logdet_tile_body(const T *As, size_t stride, const T *Cs, const T *Ds, T *out0, T *out1, int *info,
                                                 int n_rt, unsigned batch, T *panel)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    constexpr int N = 16 * NT;
    constexpr int NX = NT + (BORDER ? 1 : 0);  // tile rows/cols of the (bordered) matrix; R = NT is the border
    [[maybe_unused]] constexpr int R = NX - 1;  // the border's tile row (BORDER only)
    constexpr int NKB = 4 * NT;
    typedef PanelSolve<NX, true, T> PS;
    const int l = threadIdx.x;

    for (unsigned mat = blockIdx.x; mat < batch; mat += gridDim.x) {
        int n = FULL ? N : n_rt;  // run-time n opaque once per matrix, predicates on the edge tiles only: see gj_tile_body
        if (!FULL) asm volatile("" : "+s"(n));
        const T *A = As + (size_t)mat * stride;
        int q = l >> 4, c = l & 15;
        asm volatile("" : "+v"(q), "+v"(c));  // see matinv_gj_tile_f64

        vec4 acc[NX][NX];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) {
                if (tj > ti) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * ti + G::trow(r, q), col = 16 * tj + c;
                    const bool in = FULL || ti < NT - 1 || (row < n && col < n);  // tj <= ti: only the last tile row reaches beyond n
                    const int hi = row > col ? row : col, lo = row > col ? col : row;
                    // only the lower triangle is read (mirror position inside the diagonal tiles)
                    T v = in ? A[(unsigned)(lo * n + hi)] : ((row == col) ? (T)1 : (T)0);
                    if (BORDER && Cs && ti == tj && row == col && in) v += Cs[(size_t)mat * n + row];
                    acc[ti][tj][r] = v;
                }
            }
        if constexpr (BORDER) {
            const T *vd = Ds + (size_t)mat * n;
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) {
                const int col = 16 * tj + c;
                const bool in = FULL || tj < NT - 1 || col < n;
                const T w = in ? vd[col] : (T)0;
                acc[R][tj][0] = (q == 0) ? w : (T)0;  // border row trow(0,0) holds d; the others are zero
                acc[R][tj][1] = (T)0, acc[R][tj][2] = (T)0, acc[R][tj][3] = (T)0;
            }
            acc[R][R] = vec4{(T)0, (T)0, (T)0, (T)0};
        }

        unsigned long long bad = 0;
        int binfo = 0;  // column of the first non-positive pivot + 1
        PivotProduct<T> prod;
        T aop[NX], bop[NX];
        spd_panel_to_lds<NX, T>(panel, acc, 0, q, c);
        wave_lds_sync();
        {
            PS ps0;
            ps0.binfo = &binfo;
#pragma unroll
            for (int s = 0; s < PS::NSTAGE; ++s) ps0.stage(s, panel, 0, q, c, aop, bop, bad);
            prod.fold(ps0.d[0][0], ps0.u11, ps0.u22, ps0.u33);
        }
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            if (kb + 1 < NKB) {
                spd_prep_operands<NX, T>(acc, bop, kb, q, c);
                const int tn = (kb + 1) >> 2;
                // (a) the tile column the next panel is read from (rows above it are dead)
#pragma unroll
                for (int ti = 0; ti < NX; ++ti) {
                    if (ti < tn) continue;
                    acc[ti][tn] = G::mfma(aop[ti], bop[tn], acc[ti][tn]);
                }
                // (b) the other LIVE lower tiles, pinned between the pieces of the next panel. Live = right of the next panel's tile
                // column: the pivot block's own tile column is only read again through that panel (a factorisation, no inverse)
                constexpr int NS = PS::NSTAGE;
                int nb = 0;  // number of (b) tiles: folds to a literal
#pragma unroll
                for (int ti = 0; ti < NX; ++ti)
#pragma unroll
                    for (int tj = 0; tj < NX; ++tj)
                        if (tj <= ti && tj > tn) ++nb;
                T aop_next[NX], bop_next[NX];
                PS ps;
                ps.binfo = &binfo;
                int count = 0, ev = 0;
                auto run_events = [&](bool flush) {
#pragma unroll
                    for (int e = 0; e < NS + 1; ++e) {
                        const int lead = nb < 2 ? nb : 2;
                        const int thr = (e == 0) ? lead : lead + ((nb - lead) * e) / NS;
                        if (e == ev && (flush || thr <= count)) {
                            __builtin_amdgcn_sched_barrier(0);
                            if (e == 0) {
                                wave_lds_sync();
                                spd_panel_to_lds<NX, T>(panel, acc, kb + 1, q, c);
                                wave_lds_sync();
                            } else if (e - 1 < 6 || e - 1 - 6 >= tn) {  // tile rows above the next pivot block are dead
                                ps.stage(e - 1, panel, kb + 1, q, c, aop_next, bop_next, bad);
                                if (e - 1 == 3) prod.fold(ps.d[0][0], ps.u11, ps.u22, ps.u33);
                            }
                            __builtin_amdgcn_sched_barrier(0);
                            ++ev;
                        }
                    }
                };
                run_events(false);
#pragma unroll
                for (int ti = 0; ti < NX; ++ti)
#pragma unroll
                    for (int tj = 0; tj < NX; ++tj) {
                        if (tj > ti || tj <= tn) continue;
                        acc[ti][tj] = G::mfma(aop[ti], bop[tj], acc[ti][tj]);
                        ++count;
                        run_events(false);
                    }
                run_events(true);
#pragma unroll
                for (int ti = 0; ti < NX; ++ti) { aop[ti] = aop_next[ti]; bop[ti] = bop_next[ti]; }
            } else if constexpr (BORDER) {
                // last pivot block: only the corner matters
                spd_prep_operands<NX, T>(acc, bop, kb, q, c);
                acc[R][R] = G::mfma(aop[R], bop[R], acc[R][R]);
            }
        }

        const bool ok = bad == 0;
        const T ld = prod.log_value();
        if constexpr (BORDER) {
            // corner tile register 0, lane 0: G[d][d] = -d^T M^-1 d
            const T g = acc[R][R][0];
            const T half = (T)0.5;
            if (l == 0) out0[mat] = ok ? half * g - half * ld - (T)n * (T)0.91893853320467274178 : nan_of<T>();
        } else if (l == 0) {
            out0[mat] = ok ? ld : nan_of<T>();
            if (out1) out1[mat] = ok ? (T)1 : nan_of<T>();
        }
        int code = binfo;
        if constexpr (sizeof(T) == 4) {
            if (bad != 0) {  // wave-uniform; rejected matrices only: the fp32 tile order does not say which column fails FIRST (tile_common.hpp)
                const int nat = spd_natural_first_failure<NT, T>(A, (BORDER && Cs) ? Cs + (size_t)mat * n : nullptr, n, panel, l);
                if (nat) code = nat;
            }
        }
        if (info && l == 0) info[mat] = code;
        wave_lds_sync();
    }
}

// the register budget of matinv_gp_tile_f64, except the bordered 5 x 5 form: with the pivot fold beside the panel solve it is 6 registers
// over the 256 of two waves per SIMD, so it takes one wave per SIMD like the 6 x 6 forms rather than spill
template <int NT, bool FULL, bool BORDER>
__global__ __launch_bounds__(64, (NT >= 6 || (BORDER && NT >= 5)) ? 1 : 2) void matinv_logdet_tile_f64(const double *As, size_t stride, const double *Cs,
                                                                              const double *Ds, double *out0, double *out1, int *info,
                                                                              int n_rt, unsigned batch)
{
    __shared__ __attribute__((aligned(16))) double panel[(16 * NT + 16) * 4];
    logdet_tile_body<double, NT, FULL, BORDER>(As, stride, Cs, Ds, out0, out1, info, n_rt, batch, panel);
}

template <int NT, bool FULL, bool BORDER>
__global__ __launch_bounds__(64, NT >= 6 ? 2 : 3) void matinv_logdet_tile_f32(const float *As, size_t stride, const float *Cs,
                                                                              const float *Ds, float *out0, float *out1, int *info,
                                                                              int n_rt, unsigned batch)
{
    __shared__ __attribute__((aligned(16))) float panel[(16 * NT + 16) * 4];
    logdet_tile_body<float, NT, FULL, BORDER>(As, stride, Cs, Ds, out0, out1, info, n_rt, batch, panel);
}

// border == false: logdet (Cs, Ds unused); border == true: logml
template <class T>
hipError_t launch_logdet_tile(int n, bool border, const T *As, size_t stride, const T *Cs, const T *Ds, T *out0, T *out1, size_t batch,
                              int *info, hipStream_t stream)
{
    if (!logdet_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = tile_grid(batch, 8u), b = (unsigned)batch;
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        auto go = [&](auto BORDER) {
            if constexpr (sizeof(T) == 8)
                hipLaunchKernelGGL((matinv_logdet_tile_f64<NT, FULL, BORDER>), dim3(grid), dim3(64), 0, stream, As, stride, Cs, Ds, out0, out1,
                                   info, n, b);
            else
                hipLaunchKernelGGL((matinv_logdet_tile_f32<NT, FULL, BORDER>), dim3(grid), dim3(64), 0, stream, As, stride, Cs, Ds, out0, out1,
                                   info, n, b);
        };
        if (border) go(std::true_type{});
        else go(std::false_type{});
    });
    return hipGetLastError();
}
}  // namespace matinv
