// whiten_tile_impl.hpp (instantiated by whiten_tile_kernels.hip for f64 and whiten_tile_f32_kernels.hip for f32) -- whitened points,
// squared Mahalanobis distances, the log-determinant and the Gaussian log-density of batched SPD matrices on the MFMA tile layout, n <= 96:
//     C = L L^T (lower triangle of C read),   W[:, s] = L^-1 (x_s - m)   (m optional),   maha[s] = ||W[:, s]||^2,
//     logdet = 2 sum_i log L_ii,   logpdf[s] = -1/2 (maha[s] + logdet + n log 2 pi)
// The load (tile_nat for fp32, so that the sweep's order is the natural order), the PanelSolve pipeline, the block-step loop and the
// `columns` step that leaves the factor in registers are those of colour_tile_body (colour_tile_impl.hpp), copied once more so that every
// earlier kernel compiles to what it compiled to before; the factor itself is not stored. What this form adds:
//   * columns() keeps lop[kb][ti] = -L[16 ti + c][pivot q of block step kb] (the A operand of the update below, negated once) and, per
//     block step, one more A operand mop[kb]: with the unit-lower factor l10 .. l32 of the 4 x 4 pivot block and its squared Cholesky
//     diagonal u, the diagonal block of L is l diag(sqrt u), its inverse M = diag(1 / sqrt u) l^-1. l^-1 costs six multiply-adds, the same
//     in every lane; lane (q, c) keeps M[t][q] when c is the tile-local row that accumulator register 0 of lane group t holds (fp64: c = t,
//     fp32: c = 4 t), and zero otherwise. The four pivots of the step are folded into a PivotProduct, as in logdet_tile_body.
//   * Forward substitution over a group of 16 points, straight out of registers. y[ti][r] = (x - m)[16 ti + trow(r, q)][point c] is an
//     accumulator-layout tile, and in both TileGeos pivot t of block rK is row trow(rK, t): y[tK][rK] of lane (t, c) IS the B operand
//     (K index t, column c) of the step's four right-hand sides. Per block step kb = 4 tK + rK ascending:
//         d = mfma(mop[kb], y[tK][rK], 0)          d[0] of lane (t, c) = w of pivot t, point c: in B layout again
//         part = fma(w, w, part)                   the lane's share of ||w||^2
//         y[ti] = mfma(lop[kb][ti], w, y[ti])      ti >= tK
//         y[tK][rK] = w                            the solved rows take the place of their right-hand sides
//     Two dependent MFMAs per block step and no transposition through LDS. The rows beyond n meet the identity padding and stay zero.
//   * maha[s]: the 16 lanes (t, s) of the four lane groups hold the partial sums over pivots t = 0 .. 3 of all block steps; they meet in
//     LDS as ((p0 + p1) + (p2 + p3)). logpdf = -1/2 fma(n, log 2 pi, maha + logdet) with the logdet the caller gets.
//   * W for a group leaves through the group buffer, so every global access of the epilogue is a run of consecutive elements.
// Nothing in the order of operations of an output depends on batch, grid, S, or the group or lane of a point; which outputs are stored is
// decided by wave-uniform pointers and changes no operation. X is read only when W, maha or logpdf is requested.
// x = m: y = +0, every product is a zero and the accumulators start at +0: W = +0.0 and maha = +0.0.
// HBM traffic per matrix: n^2 / 2 + n + n S elements in, n S + 2 S + 1 out.
// A non-positive (or NaN) pivot makes info = its column + 1 and every requested output NaN: no fallback launch.
//
// The kernels are the whiten forms of the SPD inversion kernels whose sweep they run: overloads of matinv_spd_tile_f64 / _f32 with seven
// more trailing template arguments ("Whitening").
#pragma once
#include "colour_tile_impl.hpp"  // tile_nat, colour_sqrt; predict_qstride, predict_tile_grid
#include "pivot_product.hpp"

namespace matinv {

template <class T, int NT, bool FULL>
__device__ __forceinline__ void whiten_tile_body(const T *Cs, size_t stride, const T *Ms, const T *Xs, int npoint, T *Ws, T *Mh, T *Ld, T *Lp,
                                                 int *info, int n_rt, unsigned batch, T *panel, T *ml, T *xq)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    constexpr int N = 16 * NT;
    constexpr int NKB = 4 * NT;
    constexpr int NS = predict_qstride(N);
    typedef PanelSolve<NT, true, T> PS;
    const int l = threadIdx.x;

    for (unsigned mat = blockIdx.x; mat < batch; mat += gridDim.x) {
        int n = FULL ? N : n_rt;  // run-time n opaque once per matrix, predicates on the edge tiles only: see gj_tile_body
        if (!FULL) asm volatile("" : "+s"(n));
        const T *A = Cs + (size_t)mat * stride;
        int q = l >> 4, c = l & 15;
        asm volatile("" : "+v"(q), "+v"(c));  // see matinv_gj_tile_f64
        const int cn = tile_nat<T>(c);  // the natural tile-local column (and panel row) of this lane

        vec4 acc[NT][NT];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) {
                if (tj > ti) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * ti + tile_nat<T>(G::trow(r, q)), col = 16 * tj + cn;
                    const bool in = FULL || ti < NT - 1 || (row < n && col < n);  // tj <= ti: only the last tile row reaches beyond n
                    const int hi = row > col ? row : col, lo = row > col ? col : row;
                    // only the lower triangle is read (mirror position inside the diagonal tiles)
                    acc[ti][tj][r] = in ? A[(unsigned)(lo * n + hi)] : ((row == col) ? (T)1 : (T)0);
                }
            }

        unsigned long long bad = 0;
        int binfo = 0;  // position of the first non-positive pivot + 1
        PivotProduct<T> prod;
        T aop[NT], bop[NT];
        T lop[NKB][NT];  // lop[kb][ti], ti >= kb / 4: -L[16 ti + c][pivot q of block step kb], the A operand of the substitution's update
        T mop[NKB];      // mop[kb]: (diag(1 / sqrt u) l^-1)[t][q] in the lane whose c is row trow(0, t), else 0: the A operand of its solve
        // the accumulator register 0 of lane group t holds tile-local row trow(0, t): fp64 t, fp32 4 t
        const bool slot = sizeof(T) == 8 ? c < 4 : (c & 3) == 0;
        const int tc = sizeof(T) == 8 ? (c & 3) : (c >> 2);

        // the four Cholesky columns of block step kb out of its solved pivot block and the panel in LDS, and the inverse of its diagonal block
        auto columns = [&](const PS &ps, const int kb) {
            const int tK = kb >> 2, rK = kb & 3;
            prod.fold(ps.d[0][0], ps.u11, ps.u22, ps.u33);
            const T u01 = (q & 1) ? ps.u11 : ps.d[0][0], u23 = (q & 1) ? ps.u33 : ps.u22;
            const T sq = colour_sqrt((q & 2) ? u23 : u01);
            const T rq = (T)1 / sq;
            const int coll = tile_nat<T>(G::pcol(rK, q));
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                if (ti < tK) continue;
                const T *w = &panel[(16 * ti + c) * 4];
                const T x0 = w[0];
                const T x1 = fma_t(-ps.l10, x0, w[1]);
                const T x2 = fma_t(-ps.l21, x1, fma_t(-ps.l20, x0, w[2]));
                const T x3 = fma_t(-ps.l32, x2, fma_t(-ps.l31, x1, fma_t(-ps.l30, x0, w[3])));
                const T x01 = (q & 1) ? x1 : x0, x23 = (q & 1) ? x3 : x2;
                T v = ((q & 2) ? x23 : x01) * rq;
                if (ti == tK) v = cn < coll ? (T)0 : (cn == coll ? sq : v);
                v = -v;
                asm volatile("" : "+v"(v));  // formed HERE, not in the epilogue's branch out of the four panel values: see mop below
                lop[kb][ti] = v;
            }
            // row tc of l^-1 (unit lower), column q; the diagonal block of L is l diag(sqrt u)
            const T m10 = -ps.l10, m21 = -ps.l21, m32 = -ps.l32;
            const T m20 = fma_t(ps.l21, ps.l10, -ps.l20);
            const T m31 = fma_t(ps.l32, ps.l21, -ps.l31);
            const T m30 = fma_t(-ps.l32, m20, fma_t(-ps.l31, m10, -ps.l30));
            const T r2 = q == 0 ? m20 : m21, r3 = q == 0 ? m30 : (q == 1 ? m31 : m32);
            T e = tc == 1 ? m10 : (tc == 2 ? r2 : r3);
            e = q > tc ? (T)0 : (q == tc ? (T)1 : e);
            const T uc01 = (tc & 1) ? ps.u11 : ps.d[0][0], uc23 = (tc & 1) ? ps.u33 : ps.u22;
            const T rqc = (T)1 / colour_sqrt((tc & 2) ? uc23 : uc01);
            T mo = slot ? e * rqc : (T)0;
            // formed HERE: without the pin hipcc sinks these lines into the epilogue's branch and keeps l and u of all 4 NT block steps
            // alive until then (hundreds of spilled registers), as it does with the pivots of PivotProduct::fold
            asm volatile("" : "+v"(mo));
            mop[kb] = mo;
        };

        spd_panel_to_lds<NT, T>(panel, acc, 0, q, c);
        wave_lds_sync();
        {
            PS ps0;
            ps0.binfo = &binfo;
#pragma unroll
            for (int s = 0; s < PS::NSTAGE; ++s) ps0.stage(s, panel, 0, q, c, aop, bop, bad);
            columns(ps0, 0);
        }
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            if (kb + 1 < NKB) {
                spd_prep_operands<NT, T>(acc, bop, kb, q, c);
                const int tn = (kb + 1) >> 2;
                // (a) the tile column the next panel is read from (rows above it are dead)
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) {
                    if (ti < tn) continue;
                    acc[ti][tn] = G::mfma(aop[ti], bop[tn], acc[ti][tn]);
                }
                // (b) the other LIVE lower tiles, pinned between the pieces of the next panel. Live = right of the next panel's tile
                // column: the pivot block's own tile column is only read again through that panel (a factorisation, no inverse)
                constexpr int NSG = PS::NSTAGE;
                int nb = 0;  // number of (b) tiles: folds to a literal
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int tj = 0; tj < NT; ++tj)
                        if (tj <= ti && tj > tn) ++nb;
                T aop_next[NT], bop_next[NT];
                PS ps;
                ps.binfo = &binfo;
                int count = 0, ev = 0;
                auto run_events = [&](bool flush) {
#pragma unroll
                    for (int e = 0; e < NSG + 1; ++e) {
                        const int lead = nb < 2 ? nb : 2;
                        const int thr = (e == 0) ? lead : lead + ((nb - lead) * e) / NSG;
                        if (e == ev && (flush || thr <= count)) {
                            __builtin_amdgcn_sched_barrier(0);
                            if (e == 0) {
                                wave_lds_sync();
                                spd_panel_to_lds<NT, T>(panel, acc, kb + 1, q, c);
                                wave_lds_sync();
                            } else if (e - 1 < 6 || e - 1 - 6 >= tn) {  // tile rows above the next pivot block are dead
                                ps.stage(e - 1, panel, kb + 1, q, c, aop_next, bop_next, bad);
                            }
                            __builtin_amdgcn_sched_barrier(0);
                            ++ev;
                        }
                    }
                };
                run_events(false);
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int tj = 0; tj < NT; ++tj) {
                        if (tj > ti || tj <= tn) continue;
                        acc[ti][tj] = G::mfma(aop[ti], bop[tj], acc[ti][tj]);
                        ++count;
                        run_events(false);
                    }
                run_events(true);
                columns(ps, kb + 1);  // the panel of step kb + 1 stays in LDS until the next step stages its own
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) { aop[ti] = aop_next[ti]; bop[ti] = bop_next[ti]; }
            }
        }

        const bool ok = bad == 0;
        const T ld = prod.log_value();
        if (Ld && l == 0) Ld[mat] = ok ? ld : nan_of<T>();
        if (Ws || Mh || Lp) {  // wave-uniform; the points are not read otherwise
            const size_t first = (size_t)mat * npoint;
            wave_lds_sync();  // the last panel has been consumed
#pragma unroll
            for (int k = 0; k < (N + 63) / 64; ++k) {
                const int i = l + 64 * k;
                if (i < N) ml[i] = (Ms && (FULL || i < n)) ? Ms[(size_t)mat * n + i] : (T)0;
            }
            const int ngroups = (npoint + 15) >> 4;
            for (int g = 0; g < ngroups; ++g) {
                // lane coordinates and n opaque once per group: otherwise the offsets of the staging loads and of the LDS reads are
                // hoisted out of this loop and the allocator spills them beside the factor (as in predict_tile_body)
                int ng = n, lg = l, qg = q, cg = c;
                if (!FULL) asm volatile("" : "+s"(ng));
                asm volatile("" : "+v"(lg), "+v"(qg), "+v"(cg));
                const int left = npoint - 16 * g;  // points from this group's first on
                const T *Xg = Xs + (first + 16 * (size_t)g) * ng;
                wave_lds_sync();  // the previous group's reads of xq and panel, this matrix's writes of ml
                // the group's 16 n contiguous elements, consecutive lanes on consecutive elements of one point
#pragma unroll
                for (int k = 0; k < N / 4; ++k) {
                    const int e = lg + 64 * k, j = e / N, i = e - j * N;
                    const bool in = (FULL || i < ng) && j < left;
                    xq[j * NS + i] = in ? Xg[(unsigned)(j * ng + i)] : (T)0;
                }
                wave_lds_sync();
                T *const xc = xq + cg * NS;  // the point of this lane
                vec4 y[NT];
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * ti + tile_nat<T>(G::trow(r, qg));
                        y[ti][r] = xc[row] - ml[row];
                    }
                T part = (T)0;
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) {
                    const int tK = kb >> 2, rK = kb & 3;
                    const vec4 d = G::mfma(mop[kb], y[tK][rK], vec4{(T)0, (T)0, (T)0, (T)0});
                    const T w = d[0];
                    part = fma_t(w, w, part);
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti) {
                        if (ti < tK) continue;
                        y[ti] = G::mfma(lop[kb][ti], w, y[ti]);
                    }
                    y[tK][rK] = w;
                }
                wave_lds_sync();  // the right-hand sides have been read: the buffer takes the group's W, point by point
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) xc[16 * ti + tile_nat<T>(G::trow(r, qg))] = ok ? y[ti][r] : nan_of<T>();
                panel[lg] = part;
                wave_lds_sync();
                if (Ws) {  // wave-uniform
                    T *Wg = Ws + (first + 16 * (size_t)g) * ng;
#pragma unroll
                    for (int k = 0; k < N / 4; ++k) {
                        const int e = lg + 64 * k, j = e / N, i = e - j * N;
                        if ((FULL || i < ng) && j < left) Wg[(unsigned)(j * ng + i)] = xq[j * NS + i];
                    }
                }
                if (lg < 16 && lg < left) {
                    const T mh = (panel[lg] + panel[16 + lg]) + (panel[32 + lg] + panel[48 + lg]);
                    const size_t at = first + 16 * (size_t)g + lg;
                    if (Mh) Mh[at] = ok ? mh : nan_of<T>();
                    // log 2 pi
                    if (Lp) Lp[at] = ok ? (T)-0.5 * fma_t((T)ng, (T)1.83787706640934548356, mh + ld) : nan_of<T>();
                }
            }
        }
        // PanelSolve names a tile-local position; the column is the natural index it holds
        int code = binfo ? ((binfo - 1) & ~15) + tile_nat<T>((binfo - 1) & 15) + 1 : 0;
        if constexpr (sizeof(T) == 4) {
            if (bad != 0) {  // wave-uniform; rejected matrices only: the natural-order recount of the other fp32 forms (tile_common.hpp)
                wave_lds_sync();
                const int nat = spd_natural_first_failure<NT, T>(A, (const T *)nullptr, n, panel, l);
                if (nat) code = nat;
            }
        }
        if (info && l == 0) info[mat] = code;
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// The whiten forms of matinv_spd_tile_f64 / matinv_spd_tile_f32 (tile_impl.hpp): the same names with a third to a ninth template
// argument. Launch bounds: those of the colour forms for the same NT (colour_tile_impl.hpp), one wave per SIMD fewer where a form spills
// under them: the ragged 4 x 4 forms (2 registers in fp64, 13 in fp32) and the ragged fp32 6 x 6 form (8), which keep one more A
// operand per block step than the colour forms and the edge predicates beside it (profiles/whiten_kernel_registers.txt). No form uses
// scratch.
constexpr int whiten_f64_waves(int nt, bool full) { return nt == 4 && !full ? 1 : colour_f64_waves(nt); }
constexpr int whiten_f32_waves(int nt, bool full) { return nt == 6 && !full ? 1 : (nt == 4 && !full ? 2 : colour_f32_waves(nt)); }

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN>
__global__ __launch_bounds__(64, whiten_f64_waves(NT, FULL)) void matinv_spd_tile_f64(const double *Cs, size_t stride, const double *Ms,
                                                                                       const double *Xs, int npoint, double *Ws, double *Mh,
                                                                                       double *Ld, double *Lp, int *info, int n_rt,
                                                                                       unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN, "the nine-argument form is the whiten kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    __shared__ double ml[16 * NT], xq[16 * predict_qstride(16 * NT)];
    whiten_tile_body<double, NT, FULL>(Cs, stride, Ms, Xs, npoint, Ws, Mh, Ld, Lp, info, n_rt, batch, panel, ml, xq);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN>
__global__ __launch_bounds__(64, whiten_f32_waves(NT, FULL)) void matinv_spd_tile_f32(const float *Cs, size_t stride, const float *Ms,
                                                                                       const float *Xs, int npoint, float *Ws, float *Mh,
                                                                                       float *Ld, float *Lp, int *info, int n_rt,
                                                                                       unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN, "the nine-argument form is the whiten kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    __shared__ float ml[16 * NT], xq[16 * predict_qstride(16 * NT)];
    whiten_tile_body<float, NT, FULL>(Cs, stride, Ms, Xs, npoint, Ws, Mh, Ld, Lp, info, n_rt, batch, panel, ml, xq);
}

template <class T>
hipError_t launch_whiten_tile(int n, int npoint, const T *Cs, size_t stride, const T *Ms, const T *Xs, T *Ws, T *Mh, T *Ld, T *Lp,
                              size_t batch, int *info, hipStream_t stream)
{
    if (!whiten_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = predict_tile_grid(batch), b = (unsigned)batch;  // 256 * 12 workgroups a round (predict_tile_impl.hpp)
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true, true, true, true, true, true>), dim3(grid), dim3(64), 0, stream, Cs,
                               stride, Ms, Xs, npoint, Ws, Mh, Ld, Lp, info, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true, true, true, true, true, true>), dim3(grid), dim3(64), 0, stream, Cs,
                               stride, Ms, Xs, npoint, Ws, Mh, Ld, Lp, info, n, b);
    });
    return hipGetLastError();
}
}  // namespace matinv
