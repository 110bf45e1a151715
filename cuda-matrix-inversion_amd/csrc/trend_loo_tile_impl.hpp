// trend_loo_tile_impl.hpp (instantiated by trend_loo_tile_kernels.hip for f64 and trend_loo_tile_f32_kernels.hip for f32) -- leave-one-out
// cross-validation of a GP with a linear trend (universal kriging) on the MFMA tile layout, n <= 96. With M = B + diag c (c optional),
// Kinv = M^-1, H = [h_1 .. h_K] the basis vectors (K = nbasis <= 16), A = H^T Kinv H, P = Kinv - Kinv H A^-1 H^T Kinv, D targets y_t and
// alpha_t = P y_t, Dubrule's identities (the zero-mean formulas of loo_tile_impl.hpp with P in place of Kinv):
//     var[i] = 1 / P_ii        mean[t][i] = y_ti - alpha_ti / P_ii        logpl[t] = sum_i (1/2 log P_ii - 1/2 alpha_ti^2 / P_ii) - n/2 log 2 pi
// The load, the PanelSolve pipeline and the block-step loop are those of trend_grad_tile_body (trend_grad_tile_impl.hpp), copied once more
// so that every earlier kernel compiles to what it compiled to before; the pivot product is left out (no output holds a log-determinant). A copy of spd_load_lower and
// spd_full_sweep (spd_sweep.hpp) as it stands: called from the shared header these forms pair their LDS stores differently and spill more
// SGPRs into VGPR lanes ("The shared SPD sweep"); a change to the sweep is made there and here.
// The sweep ends with W = -Kinv in the lower tiles. Phase 1 of trend_grad_tile_body follows without its logml and beta stores: H staged,
// T_H = W H parked in hq, A factored by the wave with the quotient update, L^-1 in its 16 x 17 LDS tile. Then, new here:
//   1. U = T_H L^-T on the MFMA unit, 4 MFMAs per tile row (step 2a of trend_grad_tile_body), kept in registers: hq still holds T_H for the
//      target loop. Lane (q, c) holds U[16 ti + trow(r, q)][b = c]; its square is summed over the 16 c lanes by DPP (dpp_row_sum16), no
//      ds_bpermute round trip. Only the diagonal of U U^T = Kinv H A^-1 H^T Kinv is ever formed.
//   2. P_ii = -W_ii - sum_b U_ib^2 by the one lane that holds the diagonal element of tile (t, t), as in loo_tile_body, into the tile t0
//      (free once A is factored). 1 / P_ii and 1/2 log P_ii are computed once per index and kept in t0; the same lanes write var as
//      contiguous runs. P_ii not > 0 (or NaN) for a real index feeds a wave-uniform flag through a ballot.
//   3. per group of 16 targets: T_g = W Y_g, -beta, T_g += T_H (-beta) = -alpha exactly as trend_tile_body; in registers
//      mu = y + T_g / P_ii and the lane's share of sum_i (1/2 log P_ii - 1/2 alpha^2 / P_ii): four chains by register r over the tile rows,
//      ((p0 + p1) + (p2 + p3)), the four q groups by two __shfl_xor (dot_t of trend_tile_body). mean leaves through the group buffer aq, so
//      that consecutive lanes store consecutive i (the alpha store of trend_tile_body).
// Every loop over the basis runs over all 16 slots in a fixed order; nothing in the order of operations of an output depends on batch, grid,
// D, or the group or lane of a target; which outputs are stored is decided by wave-uniform pointers. var depends on M and H only; Y is read
// only with mean or logpl.
// HBM traffic per matrix: n^2 / 2 + n + K n + D n elements in, n + D n + D out.
// info: the 1-based column of the first non-positive (or NaN) pivot of M (PanelSolve::binfo; fp32: the natural-order redo); else n + b
// for the first non-positive (or NaN) pivot b of A; else n + K + i for the first point i (1-based) whose computed P_ii is not > 0. Any of
// them makes every requested output of the matrix NaN: no fallback launch. A tiny positive P_ii is returned as it is (a huge variance).
//
// The kernels are overloads of matinv_spd_tile_f64 / _f32 with twelve more trailing template arguments ("Leave-one-out
// cross-validation of the trend model").
#pragma once
#include "trend_grad_tile_impl.hpp"  // TREND_TS, the launch bounds of the trend forms, dpp_row_sum16
#include "loo_tile_impl.hpp"         // loo_log

namespace matinv {

// Epilogue layout (lane l = 16 q + c; the lane holds W[16 ti + trow(r, q)][16 tj + c] in acc[ti][tj][r], tj <= ti):
//   LDS: panel[4 N] (the sweep's, the panel of each block step again in every build_t), aq[16 (N + 1)] = the 16 vectors of ONE group (basis,
//        targets, then mean), vector j at aq + j (N + 1), zero beyond n and beyond the group; hq[16 (N + 1)] = T_H, vector b at
//        hq + b (N + 1); three 16 x 17 tiles: t0 = A while it is factored, then P_ii at t0 + i on its way to 1 / P_ii at t0 + i and
//        1/2 log P_ii at t0 + N + i (2 N <= 192 of its 272 elements); t2 = L^-1; t3 = -beta of the current target group.
template <class T, int NT, bool FULL>
__device__ __forceinline__ void trend_loo_tile_body(const T *Bs, const T *Cs, const T *Hs, const T *Ys, int nbasis, int ntarget, T *Mn, T *Vr,
                                                    T *Lp, int *info, int n_rt, unsigned batch, T *panel, T *aq, T *hq, T *sm)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    constexpr int N = 16 * NT;
    constexpr int NKB = 4 * NT;
    constexpr int NS = predict_qstride(N);
    constexpr int TS = TREND_TS;
    static_assert(2 * N <= 16 * TS, "1 / P_ii and 1/2 log P_ii share the tile A was factored in");
    typedef PanelSolve<NT, true, T> PS;
    const int l = threadIdx.x;
    T *const t0 = sm, *const t2 = sm + 16 * TS, *const t3 = sm + 32 * TS;

    for (unsigned mat = blockIdx.x; mat < batch; mat += gridDim.x) {
        int n = FULL ? N : n_rt;  // run-time n opaque once per matrix, predicates on the edge tiles only: see gj_tile_body
        if (!FULL) asm volatile("" : "+s"(n));
        const T *A = Bs + (size_t)mat * n * n;
        int q = l >> 4, c = l & 15;
        asm volatile("" : "+v"(q), "+v"(c));  // see matinv_gj_tile_f64

        // W = A^T tile layout, lower tiles only; in the diagonal tiles the strictly upper elements come from their mirror position,
        // so only the lower triangle of B is ever read (spd_tile_body)
        vec4 acc[NT][NT];
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
                    T v = in ? A[(unsigned)(lo * n + hi)] : ((row == col) ? (T)1 : (T)0);
                    if (Cs && ti == tj && row == col && in) v += Cs[(size_t)mat * n + row];
                    acc[ti][tj][r] = v;
                }
            }
        unsigned long long bad = 0;
        int binfo = 0;  // column of the first non-positive pivot + 1
        T aop[NT], bop[NT];

        spd_panel_to_lds<NT, T>(panel, acc, 0, q, c);
        wave_lds_sync();
        {
            PS ps0;
            ps0.binfo = &binfo;
#pragma unroll
            for (int s = 0; s < PS::NSTAGE; ++s) ps0.stage(s, panel, 0, q, c, aop, bop, bad);
        }
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            // ragged n: a block step over four columns of identity padding only touches padding -- skipped (as in gj_tile_body)
            if (!FULL && kb > 4 * (NT - 1) && kb - 4 * (NT - 1) >= G::real_blocks(n - 16 * (NT - 1))) continue;
            spd_prep_operands<NT, T>(acc, bop, kb, q, c);
            if (kb + 1 < NKB) {
                const int tn = (kb + 1) >> 2;
                // (a) the tiles the next panel is read from: column tn (ti >= tn) and row tn (tj < tn)
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) {
                    if (ti < tn) continue;
                    acc[ti][tn] = G::mfma(aop[ti], bop[tn], acc[ti][tn]);
                }
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) {
                    if (tj >= tn) continue;
                    acc[tn][tj] = G::mfma(aop[tn], bop[tj], acc[tn][tj]);
                }
                // (b) the other lower tiles, pinned between the pieces of the next panel: 2 MFMAs cover the latency of (a), then the
                //     panel is staged, then the remaining MFMAs are spread evenly over the solve stages (counters fold to literals)
                constexpr int NB = NT * (NT + 1) / 2 - NT;
                constexpr int NSG = PS::NSTAGE;
                T aop_next[NT], bop_next[NT];
                PS ps;
                ps.binfo = &binfo;
                int count = 0, ev = 0;  // MFMAs of (b) issued so far; next event (0 = stage the panel, 1 + s = stage s)
                auto run_events = [&](bool flush) {
#pragma unroll
                    for (int e = 0; e < NSG + 1; ++e) {
                        const int lead = NB < 2 ? NB : 2;
                        const int thr = (e == 0) ? lead : lead + ((NB - lead) * e) / NSG;
                        if (e == ev && (flush || thr <= count)) {
                            __builtin_amdgcn_sched_barrier(0);
                            if (e == 0) {
                                wave_lds_sync();
                                spd_panel_to_lds<NT, T>(panel, acc, kb + 1, q, c);
                                wave_lds_sync();
                            } else {
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
                        if (tj > ti || ti == tn || tj == tn) continue;
                        acc[ti][tj] = G::mfma(aop[ti], bop[tj], acc[ti][tj]);
                        ++count;
                        run_events(false);
                    }
                run_events(true);
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) { aop[ti] = aop_next[ti]; bop[ti] = bop_next[ti]; }
            } else {
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int tj = 0; tj < NT; ++tj) {
                        if (tj > ti) continue;
                        acc[ti][tj] = G::mfma(aop[ti], bop[tj], acc[ti][tj]);
                    }
            }
        }

        // ---- epilogue: W = -M^-1 in the lower tiles ------------------------------------------------------------------------------
        // the group buffer takes 16 vectors of n elements, consecutive lanes on consecutive elements of one vector, zero beyond n and
        // beyond the `left` vectors there are
        auto stage = [&](const T *src, int left, int ns, int ls) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < N / 4; ++k) {
                const int e = ls + 64 * k, j = e / N, i = e - j * N;
                const bool in = (FULL || i < ns) && j < left;
                aq[j * NS + i] = in ? src[(unsigned)(j * ns + i)] : (T)0;
            }
        };
        // T = W X for the group X in the buffer: lane (q, c) ends with T[16 ti + trow(r, q)][vector c] in tq[ti][r]
        auto build_t = [&](vec4(&tq)[NT], int ns, int qs, int cs) __attribute__((always_inline)) {
            const T *const xc = aq + cs * NS;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) tq[ti][r] = (T)0;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                // the block steps the sweep skipped hold identity padding, and the vectors are zero there
                if (!FULL && kb > 4 * (NT - 1) && kb - 4 * (NT - 1) >= G::real_blocks(ns - 16 * (NT - 1))) continue;
                const int tK = kb >> 2, rK = kb & 3;
                wave_lds_sync();
                spd_panel_to_lds<NT, T>(panel, acc, kb, qs, cs);
                wave_lds_sync();
                const T b = xc[16 * tK + G::pcol(rK, qs)];
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) tq[ti] = G::mfma(panel[(16 * ti + cs) * 4 + qs], b, tq[ti]);
            }
        };
        // C = X^T T, X the group in the buffer: lane (q, c) ends with C[r] = x_j^T T[:, c], j = trow(r, q) (predict_cov_tile_body)
        auto block_t = [&](const vec4(&tq)[NT], vec4 cb, int qs, int cs) __attribute__((always_inline)) -> vec4 {
            const T *const xr = aq + cs * NS;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) cb = G::mfma(xr[16 * ti + G::trow(r, qs)], tq[ti][r], cb);
            return cb;
        };
        // C = T_H^T X, both from LDS: lane (q, c) ends with C[r] = -(H^T Kinv x_c)[b], b = trow(r, q)
        auto block_h = [&](int qs, int cs) __attribute__((always_inline)) -> vec4 {
            const T *const hr = hq + cs * NS, *const xc = aq + cs * NS;
            vec4 cb;
#pragma unroll
            for (int r = 0; r < 4; ++r) cb[r] = (T)0;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * ti + G::trow(r, qs);
                    cb = G::mfma(hr[i], xc[i], cb);
                }
            return cb;
        };

        // ---- H, T_H = W H to hq, A = -H^T T_H to t0 (trend_tile_body, steps 1 and 2) ---------------------------------------------
        int abad = 0;  // pivot of A that fails first, 1-based (wave-uniform)
        {
            int nh = n, lh = l, qh = q, ch = c;
            if (!FULL) asm volatile("" : "+s"(nh));
            asm volatile("" : "+v"(lh), "+v"(qh), "+v"(ch));
            wave_lds_sync();  // the sweep's last reads of the panel; the previous matrix's reads of every buffer
            stage(Hs + (size_t)mat * nbasis * nh, nbasis, nh, lh);
            wave_lds_sync();
            vec4 tq[NT];
            build_t(tq, nh, qh, ch);
            vec4 cb;
#pragma unroll
            for (int r = 0; r < 4; ++r) cb[r] = (T)0;
            cb = block_t(tq, cb, qh, ch);
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) hq[ch * NS + 16 * ti + G::trow(r, qh)] = tq[ti][r];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int bp = G::trow(r, qh);
                t0[bp * TS + ch] = (bp == ch && bp >= nbasis) ? (T)1 : -cb[r];  // W = -Kinv; identity diagonal beyond K
            }
            // ---- A = L L^T in LDS, right-looking, the lower triangle only, and L^-1 with it (trend_tile_body, step 3): the rolled loop,
            // the unscaled column and the IEEE quotient A[jj][j] / d, so that a basis vector that repeats an earlier one bit for bit gets a
            // pivot of exactly 0 and the code matinv_trend_batched reports
#pragma unroll
            for (int m = 0; m < 4; ++m) t2[(qh + 4 * m) * TS + ch] = (qh + 4 * m == ch) ? (T)1 : (T)0;
#pragma unroll 1
            for (int j = 0; j < nbasis; ++j) {
                wave_lds_sync();
                const T d = t0[j * TS + j];
                if (!(d > (T)0) && abad == 0) abad = j + 1;
                T sd, rs;
                sqrt_and_rsqrt(d, sd, rs);
                const T aij = t0[ch * TS + j];  // A[c][j] of the trailing matrix
                const T xj = t2[j * TS + ch] * rs;   // X[j][c], final
                if (qh == (j & 3)) t2[j * TS + ch] = xj;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int jj = qh + 4 * m;  // a column of the trailing matrix, and a row of X
                    if (jj > j) {
                        const T ajj = t0[jj * TS + j];  // A[jj][j] of the trailing matrix = L[jj][j] L[j][j]
                        if (ch >= jj) t0[ch * TS + jj] = fma_t(-aij, ajj / d, t0[ch * TS + jj]);
                        t2[jj * TS + ch] = fma_t(-(ajj * rs), xj, t2[jj * TS + ch]);
                    }
                }
            }
            wave_lds_sync();
        }
        // z = L^-1 v for the 16 x 16 block v in the accumulator layout (lane (q, c): v[trow(r, q)][c] in register r, which is the
        // B operand of an MFMA whose k index runs over trow(r, q)); the result in the same layout
        auto linv_mul = [&](vec4 v, int qs, int cs) __attribute__((always_inline)) -> vec4 {
            vec4 z;
#pragma unroll
            for (int r = 0; r < 4; ++r) z[r] = (T)0;
#pragma unroll
            for (int r = 0; r < 4; ++r) z = G::mfma(t2[cs * TS + G::trow(r, qs)], v[r], z);
            return z;
        };
        // L^-T z, likewise
        auto linvt_mul = [&](vec4 v, int qs, int cs) __attribute__((always_inline)) -> vec4 {
            vec4 z;
#pragma unroll
            for (int r = 0; r < 4; ++r) z[r] = (T)0;
#pragma unroll
            for (int r = 0; r < 4; ++r) z = G::mfma(t2[G::trow(r, qs) * TS + cs], v[r], z);
            return z;
        };

        // ---- the diagonal of P: U = T_H L^-T in registers, its row sums of squares by DPP, P_ii = -W_ii - sum_b U_ib^2 ------------
        T *const rp = t0, *const hl = t0 + N;  // 1 / P_ii and 1/2 log P_ii; A has been factored and t0 is free
        int pbad = 0;                          // first point whose P_ii is not > 0, 1-based (wave-uniform)
        {
            // lane (q, c) supplies T_H[16 ti + c][4 kk + q] as the A operand and L^-T[4 kk + q][c] = L^-1[c][4 kk + q] as the B operand,
            // and ends with U[16 ti + trow(r, q)][c]; its columns beyond K are exact zeros (T_H is zero there, L^-1 the identity)
            int nu = n, lu = l, qu = q, cu = c;
            if (!FULL) asm volatile("" : "+s"(nu));
            asm volatile("" : "+v"(lu), "+v"(qu), "+v"(cu));
            vec4 uq[NT];
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) uq[ti][r] = (T)0;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const T lt = t2[cu * TS + 4 * kk + qu];
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) uq[ti] = G::mfma(hq[(4 * kk + qu) * NS + 16 * ti + cu], lt, uq[ti]);
            }
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const T s = dpp_row_sum16(uq[ti][r] * uq[ti][r]);
                    if (G::trow(r, qu) == cu) t0[16 * ti + cu] = -acc[ti][ti][r] - s;  // the one lane that holds W_ii
                }
            wave_lds_sync();
            // once per index: the check, 1 / P_ii, 1/2 log P_ii. Index i is read and written by the same lane.
            constexpr int NR = (N + 63) / 64;
            T pv[NR];
            unsigned long long neg[NR];
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                const int i = lu + 64 * k;
                pv[k] = i < N ? t0[i] : (T)1;
                neg[k] = __ballot(i < N && (FULL || i < nu) && !(pv[k] > (T)0));
            }
#pragma unroll
            for (int k = NR - 1; k >= 0; --k)
                if (neg[k]) pbad = 64 * k + (int)__builtin_ctzll(neg[k]) + 1;
            const bool okv = bad == 0 && abad == 0 && pbad == 0;
#pragma unroll
            for (int k = 0; k < NR; ++k) {
                const int i = lu + 64 * k;
                const T rk = (T)1 / pv[k];
                if (i < N) {
                    rp[i] = rk;
                    hl[i] = (T)0.5 * loo_log(pv[k]);
                    if (Vr && (FULL || i < nu)) Vr[(size_t)mat * nu + i] = okv ? rk : nan_of<T>();  // wave-uniform pointer
                }
            }
            wave_lds_sync();
        }
        const bool ok = bad == 0 && abad == 0 && pbad == 0;

        // ---- the targets in groups of 16 (trend_tile_body, step 5) --------------------------------------------------------------------
        const int ngroups = (Mn || Lp) ? (ntarget + 15) >> 4 : 0;  // wave-uniform; the targets are not read otherwise
        for (int g = 0; g < ngroups; ++g) {
            int ng = n, lg = l, qg = q, cg = c;
            if (!FULL) asm volatile("" : "+s"(ng));
            asm volatile("" : "+v"(lg), "+v"(qg), "+v"(cg));
            const int left = ntarget - 16 * g;  // targets from this group's first on
            const size_t first = (size_t)mat * ntarget + 16 * (size_t)g;
            wave_lds_sync();  // the previous group's reads of the buffer, of the panel and of the tiles
            stage(Ys + first * ng, left, ng, lg);
            wave_lds_sync();
            T *const yc = aq + cg * NS;  // the vector of this lane's target
            vec4 tq[NT];
            build_t(tq, ng, qg, cg);
            {
                // -(H^T Kinv y_c)[trow(r, q)], then -beta = L^-T (L^-1 of it), every step a 16 x 16 x 16 product on the MFMA unit
                const vec4 nb4 = linvt_mul(linv_mul(block_h(qg, cg), qg, cg), qg, cg);
#pragma unroll
                for (int r = 0; r < 4; ++r) t3[G::trow(r, qg) * TS + cg] = nb4[r];
                wave_lds_sync();
            }
            // T_g <- T_g - T_H beta = W (y - H beta) = -alpha
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const T nb = t3[(4 * kk + qg) * TS + cg];
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) tq[ti] = G::mfma(hq[(4 * kk + qg) * NS + 16 * ti + cg], nb, tq[ti]);
            }
            // mu = y + T_g / P_ii in place of T_g, and the lane's share of sum_i (1/2 log P_ii - 1/2 alpha^2 / P_ii); a row of identity
            // padding holds y = alpha = 0 and P = 1 and is left out of the sum
            T part[4] = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * ti + G::trow(r, qg);
                    const bool in = FULL || ti < NT - 1 || i < ng;
                    const T na = tq[ti][r], w = na * rp[i];  // -alpha, -alpha / P_ii
                    if (in) part[r] += fma_t((T)-0.5 * na, w, hl[i]);
                    tq[ti][r] = yc[i] + w;
                }
            T s = (part[0] + part[1]) + (part[2] + part[3]);
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            // 1/2 log 2 pi
            if (Lp && qg == 0 && cg < left) Lp[first + cg] = ok ? fma_t(-(T)ng, (T)0.91893853320467274178, s) : nan_of<T>();
            if (Mn) {             // wave-uniform
                wave_lds_sync();  // the targets have been read: the buffer takes the group's mean, vector by vector
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) yc[16 * ti + G::trow(r, qg)] = ok ? tq[ti][r] : nan_of<T>();
                wave_lds_sync();
                // opaque once more (multi_target_tile_body)
                int na = ng, la = lg;
                if (!FULL) asm volatile("" : "+s"(na));
                asm volatile("" : "+v"(la));
                T *Mg = Mn + first * na;
#pragma unroll
                for (int k = 0; k < N / 4; ++k) {
                    const int e = la + 64 * k, j = e / N, i = e - j * N;
                    if ((FULL || i < na) && j < left) Mg[(unsigned)(j * na + i)] = aq[j * NS + i];
                }
            }
        }
        int code = binfo;
        if constexpr (sizeof(T) == 4) {
            if (bad != 0) {  // wave-uniform; rejected matrices only: the fp32 tile order does not say which column fails FIRST (tile_common.hpp)
                wave_lds_sync();  // the last reads of the panel
                const int nat = spd_natural_first_failure<NT, T>(A, Cs ? Cs + (size_t)mat * n : nullptr, n, panel, l);
                if (nat) code = nat;
            }
        }
        if (bad == 0 && abad != 0) code = n + abad;
        if (bad == 0 && abad == 0 && pbad != 0) code = n + nbasis + pbad;
        if (l == 0 && info) info[mat] = code;
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// The leave-one-out forms of the trend kernels: matinv_spd_tile_f64 / matinv_spd_tile_f32 with a third to a fourteenth template argument,
// under the launch bounds of the trend forms of the same NT (trend_tile_impl.hpp): the live set of the target loop is theirs, and the
// diagonal of P holds NT blocks of U beside the accumulators, fewer registers than the target loop. One form spills under them and takes
// one wave per SIMD less: the ragged fp64 5 x 5 (53 registers, 120 bytes of scratch at two waves), as its trend gradient form does. With
// that no form uses scratch and no fp32 form uses an AGPR: profiles/trend_loo_kernel_registers.txt.
constexpr int trend_loo_f64_waves(int nt, bool full) { return trend_f64_waves(nt, full) - ((nt == 5 && !full) ? 1 : 0); }

#define MATINV_TREND_LOO_ARGS                                                                                                             \
    LOO &&GRAD &&PREDICT &&COV &&LOOGRAD &&COLOUR &&WHITEN &&MULTI &&MTGRAD &&TREND &&TRENDGRAD &&TRENDLOO

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD,
          bool TREND, bool TRENDGRAD, bool TRENDLOO>
__global__ __launch_bounds__(64, trend_loo_f64_waves(NT, FULL)) void matinv_spd_tile_f64(const double *Bs, const double *Cs, const double *Hs,
                                                                                              const double *Ys, int nbasis, int ntarget,
                                                                                              double *Mn, double *Vr, double *Lp, int *info,
                                                                                              int n_rt, unsigned batch)
{
    static_assert(MATINV_TREND_LOO_ARGS, "the fourteen-argument form is the trend leave-one-out kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    __shared__ double aq[16 * predict_qstride(16 * NT)];
    __shared__ double hq[16 * predict_qstride(16 * NT)];
    __shared__ double sm[48 * TREND_TS];
    trend_loo_tile_body<double, NT, FULL>(Bs, Cs, Hs, Ys, nbasis, ntarget, Mn, Vr, Lp, info, n_rt, batch, panel, aq, hq, sm);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD,
          bool TREND, bool TRENDGRAD, bool TRENDLOO>
__global__ __launch_bounds__(64, trend_f32_waves(NT, FULL)) void matinv_spd_tile_f32(const float *Bs, const float *Cs, const float *Hs,
                                                                                          const float *Ys, int nbasis, int ntarget, float *Mn,
                                                                                          float *Vr, float *Lp, int *info, int n_rt,
                                                                                          unsigned batch)
{
    static_assert(MATINV_TREND_LOO_ARGS, "the fourteen-argument form is the trend leave-one-out kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    __shared__ float aq[16 * predict_qstride(16 * NT)];
    __shared__ float hq[16 * predict_qstride(16 * NT)];
    __shared__ float sm[48 * TREND_TS];
    trend_loo_tile_body<float, NT, FULL>(Bs, Cs, Hs, Ys, nbasis, ntarget, Mn, Vr, Lp, info, n_rt, batch, panel, aq, hq, sm);
}
#undef MATINV_TREND_LOO_ARGS

template <class T>
hipError_t launch_trend_loo_tile(int n, int nbasis, int ntarget, const T *Bs, const T *Cs, const T *Hs, const T *Ys, T *Mn, T *Vr, T *Lp,
                                 size_t batch, int *info, hipStream_t stream)
{
    if (!trend_loo_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = predict_tile_grid(batch), b = (unsigned)batch;  // the grid of the trend launcher
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true, true, true, true, true, true, true, true, true, true, true>),
                               dim3(grid), dim3(64), 0, stream, Bs, Cs, Hs, Ys, nbasis, ntarget, Mn, Vr, Lp, info, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true, true, true, true, true, true, true, true, true, true, true>),
                               dim3(grid), dim3(64), 0, stream, Bs, Cs, Hs, Ys, nbasis, ntarget, Mn, Vr, Lp, info, n, b);
    });
    return hipGetLastError();
}
}  // namespace matinv
