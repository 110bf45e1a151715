// trend_grad_tile_impl.hpp (instantiated by trend_grad_tile_kernels.hip for f64 and trend_grad_tile_f32_kernels.hip for f32) -- gradients
// of the restricted (REML) log marginal likelihood of a GP with a linear trend on the MFMA tile layout, n <= 96. With M = B + diag c
// (c optional), Kinv = M^-1, H = [h_1 .. h_K] the basis vectors (K = nbasis <= 16), A = H^T Kinv H, P = Kinv - Kinv H A^-1 H^T Kinv, D
// targets y_t, alpha_t = P y_t and P' symmetric derivative matrices dM_p:
//     G = sum_t alpha_t alpha_t^T - D P      grad[p] = 1/2 sum_ij G_ij dM_p[i][j]      gradc[i] = 1/2 G_ii
//     logml_t = -1/2 (y_t^T alpha_t + log det M + log det A + (n - K) log 2 pi)    alpha[t] = alpha_t    beta[t] = A^-1 H^T Kinv y_t
// the gradient of sum_t logml_t of matinv_trend_batched with respect to the parameter behind dM_p and to c_i (H does not depend on
// either). The load, the PanelSolve pipeline, the block-step loop and the pivot fold are those of trend_tile_body (trend_tile_impl.hpp),
// copied once more so that every earlier kernel compiles to what it compiled to before. A copy of spd_load_lower and
// spd_full_sweep (spd_sweep.hpp) as it stands: called from the shared header these forms pair their LDS stores differently and spill more
// SGPRs into VGPR lanes ("The shared SPD sweep"); a change to the sweep is made there and here. The sweep ends with W = -Kinv in the lower
// tiles. The epilogue has two phases:
//   1. trend_tile_body's without queries and without covbeta: H staged, T_H = W H parked in hq, A factored by the wave with the quotient
//      update, L^-1 in a 16 x 17 LDS tile, log det A through a PivotProduct; per group of 16 targets T_g = W Y_g, -beta,
//      T_g += T_H (-beta) = -alpha, then logml, beta and alpha out. The instructions and the reduction order are trend's, so logml, alpha
//      and beta carry the bits of matinv_trend_batched for the same inputs.
//   2. (grad or gradc asked for) after the last target group, when T_H is no longer needed intact:
//      a. U = T_H L^-T on the MFMA unit, 4 MFMAs per tile row: the A operand from hq, L^-T from its tile. U U^T = Kinv H A^-1 H^T Kinv
//         whatever the sign of T_H. U goes back over hq; its columns beyond K are exact zeros (T_H is zero there and L^-1 is the
//         identity there).
//      b. acc[ti][tj] += U[ti] U[tj]^T, four 16 x 16 x 4 MFMAs per lower tile, read from hq as multi_target_grad_tile_body reads alpha_g
//         from the group buffer: the accumulators hold W + U U^T = -P.
//      c. acc <- D acc, then acc[ti][tj] += alpha_g[ti] alpha_g[tj]^T group by group, exactly as multi_target_grad_tile_body: with
//         D <= 16 out of the group buffer, with more from dAlpha when that is asked for and from a library workspace of D n elements
//         per workgroup otherwise. Both hold the same values and are read in the same order: asking for alpha changes no bit of grad.
//      d. the weights (1/2 in the diagonal tiles, 1 below), gradc out of the diagonal tiles through the panel buffer, and the per-p
//         contraction of logml_grad_tile_body as it stands: each dM_p is read once per matrix whatever D and K are.
// Nothing in the order of operations depends on batch, grid or P; which outputs are stored is decided by wave-uniform pointers.
// HBM traffic per matrix: n^2 / 2 + n + K n + D n + P n^2 / 2 elements in, P + n + D + D n + D K out; D > 16: D n more, out and back in
// through L2.
// info: the 1-based column of the first non-positive (or NaN) pivot of M (PanelSolve::binfo; fp32: the natural-order redo); else n + b
// for the first non-positive (or NaN) pivot b of A. Either makes every requested output of the matrix NaN: no fallback launch.
//
// The kernels are overloads of matinv_spd_tile_f64 / _f32 with eleven more trailing template arguments ("Gradients of the
// restricted log marginal likelihood").
#pragma once
#include "trend_tile_impl.hpp"              // TREND_TS, the launch bounds of the trend forms
#include "multi_target_grad_tile_impl.hpp"  // the launch bounds of the multi-target gradient forms, dpp_row_sum16

namespace matinv {

// Epilogue layout (lane l = 16 q + c; the lane holds W[16 ti + trow(r, q)][16 tj + c] in acc[ti][tj][r], tj <= ti):
//   LDS: panel[4 N] (the sweep's, the panel of each block step again in phase 1, gradc on its way out in phase 2), aq[16 (N + 1)] = the
//        16 vectors of ONE group (basis, targets, then alpha), vector j at aq + j (N + 1), zero beyond n and beyond the group;
//        hq[16 (N + 1)] = T_H in phase 1, U in phase 2, vector b at hq + b (N + 1); three 16 x 17 tiles: t0 = A while it is factored,
//        t2 = L^-1, t3 = -beta of the current target group.
//   abase: where the alpha of this matrix is stored: dAlpha, else the workgroup's slice of the workspace (D > 16 only), else nowhere.
template <class T, int NT, bool FULL>
__device__ __forceinline__ void trend_grad_tile_body(const T *Bs, const T *Cs, const T *Hs, const T *Ys, const T *dMs, int nbasis,
                                                     int ntarget, int nparam, T *grad, T *gradc, T *Lm, T *Al, T *Be, T *ws, int *info,
                                                     int n_rt, unsigned batch, T *panel, T *aq, T *hq, T *sm)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    constexpr int N = 16 * NT;
    constexpr int NKB = 4 * NT;
    constexpr int NS = predict_qstride(N);
    constexpr int TS = TREND_TS;
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
        PivotProduct<T> prod;
        T aop[NT], bop[NT];

        spd_panel_to_lds<NT, T>(panel, acc, 0, q, c);
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
                                // the pivots of step kb + 1 are complete after stage 3 (logdet_tile_body); a step of identity padding
                                // that the next iteration skips folds four exact ones
                                if (e - 1 == 3) prod.fold(ps.d[0][0], ps.u11, ps.u22, ps.u33);
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
        const T ld = prod.log_value();

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
        // s_c = sum_i T[i][c] x_c[i] over the group in the buffer: four chains by register r, ((p0 + p1) + (p2 + p3)), the four q groups
        // by two __shfl_xor (multi_target_tile_body)
        auto dot_t = [&](const vec4(&tq)[NT], int qs, int cs) __attribute__((always_inline)) -> T {
            const T *const xc = aq + cs * NS;
            T part[4] = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) part[r] = fma_t(tq[ti][r], xc[16 * ti + G::trow(r, qs)], part[r]);
            T s = (part[0] + part[1]) + (part[2] + part[3]);
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            return s;
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

        // ---- 1, 2: H, T_H = W H to hq, A = -H^T T_H to t0 ---------------------------------------------------------------------
        int abad = 0;  // pivot of A that fails first, 1-based (wave-uniform)
        T ldA;
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
            // ---- 3: A = L L^T in LDS, right-looking, the lower triangle only, and L^-1 with it: column-oriented forward substitution
            // on the identity, X[j][:] *= 1 / L_jj, X[i][:] -= L_ij X[j][:] for i > j. In the factorisation lane (q, c) serves row c
            // and the columns q, q + 4, q + 8, q + 12; in the substitution column c and the rows q, q + 4, q + 8, q + 12. The loop is
            // rolled (unrolled, its 16 steps held 70 more registers than the sweep) and ends at K: a step on the identity padding
            // would multiply by an exact 1 and subtract exact zeros.
            PivotProduct<T> prodA;
#pragma unroll
            for (int m = 0; m < 4; ++m) t2[(qh + 4 * m) * TS + ch] = (qh + 4 * m == ch) ? (T)1 : (T)0;
#pragma unroll 1
            for (int j = 0; j < nbasis; ++j) {
                wave_lds_sync();
                const T d = t0[j * TS + j];
                if (!(d > (T)0) && abad == 0) abad = j + 1;
                T sd, rs;
                sqrt_and_rsqrt(d, sd, rs);
                prodA.fold(d);
                const T aij = t0[ch * TS + j];  // A[c][j] of the trailing matrix
                const T xj = t2[j * TS + ch] * rs;   // X[j][c], final
                if (qh == (j & 3)) t2[j * TS + ch] = xj;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int jj = qh + 4 * m;  // a column of the trailing matrix, and a row of X
                    if (jj > j) {
                        const T ajj = t0[jj * TS + j];  // A[jj][j] of the trailing matrix = L[jj][j] L[j][j]
                        // the update with the unscaled column and the IEEE quotient A[jj][j] / d: a basis vector that repeats an
                        // earlier one bit for bit has A[jj][j] = d = A[jj][jj] bit for bit, the quotient is exactly 1 and its pivot
                        // exactly 0 -- reported, where fl(L^2) could land either side of d
                        if (ch >= jj) t0[ch * TS + jj] = fma_t(-aij, ajj / d, t0[ch * TS + jj]);
                        t2[jj * TS + ch] = fma_t(-(ajj * rs), xj, t2[jj * TS + ch]);
                    }
                }
            }
            wave_lds_sync();
            ldA = prodA.log_value();
        }
        const bool ok = bad == 0 && abad == 0;
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

        // ---- phase 1: the targets in groups of 16 (trend_tile_body) -----------------------------------------------------------------
        const bool second = grad || gradc;        // wave-uniform
        const int ngroups = (ntarget + 15) >> 4;  // wave-uniform; every output needs the targets
        T *const abase = Al ? Al + (size_t)mat * ntarget * n : (ws ? ws + (size_t)blockIdx.x * ntarget * n : nullptr);
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
            if (Be) {  // wave-uniform; the group's beta is a run of 16 K elements (fewer in the last group)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int f = lg + 64 * k, tt = f / nbasis, b = f - tt * nbasis;
                    if (f < 16 * nbasis && tt < left) Be[first * nbasis + f] = ok ? -t3[b * TS + tt] : nan_of<T>();
                }
            }
            // T_g <- T_g - T_H beta = W (y - H beta) = -alpha
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const T nb = t3[(4 * kk + qg) * TS + cg];
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) tq[ti] = G::mfma(hq[(4 * kk + qg) * NS + 16 * ti + cg], nb, tq[ti]);
            }
            {
                const T s = dot_t(tq, qg, cg);
                if (qg == 0 && cg < left) {
                    const T qd = -s;  // W = -Kinv
                    // log 2 pi
                    if (Lm)
                        Lm[first + cg] = ok ? (T)-0.5 * fma_t((T)(ng - nbasis), (T)1.83787706640934548356, qd + (ld + ldA)) : nan_of<T>();
                }
            }
            if (Al || second) {   // wave-uniform
                wave_lds_sync();  // the targets have been read: the buffer takes the group's alpha, vector by vector
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) yc[16 * ti + G::trow(r, qg)] = ok ? -tq[ti][r] : nan_of<T>();
                wave_lds_sync();
                if (abase) {  // wave-uniform
                    // opaque once more (multi_target_tile_body)
                    int na = ng, la = lg;
                    if (!FULL) asm volatile("" : "+s"(na));
                    asm volatile("" : "+v"(la));
                    T *Ag = abase + 16 * (size_t)g * na;
#pragma unroll
                    for (int k = 0; k < N / 4; ++k) {
                        const int e = la + 64 * k, j = e / N, i = e - j * N;
                        if ((FULL || i < na) && j < left) Ag[(unsigned)(j * na + i)] = aq[j * NS + i];
                    }
                }
            }
        }

        // ---- phase 2: G = sum_t alpha_t alpha_t^T + D (W + U U^T) in place of W, weighted; gradc and the contraction ----------------
        if (second) {  // wave-uniform
            {
                // a. U = T_H L^-T: lane (q, c) supplies T_H[16 ti + c][4 kk + q] as the A operand and L^-T[4 kk + q][c] = L^-1[c][4 kk + q]
                //    as the B operand, and ends with U[16 ti + trow(r, q)][c], which goes where T_H[..][c] was
                int qu = q, cu = c;
                asm volatile("" : "+v"(qu), "+v"(cu));
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
                wave_lds_sync();  // every lane has read T_H
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) hq[cu * NS + 16 * ti + G::trow(r, qu)] = uq[ti][r];
                wave_lds_sync();
                // b. acc += U U^T: MFMA step s takes the columns 4 s ... 4 s + 3 of U; the same value is the A and the B operand
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    T op[NT];
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti) op[ti] = hq[(4 * s + qu) * NS + 16 * ti + cu];
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                        for (int tj = 0; tj <= ti; ++tj) acc[ti][tj] = G::mfma(op[ti], op[tj], acc[ti][tj]);
                }
            }
            // c. as multi_target_grad_tile_body from here on
            const T dscale = (T)ntarget;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj <= ti; ++tj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[ti][tj][r] *= dscale;
            if (ngroups > 1) {
                // this wavefront's stores of alpha have reached memory before it reads them back: a counter wait, no other workgroup
                // ever touches these addresses. This relies on the 64-thread launch: ONE wavefront per workgroup writes and reads its
                // own slice. A form with more wavefronts per workgroup needs a workgroup barrier here as well.
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
            for (int g = 0; g < ngroups; ++g) {
                int ng = n, lg = l, qg = q, cg = c;  // opaque once per group, for the reason given in phase 1
                if (!FULL) asm volatile("" : "+s"(ng));
                asm volatile("" : "+v"(lg), "+v"(qg), "+v"(cg));
                if (ngroups > 1) {  // wave-uniform: with one group its alpha is still in the buffer
                    const int left = ntarget - 16 * g;
                    const T *Sg = abase + 16 * (size_t)g * ng;
                    wave_lds_sync();  // the previous group's operand reads
#pragma unroll
                    for (int k = 0; k < N / 4; ++k) {
                        const int e = lg + 64 * k, j = e / N, i = e - j * N;
                        const bool in = (FULL || i < ng) && j < left;
                        aq[j * NS + i] = in ? Sg[(unsigned)(j * ng + i)] : (T)0;
                    }
                    wave_lds_sync();
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    T op[NT];
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti) op[ti] = aq[(4 * s + qg) * NS + 16 * ti + cg];
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                        for (int tj = 0; tj <= ti; ++tj) acc[ti][tj] = G::mfma(op[ti], op[tj], acc[ti][tj]);
                }
            }
            // d. the weights of logml_grad_tile_body: 1/2 in the diagonal tiles (both triangles stored), 1 in the strictly lower ones
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[ti][ti][r] *= (T)0.5;
            if (gradc) {  // wave-uniform
                wave_lds_sync();  // the last panel of phase 1 has been consumed
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (G::trow(r, q) == c) panel[16 * ti + c] = acc[ti][ti][r];  // the one lane that holds G_ii / 2
                wave_lds_sync();
#pragma unroll
                for (int k = 0; k < (N + 63) / 64; ++k) {
                    const int i = l + 64 * k;
                    if (i < N && (FULL || i < n)) gradc[(size_t)mat * n + i] = ok ? panel[i] : nan_of<T>();
                }
            }
            if (grad) {  // wave-uniform
                for (int p = 0; p < nparam; ++p) {
                    // lane coordinates and n opaque once per p (multi_target_grad_tile_body)
                    int np = n, qp = q, cp = c;
                    if (!FULL) asm volatile("" : "+s"(np));
                    asm volatile("" : "+v"(qp), "+v"(cp));
                    const T *D = dMs + ((size_t)mat * nparam + p) * np * np;
                    T part[4] = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti) {
#pragma unroll
                        for (int tj = 0; tj <= ti; ++tj) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int row = 16 * ti + G::trow(r, qp), col = 16 * tj + cp;
                                const bool in = FULL || ti < NT - 1 || (row < np && col < np);
                                const int hi = row > col ? row : col, lo = row > col ? col : row;
                                const T v = in ? D[(unsigned)(lo * np + hi)] : (T)0;  // beyond n: never issued, counts as 0
                                part[r] = fma_t(acc[ti][tj][r], v, part[r]);
                            }
                        }
                    }
                    T s = (part[0] + part[1]) + (part[2] + part[3]);
                    s = dpp_row_sum16(s);
                    s += __shfl_xor(s, 16);
                    s += __shfl_xor(s, 32);
                    if (l == 0) grad[(size_t)mat * nparam + p] = ok ? s : nan_of<T>();
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
        if (l == 0 && info) info[mat] = code;
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// The gradient forms of the trend kernels: matinv_spd_tile_f64 / matinv_spd_tile_f32 with a third to a thirteenth template argument.
// Launch bounds: the smaller of the trend form's and the multi-target gradient form's for the same NT (phase 1 has the live set of the
// first, phase 2 that of the second plus the NT blocks of U for a moment), one wave per SIMD fewer where a form does not fit them:
// profiles/trend_grad_kernel_registers.txt. No form uses scratch, and no fp32 form keeps MFMA operands in AGPRs.
constexpr int trend_grad_min(int a, int b) { return a < b ? a : b; }
constexpr int trend_grad_f64_waves(int nt, bool full)
{
    return trend_grad_min(trend_f64_waves(nt, full), multi_target_grad_f64_waves(nt, full));
}
constexpr int trend_grad_f32_waves(int nt, bool full) { return trend_grad_min(trend_f32_waves(nt, full), multi_target_f32_waves(nt, full)); }

#define MATINV_TREND_GRAD_ARGS                                                                                                             \
    LOO &&GRAD &&PREDICT &&COV &&LOOGRAD &&COLOUR &&WHITEN &&MULTI &&MTGRAD &&TREND &&TRENDGRAD

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD,
          bool TREND, bool TRENDGRAD>
__global__ __launch_bounds__(64, trend_grad_f64_waves(NT, FULL)) void matinv_spd_tile_f64(
    const double *Bs, const double *Cs, const double *Hs, const double *Ys, const double *dMs, int nbasis, int ntarget, int nparam,
    double *grad, double *gradc, double *Lm, double *Al, double *Be, double *ws, int *info, int n_rt, unsigned batch)
{
    static_assert(MATINV_TREND_GRAD_ARGS, "the thirteen-argument form is the trend gradient kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    __shared__ double aq[16 * predict_qstride(16 * NT)];
    __shared__ double hq[16 * predict_qstride(16 * NT)];
    __shared__ double sm[48 * TREND_TS];
    trend_grad_tile_body<double, NT, FULL>(Bs, Cs, Hs, Ys, dMs, nbasis, ntarget, nparam, grad, gradc, Lm, Al, Be, ws, info, n_rt, batch,
                                           panel, aq, hq, sm);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD,
          bool TREND, bool TRENDGRAD>
__global__ __launch_bounds__(64, trend_grad_f32_waves(NT, FULL)) void matinv_spd_tile_f32(
    const float *Bs, const float *Cs, const float *Hs, const float *Ys, const float *dMs, int nbasis, int ntarget, int nparam, float *grad,
    float *gradc, float *Lm, float *Al, float *Be, float *ws, int *info, int n_rt, unsigned batch)
{
    static_assert(MATINV_TREND_GRAD_ARGS, "the thirteen-argument form is the trend gradient kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    __shared__ float aq[16 * predict_qstride(16 * NT)];
    __shared__ float hq[16 * predict_qstride(16 * NT)];
    __shared__ float sm[48 * TREND_TS];
    trend_grad_tile_body<float, NT, FULL>(Bs, Cs, Hs, Ys, dMs, nbasis, ntarget, nparam, grad, gradc, Lm, Al, Be, ws, info, n_rt, batch,
                                          panel, aq, hq, sm);
}
#undef MATINV_TREND_GRAD_ARGS

template <class T>
hipError_t launch_trend_grad_tile(int n, int nbasis, int ntarget, int nparam, const T *Bs, const T *Cs, const T *Hs, const T *Ys,
                                  const T *dMs, T *grad, T *gradc, T *Lm, T *Al, T *Be, size_t batch, int *info, hipStream_t stream)
{
    if (!trend_grad_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    unsigned grid = predict_tile_grid(batch);  // the grid of the multi-target launcher
    const unsigned b = (unsigned)batch;
    // more than one group of targets and no dAlpha to read them back from: D n elements per workgroup, sized by the grid, which gives
    // way where that would pass the workspace cap of the blocked paths (launch_multi_target_grad_tile)
    T *ws = nullptr;
    const bool need_ws = (grad || gradc) && !Al && ntarget > 16;
    if (need_ws) {
        const size_t fit = blocked_workspace_cap() / ((size_t)ntarget * n * sizeof(T));
        if (fit < grid) grid = fit < 1 ? 1u : (unsigned)fit;
        const hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), (size_t)grid * ntarget * n * sizeof(T), stream);
        if (e != hipSuccess) return e;
    }
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true, true, true, true, true, true, true, true, true, true>), dim3(grid),
                               dim3(64), 0, stream, Bs, Cs, Hs, Ys, dMs, nbasis, ntarget, nparam, grad, gradc, Lm, Al, Be, ws, info, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true, true, true, true, true, true, true, true, true, true>), dim3(grid),
                               dim3(64), 0, stream, Bs, Cs, Hs, Ys, dMs, nbasis, ntarget, nparam, grad, gradc, Lm, Al, Be, ws, info, n, b);
    });
    const hipError_t e = hipGetLastError();
    const hipError_t e2 = need_ws ? scratch_free(ws, stream) : hipSuccess;
    return e != hipSuccess ? e : e2;
}
}  // namespace matinv
