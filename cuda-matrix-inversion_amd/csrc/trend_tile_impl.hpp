// trend_tile_impl.hpp (instantiated by trend_tile_kernels.hip for f64 and trend_tile_f32_kernels.hip for f32) -- GP regression with a
// linear trend (universal kriging; Rasmussen & Williams 2.7 in the vague-prior limit) on the MFMA tile layout, n <= 96. With
// M = B + diag c (c optional), Kinv = M^-1, H = [h_1 .. h_K] the basis vectors (K = nbasis <= 16), y_t target t, and for query j the
// cross-covariance a_j, the basis values g_j and the prior variance e_j:
//     A = H^T Kinv H          covbeta = A^-1          beta_t = A^-1 H^T Kinv y_t          alpha_t = Kinv (y_t - H beta_t)
//     quad_t = y_t^T alpha_t  logml_t = -1/2 (quad_t + log det M + log det A + (n - K) log 2 pi)
//     mean[t][j] = a_j^T alpha_t + g_j^T beta_t
//     var[j] = e_j - a_j^T Kinv a_j + r_j^T A^-1 r_j,   r_j = g_j - H^T Kinv a_j
// The load, the PanelSolve pipeline, the block-step loop and the pivot fold are those of multi_target_tile_body
// (multi_target_tile_impl.hpp), copied once more so that every earlier kernel compiles to what it compiled to before. A copy of spd_load_lower and
// spd_full_sweep (spd_sweep.hpp) as it stands: called from the shared header these forms pair their LDS stores differently and spill more
// SGPRs into VGPR lanes ("The shared SPD sweep"); a change to the sweep is made there and here. The sweep ends with
// W = -Kinv in the lower tiles. What this form adds is the epilogue:
//   1. H is staged as ONE group of 16 vectors, zero beyond K and beyond n. T_H = W H is built as every T_g is; -A = H^T T_H is one
//      16 x 16 block in 4 NT MFMAs. A gets an identity diagonal beyond K (its off-diagonal padding is exactly zero: zero operands).
//   2. T_H is parked in a second group-sized LDS buffer hq, vector b at hq + b (N + 1): there it is the A operand of every later product
//      with Kinv H, and no accumulator-sized set of registers has to live through the target and query loops (see the launch bounds).
//   3. The wave factors A = L L^T in LDS, right-looking, one column a step, reading the lower triangle only, and forms L^-1 in the same
//      steps (forward substitution on the identity); log det A comes from the pivots through a PivotProduct. L^-1 stays in a
//      16 x 17 LDS tile: every later product with A^-1 is a 16 x 16 x 16 product on the MFMA unit with L^-1 or L^-T as the A operand. A
//      block in the accumulator layout is already a B operand (its k index runs over trow(r, q)), so these products chain without a
//      trip through LDS. covbeta = L^-T L^-1 is four MFMAs; its lower triangle is stored to both positions.
//   4. var, once per query group, independent of the targets: T_A = W A_h and a^T Kinv a as predict_tile_body has them; the block
//      T_H^T A_h = -(H^T Kinv a_j) with both operands read from LDS; r = g + that block; z = L^-1 r, r^T A^-1 r = sum z_b^2 >= 0.
//   5. per target group: T_g = W Y_g; the block T_H^T Y_g = -(H^T Kinv y_t); -beta = L^-T (L^-1 of it) goes to a 16 x 17 LDS tile;
//      T_g += T_H (-beta) in four 16 x 16 x 4 MFMAs per tile row, which makes T_g = W (y - H beta) = -alpha. quad, alpha and the mean
//      block follow as in multi_target_tile_body; the mean block takes four more MFMAs G_h (-beta) on the same accumulator.
// Every loop over the basis runs over all 16 slots in a fixed order; a padding slot contributes an exact zero (or an exact factor 1), so
// K enters the bits only through the vectors themselves. Nothing in the order of operations of an output depends on batch, grid, D, Q,
// or the group or lane of a target or query; which outputs are stored is decided by wave-uniform pointers and changes no operation of
// another output. Y is read only with beta, alpha, quad, logml or mean; A and G only with mean or var; E only with var.
// HBM traffic per matrix: n^2 / 2 + n + K n + D n + (ceil(D / 16) + 1) Q (n + K) + Q elements in (the query terms only when mean / var
// are asked for), K^2 + D K + D n + 2 D + D Q + Q out.
// info: the 1-based column of the first non-positive (or NaN) pivot of M (PanelSolve::binfo; fp32: the natural-order redo); else n + b
// for the first non-positive (or NaN) pivot b of A. Either makes every requested output of the matrix NaN: no fallback launch.
//
// The kernels are overloads of matinv_spd_tile_f64 / _f32 with ten more trailing template arguments ("Regression with a
// linear trend").
#pragma once
#include "multi_target_tile_impl.hpp"  // predict_qstride, predict_tile_grid, the launch bounds of the multi-target forms
#include "chol_block.hpp"              // sqrt_and_rsqrt

namespace matinv {

constexpr int TREND_TS = 17;  // row stride of the 16 x 16 LDS tiles

template <class T, int NT, bool FULL>
__device__ __forceinline__ void trend_tile_body(const T *Bs, const T *Cs, const T *Hs, const T *Ys, const T *As, const T *Gs, const T *Es,
                                                int nbasis, int ntarget, int nquery, T *Be, T *Cb, T *Al, T *Qd, T *Lm, T *Mn, T *Vr,
                                                int *info, int n_rt, unsigned batch, T *panel, T *aq, T *hq, T *sm)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    constexpr int N = 16 * NT;
    constexpr int NKB = 4 * NT;
    constexpr int NS = predict_qstride(N);
    constexpr int TS = TREND_TS;
    typedef PanelSolve<NT, true, T> PS;
    const int l = threadIdx.x;
    // the four 16 x 17 tiles: t0 = A while it is factored, then the tile the mean block is transposed through; t1 = G_h; t2 = L^-1;
    // t3 = -beta of the current target group
    T *const t0 = sm, *const t1 = sm + 16 * TS, *const t2 = sm + 32 * TS, *const t3 = sm + 48 * TS;

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

        {
            int qb = q, cv = c;
            asm volatile("" : "+v"(qb), "+v"(cv));
            if (Cb) {  // wave-uniform
                // covbeta = L^-T L^-1 in four MFMAs, both operands the same LDS element: lane (q, c) ends with element
                // (trow(r, q), c). The lower triangle is stored to both positions.
                vec4 cv4;
#pragma unroll
                for (int r = 0; r < 4; ++r) cv4[r] = (T)0;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const T v = t2[(4 * kk + qb) * TS + cv];
                    cv4 = G::mfma(v, v, cv4);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int b1 = G::trow(r, qb), b2 = cv;
                    if (b1 >= b2 && b1 < nbasis) {
                        const T v = ok ? cv4[r] : nan_of<T>();
                        T *const o = Cb + (size_t)mat * nbasis * nbasis;
                        o[b1 * nbasis + b2] = v;
                        o[b2 * nbasis + b1] = v;
                    }
                }
            }
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

        // ---- 4: var, once per query group ---------------------------------------------------------------------------------------
        const int nvgroups = Vr ? (nquery + 15) >> 4 : 0;  // wave-uniform
        for (int h = 0; h < nvgroups; ++h) {
            // lane coordinates and n opaque once per group (multi_target_tile_body)
            int nr = n, lr = l, qr = q, cr = c;
            if (!FULL) asm volatile("" : "+s"(nr));
            asm volatile("" : "+v"(lr), "+v"(qr), "+v"(cr));
            const int leftq = nquery - 16 * h;
            const size_t firstq = (size_t)mat * nquery + 16 * (size_t)h;
            wave_lds_sync();  // the previous group's reads of the buffer and of t0
            stage(As + firstq * nr, leftq, nr, lr);
            wave_lds_sync();
            vec4 tq[NT];
            build_t(tq, nr, qr, cr);
            const T aka = -dot_t(tq, qr, cr);  // a^T Kinv a; W = -Kinv
            const vec4 cb = block_h(qr, cr);   // -(H^T Kinv a_c)[trow(r, q)]
            vec4 rv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = G::trow(r, qr);
                const T gv = (b < nbasis && cr < leftq) ? Gs[(firstq + cr) * nbasis + b] : (T)0;
                rv[r] = gv + cb[r];
            }
            // z = L^-1 r, r^T A^-1 r = sum z_b^2: ((z0^2 + z1^2) + (z2^2 + z3^2)) per lane, the four q groups by two __shfl_xor
            const vec4 z = linv_mul(rv, qr, cr);
            T rar = fma_t(z[0], z[0], z[1] * z[1]) + fma_t(z[2], z[2], z[3] * z[3]);
            rar += __shfl_xor(rar, 16);
            rar += __shfl_xor(rar, 32);
            if (qr == 0 && cr < leftq) Vr[firstq + cr] = ok ? (Es[firstq + cr] - aka) + rar : nan_of<T>();
        }

        // ---- 5: the targets in groups of 16 -------------------------------------------------------------------------------------
        const int ngroups = (Be || Al || Qd || Lm || Mn) ? (ntarget + 15) >> 4 : 0;  // wave-uniform; the targets are not read otherwise
        const int nqgroups = Mn ? (nquery + 15) >> 4 : 0;                             // nor the queries
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
                    if (Qd) Qd[first + cg] = ok ? qd : nan_of<T>();
                    // log 2 pi
                    if (Lm)
                        Lm[first + cg] = ok ? (T)-0.5 * fma_t((T)(ng - nbasis), (T)1.83787706640934548356, qd + (ld + ldA)) : nan_of<T>();
                }
            }
            if (Al) {             // wave-uniform
                wave_lds_sync();  // the targets have been read: the buffer takes the group's alpha, vector by vector
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) yc[16 * ti + G::trow(r, qg)] = ok ? -tq[ti][r] : nan_of<T>();
                wave_lds_sync();
                // opaque once more (multi_target_tile_body)
                int na = ng, la = lg;
                if (!FULL) asm volatile("" : "+s"(na));
                asm volatile("" : "+v"(la));
                T *Ag = Al + first * na;
#pragma unroll
                for (int k = 0; k < N / 4; ++k) {
                    const int e = la + 64 * k, j = e / N, i = e - j * N;
                    if ((FULL || i < na) && j < left) Ag[(unsigned)(j * na + i)] = aq[j * NS + i];
                }
            }
            for (int h = 0; h < nqgroups; ++h) {
                int nr = ng, lr = lg, qr = qg, cr = cg;
                if (!FULL) asm volatile("" : "+s"(nr));
                asm volatile("" : "+v"(lr), "+v"(qr), "+v"(cr));
                const int leftq = nquery - 16 * h;
                const size_t firstq = (size_t)mat * nquery + 16 * (size_t)h;
                wave_lds_sync();  // the previous block's reads of the buffer and of the tiles, the stores of alpha
                stage(As + firstq * nr, leftq, nr, lr);
                // G_h, element (j, b) at t1 + j TS + b, zero beyond Q and beyond K
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = lr + 64 * k, j = e >> 4, b = e & 15;
                    t1[j * TS + b] = (j < leftq && b < nbasis) ? Gs[(firstq + j) * nbasis + b] : (T)0;
                }
                wave_lds_sync();
                vec4 cb;
#pragma unroll
                for (int r = 0; r < 4; ++r) cb[r] = (T)0;
                cb = block_t(tq, cb, qr, cr);  // C[r] = -a_j^T alpha_t, j = 16 h + trow(r, q), t = 16 g + c
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) cb = G::mfma(t1[cr * TS + 4 * kk + qr], t3[(4 * kk + qr) * TS + cr], cb);  // - g_j^T beta_t
                // transposed through t0 so that consecutive lanes store consecutive queries (multi_target_tile_body)
#pragma unroll
                for (int r = 0; r < 4; ++r) t0[G::trow(r, qr) * TS + cr] = ok ? -cb[r] : nan_of<T>();  // [query][target]
                wave_lds_sync();
                const int jq = 16 * h + cr;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tl = G::trow(r, qr);
                    const T w = t0[cr * TS + tl];
                    if (tl < left && cr < leftq) Mn[(first + tl) * (size_t)nquery + jq] = w;
                }
            }
        }
        int code = binfo;
        if constexpr (sizeof(T) == 4) {
            if (bad != 0) {  // wave-uniform; rejected matrices only: the fp32 tile order does not say which column fails FIRST (tile_common.hpp)
                wave_lds_sync();  // the last group's reads of the panel
                const int nat = spd_natural_first_failure<NT, T>(A, Cs ? Cs + (size_t)mat * n : nullptr, n, panel, l);
                if (nat) code = nat;
            }
        }
        if (bad == 0 && abad != 0) code = n + abad;
        if (l == 0 && info) info[mat] = code;
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// The trend forms of matinv_spd_tile_f64 / matinv_spd_tile_f32 (tile_impl.hpp): the same names with a third to a twelfth template
// argument. Launch bounds: those of the multi-target forms for the same NT (the same live set: accumulators, T_g and one block; Kinv H
// and the inverse factor of A live in LDS), one wave per SIMD fewer where a form does not fit them. Under the multi-target bounds no form
// spilled to scratch, but the fp64 1 x 1 to 3 x 3 forms and the fp32 4 x 4 forms did not reach the occupancy asked for (125 to 187
// registers against 128 or 168; hipcc then lowers the occupancy by itself and warns), and the fp32 4 x 4 forms parked 48 and 54
// accumulator registers in AGPRs, with which the full fp32 4 x 4 kernel rejected every matrix on the GPU (the AGPR-form MFMA fault of
// this compiler that the Makefile describes for the wide fp32 sweeps). With one wave fewer they use no AGPR:
// profiles/trend_kernel_registers.txt. No form uses scratch.
constexpr int trend_f64_waves(int nt, bool full)
{
    const bool spills = nt <= 3;
    return multi_target_f64_waves(nt, full) - (spills ? 1 : 0);
}
constexpr int trend_f32_waves(int nt, bool full)
{
    const bool spills = nt == 4;
    return multi_target_f32_waves(nt, full) - (spills ? 1 : 0);
}

#define MATINV_TREND_ARGS                                                                                                                  \
    LOO &&GRAD &&PREDICT &&COV &&LOOGRAD &&COLOUR &&WHITEN &&MULTI &&MTGRAD &&TREND

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD,
          bool TREND>
__global__ __launch_bounds__(64, trend_f64_waves(NT, FULL)) void matinv_spd_tile_f64(
    const double *Bs, const double *Cs, const double *Hs, const double *Ys, const double *As, const double *Gs, const double *Es, int nbasis,
    int ntarget, int nquery, double *Be, double *Cb, double *Al, double *Qd, double *Lm, double *Mn, double *Vr, int *info, int n_rt,
    unsigned batch)
{
    static_assert(MATINV_TREND_ARGS, "the twelve-argument form is the trend kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    __shared__ double aq[16 * predict_qstride(16 * NT)];
    __shared__ double hq[16 * predict_qstride(16 * NT)];
    __shared__ double sm[64 * TREND_TS];
    trend_tile_body<double, NT, FULL>(Bs, Cs, Hs, Ys, As, Gs, Es, nbasis, ntarget, nquery, Be, Cb, Al, Qd, Lm, Mn, Vr, info, n_rt, batch,
                                      panel, aq, hq, sm);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD,
          bool TREND>
__global__ __launch_bounds__(64, trend_f32_waves(NT, FULL)) void matinv_spd_tile_f32(
    const float *Bs, const float *Cs, const float *Hs, const float *Ys, const float *As, const float *Gs, const float *Es, int nbasis,
    int ntarget, int nquery, float *Be, float *Cb, float *Al, float *Qd, float *Lm, float *Mn, float *Vr, int *info, int n_rt,
    unsigned batch)
{
    static_assert(MATINV_TREND_ARGS, "the twelve-argument form is the trend kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    __shared__ float aq[16 * predict_qstride(16 * NT)];
    __shared__ float hq[16 * predict_qstride(16 * NT)];
    __shared__ float sm[64 * TREND_TS];
    trend_tile_body<float, NT, FULL>(Bs, Cs, Hs, Ys, As, Gs, Es, nbasis, ntarget, nquery, Be, Cb, Al, Qd, Lm, Mn, Vr, info, n_rt, batch,
                                     panel, aq, hq, sm);
}
#undef MATINV_TREND_ARGS

template <class T>
hipError_t launch_trend_tile(int n, int nbasis, int ntarget, int nquery, const T *Bs, const T *Cs, const T *Hs, const T *Ys, const T *As,
                             const T *Gs, const T *Es, T *Be, T *Cb, T *Al, T *Qd, T *Lm, T *Mn, T *Vr, size_t batch, int *info,
                             hipStream_t stream)
{
    if (!trend_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = predict_tile_grid(batch), b = (unsigned)batch;  // the grid of the multi-target launcher
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true, true, true, true, true, true, true, true, true>), dim3(grid),
                               dim3(64), 0, stream, Bs, Cs, Hs, Ys, As, Gs, Es, nbasis, ntarget, nquery, Be, Cb, Al, Qd, Lm, Mn, Vr, info, n,
                               b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true, true, true, true, true, true, true, true, true>), dim3(grid),
                               dim3(64), 0, stream, Bs, Cs, Hs, Ys, As, Gs, Es, nbasis, ntarget, nquery, Be, Cb, Al, Qd, Lm, Mn, Vr, info, n,
                               b);
    });
    return hipGetLastError();
}
}  // namespace matinv
