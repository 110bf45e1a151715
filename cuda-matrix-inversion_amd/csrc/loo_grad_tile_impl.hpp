// loo_grad_tile_impl.hpp (instantiated by loo_grad_tile_kernels.hip for f64 and loo_grad_tile_f32_kernels.hip for f32) -- gradients of
// the batched GP leave-one-out log pseudo-likelihood (Rasmussen & Williams, 5.4.2) on the MFMA tile layout, n <= 96. With
// M = B + diag c (c optional), K = M^-1, alpha = K d, kappa_i = K_ii and P symmetric derivative matrices dM_p:
//     b_i = alpha_i / kappa_i      beta = K b      s_i = (1 + alpha_i^2 / kappa_i) / kappa_i      H = K diag(s) K
//     G = 1/2 (alpha beta^T + beta alpha^T) - 1/2 H
//     grad[p] = sum_ij G_ij dM_p[i][j]      gradc[i] = G_ii      logpl = sum_i (1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i) - n/2 log 2 pi
// The load, the PanelSolve pipeline and the block-step loop are spd_load_lower and spd_full_sweep of spd_sweep.hpp, which the other GP
// tile kernels call, kept HERE as a copy of their own: called from the shared header, the fp32 forms lost the constant offsets of a fifth
// of their panel stores (one address register per store, 7 to 23 registers more) and the full fp32 6 x 6 form spilled 12 registers to
// scratch ("The shared SPD sweep"). A change to the sweep is made there and here. The sweep ends with W = -M^-1 in the lower tiles (diagonal tiles
// complete); the epilogue folds alpha, kappa and beta out of the registers as the gradient epilogue does, builds H one tile column at
// a time on the MFMA unit as the prediction epilogue builds T = W A, turns that column into G in place and contracts it with the same
// tiles of each dM_p streamed from HBM. Neither M, its inverse nor H is ever stored.
// HBM traffic per matrix: (P + 1) n^2 / 2 + 2 n elements in, P + n + 1 out (grad is read back NT - 1 times by the lane that wrote it).
// A non-positive (or NaN) pivot makes info = its column + 1 (PanelSolve::binfo) and every output NaN: no fallback launch.
//
// The kernels are the LOO-gradient forms of the SPD inversion kernels whose sweep they run: overloads of matinv_spd_tile_f64 / _f32 with
// five more trailing template arguments ("Gradients of the leave-one-out pseudo-likelihood", says why).
#pragma once
#include <utility>

#include "predict_tile_impl.hpp"  // predict_qstride, predict_tile_grid, the launch bounds of the prediction forms; dpp_row_sum16

namespace matinv {

__device__ __forceinline__ double loo_grad_log(double v) { return log(v); }
__device__ __forceinline__ float loo_grad_log(float v) { return logf(v); }

// f(integral_constant<int, 0>) ... f(integral_constant<int, NT - 1>): the tile column is a compile-time number inside a body that holds
// a run-time loop (the accumulators are indexed with it)
template <class F, int... I>
__device__ __forceinline__ void loo_grad_for_each_column(F &&f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>{}), ...);
}

// Epilogue layout (lane l = 16 q + c; the lane holds W[16 ti + trow(r, q)][16 tj + c] in acc[ti][tj][r], tj <= ti):
//   LDS: panel[4 N] (the sweep's; x, the row part of W x and kappa during the two vector products, then the panel of each block step
//        again), four N-vectors al = alpha, be = beta, sv = s (zero beyond n), bv = b, and aq[16 (N + 1)] = the 16 columns of diag(s) W
//        of the current tile column, column j at aq + j (N + 1).
//   1. alpha = -W d, kappa = -diag W as in logml_grad_tile_body: row part over the 16 c lanes by DPP, mirror part over the four q groups.
//      Every lane then holds alpha of index 16 tj + c for each tj and computes b, s and the logpl term of that index: one division and
//      one logarithm each. The terms are summed over tj in ascending order, then over the 16 c lanes by DPP; lane 0 stores logpl.
//   2. beta = -W b: the same product with b in place of d.
//   3. per tile column tj: the columns 16 tj .. 16 tj + 15 of diag(s) W go to aq from the accumulators (tile rows ti >= tj from
//      acc[ti][tj], the rows above from the transposes of acc[tj][ti]); then, as in predict_tile_body, for every real block step kb the
//      four columns of W that block holds go to the LDS panel and one MFMA per tile row ti >= tj adds to h[ti]. W = -K, so
//      h = (-K) S (-K) = H, in the accumulator layout of the tiles [ti][tj]. 4 NT (NT - tj) MFMAs per column; W stays intact.
//   4. h[ti][r] <- w (1/2 (alpha_row beta_col + beta_row alpha_col) - 1/2 h[ti][r]), w = 1 in the diagonal tile (both triangles
//      stored), 2 below (each tile stands for its mirror): grad is the whole sum over i and j, and G carries its own factors 1/2
//      (logml_grad_tile_body has w = 1/2 and 1 because its gradient is HALF that sum). The lane that holds a diagonal element stores
//      gradc, unweighted.
//   5. per p: the lane's 4 (NT - tj) products with the tiles [ti][tj] of dM_p (addressing and predication of the load of B; the diagonal
//      tile through the (lo, hi) mirror) in four chains by register, ((p0 + p1) + (p2 + p3)), the 16 c lanes by DPP, the four q groups
//      by two __shfl_xor. Lane 0 stores the partial sum of tile column 0 to grad[p] and adds those of the later columns to what it
//      stored, in ascending tj: an order that knows nothing of batch, grid, P or the position of p.
template <class T, int NT, bool FULL>
__device__ __forceinline__ void loo_grad_tile_body(const T *Bs, const T *Cs, const T *Ds, const T *dMs, int nparam, T *grad, T *gradc,
                                                   T *logpl, int *info, int n_rt, unsigned batch, T *panel, T *vecs, T *aq)
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
        const bool ok = bad == 0;
        const T *vd = Ds + (size_t)mat * n;
        T *const sd = panel, *const rs = panel + N, *const kap = panel + 2 * N;
        T *const al = vecs, *const be = vecs + N, *const sv = vecs + 2 * N, *const bv = vecs + 3 * N;
        wave_lds_sync();  // the last panel has been consumed
#pragma unroll
        for (int k = 0; k < (N + 63) / 64; ++k) {
            const int i = l + 64 * k;
            if (i < N) sd[i] = (FULL || i < n) ? vd[i] : (T)0;  // identity padding contributes nothing
        }
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (G::trow(r, q) == c) kap[16 * ti + c] = -acc[ti][ti][r];  // the one lane that holds W_ii
        // col[tj] = -(W x)[16 tj + c], x an N-vector in LDS: the row and mirror parts of logml_grad_tile_body
        auto minus_w_times = [&](const T *x, T (&col)[NT]) {
            wave_lds_sync();  // x is written; the previous product's reads of rs are done
            T colacc[NT];
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) colacc[tj] = (T)0;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                T rowacc[4] = {(T)0, (T)0, (T)0, (T)0};
                T xr[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) xr[r] = x[16 * ti + G::trow(r, q)];
#pragma unroll
                for (int tj = 0; tj <= ti; ++tj) {
                    const T xc = x[16 * tj + c];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        rowacc[r] = fma_t(acc[ti][tj][r], xc, rowacc[r]);
                        if (tj < ti) colacc[tj] = fma_t(acc[ti][tj][r], xr[r], colacc[tj]);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    rowacc[r] = dpp_row_sum16(rowacc[r]);
                    if (c == 0) rs[16 * ti + G::trow(r, q)] = rowacc[r];
                }
            }
#pragma unroll
            for (int tj = 0; tj < NT - 1; ++tj) {
                colacc[tj] += __shfl_xor(colacc[tj], 16);
                colacc[tj] += __shfl_xor(colacc[tj], 32);
            }
            wave_lds_sync();
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) col[tj] = -(rs[16 * tj + c] + colacc[tj]);  // W = -M^-1
        };
        T acol[NT];
        minus_w_times(sd, acol);
        T term = (T)0;
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
            const int i = 16 * tj + c;
            const bool in = FULL || tj < NT - 1 || i < n;
            const T a = acol[tj];
            const T kappa = kap[i];
            const T rk = (T)1 / kappa;
            const T b = a * rk;
            if (in) term += (T)0.5 * loo_grad_log(kappa) - (T)0.5 * a * b;
            if (q == 0) {  // the four q groups hold the same bits
                al[i] = a;
                bv[i] = b;
                sv[i] = in ? fma_t(a, b, (T)1) * rk : (T)0;
            }
        }
        term = dpp_row_sum16(term);
        if (l == 0 && logpl) logpl[mat] = ok ? term - (T)n * (T)0.91893853320467274178 : nan_of<T>();
        if (grad || gradc) {  // wave-uniform
            T bcol[NT];
            minus_w_times(bv, bcol);
#pragma unroll
            for (int tj = 0; tj < NT; ++tj)
                if (q == 0) be[16 * tj + c] = bcol[tj];
            loo_grad_for_each_column(
                [&](auto TJ) __attribute__((always_inline)) {
                    constexpr int tj = decltype(TJ)::value;
                    // lane coordinates and n opaque once per tile column: otherwise the LDS offsets of all NT columns are hoisted and
                    // the allocator spills them beside the accumulators (as in the loops over p and over the query groups)
                    int nc = n, qs = q, cs = c;
                    if (!FULL) asm volatile("" : "+s"(nc));
                    asm volatile("" : "+v"(qs), "+v"(cs));
                    wave_lds_sync();  // the previous column's reads of aq and of the panel; this matrix's writes of al, be, sv
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (ti >= tj) {
                                const int row = 16 * ti + G::trow(r, qs);
                                aq[cs * NS + row] = sv[row] * acc[ti][tj][r];
                            } else {  // W[16 ti + c][16 tj + trow] = W[16 tj + trow][16 ti + c]
                                const int row = 16 * ti + cs;
                                aq[G::trow(r, qs) * NS + row] = sv[row] * acc[tj][ti][r];
                            }
                        }
                    wave_lds_sync();
                    const T *const ac = aq + cs * NS;  // this lane's column of diag(s) W
                    vec4 h[NT];
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                        for (int r = 0; r < 4; ++r) h[ti][r] = (T)0;
#pragma unroll
                    for (int kb = 0; kb < NKB; ++kb) {
                        // the block steps the sweep skipped hold identity padding, and s is zero there
                        if (!FULL && kb > 4 * (NT - 1) && kb - 4 * (NT - 1) >= G::real_blocks(nc - 16 * (NT - 1))) continue;
                        const int tK = kb >> 2, rK = kb & 3;
                        wave_lds_sync();
                        spd_panel_to_lds<NT, T>(panel, acc, kb, qs, cs);
                        wave_lds_sync();
                        const T b = ac[16 * tK + G::pcol(rK, qs)];
#pragma unroll
                        for (int ti = 0; ti < NT; ++ti) {
                            if (ti < tj) continue;
                            h[ti] = G::mfma(panel[(16 * ti + cs) * 4 + qs], b, h[ti]);
                        }
                    }
                    // G of the column, in place of H
                    const int icol = 16 * tj + cs;
                    const bool col_in = FULL || tj < NT - 1 || icol < nc;
                    const T ac_ = al[icol], bc_ = be[icol];
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti) {
                        if (ti < tj) continue;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * ti + G::trow(r, qs);
                            const T u = fma_t((T)-0.5, h[ti][r], (T)0.5 * fma_t(al[row], bc_, be[row] * ac_));
                            if (ti == tj && gradc && G::trow(r, qs) == cs && col_in)
                                gradc[(size_t)mat * nc + icol] = ok ? u : nan_of<T>();
                            h[ti][r] = (ti == tj) ? u : (T)2 * u;
                        }
                    }
                    if (grad) {  // wave-uniform
                        for (int p = 0; p < nparam; ++p) {
                            // opaque once per p: otherwise the element offsets (and, ragged, as many predicates) are hoisted out of this loop
                            int np = nc, qp = qs, cp = cs;
                            if (!FULL) asm volatile("" : "+s"(np));
                            asm volatile("" : "+v"(qp), "+v"(cp));
                            const T *D = dMs + ((size_t)mat * nparam + p) * np * np;
                            T part[4] = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
                            for (int ti = 0; ti < NT; ++ti) {
                                if (ti < tj) continue;
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    const int row = 16 * ti + G::trow(r, qp), col = 16 * tj + cp;
                                    const bool in = FULL || ti < NT - 1 || (row < np && col < np);
                                    const int hi = row > col ? row : col, lo = row > col ? col : row;
                                    const T v = in ? D[(unsigned)(lo * np + hi)] : (T)0;  // beyond n: never issued, counts as 0
                                    part[r] = fma_t(h[ti][r], v, part[r]);
                                }
                            }
                            T s = (part[0] + part[1]) + (part[2] + part[3]);
                            s = dpp_row_sum16(s);
                            s += __shfl_xor(s, 16);
                            s += __shfl_xor(s, 32);
                            if (l == 0) {
                                T *const out = grad + (size_t)mat * nparam + p;
                                const T sum = (tj == 0) ? s : *out + s;  // the columns before this one, in ascending tj
                                *out = ok ? sum : nan_of<T>();
                            }
                        }
                    }
                },
                std::make_integer_sequence<int, NT>{});
        }
        int code = binfo;
        if constexpr (sizeof(T) == 4) {
            if (bad != 0) {  // wave-uniform; rejected matrices only: the fp32 tile order does not say which column fails FIRST (tile_common.hpp)
                wave_lds_sync();  // the last column's reads of the panel
                const int nat = spd_natural_first_failure<NT, T>(A, Cs ? Cs + (size_t)mat * n : nullptr, n, panel, l);
                if (nat) code = nat;
            }
        }
        if (l == 0 && info) info[mat] = code;
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// The LOO-gradient forms of matinv_spd_tile_f64 / matinv_spd_tile_f32 (tile_impl.hpp): the same names with seven template arguments,
// the launch bounds of the prediction forms for the same NT (predict_tile_impl.hpp); profiles/loo_grad_kernel_registers.txt.
constexpr int loo_grad_f64_waves(int nt, bool full) { return predict_f64_waves(nt, full); }
constexpr int loo_grad_f32_waves(int nt, bool full) { return predict_f32_waves(nt, full); }

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD>
__global__ __launch_bounds__(64, loo_grad_f64_waves(NT, FULL)) void matinv_spd_tile_f64(const double *Bs, const double *Cs, const double *Ds,
                                                                                               const double *dMs, int nparam, double *grad,
                                                                                               double *gradc, double *logpl, int *info, int n_rt,
                                                                                               unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD, "the seven-argument form is the leave-one-out gradient kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    __shared__ double vecs[16 * NT * 4], aq[16 * predict_qstride(16 * NT)];
    loo_grad_tile_body<double, NT, FULL>(Bs, Cs, Ds, dMs, nparam, grad, gradc, logpl, info, n_rt, batch, panel, vecs, aq);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD>
__global__ __launch_bounds__(64, loo_grad_f32_waves(NT, FULL)) void matinv_spd_tile_f32(const float *Bs, const float *Cs, const float *Ds,
                                                                                               const float *dMs, int nparam, float *grad,
                                                                                               float *gradc, float *logpl, int *info, int n_rt,
                                                                                               unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD, "the seven-argument form is the leave-one-out gradient kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    __shared__ float vecs[16 * NT * 4], aq[16 * predict_qstride(16 * NT)];
    loo_grad_tile_body<float, NT, FULL>(Bs, Cs, Ds, dMs, nparam, grad, gradc, logpl, info, n_rt, batch, panel, vecs, aq);
}

template <class T>
hipError_t launch_loo_grad_tile(int n, int nparam, const T *Bs, const T *Cs, const T *Ds, const T *dMs, T *grad, T *gradc, T *logpl,
                                size_t batch, int *info, hipStream_t stream)
{
    if (!loo_grad_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = predict_tile_grid(batch), b = (unsigned)batch;
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true, true, true, true>), dim3(grid), dim3(64), 0, stream, Bs, Cs, Ds, dMs,
                               nparam, grad, gradc, logpl, info, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true, true, true, true>), dim3(grid), dim3(64), 0, stream, Bs, Cs, Ds, dMs,
                               nparam, grad, gradc, logpl, info, n, b);
    });
    return hipGetLastError();
}
}  // namespace matinv
