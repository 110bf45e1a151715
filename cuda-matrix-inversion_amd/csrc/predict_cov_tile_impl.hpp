// predict_cov_tile_impl.hpp (instantiated by predict_cov_tile_kernels.hip for f64 and predict_cov_tile_f32_kernels.hip for f32) -- the
// joint predictive covariance between a GP's query points on the MFMA tile layout, n <= 96. With M = B + diag c (c optional), K = M^-1,
// alpha = K d and Q query points per matrix, a_i the cross-covariance vector of query i and E the Q x Q prior covariance of the queries:
//     mean[i] = a_i^T alpha      cov[i][j] = E[i][j] - a_i^T K a_j
// The load, the PanelSolve pipeline and the block-step loop are spd_load_lower and spd_full_sweep of spd_sweep.hpp, kept HERE as a copy
// of their own: called from the shared header, the 1 x 1 and 2 x 2 forms came out with other v_cndmask counts ("The shared
// SPD sweep"). A change to the sweep is made there and here. The alpha step is that of predict_tile_body (predict_tile_impl.hpp). The
// sweep ends with W = -M^-1 in the lower tiles; the
// epilogue takes the queries in groups of 16 as the prediction form does, and for every column group g builds T_g = W A_g once and
// multiplies it with A_g'^T for every row group g' >= g on the MFMA unit: only the lower block triangle is computed, the upper one is a
// copy of its bits, and neither M nor its inverse is ever stored.
// HBM traffic per matrix: n^2 / 2 + 2 n + 16 n G (G + 1) / 2 + Q^2 / 2 elements in (G = ceil(Q / 16)), Q^2 + Q out.
// A non-positive (or NaN) pivot makes info = its column + 1 (PanelSolve::binfo) and every output NaN: no fallback launch.
//
// The kernels are the covariance forms of the SPD inversion kernels whose sweep they run: overloads of matinv_spd_tile_f64 / _f32 with
// four more trailing template arguments ("Joint predictive covariance", says why).
#pragma once
#include "predict_tile_impl.hpp"  // predict_qstride, predict_tile_grid, the launch bounds of the prediction forms

namespace matinv {

// Epilogue layout (lane l = 16 q + c; the lane holds W[16 ti + trow(r, q)][16 tj + c] in acc[ti][tj][r], tj <= ti):
//   LDS: panel[4 N], al[N] = alpha, aq[16 (N + 1)] = the 16 query vectors of ONE group, as in predict_tile_body.
//   alpha, mean : the operations of predict_tile_body in its order, so mean carries the bits matinv_predict_batched returns.
//   for every column group g:
//     stage A_g; mean of its 16 queries; T_g = W A_g as in predict_tile_body: lane (q, c) holds T_g[16 ti + trow(r, q)][c] in tq[ti][r].
//     for every row group g' >= g (g' = g: A_g is staged already; g' > g: the same buffer is restaged, T_g lives in registers):
//       C = A_g'^T T_g, 16 x 16: for fixed (ti, r) the four lane groups q hold rows 16 ti + trow(r, q) of T_g, one per q -- a K-slab
//           of four rows in the lane layout of the MFMA's B operand as it stands; the A operand of the slab is the same four rows of
//           A_g', lane (q, c) reading a_c[16 ti + trow(r, q)] of group g'. 4 NT MFMAs in the order (ti, r), no shuffle. Lane (q, c)
//           ends with C[r] = -a_i^T K a_j, i = 16 g' + trow(r, q), j = 16 g + c, because trow is the MFMA's D-row map.
//       cov[i][j] = E[i][j] + C[r], stored at (i, j) and, the same bits, at (j, i); in the diagonal block only lanes with i >= j store.
//       Stores are predicated on i, j < Q; only the lower triangle of E is read. The block has consecutive lanes on consecutive j,
//       which is the order of the (j, i) store; E and the (i, j) store want them on consecutive i, so E comes in and the block goes
//       out transposed through a 16 x 17 tile in the query buffer (two LDS round trips of four elements a lane): every global access
//       of the epilogue is then a run of 16 consecutive elements.
//   The order of operations for (i, j), i >= j, knows nothing of batch, grid, Q, the groups of i and j or their lanes (every row and
//   every column of an MFMA is computed alike).
template <class T, int NT, bool FULL>
__device__ __forceinline__ void predict_cov_tile_body(const T *Bs, const T *Cs, const T *Ds, const T *As, int nquery, const T *Es,
                                                      T *mean, T *cov, int *info, int n_rt, unsigned batch, T *panel, T *al, T *aq)
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
        if (mean) {  // wave-uniform: alpha = -W d to LDS (the row and mirror parts of logml_grad_tile_body)
            const T *vd = Ds + (size_t)mat * n;
            wave_lds_sync();  // the last panel has been consumed
            T *const sd = panel, *const rs = panel + N;
#pragma unroll
            for (int k = 0; k < (N + 63) / 64; ++k) {
                const int i = l + 64 * k;
                if (i < N) sd[i] = (FULL || i < n) ? vd[i] : (T)0;  // identity padding contributes nothing
            }
            wave_lds_sync();
            T colacc[NT];
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) colacc[tj] = (T)0;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                T rowacc[4] = {(T)0, (T)0, (T)0, (T)0};
                T dr[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) dr[r] = sd[16 * ti + G::trow(r, q)];
#pragma unroll
                for (int tj = 0; tj <= ti; ++tj) {
                    const T dc = sd[16 * tj + c];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        rowacc[r] = fma_t(acc[ti][tj][r], dc, rowacc[r]);
                        if (tj < ti) colacc[tj] = fma_t(acc[ti][tj][r], dr[r], colacc[tj]);
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
            for (int tj = 0; tj < NT; ++tj) {
                const int i = 16 * tj + c;
                if (q == 0) al[i] = -(rs[i] + colacc[tj]);  // W = -M^-1; the four q groups hold the same bits
            }
        }
        const int ngroups = (nquery + 15) >> 4;
        T *const covm = cov ? cov + (size_t)mat * nquery * nquery : nullptr;
        const T *const Em = (cov && Es) ? Es + (size_t)mat * nquery * nquery : nullptr;
        for (int g = 0; g < ngroups; ++g) {
            // lane coordinates and n opaque once per group: otherwise the offsets of the staging loads and of the LDS reads are hoisted
            // out of this loop and the allocator spills them beside the accumulators (as in the loop over p of logml_grad_tile_body)
            int ng = n, lg = l, qg = q, cg = c;
            if (!FULL) asm volatile("" : "+s"(ng));
            asm volatile("" : "+v"(lg), "+v"(qg), "+v"(cg));
            const int left = nquery - 16 * g;  // queries from this group's first on
            const size_t first = (size_t)mat * nquery + 16 * (size_t)g;
            const T *Aq = As + first * ng;
            wave_lds_sync();  // the previous group's reads of aq, this matrix's writes of al
            // the group's 16 n contiguous elements, consecutive lanes on consecutive elements of one vector
#pragma unroll
            for (int k = 0; k < N / 4; ++k) {
                const int e = lg + 64 * k, j = e / N, i = e - j * N;
                const bool in = (FULL || i < ng) && j < left;
                aq[j * NS + i] = in ? Aq[(unsigned)(j * ng + i)] : (T)0;
            }
            wave_lds_sync();
            const T *const ac = aq + cg * NS;  // the vector of this lane's query
            if (mean) {                        // wave-uniform; before the row groups restage aq
                T part[4] = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * ti + G::trow(r, qg);
                        part[r] = fma_t(ac[row], al[row], part[r]);
                    }
                T s = (part[0] + part[1]) + (part[2] + part[3]);
                s += __shfl_xor(s, 16);
                s += __shfl_xor(s, 32);
                if (qg == 0 && cg < left) mean[first + cg] = ok ? s : nan_of<T>();
            }
            if (cov) {  // wave-uniform
                vec4 tq[NT];
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) tq[ti][r] = (T)0;
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) {
                    // the block steps the sweep skipped hold identity padding, and a is zero there
                    if (!FULL && kb > 4 * (NT - 1) && kb - 4 * (NT - 1) >= G::real_blocks(ng - 16 * (NT - 1))) continue;
                    const int tK = kb >> 2, rK = kb & 3;
                    wave_lds_sync();
                    spd_panel_to_lds<NT, T>(panel, acc, kb, qg, cg);
                    wave_lds_sync();
                    const T b = ac[16 * tK + G::pcol(rK, qg)];
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti) tq[ti] = G::mfma(panel[(16 * ti + cg) * 4 + qg], b, tq[ti]);
                }
                const int j = 16 * g + cg;  // this lane's column of cov
                for (int gp = g; gp < ngroups; ++gp) {
                    // opaque once per row group, for the reason given at the loop over g
                    int nr = ng, lr = lg, qr = qg, cr = cg;
                    if (!FULL) asm volatile("" : "+s"(nr));
                    asm volatile("" : "+v"(lr), "+v"(qr), "+v"(cr));
                    if (gp > g) {  // wave-uniform: the row group's vectors take the place of the column group's
                        const int leftr = nquery - 16 * gp;
                        const T *Ar = As + ((size_t)mat * nquery + 16 * (size_t)gp) * nr;
                        wave_lds_sync();  // the previous block's reads of aq
#pragma unroll
                        for (int k = 0; k < N / 4; ++k) {
                            const int e = lr + 64 * k, jj = e / N, i = e - jj * N;
                            const bool in = (FULL || i < nr) && jj < leftr;
                            aq[jj * NS + i] = in ? Ar[(unsigned)(jj * nr + i)] : (T)0;
                        }
                        wave_lds_sync();
                    }
                    const T *const ar = aq + cr * NS;  // as the A operand lane (q, c) supplies row c of A_g'^T
                    vec4 cb;
#pragma unroll
                    for (int r = 0; r < 4; ++r) cb[r] = (T)0;
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                        for (int r = 0; r < 4; ++r) cb = G::mfma(ar[16 * ti + G::trow(r, qr)], tq[ti][r], cb);
                    // E and the lower store want consecutive lanes on consecutive i (element (i, j) at j Q + i), the block has them on
                    // consecutive j: both go through a 16 x 16 tile in the query buffer, which is free once the MFMAs have read it
                    // (the next row group, or the next column group, restages it). In the transposed layout lane (q, c) serves
                    // i = 16 g' + c, j = 16 g + trow(r, q).
                    constexpr int TS = 17;  // 16 (N + 1) >= 16 * 17 elements
                    const int it = 16 * gp + cr;
                    wave_lds_sync();  // the A operands have been read
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int jl = G::trow(r, qr), jt = 16 * g + jl;
                        const bool in = it < nquery && jt < nquery && it >= jt;
                        aq[jl * TS + cr] = (Em && in) ? Em[(unsigned)jt * (unsigned)nquery + (unsigned)it] : (T)0;
                    }
                    wave_lds_sync();
                    T v[4];  // E[i][j] + C in the block's layout: i by (r, q), j by c
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = ok ? aq[cr * TS + G::trow(r, qr)] + cb[r] : nan_of<T>();
                    wave_lds_sync();
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int il = G::trow(r, qr), i = 16 * gp + il;  // i >= j in every block below the diagonal ones
                        aq[il * TS + cr] = v[r];
                        if (i < nquery && j < nquery && i >= j) covm[(unsigned)i * (unsigned)nquery + (unsigned)j] = v[r];  // the mirror
                    }
                    wave_lds_sync();
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int jl = G::trow(r, qr), jt = 16 * g + jl;
                        const T w = aq[cr * TS + jl];  // the bits of (i, j) = (it, jt)
                        if (it < nquery && jt < nquery && it >= jt) covm[(unsigned)jt * (unsigned)nquery + (unsigned)it] = w;
                    }
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
        if (l == 0 && info) info[mat] = code;
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// The covariance forms of matinv_spd_tile_f64 / matinv_spd_tile_f32 (tile_impl.hpp): the same names with a third to a sixth template
// argument. Launch bounds: those of the prediction forms for the same NT (predict_tile_impl.hpp), one wave per SIMD fewer where a form
// spills under them (profiles/predict_cov_kernel_registers.txt); no form uses scratch.
constexpr int predict_cov_f64_waves(int nt, bool full) { return predict_f64_waves(nt, full); }
constexpr int predict_cov_f32_waves(int nt, bool full) { return predict_f32_waves(nt, full); }

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV>
__global__ __launch_bounds__(64, predict_cov_f64_waves(NT, FULL)) void matinv_spd_tile_f64(const double *Bs, const double *Cs,
                                                                                                  const double *Ds, const double *As, int nquery,
                                                                                                  const double *Es, double *mean, double *cov,
                                                                                                  int *info, int n_rt, unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV, "the six-argument form is the predictive-covariance kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    __shared__ double al[16 * NT], aq[16 * predict_qstride(16 * NT)];
    predict_cov_tile_body<double, NT, FULL>(Bs, Cs, Ds, As, nquery, Es, mean, cov, info, n_rt, batch, panel, al, aq);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV>
__global__ __launch_bounds__(64, predict_cov_f32_waves(NT, FULL)) void matinv_spd_tile_f32(const float *Bs, const float *Cs, const float *Ds,
                                                                                                  const float *As, int nquery, const float *Es,
                                                                                                  float *mean, float *cov, int *info, int n_rt,
                                                                                                  unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV, "the six-argument form is the predictive-covariance kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    __shared__ float al[16 * NT], aq[16 * predict_qstride(16 * NT)];
    predict_cov_tile_body<float, NT, FULL>(Bs, Cs, Ds, As, nquery, Es, mean, cov, info, n_rt, batch, panel, al, aq);
}

template <class T>
hipError_t launch_predict_cov_tile(int n, int nquery, const T *Bs, const T *Cs, const T *Ds, const T *As, const T *Es, T *mean, T *cov,
                                   size_t batch, int *info, hipStream_t stream)
{
    if (!predict_cov_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = predict_tile_grid(batch), b = (unsigned)batch;  // 256 * 12 workgroups a round (predict_tile_impl.hpp)
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true, true, true>), dim3(grid), dim3(64), 0, stream, Bs, Cs, Ds, As, nquery,
                               Es, mean, cov, info, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true, true, true>), dim3(grid), dim3(64), 0, stream, Bs, Cs, Ds, As, nquery,
                               Es, mean, cov, info, n, b);
    });
    return hipGetLastError();
}
}  // namespace matinv
