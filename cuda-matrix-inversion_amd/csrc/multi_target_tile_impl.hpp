// multi_target_tile_impl.hpp (instantiated by multi_target_tile_kernels.hip for f64 and multi_target_tile_f32_kernels.hip for f32) --
// multi-output GP solves on the MFMA tile layout, n <= 96: D target vectors and Q query points per covariance matrix. With M = B + diag c
// (c optional), K = M^-1, y_t target t and a_j the cross-covariance vector of query j:
//     alpha_t = K y_t      quad_t = y_t^T K y_t      logdet = log det M      logml_t = -1/2 (quad_t + logdet + n log 2 pi)
//     mean[t][j] = a_j^T alpha_t
// The load, the PanelSolve pipeline and the block-step loop are spd_load_lower and spd_full_sweep (spd_sweep.hpp), shared with every
// other GP tile kernel. What this form adds:
//   * the four pivots of each block step (PanelSolve's d[0][0], u11, u22, u33, the same value in every lane) are folded into a
//     PivotProduct right after stage 3 of the step's solve (the sweep's on_pivots), as in logdet_tile_body; the fold pins its result where it is formed
//     (pivot_product.hpp; whiten_tile_impl.hpp tells what the compiler does without such a pin). The block steps a ragged form skips hold
//     identity padding: their pivots are exactly 1 and a product with 1 is exact, so folded or not they contribute nothing. One
//     log_value() per matrix.
//   * the sweep ends with W = -M^-1 in the lower tiles; the targets are taken in groups of 16 exactly as predict_tile_body takes the
//     queries: T_g = W Y_g is MFMA work and stays in registers, alpha = -T_g leaves through the group buffer, quad = -sum T y.
//   * mean: for every query group h the group buffer is restaged with A_h and the 16 x 16 block A_h^T T_g is the 4 NT MFMAs of
//     predict_cov_tile_body. A is re-read once per target group; the other loop order would rebuild T for every block.
// Nothing in the order of operations of an output depends on batch, grid, D, Q, or the group or lane of a target or query; which outputs
// are stored is decided by wave-uniform pointers and changes no operation of another output. Y is read only when alpha, quad, logml or
// mean is requested, A only with mean.
// HBM traffic per matrix: n^2 / 2 + n + D n + ceil(D / 16) Q n elements in, D n + 2 D + 1 + D Q out.
// A non-positive (or NaN) pivot makes info = its column + 1 (PanelSolve::binfo) and every requested output NaN: no fallback launch.
//
// The kernels are the multi-target forms of the SPD inversion kernels whose sweep they run: overloads of matinv_spd_tile_f64 / _f32 with
// eight more trailing template arguments ("Multi-output solves").
#pragma once
#include "predict_cov_tile_impl.hpp"  // predict_qstride, predict_tile_grid, the launch bounds of the covariance forms
#include "pivot_product.hpp"

namespace matinv {

// Epilogue layout (lane l = 16 q + c; the lane holds W[16 ti + trow(r, q)][16 tj + c] in acc[ti][tj][r], tj <= ti):
//   LDS: panel[4 N] (the sweep's, then the panel of each block step again), aq[16 (N + 1)] = the 16 vectors of ONE group (targets, then
//        alpha on its way out, then queries), vector j at aq + j (N + 1), zero beyond n and beyond D (or Q).
//   for every target group g:
//     stage Y_g; T_g = W Y_g as predict_tile_body builds tq: lane (q, c) holds T_g[16 ti + trow(r, q)][target c] in tq[ti][r].
//     quad  : s = sum_ti sum_r tq[ti][r] y_c[16 ti + trow(r, q)] in four chains by register r, ((p0 + p1) + (p2 + p3)), the four q groups
//             by two __shfl_xor (16, 32); quad = -s because W = -K. logml = -1/2 fma(n, log 2 pi, quad + logdet).
//     alpha : -tq goes to the group buffer in place of y and leaves in runs of n elements per vector.
//     mean, for every query group h: restage the buffer with A_h (T_g lives in registers); C = A_h^T T_g, 16 x 16, in 4 NT MFMAs in the
//             order (ti, r) with no shuffle (predict_cov_tile_body): lane (q, c) ends with C[r] = -a_j^T alpha_t, j = 16 h + trow(r, q),
//             t = 16 g + c. Element (t, j) lives at t Q + j, so the store wants consecutive lanes on consecutive j: the block goes out
//             transposed through a 16 x 17 tile in the group buffer, every global access a run of 16 consecutive elements, predicated
//             on t < D and j < Q.
template <class T, int NT, bool FULL>
__device__ __forceinline__ void multi_target_tile_body(const T *Bs, const T *Cs, const T *Ys, const T *As, int ntarget, int nquery, T *Al,
                                                       T *Qd, T *Ld, T *Lm, T *Mn, int *info, int n_rt, unsigned batch, T *panel, T *aq)
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

        // the load and the sweep the GP tile kernels share (spd_sweep.hpp): W = -M^-1 in the lower tiles, diagonal tiles complete; the
        // four pivots of each block step are folded where they are formed (a step of identity padding folds four exact ones)
        vec4 acc[NT][NT];
        spd_load_lower<T, NT, FULL>(acc, A, Cs ? Cs + (size_t)mat * n : nullptr, n, q, c);
        unsigned long long bad = 0;
        int binfo = 0;  // column of the first non-positive pivot + 1
        PivotProduct<T> prod;
        spd_full_sweep<T, NT, FULL>(acc, panel, n, q, c, bad, binfo, [&](const PS &ps) { prod.fold(ps.d[0][0], ps.u11, ps.u22, ps.u33); });

        // ---- epilogue: W = -M^-1 in the lower tiles ------------------------------------------------------------------------------
        const bool ok = bad == 0;
        const T ld = prod.log_value();
        if (Ld && l == 0) Ld[mat] = ok ? ld : nan_of<T>();
        const int ngroups = (Al || Qd || Lm || Mn) ? (ntarget + 15) >> 4 : 0;  // wave-uniform; the targets are not read otherwise
        const int nqgroups = Mn ? (nquery + 15) >> 4 : 0;                       // nor the queries
        for (int g = 0; g < ngroups; ++g) {
            // lane coordinates and n opaque once per group: otherwise the offsets of the staging loads and of the LDS reads are hoisted
            // out of this loop and the allocator spills them beside the accumulators (as in predict_tile_body)
            int ng = n, lg = l, qg = q, cg = c;
            if (!FULL) asm volatile("" : "+s"(ng));
            asm volatile("" : "+v"(lg), "+v"(qg), "+v"(cg));
            const int left = ntarget - 16 * g;  // targets from this group's first on
            const size_t first = (size_t)mat * ntarget + 16 * (size_t)g;
            const T *Yg = Ys + first * ng;
            wave_lds_sync();  // the previous group's reads of aq and of the panel
            // the group's 16 n contiguous elements, consecutive lanes on consecutive elements of one vector
#pragma unroll
            for (int k = 0; k < N / 4; ++k) {
                const int e = lg + 64 * k, j = e / N, i = e - j * N;
                const bool in = (FULL || i < ng) && j < left;
                aq[j * NS + i] = in ? Yg[(unsigned)(j * ng + i)] : (T)0;
            }
            wave_lds_sync();
            T *const yc = aq + cg * NS;  // the vector of this lane's target
            vec4 tq[NT];
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int r = 0; r < 4; ++r) tq[ti][r] = (T)0;
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                // the block steps the sweep skipped hold identity padding, and y is zero there
                if (!FULL && kb > 4 * (NT - 1) && kb - 4 * (NT - 1) >= G::real_blocks(ng - 16 * (NT - 1))) continue;
                const int tK = kb >> 2, rK = kb & 3;
                wave_lds_sync();
                spd_panel_to_lds<NT, T>(panel, acc, kb, qg, cg);
                wave_lds_sync();
                const T b = yc[16 * tK + G::pcol(rK, qg)];
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) tq[ti] = G::mfma(panel[(16 * ti + cg) * 4 + qg], b, tq[ti]);
            }
            {
                T part[4] = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) part[r] = fma_t(tq[ti][r], yc[16 * ti + G::trow(r, qg)], part[r]);
                T s = (part[0] + part[1]) + (part[2] + part[3]);
                s += __shfl_xor(s, 16);
                s += __shfl_xor(s, 32);
                if (qg == 0 && cg < left) {
                    const T qd = -s;  // W = -K
                    if (Qd) Qd[first + cg] = ok ? qd : nan_of<T>();
                    // log 2 pi
                    if (Lm) Lm[first + cg] = ok ? (T)-0.5 * fma_t((T)ng, (T)1.83787706640934548356, qd + ld) : nan_of<T>();
                }
            }
            if (Al) {             // wave-uniform
                wave_lds_sync();  // the targets have been read: the buffer takes the group's alpha, vector by vector
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) yc[16 * ti + G::trow(r, qg)] = ok ? -tq[ti][r] : nan_of<T>();
                wave_lds_sync();
                // opaque once more: otherwise the offsets of these stores are formed above the T_g build and live through it (four
                // forms more spilled: profiles/multi_target_kernel_registers.txt)
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
                // opaque once per query group, for the reason given at the loop over g
                int nr = ng, lr = lg, qr = qg, cr = cg;
                if (!FULL) asm volatile("" : "+s"(nr));
                asm volatile("" : "+v"(lr), "+v"(qr), "+v"(cr));
                const int leftq = nquery - 16 * h;
                const T *Ah = As + ((size_t)mat * nquery + 16 * (size_t)h) * nr;
                wave_lds_sync();  // the previous block's reads of aq, the stores of alpha
#pragma unroll
                for (int k = 0; k < N / 4; ++k) {
                    const int e = lr + 64 * k, jj = e / N, i = e - jj * N;
                    const bool in = (FULL || i < nr) && jj < leftq;
                    aq[jj * NS + i] = in ? Ah[(unsigned)(jj * nr + i)] : (T)0;
                }
                wave_lds_sync();
                const T *const ar = aq + cr * NS;  // as the A operand lane (q, c) supplies row c of A_h^T
                vec4 cb;
#pragma unroll
                for (int r = 0; r < 4; ++r) cb[r] = (T)0;
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) cb = G::mfma(ar[16 * ti + G::trow(r, qr)], tq[ti][r], cb);
                // the block has consecutive lanes on consecutive targets, the store wants them on consecutive queries: through a
                // 16 x 17 tile in the group buffer, which is free once the MFMAs have read it. In the transposed layout lane (q, c)
                // serves query 16 h + c and target 16 g + trow(r, q).
                constexpr int TS = 17;  // 16 (N + 1) >= 16 * 17 elements
                wave_lds_sync();        // the A operands have been read
#pragma unroll
                for (int r = 0; r < 4; ++r) aq[G::trow(r, qr) * TS + cr] = ok ? -cb[r] : nan_of<T>();  // [query][target]; W = -K
                wave_lds_sync();
                const int jq = 16 * h + cr;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tl = G::trow(r, qr);
                    const T w = aq[cr * TS + tl];
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
        if (l == 0 && info) info[mat] = code;
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// The multi-target forms of matinv_spd_tile_f64 / matinv_spd_tile_f32 (tile_impl.hpp): the same names with a third to a tenth template
// argument. Launch bounds: those of the covariance forms for the same NT (predict_cov_tile_impl.hpp; the same live set: accumulators,
// T_g and one block), one wave per SIMD fewer where a form spills under them: beside that live set this form keeps the pivot product, the
// log-determinant, two more pointers and one more count, and under the covariance forms' bounds the full fp64 3 x 3 (6 registers) and
// 4 x 4 (2) forms and the full fp32 6 x 6 form (4) spilled (profiles/multi_target_kernel_registers.txt). No form uses scratch.
constexpr int multi_target_f64_waves(int nt, bool full)
{
    const bool spills = (nt == 3 || nt == 4) && full;
    return predict_cov_f64_waves(nt, full) - (spills ? 1 : 0);
}
constexpr int multi_target_f32_waves(int nt, bool full)
{
    const bool spills = nt == 6 && full;
    return predict_cov_f32_waves(nt, full) - (spills ? 1 : 0);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI>
__global__ __launch_bounds__(64, multi_target_f64_waves(NT, FULL)) void matinv_spd_tile_f64(const double *Bs, const double *Cs,
                                                                                             const double *Ys, const double *As, int ntarget,
                                                                                             int nquery, double *Al, double *Qd, double *Ld,
                                                                                             double *Lm, double *Mn, int *info, int n_rt,
                                                                                             unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN && MULTI, "the ten-argument form is the multi-target kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    __shared__ double aq[16 * predict_qstride(16 * NT)];
    multi_target_tile_body<double, NT, FULL>(Bs, Cs, Ys, As, ntarget, nquery, Al, Qd, Ld, Lm, Mn, info, n_rt, batch, panel, aq);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI>
__global__ __launch_bounds__(64, multi_target_f32_waves(NT, FULL)) void matinv_spd_tile_f32(const float *Bs, const float *Cs, const float *Ys,
                                                                                             const float *As, int ntarget, int nquery,
                                                                                             float *Al, float *Qd, float *Ld, float *Lm,
                                                                                             float *Mn, int *info, int n_rt, unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN && MULTI, "the ten-argument form is the multi-target kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    __shared__ float aq[16 * predict_qstride(16 * NT)];
    multi_target_tile_body<float, NT, FULL>(Bs, Cs, Ys, As, ntarget, nquery, Al, Qd, Ld, Lm, Mn, info, n_rt, batch, panel, aq);
}

template <class T>
hipError_t launch_multi_target_tile(int n, int ntarget, int nquery, const T *Bs, const T *Cs, const T *Ys, const T *As, T *Al, T *Qd, T *Ld,
                                    T *Lm, T *Mn, size_t batch, int *info, hipStream_t stream)
{
    if (!multi_target_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = predict_tile_grid(batch), b = (unsigned)batch;  // 256 * 12 workgroups a round (predict_tile_impl.hpp)
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true, true, true, true, true, true, true>), dim3(grid), dim3(64), 0, stream,
                               Bs, Cs, Ys, As, ntarget, nquery, Al, Qd, Ld, Lm, Mn, info, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true, true, true, true, true, true, true>), dim3(grid), dim3(64), 0, stream,
                               Bs, Cs, Ys, As, ntarget, nquery, Al, Qd, Ld, Lm, Mn, info, n, b);
    });
    return hipGetLastError();
}
}  // namespace matinv
