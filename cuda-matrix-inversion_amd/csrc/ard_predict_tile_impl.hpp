// ard_predict_tile_impl.hpp (instantiated by ard_predict_tile_kernels.hip for f64 and ard_predict_tile_f32_kernels.hip for f32) -- GP
// prediction from COORDINATES on the MFMA tile layout, n <= 96: the covariance matrix AND the cross-covariance vectors of the queries are
// generated inside the kernel from n points and Q query points in d <= 16 dimensions and d + 2 hyperparameters. With theta, z = x / l, s,
// phi and M = sf2 phi(s) + sn2 I exactly as ard_tile_impl.hpp has them, K = M^-1, alpha = K y, zq_j = xq_j / l:
//     a_j[i] = sf2 phi(sum_k (z_ik - zq_jk)^2)        mean[j] = a_j^T alpha        var[j] = sf2 - a_j^T K a_j
// var is the variance of the latent function and is not clamped. Neither M, nor K, nor a cross-covariance vector reaches memory.
// HBM traffic per matrix: n d + n + d + 2 + Q d elements in, 2 Q out (a shared point set, target vector or query set is read through L2).
//
// CALLED from the kernels this one joins: ard_generate_lower, ard_natural_first_failure (ard_tile_impl.hpp), ard_m (ard_element.hpp),
// spd_full_sweep, spd_panel_to_lds (spd_sweep.hpp, tile_common.hpp), dpp_row_sum16, predict_tile_grid, predict_qstride.
// WRITTEN HERE, because the bodies they sit in are one function each and are not split (splitting them would have to leave the text of
// twenty-four compiled kernels unchanged):
//   * the prologue of ard_tile_body -- the same operations (exp theta, z = x / l dimension-major in LDS, zero beyond n), except that the
//     length scales go to 16 elements of LDS of their own (ell), since every query group needs them after the sweep has overwritten the
//     panel buffer, and that y is read with mean only;
//   * the alpha step of ard_tile_body / predict_tile_body (they are the same operations in the same order), without kappa, y^T alpha and
//     the store of alpha; alpha goes to al[N] because the panel buffer is reused by every group;
//   * the query-group loop of predict_tile_body, as it is, except that the staging loads from As are replaced by GENERATION: per group the
//     16 d query coordinates are divided by l into zq[k 16 + j] (zero beyond Q), then every lane produces its N / 4 elements of
//     aq[j (N + 1) + i] as ard_m(s, kind, sf2, sn2, false), s summed over k in the order of ard_tile_s with the rolled k loop and one
//     ard_pin per element; entries beyond n and beyond Q are zero. A query that coincides with a training point gets s = 0 exactly.
// No pivot fold: log det M is no output. A non-positive (or NaN) pivot makes info = its column + 1 (PanelSolve::binfo; fp32:
// ard_natural_first_failure, the value matinv_ard_logml_batched reports) and every requested output NaN: no fallback launch. A NaN in a
// QUERY's coordinates makes that query's a_j NaN and with it column j of T = W A and its two outputs, nothing else: every lane column of
// an MFMA is computed alike and on its own.
//
// The kernels are overloads of matinv_logdet_tile_f64 / _f32 with a fourth template argument ("Prediction from coordinates",
// says why this family leaves the naming rule of the SPD tile forms).
#pragma once
#include "ard_tile_impl.hpp"     // ard_generate_lower, ard_natural_first_failure, the launch bounds of the ARD forms
#include "predict_tile_impl.hpp"  // predict_qstride, predict_tile_grid

namespace matinv {

// LDS of one workgroup in elements: panel 4 N, z 16 N, y N, alpha N, aq 16 (N + 1), zq 256, l 16
constexpr int ard_predict_lds_elems(int nt) { return 38 * 16 * nt + 16 + 256 + 16; }
// Waves per SIMD: the bound of the ARD form of the same shape, or what the 160 KB of LDS of a compute unit hold (four SIMDs, one
// wave per workgroup) where that is less -- a launch bound above the LDS residency only takes registers away from the kernel.
constexpr int ard_predict_lds_waves(int nt, int size) { return (160 * 1024 / (ard_predict_lds_elems(nt) * size)) / 4; }
constexpr int ard_predict_min(int a, int b) { return a < b ? a : (b < 1 ? 1 : b); }
constexpr int ard_predict_f64_waves(int nt, bool full) { return ard_predict_min(nt >= 6 ? 1 : ard_f64_waves(nt, full), ard_predict_lds_waves(nt, 8)); }
constexpr int ard_predict_f32_waves(int nt, bool full) { return ard_predict_min(ard_f32_waves(nt, full), ard_predict_lds_waves(nt, 4)); }

// Layout (lane l = 16 q + c; the lane holds W[16 ti + trow(r, q)][16 tj + c] in acc[ti][tj][r], tj <= ti):
//   LDS: panel[4 N] (the sweep's; y's row part during the alpha step; the panel of each block step again in every group),
//        zs[16 N] = z, dimension k at zs + k N, ys[N] = y (both zero beyond n), al[N] = alpha, ell[16] = the length scales,
//        zq[256] = the current group's query coordinates over l, dimension k at zq + 16 k, aq[16 (N + 1)] = its 16 vectors a_j.
template <class T, int NT, bool FULL>
__device__ __forceinline__ void ard_predict_tile_body(const T *Xs, size_t xstride, const T *Ys, size_t ystride, const T *Th, const T *Xqs,
                                                      size_t xqstride, int nquery, int ndim, int kind, T *mean, T *var, int *info, int n_rt,
                                                      unsigned batch, T *panel, T *zs, T *ys, T *al, T *aq, T *zq, T *ell)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    constexpr int N = 16 * NT;
    constexpr int NKB = 4 * NT;
    constexpr int NS = predict_qstride(N);
    const int l = threadIdx.x;

    for (unsigned mat = blockIdx.x; mat < batch; mat += gridDim.x) {
        int n = FULL ? N : n_rt;  // run-time n opaque once per matrix, predicates on the edge tiles only: see gj_tile_body
        if (!FULL) asm volatile("" : "+s"(n));
        int q = l >> 4, c = l & 15;
        asm volatile("" : "+v"(q), "+v"(c));  // see matinv_gj_tile_f64

        // ---- prologue (ard_tile_body's): exp theta once per matrix, z = x / l and y to LDS -------------------------------------------
        const T *th = Th + (size_t)mat * (ndim + 2);
        const T sf2 = ard_exp(th[0]), sn2 = ard_exp(th[ndim + 1]);
        if (l < ndim) ell[l] = ard_exp(th[1 + l]);
        wave_lds_sync();
        {
            const T *X = Xs + (size_t)mat * xstride;
            const int nd = n * ndim;
            // consecutive lanes on consecutive elements of the point-major block; the slots beyond n are zeroed below
            for (int e = l; e < nd; e += 64) {
                const int i = e / ndim, k = e - i * ndim;
                zs[k * N + i] = X[e] / ell[k];
            }
            if (!FULL)
                for (int e = l; e < (N - n) * ndim; e += 64) {
                    const int k = e / (N - n), i = n + (e - k * (N - n));
                    zs[k * N + i] = (T)0;
                }
            if (mean) {  // wave-uniform: y is read for alpha only
                const T *Y = Ys + (size_t)mat * ystride;
#pragma unroll
                for (int k = 0; k < (N + 63) / 64; ++k) {
                    const int i = l + 64 * k;
                    if (i < N) ys[i] = (FULL || i < n) ? Y[i] : (T)0;
                }
            }
        }
        wave_lds_sync();

        // ---- generate (in place of spd_load_lower) and sweep: W = -M^-1 in the lower tiles ---------------------------------------------
        vec4 acc[NT][NT];
        ard_generate_lower<T, NT, FULL>(acc, zs, ndim, kind, sf2, sn2, n, q, c);
        unsigned long long bad = 0;
        int binfo = 0;  // column of the first non-positive pivot + 1
        spd_full_sweep<T, NT, FULL>(acc, panel, n, q, c, bad, binfo);

        // ---- alpha = -W y to LDS (the row and mirror parts of ard_tile_body) ----------------------------------------------------------
        const bool ok = bad == 0;
        if (mean) {          // wave-uniform
            wave_lds_sync();  // the last panel has been consumed
            T *const rs = panel;
            T colacc[NT];
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) colacc[tj] = (T)0;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                T rowacc[4] = {(T)0, (T)0, (T)0, (T)0};
                T dr[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) dr[r] = ys[16 * ti + G::trow(r, q)];
#pragma unroll
                for (int tj = 0; tj <= ti; ++tj) {
                    const T dc = ys[16 * tj + c];
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

        // ---- the queries in groups of 16 (predict_tile_body's loop; the staging loads replaced by generation) -------------------------
        const int ngroups = (nquery + 15) >> 4;
        const T *const Xq = Xqs + (size_t)mat * xqstride;
        for (int g = 0; g < ngroups; ++g) {
            // lane coordinates and n opaque once per group: otherwise the offsets of the LDS accesses are hoisted out of this loop and the
            // allocator spills them beside the accumulators (as in the loop over p of logml_grad_tile_body)
            int ng = n, lg = l, qg = q, cg = c;
            if (!FULL) asm volatile("" : "+s"(ng));
            asm volatile("" : "+v"(lg), "+v"(qg), "+v"(cg));
            const int left = nquery - 16 * g;  // queries from this group's first on
            const size_t first = (size_t)mat * nquery + 16 * (size_t)g;
            const T *const xg = Xq + 16 * (size_t)g * ndim;
            wave_lds_sync();  // the previous group's reads of aq and zq, this matrix's writes of al
            // the group's 16 ndim contiguous coordinates over l, consecutive lanes on consecutive elements; zero beyond Q
            for (int e = lg; e < 16 * ndim; e += 64) {
                const int j = e / ndim, k = e - j * ndim;
                zq[k * 16 + j] = j < left ? xg[e] / ell[k] : (T)0;
            }
            wave_lds_sync();
            // a_j[i] for the lane's N / 4 elements, four at a time; consecutive lanes on consecutive points of one query
#pragma unroll 1
            for (int k4 = 0; k4 < N / 16; ++k4) {
                int jj[4], ii[4];
                T s[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = lg + 64 * (4 * k4 + r);
                    jj[r] = e / N;
                    ii[r] = e - jj[r] * N;
                    s[r] = (T)0;
                }
#pragma unroll 1
                for (int k = 0; k < ndim; ++k) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const T d = zs[k * N + ii[r]] - zq[k * 16 + jj[r]];
                        s[r] = fma_t(d, d, s[r]);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool in = (FULL || ii[r] < ng) && jj[r] < left;
                    T v = ard_m(s[r], kind, sf2, sn2, false);
                    v = in ? v : (T)0;
                    ard_pin(v);  // one element at a time, where its distance is (ard_generate_lower)
                    aq[jj[r] * NS + ii[r]] = v;
                }
            }
            wave_lds_sync();
            const T *const ac = aq + cg * NS;  // the vector of this lane's query
            if (var) {                         // wave-uniform
                T part[4] = {(T)0, (T)0, (T)0, (T)0};
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
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) part[r] = fma_t(tq[ti][r], ac[16 * ti + G::trow(r, qg)], part[r]);
                T s = (part[0] + part[1]) + (part[2] + part[3]);
                s += __shfl_xor(s, 16);
                s += __shfl_xor(s, 32);
                if (qg == 0 && cg < left) var[first + cg] = ok ? sf2 + s : nan_of<T>();  // W = -K
            }
            if (mean) {  // wave-uniform
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
        }
        int code = binfo;
        if constexpr (sizeof(T) == 4) {
            if (bad != 0) {  // wave-uniform; rejected matrices only: the fp32 tile order does not say which column fails FIRST (tile_common.hpp)
                wave_lds_sync();  // the last group's reads of the panel
                const int nat = ard_natural_first_failure<NT, T>(zs, ndim, kind, sf2, sn2, n, panel, l);
                if (nat) code = nat;
            }
        }
        if (l == 0 && info) info[mat] = code;
        wave_lds_sync();  // the next matrix's first LDS writes must not pass this one's last reads
    }
}

#define MATINV_ARD_PREDICT_LDS(T)                                             \
    __shared__ __attribute__((aligned(16))) T panel[16 * NT * 4];            \
    __shared__ T zs[ARD_MAX_DIM * 16 * NT], ys[16 * NT], al[16 * NT];         \
    __shared__ T aq[16 * predict_qstride(16 * NT)], zq[16 * ARD_MAX_DIM], ell[ARD_MAX_DIM]

template <int NT, bool FULL, bool BORDER, bool ARDPREDICT>
__global__ __launch_bounds__(64, ard_predict_f64_waves(NT, FULL)) void matinv_logdet_tile_f64(
    const double *Xs, size_t xstride, const double *Ys, size_t ystride, const double *Th, const double *Xqs, size_t xqstride, int nquery,
    int ndim, int kind, double *mean, double *var, int *info, int n_rt, unsigned batch)
{
    static_assert(BORDER && ARDPREDICT, "the four-argument form is the prediction-from-coordinates kernel");
    MATINV_ARD_PREDICT_LDS(double);
    ard_predict_tile_body<double, NT, FULL>(Xs, xstride, Ys, ystride, Th, Xqs, xqstride, nquery, ndim, kind, mean, var, info, n_rt, batch,
                                            panel, zs, ys, al, aq, zq, ell);
}

template <int NT, bool FULL, bool BORDER, bool ARDPREDICT>
__global__ __launch_bounds__(64, ard_predict_f32_waves(NT, FULL)) void matinv_logdet_tile_f32(
    const float *Xs, size_t xstride, const float *Ys, size_t ystride, const float *Th, const float *Xqs, size_t xqstride, int nquery, int ndim,
    int kind, float *mean, float *var, int *info, int n_rt, unsigned batch)
{
    static_assert(BORDER && ARDPREDICT, "the four-argument form is the prediction-from-coordinates kernel");
    MATINV_ARD_PREDICT_LDS(float);
    ard_predict_tile_body<float, NT, FULL>(Xs, xstride, Ys, ystride, Th, Xqs, xqstride, nquery, ndim, kind, mean, var, info, n_rt, batch,
                                           panel, zs, ys, al, aq, zq, ell);
}
#undef MATINV_ARD_PREDICT_LDS

template <class T>
hipError_t launch_ard_predict_tile(int kind, int n, int ndim, int nquery, const T *Xs, size_t xstride, const T *Ys, size_t ystride,
                                   const T *Th, const T *Xqs, size_t xqstride, T *mean, T *var, size_t batch, int *info, hipStream_t stream)
{
    if (!ard_predict_tile_supports(n) || ndim < 1 || ndim > ARD_MAX_DIM || nquery < 1) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = predict_tile_grid(batch), b = (unsigned)batch;  // the grid of the prediction forms
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_logdet_tile_f64<NT, FULL, true, true>), dim3(grid), dim3(64), 0, stream, Xs, xstride, Ys, ystride, Th,
                               Xqs, xqstride, nquery, ndim, kind, mean, var, info, n, b);
        else
            hipLaunchKernelGGL((matinv_logdet_tile_f32<NT, FULL, true, true>), dim3(grid), dim3(64), 0, stream, Xs, xstride, Ys, ystride, Th,
                               Xqs, xqstride, nquery, ndim, kind, mean, var, info, n, b);
    });
    return hipGetLastError();
}
}  // namespace matinv
