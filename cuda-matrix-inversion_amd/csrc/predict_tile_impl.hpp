// predict_tile_impl.hpp (instantiated by predict_tile_kernels.hip for f64 and predict_tile_f32_kernels.hip for f32) -- GP prediction at
// many query points per covariance matrix on the MFMA tile layout, n <= 96. With M = B + diag c (c optional), K = M^-1, alpha = K d and Q
// query points per matrix, a_j the cross-covariance vector of query j and e_j its prior variance:
//     mean[j] = a_j^T alpha      var[j] = e_j - a_j^T K a_j
// The load, the PanelSolve pipeline and the block-step loop are spd_load_lower and spd_full_sweep (spd_sweep.hpp), shared with the LOO
// and the gradient kernels. The sweep ends with W = -M^-1 in
// the lower tiles (diagonal tiles complete); the epilogue folds alpha = -W d out of the registers as the gradient epilogue does, then
// takes the queries in groups of 16: a group is an N x 16 right-hand side, so T = W A is MFMA work, and neither M nor its inverse is
// ever stored.
// HBM traffic per matrix: n^2 / 2 + 2 n + Q (n + 1) elements in, 2 Q out.
// A non-positive (or NaN) pivot makes info = its column + 1 (PanelSolve::binfo) and every output NaN: no fallback launch.
//
// The kernels are the prediction forms of the SPD inversion kernels whose sweep they run: overloads of matinv_spd_tile_f64 / _f32 with
// three more trailing template arguments ("Prediction at many query points", says why).
#pragma once
#include "logml_grad_tile_impl.hpp"  // dpp_row_sum16, the launch bounds of the gradient forms

namespace matinv {

// Row stride of the staged query vectors in LDS: N + 1, so that the 16 lanes of a q group, which read 16 different vectors at one row
// index, fall into 16 different banks (odd stride) instead of one.
constexpr int predict_qstride(int n_pad) { return n_pad + 1; }

// Epilogue layout (lane l = 16 q + c; the lane holds W[16 ti + trow(r, q)][16 tj + c] in acc[ti][tj][r], tj <= ti):
//   LDS: panel[4 N] (the sweep's; d and the row part of W d during the alpha step, then the panel of each block step again),
//        al[N] = alpha, aq[16 (N + 1)] = the 16 query vectors of the current group, vector j at aq + j (N + 1), zero beyond n and
//        beyond Q.
//   alpha : as in logml_grad_tile_body -- row part over the 16 c lanes by DPP, mirror part over the four q groups. Skipped (and d not
//           read) when mean is not asked for.
//   T = W A, N x 16, one vec4 per tile row: for every real block step kb the four columns of W that block holds go to the LDS panel
//           (spd_panel_to_lds writes all N rows of them, the rows above the diagonal tile by symmetry), lane (q, c) takes
//           W[16 ti + c][pivot q] as the A operand and a_c[pivot q] as the B operand: 4 NT^2 MFMAs per group. Lane (q, c) then holds
//           T[16 ti + trow(r, q)][query c], i.e. only values of ITS query c.
//   var   : s = sum_ti sum_r T[ti][r] a_c[16 ti + trow(r, q)] in four chains by register r, ((p0 + p1) + (p2 + p3)), the four q groups
//           by two __shfl_xor (16, 32); var = e + s because W = -K. No reduction over the 16 c lanes: each is another query.
//   mean  : the same reduction of a_c[row] alpha[row].
//   Lane group q = 0 stores the 16 results as one segment, predicated on j < Q. The order of operations for query j knows nothing of
//   batch, grid, Q or the position of j in its group (every lane column of an MFMA is computed alike).
template <class T, int NT, bool FULL>
__device__ __forceinline__ void predict_tile_body(const T *Bs, const T *Cs, const T *Ds, const T *As, int nquery, const T *Es, T *mean,
                                                  T *var, int *info, int n_rt, unsigned batch, T *panel, T *al, T *aq)
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
        const T *A = Bs + (size_t)mat * n * n;
        int q = l >> 4, c = l & 15;
        asm volatile("" : "+v"(q), "+v"(c));  // see matinv_gj_tile_f64

        // the load and the sweep the GP tile kernels share (spd_sweep.hpp): W = -M^-1 in the lower tiles, diagonal tiles complete
        vec4 acc[NT][NT];
        spd_load_lower<T, NT, FULL>(acc, A, Cs ? Cs + (size_t)mat * n : nullptr, n, q, c);
        unsigned long long bad = 0;
        int binfo = 0;  // column of the first non-positive pivot + 1
        spd_full_sweep<T, NT, FULL>(acc, panel, n, q, c, bad, binfo);

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
                if (qg == 0 && cg < left) {
                    const T e = Es ? Es[first + cg] : (T)0;
                    var[first + cg] = ok ? e + s : nan_of<T>();
                }
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
                const int nat = spd_natural_first_failure<NT, T>(A, Cs ? Cs + (size_t)mat * n : nullptr, n, panel, l);
                if (nat) code = nat;
            }
        }
        if (l == 0 && info) info[mat] = code;
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// The prediction forms of matinv_spd_tile_f64 / matinv_spd_tile_f32 (tile_impl.hpp): the same names with a third, a fourth and a fifth
// template argument, the launch bounds of the gradient forms for the same NT (logml_grad_tile_impl.hpp) -- except the full fp64 6 x 6
// form, which spills under them beside its NT more accumulators (170 registers at two waves per SIMD; still 20 with T built one tile
// row at a time: profiles/predict_kernel_registers.txt) and takes one wave per SIMD like the ragged one, and no scratch.
constexpr int predict_f64_waves(int nt, bool full) { return nt >= 6 ? 1 : logml_grad_f64_waves(nt, full); }
constexpr int predict_f32_waves(int nt, bool full) { return logml_grad_f32_waves(nt, full); }

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT>
__global__ __launch_bounds__(64, predict_f64_waves(NT, FULL)) void matinv_spd_tile_f64(const double *Bs, const double *Cs, const double *Ds,
                                                                                              const double *As, int nquery, const double *Es,
                                                                                              double *mean, double *var, int *info, int n_rt,
                                                                                              unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT, "the five-argument form is the prediction kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    __shared__ double al[16 * NT], aq[16 * predict_qstride(16 * NT)];
    predict_tile_body<double, NT, FULL>(Bs, Cs, Ds, As, nquery, Es, mean, var, info, n_rt, batch, panel, al, aq);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT>
__global__ __launch_bounds__(64, predict_f32_waves(NT, FULL)) void matinv_spd_tile_f32(const float *Bs, const float *Cs, const float *Ds,
                                                                                              const float *As, int nquery, const float *Es,
                                                                                              float *mean, float *var, int *info, int n_rt,
                                                                                              unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT, "the five-argument form is the prediction kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    __shared__ float al[16 * NT], aq[16 * predict_qstride(16 * NT)];
    predict_tile_body<float, NT, FULL>(Bs, Cs, Ds, As, nquery, Es, mean, var, info, n_rt, batch, panel, al, aq);
}

// The grid of the prediction forms and of the covariance forms built on them (predict_cov_tile_impl.hpp): one place, so that what
// tests/test_grid_stride_cpu.py reads here holds for both launch sites.
inline unsigned predict_tile_grid(size_t batch) { return tile_grid(batch, 12u); }

template <class T>
hipError_t launch_predict_tile(int n, int nquery, const T *Bs, const T *Cs, const T *Ds, const T *As, const T *Es, T *mean, T *var,
                               size_t batch, int *info, hipStream_t stream)
{
    if (!predict_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = predict_tile_grid(batch), b = (unsigned)batch;
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true, true>), dim3(grid), dim3(64), 0, stream, Bs, Cs, Ds, As, nquery, Es,
                               mean, var, info, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true, true>), dim3(grid), dim3(64), 0, stream, Bs, Cs, Ds, As, nquery, Es,
                               mean, var, info, n, b);
    });
    return hipGetLastError();
}
}  // namespace matinv
