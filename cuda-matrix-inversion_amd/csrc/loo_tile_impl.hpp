// loo_tile_impl.hpp (instantiated by loo_tile_kernels.hip for f64 and loo_tile_f32_kernels.hip for f32) -- batched leave-one-out
// cross-validation of a Gaussian process (Rasmussen & Williams 5.4.2) on the MFMA tile layout, n <= 96. With M = B + diag c
// (c optional), kappa_i = [M^-1]_ii and alpha = M^-1 d:
//     mean_i = d_i - alpha_i / kappa_i      var_i = 1 / kappa_i      logpl = sum_i (1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i) - n/2 log(2 pi)
// The load, the PanelSolve pipeline and the block-step loop are spd_load_lower and spd_full_sweep of spd_sweep.hpp, which the later GP
// tile kernels call, kept HERE as a copy of their own: called from the shared header, the ragged fp32 4 x 4 form, which fills its 96
// registers to the last one, spilled 7 of them to scratch ("The shared SPD sweep"). A change to the sweep is made there and
// here. One wavefront per matrix, lower-triangular 16 x 16 accumulator tiles, the next
// block's panel solved between the MFMAs of the current one. The sweep ends with W = -M^-1 in the lower tiles (diagonal tiles
// complete); the epilogue folds diag W and W d out of the registers, so neither M nor its inverse is ever stored.
// HBM traffic per matrix: n^2 / 2 + 2 n elements in, 2 n + 1 out.
// A non-positive (or NaN) pivot makes info = its column + 1 (PanelSolve::binfo, as in logdet_tile_body) and every output NaN: no
// fallback launch.
//
// The kernels are the LOO forms of the SPD inversion kernels whose sweep they run: overloads of matinv_spd_tile_f64 / _f32 with one
// more trailing template argument ("Leave-one-out cross-validation", says why).
#pragma once
#include <cstdio>

#include "tile_common.hpp"

namespace matinv {

__device__ __forceinline__ double loo_log(double v) { return log(v); }
__device__ __forceinline__ float loo_log(float v) { return logf(v); }

// Epilogue layout (lane l = 16 q + c; the lane holds W[16 ti + trow(r, q)][16 tj + c] in acc[ti][tj][r], tj <= ti):
//   LDS, in the panel buffer (4 N elements, free after the last block step):  sd[N] = d (zero beyond n),  rs[N] = row part of W d,
//   kap[N] = -W_ii.
//   row part   : (W d)_row over the stored tiles of tile row ti -- a sum over the lane's column c, reduced across the 16 c lanes
//   mirror part: the tiles right of the diagonal are not stored; tile (ti, tj), ti > tj, stands for them: its column 16 tj + c
//                collects acc * d[row] over the lane's rows, reduced across the four q groups
// After that every lane holds, for each tj, alpha and kappa of index 16 tj + c; lane group q = 0 writes mean and var as 16-element
// segments and the 16 c lanes reduce logpl.
template <class T, int NT, bool FULL>
__device__ __forceinline__ void loo_tile_body(const T *Bs, const T *Cs, const T *Ds, T *mean, T *var, T *logpl, int *info, int n_rt,
                                              unsigned batch, T *panel)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    constexpr int N = 16 * NT;
    constexpr int NKB = 4 * NT;
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
                constexpr int NS = PS::NSTAGE;
                T aop_next[NT], bop_next[NT];
                PS ps;
                ps.binfo = &binfo;
                int count = 0, ev = 0;  // MFMAs of (b) issued so far; next event (0 = stage the panel, 1 + s = stage s)
                auto run_events = [&](bool flush) {
#pragma unroll
                    for (int e = 0; e < NS + 1; ++e) {
                        const int lead = NB < 2 ? NB : 2;
                        const int thr = (e == 0) ? lead : lead + ((NB - lead) * e) / NS;
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
        const T *vd = Ds + (size_t)mat * n;
        wave_lds_sync();  // the last panel has been consumed
        T *const sd = panel, *const rs = panel + N, *const kap = panel + 2 * N;
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
#pragma unroll
                for (int off = 1; off <= 8; off <<= 1) rowacc[r] += __shfl_xor(rowacc[r], off);
                if (c == 0) rs[16 * ti + G::trow(r, q)] = rowacc[r];
                if (G::trow(r, q) == c) kap[16 * ti + c] = -acc[ti][ti][r];  // the one lane that holds W_ii
            }
        }
#pragma unroll
        for (int tj = 0; tj < NT - 1; ++tj) {
            colacc[tj] += __shfl_xor(colacc[tj], 16);
            colacc[tj] += __shfl_xor(colacc[tj], 32);
        }
        wave_lds_sync();
        const bool ok = bad == 0;
        T term = (T)0;
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
            const int i = 16 * tj + c;
            const bool in = FULL || tj < NT - 1 || i < n;
            const T alpha = -(rs[i] + colacc[tj]);  // W = -M^-1
            const T kappa = kap[i];
            const T rk = (T)1 / kappa;
            const T t = alpha * rk;
            if (in) term += (T)0.5 * loo_log(kappa) - (T)0.5 * alpha * t;
            if (in && q == 0) {
                if (mean) mean[(size_t)mat * n + i] = ok ? sd[i] - t : nan_of<T>();
                if (var) var[(size_t)mat * n + i] = ok ? rk : nan_of<T>();
            }
        }
#pragma unroll
        for (int off = 1; off <= 8; off <<= 1) term += __shfl_xor(term, off);
        if (l == 0) {
            if (logpl) logpl[mat] = ok ? term - (T)n * (T)0.91893853320467274178 : nan_of<T>();
            if (info) info[mat] = binfo;
        }
        if constexpr (sizeof(T) == 4) {
            // Rejected matrices only (wave-uniform): the fp32 tile order does not say which column fails FIRST (tile_common.hpp), so info
            // is written once more, in a block of its own after the stores.
            if (bad != 0 && info) {
                const int nat = spd_natural_first_failure<NT, T>(Bs + (size_t)mat * n * n, Cs ? Cs + (size_t)mat * n : nullptr, n, panel, l);
                if (nat && l == 0) info[mat] = nat;
            }
        }
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// fp32, 4 x 4 tiles: built for FIVE waves per SIMD, which is what its 94 / 96 registers gave it under the bound of four -- with the
// natural-order pass behind the sweep the ragged form came out at 97 registers (104 allocated: four waves) under that bound, inlined
// or not, wherever the pass was placed; under the bound of five it is 96 again, without scratch (profiles/loo_kernel_registers.txt).
// The LOO forms of matinv_spd_tile_f64 / matinv_spd_tile_f32 (tile_impl.hpp): the same names with a third template argument, the
// same launch bounds for the same NT -- except the two fp64 ragged forms that spill under them (3 x 3 tiles at four waves per SIMD: 2
// registers, 6 x 6 at two: 8; profiles/loo_kernel_registers.txt), which take one wave less per SIMD and no scratch.
constexpr int loo_f64_waves(int nt, bool full)
{
    const int inverse = nt >= 5 ? 2 : (nt >= 4 ? 3 : 4);  // matinv_spd_tile_f64<NT, FULL>
    return inverse - ((!full && (nt == 3 || nt == 6)) ? 1 : 0);
}
template <int NT, bool FULL, bool LOO>
__global__ __launch_bounds__(64, loo_f64_waves(NT, FULL)) void matinv_spd_tile_f64(const double *Bs, const double *Cs, const double *Ds,
                                                                                          double *mean, double *var, double *logpl, int *info,
                                                                                          int n_rt, unsigned batch)
{
    static_assert(LOO, "the three-argument form is the leave-one-out kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    loo_tile_body<double, NT, FULL>(Bs, Cs, Ds, mean, var, logpl, info, n_rt, batch, panel);
}

template <int NT, bool FULL, bool LOO>
__global__ __launch_bounds__(64, NT >= 5 ? 3 : (NT == 4 ? 5 : 4)) void matinv_spd_tile_f32(const float *Bs, const float *Cs, const float *Ds, float *mean,
                                                                          float *var, float *logpl, int *info, int n_rt, unsigned batch)
{
    static_assert(LOO, "the three-argument form is the leave-one-out kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    loo_tile_body<float, NT, FULL>(Bs, Cs, Ds, mean, var, logpl, info, n_rt, batch, panel);
}

template <class T>
hipError_t launch_loo_tile(int n, const T *Bs, const T *Cs, const T *Ds, T *mean, T *var, T *logpl, size_t batch, int *info,
                           hipStream_t stream)
{
    if (!loo_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = tile_grid(batch, 12u), b = (unsigned)batch;
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true>), dim3(grid), dim3(64), 0, stream, Bs, Cs, Ds, mean, var, logpl, info, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true>), dim3(grid), dim3(64), 0, stream, Bs, Cs, Ds, mean, var, logpl, info, n, b);
    });
    return hipGetLastError();
}
}  // namespace matinv
