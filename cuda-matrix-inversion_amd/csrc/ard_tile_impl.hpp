// ard_tile_impl.hpp (instantiated by ard_tile_kernels.hip for f64 and ard_tile_f32_kernels.hip for f32) -- the GP log marginal likelihood
// and its gradient from COORDINATES on the MFMA tile layout, n <= 96: the covariance matrix is generated in registers from n points in
// d <= 16 dimensions and d + 2 hyperparameters, theta = (log sf2, log l_1 .. log l_d, log sn2). With z_ik = x_ik / l_k and
// s_ij = sum_k (z_ik - z_jk)^2 (k = 0 .. d - 1 in this order):
//     M_ij = sf2 phi(s_ij) + sn2 delta_ij        K = M^-1      alpha = K y      G = alpha alpha^T - K
//     logml     = -1/2 y^T alpha - 1/2 log det M - n/2 log 2 pi
//     grad[0]   = 1/2 sum_ij G_ij sf2 phi(s_ij)                      d / d log sf2
//     grad[1+k] = 1/2 sum_ij G_ij sf2 psi(s_ij) (z_ik - z_jk)^2      d / d log l_k        psi = -2 phi'
//     grad[d+1] = 1/2 sn2 sum_i G_ii                                 d / d log sn2
// phi and psi are those of ard_element (ard_element.hpp: squared exponential, Matern 5/2). Neither M nor K nor a derivative matrix
// reaches memory.
// The sweep is spd_full_sweep of spd_sweep.hpp, called as multi_target_tile_body calls it (the pivots folded into a PivotProduct where
// they are formed); in place of spd_load_lower every lane GENERATES the elements it owns from z in LDS. The epilogue takes alpha and kappa
// out of W = -K as logml_grad_tile_body does, turns the accumulators into G, and then
//   * one pass over the accumulators regenerates s_ij tile by tile, adds w G_ij sf2 phi into grad[0] and G_ii into grad[d + 1] and leaves
//     w G_ij sf2 psi(s_ij) in place (w = 1/2 in the diagonal tiles, which hold both triangles, 1 in the strictly lower ones, each of
//     which stands for its mirror): one transcendental per element per matrix, whatever d is;
//   * one pass of plain FMAs per dimension k: sum acc_ij (z_ik - z_jk)^2. No per-dimension accumulator registers.
// Every reduction is that of the contraction of logml_grad_tile_body: four chains by register r, ((p0 + p1) + (p2 + p3)), the 16 c lanes
// by dpp_row_sum16, the four q groups by two __shfl_xor, lane 0 stores. Nothing in the order of operations of an output depends on batch,
// grid, the strides or which outputs are requested (wave-uniform pointers decide what is stored; the gradient passes run with grad only).
// HBM traffic per matrix: n d + n + d + 2 elements in, d + 3 + n out (a shared point set or target vector is read through L2).
// A non-positive (or NaN) pivot makes info = its column + 1 (PanelSolve::binfo; fp32: the natural-order redo on regenerated tiles,
// ard_natural_first_failure) and every requested output NaN: no fallback launch.
//
// The kernels are overloads of matinv_spd_tile_f64 / _f32 with thirteen more trailing template arguments ("Hyperparameter fits
// from coordinates"). The covariance function is a wave-uniform run-time argument: it only selects the two polynomial factors in front of
// the one exponential (ard_element), so a template argument would double the forms for two selects per element.
#pragma once
#include "ard_element.hpp"  // ard_element, ard_m: the one element function
#include "multi_target_grad_tile_impl.hpp"  // the launch bounds of the multi-target gradient forms, predict_tile_grid, dpp_row_sum16
#include "pivot_product.hpp"
#include "spd_sweep.hpp"

namespace matinv {

// s_ij of the four elements a lane owns in tile (ti, tj): rows 16 ti + trow(r, q), column 16 tj + c; z in LDS, dimension k at zs + k N
// (zero beyond n). (z_i - z_j)^2 = (z_j - z_i)^2 exactly and the k order is fixed: s is bitwise symmetric.
template <class T, int NT>
__device__ __forceinline__ void ard_tile_s(const T *zs, int ndim, int ti, int tj, int q, int c, T (&s)[4])
{
    typedef TileGeo<T> G;
    constexpr int N = 16 * NT;
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = (T)0;
#pragma unroll 1
    for (int k = 0; k < ndim; ++k) {
        const T zc = zs[k * N + 16 * tj + c];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const T d = zs[k * N + 16 * ti + G::trow(r, q)] - zc;
            s[r] = fma_t(d, d, s[r]);
        }
    }
}

// the lower tiles of M in the accumulator layout of spd_load_lower: diagonal tiles complete, identity padding beyond n
template <class T, int NT, bool FULL>
__device__ __forceinline__ void ard_generate_lower(typename TileGeo<T>::vec4 (&acc)[NT][NT], const T *zs, int ndim, int kind, T sf2, T sn2,
                                                   int n, int q, int c)
{
    typedef TileGeo<T> G;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
            if (tj > ti) continue;
            T s[4];
            ard_tile_s<T, NT>(zs, ndim, ti, tj, q, c, s);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * ti + G::trow(r, q), col = 16 * tj + c;
                const bool in = FULL || ti < NT - 1 || (row < n && col < n);  // tj <= ti: only the last tile row reaches beyond n
                T v = ard_m(s[r], kind, sf2, sn2, ti == tj && row == col);
                v = in ? v : ((row == col) ? (T)1 : (T)0);
                ard_pin(v);  // one element at a time, where its distance is
                acc[ti][tj][r] = v;
            }
        }
}

// spd_natural_first_failure (tile_common.hpp) for a matrix that exists nowhere in memory: its tiles are filled by the generator, the
// natural-order factorisation is that helper's, line for line. colbuf: 16 NT elements of LDS.
template <int NT, class T>
__device__ __forceinline__ int ard_natural_first_failure(const T *zs, int ndim, int kind, T sf2, T sn2, int n, T *colbuf, int l)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    int q = l >> 4, c = l & 15;
    asm volatile("" : "+v"(q), "+v"(c));
    vec4 w[NT][NT];
    ard_generate_lower<T, NT, false>(w, zs, ndim, kind, sf2, sn2, n, q, c);
    int found = 0;
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) {
#pragma nounroll
        for (int jj = 0; jj < 16; ++jj) {
            const int j = 16 * tj + jj;
            if (found != 0 || j >= n) break;
            // column j, rows from its tile on: the lanes with c == jj hold it (diagonal tiles are complete)
            wave_lds_sync();
            if (c == jj) {
#pragma unroll
                for (int ti = tj; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) colbuf[16 * ti + G::trow(r, q)] = w[ti][tj][r];
            }
            wave_lds_sync();
            const T piv = colbuf[j];
            if (__ballot(!(piv > (T)0)) != 0ull) {  // every lane read the same element
                found = j + 1;
                break;
            }
            const T rp = (T)1 / piv;
            // rows and columns already eliminated keep rounding residue only; it never reaches a live element
#pragma unroll
            for (int tk = tj; tk < NT; ++tk) {
                const T wc = colbuf[16 * tk + c] * rp;
#pragma unroll
                for (int ti = tk; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) w[ti][tk][r] = fma_t(-colbuf[16 * ti + G::trow(r, q)], wc, w[ti][tk][r]);
            }
        }
    }
    wave_lds_sync();
    return found;
}

// Layout (lane l = 16 q + c; the lane holds W[16 ti + trow(r, q)][16 tj + c] in acc[ti][tj][r], tj <= ti):
//   LDS: panel[4 N] (the sweep's; before it the d length scales; after it rs[N] = row part of W y, kap[N] = -W_ii, al[N] = alpha),
//        zs[16 N] = z, dimension k at zs + k N, ys[N] = y; both zero beyond n, both live for the whole matrix.
template <class T, int NT, bool FULL>
__device__ __forceinline__ void ard_tile_body(const T *Xs, size_t xstride, const T *Ys, size_t ystride, const T *Th, int ndim, int kind, T *Lm,
                                              T *Gr, T *Al, int *info, int n_rt, unsigned batch, T *panel, T *zs, T *ys)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    constexpr int N = 16 * NT;
    typedef PanelSolve<NT, true, T> PS;
    const int l = threadIdx.x;

    for (unsigned mat = blockIdx.x; mat < batch; mat += gridDim.x) {
        int n = FULL ? N : n_rt;  // run-time n opaque once per matrix, predicates on the edge tiles only: see gj_tile_body
        if (!FULL) asm volatile("" : "+s"(n));
        int q = l >> 4, c = l & 15;
        asm volatile("" : "+v"(q), "+v"(c));  // see matinv_gj_tile_f64

        // ---- prologue: exp theta once per matrix, z = x / l and y to LDS ---------------------------------------------------------
        const T *th = Th + (size_t)mat * (ndim + 2);
        const T sf2 = ard_exp(th[0]), sn2 = ard_exp(th[ndim + 1]);
        if (l < ndim) panel[l] = ard_exp(th[1 + l]);
        wave_lds_sync();
        {
            const T *X = Xs + (size_t)mat * xstride;
            const T *Y = Ys + (size_t)mat * ystride;
            const int nd = n * ndim;
            // consecutive lanes on consecutive elements of the point-major block; the slots beyond n are zeroed below
            for (int e = l; e < nd; e += 64) {
                const int i = e / ndim, k = e - i * ndim;
                zs[k * N + i] = X[e] / panel[k];
            }
            if (!FULL)
                for (int e = l; e < (N - n) * ndim; e += 64) {
                    const int k = e / (N - n), i = n + (e - k * (N - n));
                    zs[k * N + i] = (T)0;
                }
#pragma unroll
            for (int k = 0; k < (N + 63) / 64; ++k) {
                const int i = l + 64 * k;
                if (i < N) ys[i] = (FULL || i < n) ? Y[i] : (T)0;
            }
        }
        wave_lds_sync();

        // ---- generate (in place of spd_load_lower) and sweep: W = -M^-1 in the lower tiles, the pivots folded where they are formed ----
        vec4 acc[NT][NT];
        ard_generate_lower<T, NT, FULL>(acc, zs, ndim, kind, sf2, sn2, n, q, c);
        wave_lds_sync();  // the length scales have been read: the panel buffer is the sweep's
        unsigned long long bad = 0;
        int binfo = 0;  // column of the first non-positive pivot + 1
        PivotProduct<T> prod;
        spd_full_sweep<T, NT, FULL>(acc, panel, n, q, c, bad, binfo, [&](const PS &ps) { prod.fold(ps.d[0][0], ps.u11, ps.u22, ps.u33); });

        // ---- epilogue: alpha and kappa as in logml_grad_tile_body --------------------------------------------------------------------
        const bool ok = bad == 0;
        const T ld = prod.log_value();
        wave_lds_sync();  // the last panel has been consumed
        T *const rs = panel, *const kap = panel + N, *const al = panel + 2 * N;
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
                if (G::trow(r, q) == c) kap[16 * ti + c] = -acc[ti][ti][r];  // the one lane that holds W_ii
            }
        }
#pragma unroll
        for (int tj = 0; tj < NT - 1; ++tj) {
            colacc[tj] += __shfl_xor(colacc[tj], 16);
            colacc[tj] += __shfl_xor(colacc[tj], 32);
        }
        wave_lds_sync();
        T acol[NT];
        T quad = (T)0;  // y^T alpha: one chain over the tile columns, then the 16 c lanes; the four q groups hold the same bits
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
            const int i = 16 * tj + c;
            const bool in = FULL || tj < NT - 1 || i < n;
            const T a = -(rs[i] + colacc[tj]);  // W = -M^-1
            acol[tj] = a;
            quad = fma_t(ys[i], a, quad);  // y is zero beyond n
            if (q == 0) al[i] = a;
            if (in && q == 0 && Al) Al[(size_t)mat * n + i] = ok ? a : nan_of<T>();
        }
        quad = dpp_row_sum16(quad);
        // log 2 pi
        if (Lm && l == 0) Lm[mat] = ok ? (T)-0.5 * fma_t((T)n, (T)1.83787706640934548356, quad + ld) : nan_of<T>();

        if (Gr) {  // wave-uniform
            wave_lds_sync();
            T *const gm = Gr + (size_t)mat * (ndim + 2);
            // one pass: G = alpha alpha^T + W; grad[0] and grad[d + 1] from it; w G sf2 psi(s) left in place
            T p0[4] = {(T)0, (T)0, (T)0, (T)0}, pn[4] = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                T ar[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) ar[r] = al[16 * ti + G::trow(r, q)];
#pragma unroll
                for (int tj = 0; tj <= ti; ++tj) {
                    const T w = (tj == ti) ? (T)0.5 : (T)1;
                    T s[4];
                    ard_tile_s<T, NT>(zs, ndim, ti, tj, q, c, s);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * ti + G::trow(r, q), col = 16 * tj + c;
                        const bool in = FULL || ti < NT - 1 || (row < n && col < n);
                        T phi, psi;
                        ard_element(s[r], kind, phi, psi);
                        const T g = fma_t(ar[r], acol[tj], acc[ti][tj][r]);
                        const T wg = in ? w * g : (T)0;  // identity padding is no part of M
                        if (ti == tj && row == col) pn[r] += in ? g : (T)0;
                        p0[r] = fma_t(wg, sf2 * phi, p0[r]);
                        T h = wg * (sf2 * psi);
                        ard_pin(h);  // one element at a time, where its distance is (ard_generate_lower)
                        ard_pin(p0[r]);
                        acc[ti][tj][r] = h;
                    }
                }
            }
            {
                T s0 = (p0[0] + p0[1]) + (p0[2] + p0[3]), sn = (pn[0] + pn[1]) + (pn[2] + pn[3]);
                s0 = dpp_row_sum16(s0);
                sn = dpp_row_sum16(sn);
                s0 += __shfl_xor(s0, 16);
                sn += __shfl_xor(sn, 16);
                s0 += __shfl_xor(s0, 32);
                sn += __shfl_xor(sn, 32);
                if (l == 0) {
                    gm[0] = ok ? s0 : nan_of<T>();
                    gm[ndim + 1] = ok ? ((T)0.5 * sn2) * sn : nan_of<T>();
                }
            }
            for (int k = 0; k < ndim; ++k) {
                // lane coordinates opaque once per k, as in the p loop of logml_grad_tile_body: otherwise the LDS offsets of all tiles
                // are hoisted out of this loop and the allocator spills them beside the accumulators
                int qk = q, ck = c;
                asm volatile("" : "+v"(qk), "+v"(ck));
                const T *const zk = zs + k * N;
                T part[4] = {(T)0, (T)0, (T)0, (T)0};
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) {
                    T zr[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) zr[r] = zk[16 * ti + G::trow(r, qk)];
#pragma unroll
                    for (int tj = 0; tj <= ti; ++tj) {
                        const T zc = zk[16 * tj + ck];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const T d = zr[r] - zc;  // beyond n: z = 0 and acc = 0
                            part[r] = fma_t(acc[ti][tj][r], d * d, part[r]);
                        }
                    }
                }
                T s = (part[0] + part[1]) + (part[2] + part[3]);
                s = dpp_row_sum16(s);
                s += __shfl_xor(s, 16);
                s += __shfl_xor(s, 32);
                if (l == 0) gm[1 + k] = ok ? s : nan_of<T>();
            }
        }
        int code = binfo;
        if constexpr (sizeof(T) == 4) {
            if (bad != 0) {  // wave-uniform; rejected matrices only: the fp32 tile order does not say which column fails FIRST (tile_common.hpp)
                wave_lds_sync();  // the last reads of the panel buffer
                const int nat = ard_natural_first_failure<NT, T>(zs, ndim, kind, sf2, sn2, n, panel, l);
                if (nat) code = nat;
            }
        }
        if (l == 0 && info) info[mat] = code;
        wave_lds_sync();  // the next matrix's first LDS writes must not pass this one's last reads
    }
}

// The ARD forms of matinv_spd_tile_f64 / matinv_spd_tile_f32: the same names with a third to a fifteenth template argument. Launch
// bounds: those of the multi-target gradient forms of the same NT (multi_target_grad_tile_impl.hpp), one wave per SIMD fewer where a form
// spills under them: the fp64 2 x 2 forms at four waves (2 and 6 registers), the fp32 4 x 4 forms at four (5 and 6) and the fp32 5 x 5
// forms at three (1 each). With that no form uses scratch (profiles/ard_logml_kernel_registers.txt).
constexpr int ard_f64_waves(int nt, bool full) { return multi_target_grad_f64_waves(nt, full) - (nt == 2 ? 1 : 0); }
constexpr int ard_f32_waves(int nt, bool full) { return multi_target_f32_waves(nt, full) - ((nt == 4 || nt == 5) ? 1 : 0); }

#define MATINV_ARD_ARGS LOO &&GRAD &&PREDICT &&COV &&LOOGRAD &&COLOUR &&WHITEN &&MULTI &&MTGRAD &&TREND &&TRENDGRAD &&TRENDLOO &&ARD

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD,
          bool TREND, bool TRENDGRAD, bool TRENDLOO, bool ARD>
__global__ __launch_bounds__(64, ard_f64_waves(NT, FULL)) void matinv_spd_tile_f64(const double *Xs, size_t xstride, const double *Ys,
                                                                                  size_t ystride, const double *Th, int ndim, int kind,
                                                                                  double *Lm, double *Gr, double *Al, int *info, int n_rt,
                                                                                  unsigned batch)
{
    static_assert(MATINV_ARD_ARGS, "the fifteen-argument form is the ARD log-marginal-likelihood kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    __shared__ double zs[ARD_MAX_DIM * 16 * NT];
    __shared__ double ys[16 * NT];
    ard_tile_body<double, NT, FULL>(Xs, xstride, Ys, ystride, Th, ndim, kind, Lm, Gr, Al, info, n_rt, batch, panel, zs, ys);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD,
          bool TREND, bool TRENDGRAD, bool TRENDLOO, bool ARD>
__global__ __launch_bounds__(64, ard_f32_waves(NT, FULL)) void matinv_spd_tile_f32(const float *Xs, size_t xstride, const float *Ys,
                                                                                  size_t ystride, const float *Th, int ndim, int kind,
                                                                                  float *Lm, float *Gr, float *Al, int *info, int n_rt,
                                                                                  unsigned batch)
{
    static_assert(MATINV_ARD_ARGS, "the fifteen-argument form is the ARD log-marginal-likelihood kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    __shared__ float zs[ARD_MAX_DIM * 16 * NT];
    __shared__ float ys[16 * NT];
    ard_tile_body<float, NT, FULL>(Xs, xstride, Ys, ystride, Th, ndim, kind, Lm, Gr, Al, info, n_rt, batch, panel, zs, ys);
}
#undef MATINV_ARD_ARGS

template <class T>
hipError_t launch_ard_tile(int kind, int n, int ndim, const T *Xs, size_t xstride, const T *Ys, size_t ystride, const T *Th, T *Lm, T *Gr,
                           T *Al, size_t batch, int *info, hipStream_t stream)
{
    if (!ard_tile_supports(n) || ndim < 1 || ndim > ARD_MAX_DIM) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = predict_tile_grid(batch), b = (unsigned)batch;  // the grid of the multi-target launchers
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true, true, true, true, true, true, true, true, true, true, true, true>),
                               dim3(grid), dim3(64), 0, stream, Xs, xstride, Ys, ystride, Th, ndim, kind, Lm, Gr, Al, info, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true, true, true, true, true, true, true, true, true, true, true, true>),
                               dim3(grid), dim3(64), 0, stream, Xs, xstride, Ys, ystride, Th, ndim, kind, Lm, Gr, Al, info, n, b);
    });
    return hipGetLastError();
}
}  // namespace matinv
