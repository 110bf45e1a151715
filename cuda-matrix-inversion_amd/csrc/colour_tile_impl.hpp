// colour_tile_impl.hpp (instantiated by colour_tile_kernels.hip for f64 and colour_tile_f32_kernels.hip for f32) -- the lower Cholesky
// factor of batched SPD matrices and the coloured samples Y = m + L Z on the MFMA tile layout, n <= 96:
//     C = L L^T (lower triangle of C read, L lower triangular with a positive diagonal),   Y[:, s] = m + L z_s   (m optional)
// The load, the PanelSolve pipeline and the block-step loop are those of logdet_tile_body with BORDER = false (logdet_tile_impl.hpp),
// copied once more so that every earlier kernel compiles to what it compiled to before. That sweep is a factorisation only: a tile column
// left of the next panel is dead. What this form adds sits between two block steps:
//   * After the pivot block of step kb is solved, PanelSolve holds its unit-lower factor l10 .. l32 and the squared Cholesky diagonal
//     u = (d[0][0], u11, u22, u33), and the LDS panel still holds the 4-wide panel P of that step (row i of the trailing matrix against
//     the four pivots). The four Cholesky columns of the step are P l^-T diag(u)^-1/2: lane (q, c) forms row 16 ti + c of X = P l^-T by
//     six FMAs, picks x_q and scales it by 1 / sqrt(u_q) -- L[16 ti + c][pivot q], for every live tile row ti. On the diagonal the value
//     is sqrt(u_q) itself, above it an exact zero.
//   * Lane (q, c) holding (row 16 ti + c, K index q) is the lane map of the MFMA's A operand, so the value is kept as it stands
//     (lop[kb][ti]: as many registers as the tile columns that died gave back) and the product L Z_g needs no transposition: per group
//     of 16 samples, one MFMA per live tile per K-slab with B = Z_g[pivot q][sample c] out of the query buffer of the prediction
//     forms. L is triangular, so slab kb reaches tile rows ti >= kb / 4 only. The accumulators start at m, so Z = 0 returns m.
//   * The same value goes to dL at once: the 16 lanes of a q group cover 16 consecutive rows of one column. The tile rows above the
//     pivot block store the zeros of the strict upper triangle.
// fp32: TileGeo<float> eliminates tile-local position 4 t + r as pivot t of block r, which is a permuted order, and the factor of a
// permuted matrix is not the factor of the matrix. This form therefore loads natural index 4 r + t into position 4 t + r (tile_nat, its
// own inverse, applied to rows and columns alike), so the sweep's order IS the natural order and every index that leaves the tile goes
// through the same map. fp64 positions are natural as they stand.
// Y for a group leaves through the query buffer, so every global access of the epilogue is a run of consecutive elements.
// HBM traffic per matrix: n^2 / 2 + n + n S elements in, n^2 + n S out.
// A non-positive (or NaN) pivot makes info = its column + 1 and every requested output NaN: no fallback launch.
//
// The kernels are the colour forms of the SPD inversion kernels whose sweep they run: overloads of matinv_spd_tile_f64 / _f32 with six
// more trailing template arguments ("Posterior samples", says why).
#pragma once
#include "predict_tile_impl.hpp"  // predict_qstride, predict_tile_grid

namespace matinv {

// natural tile-local index held at tile-local position p (see above)
template <class T>
__device__ __forceinline__ int tile_nat(int p)
{
    return sizeof(T) == 4 ? (((p & 3) << 2) | (p >> 2)) : p;
}

__device__ __forceinline__ double colour_sqrt(double v) { return __builtin_sqrt(v); }
__device__ __forceinline__ float colour_sqrt(float v) { return __builtin_sqrtf(v); }

template <class T, int NT, bool FULL>
__device__ __forceinline__ void colour_tile_body(const T *Cs, size_t stride, const T *Ms, const T *Zs, int nsample, T *Ys, T *Ls, int *info,
                                                 int info_base, int n_rt, unsigned batch, T *panel, T *ml, T *zq)
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
        const T *A = Cs + (size_t)mat * stride;
        T *const Lm = Ls ? Ls + (size_t)mat * n * n : nullptr;
        int q = l >> 4, c = l & 15;
        asm volatile("" : "+v"(q), "+v"(c));  // see matinv_gj_tile_f64
        const int cn = tile_nat<T>(c);  // the natural tile-local column (and panel row) of this lane

        vec4 acc[NT][NT];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) {
                if (tj > ti) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * ti + tile_nat<T>(G::trow(r, q)), col = 16 * tj + cn;
                    const bool in = FULL || ti < NT - 1 || (row < n && col < n);  // tj <= ti: only the last tile row reaches beyond n
                    const int hi = row > col ? row : col, lo = row > col ? col : row;
                    // only the lower triangle is read (mirror position inside the diagonal tiles)
                    acc[ti][tj][r] = in ? A[(unsigned)(lo * n + hi)] : ((row == col) ? (T)1 : (T)0);
                }
            }

        unsigned long long bad = 0;
        int binfo = 0;  // position of the first non-positive pivot + 1
        T aop[NT], bop[NT];
        T lop[NKB][NT];  // lop[kb][ti], ti >= kb / 4: L[16 ti + c][pivot q of block step kb], the A operand of the product L Z

        // the four Cholesky columns of block step kb out of its solved pivot block and the panel in LDS
        auto columns = [&](const PS &ps, const int kb) {
            const int tK = kb >> 2, rK = kb & 3;
            const T u01 = (q & 1) ? ps.u11 : ps.d[0][0], u23 = (q & 1) ? ps.u33 : ps.u22;
            const T sq = colour_sqrt((q & 2) ? u23 : u01);
            const T rq = (T)1 / sq;
            const int coll = tile_nat<T>(G::pcol(rK, q)), col = 16 * tK + coll;
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                T v = (T)0;  // the tile rows above the pivot block: the strict upper triangle
                if (ti >= tK) {
                    const T *w = &panel[(16 * ti + c) * 4];
                    const T x0 = w[0];
                    const T x1 = fma_t(-ps.l10, x0, w[1]);
                    const T x2 = fma_t(-ps.l21, x1, fma_t(-ps.l20, x0, w[2]));
                    const T x3 = fma_t(-ps.l32, x2, fma_t(-ps.l31, x1, fma_t(-ps.l30, x0, w[3])));
                    const T x01 = (q & 1) ? x1 : x0, x23 = (q & 1) ? x3 : x2;
                    v = ((q & 2) ? x23 : x01) * rq;
                    if (ti == tK) v = cn < coll ? (T)0 : (cn == coll ? sq : v);
                    lop[kb][ti] = v;
                }
                if (Lm) {  // wave-uniform
                    const int row = 16 * ti + cn;
                    if (FULL || (row < n && col < n)) Lm[(unsigned)(col * n + row)] = v;
                }
            }
        };

        spd_panel_to_lds<NT, T>(panel, acc, 0, q, c);
        wave_lds_sync();
        {
            PS ps0;
            ps0.binfo = &binfo;
#pragma unroll
            for (int s = 0; s < PS::NSTAGE; ++s) ps0.stage(s, panel, 0, q, c, aop, bop, bad);
            columns(ps0, 0);
        }
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            if (kb + 1 < NKB) {
                spd_prep_operands<NT, T>(acc, bop, kb, q, c);
                const int tn = (kb + 1) >> 2;
                // (a) the tile column the next panel is read from (rows above it are dead)
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) {
                    if (ti < tn) continue;
                    acc[ti][tn] = G::mfma(aop[ti], bop[tn], acc[ti][tn]);
                }
                // (b) the other LIVE lower tiles, pinned between the pieces of the next panel. Live = right of the next panel's tile
                // column: the pivot block's own tile column is only read again through that panel (a factorisation, no inverse)
                constexpr int NSG = PS::NSTAGE;
                int nb = 0;  // number of (b) tiles: folds to a literal
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int tj = 0; tj < NT; ++tj)
                        if (tj <= ti && tj > tn) ++nb;
                T aop_next[NT], bop_next[NT];
                PS ps;
                ps.binfo = &binfo;
                int count = 0, ev = 0;
                auto run_events = [&](bool flush) {
#pragma unroll
                    for (int e = 0; e < NSG + 1; ++e) {
                        const int lead = nb < 2 ? nb : 2;
                        const int thr = (e == 0) ? lead : lead + ((nb - lead) * e) / NSG;
                        if (e == ev && (flush || thr <= count)) {
                            __builtin_amdgcn_sched_barrier(0);
                            if (e == 0) {
                                wave_lds_sync();
                                spd_panel_to_lds<NT, T>(panel, acc, kb + 1, q, c);
                                wave_lds_sync();
                            } else if (e - 1 < 6 || e - 1 - 6 >= tn) {  // tile rows above the next pivot block are dead
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
                        if (tj > ti || tj <= tn) continue;
                        acc[ti][tj] = G::mfma(aop[ti], bop[tj], acc[ti][tj]);
                        ++count;
                        run_events(false);
                    }
                run_events(true);
                columns(ps, kb + 1);  // the panel of step kb + 1 stays in LDS until the next step stages its own
#pragma unroll
                for (int ti = 0; ti < NT; ++ti) { aop[ti] = aop_next[ti]; bop[ti] = bop_next[ti]; }
            }
        }

        const bool ok = bad == 0;
        if (!ok && Lm) {  // wave-uniform; rejected matrices only: what the block steps stored is not a factor
            for (int e = l; e < n * n; e += 64) Lm[e] = nan_of<T>();
        }
        if (Ys) {  // wave-uniform
            const size_t first = (size_t)mat * nsample;
            wave_lds_sync();  // the last panel has been consumed
#pragma unroll
            for (int k = 0; k < (N + 63) / 64; ++k) {
                const int i = l + 64 * k;
                if (i < N) ml[i] = (Ms && (FULL || i < n)) ? Ms[(size_t)mat * n + i] : (T)0;
            }
            const int ngroups = (nsample + 15) >> 4;
            for (int g = 0; g < ngroups; ++g) {
                // lane coordinates and n opaque once per group: otherwise the offsets of the staging loads and of the LDS reads are
                // hoisted out of this loop and the allocator spills them beside the factor (as in predict_tile_body)
                int ng = n, lg = l, qg = q, cg = c;
                if (!FULL) asm volatile("" : "+s"(ng));
                asm volatile("" : "+v"(lg), "+v"(qg), "+v"(cg));
                const int left = nsample - 16 * g;  // samples from this group's first on
                const T *Zg = Zs + (first + 16 * (size_t)g) * ng;
                T *Yg = Ys + (first + 16 * (size_t)g) * ng;
                wave_lds_sync();  // the previous group's reads of zq, this matrix's writes of ml
                // the group's 16 n contiguous elements, consecutive lanes on consecutive elements of one sample
#pragma unroll
                for (int k = 0; k < N / 4; ++k) {
                    const int e = lg + 64 * k, j = e / N, i = e - j * N;
                    const bool in = (FULL || i < ng) && j < left;
                    zq[j * NS + i] = in ? Zg[(unsigned)(j * ng + i)] : (T)0;
                }
                wave_lds_sync();
                T *const zc = zq + cg * NS;  // the sample of this lane
                vec4 y[NT];
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[ti][r] = ml[16 * ti + tile_nat<T>(G::trow(r, qg))];
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) {
                    const int tK = kb >> 2, rK = kb & 3;
                    const T b = zc[16 * tK + tile_nat<T>(G::pcol(rK, qg))];  // identity padding meets the zeros beyond n
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti) {
                        if (ti < tK) continue;
                        y[ti] = G::mfma(lop[kb][ti], b, y[ti]);
                    }
                }
                wave_lds_sync();  // the B operands have been read: the buffer takes the group's Y, sample by sample
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) zc[16 * ti + tile_nat<T>(G::trow(r, qg))] = ok ? y[ti][r] : nan_of<T>();
                wave_lds_sync();
#pragma unroll
                for (int k = 0; k < N / 4; ++k) {
                    const int e = lg + 64 * k, j = e / N, i = e - j * N;
                    if ((FULL || i < ng) && j < left) Yg[(unsigned)(j * ng + i)] = zq[j * NS + i];
                }
            }
        }
        // PanelSolve names a tile-local position; the column is the natural index it holds
        int code = binfo ? ((binfo - 1) & ~15) + tile_nat<T>((binfo - 1) & 15) + 1 : 0;
        if constexpr (sizeof(T) == 4) {
            if (bad != 0) {  // wave-uniform; rejected matrices only: the natural-order recount of the other fp32 forms (tile_common.hpp)
                wave_lds_sync();
                const int nat = spd_natural_first_failure<NT, T>(A, (const T *)nullptr, n, panel, l);
                if (nat) code = nat;
            }
        }
        if (info && l == 0) {
            // info_base != 0: info[mat] holds the code of an earlier stage, which stands; this stage's columns count on from info_base
            const int prior = info_base ? info[mat] : 0;
            info[mat] = prior ? prior : (code ? info_base + code : 0);
        }
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// The colour forms of matinv_spd_tile_f64 / matinv_spd_tile_f32 (tile_impl.hpp): the same names with a third to an eighth template
// argument. Launch bounds: those of the log-determinant forms for the same NT (logdet_tile_impl.hpp), one wave per SIMD fewer where a
// form spills under them: the 5 x 5 forms, which keep 15 tiles of accumulators or factor plus the samples' accumulators and spill 15 to
// 19 (fp64) and 2 to 3 (fp32) registers under the bounds of the log-determinant forms (profiles/colour_kernel_registers.txt). No form
// uses scratch.
constexpr int colour_f64_waves(int nt) { return nt >= 5 ? 1 : 2; }
constexpr int colour_f32_waves(int nt) { return nt >= 5 ? 2 : 3; }

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR>
__global__ __launch_bounds__(64, colour_f64_waves(NT)) void matinv_spd_tile_f64(const double *Cs, size_t stride, const double *Ms,
                                                                                       const double *Zs, int nsample, double *Ys, double *Ls,
                                                                                       int *info, int info_base, int n_rt, unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR, "the eight-argument form is the colour kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    __shared__ double ml[16 * NT], zq[16 * predict_qstride(16 * NT)];
    colour_tile_body<double, NT, FULL>(Cs, stride, Ms, Zs, nsample, Ys, Ls, info, info_base, n_rt, batch, panel, ml, zq);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR>
__global__ __launch_bounds__(64, colour_f32_waves(NT)) void matinv_spd_tile_f32(const float *Cs, size_t stride, const float *Ms,
                                                                                       const float *Zs, int nsample, float *Ys, float *Ls,
                                                                                       int *info, int info_base, int n_rt, unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR, "the eight-argument form is the colour kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    __shared__ float ml[16 * NT], zq[16 * predict_qstride(16 * NT)];
    colour_tile_body<float, NT, FULL>(Cs, stride, Ms, Zs, nsample, Ys, Ls, info, info_base, n_rt, batch, panel, ml, zq);
}

template <class T>
hipError_t launch_colour_tile(int n, int nsample, const T *Cs, size_t stride, const T *Ms, const T *Zs, T *Ys, T *Ls, size_t batch, int *info,
                              int info_base, hipStream_t stream)
{
    if (!colour_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = predict_tile_grid(batch), b = (unsigned)batch;  // 256 * 12 workgroups a round (predict_tile_impl.hpp)
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true, true, true, true, true>), dim3(grid), dim3(64), 0, stream, Cs, stride,
                               Ms, Zs, nsample, Ys, Ls, info, info_base, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true, true, true, true, true>), dim3(grid), dim3(64), 0, stream, Cs, stride,
                               Ms, Zs, nsample, Ys, Ls, info, info_base, n, b);
    });
    return hipGetLastError();
}
}  // namespace matinv
