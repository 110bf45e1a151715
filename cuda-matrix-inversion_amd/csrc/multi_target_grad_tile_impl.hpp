// multi_target_grad_tile_impl.hpp (instantiated by multi_target_grad_tile_kernels.hip for f64 and multi_target_grad_tile_f32_kernels.hip
// for f32) -- gradients of the multi-output GP log marginal likelihood on the MFMA tile layout, n <= 96. With M = B + diag c (c optional),
// K = M^-1, D targets y_t, alpha_t = K y_t and P symmetric derivative matrices dM_p:
//     G = sum_t alpha_t alpha_t^T - D K      grad[p] = 1/2 sum_ij G_ij dM_p[i][j]      gradc[i] = 1/2 G_ii
//     logml_t = -1/2 (y_t^T K y_t + log det M + n log 2 pi)                            alpha[t] = alpha_t
// the gradient of sum_t logml_t with respect to the parameter behind dM_p and to c_i. The load, the PanelSolve pipeline, the block-step
// loop and the pivot fold are spd_load_lower and spd_full_sweep of spd_sweep.hpp as multi_target_tile_body calls them, kept HERE as a
// copy of their own: called from the shared header, the full fp32 4 x 4 form measured 1.3 % slower ("The shared SPD sweep").
// A change to the sweep is made there and here. The epilogue has two phases:
//   1. per group of 16 targets, exactly as multi_target_tile_body: stage Y_g, T_g = W Y_g on the MFMA unit, quad and logml in its
//      reduction order, alpha_g = -T_g into the group buffer and out. logml and alpha therefore carry the bits of
//      matinv_multi_target_batched for the same inputs.
//   2. (grad or gradc asked for) after the last T_g, when W is no longer needed intact: acc <- D acc, then for every group
//      acc[ti][tj] += alpha_g[ti] alpha_g[tj]^T, four 16 x 16 x 4 MFMAs per lower tile, alpha_g read from the group buffer in operand
//      layout (the same value is the A and the B operand). With D <= 16 the one group is still in the buffer. With more, every group
//      comes back from where phase 1 stored it: dAlpha when that is asked for, a library workspace of D n elements per workgroup
//      otherwise -- the same wavefront wrote it, so a counter wait orders it. Both hold the same values and are read in the same order:
//      asking for alpha changes no bit of grad. Then the weights (1/2 in the diagonal tiles, 1 below), gradc out of the diagonal tiles
//      and the per-p contraction of logml_grad_tile_body as it stands.
// Nothing in the order of operations depends on batch, grid or P; which outputs are stored is decided by wave-uniform pointers.
// HBM traffic per matrix: n^2 / 2 + n + D n + P n^2 / 2 elements in, P + n + D + D n out; D > 16: D n more, out and back in through L2.
// A non-positive (or NaN) pivot makes info = its column + 1 (PanelSolve::binfo) and every requested output NaN: no fallback launch.
//
// The kernels are overloads of matinv_spd_tile_f64 / _f32 with nine more trailing template arguments ("Gradients of the
// multi-output log marginal likelihood").
#pragma once
#include "multi_target_tile_impl.hpp"  // the launch bounds of the multi-target forms, predict_qstride, predict_tile_grid, dpp_row_sum16

namespace matinv {

// Epilogue layout (lane l = 16 q + c; the lane holds W[16 ti + trow(r, q)][16 tj + c] in acc[ti][tj][r], tj <= ti):
//   LDS: panel[4 N] (the sweep's, the panel of each block step again in phase 1, gradc on its way out in phase 2), aq[16 (N + 1)] = the
//        16 vectors of ONE group (targets, then alpha), vector j at aq + j (N + 1), zero beyond n and beyond D.
//   phase 1: see multi_target_tile_body.
//   phase 2: MFMA step s of a group takes targets 4 s ... 4 s + 3: lane (q, c) supplies alpha_{4 s + q}[16 t + c] for tile index t, as row
//            c of the A operand (t = ti) and as column c of the B operand (t = tj). The padded targets of the last group are zero.
//   abase: where the alpha of this matrix is stored: dAlpha, else the workgroup's slice of the workspace (D > 16 only), else nowhere.
template <class T, int NT, bool FULL>
__device__ __forceinline__ void multi_target_grad_tile_body(const T *Bs, const T *Cs, const T *Ys, const T *dMs, int ntarget, int nparam,
                                                            T *grad, T *gradc, T *Lm, T *Al, T *ws, int *info, int n_rt, unsigned batch,
                                                            T *panel, T *aq)
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

        // ---- epilogue, phase 1: W = -M^-1 in the lower tiles; the targets group by group (multi_target_tile_body) ------------------
        const bool ok = bad == 0;
        const T ld = prod.log_value();
        const bool second = grad || gradc;              // wave-uniform
        const int ngroups = (ntarget + 15) >> 4;        // wave-uniform; every output needs the targets
        T *const abase = Al ? Al + (size_t)mat * ntarget * n : (ws ? ws + (size_t)blockIdx.x * ntarget * n : nullptr);
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
                    // log 2 pi
                    if (Lm) Lm[first + cg] = ok ? (T)-0.5 * fma_t((T)ng, (T)1.83787706640934548356, qd + ld) : nan_of<T>();
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
                    // opaque once more: otherwise the offsets of these stores are formed above the T_g build and live through it
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

        // ---- epilogue, phase 2: G = sum_t alpha_t alpha_t^T + D W in place of W, weighted; gradc and the contraction ----------------
        if (second) {  // wave-uniform
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
            // the weights of logml_grad_tile_body: 1/2 in the diagonal tiles (both triangles stored), 1 in the strictly lower ones
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
                    // lane coordinates and n opaque once per p: otherwise the 4 * NT (NT + 1) / 2 element offsets (and, ragged, as many
                    // predicates) are hoisted out of this loop and the allocator spills them beside the accumulators
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
        if (l == 0 && info) info[mat] = code;
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// The gradient forms of the multi-target kernels: matinv_spd_tile_f64 / matinv_spd_tile_f32 with a third to an eleventh template
// argument, under the launch bounds of the multi-target forms of the same NT (multi_target_tile_impl.hpp): the live set of phase 1 is
// theirs, and phase 2 holds fewer registers beside the accumulators (NT operands, then four partial sums and the loads of one dM_p).
// One form spills under them and takes one wave per SIMD less: the ragged fp64 5 x 5 (11 registers, 48 bytes of scratch at two waves).
// profiles/multi_target_grad_kernel_registers.txt: no form uses scratch or spills.
constexpr int multi_target_grad_f64_waves(int nt, bool full)
{
    const bool spills = nt == 5 && !full;
    return multi_target_f64_waves(nt, full) - (spills ? 1 : 0);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD>
__global__ __launch_bounds__(64, multi_target_grad_f64_waves(NT, FULL)) void matinv_spd_tile_f64(const double *Bs, const double *Cs,
                                                                                             const double *Ys, const double *dMs, int ntarget,
                                                                                             int nparam, double *grad, double *gradc, double *Lm,
                                                                                             double *Al, double *ws, int *info, int n_rt,
                                                                                             unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN && MULTI && MTGRAD,
                  "the eleven-argument form is the multi-target gradient kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    __shared__ double aq[16 * predict_qstride(16 * NT)];
    multi_target_grad_tile_body<double, NT, FULL>(Bs, Cs, Ys, dMs, ntarget, nparam, grad, gradc, Lm, Al, ws, info, n_rt, batch, panel, aq);
}

template <int NT, bool FULL, bool LOO, bool GRAD, bool PREDICT, bool COV, bool LOOGRAD, bool COLOUR, bool WHITEN, bool MULTI, bool MTGRAD>
__global__ __launch_bounds__(64, multi_target_f32_waves(NT, FULL)) void matinv_spd_tile_f32(const float *Bs, const float *Cs, const float *Ys,
                                                                                             const float *dMs, int ntarget, int nparam,
                                                                                             float *grad, float *gradc, float *Lm, float *Al,
                                                                                             float *ws, int *info, int n_rt, unsigned batch)
{
    static_assert(LOO && GRAD && PREDICT && COV && LOOGRAD && COLOUR && WHITEN && MULTI && MTGRAD,
                  "the eleven-argument form is the multi-target gradient kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    __shared__ float aq[16 * predict_qstride(16 * NT)];
    multi_target_grad_tile_body<float, NT, FULL>(Bs, Cs, Ys, dMs, ntarget, nparam, grad, gradc, Lm, Al, ws, info, n_rt, batch, panel, aq);
}

template <class T>
hipError_t launch_multi_target_grad_tile(int n, int ntarget, int nparam, const T *Bs, const T *Cs, const T *Ys, const T *dMs, T *grad,
                                         T *gradc, T *Lm, T *Al, size_t batch, int *info, hipStream_t stream)
{
    if (!multi_target_grad_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    unsigned grid = predict_tile_grid(batch);  // the grid of the multi-target launcher
    const unsigned b = (unsigned)batch;
    // more than one group of targets and no dAlpha to read them back from: D n elements per workgroup, sized by the grid, which gives
    // way where that would pass the workspace cap of the blocked paths (the stride loop takes the rest; no bit depends on the grid)
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
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true, true, true, true, true, true, true, true>), dim3(grid), dim3(64), 0,
                               stream, Bs, Cs, Ys, dMs, ntarget, nparam, grad, gradc, Lm, Al, ws, info, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true, true, true, true, true, true, true, true>), dim3(grid), dim3(64), 0,
                               stream, Bs, Cs, Ys, dMs, ntarget, nparam, grad, gradc, Lm, Al, ws, info, n, b);
    });
    const hipError_t e = hipGetLastError();
    const hipError_t e2 = need_ws ? scratch_free(ws, stream) : hipSuccess;
    return e != hipSuccess ? e : e2;
}
}  // namespace matinv
