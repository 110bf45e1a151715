// spd_sweep.hpp -- the load and the full sweep of the one-wavefront GP tile kernels ("The shared SPD sweep"). One wavefront
// per matrix, lower-triangular 16 x 16 accumulator tiles, the next block's panel solved between the MFMAs of the current one; the sweep
// ends with W = -M^-1 in the lower tiles (diagonal tiles complete). The order of operations is that of spd_tile_body (tile_impl.hpp),
// plus PanelSolve::binfo.
// CALLED by logml_grad_tile_body, predict_tile_body, multi_target_tile_body and (the sweep only: its tiles are generated, not loaded)
// ard_tile_body.
// COPIED, line for line, in loo_tile_impl.hpp, loo_grad_tile_impl.hpp, predict_cov_tile_impl.hpp, multi_target_grad_tile_impl.hpp,
// trend_tile_impl.hpp, trend_grad_tile_impl.hpp and trend_loo_tile_impl.hpp, whose kernels did not compile to the same work (or the
// same speed) when they called this header: A CHANGE TO THE SWEEP HAS TO BE MADE HERE AND IN THOSE SEVEN FILES, or the outputs that
// are tied bit for bit across families (the logml of trend_grad and of trend, say) come apart.
#pragma once
#include "tile_common.hpp"

namespace matinv {

// the default on_pivots of spd_full_sweep: nothing is done with the pivots
struct SpdIgnorePivots {
    template <class PS>
    __device__ __forceinline__ void operator()(const PS &) const
    {
    }
};

// W = A^T tile layout, lower tiles only; in the diagonal tiles the strictly upper elements come from their mirror position, so only the
// lower triangle of A is ever read (spd_tile_body). Identity padding beyond n; crow (optional) is added to the diagonal.
template <class T, int NT, bool FULL>
__device__ __forceinline__ void spd_load_lower(typename TileGeo<T>::vec4 (&acc)[NT][NT], const T *A, const T *crow, int n, int q, int c)
{
    typedef TileGeo<T> G;
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
                if (crow && ti == tj && row == col && in) v += crow[row];
                acc[ti][tj][r] = v;
            }
        }
}

// The sweep over all 4 NT block steps. bad collects the lanes' acceptance tests, binfo the column of the first non-positive pivot + 1
// (both locals of the caller, zero on entry). on_pivots(ps) is called once per block step, as soon as the step's four pivots
// (ps.d[0][0], ps.u11, ps.u22, ps.u33, the same value in every lane) are complete: after the last stage of step 0, and right after
// stage 3 of every later step's solve, between the MFMAs of the step before it. A step of identity padding that a ragged form skips
// still reports its pivots, four exact ones.
template <class T, int NT, bool FULL, class OnPivots = SpdIgnorePivots>
__device__ __forceinline__ void spd_full_sweep(typename TileGeo<T>::vec4 (&acc)[NT][NT], T *panel, int n, int q, int c,
                                               unsigned long long &bad, int &binfo, OnPivots on_pivots = OnPivots())
{
    typedef TileGeo<T> G;
    constexpr int NKB = 4 * NT;
    typedef PanelSolve<NT, true, T> PS;
    T aop[NT], bop[NT];

    spd_panel_to_lds<NT, T>(panel, acc, 0, q, c);
    wave_lds_sync();
    {
        PS ps0;
        ps0.binfo = &binfo;
#pragma unroll
        for (int s = 0; s < PS::NSTAGE; ++s) ps0.stage(s, panel, 0, q, c, aop, bop, bad);
        on_pivots(ps0);
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
                            // the pivots of step kb + 1 are complete after stage 3 (logdet_tile_body)
                            if (e - 1 == 3) on_pivots(ps);
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
}

}  // namespace matinv
