// tile_impl.hpp -- device code of kernel family "TILE": one matrix per wavefront, register-resident in 16x16 fp64 MFMA
// accumulator tiles (v_mfma_f64_16x16x4_f64), for 16 < n <= 64 (n is padded to NT*16 with an identity block), and the symmetric
// sweep on lower tiles that serves the Cholesky entry point and the fused mean / variance up to 7 x 7 (fp64) / 10 x 10 (fp32) tiles.
// The translation units that instantiate it, one group of kernels each so that they build in parallel: tile_gj_kernels.hip /
// tile_gj_f32_kernels.hip = the natural-order Gauss-Jordan kernels, tile_kernels.hip / tile_f32_kernels.hip = the symmetric sweeps
// (tile_kernels.hip also holds the family's non-template helpers), tile_big_f32_kernels.hip, spd_wide_* / gp_spd_wide_* = the widest
// one-wavefront symmetric sweeps.
#pragma once
//
// Why MFMA for an inversion: Gauss-Jordan is a sequence of rank-1 updates whose cost on the VALU is dominated by
// BROADCASTING the multiplier column / pivot row across the wavefront (2 v_readlane per fp64 value per step).
// Blocking 4 elimination steps turns the trailing update into a rank-4 update  W += Aop(n x 4) * Bop(4 x n),
// which is exactly one 16x16x4 MFMA per tile: the matrix core performs the broadcast for free and runs at the
// fp64 vector FMA rate (MI355X: fp64 matrix peak = fp64 vector peak). The VALU is left with the 4-wide panel.
//
// Data layout in registers (C/D layout of v_mfma_f64_16x16x4_f64, guide section 3 "Fragment layout"):
//   lane l = 16*q + c, tile (ti, tj), register r  <->  W[16*ti + 4*r + q][16*tj + c]
// W is the TRANSPOSE of the caller's column-major matrix (W[i][j] = mem[i*n + j]) so the 16 lanes of a row
// group read 128 contiguous bytes; inv(A^T) = inv(A)^T, so storing the result the same way yields inv(A)
// column-major. Consequences that make the blocked step cheap:
//   * Bop for block kb (pivot rows 4kb..4kb+3) is the register acc[kb/4][tj][kb%4] AS IT STANDS (lane group q
//     already holds pivot row 4kb+q) -- no data movement;
//   * the 4 pivot columns live in 16 lanes (c in [4(kb%4), +4)) of tile column kb/4; they are staged through a
//     2 KB LDS buffer to be re-read in the A-operand layout (row per lane).
//
// Blocked in-place Gauss-Jordan step (D = W[K,K], K = 4 pivot indices):
//   Aop[i,:] = -W[i,K] D^-1 (i not in K),   Aop[K,:] = D^-1,
//   W[i,J] <- W[i,J] + Aop[i,:] W[K,J]  (i not in K),   W[K,J] <- Aop[K,:] W[K,J]   for the columns J not in K,
//   W[:,K] <- Aop.
// All of it is ONE MFMA per tile: C = W with the K rows and K columns zeroed, B = W[K,:] with I_4 on the K columns.
//
// Pivoting: this fast path eliminates in natural order and VERIFIES instead of searching: every multiplier it
// forms (the 6 LU multipliers of each 4x4 pivot block and every entry of Aop outside the pivot rows) must be
// <= TAU in magnitude (threshold pivoting acceptance; scale invariant; NaN/Inf fail it). A matrix that fails is
// appended to a device work list and redone, in the same stream, by the partially pivoted ROW kernel
// (row_kernels.hip; the LDS kernel for n > 64) -- no host round trip. Diagonally dominant / SPD batches (the reference's fixtures,
// tests/generate_inverse_matrices.m:12-18) never take the fallback.
//
// Symmetric input at 64 x 64 fp64 (MATINV_TILE_SYM_SWEEP): the Gauss-Jordan entry makes no symmetry promise to its caller, so the
// kernel finds out. After the loads it compares every element with its mirror, bit for bit, in registers (tile_asymmetry). A matrix
// whose two triangles agree -- the reference's fixtures R + R^T + n I, every covariance matrix -- takes the sweep of the Cholesky
// entry point (spd_tile_body below) on its ten lower tiles, 10 MFMAs per block step instead of 16, under the acceptance test of
// THIS kernel (multipliers <= TAU, no test of signs: symmetric indefinite input is served too); the upper tiles are rebuilt from
// the lower ones at the end, so the result is exactly symmetric. Any other matrix takes the full sweep and gets the bits it always
// got. Rejects of either arm go to the same work list.
//
// Replaces the 3n launches of /root/reference/src/gauss/batched_invert.cu:84-95.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>

#include "tile_common.hpp"
#include "tile_screen.hpp"

#ifndef MATINV_TILE_GATED_PANEL
#define MATINV_TILE_GATED_PANEL 1  // 0: the pivot-block solve in all 64 lanes (A/B builds)
#endif

#ifndef MATINV_TILE_SYM_SWEEP
#define MATINV_TILE_SYM_SWEEP 1  // 0: bitwise-symmetric 64 x 64 fp64 input takes the full sweep like any other (A/B builds)
#endif

#ifndef MATINV_TILE_SYM_FRONT
#define MATINV_TILE_SYM_FRONT 1  // 0: no symmetric-only kernel in front of the two-arm 64 x 64 fp64 kernel (A/B builds)
#endif

namespace matinv {

// ---- pieces of one block step ---------------------------------------------------------------------------------

// 5.+6. B operand (pivot rows as they stand, I_4 on the pivot columns) and C operand (zero on the pivot columns: the
// MFMA then leaves Aop * I_4 = the new K columns there; zero on the pivot rows: they become D^-1 * W[K,:], a pure
// product -- no cancellation, and the step stays exactly equivariant under power-of-two scaling of the input).
// ONE asm block per block step (r05; since r02 it was 2 NT blocks, each with its own s_nop):
//   (i)  the B operand is a copy of ONE register of each tile of tile row tK, which is then zeroed -- as C++ hipcc copies
//        the whole 4-register tile to keep the old value alive (768 v_mov per 64 x 64 matrix);
//   (ii) under EXEC narrowed to the panel lanes (a compile-time lane mask: lane l = 16 q + c, panel lanes are the 16 with
//        blk(c) == rK), the pivot columns of tile column tK are zeroed and bop[tK] takes the I_4 entry `eye` (hoisted by the
//        caller: blk(c) == rK and piv(c) == q  <=>  panel lane and piv(c) == q), instead of 4 NT selects on 64-bit values and a
//        per-step select for the I_4 entries.
// Operand order: bop[tK] and tile (tK, tK) come first, so the text depends on NT only (`j` walks tK, tK + 1, ... mod NT).
// Element rK of tile (tK, tK) is a pivot-row register: zeroed in (i) in every lane, it is not bound a second time in (ii).
// The block ends in s_nop 1 before EXEC is restored: the two wait states a VALU write needs before an MFMA reads the register
// as A, B or C (hipcc pads nothing inside an asm block). Every write of the block is at or before the last move, so that one
// pad covers all of them; the MFMAs follow after the s_mov (3 states in all).
#define MATINV_PREP_ROW(MOV, b, a) MOV " %" #b ", %" #a "\n\t" MOV " %" #a ", 0\n\t"
#define MATINV_PREP_ZERO(MOV, a) MOV " %" #a ", 0\n\t"
#define MATINV_PREP_TAIL(MOV, save, eye) MOV " %0, %" #eye "\n\ts_nop 1\n\ts_mov_b64 exec, %" #save
#define MATINV_PREP_SAVE(save, mask) "s_and_saveexec_b64 %" #save ", %" #mask "\n\t"
template <int NT, class T>
__device__ __forceinline__ void prep_operands(typename TileGeo<T>::vec4 (&acc)[NT][NT], T (&bop)[NT], int kb, T eye)
{
    static_assert(NT >= 1 && NT <= 4, "prep_operands: one asm text per tile count");
    const int tK = kb >> 2, rK = kb & 3;
    // panel lanes of block rK: f64 lanes c = 4 rK .. 4 rK + 3 of every lane group, f32 lanes c with c & 3 == rK
    const unsigned long long pmask = sizeof(T) == 8 ? 0x000F000F000F000FULL << (4 * rK) : 0x1111111111111111ULL << rK;
    unsigned long long save;
    auto J = [&](int i) { return (tK + i) % NT; };
    auto R = [&](int i) { return (rK + i) & 3; };
#define ROW(i) acc[tK][J(i)][rK]
#define COL(i, r) acc[J(i)][tK][R(r)]
    if constexpr (sizeof(T) == 8) {
#define MV "v_mov_b64_e32"
        if constexpr (NT == 1)
            asm volatile(MATINV_PREP_ROW(MV, 0, 1) MATINV_PREP_SAVE(5, 6)
                         MATINV_PREP_ZERO(MV, 2) MATINV_PREP_ZERO(MV, 3) MATINV_PREP_ZERO(MV, 4) MATINV_PREP_TAIL(MV, 5, 7)
                         : "=&v"(bop[J(0)]), "+v"(ROW(0)), "+v"(COL(0, 1)), "+v"(COL(0, 2)), "+v"(COL(0, 3)), "=&s"(save)
                         : "s"(pmask), "v"(eye) : "scc");
        else if constexpr (NT == 2)
            asm volatile(MATINV_PREP_ROW(MV, 0, 2) MATINV_PREP_ROW(MV, 1, 3) MATINV_PREP_SAVE(11, 12)
                         MATINV_PREP_ZERO(MV, 4) MATINV_PREP_ZERO(MV, 5) MATINV_PREP_ZERO(MV, 6)
                         MATINV_PREP_ZERO(MV, 7) MATINV_PREP_ZERO(MV, 8) MATINV_PREP_ZERO(MV, 9) MATINV_PREP_ZERO(MV, 10)
                         MATINV_PREP_TAIL(MV, 11, 13)
                         : "=&v"(bop[J(0)]), "=&v"(bop[J(1)]), "+v"(ROW(0)), "+v"(ROW(1)),
                           "+v"(COL(0, 1)), "+v"(COL(0, 2)), "+v"(COL(0, 3)),
                           "+v"(COL(1, 0)), "+v"(COL(1, 1)), "+v"(COL(1, 2)), "+v"(COL(1, 3)), "=&s"(save)
                         : "s"(pmask), "v"(eye) : "scc");
        else if constexpr (NT == 3)
            asm volatile(MATINV_PREP_ROW(MV, 0, 3) MATINV_PREP_ROW(MV, 1, 4) MATINV_PREP_ROW(MV, 2, 5) MATINV_PREP_SAVE(17, 18)
                         MATINV_PREP_ZERO(MV, 6) MATINV_PREP_ZERO(MV, 7) MATINV_PREP_ZERO(MV, 8)
                         MATINV_PREP_ZERO(MV, 9) MATINV_PREP_ZERO(MV, 10) MATINV_PREP_ZERO(MV, 11) MATINV_PREP_ZERO(MV, 12)
                         MATINV_PREP_ZERO(MV, 13) MATINV_PREP_ZERO(MV, 14) MATINV_PREP_ZERO(MV, 15) MATINV_PREP_ZERO(MV, 16)
                         MATINV_PREP_TAIL(MV, 17, 19)
                         : "=&v"(bop[J(0)]), "=&v"(bop[J(1)]), "=&v"(bop[J(2)]), "+v"(ROW(0)), "+v"(ROW(1)), "+v"(ROW(2)),
                           "+v"(COL(0, 1)), "+v"(COL(0, 2)), "+v"(COL(0, 3)),
                           "+v"(COL(1, 0)), "+v"(COL(1, 1)), "+v"(COL(1, 2)), "+v"(COL(1, 3)),
                           "+v"(COL(2, 0)), "+v"(COL(2, 1)), "+v"(COL(2, 2)), "+v"(COL(2, 3)), "=&s"(save)
                         : "s"(pmask), "v"(eye) : "scc");
        else
            asm volatile(MATINV_PREP_ROW(MV, 0, 4) MATINV_PREP_ROW(MV, 1, 5) MATINV_PREP_ROW(MV, 2, 6) MATINV_PREP_ROW(MV, 3, 7)
                         MATINV_PREP_SAVE(23, 24)
                         MATINV_PREP_ZERO(MV, 8) MATINV_PREP_ZERO(MV, 9) MATINV_PREP_ZERO(MV, 10)
                         MATINV_PREP_ZERO(MV, 11) MATINV_PREP_ZERO(MV, 12) MATINV_PREP_ZERO(MV, 13) MATINV_PREP_ZERO(MV, 14)
                         MATINV_PREP_ZERO(MV, 15) MATINV_PREP_ZERO(MV, 16) MATINV_PREP_ZERO(MV, 17) MATINV_PREP_ZERO(MV, 18)
                         MATINV_PREP_ZERO(MV, 19) MATINV_PREP_ZERO(MV, 20) MATINV_PREP_ZERO(MV, 21) MATINV_PREP_ZERO(MV, 22)
                         MATINV_PREP_TAIL(MV, 23, 25)
                         : "=&v"(bop[J(0)]), "=&v"(bop[J(1)]), "=&v"(bop[J(2)]), "=&v"(bop[J(3)]),
                           "+v"(ROW(0)), "+v"(ROW(1)), "+v"(ROW(2)), "+v"(ROW(3)),
                           "+v"(COL(0, 1)), "+v"(COL(0, 2)), "+v"(COL(0, 3)),
                           "+v"(COL(1, 0)), "+v"(COL(1, 1)), "+v"(COL(1, 2)), "+v"(COL(1, 3)),
                           "+v"(COL(2, 0)), "+v"(COL(2, 1)), "+v"(COL(2, 2)), "+v"(COL(2, 3)),
                           "+v"(COL(3, 0)), "+v"(COL(3, 1)), "+v"(COL(3, 2)), "+v"(COL(3, 3)), "=&s"(save)
                         : "s"(pmask), "v"(eye) : "scc");
#undef MV
    } else {
#define MV "v_mov_b32_e32"
        if constexpr (NT == 1)
            asm volatile(MATINV_PREP_ROW(MV, 0, 1) MATINV_PREP_SAVE(5, 6)
                         MATINV_PREP_ZERO(MV, 2) MATINV_PREP_ZERO(MV, 3) MATINV_PREP_ZERO(MV, 4) MATINV_PREP_TAIL(MV, 5, 7)
                         : "=&v"(bop[J(0)]), "+v"(ROW(0)), "+v"(COL(0, 1)), "+v"(COL(0, 2)), "+v"(COL(0, 3)), "=&s"(save)
                         : "s"(pmask), "v"(eye) : "scc");
        else if constexpr (NT == 2)
            asm volatile(MATINV_PREP_ROW(MV, 0, 2) MATINV_PREP_ROW(MV, 1, 3) MATINV_PREP_SAVE(11, 12)
                         MATINV_PREP_ZERO(MV, 4) MATINV_PREP_ZERO(MV, 5) MATINV_PREP_ZERO(MV, 6)
                         MATINV_PREP_ZERO(MV, 7) MATINV_PREP_ZERO(MV, 8) MATINV_PREP_ZERO(MV, 9) MATINV_PREP_ZERO(MV, 10)
                         MATINV_PREP_TAIL(MV, 11, 13)
                         : "=&v"(bop[J(0)]), "=&v"(bop[J(1)]), "+v"(ROW(0)), "+v"(ROW(1)),
                           "+v"(COL(0, 1)), "+v"(COL(0, 2)), "+v"(COL(0, 3)),
                           "+v"(COL(1, 0)), "+v"(COL(1, 1)), "+v"(COL(1, 2)), "+v"(COL(1, 3)), "=&s"(save)
                         : "s"(pmask), "v"(eye) : "scc");
        else if constexpr (NT == 3)
            asm volatile(MATINV_PREP_ROW(MV, 0, 3) MATINV_PREP_ROW(MV, 1, 4) MATINV_PREP_ROW(MV, 2, 5) MATINV_PREP_SAVE(17, 18)
                         MATINV_PREP_ZERO(MV, 6) MATINV_PREP_ZERO(MV, 7) MATINV_PREP_ZERO(MV, 8)
                         MATINV_PREP_ZERO(MV, 9) MATINV_PREP_ZERO(MV, 10) MATINV_PREP_ZERO(MV, 11) MATINV_PREP_ZERO(MV, 12)
                         MATINV_PREP_ZERO(MV, 13) MATINV_PREP_ZERO(MV, 14) MATINV_PREP_ZERO(MV, 15) MATINV_PREP_ZERO(MV, 16)
                         MATINV_PREP_TAIL(MV, 17, 19)
                         : "=&v"(bop[J(0)]), "=&v"(bop[J(1)]), "=&v"(bop[J(2)]), "+v"(ROW(0)), "+v"(ROW(1)), "+v"(ROW(2)),
                           "+v"(COL(0, 1)), "+v"(COL(0, 2)), "+v"(COL(0, 3)),
                           "+v"(COL(1, 0)), "+v"(COL(1, 1)), "+v"(COL(1, 2)), "+v"(COL(1, 3)),
                           "+v"(COL(2, 0)), "+v"(COL(2, 1)), "+v"(COL(2, 2)), "+v"(COL(2, 3)), "=&s"(save)
                         : "s"(pmask), "v"(eye) : "scc");
        else
            asm volatile(MATINV_PREP_ROW(MV, 0, 4) MATINV_PREP_ROW(MV, 1, 5) MATINV_PREP_ROW(MV, 2, 6) MATINV_PREP_ROW(MV, 3, 7)
                         MATINV_PREP_SAVE(23, 24)
                         MATINV_PREP_ZERO(MV, 8) MATINV_PREP_ZERO(MV, 9) MATINV_PREP_ZERO(MV, 10)
                         MATINV_PREP_ZERO(MV, 11) MATINV_PREP_ZERO(MV, 12) MATINV_PREP_ZERO(MV, 13) MATINV_PREP_ZERO(MV, 14)
                         MATINV_PREP_ZERO(MV, 15) MATINV_PREP_ZERO(MV, 16) MATINV_PREP_ZERO(MV, 17) MATINV_PREP_ZERO(MV, 18)
                         MATINV_PREP_ZERO(MV, 19) MATINV_PREP_ZERO(MV, 20) MATINV_PREP_ZERO(MV, 21) MATINV_PREP_ZERO(MV, 22)
                         MATINV_PREP_TAIL(MV, 23, 25)
                         : "=&v"(bop[J(0)]), "=&v"(bop[J(1)]), "=&v"(bop[J(2)]), "=&v"(bop[J(3)]),
                           "+v"(ROW(0)), "+v"(ROW(1)), "+v"(ROW(2)), "+v"(ROW(3)),
                           "+v"(COL(0, 1)), "+v"(COL(0, 2)), "+v"(COL(0, 3)),
                           "+v"(COL(1, 0)), "+v"(COL(1, 1)), "+v"(COL(1, 2)), "+v"(COL(1, 3)),
                           "+v"(COL(2, 0)), "+v"(COL(2, 1)), "+v"(COL(2, 2)), "+v"(COL(2, 3)),
                           "+v"(COL(3, 0)), "+v"(COL(3, 1)), "+v"(COL(3, 2)), "+v"(COL(3, 3)), "=&s"(save)
                         : "s"(pmask), "v"(eye) : "scc");
#undef MV
    }
#undef ROW
#undef COL
}
#undef MATINV_PREP_ROW
#undef MATINV_PREP_ZERO
#undef MATINV_PREP_TAIL
#undef MATINV_PREP_SAVE

// ---- the symmetric arm of the 64 x 64 fp64 kernel (MATINV_TILE_SYM_SWEEP) ------------------------------------------------------
// A bitwise-symmetric matrix has a symmetric inverse, and the sweep of spd_tile_body reaches it on the NT (NT + 1) / 2 lower tiles:
// 10 MFMAs per block step instead of 16. gj_tile_body classifies every matrix after its loads and takes that sweep -- with the
// Gauss-Jordan ACCEPTANCE test, not the Cholesky one -- when the matrix qualifies. The pieces:

// asym |= ballot(bits of a != bits of b). An INTEGER compare: +0.0 / -0.0 differ, a NaN equals itself, so a matrix counts as
// symmetric exactly when both triangles hold the same bits. Inline asm for the reason given at note_fail.
__device__ __forceinline__ void note_differs(unsigned long long &asym, double a, double b)
{
    asm volatile("v_cmp_ne_u64_e64 vcc, %1, %2\n\ts_or_b64 %0, %0, vcc" : "+s"(asym) : "v"(a), "v"(b) : "vcc");
}

// Lanes in which some element differs from its mirror. The relabelling of PAIRED is a symmetric permutation, so the mirror of
// lane (q, c), register r of tile (ti, tj) is lane (c & 3, 4 r + q), register c >> 2 of tile (tj, ti): one tile of each of the six
// off-diagonal pairs, and each diagonal tile, goes through the padded LDS buffer and comes back transposed.
template <int NT>
__device__ __forceinline__ unsigned long long tile_asymmetry(double *tbuf, const v4d (&acc)[NT][NT], int q, int c)
{
    typedef TileGeo<double> G;
    unsigned long long asym = 0;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj) {
            // Wave-uniform early leave: a mismatch has been seen, the verdict is in. Without it a batch that is not symmetric pays all
            // ten round trips before its sweep starts: R + n I, 100 000 matrices, 3.5 % slower than without the classification.
            if (asym != 0) continue;
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < 4; ++r) tbuf[G::trow(r, q) * TILE_TSTRIDE + c] = acc[ti][tj][r];
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < 4; ++r) note_differs(asym, tbuf[c * TILE_TSTRIDE + G::trow(r, q)], acc[tj][ti][r]);
        }
    return asym;
}

// Every tile of a 4 x 4 accumulator array as ONE 256-bit register tuple at this point of the program (no instruction). Without it
// hipcc keeps the freshly loaded elements in separate register pairs through the classification and assembles the MFMA tuples of
// both arms in front of the branch: two copies of the matrix alive at once, and scratch.
__device__ __forceinline__ void pin_tiles(v4d (&acc)[4][4])
{
    asm volatile("" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]), "+v"(acc[1][0]), "+v"(acc[1][1]),
                      "+v"(acc[1][2]), "+v"(acc[1][3]), "+v"(acc[2][0]), "+v"(acc[2][1]), "+v"(acc[2][2]), "+v"(acc[2][3]),
                      "+v"(acc[3][0]), "+v"(acc[3][1]), "+v"(acc[3][2]), "+v"(acc[3][3]));
}

// (The block-step loop below -- the (a) / (b) order of the MFMAs and the event schedule that places the pieces of the next panel
// between them -- exists three times: spd_tile_body below, loo_tile_body in loo_tile_impl.hpp, and here. A change of the look-ahead
// schedule belongs in all three.)
// The look-ahead sweep of spd_tile_body on the lower tiles of acc (the upper ones are not read), with the acceptance test of the
// natural-order kernel: the six LU multipliers of each pivot block and every A-operand entry outside the pivot rows <= TAU, no test
// of the pivots' sign -- a symmetric INDEFINITE matrix that passes is inverted here as well. Block step 0 reads the panel as it was
// loaded, through the stages panel_solve runs: the same operations on the same values in the same order as the full sweep's first
// block step and as the screening kernel (tile_screen.hpp), hence their verdict. Leaves W = -A^-1 in the lower tiles.
template <int NT, bool GATED, class T>
__device__ __forceinline__ void sym_tile_sweep(typename TileGeo<T>::vec4 (&acc)[NT][NT], T *panel, int q, int c, unsigned long long &bad)
{
    typedef TileGeo<T> G;
    typedef PanelSolve<NT, false, T, GATED, true> PS;
    constexpr int NKB = 4 * NT;
    T aop[NT], bop[NT];
    spd_panel_to_lds<NT, T>(panel, acc, 0, q, c);
    wave_lds_sync();
    {
        PS ps0;
#pragma unroll
        for (int s = 0; s < PS::NSTAGE; ++s) ps0.stage(s, panel, 0, q, c, aop, bop, bad);
    }
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        spd_prep_operands<NT, T>(acc, bop, kb, q, c);
        if (kb + 1 < NKB) {
            const int tn = (kb + 1) >> 2;
            // (a) the tiles the next panel is read from: column tn (ti >= tn) and row tn (tj < tn)
#pragma unroll
            for (int ti = tn; ti < NT; ++ti) acc[ti][tn] = G::mfma(aop[ti], bop[tn], acc[ti][tn]);
#pragma unroll
            for (int tj = 0; tj < tn; ++tj) acc[tn][tj] = G::mfma(aop[tn], bop[tj], acc[tn][tj]);
            // (b) the other lower tiles between the pieces of the next panel, as in spd_tile_body
            constexpr int NB = NT * (NT + 1) / 2 - NT;
            constexpr int NS = PS::NSTAGE;
            T aop_next[NT], bop_next[NT];
            PS ps;
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
                for (int tj = 0; tj <= ti; ++tj) {
                    if (ti == tn || tj == tn) continue;
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
                for (int tj = 0; tj <= ti; ++tj) acc[ti][tj] = G::mfma(aop[ti], bop[tj], acc[ti][tj]);
        }
    }
}

// W = -A^-1 in the lower tiles -> A^-1 in all of them: the sign flipped, the six upper tiles rebuilt as the transposes of their
// mirrors, and the upper triangle of each diagonal tile taken from its lower one (the sweep keeps the two equal only up to
// rounding), all through the padded LDS buffer. The result is bitwise symmetric.
template <int NT>
__device__ __forceinline__ void sym_tile_finish(double *tbuf, v4d (&acc)[NT][NT], int q, int c)
{
    typedef TileGeo<double> G;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj <= ti; ++tj) {
            acc[ti][tj] = -acc[ti][tj];
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < 4; ++r) tbuf[G::trow(r, q) * TILE_TSTRIDE + c] = acc[ti][tj][r];
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double t = tbuf[c * TILE_TSTRIDE + G::trow(r, q)];
                acc[tj][ti][r] = (ti != tj || G::trow(r, q) < c) ? t : acc[tj][ti][r];
            }
        }
}

// One matrix per wavefront; see the file header. T = double or float.
// The 4 x 4-tile fp64 kernels (FULL, both values of EARLY) have two arms: loads -> classification -> [symmetric: sym_tile_sweep on
// the lower tiles, sym_tile_finish | otherwise: the block steps below] -> stores / work list. Both arms end in the same store text,
// expanded once per arm (see `leave` at the end of the body for why they do not meet in front of it). The arms share no per-lane
// constant: the symmetric one launders its own copy of the lane coordinates. Figures, tools/kernel_regs.py: 222 VGPRs (EARLY: 224),
// no scratch, no AGPRs; as a diamond that meets at one copy of the stores 256 VGPRs and 132 - 328 B of scratch.
// (Tried, not kept: letting a matrix that has already failed the acceptance test skip the remaining block steps through
// nested scalar branches after every fourth step -- no loop exit, accumulators dead on the rejected path. hipcc answers the
// control flow with 256 VGPRs + 344 B of scratch in the headline kernel instead of 212 and none.)
// (Tried and measured, not kept: pinning "B operand = copy of the pivot-row register, then zero it" as two asm moves per tile
// column -- hipcc copies the whole 4-register tile instead, 768 v_mov per 64x64 matrix. The asm version issues 173 fewer
// VALU instructions per matrix (2 653 -> 2 480, 200 VGPRs instead of 212) and, A/B on one box, is 1 % faster at 64x64
// (1.556 vs 1.575 ms per 100 k), 2-6 % at 48x48. But hipcc inserts no hazard wait states after an asm block: a move inside it
// followed directly by the MFMA that reads the register is a VALU-write -> MFMA-read hazard, and the same change in the
// four-wave kernel did produce wrong results. Not worth 1 %.)
// (Tried and measured, not kept: streaming half of the wave's NEXT matrix into LDS with global_load_lds_dwordx4 during
// the elimination. The exposed time per matrix is load LATENCY, not bytes: 1.651 ms with, 1.645 ms without at 100 k x 64^2.)
template <class T, int NT, bool FULL, bool LOOKAHEAD, bool EARLY = false>
__device__ __forceinline__ void gj_tile_body(BatchRef<const T> Ain, BatchRef<T> Xout, int *info, int n_rt, unsigned batch,
                                             int *work_count, int *work_list, T *panel, const int *in_count, const int *in_list)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    typedef typename G::vec2 vec2;
    constexpr int N = 16 * NT;
    constexpr int NKB = 4 * NT;
    // PAIRED: 16-byte global accesses. The labels (tile, register, lane) -> (matrix row, matrix column) are ours to
    // choose as long as pivot block kb uses the same index set for its rows (tile row kb/4, register kb%4, q = 0..3)
    // and columns (tile column kb/4, lanes c = 4(kb%4)..+3). With
    //     row(ti, r, q) = 32(ti>>1) + 8r + 2q + (ti&1),    col(tj, c) = 32(tj>>1) + 2c + (tj&1)
    // lane c of the tile-column pair (2u, 2u+1) owns the ADJACENT columns 32u+2c, 32u+2c+1 of its row, i.e. one
    // 16-byte access feeds two tiles and a 16-lane group covers 256 contiguous bytes. Nothing else in the kernel
    // depends on the relabelling (a symmetric permutation of the matrix: inv(P A P^T) = P inv(A) P^T).
    constexpr bool PAIRED = FULL && (NT % 2 == 0);
    // the pivot-block solve in one lane per row of 16 (PanelSolve, GATED): the headline instantiation
    constexpr bool GATED = MATINV_TILE_GATED_PANEL && sizeof(T) == 8 && NT == 4 && FULL && LOOKAHEAD && !EARLY;
    // the symmetric arm (see tile_asymmetry / sym_tile_sweep / sym_tile_finish above): both instantiations of the 64 x 64 fp64
    // kernel, the one behind the screening pass included -- the arm is the same code in both, so they give the same bits
    constexpr bool SYM = MATINV_TILE_SYM_SWEEP && sizeof(T) == 8 && NT == 4 && FULL && LOOKAHEAD;
    const int l = threadIdx.x;

    // accept-list form (behind the screening kernel below): in_list[0 .. *in_count)
    const unsigned todo = in_count ? (unsigned)*in_count : batch;
    for (unsigned item = blockIdx.x; item < todo; item += gridDim.x) {
        const unsigned mat = in_list ? (unsigned)in_list[item] : item;
        const T *A = Ain.at_uniform(mat);
        T *X = Xout.at_uniform(mat);
        // run-time n: made opaque once per matrix, otherwise LICM hoists the 16 NT^2 tile offsets (products with n) and
        // the bounds predicates of both the load and the store loop out of this loop (370-510 VGPRs, one wave per SIMD)
        int n = FULL ? N : n_rt;
        if (!FULL) asm volatile("" : "+s"(n));
        // Launder the lane coordinates once per matrix: otherwise LICM hoists the ~60 per-lane constants of the 4*NT
        // unrolled block steps (I_4 lanes, e_q entries, lane masks) out of this loop and the allocator spills them.
        int q = l >> 4, c = l & 15;
        // (addresses keep using the un-laundered lane id so they stay in saddr + 32-bit voffset + immediate form)
        const unsigned lane_off = (unsigned)(G::trow(0, l >> 4) * n + (l & 15));
        asm volatile("" : "+v"(q), "+v"(c));
        // I_4 entry of the B operand in the panel lanes of any block (prep_operands), once per matrix
        const T eye = G::piv(c) == q ? (T)1 : (T)0;
        // one per-lane element offset + wave-uniform (compile-time when FULL) tile offsets keep the 16*NT*NT
        // addresses out of VGPRs
        vec4 acc[NT][NT];
        if (PAIRED) {
            // 16-byte accesses: see the index relabelling above (rows/cols of tile pairs interleaved by parity)
            const unsigned lane_off2 = (unsigned)(2 * G::trow(0, l >> 4) * N + 2 * (l & 15));
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int u = 0; u < NT / 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned uoff = (unsigned)((32 * (ti >> 1) + 2 * G::trow(r, 0) + (ti & 1)) * N + 32 * u);
                        const vec2 v = __builtin_nontemporal_load(reinterpret_cast<const vec2 *>(A + uoff + lane_off2));
                        acc[ti][2 * u][r] = v[0];
                        acc[ti][2 * u + 1][r] = v[1];
                    }
        } else {
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * ti + G::trow(r, q), col = 16 * tj + c;
                        // identity padding beyond n: blockdiag(A, I)^-1 = blockdiag(A^-1, I). Only the last tile row and
                        // column can reach beyond n (n > 16 (NT - 1)): the interior tiles load without a predicate.
                        const unsigned uoff = (unsigned)((16 * ti + G::trow(r, 0)) * n + 16 * tj);
                        const bool edge = !FULL && (ti == NT - 1 || tj == NT - 1);
                        acc[ti][tj][r] = (!edge || (row < n && col < n)) ? A[uoff + lane_off] : ((row == col) ? (T)1 : (T)0);
                    }
        }
        unsigned long long bad = 0;  // wave-uniform: lanes that saw a multiplier above TAU (or NaN)
        T aop[NT], bop[NT];

        // Symmetric input? Wave-uniform, decided in registers once the loads are in. The verdict has two ARMS, each a whole sweep
        // that ends in the stores -- not a way out of the unrolled chain of block steps (see the early-exit notes above).
        bool sym = false;
#ifndef MATINV_TILE_LDST_ONLY
        if constexpr (SYM) {
            pin_tiles(acc);
            sym = tile_asymmetry<NT>(panel, acc, q, c) == 0;
        }
#endif

        // -DMATINV_TILE_LDST_ONLY (tools/build_ldst_variant.sh, profiling only): no elimination at all -- the kernel's loads and
        // stores in their real access pattern and launch shape, to price what the memory side alone costs
#ifdef MATINV_TILE_LDST_ONLY
        if (false) {
#else
        if (SYM && sym) {
            // the symmetric arm: after the other one, below
        } else if (LOOKAHEAD) {
#endif
            panel_to_lds<NT, T>(panel, acc, 0, q, c);
            wave_lds_sync();
            panel_solve<NT, GATED>(panel, 0, q, c, aop, bad);
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                // ragged n: a block step whose four columns are all identity padding changes nothing (pivot block I,
                // pivot rows and columns zero elsewhere) -- skipped on a wave-uniform branch. Only the last tile column
                // can hold such blocks. (The look-ahead of the step before it has solved that panel for nothing.)
                if (!FULL && kb > 4 * (NT - 1) && kb - 4 * (NT - 1) >= G::real_blocks(n - 16 * (NT - 1))) continue;
                prep_operands<NT, T>(acc, bop, kb, eye);
                if (kb + 1 < NKB) {
                    const int tn = (kb + 1) >> 2;
                    // (a) the tile column holding the next pivot columns first ...
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti)
                        acc[ti][tn] = G::mfma(aop[ti], bop[tn], acc[ti][tn]);
                    // (b) the other NT*(NT-1) tiles, pinned in program order between the pieces of the next
                    //     panel: 2 MFMAs cover the latency of (a) before the panel columns are read back, then one
                    //     MFMA after every stage. sched_barrier(0) keeps hipcc from re-clustering them.
                    constexpr int NB = NT * (NT - 1);
                    int pend = 0;  // folds to a literal: everything here is fully unrolled
                    auto issue_b = [&](int count) {
#pragma unroll
                        for (int z = 0; z < count; ++z) {
                            if (pend < NB) {
                                const int tjx = pend / NT, ti = pend % NT;
                                const int tj = tjx + (tjx >= tn ? 1 : 0);
                                acc[ti][tj] = G::mfma(aop[ti], bop[tj], acc[ti][tj]);
                                ++pend;
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    };
                    __builtin_amdgcn_sched_barrier(0);
                    issue_b(2);
                    wave_lds_sync();  // panel(kb) has been consumed (aop is in registers)
                    panel_to_lds<NT, T>(panel, acc, kb + 1, q, c);
                    wave_lds_sync();
                    __builtin_amdgcn_sched_barrier(0);
                    T aop_next[NT];
                    PanelSolve<NT, false, T, GATED> ps;
                    constexpr int NS = PanelSolve<NT, false, T, GATED>::NSTAGE;
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        // spread the remaining MFMAs evenly over the stages
                        issue_b(((NB - 2) * (s + 1)) / NS - ((NB - 2) * s) / NS);
                        ps.stage(s, panel, kb + 1, q, c, aop_next, bad);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    issue_b(NB);  // whatever is left (NT < 3)
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti) aop[ti] = aop_next[ti];
                    // r04, EARLY only (the instantiations that run behind the screening pass): ONE way out for a matrix that has already
                    // failed the acceptance test -- after the block steps of the first tile column (the panel of block 4 is solved by now:
                    // five of the 4 NT tests). A general matrix that slipped through the screen (one in five U(0,1) matrices passes block 0)
                    // then costs a quarter of the sweep. Not in the default instantiation: with this one branch hipcc allocates the 4 x 4-tile
                    // kernel 256 VGPRs and spills 79 (212 and none without); the nested form -- a test after every fourth step -- was worse.
                    if (EARLY && NT > 1 && kb == 3 && bad != 0) break;
                } else {
#pragma unroll
                    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                        for (int tj = 0; tj < NT; ++tj)
                            acc[ti][tj] = G::mfma(aop[ti], bop[tj], acc[ti][tj]);
                }
            }
        } else {
#ifdef MATINV_TILE_LDST_ONLY
            (void)aop, (void)bop;
#else
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                if (!FULL && kb > 4 * (NT - 1) && kb - 4 * (NT - 1) >= G::real_blocks(n - 16 * (NT - 1))) continue;  // all-padding block step (see above)
                panel_to_lds<NT, T>(panel, acc, kb, q, c);
                wave_lds_sync();
                panel_solve<NT>(panel, kb, q, c, aop, bad);
                wave_lds_sync();  // panel is rewritten by the next block step
                prep_operands<NT, T>(acc, bop, kb, eye);
                // 7. rank-4 update of every tile on the matrix cores
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int tj = 0; tj < NT; ++tj)
                        acc[ti][tj] = G::mfma(aop[ti], bop[tj], acc[ti][tj]);
            }
#endif
        }

        // The way out: accepted -> the stores and info = 0, rejected -> the work list. The kernel with the symmetric arm leaves from
        // each arm through its own copy of this text (a lambda). Meeting at ONE copy makes every tile live across both arms, and hipcc
        // then assembles the MFMA register tuples of both in front of the branch: 256 VGPRs and 132 - 328 B of scratch, whatever
        // pins the tiles. Every other instantiation keeps the text in line, as it was -- hence the macro: called as a lambda everywhere
        // the same text changes the register figures of the ragged kernels (NT = 3: 177 -> 169 VGPRs, NT = 4: 256 + 100 B of scratch
        // -> 247 and none), which were not measured here and therefore stay what they were. The lambda itself is declared in the
        // instantiation with the arm only: declared and unused elsewhere it still moved register copies in the 48 x 48 kernel and
        // changed the code, and the bits, of the fp32 kernels.
#define MATINV_GJ_TILE_LEAVE                                                                                                \
        if (bad == 0) {                                                                                                     \
            if (PAIRED) {                                                                                                   \
                const unsigned lane_off2 = (unsigned)(2 * G::trow(0, l >> 4) * N + 2 * (l & 15));                           \
_Pragma("unroll")                                                                                                           \
                for (int ti = 0; ti < NT; ++ti)                                                                             \
_Pragma("unroll")                                                                                                           \
                    for (int u = 0; u < NT / 2; ++u)                                                                        \
_Pragma("unroll")                                                                                                           \
                        for (int r = 0; r < 4; ++r) {                                                                       \
                            const unsigned uoff = (unsigned)((32 * (ti >> 1) + 2 * G::trow(r, 0) + (ti & 1)) * N + 32 * u); \
                            vec2 v;                                                                                         \
                            v[0] = acc[ti][2 * u][r];                                                                       \
                            v[1] = acc[ti][2 * u + 1][r];                                                                   \
                            __builtin_nontemporal_store(v, reinterpret_cast<vec2 *>(X + uoff + lane_off2));                 \
                        }                                                                                                   \
            } else {                                                                                                        \
_Pragma("unroll")                                                                                                           \
                for (int ti = 0; ti < NT; ++ti)                                                                             \
_Pragma("unroll")                                                                                                           \
                    for (int tj = 0; tj < NT; ++tj)                                                                         \
_Pragma("unroll")                                                                                                           \
                        for (int r = 0; r < 4; ++r) {                                                                       \
                            const int row = 16 * ti + G::trow(r, q), col = 16 * tj + c;                                     \
                            const unsigned uoff = (unsigned)((16 * ti + G::trow(r, 0)) * n + 16 * tj);                      \
                            const bool edge = !FULL && (ti == NT - 1 || tj == NT - 1);                                      \
                            if (!edge || (row < n && col < n)) X[uoff + lane_off] = acc[ti][tj][r];                         \
                        }                                                                                                   \
            }                                                                                                               \
            if (info && l == 0) info[mat] = 0;                                                                              \
        } else if (l == 0) {                                                                                                \
            const int slot = atomicAdd(work_count, 1);                                                                      \
            work_list[slot] = (int)mat;                                                                                     \
        }
        if constexpr (SYM) {
            auto leave = [&]() {
                MATINV_GJ_TILE_LEAVE
            };
            if (!sym) {
                leave();
            } else {
                // lane coordinates of the arm's own: its per-lane constants are then formed inside it and do not live across the
                // other arm, which has no register to spare for them
                int qs = q, cs = c;
                asm volatile("" : "+v"(qs), "+v"(cs));
                wave_lds_sync();  // the transpose buffer becomes the panel
                sym_tile_sweep<NT, MATINV_TILE_GATED_PANEL != 0, T>(acc, panel, qs, cs, bad);
                wave_lds_sync();  // ... and the transpose buffer again
                if (bad == 0) sym_tile_finish<NT>(panel, acc, qs, cs);  // wave-uniform; a reject goes to the work list as it is
                leave();
            }
        } else {
            MATINV_GJ_TILE_LEAVE
        }
        if (LOOKAHEAD) wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// ---- the symmetric-only form of the 64 x 64 fp64 kernel (MATINV_TILE_SYM_FRONT) ------------------------------------------------
// The two-arm kernel above is allocated for its full sweep (222 VGPRs, two waves per SIMD) although a symmetric batch never runs it.
// This form holds the symmetric arm alone -- the same sym_tile_sweep, sym_tile_finish and store text, hence the same bits -- at three
// waves per SIMD. A matrix that is not symmetric is not inverted here: its index goes to a list of its own, and the two-arm kernel
// takes that list as its accept list (launch_gj_tile_natural). Nothing is stored for it and its info is left alone.

// Item k of the classification: the six off-diagonal pairs first (their upper tiles are dead once compared), then the diagonal tiles.
constexpr int sym_cls_ti(int k) { return k < 6 ? (k < 1 ? 1 : (k < 3 ? 2 : 3)) : k - 6; }
constexpr int sym_cls_tj(int k) { return k < 6 ? (k < 1 ? 0 : (k < 3 ? k - 1 : k - 3)) : k - 6; }

// The verdict of tile_asymmetry (== 0), CB tiles per LDS round trip and without the early leave: every element against its mirror as
// 64-bit integers. tbuf: CB padded 16 x 16 transpose buffers.
template <int CB>
__device__ __forceinline__ bool tile_symmetric_batched(double *tbuf, const v4d (&acc)[4][4], int q, int c)
{
    typedef TileGeo<double> G;
    constexpr int NITEM = 10, TSZ = 16 * TILE_TSTRIDE;
    unsigned long long asym = 0;
#pragma unroll
    for (int g = 0; g < NITEM; g += CB) {
        wave_lds_sync();
#pragma unroll
        for (int k = g; k < g + CB && k < NITEM; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) tbuf[(k - g) * TSZ + G::trow(r, q) * TILE_TSTRIDE + c] = acc[sym_cls_ti(k)][sym_cls_tj(k)][r];
        wave_lds_sync();
#pragma unroll
        for (int k = g; k < g + CB && k < NITEM; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                note_differs(asym, tbuf[(k - g) * TSZ + c * TILE_TSTRIDE + G::trow(r, q)], acc[sym_cls_tj(k)][sym_cls_ti(k)][r]);
    }
    return asym == 0;
}

constexpr int TILE_SYM_CLS_BATCH = 5;  // tiles per round trip of the classification: two round trips instead of ten, 10 880 B of LDS

__device__ __forceinline__ void gj_tile_sym_body(BatchRef<const double> Ain, BatchRef<double> Xout, int *info, unsigned batch, int *work_count,
                                                 int *work_list, int *ns_count, int *ns_list, double *panel)
{
    typedef double T;
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    typedef typename G::vec2 vec2;
    constexpr int NT = 4, N = 16 * NT;
    constexpr bool FULL = true, PAIRED = true;  // what the store text of gj_tile_body reads
    const int l = threadIdx.x;

    for (unsigned mat = blockIdx.x; mat < batch; mat += gridDim.x) {
        const T *A = Ain.at_uniform(mat);
        T *X = Xout.at_uniform(mat);
        constexpr int n = N;
        constexpr unsigned lane_off = 0;  // the store text's other branch only
        int q = l >> 4, c = l & 15;
        asm volatile("" : "+v"(q), "+v"(c));  // see gj_tile_body
        vec4 acc[NT][NT];
        {
            const unsigned lane_off2 = (unsigned)(2 * G::trow(0, l >> 4) * N + 2 * (l & 15));
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int u = 0; u < NT / 2; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned uoff = (unsigned)((32 * (ti >> 1) + 2 * G::trow(r, 0) + (ti & 1)) * N + 32 * u);
                        const vec2 v = __builtin_nontemporal_load(reinterpret_cast<const vec2 *>(A + uoff + lane_off2));
                        acc[ti][2 * u][r] = v[0];
                        acc[ti][2 * u + 1][r] = v[1];
                    }
        }
        unsigned long long bad = 0;
        if (tile_symmetric_batched<TILE_SYM_CLS_BATCH>(panel, acc, q, c)) {
            wave_lds_sync();  // the transpose buffer becomes the panel
            sym_tile_sweep<NT, MATINV_TILE_GATED_PANEL != 0, T>(acc, panel, q, c, bad);
            wave_lds_sync();  // ... and the transpose buffer again
            if (bad == 0) sym_tile_finish<NT>(panel, acc, q, c);  // wave-uniform; a reject goes to the work list as it is
            MATINV_GJ_TILE_LEAVE
        } else if (l == 0) {
            const int slot = atomicAdd(ns_count, 1);
            ns_list[slot] = (int)mat;
        }
        wave_lds_sync();
    }
}
#undef MATINV_GJ_TILE_LEAVE


// FULL: n == 16*NT known at compile time (constant address offsets, no bounds checks).
// LOOKAHEAD: software pipelining across block steps -- the tile column that holds the NEXT pivot columns is updated
// first, the next panel is extracted and solved while the remaining MFMAs of the current step are in flight.
template <int NT, bool FULL, bool LOOKAHEAD, bool EARLY = false>
__global__ __launch_bounds__(64, 2) void matinv_gj_tile_f64(BatchRef<const double> Ain,
                                                                                 BatchRef<double> Xout, int *info,
                                                                                 int n_rt, unsigned batch,
                                                                                 int *work_count, int *work_list, const int *in_count,
                                                                                 const int *in_list)
{
    // [row][4 pivot columns]; the symmetric arm also uses it as the padded 16 x 16 transpose buffer
    constexpr bool SYM = MATINV_TILE_SYM_SWEEP && NT == 4 && FULL && LOOKAHEAD;
    __shared__ __attribute__((aligned(16))) double panel[SYM && 16 * NT * 4 < 16 * TILE_TSTRIDE ? 16 * TILE_TSTRIDE : 16 * NT * 4];
    gj_tile_body<double, NT, FULL, LOOKAHEAD, EARLY>(Ain, Xout, info, n_rt, batch, work_count, work_list, panel, in_count, in_list);
}

// The symmetric-only form (gj_tile_sym_body): an overload with one more, trailing, template argument, so that the kernels above keep
// their symbols and their code. Instantiated for <4, true, true, false, true> only. 168 VGPRs, no scratch, three waves per SIMD.
template <int NT, bool FULL, bool LOOKAHEAD, bool EARLY, bool SYMONLY>
__global__ __launch_bounds__(64, 3) void matinv_gj_tile_f64(BatchRef<const double> Ain, BatchRef<double> Xout, int *info, int n_rt,
                                                            unsigned batch, int *work_count, int *work_list, int *ns_count, int *ns_list)
{
    static_assert(NT == 4 && FULL && LOOKAHEAD && !EARLY && SYMONLY, "the symmetric-only form exists at 64 x 64 only");
    (void)n_rt;
    __shared__ __attribute__((aligned(16))) double panel[TILE_SYM_CLS_BATCH * 16 * TILE_TSTRIDE];
    static_assert(sizeof(panel) >= sizeof(double) * 16 * NT * 4 && 12 * sizeof(panel) <= 160 * 1024, "panel + transpose buffers, 12 workgroups per CU");
    gj_tile_sym_body(Ain, Xout, info, batch, work_count, work_list, ns_count, ns_list, panel);
}

// fp32 (the reference's DataType): v_mfma_f32_16x16x4_f32, 4 VGPRs per tile (64 at n = 64), same algorithm; the pivot
// blocks follow the f32 accumulator layout (TileGeo<float>).
template <int NT, bool FULL, bool LOOKAHEAD, bool EARLY = false>
__global__ __launch_bounds__(64, FULL ? 4 : 3) void matinv_gj_tile_f32(BatchRef<const float> Ain, BatchRef<float> Xout, int *info,
                                                           int n_rt, unsigned batch, int *work_count, int *work_list, const int *in_count,
                                                           const int *in_list)
{
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    gj_tile_body<float, NT, FULL, LOOKAHEAD, EARLY>(Ain, Xout, info, n_rt, batch, work_count, work_list, panel, in_count, in_list);
}

// ================================================================================================================
// SPD inputs: symmetric blocked sweep on LOWER-TRIANGULAR tile storage (the square-root-free member of the Cholesky
// family: the same Schur complements as A = L L^T, pivots = squares of the Cholesky diagonal, no pivot search needed
// and none wanted). Serves MATINV_ALGO_CHOLESKY for n <= 64 in place of the reference's four Cholesky kernel families
// (/root/reference/src/inverse_cholesky_gpu.cu:55-765); the literal L L^T / L^-1 / L^-T L^-1 phases stay available in
// the LDS family (and behind the reference's sub-phase entry points).
//
// Sweeping the pivot block K (D = W[K,K], P = W[:,K], Q = P D^-1) maps the symmetric W to the symmetric
//     W[I,J] <- W[I,J] - Q[I] P[J]^T,    W[I,K] <- Q[I],    W[K,J] <- Q[J]^T,    W[K,K] <- -D^-1       (I, J not in K)
// and after all blocks W = -A^-1. Only tiles (ti >= tj) are kept: NT(NT+1)/2 tiles = 80 VGPRs at n = 64 instead of 128
// (3 waves per SIMD instead of 2), 10 MFMAs per block step instead of 16, and only the lower triangle is read from HBM.
// Per tile it is the same single MFMA as the Gauss-Jordan kernel: A operand = -Q (rows K: +D^-1, C zeroed), B operand
// = P^T -- by symmetry the OLD panel itself, read back from LDS in the layout it was staged in -- with -I_4 on the K
// columns. Panel rows above the pivot block are not stored as a column: they are the pivot ROWS of tile row tK
// (W[I,K] = W[K,I]^T), which already sit in A-operand lane order.
// The upper triangle of the result is produced at the end by transposing each off-diagonal tile through LDS.
// Rejected (some pivot <= 0: not SPD, or NaN): work list -> LDS Cholesky kernel, which also reports info exactly.
// GP (r03) = the fused Gaussian-process scalars on this sweep, for the sizes where the bordered form of gp_tile_impl.hpp no
// longer fits one wavefront's registers (f64 80 < n <= 96: 7 x 7 bordered lower tiles = 224 VGPRs spill; 6 x 6 = 168 do not):
// M = B + diag c is inverted in registers exactly as for the Cholesky entry point (the diagonal added while loading), nothing
// is stored, and a^T M^-1 d is folded straight out of the lower accumulator tiles (an off-diagonal tile counts for its mirror
// too); the two vectors are staged once per item in the LDS panel, which is free by then. n^2 / 2 elements read, one scalar out.
template <class T>
struct SpdGp {
    const T *a, *c, *d, *e;  // d == nullptr: variance, out = e - a^T M^-1 a
    T *out;
};

template <class T, int NT, bool FULL, bool GP = false>
__device__ __forceinline__ void spd_tile_body(BatchRef<const T> Ain, BatchRef<T> Xout, int *info, int n_rt, unsigned batch,
                                              int *work_count, int *work_list, T *panel, SpdGp<T> gp = SpdGp<T>())
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    constexpr int N = 16 * NT;
    constexpr int NKB = 4 * NT;
    constexpr int TSTRIDE = TILE_TSTRIDE;  // padded row stride of the 16x16 transpose buffer
    const int l = threadIdx.x;

    for (unsigned mat = blockIdx.x; mat < batch; mat += gridDim.x) {
        const T *A = Ain.at_uniform(mat);
        T *X = Xout.at_uniform(mat);
        int n = FULL ? N : n_rt;  // run-time n opaque once per matrix, predicates on the edge tiles only: see gj_tile_body
        if (!FULL) asm volatile("" : "+s"(n));
        int q = l >> 4, c = l & 15;
        const unsigned lane_off = (unsigned)((l >> 4) * n + (l & 15));
        asm volatile("" : "+v"(q), "+v"(c));  // see matinv_gj_tile_f64

        // W = A^T tile layout as in the Gauss-Jordan kernel; lower tiles only. In the diagonal tiles the strictly
        // upper elements are fetched from their mirror position, so ONLY the lower triangle of A is ever read.
        vec4 acc[NT][NT];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) {
                if (tj > ti) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * ti + G::trow(r, q), col = 16 * tj + c;
                    T v;
                    if (ti == tj) {
                        const int hi = row > col ? row : col, lo = row > col ? col : row;
                        // memory element (r_mem, c_mem) of column-major A sits at c_mem*n + r_mem; W[row][col] =
                        // mem[row*n + col] = A[col][row]; its mirror mem[col*n + row]. Lower triangle of A
                        // (r_mem >= c_mem) <=> mem index (small*n + big).
                        v = (FULL || ti < NT - 1 || (row < n && col < n)) ? A[(unsigned)(lo * n + hi)] : ((row == col) ? (T)1 : (T)0);
                        if (GP && row == col && (FULL || ti < NT - 1 || row < n)) v += gp.c[(size_t)mat * n + row];  // addDiagonal, gauss_bench.cu:38-43
                    } else {
                        // ti > tj: row > col: W[row][col] = mem[row*n + col] = A[col][row] is in A's UPPER triangle;
                        // take its mirror A[row][col] = mem[col*n + row] instead
                        v = (FULL || ti < NT - 1 || (row < n && col < n)) ? A[(unsigned)(col * n + row)] : (T)0;  // tj < ti <= NT-1
                    }
                    acc[ti][tj][r] = v;
                }
            }
        (void)lane_off;
        unsigned long long bad = 0;
        T aop[NT], bop[NT];

        spd_panel_to_lds<NT, T>(panel, acc, 0, q, c);
        wave_lds_sync();
        {
            PanelSolve<NT, true, T> ps0;
#pragma unroll
            for (int s = 0; s < PanelSolve<NT, true, T>::NSTAGE; ++s) ps0.stage(s, panel, 0, q, c, aop, bop, bad);
        }
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const int tK = kb >> 2;
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
                // (b) the other lower tiles, pinned between the pieces of the next panel: 2 MFMAs cover the latency of
                //     (a), then the panel is staged, then the remaining MFMAs are spread evenly over the solve stages.
                //     Everything below is fully unrolled: the counters fold to literals.
                constexpr int NB = NT * (NT + 1) / 2 - NT;
                constexpr int NS = PanelSolve<NT, true, T>::NSTAGE;
                T aop_next[NT], bop_next[NT];
                PanelSolve<NT, true, T> ps;
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
            (void)tK;
        }

        if (GP && bad == 0) {
            // W = -M^-1 in the lower tiles (diagonal tiles complete). s = sum_ij a_i W_ij d_j: lane (q, c) holds W[row][col] with
            // row = 16 ti + trow(r, q), col = 16 tj + c; an off-diagonal tile also stands for its mirror W[col][row].
            const T *va = gp.a + (size_t)mat * n;
            const T *vd = gp.d ? gp.d + (size_t)mat * n : va;
            wave_lds_sync();  // the last panel has been consumed
            T *const sa = panel, *const sd = panel + N;  // [N] each; the panel buffer holds 4 N elements
#pragma unroll
            for (int k = 0; k < (N + 63) / 64; ++k) {
                const int i = l + 64 * k;
                if (i < N) {
                    sa[i] = (FULL || i < n) ? va[i] : (T)0;  // identity padding contributes nothing
                    sd[i] = (FULL || i < n) ? vd[i] : (T)0;
                }
            }
            wave_lds_sync();
            T s = 0;
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) {
                const T ac = sa[16 * tj + c], dc = sd[16 * tj + c];
#pragma unroll
                for (int ti = tj; ti < NT; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * ti + G::trow(r, q);
                        const T ar = sa[row], dr = sd[row];
                        const T wgt = (ti == tj) ? ar * dc : fma_t(ar, dc, dr * ac);
                        s = fma_t(acc[ti][tj][r], wgt, s);
                    }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
            if (l == 0) {
                gp.out[mat] = gp.d ? -s : gp.e[mat] + s;  // W = -M^-1
                if (info) info[mat] = 0;
            }
        } else if (bad == 0) {
            // W = -A^-1 (lower tiles). Lower tiles + diagonal tiles go out directly; the mirror of every off-diagonal
            // tile is transposed through LDS so that it, too, is written as 128-byte row segments.
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj < NT; ++tj) {
                    if (tj > ti) continue;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * ti + G::trow(r, q), col = 16 * tj + c;
                        if (FULL || ti < NT - 1 || (row < n && col < n)) X[(unsigned)(row * n + col)] = -acc[ti][tj][r];
                    }
                    if (tj < ti) {
                        wave_lds_sync();
#pragma unroll
                        for (int r = 0; r < 4; ++r) panel[G::trow(r, q) * TSTRIDE + c] = -acc[ti][tj][r];
                        wave_lds_sync();
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            // element (row 16tj + 4r + q, col 16ti + c) of the result = tile(ti,tj)[c][4r + q]
                            const int row = 16 * tj + G::trow(r, q), col = 16 * ti + c;
                            const T v = panel[c * TSTRIDE + G::trow(r, q)];
                            if (FULL || ti < NT - 1 || (row < n && col < n)) X[(unsigned)(row * n + col)] = v;
                        }
                    }
                }
            if (info && l == 0) info[mat] = 0;
        } else if (l == 0) {
            const int slot = atomicAdd(work_count, 1);
            work_list[slot] = (int)mat;
        }
        wave_lds_sync();
    }
}


template <int NT, bool FULL>
__global__ __launch_bounds__(64, NT >= 7 ? 1 : (NT >= 5 ? 2 : (NT >= 4 ? 3 : 4))) void matinv_spd_tile_f64(BatchRef<const double> Ain, BatchRef<double> Xout,
                                                                          int *info, int n_rt, unsigned batch,
                                                                          int *work_count, int *work_list)
{
    // the LDS buffer serves both as the [row][4] panel and as the padded 16x16 transpose buffer
    __shared__ __attribute__((aligned(16))) double panel[(16 * NT * 4 > 16 * 17) ? 16 * NT * 4 : 16 * 17];
    spd_tile_body<double, NT, FULL>(Ain, Xout, info, n_rt, batch, work_count, work_list, panel);
}

template <int NT, bool FULL>
// 9 x 9 / 10 x 10 tiles (r03): 180 / 220 accumulator registers, more than two waves per SIMD can hold (built for two: 736 / 1104 B
// of scratch per lane; 1.16e7 / 1.04e7 / 4.4e6 inv/s at 130^2 / 144^2 / 160^2 -- still 2.4x / 1.15x the one-wavefront-per-tile-column
// kernel). Built for ONE wave per SIMD (MATINV_SPD_WIDE_OCC=1, set by the Makefile for the two wide translation units) hipcc keeps
// every accumulator in AGPRs without a spill -- and with its default AGPR-FORM MFMAs (v_mfma a[..], v, v, a[..]) that build computes
// garbage from the second block step on: every matrix rejected, the LDS fallback did all the work at 7e5 inv/s. Same bits with s_nop
// padding around every MFMA group and with -amdgpu-mfma-padding-ratio=100, so not a wait-state hazard; partially overlapping dst / C
// register tuples, which that build is full of, are fine in isolation (tools/mfma_overlap_check.hip). With -mllvm
// -amdgpu-mfma-vgpr-form=1 (MFMAs on VGPRs, the AGPRs as parking space: 256 + 132 / 256 registers, no scratch) the same source is
// correct: 1.26e7 / 1.20e7 / 9.3e6 inv/s. The fp64 7 x 7 kernel in AGPR form is unaffected (its 256-bit MFMA results never overlap
// their C operand). 11 x 11 tiles (264 registers): the 44 block steps exceed the unroll threshold of the build (the loop stays, 2 KB of
// scratch per lane); with -pragma-unroll-threshold=8000000 hipcc had not finished that one kernel after 15 minutes.
#ifndef MATINV_SPD_WIDE_OCC
#define MATINV_SPD_WIDE_OCC 2
#endif
__global__ __launch_bounds__(64, NT >= 9 ? MATINV_SPD_WIDE_OCC : (NT >= 7 ? 2 : (NT >= 5 ? 3 : 4))) void matinv_spd_tile_f32(BatchRef<const float> Ain, BatchRef<float> Xout, int *info,
                                                            int n_rt, unsigned batch, int *work_count, int *work_list)
{
    __shared__ __attribute__((aligned(16))) float panel[(16 * NT * 4 > 16 * 17) ? 16 * NT * 4 : 16 * 17];
    spd_tile_body<float, NT, FULL>(Ain, Xout, info, n_rt, batch, work_count, work_list, panel);
}

// fused mean / variance on the SPD sweep (run-time n only): f64 6 x 6 tiles (80 < n <= 96), f32 7 x 7 (96 < n <= 112)
template <int NT>
__global__ __launch_bounds__(64, NT >= 7 ? 1 : 2) void matinv_gp_spd_tile_f64(const double *As, const double *Bs, const double *Cs, const double *Ds,
                                                               const double *Es, double *out, int *info, int n_rt, unsigned batch,
                                                               int *work_count, int *work_list)
{
    __shared__ __attribute__((aligned(16))) double panel[(16 * NT * 4 > 16 * 17) ? 16 * NT * 4 : 16 * 17];
    BatchRef<const double> A{Bs, (size_t)n_rt * n_rt, nullptr};
    BatchRef<double> X{nullptr, 0, nullptr};
    spd_tile_body<double, NT, false, true>(A, X, info, n_rt, batch, work_count, work_list, panel, SpdGp<double>{As, Cs, Ds, Es, out});
}
template <int NT>
__global__ __launch_bounds__(64, NT >= 9 ? MATINV_SPD_WIDE_OCC : 2) void matinv_gp_spd_tile_f32(const float *As, const float *Bs, const float *Cs, const float *Ds,
                                                               const float *Es, float *out, int *info, int n_rt, unsigned batch,
                                                               int *work_count, int *work_list)
{
    __shared__ __attribute__((aligned(16))) float panel[(16 * NT * 4 > 16 * 17) ? 16 * NT * 4 : 16 * 17];
    BatchRef<const float> A{Bs, (size_t)n_rt * n_rt, nullptr};
    BatchRef<float> X{nullptr, 0, nullptr};
    spd_tile_body<float, NT, false, true>(A, X, info, n_rt, batch, work_count, work_list, panel, SpdGp<float>{As, Cs, Ds, Es, out});
}

// ---- launchers shared by the fp64 and fp32 translation units (explicitly instantiated there) -----------------------------------

// The natural-order pass of the Gauss-Jordan entry point for n <= 64 (default policy): [screen +] verified natural-order kernel, then
// the pivoting kernel over the matrices they rejected, all in `stream`. ws: [0] rejected, [1] singular, [2] accepted (screened launches),
// [4 .. 4+batch) rejected matrices, then the singular ones among them, then the accepted ones.
//
// 64 x 64 fp64, unscreened (MATINV_TILE_SYM_FRONT): the FRONT route runs the symmetric-only form over the batch and then the two-arm
// kernel over the matrices that form found not symmetric (ws[3] counts them, their list takes the place of the accepted one: a
// screened launch never takes the front route), on one round of resident workgroups -- an empty list costs one small launch. The
// DIRECT route is the two-arm kernel over the batch. Which of them runs is decided by launch history alone
// (tile_policy_use_sym_front); a matrix gets the same bits either way, since its arm is the same code in both kernels.
bool tile_policy_use_screen(bool f64, int nt);
bool tile_policy_use_sym_front(int nt);
hint_t *tile_policy_record_sym_front(int nt);
template <class T>
hipError_t launch_gj_tile_natural(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream)
{
    constexpr bool F64 = sizeof(T) == 8;
    const TileShape s = tile_shape(n);
    const bool rowlane2 = rowlane2_supports(n);
    const bool screen = !rowlane2 && tile_policy_use_screen(F64, s.nt);
    const bool front = MATINV_TILE_SYM_FRONT && MATINV_TILE_SYM_SWEEP && F64 && n == 64 && !screen && tile_policy_use_sym_front(s.nt);
    return with_scratch_ints((screen || front ? 3 : 2) * batch + 4, 4, stream, [&](int *ws) {
        int *const rej_count = ws, *const sing_count = ws + 1, *const acc_count = ws + 2, *const ns_count = ws + 3;
        int *const rej_list = ws + 4, *const sing_list = ws + 4 + batch, *const acc_list = ws + 4 + 2 * batch, *const ns_list = acc_list;
        hipError_t e;
        if constexpr (F64) {
            if (front) {
                const unsigned b = (unsigned)batch;
                hipLaunchKernelGGL((matinv_gj_tile_f64<4, true, true, false, true>), dim3(tile_grid(batch, 12u)), dim3(64), 0, stream, A, X, info,
                                   n, b, rej_count, rej_list, ns_count, ns_list);
                hipLaunchKernelGGL((matinv_gj_tile_f64<4, true, true>), dim3(tile_grid(batch, 8u, 1u)), dim3(64), 0, stream, A, X, info, n, b,
                                   rej_count, rej_list, ns_count, ns_list);
                e = hipGetLastError();
                if (e == hipSuccess)
                    e = launch_gj_tilep_worklist<T>(n, A, X, batch, rej_count, rej_list, sing_count, sing_list, info, stream,
                                                    tile_policy_record(F64, s.nt, batch), false, ns_count, tile_policy_record_sym_front(s.nt));
                return e;
            }
        }
        if (rowlane2) {
            e = enqueue_gj_rowlane2<T>(n, A, X, batch, info, stream, rej_count, rej_list);
        } else {
            // grid-stride over the batch: enough waves to fill 256 CUs several times over, few enough to amortise setup
            const unsigned grid = tile_grid(batch, F64 ? 8u : 16u), b = (unsigned)batch;
            const unsigned sgrid = tile_grid(batch, 16u, 1u);  // screening: every resident wave takes many matrices
            with_tile<1, 4>(s, [&](auto NT, auto FULL) {
                // behind the screening pass the natural-order kernel takes its early-exit instantiation (NT >= 3; see gj_tile_body)
                constexpr bool EARLY = NT >= 3;
                if constexpr (F64) {
                    if (!screen) {
                        hipLaunchKernelGGL((matinv_gj_tile_f64<NT, FULL, true>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, rej_count,
                                           rej_list, nullptr, nullptr);
                        return;
                    }
                    hipLaunchKernelGGL((matinv_gj_tile_screen_f64<NT, FULL>), dim3(sgrid), dim3(64), 0, stream, A, n, b, rej_count, rej_list,
                                       acc_count, acc_list);
                    hipLaunchKernelGGL((matinv_gj_tile_f64<NT, FULL, true, EARLY>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, rej_count,
                                       rej_list, acc_count, acc_list);
                } else {
                    if (!screen) {
                        hipLaunchKernelGGL((matinv_gj_tile_f32<NT, FULL, true>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, rej_count,
                                           rej_list, nullptr, nullptr);
                        return;
                    }
                    hipLaunchKernelGGL((matinv_gj_tile_screen_f32<NT, FULL>), dim3(sgrid), dim3(64), 0, stream, A, n, b, rej_count, rej_list,
                                       acc_count, acc_list);
                    hipLaunchKernelGGL((matinv_gj_tile_f32<NT, FULL, true, EARLY>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, rej_count,
                                       rej_list, acc_count, acc_list);
                }
            });
            e = hipGetLastError();
        }
        if (e == hipSuccess)
            e = launch_gj_tilep_worklist<T>(n, A, X, batch, rej_count, rej_list, sing_count, sing_list, info, stream,
                                            tile_policy_record(F64, s.nt, batch), screen);
        return e;
    });
}

template <class T>
hipError_t launch_gj_tile(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream)
{
    if (!tile_family_supports<T>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // (r03, measured and not kept: the natural-order sweep of 5 x 5 / 6 x 6 tiles on ONE wavefront with the accumulators in AGPRs,
    // one wave per SIMD -- 2.6e7 / 2.5e7 inv/s at 72^2 / 80^2, the same as two wavefronts per matrix, and 1.7e7 against 2.0e7 at
    // 96^2, 1.2e7 against 2.1e7 at 88^2 (ragged: 720 B of scratch). All n^2 tiles instead of the lower triangle: with one wave
    // per SIMD nothing hides the panel solve between the MFMAs. The symmetric sweep, half the tiles, does gain: launch_spd_tile.)
    if (n > 64) return launch_gj_tile4<T>(n, A, X, batch, info, stream);
    if (tile_policy_use_pivot(sizeof(T) == 8, tile_shape(n).nt)) return launch_gj_tilep<T>(n, A, X, batch, info, stream);
    return launch_gj_tile_natural<T>(n, A, X, batch, info, stream);
}

// The instantiation of the one-wavefront symmetric sweep that serves n: FULL except for the fp32 kernels of 8 x 8 tiles and more, which
// take run-time n only (the compile-time-n one measured 2.3e6 inv/s against 2.1e7 at 128^2)
constexpr TileShape spd_tile_shape(bool f64, int n) { return {(n + 15) / 16, n % 16 == 0 && (f64 || n < 128)}; }

// fused pipeline on the SPD sweep: f64 80 < n <= 96 (6 x 6 tiles), f32 96 < n <= 112 (7 x 7); rejects (not SPD) -> LDS pipeline
hipError_t enqueue_spd_tile_big_f32(int n, BatchRef<const float> A, BatchRef<float> X, unsigned grid, unsigned b, int *info, int *ws,
                                    hipStream_t stream);
template <class T>
hipError_t launch_gp_spd_tile(int n, const T *As, const T *Bs, const T *Cs, const T *Ds, const T *Es, T *out, size_t batch, int *info,
                              hipStream_t stream)
{
    if (!gp_spd_tile_supports(sizeof(T) == 8, n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    return with_scratch_ints(batch + 1, 1, stream, [&](int *ws) {
        const unsigned grid = tile_grid(batch, 8u), b = (unsigned)batch;
        hipError_t e = hipSuccess;
        if constexpr (sizeof(T) == 8) {
            if (n <= 96) hipLaunchKernelGGL((matinv_gp_spd_tile_f64<6>), dim3(grid), dim3(64), 0, stream, As, Bs, Cs, Ds, Es, out, info, n, b, ws, ws + 1);
            else e = enqueue_gp_spd_tile_wide_f64(n, As, Bs, Cs, Ds, Es, out, grid, b, info, ws, stream);
        } else {
            if (n <= 112) hipLaunchKernelGGL((matinv_gp_spd_tile_f32<7>), dim3(grid), dim3(64), 0, stream, As, Bs, Cs, Ds, Es, out, info, n, b, ws, ws + 1);
            else if (n <= 128) hipLaunchKernelGGL((matinv_gp_spd_tile_f32<8>), dim3(grid), dim3(64), 0, stream, As, Bs, Cs, Ds, Es, out, info, n, b, ws, ws + 1);
            else e = enqueue_gp_spd_tile_wide_f32(n, As, Bs, Cs, Ds, Es, out, grid, b, info, ws, stream);
        }
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = launch_gp_lds_worklist<T>(n, As, Bs, Cs, Ds, Es, out, ws, ws + 1, info, stream);
        return e;
    });
}

}  // namespace matinv
