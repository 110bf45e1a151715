// tile_kernels.inc (compiled in parts selected with MATINV_TILE_PART so that they build in parallel: tile_kernels.hip = the fp64 SPD / fused-pipeline
// kernels + the family's non-template helpers, tile_f32_kernels.hip = their fp32 half, tile_gj_kernels.hip / tile_gj_f32_kernels.hip = the natural-order
// Gauss-Jordan kernels, spd_wide_* / gp_spd_wide_* = the widest one-wavefront symmetric sweeps) -- kernel family "TILE": one matrix per wavefront, register-resident in 16x16 fp64 MFMA
// accumulator tiles (v_mfma_f64_16x16x4_f64), for 16 < n <= 64 (n is padded to NT*16 with an identity block).
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
// Replaces the 3n launches of /root/reference/src/gauss/batched_invert.cu:84-95.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>

#include "tile_common.hpp"
#include "tile_screen.hpp"

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

// One matrix per wavefront; see the file header. T = double or float.
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

        // -DMATINV_TILE_LDST_ONLY (tools/build_ldst_variant.sh, profiling only): no elimination at all -- the kernel's loads and
        // stores in their real access pattern and launch shape, to price what the memory side alone costs
#ifdef MATINV_TILE_LDST_ONLY
        if (false) {
#else
        if (LOOKAHEAD) {
#endif
            panel_to_lds<NT, T>(panel, acc, 0, q, c);
            wave_lds_sync();
            panel_solve<NT>(panel, 0, q, c, aop, bad);
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
                    PanelSolve<NT, false, T> ps;
                    constexpr int NS = PanelSolve<NT, false, T>::NSTAGE;
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

        if (bad == 0) {
            if (PAIRED) {
                const unsigned lane_off2 = (unsigned)(2 * G::trow(0, l >> 4) * N + 2 * (l & 15));
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int u = 0; u < NT / 2; ++u)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const unsigned uoff = (unsigned)((32 * (ti >> 1) + 2 * G::trow(r, 0) + (ti & 1)) * N + 32 * u);
                            vec2 v;
                            v[0] = acc[ti][2 * u][r];
                            v[1] = acc[ti][2 * u + 1][r];
                            __builtin_nontemporal_store(v, reinterpret_cast<vec2 *>(X + uoff + lane_off2));
                        }
            } else {
#pragma unroll
                for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                    for (int tj = 0; tj < NT; ++tj)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * ti + G::trow(r, q), col = 16 * tj + c;
                            const unsigned uoff = (unsigned)((16 * ti + G::trow(r, 0)) * n + 16 * tj);
                            const bool edge = !FULL && (ti == NT - 1 || tj == NT - 1);
                            if (!edge || (row < n && col < n)) X[uoff + lane_off] = acc[ti][tj][r];
                        }
            }
            if (info && l == 0) info[mat] = 0;
        } else if (l == 0) {
            const int slot = atomicAdd(work_count, 1);
            work_list[slot] = (int)mat;
        }
        if (LOOKAHEAD) wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}


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
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];  // [row][4 pivot columns]
    gj_tile_body<double, NT, FULL, LOOKAHEAD, EARLY>(Ain, Xout, info, n_rt, batch, work_count, work_list, panel, in_count, in_list);
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

// The natural-order pass of the Gauss-Jordan entry point for n <= 64 (default policy): [screen +] verified natural-order kernel, then
// the pivoting kernel over the matrices they rejected, all in `stream`. ws: [0] rejected, [1] singular, [2] accepted (screened launches),
// [4 .. 4+batch) rejected matrices, then the singular ones among them, then the accepted ones.
bool tile_policy_use_screen(bool f64, int nt);
template <class T>
static hipError_t launch_gj_tile_natural(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream)
{
    constexpr bool F64 = sizeof(T) == 8;
    const int nt = (n + 15) / 16;
    const bool rowlane2 = rowlane2_natural_use(F64, n);
    const bool screen = !rowlane2 && tile_policy_use_screen(F64, nt);
    int *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), ((screen ? 3 : 2) * batch + 4) * sizeof(int), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(ws, 0, 4 * sizeof(int), stream);
    if (e != hipSuccess) {
        (void)scratch_free(ws, stream);
        return e;
    }
    int *const rej_count = ws, *const sing_count = ws + 1, *const acc_count = ws + 2;
    int *const rej_list = ws + 4, *const sing_list = ws + 4 + batch, *const acc_list = ws + 4 + 2 * batch;
    // grid-stride over the batch: enough waves to fill 256 CUs several times over, few enough to amortise setup
    const unsigned per_cu = F64 ? 8u : 16u;
    const unsigned grid = (unsigned)(batch < 256u * per_cu * tile_grid_rounds() ? batch : 256u * per_cu * tile_grid_rounds());
    const unsigned b = (unsigned)batch;
    const int *in_count = screen ? acc_count : nullptr, *in_list = screen ? acc_list : nullptr;
    const unsigned sgrid = (unsigned)(batch < 256u * 16u ? batch : 256u * 16u);  // screening: every resident wave takes many matrices
#define TILE_LAUNCH2(NT_, EARLY_)                                                                                     \
    do {                                                                                                              \
        if constexpr (F64) {                                                                                          \
            if (screen && n == 16 * NT_)                                                                              \
                hipLaunchKernelGGL((matinv_gj_tile_screen_f64<NT_, true>), dim3(sgrid), dim3(64), 0, stream, A, n, b, rej_count, rej_list, acc_count, acc_list); \
            else if (screen)                                                                                          \
                hipLaunchKernelGGL((matinv_gj_tile_screen_f64<NT_, false>), dim3(sgrid), dim3(64), 0, stream, A, n, b, rej_count, rej_list, acc_count, acc_list); \
            if (n == 16 * NT_)                                                                                        \
                hipLaunchKernelGGL((matinv_gj_tile_f64<NT_, true, true, (EARLY_) && NT_ >= 3>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, rej_count, rej_list, in_count, in_list); \
            else                                                                                                      \
                hipLaunchKernelGGL((matinv_gj_tile_f64<NT_, false, true, (EARLY_) && NT_ >= 3>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, rej_count, rej_list, in_count, in_list); \
        } else {                                                                                                      \
            if (screen && n == 16 * NT_)                                                                              \
                hipLaunchKernelGGL((matinv_gj_tile_screen_f32<NT_, true>), dim3(sgrid), dim3(64), 0, stream, A, n, b, rej_count, rej_list, acc_count, acc_list); \
            else if (screen)                                                                                          \
                hipLaunchKernelGGL((matinv_gj_tile_screen_f32<NT_, false>), dim3(sgrid), dim3(64), 0, stream, A, n, b, rej_count, rej_list, acc_count, acc_list); \
            if (n == 16 * NT_)                                                                                        \
                hipLaunchKernelGGL((matinv_gj_tile_f32<NT_, true, true, (EARLY_) && NT_ >= 3>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, rej_count, rej_list, in_count, in_list); \
            else                                                                                                      \
                hipLaunchKernelGGL((matinv_gj_tile_f32<NT_, false, true, (EARLY_) && NT_ >= 3>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, rej_count, rej_list, in_count, in_list); \
        }                                                                                                             \
    } while (0)
    // behind the screening pass the natural-order kernel takes its early-exit instantiation (NT >= 3; see gj_tile_body)
#define TILE_LAUNCH(NT_)                                                                                              \
    do {                                                                                                              \
        if (screen) TILE_LAUNCH2(NT_, true);                                                                          \
        else TILE_LAUNCH2(NT_, false);                                                                                \
    } while (0)
    if (rowlane2) {
        e = enqueue_gj_rowlane2<T>(n, A, X, batch, info, stream, rej_count, rej_list);
    } else {
        switch (nt) {
        case 1: TILE_LAUNCH(1); break;
        case 2: TILE_LAUNCH(2); break;
        case 3: TILE_LAUNCH(3); break;
        default: TILE_LAUNCH(4); break;
        }
        e = hipGetLastError();
    }
#undef TILE_LAUNCH
#undef TILE_LAUNCH2
    if (e == hipSuccess)
        e = launch_gj_tilep_worklist<T>(n, A, X, batch, rej_count, rej_list, sing_count, sing_list, info, stream, tile_policy_record(F64, nt, batch), screen);
    hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
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
    constexpr int TSTRIDE = 17;  // padded row stride of the 16x16 transpose buffer (conflict-free reads)
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

// ------------------------------------------------------------------------------------------------
template <class T>
bool tile_family_supports(int n);
template <class T>
hipError_t launch_gj_tile(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
template <class T>
bool spd_tile_supports(int n);
template <class T>
hipError_t launch_spd_tile(int n, BatchRef<const T> A, BatchRef<T> X, size_t batch, int *info, hipStream_t stream);
// explicit specialisations, defined in the part named in the comment
template <>
bool tile_family_supports<double>(int n);  // 64
template <>
bool tile_family_supports<float>(int n);   // 64
template <>
bool spd_tile_supports<double>(int n);     // 64
template <>
bool spd_tile_supports<float>(int n);      // 64

#if MATINV_TILE_PART == 64
// r03: ONE wavefront per matrix beyond what 256 registers hold. A gfx950 wave may own up to 512 registers -- 256 VGPRs + 256
// AGPRs, one file, and MFMA accumulates in AGPRs directly -- when its kernel asks for one wave per SIMD: hipcc then keeps the
// accumulator tiles in AGPRs (fp64 7 x 7 lower tiles: 190 VGPRs + 224 AGPRs, no scratch). Four matrices per CU, no workgroup barrier,
// no panel solve repeated per wave; r01/r02 stopped the one-wave kernels at 256 registers (two waves per SIMD) and went to several
// wavefronts per matrix from there.

// Measured at 100 k x 64^2 f64: 1 / 4 / 16 / 64 rounds -> 1.631 / 1.600 / 1.579 / 1.570 ms per launch: the hardware
// dispatcher balances better than a static stride does, so the grids are (nearly) one workgroup per matrix and the stride
// loop only matters for batches beyond 64 rounds.
unsigned tile_grid_rounds()
{
    static const unsigned rounds = []() {
        const char *s = getenv("MATINV_TILE_GRID_MULT");
        const int v = s && *s ? atoi(s) : 64;
        return (unsigned)(v < 1 ? 1 : v);
    }();
    return rounds;
}

// ---- natural order or pivot search? -------------------------------------------------------------------------------------
// The verified-natural-order kernel is the fast path for diagonally dominant / SPD batches (0.50 of HBM at 64 x 64); a matrix
// that fails its acceptance test is redone by the pivoting kernel in the same stream. Three policies (matinv_set_gj_policy,
// MATINV_GJ_POLICY=natural|pivot|adaptive):
//   NATURAL_FIRST (default since r03): every launch runs the natural-order kernel, rejects go to the pivoting kernel. What a
//       matrix's result is depends on that matrix alone -- no launch history, no batch mates: the same call gives the same
//       bits again, and a sharded batch the bits of the single launch. A batch of GENERAL matrices pays both kernels.
//   PIVOT: every launch goes straight to the pivoting kernel (equally deterministic; what the reference's LU entry points,
//       inverse_lu_cuda_batched_*, take: partial pivoting is their contract, src/gauss/inverse_gpu.cu:16-58).
//   ADAPTIVE (r02 behaviour, opt-in): per (device, dtype, tile count) the launcher remembers how the LAST natural-order launch
//       that has completed went -- (rejected, batch) come back as ONE 8-byte store of the work-list kernel into pinned host
//       memory, never waited for -- and sends a batch straight to the pivoting kernel while at least a quarter of that launch
//       was rejected; every 32nd launch in that state probes the natural order again. Fastest for callers that alternate
//       rarely; a matrix that the natural-order kernel would accept although partial pivoting would move rows gets the
//       pivoting kernel's bits or the natural ones depending on what ran before.
// All of the state is per device and atomic: host threads driving different devices (or one device) do not race on it.
namespace {
constexpr int kMaxDevices = 16, kSlotsPerDevice = 64;
struct HintSlot {
    std::atomic<unsigned long long> pair;       // (batch << 32) | rejected of the last completed natural-order launch: device store
    std::atomic<unsigned> launches_in_pivot_mode;
};
HintSlot *hint_slots()
{
    static HintSlot *slots = []() -> HintSlot * {
        void *p = nullptr;
        if (hipHostMalloc(&p, sizeof(HintSlot) * kMaxDevices * kSlotsPerDevice, hipHostMallocPortable) != hipSuccess) return nullptr;
        memset(p, 0, sizeof(HintSlot) * kMaxDevices * kSlotsPerDevice);
        return static_cast<HintSlot *>(p);
    }();
    return slots;
}
std::atomic<int> g_policy{-1};  // -1: not read from the environment yet
std::atomic<unsigned long long> g_natural_launches{0}, g_pivot_launches{0};
std::atomic<int> g_last_slot{0};
int slot_index(bool f64, int nt)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) dev = 0;
    return (dev % kMaxDevices) * kSlotsPerDevice + (f64 ? 32 : 0) + (nt & 31);
}
}  // namespace

int gj_policy()
{
    int v = g_policy.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *s = getenv("MATINV_GJ_POLICY");
        v = MATINV_GJ_NATURAL_FIRST;
        if (s && !strcmp(s, "pivot")) v = MATINV_GJ_PIVOT;
        else if (s && !strcmp(s, "adaptive")) v = MATINV_GJ_ADAPTIVE;
        int expected = -1;
        if (!g_policy.compare_exchange_strong(expected, v)) v = expected;  // somebody set it meanwhile
    }
    return v;
}

int set_gj_policy(int policy)
{
    const int old = gj_policy();
    g_policy.store(policy, std::memory_order_relaxed);
    return old;
}

bool tile_policy_use_pivot(bool f64, int nt)
{
    const int pol = gj_policy();
    bool pivot = pol == MATINV_GJ_PIVOT;
    if (pol == MATINV_GJ_ADAPTIVE) {
        HintSlot *h = hint_slots();
        const int idx = slot_index(f64, nt);
        g_last_slot.store(idx, std::memory_order_relaxed);
        if (h) {
            const unsigned long long pr = h[idx].pair.load(std::memory_order_relaxed);
            const unsigned long long batch = pr >> 32, rejected = pr & 0xffffffffull;
            if (batch > 0 && 4ull * rejected >= batch)
                pivot = ((h[idx].launches_in_pivot_mode.fetch_add(1, std::memory_order_relaxed) + 1) % 32u) != 0;  // every 32nd probes
        }
    }
    (pivot ? g_pivot_launches : g_natural_launches).fetch_add(1, std::memory_order_relaxed);
    return pivot;
}

// before a natural-order launch: where the work-list kernel that follows it in the stream stores (batch << 32) | rejected
// (pinned host memory, one 8-byte store, never waited for), or nullptr when nobody reads it
hint_t *tile_policy_record(bool f64, int nt, size_t batch)
{
    (void)batch;
    if (gj_policy() == MATINV_GJ_PIVOT) return nullptr;
    HintSlot *h = hint_slots();
    if (!h) return nullptr;
    static_assert(sizeof(std::atomic<unsigned long long>) == sizeof(hint_t), "the device stores into the atomic's storage");
    return reinterpret_cast<hint_t *>(&h[slot_index(f64, nt)].pair);
}

// NATURAL_FIRST: run the screening kernel (gj_tile_screen_body) in front of the natural-order kernel? Yes while the last completed
// natural-order launch of this class rejected at least a quarter of its batch. It changes what a launch costs, never what it
// computes. MATINV_TILE_SCREEN=0 / 1: never / always (tests, A/B).
bool tile_policy_use_screen(bool f64, int nt)
{
    static const int forced = []() {
        const char *s = getenv("MATINV_TILE_SCREEN");
        return !s || !*s ? -1 : (*s == '0' ? 0 : 1);
    }();
    if (forced >= 0) return forced == 1;
    if (gj_policy() != MATINV_GJ_NATURAL_FIRST) return false;
    HintSlot *h = hint_slots();
    if (!h) return false;
    const unsigned long long pr = h[slot_index(f64, nt)].pair.load(std::memory_order_relaxed);
    const unsigned long long batch = pr >> 32, rejected = pr & 0xffffffffull;
    return batch > 0 && 4ull * rejected >= batch;
}

TileStats tile_stats()
{
    HintSlot *h = hint_slots();
    TileStats t{g_natural_launches.load(), g_pivot_launches.load(), 0, 0};
    if (h) {
        const unsigned long long pr = h[g_last_slot.load()].pair.load(std::memory_order_relaxed);
        t.last_rejected = pr & 0xffffffffull;
        t.last_batch = pr >> 32;
    }
    return t;
}

template <>
bool tile_family_supports<double>(int n) { return n >= 1 && n <= 192; }  // 64 < n: tile4_kernels.hip (up to 12 x 12 tiles)
template <>
bool tile_family_supports<float>(int n) { return n >= 1 && n <= 256; }


template <>
bool spd_tile_supports<double>(int n) { return n >= 1 && n <= 192; }  // 64 < n: tile4_kernels.hip (up to 12 x 12 tiles)
template <>
bool spd_tile_supports<float>(int n) { return n >= 1 && n <= 256; }

#endif

// fused pipeline on the SPD sweep: f64 80 < n <= 96 (6 x 6 tiles), f32 96 < n <= 112 (7 x 7); rejects (not SPD) -> LDS pipeline
#if MATINV_TILE_PART == 64
// largest n the ONE-wavefront symmetric sweep takes: fp64 7 x 7 lower tiles (224 accumulator registers, VGPRs + AGPRs, one wave
// per SIMD); fp32 10 x 10 (55 tiles = 220 registers, one wave per SIMD; 11 x 11 = 264: 2 KB of scratch per lane)
int spd_onewave_max(bool f64) { return f64 ? 112 : 160; }
bool gp_spd_tile_supports(bool f64, int n) { return n > (f64 ? 80 : 96) && n <= spd_onewave_max(f64); }
#endif

template <class T>
static hipError_t launch_gp_spd_tile_impl(int n, const T *As, const T *Bs, const T *Cs, const T *Ds, const T *Es, T *out, size_t batch,
                                          int *info, hipStream_t stream)
{
    if (!gp_spd_tile_supports(sizeof(T) == 8, n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    int *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), (batch + 1) * sizeof(int), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(ws, 0, sizeof(int), stream);
    if (e != hipSuccess) {
        (void)scratch_free(ws, stream);
        return e;
    }
    const unsigned grid = (unsigned)(batch < 256u * 8u * tile_grid_rounds() ? batch : 256u * 8u * tile_grid_rounds());
    const unsigned b = (unsigned)batch;
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
    hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

// fp32, 7 x 7 and 8 x 8 lower tiles on one wavefront (Cholesky entry point; the fused pipeline of those sizes): tile_big_f32_kernels.hip
hipError_t enqueue_spd_tile_big_f32(int n, BatchRef<const float> A, BatchRef<float> X, unsigned grid, unsigned b, int *info, int *ws,
                                    hipStream_t stream);
#if MATINV_TILE_PART == 35
template <>
hipError_t launch_gp_spd_tile<float>(int n, const float *As, const float *Bs, const float *Cs, const float *Ds, const float *Es, float *out,
                                     size_t batch, int *info, hipStream_t stream)
{
    return launch_gp_spd_tile_impl<float>(n, As, Bs, Cs, Ds, Es, out, batch, info, stream);
}

hipError_t enqueue_spd_tile_big_f32(int n, BatchRef<const float> A, BatchRef<float> X, unsigned grid, unsigned b, int *info, int *ws,
                                    hipStream_t stream)
{
    if (n == 112) hipLaunchKernelGGL((matinv_spd_tile_f32<7, true>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1);
    else if (n <= 112) hipLaunchKernelGGL((matinv_spd_tile_f32<7, false>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1);
    // 8 x 8: the run-time-n instantiation also for n = 128 (the compile-time-n one measured 2.3e6 inv/s against 2.1e7)
    else hipLaunchKernelGGL((matinv_spd_tile_f32<8, false>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1);
    return hipGetLastError();
}
#endif
#if MATINV_TILE_PART == 36  // tile_gj_f32_kernels.hip: the natural-order Gauss-Jordan kernels by themselves (build time)
template <>
hipError_t launch_gj_tile<float>(int n, BatchRef<const float> A, BatchRef<float> X, size_t batch, int *info,
                                 hipStream_t stream)
{
    if (!tile_family_supports<float>(n)) return hipErrorInvalidValue;
    if (n > 64) return launch_gj_tile4<float>(n, A, X, batch, info, stream);
    if (batch == 0) return hipSuccess;
    if (tile_policy_use_pivot(false, (n + 15) / 16)) return launch_gj_tilep<float>(n, A, X, batch, info, stream);
    return launch_gj_tile_natural<float>(n, A, X, batch, info, stream);
}
#endif
#if MATINV_TILE_PART == 32

template <>
hipError_t launch_spd_tile<float>(int n, BatchRef<const float> A, BatchRef<float> X, size_t batch, int *info,
                                  hipStream_t stream)
{
    if (!spd_tile_supports<float>(n)) return hipErrorInvalidValue;
    // one wavefront holds the lower triangle up to 7 x 7 tiles at two waves per SIMD, 8 x 8 (144 accumulator registers) since r03,
    // and 9 x 9 / 10 x 10 (180 / 220) at one wave per SIMD with VGPR-form MFMAs and AGPR parking space (spd_wide_f32_kernels.hip)
    if (n > spd_onewave_max(false)) return launch_spd_tile4<float>(n, A, X, batch, info, stream);
    if (batch == 0) return hipSuccess;
    int *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), (batch + 1) * sizeof(int), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(ws, 0, sizeof(int), stream);
    if (e != hipSuccess) {
        (void)scratch_free(ws, stream);
        return e;
    }
    const int nt = (n + 15) / 16;
    const unsigned grid = (unsigned)(batch < 256u * 16u * tile_grid_rounds() ? batch : 256u * 16u * tile_grid_rounds());
    const unsigned b = (unsigned)batch;
#define SPD_LAUNCH_F32(NT_)                                                                                           \
    if (n == 16 * NT_)                                                                                                \
        hipLaunchKernelGGL((matinv_spd_tile_f32<NT_, true>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1); \
    else                                                                                                              \
        hipLaunchKernelGGL((matinv_spd_tile_f32<NT_, false>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1)
    switch (nt) {
    case 1: SPD_LAUNCH_F32(1); break;
    case 2: SPD_LAUNCH_F32(2); break;
    case 3: SPD_LAUNCH_F32(3); break;
    case 4: SPD_LAUNCH_F32(4); break;
    case 5: SPD_LAUNCH_F32(5); break;
    case 6: SPD_LAUNCH_F32(6); break;
    case 7:
    case 8: e = enqueue_spd_tile_big_f32(n, A, X, grid, b, info, ws, stream); break;
    default: e = enqueue_spd_tile_wide_f32(n, A, X, grid, b, info, ws, stream); break;
    }
#undef SPD_LAUNCH_F32
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = launch_chol_lds_worklist<float>(n, A, X, ws, ws + 1, info, stream);
    hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

#endif

#if MATINV_TILE_PART == 33
// fp32 symmetric sweep of 9 x 9 / 10 x 10 lower tiles on ONE wavefront (128 < n <= 160), run-time n only; translation units of
// their own (spd_wide_f32_kernels.hip, gp_spd_wide_f32_kernels.hip): each fully unrolled instantiation takes over a minute to compile
hipError_t enqueue_spd_tile_wide_f32(int n, BatchRef<const float> A, BatchRef<float> X, unsigned grid, unsigned b, int *info, int *ws,
                                     hipStream_t stream)
{
    switch ((n + 15) / 16) {
    case 9: hipLaunchKernelGGL((matinv_spd_tile_f32<9, false>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1); break;
    case 10: hipLaunchKernelGGL((matinv_spd_tile_f32<10, false>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
#endif
#if MATINV_TILE_PART == 34
hipError_t enqueue_gp_spd_tile_wide_f32(int n, const float *As, const float *Bs, const float *Cs, const float *Ds, const float *Es, float *out,
                                        unsigned grid, unsigned b, int *info, int *ws, hipStream_t stream)
{
    switch ((n + 15) / 16) {
    case 9: hipLaunchKernelGGL((matinv_gp_spd_tile_f32<9>), dim3(grid), dim3(64), 0, stream, As, Bs, Cs, Ds, Es, out, info, n, b, ws, ws + 1); break;
    case 10: hipLaunchKernelGGL((matinv_gp_spd_tile_f32<10>), dim3(grid), dim3(64), 0, stream, As, Bs, Cs, Ds, Es, out, info, n, b, ws, ws + 1); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
#endif

#if MATINV_TILE_PART == 65
// fp64 symmetric sweep of 7 x 7 lower tiles on ONE wavefront (96 < n <= 112; 224 accumulator registers, one wave per SIMD): a translation
// unit of its own (spd_wide_f64_kernels.hip) so that it can be compiled with VGPR-form MFMAs and the AGPRs as parking space -- with
// hipcc's default AGPR-form MFMAs the same kernels are correct here (256-bit results never overlap their C operand) but slower:
// Cholesky 112^2 1.36e7 -> 1.59e7 inv/s, pipeline 1.42e7 -> 1.48e7 items/s
hipError_t enqueue_spd_tile_wide_f64(int n, BatchRef<const double> A, BatchRef<double> X, unsigned grid, unsigned b, int *info, int *ws,
                                     hipStream_t stream)
{
    if (n == 112) hipLaunchKernelGGL((matinv_spd_tile_f64<7, true>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1);
    else hipLaunchKernelGGL((matinv_spd_tile_f64<7, false>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1);
    return hipGetLastError();
}
hipError_t enqueue_gp_spd_tile_wide_f64(int n, const double *As, const double *Bs, const double *Cs, const double *Ds, const double *Es,
                                        double *out, unsigned grid, unsigned b, int *info, int *ws, hipStream_t stream)
{
    hipLaunchKernelGGL((matinv_gp_spd_tile_f64<7>), dim3(grid), dim3(64), 0, stream, As, Bs, Cs, Ds, Es, out, info, n, b, ws, ws + 1);
    return hipGetLastError();
}
#endif

#if MATINV_TILE_PART == 64
template <>
hipError_t launch_gp_spd_tile<double>(int n, const double *As, const double *Bs, const double *Cs, const double *Ds, const double *Es,
                                      double *out, size_t batch, int *info, hipStream_t stream)
{
    return launch_gp_spd_tile_impl<double>(n, As, Bs, Cs, Ds, Es, out, batch, info, stream);
}

#endif
#if MATINV_TILE_PART == 66  // tile_gj_kernels.hip
template <>
hipError_t launch_gj_tile<double>(int n, BatchRef<const double> A, BatchRef<double> X, size_t batch, int *info,
                                  hipStream_t stream)
{
    if (!tile_family_supports<double>(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    // (r03, measured and not kept: the natural-order sweep of 5 x 5 / 6 x 6 tiles on ONE wavefront with the accumulators in AGPRs,
    // one wave per SIMD -- 2.6e7 / 2.5e7 inv/s at 72^2 / 80^2, the same as two wavefronts per matrix, and 1.7e7 against 2.0e7 at
    // 96^2, 1.2e7 against 2.1e7 at 88^2 (ragged: 720 B of scratch). All n^2 tiles instead of the lower triangle: with one wave
    // per SIMD nothing hides the panel solve between the MFMAs. The symmetric sweep, half the tiles, does gain: launch_spd_tile.)
    if (n > 64) return launch_gj_tile4<double>(n, A, X, batch, info, stream);
    if (tile_policy_use_pivot(true, (n + 15) / 16)) return launch_gj_tilep<double>(n, A, X, batch, info, stream);
    return launch_gj_tile_natural<double>(n, A, X, batch, info, stream);
}
#endif
#if MATINV_TILE_PART == 64

template <>
hipError_t launch_spd_tile<double>(int n, BatchRef<const double> A, BatchRef<double> X, size_t batch, int *info,
                                   hipStream_t stream)
{
    if (!spd_tile_supports<double>(n)) return hipErrorInvalidValue;
    // one wavefront holds the lower triangle up to 6 x 6 tiles in 256 registers (two waves per SIMD) and 7 x 7 in VGPRs + AGPRs
    // (one wave per SIMD, r03; before that 7 x 7 spilled: 5.8e6 inv/s at 112 x 112 against 9.9e6 on four wavefronts)
    if (spd_tile2_supports(true, n)) return launch_spd_tile2(n, A, X, batch, info, stream);  // 112 < n <= 128: two waves, lower tiles
    if (n > 112) return launch_spd_tile4<double>(n, A, X, batch, info, stream);  // 176 < n <= 192: one wavefront per tile column
    if (batch == 0) return hipSuccess;
    int *ws = nullptr;
    hipError_t e = scratch_alloc(reinterpret_cast<void **>(&ws), (batch + 1) * sizeof(int), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(ws, 0, sizeof(int), stream);
    if (e != hipSuccess) {
        (void)scratch_free(ws, stream);
        return e;
    }
    const int nt = (n + 15) / 16;
    const unsigned grid = (unsigned)(batch < 256u * 12u * tile_grid_rounds() ? batch : 256u * 12u * tile_grid_rounds());
    const unsigned b = (unsigned)batch;
#define SPD_LAUNCH(NT_)                                                                                               \
    if (n == 16 * NT_)                                                                                                \
        hipLaunchKernelGGL((matinv_spd_tile_f64<NT_, true>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1); \
    else                                                                                                              \
        hipLaunchKernelGGL((matinv_spd_tile_f64<NT_, false>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1)
    switch (nt) {
    case 1: SPD_LAUNCH(1); break;
    case 2: SPD_LAUNCH(2); break;
    case 3: SPD_LAUNCH(3); break;
    case 4: SPD_LAUNCH(4); break;
    case 5: SPD_LAUNCH(5); break;
    case 6: SPD_LAUNCH(6); break;
    default: e = enqueue_spd_tile_wide_f64(n, A, X, grid, b, info, ws, stream); break;  // 7 x 7: spd_wide_f64_kernels.hip
    }
#undef SPD_LAUNCH
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = launch_chol_lds_worklist<double>(n, A, X, ws, ws + 1, info, stream);
    hipError_t e2 = scratch_free(ws, stream);
    return e != hipSuccess ? e : e2;
}

const char *name_spd_tile(bool f64, int n)
{
    if (spd_tile2_supports(f64, n)) return name_spd_tile2(false, n);
    if (n > spd_onewave_max(f64)) return name_tile4(f64, true, n);
    static thread_local char buf[48];
    snprintf(buf, sizeof buf, "matinv_spd_tile_%s<%d, %s>", f64 ? "f64" : "f32", (n + 15) / 16,
             ((n % 16) == 0 && !(n >= 128 && !f64)) ? "true" : "false");
    return buf;
}

const char *name_gj_tile(bool f64, int n)
{
    if (n > 64) return name_tile4(f64, false, n);
    if (rowlane2_natural_use(f64, n)) return name_gj_rowlane2(f64, n);
    if (!f64) {
        const bool fullf = (n % 16) == 0;
        switch ((n + 15) / 16) {
        case 1: return fullf ? "matinv_gj_tile_f32<1, true, true>" : "matinv_gj_tile_f32<1, false, true>";
        case 2: return fullf ? "matinv_gj_tile_f32<2, true, true>" : "matinv_gj_tile_f32<2, false, true>";
        case 3: return fullf ? "matinv_gj_tile_f32<3, true, true>" : "matinv_gj_tile_f32<3, false, true>";
        default: return fullf ? "matinv_gj_tile_f32<4, true, true>" : "matinv_gj_tile_f32<4, false, true>";
        }
    }
    const bool full = (n % 16) == 0;
    switch ((n + 15) / 16) {
    case 1: return full ? "matinv_gj_tile_f64<1, true, true>" : "matinv_gj_tile_f64<1, false, true>";
    case 2: return full ? "matinv_gj_tile_f64<2, true, true>" : "matinv_gj_tile_f64<2, false, true>";
    case 3: return full ? "matinv_gj_tile_f64<3, true, true>" : "matinv_gj_tile_f64<3, false, true>";
    default: return full ? "matinv_gj_tile_f64<4, true, true>" : "matinv_gj_tile_f64<4, false, true>";
    }
}

#endif

}  // namespace matinv
