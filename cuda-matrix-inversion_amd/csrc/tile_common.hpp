// tile_common.hpp -- pieces shared by the MFMA-tile kernel families (tile_kernels.hip: one wavefront per matrix,
// n <= 64; tile4_kernels.hip: four wavefronts per matrix, 64 < n <= 128).
#pragma once
#include "common.hpp"

namespace matinv {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

constexpr double TILE_TAU = 4.0;
constexpr int TILE_TSTRIDE = 17;  // padded row stride of the 16 x 16 LDS transpose buffer of the lower-tile sweeps (conflict-free reads)

// Scalar-type traits of the tile kernels. The two 16x16x4 MFMAs differ in their C/D lane map (checked on hardware with
// tools/mfma_layout_check.hip):   f64: tile row = 4*reg + (lane>>4)      f32: tile row = 4*(lane>>4) + reg
// (column = lane&15 for both). A pivot block must be the 4 rows that ONE accumulator register holds across the four lane
// groups q = 0..3 (that is what makes the B operand free), and its 4 columns must carry the same tile-local indices:
//   f64: block b = rows/cols 4b .. 4b+3          (lane c belongs to block c>>2, is pivot number c&3)
//   f32: block b = rows/cols b, b+4, b+8, b+12   (lane c belongs to block c&3,  is pivot number c>>2)
// i.e. the f32 kernels eliminate in a permuted order -- a symmetric relabelling, invisible in the result, but not in WHICH pivot
// is the first to fail: an f32 kernel that reports through PanelSolve::binfo names a column of the right 16-column tile (every
// earlier tile passed in either order), not necessarily the first non-positive leading minor (include/matinv.h, dInfo).
template <class T>
struct TileGeo;
template <>
struct TileGeo<double> {
    typedef v4d vec4;
    typedef v2d vec2;
    static __device__ __forceinline__ int trow(int r, int q) { return 4 * r + q; }
    static __device__ __forceinline__ int blk(int c) { return c >> 2; }
    static __device__ __forceinline__ int piv(int c) { return c & 3; }
    // tile-local column of pivot t in block rK; register / lane group of the tile-local row s (inverse of trow)
    static __device__ __forceinline__ int pcol(int rK, int t) { return 4 * rK + t; }
    // ragged n: blocks of the LAST tile column that hold at least one real column when rem = n - 16 (NT - 1) of its columns
    // are real (blocks from this number on are identity padding only and are not run)
    static __device__ __forceinline__ int real_blocks(int rem) { return (rem + 3) >> 2; }
    static __device__ __forceinline__ int slot_r(int s) { return (s >> 2) & 3; }
    static __device__ __forceinline__ int slot_q(int s) { return s & 3; }
    static __device__ __forceinline__ vec4 mfma(double a, double b, vec4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
};
template <>
struct TileGeo<float> {
    typedef v4f vec4;
    typedef v2f vec2;
    static __device__ __forceinline__ int trow(int r, int q) { return 4 * q + r; }
    static __device__ __forceinline__ int blk(int c) { return c & 3; }
    static __device__ __forceinline__ int piv(int c) { return c >> 2; }
    static __device__ __forceinline__ int pcol(int rK, int t) { return 4 * t + rK; }
    static __device__ __forceinline__ int real_blocks(int rem) { return rem < 4 ? rem : 4; }  // block rK = columns rK, rK + 4, ...
    static __device__ __forceinline__ int slot_r(int s) { return s & 3; }
    static __device__ __forceinline__ int slot_q(int s) { return (s >> 2) & 3; }
    static __device__ __forceinline__ vec4 mfma(float a, float b, vec4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};

// LDS ordering inside a ONE-wavefront workgroup: the LDS executes a wave's DS instructions in issue order, so a ds_read
// after a ds_write needs no counter wait -- only the compiler must keep the order. __syncthreads() would also work but
// is a workgroup-scope fence: it drains vmcnt, i.e. it would wait for the asynchronous LDS-DMA prefetch of the next
// matrix (and for the previous matrix's stores) in the middle of the elimination.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

__device__ __forceinline__ double fast_rcp(double x)
{
    // v_rcp_f64 + two Newton steps: full fp64 accuracy for normal x (no denormal/overflow fix-up needed here:
    // a pivot that small or large fails the TAU acceptance test and the matrix goes to the pivoted fallback)
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    return r;
}

// Acceptance test, wave-wide, evaluated on the spot and accumulated in an SGPR pair: bad |= ballot(!(|v| <= TAU)) (NaN
// fails). It is inline asm on purpose: written in C++ (`ok = ok && ...`, `bad |= __ballot(...)`, or a lane-local running
// max) hipcc sinks every comparison to the end of the kernel and keeps all multipliers of all 4*NT block steps alive
// (hundreds of VGPRs, or dozens of SGPR pairs spilled through v_writelane -- measured: 2x slower). TAU = 4.0 is an
// inline constant of the ISA.
__device__ __forceinline__ void note_fail(unsigned long long &bad, double v)
{
    static_assert(TILE_TAU == 4.0, "the asm below hard-codes the inline constant 4.0");
    asm volatile("v_cmp_nle_f64_e64 vcc, |%1|, 4.0\n\ts_or_b64 %0, %0, vcc" : "+s"(bad) : "v"(v) : "vcc");
}
__device__ __forceinline__ void note_fail(unsigned long long &bad, float v)
{
    asm volatile("v_cmp_nle_f32_e64 vcc, |%1|, 4.0\n\ts_or_b64 %0, %0, vcc" : "+s"(bad) : "v"(v) : "vcc");
}
// the same, lanes in `skip` exempt: one compare and a scalar mask instead of a select of the tested value per lane
__device__ __forceinline__ void note_fail_except(unsigned long long &bad, double v, unsigned long long skip)
{
    asm volatile("v_cmp_nle_f64_e64 vcc, |%1|, 4.0\n\ts_andn2_b64 vcc, vcc, %2\n\ts_or_b64 %0, %0, vcc" : "+s"(bad) : "v"(v), "s"(skip) : "vcc", "scc");
}
__device__ __forceinline__ void note_fail_except(unsigned long long &bad, float v, unsigned long long skip)
{
    asm volatile("v_cmp_nle_f32_e64 vcc, |%1|, 4.0\n\ts_andn2_b64 vcc, vcc, %2\n\ts_or_b64 %0, %0, vcc" : "+s"(bad) : "v"(v), "s"(skip) : "vcc", "scc");
}
__device__ __forceinline__ float fast_rcp(float x)
{
    float r = __builtin_amdgcn_rcpf(x);
    float e = __builtin_fmaf(-x, r, 1.0f);
    return __builtin_fmaf(r, e, r);
}

// 2.-4. read the pivot block D and this lane's panel rows from LDS, invert D (column q), form the A operand
//       aop[ti] = Aop[16ti + c][q] and update the acceptance flag. Split into NSTAGE pieces of roughly equal
//       VALU/LDS work so the look-ahead loop can issue one MFMA of the CURRENT block step between two pieces of the
//       NEXT step's panel (hardware issues in order: MFMA, ~64 cycles of VALU, MFMA, ... keeps both pipes busy).
// !(v > 0) accumulated like note_fail: SPD mode rejects a non-positive (or NaN) pivot
__device__ __forceinline__ void note_nonpositive(unsigned long long &bad, double v)
{
    asm volatile("v_cmp_ngt_f64_e64 vcc, %1, 0\n\ts_or_b64 %0, %0, vcc" : "+s"(bad) : "v"(v) : "vcc");
}
__device__ __forceinline__ void note_nonpositive(unsigned long long &bad, float v)
{
    asm volatile("v_cmp_ngt_f32_e64 vcc, %1, 0\n\ts_or_b64 %0, %0, vcc" : "+s"(bad) : "v"(v) : "vcc");
}

// the same, and binfo = val at the FIRST pivot that fails (binfo stays 0 while every pivot was positive). All in scalar
// instructions inside one asm block: written as a C++ select on `bad` hipcc spills hundreds of SGPRs in the 12 x 12 tile kernel.
__device__ __forceinline__ void note_nonpositive_first(unsigned long long &bad, int &binfo, double v, int val)
{
    int tmp;
    asm volatile("v_cmp_ngt_f64_e64 vcc, %[v], 0\n\t"
                 "s_cmp_eq_u64 %[bad], 0\n\t"
                 "s_cselect_b32 %[tmp], %[val], 0\n\t"
                 "s_cmp_lg_u64 vcc, 0\n\t"
                 "s_cselect_b32 %[tmp], %[tmp], 0\n\t"
                 "s_or_b32 %[binfo], %[binfo], %[tmp]\n\t"
                 "s_or_b64 %[bad], %[bad], vcc"
                 : [bad] "+s"(bad), [binfo] "+s"(binfo), [tmp] "=&s"(tmp)
                 : [v] "v"(v), [val] "s"(val)
                 : "vcc", "scc");
}
__device__ __forceinline__ void note_nonpositive_first(unsigned long long &bad, int &binfo, float v, int val)
{
    int tmp;
    asm volatile("v_cmp_ngt_f32_e64 vcc, %[v], 0\n\t"
                 "s_cmp_eq_u64 %[bad], 0\n\t"
                 "s_cselect_b32 %[tmp], %[val], 0\n\t"
                 "s_cmp_lg_u64 vcc, 0\n\t"
                 "s_cselect_b32 %[tmp], %[tmp], 0\n\t"
                 "s_or_b32 %[binfo], %[binfo], %[tmp]\n\t"
                 "s_or_b64 %[bad], %[bad], vcc"
                 : [bad] "+s"(bad), [binfo] "+s"(binfo), [tmp] "=&s"(tmp)
                 : [v] "v"(v), [val] "s"(val)
                 : "vcc", "scc");
}

// ---- error path of the fp32 kernels that write info themselves ---------------------------------------------------------------------
// The fp32 sweeps eliminate the 16 columns of a tile in the order of TileGeo<float>::pcol, so the first pivot they see fail lies in the
// right tile but is not necessarily the first non-positive leading minor, which is what info has to name (include/matinv.h). A matrix
// that failed is therefore factorised once more in NATURAL order, one column at a time (rank-1 LDL^T steps, no blocking), until the
// first non-positive (or NaN) pivot shows. Only rejected matrices come here: the sweep itself is what it was.
// Returns the 1-based column, or 0 when every natural-order pivot was positive (a borderline matrix that only the rounding of the
// permuted order rejects: the caller keeps the sweep's own code).
//
// One wavefront, matrix re-read from memory (lower triangle of the column-major n x n block at A, leading dimension n; cdiag: optional
// vector added to the diagonal) into lower accumulator tiles -- the sweep's own are dead by now. colbuf: 16 NT elements of LDS.
template <int NT, class T>
__device__ __forceinline__ int spd_natural_first_failure(const T *A, const T *cdiag, int n, T *colbuf, int l)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    int q = l >> 4, c = l & 15;
    asm volatile("" : "+v"(q), "+v"(c));
    vec4 w[NT][NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
            if (tj > ti) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * ti + G::trow(r, q), col = 16 * tj + c;
                const bool in = row < n && col < n;
                const int hi = row > col ? row : col, lo = row > col ? col : row;
                T v = in ? A[(unsigned)(lo * n + hi)] : ((row == col) ? (T)1 : (T)0);
                if (cdiag && ti == tj && row == col && in) v += cdiag[row];
                w[ti][tj][r] = v;
            }
        }
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

// The same for one wavefront on a block in LDS: S, m x m, column-major with leading dimension ld, lower triangle; destroyed.
template <class T>
__device__ __forceinline__ int spd_natural_first_failure_lds(T *S, int ld, int m, int l)
{
    int found = 0;
    for (int j = 0; j < m && found == 0; ++j) {
        wave_lds_sync();
        const T piv = S[j * ld + j];
        if (__ballot(!(piv > (T)0)) != 0ull) {
            found = j + 1;
        } else {
            const T rp = (T)1 / piv;
            const int k = m - j - 1;
            for (int e = l; e < k * k; e += 64) {
                const int cc = e / k, rr = e - cc * k;
                if (rr >= cc) {
                    const int C = j + 1 + cc, R = j + 1 + rr;
                    S[C * ld + R] = fma_t(-S[j * ld + R], S[j * ld + C] * rp, S[C * ld + R]);
                }
            }
        }
    }
    wave_lds_sync();
    return found;
}

// SPD = true: symmetric blocked sweep for SPD input (see matinv_spd_tile_f64). Same arithmetic for D^-1 and Aop; the
// acceptance test becomes "all four pivots of D positive" (they are the squares of the Cholesky diagonal), and the
// stage of tile row ti also returns bsym[ti] = P[16ti + c][q], the B operand by symmetry (W[K, J] = W[J, K]^T).
//
// GATED = true: stages 0-5 -- the LU factorisation of D, its four reciprocals and the two triangular solves -- compute numbers that
// depend on the lane through q = lane >> 4 only, so they run in ONE lane per row of 16 (c == 0; EXEC narrowed by a compile-time lane
// mask, restored inside each stage: no MFMA is ever issued under the narrowed mask; the reads of D from LDS included), and x0 .. x3
// reach the other 15 lanes of the row by DPP row_newbcast:0 at the end of stage 5 (stage_gated below). Same operations on the same operands in the same order per value, hence the same bits;
// a masked lane contributes a zero bit to `bad |= vcc` and the tested values are uniform per q, so the verdict is the same as well.
constexpr unsigned long long PANEL_GATE_LANES = 0x0001000100010001ULL;  // lane 16 q, q = 0 .. 3
constexpr int DPP_ROW_NEWBCAST0 = 0x150;                                 // LLVM DppCtrl: lane 0 of each row of 16

// BSYM: the stages of the tile rows return bsym. It comes with SPD; the symmetric arm of the Gauss-Jordan kernel (gj_tile_body)
// asks for it on its own: bsym AND the multiplier test, gated or not.
template <int NT, bool SPD = false, class T = double, bool GATED = false, bool BSYM = SPD>
struct PanelSolve {
    typedef TileGeo<T> G;
    static constexpr int NSTAGE = 6 + NT;
    int *binfo = nullptr;  // SPD: when set, *binfo becomes (column of the FIRST non-positive pivot in elimination order) + 1 (scalar selects only)
    T d[4][4];
    T r0, r1, r2, r3, l10, l20, l30, l21, l31, l32, u11, u12, u13, u22, u23, u33;
    T a21, a22, a23, a31, a32, a33, b32, b33, y0, y1, y2, y3, x0, x1, x2, x3;

    __device__ __forceinline__ void stage(int s, const T *panel, int kb, int q, int c, T (&aop)[NT],
                                          unsigned long long &bad)
    {
        T unused[NT];
        stage(s, panel, kb, q, c, aop, unused, bad);
    }
    __device__ __forceinline__ void stage(int s, const T *panel, int kb, int q, int c, T (&aop)[NT],
                                          T (&bsym)[NT], unsigned long long &bad)
    {
        if constexpr (GATED) {
            if (s < 6) {
                stage_gated(s, panel, kb, q, bad);
                return;
            }
        }
        stage_impl(s, panel, kb, q, c, aop, bsym, bad);
    }

    // Stages 0-5 of the GATED mode, fp64. Each piece is asm that narrows EXEC to PANEL_GATE_LANES on entry and restores it on exit, so
    // the compiler sees straight-line code on ordinary values (a C++ branch per piece costs the headline kernel 48 VGPRs and 84 B of
    // scratch) and no MFMA or register copy of its own can land under the narrowed mask. The LU factors overwrite d in place:
    // d[i][j] = l_ij below the diagonal, u_ij on and above it; y becomes x. Operation for operation it is stage_impl's arithmetic.
    // Hazards (nothing is padded inside an asm block): one wait state between v_rcp_f64 and the first use of its result; the LDS reads
    // are waited for before the block ends; two wait states between the last write of x and the DPP reads that follow stage 5.
#define MATINV_PS_BEGIN "s_and_saveexec_b64 %[save], %[lanes]\n\t"
#define MATINV_PS_END "s_mov_b64 exec, %[save]"
#define MATINV_PS_RCP(r, x) /* fast_rcp */                                                                                             \
    "v_rcp_f64_e32 %[" #r "], %[" #x "]\n\ts_nop 0\n\t"                                                                               \
    "v_fma_f64 %[e], -%[" #x "], %[" #r "], 1.0\n\tv_fmac_f64_e32 %[" #r "], %[" #r "], %[e]\n\t"                                     \
    "v_fma_f64 %[e], -%[" #x "], %[" #r "], 1.0\n\tv_fmac_f64_e32 %[" #r "], %[" #r "], %[e]\n\t"
#define MATINV_PS_FMA(d, a, b, c) "v_fma_f64 %[" #d "], -%[" #a "], %[" #b "], %[" #c "]\n\t" /* d = c - a b */
#define MATINV_PS_MUL(d, a, b) "v_mul_f64 %[" #d "], %[" #a "], %[" #b "]\n\t"
#define MATINV_PS_TEST(v) "v_cmp_nle_f64_e64 vcc, |%[" #v "]|, 4.0\n\ts_or_b64 %[bad], %[bad], vcc\n\t"
    __device__ __forceinline__ void stage_gated(int s, const T *panel, int kb, int q, unsigned long long &bad)
    {
        static_assert(!GATED || (sizeof(T) == 8 && !SPD), "the gated pivot-block solve is written for fp64 and the multiplier test");
        static_assert(TILE_TAU == 4.0, "the asm below hard-codes the inline constant 4.0");
        const unsigned long long lanes = PANEL_GATE_LANES;
        unsigned long long save;
        T e;
        if (s == 0) {
            // row i of D: 32 bytes at panel + 32 (4 kb + i)  (f64: trow(rK, i) = 4 rK + i)
            const unsigned addr = (unsigned)(unsigned long long)panel + 128u * (unsigned)kb;
            typename G::vec2 d0a, d0b, d1a, d1b, d2a, d2b, d3a, d3b;
            asm volatile(MATINV_PS_BEGIN
                         "ds_read_b128 %[d0a], %[addr]\n\tds_read_b128 %[d0b], %[addr] offset:16\n\t"
                         "ds_read_b128 %[d1a], %[addr] offset:32\n\tds_read_b128 %[d1b], %[addr] offset:48\n\t"
                         "ds_read_b128 %[d2a], %[addr] offset:64\n\tds_read_b128 %[d2b], %[addr] offset:80\n\t"
                         "ds_read_b128 %[d3a], %[addr] offset:96\n\tds_read_b128 %[d3b], %[addr] offset:112\n\t"
                         "s_waitcnt lgkmcnt(0)\n\t" MATINV_PS_END
                         : [d0a] "=&v"(d0a), [d0b] "=&v"(d0b), [d1a] "=&v"(d1a), [d1b] "=&v"(d1b), [d2a] "=&v"(d2a), [d2b] "=&v"(d2b),
                           [d3a] "=&v"(d3a), [d3b] "=&v"(d3b), [save] "=&s"(save)
                         : [lanes] "s"(lanes), [addr] "v"(addr)
                         : "scc", "memory");
            d[0][0] = d0a[0], d[0][1] = d0a[1], d[0][2] = d0b[0], d[0][3] = d0b[1];
            d[1][0] = d1a[0], d[1][1] = d1a[1], d[1][2] = d1b[0], d[1][3] = d1b[1];
            d[2][0] = d2a[0], d[2][1] = d2a[1], d[2][2] = d2b[0], d[2][3] = d2b[1];
            d[3][0] = d3a[0], d[3][1] = d3a[1], d[3][2] = d3b[0], d[3][3] = d3b[1];
            asm volatile(MATINV_PS_BEGIN MATINV_PS_RCP(r0, d00)
                         MATINV_PS_MUL(l10, l10, r0) MATINV_PS_MUL(l20, l20, r0) MATINV_PS_MUL(l30, l30, r0) MATINV_PS_END
                         : [r0] "=&v"(r0), [e] "=&v"(e), [l10] "+v"(d[1][0]), [l20] "+v"(d[2][0]), [l30] "+v"(d[3][0]), [save] "=&s"(save)
                         : [lanes] "s"(lanes), [d00] "v"(d[0][0])
                         : "scc");
        } else if (s == 1) {
            asm volatile(MATINV_PS_BEGIN
                         MATINV_PS_FMA(u11, l10, d01, u11) MATINV_PS_FMA(u12, l10, d02, u12) MATINV_PS_FMA(u13, l10, d03, u13)
                         MATINV_PS_FMA(a21, l20, d01, a21) MATINV_PS_FMA(a22, l20, d02, a22) MATINV_PS_FMA(a23, l20, d03, a23)
                         MATINV_PS_FMA(a31, l30, d01, a31) MATINV_PS_FMA(a32, l30, d02, a32) MATINV_PS_FMA(a33, l30, d03, a33)
                         MATINV_PS_RCP(r1, u11) MATINV_PS_END
                         : [u11] "+v"(d[1][1]), [u12] "+v"(d[1][2]), [u13] "+v"(d[1][3]), [a21] "+v"(d[2][1]), [a22] "+v"(d[2][2]),
                           [a23] "+v"(d[2][3]), [a31] "+v"(d[3][1]), [a32] "+v"(d[3][2]), [a33] "+v"(d[3][3]), [r1] "=&v"(r1),
                           [e] "=&v"(e), [save] "=&s"(save)
                         : [lanes] "s"(lanes), [l10] "v"(d[1][0]), [l20] "v"(d[2][0]), [l30] "v"(d[3][0]), [d01] "v"(d[0][1]),
                           [d02] "v"(d[0][2]), [d03] "v"(d[0][3])
                         : "scc");
        } else if (s == 2) {
            asm volatile(MATINV_PS_BEGIN
                         MATINV_PS_MUL(l21, l21, r1) MATINV_PS_MUL(l31, l31, r1)
                         MATINV_PS_FMA(u22, l21, u12, u22) MATINV_PS_FMA(u23, l21, u13, u23)
                         MATINV_PS_FMA(b32, l31, u12, b32) MATINV_PS_FMA(b33, l31, u13, b33)
                         MATINV_PS_RCP(r2, u22)
                         MATINV_PS_MUL(b32, b32, r2) MATINV_PS_FMA(b33, b32, u23, b33) MATINV_PS_END
                         : [l21] "+v"(d[2][1]), [l31] "+v"(d[3][1]), [u22] "+v"(d[2][2]), [u23] "+v"(d[2][3]), [b32] "+v"(d[3][2]),
                           [b33] "+v"(d[3][3]), [r2] "=&v"(r2), [e] "=&v"(e), [save] "=&s"(save)
                         : [lanes] "s"(lanes), [r1] "v"(r1), [u12] "v"(d[1][2]), [u13] "v"(d[1][3])
                         : "scc");
        } else if (s == 3) {
            // a zero / non-finite last pivot needs no test of its own: see stage_impl
            asm volatile(MATINV_PS_BEGIN MATINV_PS_RCP(r3, u33)
                         MATINV_PS_TEST(l10) MATINV_PS_TEST(l20) MATINV_PS_TEST(l30) MATINV_PS_TEST(l21) MATINV_PS_TEST(l31)
                         MATINV_PS_TEST(l32) MATINV_PS_END
                         : [r3] "=&v"(r3), [e] "=&v"(e), [bad] "+s"(bad), [save] "=&s"(save)
                         : [lanes] "s"(lanes), [u33] "v"(d[3][3]), [l10] "v"(d[1][0]), [l20] "v"(d[2][0]), [l30] "v"(d[3][0]),
                           [l21] "v"(d[2][1]), [l31] "v"(d[3][1]), [l32] "v"(d[3][2])
                         : "vcc", "scc");
        } else if (s == 4) {
            // L y = e_q (y0 = e_q[0]); the right-hand side enters as the addend of the first FMA of its row
            y0 = (q == 0) ? (T)1 : (T)0;
            const T e1 = (q == 1) ? (T)1 : (T)0, e2 = (q == 2) ? (T)1 : (T)0, e3 = (q == 3) ? (T)1 : (T)0;
            asm volatile(MATINV_PS_BEGIN
                         MATINV_PS_FMA(y1, l10, y0, e1)
                         MATINV_PS_FMA(y2, l20, y0, e2) MATINV_PS_FMA(y2, l21, y1, y2)
                         MATINV_PS_FMA(y3, l30, y0, e3) MATINV_PS_FMA(y3, l31, y1, y3) MATINV_PS_FMA(y3, l32, y2, y3) MATINV_PS_END
                         : [y1] "=&v"(y1), [y2] "=&v"(y2), [y3] "=&v"(y3), [save] "=&s"(save)
                         : [lanes] "s"(lanes), [y0] "v"(y0), [e1] "v"(e1), [e2] "v"(e2), [e3] "v"(e3), [l10] "v"(d[1][0]),
                           [l20] "v"(d[2][0]), [l30] "v"(d[3][0]), [l21] "v"(d[2][1]), [l31] "v"(d[3][1]), [l32] "v"(d[3][2])
                         : "scc");
        } else {
            // U x = y, x1 .. x3 in place of y1 .. y3; then x0 .. x3 of lane 16 q to the whole row
            asm volatile(MATINV_PS_BEGIN
                         MATINV_PS_MUL(y3, y3, r3)
                         MATINV_PS_FMA(y2, u23, y3, y2) MATINV_PS_MUL(y2, y2, r2)
                         MATINV_PS_FMA(y1, u12, y2, y1) MATINV_PS_FMA(y1, u13, y3, y1) MATINV_PS_MUL(y1, y1, r1)
                         MATINV_PS_FMA(x0, d01, y1, y0) MATINV_PS_FMA(x0, d02, y2, x0) MATINV_PS_FMA(x0, d03, y3, x0)
                         MATINV_PS_MUL(x0, x0, r0) "s_nop 1\n\t" MATINV_PS_END
                         : [x0] "=&v"(x0), [y1] "+v"(y1), [y2] "+v"(y2), [y3] "+v"(y3), [save] "=&s"(save)
                         : [lanes] "s"(lanes), [y0] "v"(y0), [r0] "v"(r0), [r1] "v"(r1), [r2] "v"(r2), [r3] "v"(r3), [d01] "v"(d[0][1]),
                           [d02] "v"(d[0][2]), [d03] "v"(d[0][3]), [u12] "v"(d[1][2]), [u13] "v"(d[1][3]), [u23] "v"(d[2][3])
                         : "scc");
            x0 = __builtin_amdgcn_update_dpp(x0, x0, DPP_ROW_NEWBCAST0, 0xf, 0xf, false);
            x1 = __builtin_amdgcn_update_dpp(y1, y1, DPP_ROW_NEWBCAST0, 0xf, 0xf, false);
            x2 = __builtin_amdgcn_update_dpp(y2, y2, DPP_ROW_NEWBCAST0, 0xf, 0xf, false);
            x3 = __builtin_amdgcn_update_dpp(y3, y3, DPP_ROW_NEWBCAST0, 0xf, 0xf, false);
        }
    }
#undef MATINV_PS_BEGIN
#undef MATINV_PS_END
#undef MATINV_PS_RCP
#undef MATINV_PS_FMA
#undef MATINV_PS_MUL
#undef MATINV_PS_TEST
    __device__ __forceinline__ void stage_impl(int s, const T *panel, int kb, int q, int c, T (&aop)[NT],
                                               T (&bsym)[NT], unsigned long long &bad)
    {
        const int tK = kb >> 2, rK = kb & 3;
        const bool panel_lane = G::blk(c) == rK;
        if (s == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) d[i][j] = panel[(16 * tK + G::trow(rK, i)) * 4 + j];
            // LU of D without pivoting (multipliers checked below)
            r0 = fast_rcp(d[0][0]);
            l10 = d[1][0] * r0, l20 = d[2][0] * r0, l30 = d[3][0] * r0;
        } else if (s == 1) {
            u11 = fma_t(-l10, d[0][1], d[1][1]), u12 = fma_t(-l10, d[0][2], d[1][2]);
            u13 = fma_t(-l10, d[0][3], d[1][3]);
            a21 = fma_t(-l20, d[0][1], d[2][1]), a22 = fma_t(-l20, d[0][2], d[2][2]);
            a23 = fma_t(-l20, d[0][3], d[2][3]);
            a31 = fma_t(-l30, d[0][1], d[3][1]), a32 = fma_t(-l30, d[0][2], d[3][2]);
            a33 = fma_t(-l30, d[0][3], d[3][3]);
            r1 = fast_rcp(u11);
        } else if (s == 2) {
            l21 = a21 * r1, l31 = a31 * r1;
            u22 = fma_t(-l21, u12, a22), u23 = fma_t(-l21, u13, a23);
            b32 = fma_t(-l31, u12, a32), b33 = fma_t(-l31, u13, a33);
            r2 = fast_rcp(u22);
            l32 = b32 * r2;
            u33 = fma_t(-l32, u23, b33);
        } else if (s == 3) {
            r3 = fast_rcp(u33);
            if (SPD) {
                if (binfo) {
                    note_nonpositive_first(bad, *binfo, d[0][0], 16 * tK + G::pcol(rK, 0) + 1);
                    note_nonpositive_first(bad, *binfo, u11, 16 * tK + G::pcol(rK, 1) + 1);
                    note_nonpositive_first(bad, *binfo, u22, 16 * tK + G::pcol(rK, 2) + 1);
                    note_nonpositive_first(bad, *binfo, u33, 16 * tK + G::pcol(rK, 3) + 1);
                } else {
                    note_nonpositive(bad, d[0][0]), note_nonpositive(bad, u11);
                    note_nonpositive(bad, u22), note_nonpositive(bad, u33);
                }
            } else {
                note_fail(bad, l10), note_fail(bad, l20), note_fail(bad, l30);
                note_fail(bad, l21), note_fail(bad, l31), note_fail(bad, l32);
            }
            // a zero / non-finite last pivot needs no test of its own: r3 = inf/NaN makes x, hence every Aop entry
            // outside the pivot rows (0 * inf = NaN included), fail the test in the last stages
        } else if (s == 4) {
            // L y = e_q
            y0 = (q == 0) ? (T)1 : (T)0;
            y1 = fma_t(-l10, y0, (q == 1) ? (T)1 : (T)0);
            y2 = fma_t(-l21, y1, fma_t(-l20, y0, (q == 2) ? (T)1 : (T)0));
            y3 = fma_t(-l32, y2, fma_t(-l31, y1, fma_t(-l30, y0, (q == 3) ? (T)1 : (T)0)));
        } else if (s == 5) {
            // U x = y : x = column q of D^-1
            x3 = y3 * r3;
            x2 = fma_t(-u23, x3, y2) * r2;
            x1 = fma_t(-u13, x3, fma_t(-u12, x2, y1)) * r1;
            x0 = fma_t(-d[0][3], x3, fma_t(-d[0][2], x2, fma_t(-d[0][1], x1, y0))) * r0;
        } else {
            const int ti = s - 6;
            const T *w = &panel[(16 * ti + c) * 4];
            const T w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
            // -(w . x) with the negation on the inputs: the FMAs' neg modifiers instead of a sign flip afterwards (the same
            // bits: round-to-nearest is symmetric)
            T v = fma_t(-w3, x3, fma_t(-w2, x2, fma_t(-w1, x1, -w0 * x0)));
            if (ti == tK) {
                // pivot rows: D^-1 itself (their C operand is zeroed), exempt from the multiplier test
                const int m = G::piv(c);
                const T x01 = (m & 1) ? x1 : x0, x23 = (m & 1) ? x3 : x2;
                const T xm = (m & 2) ? x23 : x01;
                if (!SPD) note_fail_except(bad, v, __ballot(panel_lane));
                v = panel_lane ? xm : v;
            } else {
                if (!SPD) note_fail(bad, v);
            }
            aop[ti] = v;
            if (BSYM && SPD) {
                const T w01 = (q & 1) ? w1 : w0, w23 = (q & 1) ? w3 : w2;
                bsym[ti] = (q & 2) ? w23 : w01;
            } else if (BSYM) {
                bsym[ti] = w[q];  // one more LDS read in place of three selects on 64-bit values (408 v_cndmask_b32 per 64 x 64 matrix)
            }
        }
    }
};

template <int NT, bool GATED = false, class T>
__device__ __forceinline__ void panel_solve(const T *panel, int kb, int q, int c, T (&aop)[NT],
                                            unsigned long long &bad)
{
    PanelSolve<NT, false, T, GATED> ps;
#pragma unroll
    for (int s = 0; s < PanelSolve<NT, false, T, GATED>::NSTAGE; ++s) ps.stage(s, panel, kb, q, c, aop, bad);
}

// ---- symmetric (lower-triangular tile storage) helpers, shared by the SPD inverse and the fused GP kernel ----------
template <int NT, class T>
__device__ __forceinline__ void spd_panel_to_lds(T *panel, const typename TileGeo<T>::vec4 (&acc)[NT][NT], int kb, int q, int c)
{
    typedef TileGeo<T> G;
    const int tK = kb >> 2, rK = kb & 3;
    if (G::blk(c) == rK) {
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
            if (ti < tK) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) panel[(16 * ti + G::trow(r, q)) * 4 + G::piv(c)] = acc[ti][tK][r];
        }
    }
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        if (ti >= tK) continue;
        panel[(16 * ti + c) * 4 + q] = acc[tK][ti][rK];  // W[16ti + c][pivot q] = W[pivot q][16ti + c]
    }
}

template <int NT, class T>
__device__ __forceinline__ void spd_prep_operands(typename TileGeo<T>::vec4 (&acc)[NT][NT], T (&bop)[NT], int kb, int q, int c)
{
    typedef TileGeo<T> G;
    const int tK = kb >> 2, rK = kb & 3;
    const bool panel_lane = G::blk(c) == rK;
    const bool diag_lane = panel_lane && (G::piv(c) == q);
    bop[tK] = panel_lane ? (diag_lane ? (T)-1 : (T)0) : bop[tK];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
        if (ti < tK) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[ti][tK][r] = panel_lane ? (T)0 : acc[ti][tK][r];
    }
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) {
        if (tj > tK) continue;
        acc[tK][tj][rK] = (T)0;
    }
}

}  // namespace matinv
