// logml_grad_tile_impl.hpp (instantiated by logml_grad_tile_kernels.hip for f64 and logml_grad_tile_f32_kernels.hip for f32) -- gradients
// of the batched GP log marginal likelihood on the MFMA tile layout, n <= 96. With M = B + diag c (c optional), K = M^-1, alpha = K d and
// P symmetric derivative matrices dM_p:
//     grad[p]  = 1/2 sum_ij (alpha_i alpha_j - K_ij) dM_p[i][j]      gradc[i] = 1/2 (alpha_i^2 - K_ii)      alpha[i] = alpha_i
// The load, the PanelSolve pipeline and the block-step loop are spd_load_lower and spd_full_sweep (spd_sweep.hpp), shared with
// loo_tile_body (loo_tile_impl.hpp) and every later GP tile kernel. The sweep
// ends with W = -M^-1 in the lower tiles (diagonal tiles complete); the epilogue folds diag W and W d out of the registers as the LOO
// epilogue does, turns the accumulators into G = alpha alpha^T + W in place and contracts them with the lower tiles of each dM_p
// streamed from HBM, so neither M nor its inverse is ever stored.
// HBM traffic per matrix: (P + 1) n^2 / 2 + 2 n elements in, P + 2 n out.
// A non-positive (or NaN) pivot makes info = its column + 1 (PanelSolve::binfo) and every output NaN: no fallback launch.
//
// The kernels are the gradient forms of the SPD inversion kernels whose sweep they run: overloads of matinv_spd_tile_f64 / _f32 with two
// more trailing template arguments ("Gradients of the log marginal likelihood", says why).
#pragma once
#include <cstdio>

#include "spd_sweep.hpp"

namespace matinv {

// Sum over the 16 lanes of a DPP row (the lanes of one q group), every lane receives it: two quad permutes, row_half_mirror,
// row_mirror. Floating-point addition is commutative, so the 16 lanes end with the same bits. No LDS round trip (a __shfl_xor is a
// ds_bpermute behind an s_waitcnt). Needs all 64 lanes active.
constexpr int DPP_QUAD_XOR1 = 0xB1;         // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;         // quad_perm:[2,3,0,1]
constexpr int DPP_ROW_HALF_MIRROR = 0x141;  // lane i of each half row reads lane 7 - i
constexpr int DPP_ROW_MIRROR = 0x140;       // lane i of each row reads lane 15 - i
template <class T>
__device__ __forceinline__ T dpp_row_sum16(T v)
{
    v += __builtin_amdgcn_update_dpp(v, v, DPP_QUAD_XOR1, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(v, v, DPP_QUAD_XOR2, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(v, v, DPP_ROW_HALF_MIRROR, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(v, v, DPP_ROW_MIRROR, 0xf, 0xf, false);
    return v;
}

// Epilogue layout (lane l = 16 q + c; the lane holds W[16 ti + trow(r, q)][16 tj + c] in acc[ti][tj][r], tj <= ti):
//   LDS, in the panel buffer (4 N elements, free after the last block step):  sd[N] = d (zero beyond n),  rs[N] = row part of W d,
//   kap[N] = -W_ii,  al[N] = alpha.
//   alpha, kappa: as in loo_tile_body -- the row part of W d summed over the 16 c lanes (here by DPP), the mirror part over the four q
//                 groups; every lane then holds alpha of index 16 tj + c for each tj. Lane group q = 0 writes alpha and gradc as
//                 16-element segments and alpha to LDS, from where every lane reads alpha of its four rows per tile row.
//   G           : acc[ti][tj][r] <- w (alpha_row alpha_col + acc[ti][tj][r]),  w = 1/2 in the diagonal tiles (both triangles stored),
//                 w = 1 in the strictly lower ones (each stands for its mirror, which is not stored).
//   contraction : per p, the lane's 4 * NT (NT + 1) / 2 products with dM_p (same addressing and predication as the load of B; diagonal
//                 tiles through the (lo, hi) mirror) in four chains by register, ((p0 + p1) + (p2 + p3)), the 16 c lanes by DPP, the
//                 four q groups by two __shfl_xor: a fixed order that knows nothing of batch, grid or P. Lane 0 stores.
template <class T, int NT, bool FULL>
__device__ __forceinline__ void logml_grad_tile_body(const T *Bs, const T *Cs, const T *Ds, const T *dMs, int nparam, T *grad, T *gradc,
                                                     T *alpha, int *info, int n_rt, unsigned batch, T *panel)
{
    typedef TileGeo<T> G;
    typedef typename G::vec4 vec4;
    constexpr int N = 16 * NT;
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
        const T *vd = Ds + (size_t)mat * n;
        wave_lds_sync();  // the last panel has been consumed
        T *const sd = panel, *const rs = panel + N, *const kap = panel + 2 * N, *const al = panel + 3 * N;
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
        T acol[NT];
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
            const int i = 16 * tj + c;
            const bool in = FULL || tj < NT - 1 || i < n;
            const T a = -(rs[i] + colacc[tj]);  // W = -M^-1
            acol[tj] = a;
            if (q == 0) al[i] = a;  // the four q groups hold the same bits
            if (in && q == 0) {
                if (alpha) alpha[(size_t)mat * n + i] = ok ? a : nan_of<T>();
                if (gradc) gradc[(size_t)mat * n + i] = ok ? (T)0.5 * fma_t(a, a, -kap[i]) : nan_of<T>();
            }
        }
        if (grad) {  // wave-uniform
            wave_lds_sync();
            // G = alpha alpha^T + W, weighted, in place of W
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                T ar[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) ar[r] = al[16 * ti + G::trow(r, q)];
#pragma unroll
                for (int tj = 0; tj <= ti; ++tj) {
                    const T w = (tj == ti) ? (T)0.5 : (T)1;
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[ti][tj][r] = w * fma_t(ar[r], acol[tj], acc[ti][tj][r]);
                }
            }
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
        int code = binfo;
        if constexpr (sizeof(T) == 4) {
            if (bad != 0) {  // wave-uniform; rejected matrices only: the fp32 tile order does not say which column fails FIRST (tile_common.hpp)
                const int nat = spd_natural_first_failure<NT, T>(A, Cs ? Cs + (size_t)mat * n : nullptr, n, panel, l);
                if (nat) code = nat;
            }
        }
        if (l == 0 && info) info[mat] = code;
        wave_lds_sync();  // the next matrix's first panel write must not pass this one's last reads
    }
}

// The gradient forms of matinv_spd_tile_f64 / matinv_spd_tile_f32 (tile_impl.hpp): the same names with a third and a fourth template
// argument, the launch bounds of the LOO forms for the same NT (loo_tile_impl.hpp) -- except the two ragged forms that spill under them
// (fp64 4 x 4 tiles at three waves per SIMD: 6 registers, fp32 6 x 6 at three: 21; profiles/logml_grad_kernel_registers.txt), which take
// one wave less per SIMD and no scratch.
constexpr int logml_grad_f64_waves(int nt, bool full)
{
    const int inverse = nt >= 5 ? 2 : (nt >= 4 ? 3 : 4);                 // matinv_spd_tile_f64<NT, FULL>
    const int loo = inverse - ((!full && (nt == 3 || nt == 6)) ? 1 : 0);  // matinv_spd_tile_f64<NT, FULL, true>
    return loo - ((!full && nt == 4) ? 1 : 0);
}
constexpr int logml_grad_f32_waves(int nt, bool full)
{
    const int loo = nt >= 5 ? 3 : 4;  // matinv_spd_tile_f32<NT, FULL, true>, the inverse's
    return loo - ((!full && nt == 6) ? 1 : 0);
}

template <int NT, bool FULL, bool LOO, bool GRAD>
__global__ __launch_bounds__(64, logml_grad_f64_waves(NT, FULL)) void matinv_spd_tile_f64(const double *Bs, const double *Cs,
                                                                                                 const double *Ds, const double *dMs, int nparam,
                                                                                                 double *grad, double *gradc, double *alpha,
                                                                                                 int *info, int n_rt, unsigned batch)
{
    static_assert(LOO && GRAD, "the four-argument form is the log-marginal-likelihood gradient kernel");
    __shared__ __attribute__((aligned(16))) double panel[16 * NT * 4];
    logml_grad_tile_body<double, NT, FULL>(Bs, Cs, Ds, dMs, nparam, grad, gradc, alpha, info, n_rt, batch, panel);
}

template <int NT, bool FULL, bool LOO, bool GRAD>
__global__ __launch_bounds__(64, logml_grad_f32_waves(NT, FULL)) void matinv_spd_tile_f32(const float *Bs, const float *Cs, const float *Ds,
                                                                                                 const float *dMs, int nparam, float *grad,
                                                                                                 float *gradc, float *alpha, int *info, int n_rt,
                                                                                                 unsigned batch)
{
    static_assert(LOO && GRAD, "the four-argument form is the log-marginal-likelihood gradient kernel");
    __shared__ __attribute__((aligned(16))) float panel[16 * NT * 4];
    logml_grad_tile_body<float, NT, FULL>(Bs, Cs, Ds, dMs, nparam, grad, gradc, alpha, info, n_rt, batch, panel);
}

template <class T>
hipError_t launch_logml_grad_tile(int n, int nparam, const T *Bs, const T *Cs, const T *Ds, const T *dMs, T *grad, T *gradc, T *alpha,
                                  size_t batch, int *info, hipStream_t stream)
{
    if (!logml_grad_tile_supports(n)) return hipErrorInvalidValue;
    if (batch == 0) return hipSuccess;
    const unsigned grid = tile_grid(batch, 12u), b = (unsigned)batch;
    with_tile<1, 6>(tile_shape(n), [&](auto NT, auto FULL) {
        if constexpr (sizeof(T) == 8)
            hipLaunchKernelGGL((matinv_spd_tile_f64<NT, FULL, true, true>), dim3(grid), dim3(64), 0, stream, Bs, Cs, Ds, dMs, nparam, grad, gradc,
                               alpha, info, n, b);
        else
            hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL, true, true>), dim3(grid), dim3(64), 0, stream, Bs, Cs, Ds, dMs, nparam, grad, gradc,
                               alpha, info, n, b);
    });
    return hipGetLastError();
}
}  // namespace matinv
