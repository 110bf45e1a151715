// spd_wide_f64_kernels.hip -- fp64 one-wavefront symmetric sweep of 7 x 7 lower tiles (96 < n <= 112; 224 accumulator registers, one
// wave per SIMD), inverse and fused mean / variance (tile_impl.hpp). A translation unit of its own so that it can be compiled with
// VGPR-form MFMAs and the AGPRs as parking space -- with hipcc's default AGPR-form MFMAs the same kernels are correct here (256-bit
// results never overlap their C operand) but slower: Cholesky 112^2 1.36e7 -> 1.59e7 inv/s, pipeline 1.42e7 -> 1.48e7 items/s.
#ifndef MATINV_MFMA_VGPR_FORM
#error "build with -mllvm -amdgpu-mfma-vgpr-form=1 -DMATINV_MFMA_VGPR_FORM=1 (Makefile)"
#endif
#include "tile_impl.hpp"

namespace matinv {

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

}  // namespace matinv
