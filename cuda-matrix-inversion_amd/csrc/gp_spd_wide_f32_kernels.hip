// gp_spd_wide_f32_kernels.hip -- fp32 fused mean / variance on the one-wavefront symmetric sweep of 9 x 9 / 10 x 10 lower tiles
// (128 < n <= 160), run-time n only (tile_impl.hpp).
#ifndef MATINV_MFMA_VGPR_FORM
#error "build with -mllvm -amdgpu-mfma-vgpr-form=1 -DMATINV_MFMA_VGPR_FORM=1 (Makefile)"
#endif
#ifndef MATINV_SPD_WIDE_OCC
#error "build with -DMATINV_SPD_WIDE_OCC=1 (Makefile): one wave per SIMD"
#endif
#include "tile_impl.hpp"

namespace matinv {

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

}  // namespace matinv
