// tile_big_f32_kernels.hip -- fp32 one-wavefront symmetric sweeps of 7 x 7 / 8 x 8 lower tiles (Cholesky entry point, 96 < n <= 128)
// and the fused mean / variance on them (tile_impl.hpp); a translation unit of their own so that the fp32 half builds in parallel.
#include "tile_impl.hpp"

namespace matinv {

template hipError_t launch_gp_spd_tile<float>(int, const float *, const float *, const float *, const float *, const float *, float *,
                                              size_t, int *, hipStream_t);

hipError_t enqueue_spd_tile_big_f32(int n, BatchRef<const float> A, BatchRef<float> X, unsigned grid, unsigned b, int *info, int *ws,
                                    hipStream_t stream)
{
    if (n == 112) hipLaunchKernelGGL((matinv_spd_tile_f32<7, true>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1);
    else if (n <= 112) hipLaunchKernelGGL((matinv_spd_tile_f32<7, false>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1);
    // 8 x 8: the run-time-n instantiation also for n = 128 (spd_tile_shape)
    else hipLaunchKernelGGL((matinv_spd_tile_f32<8, false>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1);
    return hipGetLastError();
}

}  // namespace matinv
