// tile_f32_kernels.hip -- fp32 symmetric sweeps of the one-wavefront MFMA tile family (tile_impl.hpp) up to 6 x 6 lower tiles: the
// Cholesky entry point (launch_spd_tile<float>); larger sizes go to tile_big_f32_kernels.hip and spd_wide_f32_kernels.hip.
#include "tile_impl.hpp"

namespace matinv {

template <>
hipError_t launch_spd_tile<float>(int n, BatchRef<const float> A, BatchRef<float> X, size_t batch, int *info, hipStream_t stream)
{
    if (!spd_tile_supports<float>(n)) return hipErrorInvalidValue;
    // one wavefront holds the lower triangle up to 7 x 7 tiles at two waves per SIMD, 8 x 8 (144 accumulator registers) since r03,
    // and 9 x 9 / 10 x 10 (180 / 220) at one wave per SIMD with VGPR-form MFMAs and AGPR parking space (spd_wide_f32_kernels.hip)
    if (n > spd_onewave_max(false)) return launch_spd_tile4<float>(n, A, X, batch, info, stream);
    if (batch == 0) return hipSuccess;
    return with_scratch_ints(batch + 1, 1, stream, [&](int *ws) {
        const TileShape s = spd_tile_shape(false, n);
        const unsigned grid = tile_grid(batch, 16u), b = (unsigned)batch;
        hipError_t e = hipSuccess;
        if (s.nt <= 6)
            with_tile<1, 6>(s, [&](auto NT, auto FULL) {
                hipLaunchKernelGGL((matinv_spd_tile_f32<NT, FULL>), dim3(grid), dim3(64), 0, stream, A, X, info, n, b, ws, ws + 1);
            });
        else if (s.nt <= 8)
            e = enqueue_spd_tile_big_f32(n, A, X, grid, b, info, ws, stream);
        else
            e = enqueue_spd_tile_wide_f32(n, A, X, grid, b, info, ws, stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = launch_chol_lds_worklist<float>(n, A, X, ws, ws + 1, info, stream);
        return e;
    });
}

}  // namespace matinv
