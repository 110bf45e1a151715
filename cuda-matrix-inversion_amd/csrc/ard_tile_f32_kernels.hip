// ard_tile_f32_kernels.hip -- fp32 instantiation of the one-wavefront tile kernels of the GP log marginal likelihood from coordinates
// (ard_tile_impl.hpp); a translation unit of its own so that the two precisions compile in parallel
#include "ard_tile_impl.hpp"

namespace matinv {

template hipError_t launch_ard_tile<float>(int, int, int, const float *, size_t, const float *, size_t, const float *, float *, float *,
                                           float *, size_t, int *, hipStream_t);

}  // namespace matinv
