// colour_tile_f32_kernels.hip -- fp32 instantiation of the one-wavefront Cholesky-factor / coloured-sample tile kernels
// (colour_tile_impl.hpp); a translation unit of its own so that the two precisions compile in parallel
#include "colour_tile_impl.hpp"

namespace matinv {

template hipError_t launch_colour_tile<float>(int, int, const float *, size_t, const float *, const float *, float *, float *, size_t, int *,
                                              int, hipStream_t);

}  // namespace matinv
