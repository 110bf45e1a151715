// trend_loo_tile_f32_kernels.hip -- fp32 instantiation of the one-wavefront tile kernels of the leave-one-out cross-validation of a GP
// with a linear trend (trend_loo_tile_impl.hpp); a translation unit of its own so that the two precisions compile in parallel
#include "trend_loo_tile_impl.hpp"

namespace matinv {

template hipError_t launch_trend_loo_tile<float>(int, int, int, const float *, const float *, const float *, const float *, float *, float *,
                                                 float *, size_t, int *, hipStream_t);

}  // namespace matinv
