// ard_predict_tile_f32_kernels.hip -- fp32 instantiation of the one-wavefront tile kernels of GP prediction from coordinates
// (ard_predict_tile_impl.hpp); a translation unit of its own so that the two precisions compile in parallel
#include "ard_predict_tile_impl.hpp"

namespace matinv {

template hipError_t launch_ard_predict_tile<float>(int, int, int, int, const float *, size_t, const float *, size_t, const float *,
                                                   const float *, size_t, float *, float *, size_t, int *, hipStream_t);

}  // namespace matinv
