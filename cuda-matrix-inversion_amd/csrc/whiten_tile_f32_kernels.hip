// whiten_tile_f32_kernels.hip -- fp32 instantiation of the one-wavefront whitening / Mahalanobis / log-density tile kernels
// (whiten_tile_impl.hpp); a translation unit of its own so that the two precisions compile in parallel
#include "whiten_tile_impl.hpp"

namespace matinv {

template hipError_t launch_whiten_tile<float>(int, int, const float *, size_t, const float *, const float *, float *, float *, float *,
                                              float *, size_t, int *, hipStream_t);

}  // namespace matinv
